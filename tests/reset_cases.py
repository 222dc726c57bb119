"""Inputs and references of the reset tests (eogs2_amd.reset, include/eogs_reset.h).

The references are the reference's own lines restated with torch ops and run on the CPU, in fp32 and in float64:
densification_pruning/color_reset_op.py:42-88 (erosion, grid_sample, `< 0.5`, OR; the three assignments and the masked fills
of the moments) and scene/gaussian_model.py:347-352 (reset_opacity). Two statements of eogs_reset.h that the reference's
lines do not make are applied on top: a non-finite projected coordinate flags nothing in that view, and a retired row is
never flagged.

Margin: the fp32 and the float64 flags may differ only on rows whose float64 sample lies within
`m = (max(H, W) + 1) * 2**-20` of 0.5 in some view: a few fp32 ulps of a pixel coordinate times the map's slope of at most 1
per pixel (the reference's matmul fixes no summation order, so the projection's last bits are not defined). Such rows are
left out of a comparison; they may be at most 0.1 % of a case, i.e. none with fewer than 1000 rows.
"""
import types

import torch
import torch.nn.functional as F

C0 = 0.28209479177387814
RETIRED_LOGIT = -1.0e30
BORDERLINE_SHARE = 1e-3
FLAG_SEED = 9800  # (the borderline share of every case was confirmed for this seed: tests/test_reset_api.py)

ERODE_SHAPES = [(1, 1), (1, 9), (5, 7), (33, 65), (37, 53)]
FLAG_P = [1, 63, 64, 65, 257, 4099]
FLAG_VIEWS = {1: [(19, 23)], 3: [(19, 23), (1, 1), (40, 70)],
              17: [(19, 23), (1, 1), (40, 70), (33, 65), (8, 1), (1, 12)] * 2 + [(24, 32), (5, 7), (64, 64), (37, 53), (16, 9)]}


def margin(H, W):
    return (max(H, W) + 1) * 2.0 ** -20


# ---- erosion ----
def erode_input(H, W, seed=0):
    """A shadow map with values inside and outside [0, 1], exact 0 and 1 plateaus and (when it has room) one NaN pixel."""
    g = torch.Generator().manual_seed(4000 + 131 * H + W + seed)
    s = torch.rand(H, W, generator=g) * 1.4 - 0.2
    s[torch.rand(H, W, generator=g) < 0.15] = 1.0
    s[torch.rand(H, W, generator=g) < 0.10] = 0.0
    if H * W >= 9:
        s[H // 2, (2 * W) // 3] = float("nan")
    return s.contiguous()


def erode_ref(s):
    """color_reset_op.py:48-53"""
    return (1 - torch.max_pool2d(1 - s[None, None], 5, stride=1, padding=2))[0, 0]


def same_bits(a, b):
    """Bit equality of two fp32 tensors; a NaN equals a NaN (IEEE 754 leaves a NaN's payload and sign to the implementation)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = torch.isnan(a)
    if not torch.equal(nan, torch.isnan(b)):
        return False
    return torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan])


# ---- flags ----
def shadow_map(H, W, g, binary):
    """A mostly lit shadow map with dark spots (the erosion widens them by two pixels): smooth with a slope well under 1 per
    pixel, or binary. A map narrower than 8 pixels is lit everywhere: what it flags is what projects outside it (a dark one
    would settle every row of its case)."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    a, b, c, d = (torch.rand(4, generator=g) * 0.5 + 0.1).tolist()
    wave = torch.sin(a * x + 3.0 * b) * torch.cos(c * y + 3.0 * d)
    if min(H, W) < 8:
        return (0.75 + 0.1 * wave).contiguous()
    s = (1.35 + 1.0 * wave).clamp(0.0, 1.0)  # (crosses 0.5 where the wave is steep: few samples land near the threshold)
    if binary:
        s = (s > 0.5).to(torch.float32)
    return s.contiguous()


def flags_case(P, n_views):
    """xyz f32[P,3], opacity logits f32[P], views [(shadowmap, affine)]. View 0's matrix is the identity on (x, y), so the
    leading rows hit chosen coordinates of that view exactly: a retired row that would be flagged, a NaN row, the corners
    and the centre, just outside +-1, far outside, pixel centres. The other rows are uniform in [-1.1, 1.1]^3 (about a
    sixth projects outside view 0); the other views' matrices mix all three coordinates and keep most rows inside, so that a
    row's verdict is not settled by the zeros padding alone."""
    g = torch.Generator().manual_seed(FLAG_SEED + 17 * P + n_views)
    sizes = FLAG_VIEWS[n_views]
    views = []
    for k, (H, W) in enumerate(sizes):
        A = torch.zeros(4, 4)
        A[3, 3] = 1.0
        if k == 0:
            A[0, 0] = A[1, 1] = A[2, 2] = 1.0
        else:
            A[:3, :3] = torch.eye(3) * (0.5 + 0.2 * torch.rand(1, generator=g)) + 0.08 * torch.randn(3, 3, generator=g)
            A[3, :3] = 0.05 * torch.randn(3, generator=g)
        views.append((shadow_map(H, W, g, binary=k % 2 == 1), A.contiguous()))
    H0, W0 = sizes[0]
    special = [(5.0e5, -3.0e4), (float("nan"), 0.25), (1.0, 1.0), (-1.0, -1.0), (0.0, 0.0), (1.0, -1.0), (-1.0, 1.0),
               (1.0 + 2.0 ** -23, 0.0), (0.0, -1.0 - 2.0 ** -23), (1.0 + 1e-6, 1.0 + 1e-6), (-1.0 - 1e-3, 0.5), (1.0e6, 1.0e6),
               (-7.0e9, 0.0), (float("inf"), 0.0)]
    # (1 + 2^-23 is the fp32 neighbour of 1)
    special += [(2.0 * j / (W0 - 1) - 1.0, 2.0 * i / (H0 - 1) - 1.0) for i, j in ((0, 0), (3, 5), (H0 - 1, W0 - 1), (7, 22), (18, 1))]
    xyz = torch.rand(P, 3, generator=g) * 2.2 - 1.1
    n = min(P, len(special))
    xyz[:n, :2] = torch.tensor(special[:n], dtype=torch.float32)
    opacity = torch.randn(P, generator=g) * 3.0
    opacity[0] = RETIRED_LOGIT  # row 0 projects far outside view 0: flagged by the zeros padding, were it not retired
    if P > 40:
        opacity[33] = RETIRED_LOGIT
        opacity[34] = float("nan")  # (a NaN logit is not a retired row)
    return xyz.contiguous(), opacity.contiguous(), views


def view_samples(xyz, shadow, affine, dtype):
    """color_reset_op.py:46-61 and affine_cameras.py:432-438 in `dtype`: the sample per Gaussian and whether its projection
    is finite."""
    xyz, shadow, affine = xyz.to(dtype), shadow.to(dtype), affine.to(dtype)
    pts = xyz @ affine[:3, :2] + affine[3, :2]
    e = erode_ref(shadow)
    finite = torch.isfinite(pts).all(dim=1)
    safe = torch.where(finite[:, None], pts, torch.zeros_like(pts))  # (grid_sample is undefined on non-finite coordinates)
    smp = F.grid_sample(e[None, None], safe[None, None], mode="bilinear", align_corners=True, padding_mode="zeros")[0, 0, 0]
    return smp, finite


def flags_ref(xyz, views, opacity=None, dtype=torch.float32):
    """(flags bool[P], borderline bool[P]): the reference's verdict in `dtype`, and the rows whose sample lies within the
    margin of 0.5 in some view."""
    P = xyz.shape[0]
    flags = torch.zeros(P, dtype=torch.bool)
    borderline = torch.zeros(P, dtype=torch.bool)
    for shadow, affine in views:
        smp, finite = view_samples(xyz, shadow, affine, dtype)
        flags |= (smp < 0.5) & finite
        borderline |= ((smp.double() - 0.5).abs() <= margin(*shadow.shape)) & finite
    if opacity is not None:
        flags &= ~(opacity < 0.5 * RETIRED_LOGIT)
    return flags, borderline


def check_flags(got, xyz, views, opacity=None):
    """Asserts the library's flags against both references: equal to the fp32 one on every row outside the float64 margin,
    the rows inside it under the cap."""
    f32, _ = flags_ref(xyz, views, opacity, torch.float32)
    f64, borderline = flags_ref(xyz, views, opacity, torch.float64)
    P = xyz.shape[0]
    n_border = int(borderline.sum())
    print(f"P {P} views {len(views)}: flagged {int(f32.sum())}, borderline {n_border}, fp32 vs float64 differ on {int((f32 != f64).sum())}")
    assert n_border <= BORDERLINE_SHARE * P, (n_border, P)
    got = got.detach().cpu().to(torch.bool)
    bad = (got != f32) & ~borderline
    assert not bool(bad.any()), f"{int(bad.sum())} rows differ from the fp32 reference, first {bad.nonzero()[:5].flatten().tolist()}"
    return borderline


# ---- the fills ----
GROUPS = (("xyz", (3,)), ("f_dc", (1, 3)), ("f_rest", (0, 3)), ("opacity", (1,)), ("scaling", (3,)), ("rotation", (4,)))


def make_optimizer(P, device, seed=0, with_state=True, cls=None):
    """A model's six one-tensor parameter groups (gaussian_model.py:228-262) with random parameters, moments and step counts."""
    g = torch.Generator().manual_seed(500 + seed)
    groups = []
    for name, tail in GROUPS:
        p = torch.nn.Parameter(torch.randn((P,) + tail, generator=g).to(device))
        groups.append(dict(params=[p], lr=1e-3, name=name))
    opt = (cls or torch.optim.Adam)(groups, lr=0.0, eps=1e-15)
    if with_state:
        for k, group in enumerate(opt.param_groups):
            p = group["params"][0]
            opt.state[p] = {"step": torch.tensor(float(7 + k)), "exp_avg": torch.randn(p.shape, generator=g).to(device),
                            "exp_avg_sq": torch.rand(p.shape, generator=g).to(device)}
    return opt


def snapshot(opt):
    """{name: (param, exp_avg, exp_avg_sq, step)} as CPU clones (None where there is no state)."""
    out = {}
    for group in opt.param_groups:
        p = group["params"][0]
        st = opt.state.get(p) or {}
        c = lambda t: None if t is None else t.detach().cpu().clone()  # noqa: E731
        out[group["name"]] = (c(p), c(st.get("exp_avg")), c(st.get("exp_avg_sq")), c(st.get("step")))
    return out


def identities(opt):
    """What must survive an in-place reset: the Parameter objects, the moment tensors and their addresses."""
    out = []
    for group in opt.param_groups:
        p = group["params"][0]
        st = opt.state.get(p) or {}
        out.append((id(p), p.data_ptr(), id(st.get("exp_avg")), id(st.get("exp_avg_sq")),
                    None if st.get("exp_avg") is None else (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())))
    return out


def color_reset_ref(snap, to_reset):
    """color_reset_op.py:66-88 on a snapshot (CPU fp32): the expected snapshot."""
    to_reset = to_reset.to(torch.bool).cpu()
    out = {k: tuple(None if t is None else t.clone() for t in v) for k, v in snap.items()}
    opacity, f_dc, scaling = out["opacity"][0], out["f_dc"][0], out["scaling"][0]
    inverse_sigmoid = lambda x: torch.log(x / (1 - x))  # noqa: E731
    opacity[to_reset] = inverse_sigmoid(0.005 * torch.ones_like(opacity[to_reset]))
    f_dc[to_reset] = (torch.full_like(f_dc[to_reset], 1.1) - 0.5) / C0  # RGB2SH
    scaling[to_reset] = torch.log((1.0 / 400) * torch.ones_like(scaling[to_reset]))
    for name in ("opacity", "f_dc", "scaling"):
        param, m1, m2, _ = out[name]
        if m1 is None:
            continue
        mask = to_reset.squeeze().clone()
        while len(mask.shape) < len(param.shape):
            mask = mask.unsqueeze(-1)
        m1.masked_fill_(mask, 0.0)
        m2.masked_fill_(mask, 0.0)
    return out


def assert_snapshots_equal(got, want, skip_rows=None):
    """Bit equality of two snapshots; `skip_rows` (bool[P]) leaves rows out (the borderline rows of a flags comparison)."""
    for name in want:
        for what, a, b in zip(("param", "exp_avg", "exp_avg_sq", "step"), got[name], want[name]):
            assert (a is None) == (b is None), (name, what)
            if a is None:
                continue
            if skip_rows is not None and what != "step":
                a, b = a[~skip_rows], b[~skip_rows]
            assert same_bits(a, b), f"{name}.{what} differs"


# ---- reset_opacity ----
def opacity_logits(P, seed=0):
    g = torch.Generator().manual_seed(800 + seed)
    l = torch.rand(P, 1, generator=g) * 60.0 - 30.0
    cap = reset_opacity_constant()
    special = torch.cat([torch.tensor([30.0, -30.0]), cap, torch.nextafter(cap, torch.zeros(1)), torch.nextafter(cap, -torch.ones(1) * 9.0),
                         torch.tensor([0.0, -4.0])])  # the extremes, the cap itself, its fp32 neighbours above and below
    n = min(P, special.numel())
    l[:n, 0] = special[:n]
    if P > 20:
        l[11, 0] = float("nan")
        l[13, 0] = RETIRED_LOGIT
    return l.contiguous()


def reset_opacity_ref64(logit):
    """gaussian_model.py:347-352 in float64 (the cap is the fp32 0.01 the reference's `ones_like(...) * 0.01` holds)."""
    o = torch.sigmoid(logit.double())
    o = torch.min(o, torch.ones_like(o) * float(torch.ones(1) * 0.01))
    return torch.log(o / (1 - o))


def reset_opacity_constant():
    """What the reference stores at and above the cap: inverse_sigmoid of the fp32 0.01, in fp32."""
    x = torch.ones(1) * 0.01
    return torch.log(x / (1 - x))


def ulp_distance(a32, b64):
    """|a - b| in units of the fp32 spacing at b (float64 tensor)."""
    b32 = b64.float()
    spacing = (torch.nextafter(b32.abs(), torch.full_like(b32, float("inf"))) - b32.abs()).double()
    return (a32.double() - b64).abs() / spacing


# ---- render_all_views / color_reset end to end ----
def make_cameras(device, sizes=((24, 32), (20, 28))):
    """Duck-typed training cameras with what renderer.py, renderer_cc_shadow.py and AffineCamera.render_pipeline read. The
    world-to-view matrix is NOT the affine matrix (its last row is shifted), the lower altitude bound is no value the
    background starts with, and each camera has a sun camera of its own at twice the size."""
    from eogs2_amd.shade import render_pipeline
    from eogs2_amd.synthetic import ALT_SCALE, make_camera

    def bare(H, W, seed):
        c = types.SimpleNamespace(FoVx=1.0, FoVy=1.0, learn_wv_only_lastparam=False, image_height=H, image_width=W,
                                  camera_center=torch.zeros(3, device=device), image_name=f"view_{seed}")
        c.affine = make_camera(H, W, seed=seed, device=device)
        c.world_view_transform = c.full_proj_transform = c.affine
        return c

    cams = []
    g = torch.Generator().manual_seed(3)
    for k, (H, W) in enumerate(sizes):
        c = bare(H, W, 20 + k)
        wvt = c.affine.clone()
        wvt[3, :2] += torch.tensor([0.03, -0.02], device=device)
        c.world_view_transform = c.full_proj_transform = wvt
        c.altitude_bounds = torch.tensor([-11.0 - k, 40.0], device=device)
        c.UV_grid = torch.meshgrid(torch.linspace(-1, 1, W, device=device), torch.linspace(-1, 1, H, device=device), indexing="xy")
        sun = bare(2 * H, 2 * W, 40 + k)
        cam2sun = torch.eye(3, device=device)
        cam2sun[:2, 2] = (sun.affine[2, :2] - c.affine[2, :2]) / ALT_SCALE
        c.get_sun_camera = lambda sun=sun, cam2sun=cam2sun: (sun, cam2sun)
        c.use_cc, c.use_exposure, c.use_shadow = True, False, True
        c.color_correction = torch.nn.Conv2d(3, 3, 1, bias=True).to(device)
        with torch.no_grad():
            c.color_correction.weight.copy_((torch.eye(3) + 0.1 * torch.randn(3, 3, generator=g)).reshape(3, 3, 1, 1))
            c.color_correction.bias.zero_()
        c.inshadow_color_correction = torch.full((3, 1, 1), 0.05, device=device)
        c.render_pipeline = lambda raw_render, sun_altitude_diff=None, c=c: render_pipeline(c, raw_render, sun_altitude_diff)
        cams.append(c)
    return cams


class Model:
    """The attributes render() and color_reset read from a GaussianModel, over an optimizer's groups."""
    active_sh_degree = 0

    def __init__(self, optimizer):
        self.optimizer = optimizer
        by = {g["name"]: g["params"][0] for g in optimizer.param_groups}
        self._xyz, self._features_dc, self._opacity = by["xyz"], by["f_dc"], by["opacity"]
        self._scaling, self._rotation = by["scaling"], by["rotation"]

    get_xyz = property(lambda s: s._xyz)


def make_model(P, device, seed=0):
    """A volume scene's Gaussians as raw parameters in an optimizer with state (make_optimizer's moments and steps)."""
    from eogs2_amd.synthetic import make_scene

    sc = make_scene(P, 24, 32, seed=seed, opacity="trained", device=device)
    opt = make_optimizer(P, device, seed=seed)
    by = {g["name"]: g["params"][0] for g in opt.param_groups}
    op = sc["opacities"].reshape(P, 1).clamp(1e-4, 1 - 1e-4)
    with torch.no_grad():
        by["xyz"].copy_(sc["means3D"])
        by["f_dc"].copy_(((sc["colors"][:, :3] - 0.5) / C0).reshape(P, 1, 3))
        by["opacity"].copy_(torch.log(op / (1 - op)))
        by["scaling"].copy_(torch.log(sc["scales"]))  # (gaps between the splats: the sun view sees ground where the view sees a splat)
        by["rotation"].copy_(sc["rotations"])
    return Model(opt)
