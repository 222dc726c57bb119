"""GPU: the random-camera loss in full (eogs2_amd.randomcam, include/eogs_randomcam.h).

* Parity: every fixture of tests/golden/randomcam (the reference's own `RandomcamRendering_Loss.forward` on the CPU, both render
  types, `use_gt` off and on; tests/golden/make_golden_randomcam.py) goes through `RandomcamRendering_Loss.forward` with the
  renders handed in; each loss and each gradient array is held to the float64 result within 16 x d32 of that array, d32 = the
  reference's own max |float32 - float64| (the factor: four reused kernels in a chain, each summing in its own fixed order,
  and the composed matrix).
* The identity: with cam2virt = I, `virtual_to_sun` returns camera_to_sun bit for bit and the virtual altitude difference is
  V_alt - resample(sun plane, camera_to_sun, uva) bit for bit.
* `cmloss`: three planes with both gradients are `shade.randomcam_l` bit for bit; one plane; a side without gradient; the empty map;
  `_forward` on the map `forward` builds.
* Sharing the sun render: the same loss bits as rendering twice, model gradients within the parity bar; the altitude-only sun
  render gives the full one's sample and gradients.
* A recorded step with drawn virtual cameras and `rawrender_wshadow`: two replays are two eager iterations bit for bit, one recording.
"""
import types

import numpy as np
import pytest
import torch

import randomcam_cases as RC
from util import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().cpu().reshape(-1).view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ---- parity with the reference ------------------------------------------------------------------------------------------
def build_camera(inp, dev):
    """The duck-typed true camera of a fixture and {result name: Parameter}."""
    from eogs2_amd.pan import PanMap

    kind = str(inp["kind"])
    t = lambda k: torch.from_numpy(inp[k]).to(dev)  # noqa: E731
    cam = types.SimpleNamespace(use_cc=False, use_exposure=False, use_shadow=True)
    leaves = {}
    if kind == "exposure":
        cam.use_exposure = True
        cam.exposure = torch.nn.Parameter(t("exposure"))
        leaves["g_exposure"] = cam.exposure
    else:
        n = 1 if kind == "pan_base_first" else 3
        cam.use_cc = True
        cam.color_correction = torch.nn.Conv2d(n, n, 1, bias=True).to(dev)
        with torch.no_grad():
            cam.color_correction.weight.copy_(t("cc_weight"))
            cam.color_correction.bias.copy_(t("cc_bias"))
        leaves.update(g_cc_weight=cam.color_correction.weight, g_cc_bias=cam.color_correction.bias)
    cam.inshadow_color_correction = torch.nn.Parameter(t("inshadow"))
    leaves["g_inshadow"] = cam.inshadow_color_correction
    if kind == "pan_identity":
        cam.msi_to_pan, cam.weird_pan_setup = PanMap("identity"), False
    elif kind == "pan_base_first":
        w, b = torch.nn.Parameter(t("map_weight")), torch.nn.Parameter(t("map_bias"))
        cam.msi_to_pan, cam.weird_pan_setup = PanMap("base", weight=w, bias=b, remove_sigm=False), True
        leaves.update(g_map_weight=w, g_map_bias=b)
    camera_to_sun = t("camera_to_sun")
    cam.get_sun_camera = lambda: (None, camera_to_sun)
    return cam, leaves


def run_variant(inp, render_type, use_gt, dev):
    from eogs2_amd.randomcam import RandomcamRendering_Loss

    t = lambda k: torch.from_numpy(inp[k]).to(dev)  # noqa: E731
    cam, leaves = build_camera(inp, dev)
    V, S = t("virtual_render").requires_grad_(True), t("sun_render").requires_grad_(True)
    A, raw, shaded = t("altitude_render").requires_grad_(True), t("raw_render").requires_grad_(True), t("shaded").requires_grad_(True)
    uva = torch.stack((t("U"), t("V"), A), dim=-1)
    wshadow = render_type == "rawrender_wshadow"
    gt = t("gt_shaded") if wshadow else t("gt_raw")
    fn = RandomcamRendering_Loss(1.0, 1.0, render_type, use_gt=bool(use_gt))
    kw = dict(virtual_render=V, sun_render=S) if wshadow else dict(virtual_render=V)
    L_alt, L_rgb = fn.forward(None, cam, t("cam2virt"), uva, None, None, None, A, raw, gt, shaded, **kw)
    up = t("upstream")
    (up[0] * L_alt + up[1] * L_rgb).backward()
    got = dict(L_alt=L_alt, L_rgb=L_rgb, g_virtual_render=V.grad, g_sun_render=S.grad, g_altitude_render=A.grad, g_raw_render=raw.grad,
               g_shaded=shaded.grad)
    got.update({k: p.grad for k, p in leaves.items()})
    return got


@pytest.mark.parametrize("setup,render_type,use_gt", RC.variants())
def test_parity_with_the_reference(dev, capsys, setup, render_type, use_gt):
    inp = RC.load_inputs(setup)
    want = RC.load_results(setup, render_type, use_gt)
    got = run_variant(inp, render_type, use_gt, dev)
    failures = []
    with capsys.disabled():
        for name, (ref64, d32) in want.items():
            assert got[name] is not None, name
            mine = got[name].detach().cpu().double().numpy().reshape(ref64.shape)
            err = float(np.abs(mine - ref64).max())
            print(f"\n  {setup} {render_type} gt{use_gt} {name}: err {err:.3e} d32 {d32:.3e} ratio {err / d32 if d32 else float(err > 0):.2f}", end="")
            if not err <= RC.RESULT_FACTOR * d32:
                failures.append((name, err, d32))
    # what the reference leaves without a gradient has none here, or zeros
    for name, g in got.items():
        if name not in want and g is not None:
            assert not bool(g.any()), name
    assert not failures, failures


# ---- the identity ---------------------------------------------------------------------------------------------------------
def test_identity_gives_camera_to_sun_and_the_plain_sun_lookup(dev, monkeypatch):
    from eogs2_amd import shade
    from eogs2_amd.randomcam import render_resample_virtual_camera_wshadowmapping, virtual_to_sun
    from eogs2_amd.resample import resample

    inp = RC.load_inputs("identity")
    t = lambda k: torch.from_numpy(inp[k]).to(dev)  # noqa: E731
    I, S = t("cam2virt"), t("camera_to_sun")
    assert torch.equal(I.cpu(), torch.eye(3))
    V2S, K = virtual_to_sun(I, S)
    assert same_bits(V2S, S) and same_bits(K, S)
    out = torch.full((18,), 7.0, device=dev)
    a, b = virtual_to_sun(I, S, out=out)
    assert a.data_ptr() == out.data_ptr() and same_bits(out[:9], S.reshape(-1)) and same_bits(out[9:], S.reshape(-1))
    seen = {}
    inner = shade.render_pipeline

    def spy(cam, raw_render, sun_altitude_diff=None):
        seen["diff"] = sun_altitude_diff.detach().clone()
        return inner(cam, raw_render, sun_altitude_diff)

    monkeypatch.setattr(shade, "render_pipeline", spy)
    cam, _ = build_camera(inp, dev)
    uva = torch.stack((t("U"), t("V"), t("altitude_render")), dim=-1)
    Vr, Sr = t("virtual_render"), t("sun_render")
    render_resample_virtual_camera_wshadowmapping(None, cam, I, uva, None, None, None, virtual_render=Vr, sun_render=Sr)
    plain, _ = resample(Sr[3:4], S, uva, n_out=1, fill_channel=0, fill_value=-100.0)
    assert same_bits(seen["diff"], Vr[3] - plain[0])


def test_compose_on_the_device_is_within_one_ulp_of_float64(dev):
    from eogs2_amd.randomcam import virtual_to_sun

    for name, c, s in RC.compose_cases():
        gV, gK = virtual_to_sun(torch.from_numpy(c).to(dev), torch.from_numpy(s).to(dev))
        V64, K64 = RC.compose_float64(c, s)  # numpy's float64 inv(C) @ S and inv(C) @ S @ C: the bound the host text is held to on the CPU
        assert np.all(np.abs(gV.cpu().numpy().astype(np.float64) - V64) <= RC.ulp32(V64)), name
        assert np.all(np.abs(gK.cpu().numpy().astype(np.float64) - K64) <= RC.ulp32(K64)), name
    for name, c in RC.SINGULAR:
        gV, gK = virtual_to_sun(torch.from_numpy(c).to(dev), torch.from_numpy(RC.shear(0.25, -0.5)).to(dev))
        assert bool(torch.isnan(gV).all()) and bool(torch.isnan(gK).all()), name


def test_forward_underscore_on_the_map_forward_builds(dev):
    """`_forward` over the occlusion map of main_loss.py:151-154 gives `forward`'s losses and gradients bit for bit."""
    from eogs2_amd.randomcam import RandomcamRendering_Loss, cmloss

    fn = RandomcamRendering_Loss(1.0, 1.0, "rawrender")
    for C in (1, 3):
        alt, a, b, uv = _cmloss_inputs(dev, C, 33, 47, 21 + C)
        want = _run_loss(cmloss, alt, a, b, uv)

        def through_forward_(alt_, a_, b_, uv_):
            occ = ((alt_.abs() < 0.30) * (uv_.abs() < 1).all(-1)).detach()
            return fn._forward(occ, alt_, a_ - b_)

        got = _run_loss(through_forward_, alt, a, b, uv)
        for i, (g, w) in enumerate(zip(got, want)):
            assert same_bits(g, w), (C, i)
    alt, a, b, uv = _cmloss_inputs(dev, 3, 8, 8, 4, empty=True)
    L = fn._forward(torch.zeros(8, 8, dtype=torch.bool, device=dev), alt, a - b)
    assert L[0].is_cuda and float(L[0]) == 0.0 and float(L[1]) == 0.0


# ---- cmloss -----------------------------------------------------------------------------------------------------------------
def _cmloss_inputs(dev, C, H, W, seed, empty=False):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.rand((C, H, W), generator=g), torch.rand((C, H, W), generator=g)
    b[:, 1, :5] = a[:, 1, :5]  # exact ties: sign(0) = 0
    alt = 0.2 * torch.randn((H, W), generator=g)
    alt[2, :3] = 0.0
    uv = 1.3 * (2 * torch.rand((H, W, 2), generator=g) - 1)
    if empty:
        uv = uv.abs() + 1.0
    return [x.to(dev) for x in (alt, a, b, uv)]


def _run_loss(fn, alt, a, b, uv, grad_a=True, grad_b=True):
    alt, a, b = alt.clone().requires_grad_(True), a.clone().requires_grad_(grad_a), b.clone().requires_grad_(grad_b)
    L = fn(alt, a, b, uv)
    (0.7 * L[0] - 1.3 * L[1]).backward()
    return L[0].detach(), L[1].detach(), alt.grad, a.grad, b.grad


@pytest.mark.parametrize("H,W", [(19, 37), (33, 47), (600, 500)])  # one workgroup's worth, several, more than the 1024 of a launch
def test_cmloss_three_planes_is_randomcam_l_bit_for_bit(dev, H, W):
    from eogs2_amd.randomcam import cmloss
    from eogs2_amd.shade import randomcam_l

    x = _cmloss_inputs(dev, 3, H, W, 5)
    got, want = _run_loss(cmloss, *x), _run_loss(randomcam_l, *x)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), i
    assert float(got[0]) > 0 and float(got[1]) > 0


def _float64_loss(alt, a, b, uv):
    alt, a, b, uv = (x.detach().cpu().double() for x in (alt, a, b, uv))
    occ = ((alt.abs() < 0.30) * (uv.abs() < 1).all(-1))
    n = occ.sum()
    return (alt.abs() * occ).sum() / n, ((a - b).abs() * occ).sum() / n, occ


@pytest.mark.parametrize("C", [1, 2, 4])
def test_cmloss_other_plane_counts(dev, C):
    from eogs2_amd.randomcam import cmloss

    H, W = 33, 47
    x = _cmloss_inputs(dev, C, H, W, 11 + C)
    L_alt, L_rgb, g_alt, g_a, g_b = _run_loss(cmloss, *x)
    w_alt, w_rgb, occ = _float64_loss(*x)
    # Sums of non-negative fp32 terms: the error is at most (roundings on the longest path) x u x the sum. The path: the difference
    # (1), the planes of a pixel (C - 1), the lane's own pixels (1 at this size), six butterfly levels and three wave sums, twice
    # (workgroup, then the partials), and the division: 22 + C.
    u = 2.0 ** -24
    assert abs(float(L_alt) - float(w_alt)) <= (22 + C) * u * float(w_alt) and abs(float(L_rgb) - float(w_rgb)) <= (22 + C) * u * float(w_rgb)
    n = float(occ.sum())
    alt, a, b, _ = (t.cpu().double() for t in x)
    want_alt = 0.7 / n * occ * torch.sign(alt)
    want_a = -1.3 / n * occ * torch.sign(a - b)
    assert float((g_alt.cpu().double() - want_alt).abs().max()) <= 2 * u * 0.7 / n  # one division, one product
    assert float((g_a.cpu().double() - want_a).abs().max()) <= 2 * u * 1.3 / n
    assert same_bits(g_b, -g_a)
    assert bool((g_a[:, 1, :5] == 0).all())  # the ties


@pytest.mark.parametrize("C", [1, 3])
def test_cmloss_either_side_without_gradient(dev, C):
    from eogs2_amd.randomcam import cmloss

    x = _cmloss_inputs(dev, C, 24, 20, 3)
    both = _run_loss(cmloss, *x)
    only_b = _run_loss(cmloss, *x, grad_a=False)  # use_gt: the ground truth takes no gradient
    only_a = _run_loss(cmloss, *x, grad_b=False)
    neither = _run_loss(cmloss, *x, grad_a=False, grad_b=False)
    assert only_b[3] is None and only_a[4] is None and neither[3] is None and neither[4] is None
    for r in (only_b, only_a, neither):
        assert same_bits(r[0], both[0]) and same_bits(r[1], both[1]) and same_bits(r[2], both[2])
    assert same_bits(only_b[4], both[4]) and same_bits(only_a[3], both[3])


@pytest.mark.parametrize("C", [1, 3])
def test_cmloss_empty_mask(dev, C):
    from eogs2_amd.randomcam import cmloss

    x = _cmloss_inputs(dev, C, 8, 8, 4, empty=True)
    x[1][0, 0, 0] = float("nan")  # outside the mask: not read into the sums
    L_alt, L_rgb, g_alt, g_a, g_b = _run_loss(cmloss, *x)
    assert L_alt.is_cuda and float(L_alt) == 0.0 and float(L_rgb) == 0.0
    zero = torch.zeros(1, dtype=torch.int32)
    for g in (g_alt, g_a, g_b):
        assert bool((bits(g) == zero).all())  # +0 everywhere


# ---- a small scene: sharing the sun render, the recorded step ----------------------------------------------------------------
C0 = 0.28209479177387814


class _Camera:
    def __init__(self, vm, H, W):
        self.FoVx = self.FoVy = 1.0
        self.affine = self.world_view_transform = self.full_proj_transform = vm
        self.image_height, self.image_width = H, W
        self.camera_center = torch.zeros(3, device=vm.device)


class _Scene:
    """64 x 64, about 1 k Gaussians: a view, its sun camera at twice the size, a virtual camera, a colour camera with shadow."""

    NAMES = ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation")

    def __init__(self, dev, P=1000, H=64, W=64):
        from eogs2_amd.synthetic import make_camera, make_scene

        sc = make_scene(P, H, W, seed=0, opacity="trained", device=dev)
        self.dev, self.H, self.W = dev, H, W
        self.model = types.SimpleNamespace(active_sh_degree=0)
        op = sc["opacities"].squeeze(1).clamp(1e-4, 1 - 1e-4)
        for n, v in zip(self.NAMES, (sc["means3D"], ((sc["colors"][:, :3] - 0.5) / C0).reshape(P, 1, 3), torch.log(op / (1 - op)),
                                     torch.log(sc["scales"]), sc["rotations"])):
            setattr(self.model, n, v.clone().contiguous().requires_grad_(True))
        self.cam = _Camera(sc["viewmatrix"], H, W)
        self.sun = _Camera(make_camera(2 * H, 2 * W, seed=5, device=dev), 2 * H, 2 * W)
        self.rnd = _Camera(make_camera(H, W, seed=9, device=dev), H, W)
        self.cam2sun, self.cam2rnd = torch.eye(3, device=dev), torch.eye(3, device=dev)
        self.cam2sun[:2, 2] = (self.sun.affine[2, :2] - self.cam.affine[2, :2]) / 350.0
        self.cam2rnd[:2, 2] = (self.rnd.affine[2, :2] - self.cam.affine[2, :2]) / 350.0
        self.pipe = types.SimpleNamespace(debug=False, antialiasing=False, compute_cov3D_python=False, require_radii=False)
        self.bg = sc["bg"]
        self.U, self.V = torch.meshgrid(torch.linspace(-1, 1, W, device=dev), torch.linspace(-1, 1, H, device=dev), indexing="xy")
        g = torch.Generator().manual_seed(2)
        c = types.SimpleNamespace(use_cc=True, use_exposure=False, use_shadow=True)
        c.color_correction = torch.nn.Conv2d(3, 3, 1, bias=True).to(dev)
        with torch.no_grad():
            c.color_correction.weight.copy_((torch.eye(3) + 0.15 * torch.randn(3, 3, generator=g)).reshape(3, 3, 1, 1))
            c.color_correction.bias.zero_()
        c.inshadow_color_correction = torch.nn.Parameter(torch.full((3, 1, 1), 0.05, device=dev))
        c.get_sun_camera = lambda: (self.sun, self.cam2sun)
        self.true_cam = c
        self.camera_parameters = [*c.color_correction.parameters(), c.inshadow_color_correction]
        self.gt = torch.rand((3, H, W), generator=g).to(dev)

    def parameters(self):
        return [getattr(self.model, n) for n in self.NAMES] + self.camera_parameters

    def iteration(self, share, altitude_only=False, use_gt=False):
        """train_pan.py:279-330,375-391 in small: the view, the sun lookup, the render pipeline, the random-camera loss."""
        from eogs2_amd.randomcam import RandomcamRendering_Loss
        from eogs2_amd.render import render
        from eogs2_amd.resample import resample
        from eogs2_amd.shade import render_pipeline

        for p in self.parameters():
            p.grad = None
        m = self.model
        out = render(self.cam, m, self.pipe, self.bg)["render"]
        img, altitude = out[:3], out[3]
        uva = torch.stack((self.U, self.V, altitude / 350.0), dim=-1)
        sun_img = render(self.sun, m, self.pipe, self.bg, altitude_only=altitude_only)["render"]
        plane = sun_img if altitude_only else sun_img[3:4]
        smp, _ = resample(plane, self.cam2sun, uva, n_out=1, fill_channel=0)
        shaded = render_pipeline(self.true_cam, img, altitude - smp[0])["shaded"]
        fn = RandomcamRendering_Loss(1.0, 1.0, "rawrender_wshadow", use_gt=use_gt)
        L_alt, L_rgb = fn.forward(self.rnd, self.true_cam, self.cam2rnd, uva, m, self.pipe, self.bg, altitude, img, self.gt, shaded,
                                  sun_render=sun_img if share else None)
        ((shaded - self.gt).abs().mean() + 1e-2 * L_alt + L_rgb).backward()
        return (L_alt.detach(), L_rgb.detach()) + tuple(p.grad for p in self.parameters())


@pytest.fixture(scope="module")
def scene(dev):
    return _Scene(dev)


def test_shared_sun_render_is_the_second_render(dev, scene, capsys):
    twice = [t.clone() for t in scene.iteration(share=False)]
    shared = [t.clone() for t in scene.iteration(share=True)]
    assert float(twice[0]) > 0 and float(twice[1]) > 0 and np.isfinite(float(twice[0])) and np.isfinite(float(twice[1]))
    assert same_bits(shared[0], twice[0]) and same_bits(shared[1], twice[1])  # the same image, the same bits
    with capsys.disabled():
        for i, (a, b) in enumerate(zip(shared[2:], twice[2:])):  # two backward passes summed by autograd against one over the sum
            mx = assert_close(a, b, f"gradient {i}", allow_flips=False)
            print(f"\n  shared against twice, gradient {i}: {mx:.3e}", end="")


def test_altitude_only_sun_render_gives_the_full_ones(dev, scene, capsys):
    full = [t.clone() for t in scene.iteration(share=True)]
    alt = [t.clone() for t in scene.iteration(share=True, altitude_only=True)]
    with capsys.disabled():
        for i, (a, b) in enumerate(zip(alt, full)):  # (the altitude-only render is another kernel instance: the parity bar)
            mx = assert_close(a.reshape(-1) if a.ndim == 0 else a, b.reshape(-1) if b.ndim == 0 else b, f"result {i}", allow_flips=False)
            print(f"\n  altitude-only against full, result {i}: {mx:.3e}", end="")


def test_recorded_step_with_drawn_cameras_replays_the_eager_iterations(dev):
    from eogs2_amd.draw import DrawStream, IterationDraws
    from eogs2_amd.graph import GraphedStep
    from eogs2_amd.render import render

    sc = _Scene(dev)
    extent = 0.02
    view_affine = sc.cam.affine.clone()
    stream = DrawStream(12345, device=dev)
    draws = IterationDraws(stream)
    shear = torch.zeros(2, device=dev)
    draws.add_camera(view_affine, torch.zeros(3, device=dev), virt_affine=sc.rnd.affine, cam2virt=sc.cam2rnd, shear=shear, extent=extent,
                     cam2virt_scale=350.0)
    with torch.no_grad():  # the list workspaces of the recording are sized for the shear's whole range (examples/train_synthetic.py)
        for d0, d1 in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
            corner = view_affine.clone()
            corner[:3, 0] += d0 * extent * view_affine[:3, 2]
            corner[:3, 1] += d1 * extent * view_affine[:3, 2]
            sc.rnd.affine.copy_(corner)
            render(sc.rnd, sc.model, sc.pipe, sc.bg)

    def step():
        draws.draw()  # this iteration's virtual camera and cam2virt; the compose launch inside the loss follows it
        res = sc.iteration(share=True)
        stream.advance()
        return res + (shear.clone(),)

    stream.seek(0)
    eager = [[t.clone() for t in step()] for _ in range(2)]
    assert not same_bits(eager[0][-1], eager[1][-1])  # another camera in the second iteration
    assert not same_bits(eager[0][1], eager[1][1])
    stream.seek(0)
    g = GraphedStep(step, warmup=1)
    stream.seek(0)  # (the warm-up run was an iteration of its own)
    for k in range(2):
        got = [t.clone() for t in g()]
        for i, (a, b) in enumerate(zip(got, eager[k])):
            assert same_bits(a, b), (k, i)
    assert g.replays == 2 and g.recaptures == 0  # one recording
    assert stream.position() == 2
