"""Edge cases of the bucketed-gather backward (eogs2_amd/csrc/bucket_gather.h) shared by tests/test_resample_cases.py (CPU:
the cases themselves are checked) and the GPU tests of the virtual-camera resample (tests/test_gpu_resample.py) and of the
flow warp (tests/test_gpu_flow.py): seeded inputs, the reference's fp32 op sequences, the comparison rule, and the host
geometry the tests need. No float64 reference lives here: that is oracle/resample_oracle.py for the resample and
flow_cases.warp / flow_cases.warp_adjoint for the flow.

A case is a dict of tensors plus `guards`, the kernel lines it exists for. A resample case has `vr` (C, Hv, Wv), `U`, `V`,
`alt` (H, W), `M` (cam2virt), upstream gradients `w_s` (n_out, H, W) and `w_uv` (H, W, 2), `n_out`, `fill_channel` and
`lattice`; a flow case has `img`, `up` (C, H, W) and `flow` (1, 2, H, W).

THE COMPARISON RULE (compare_resample, compare_flow)

* Tolerance TOL = 1e-4 of the maximum of the quantity: the channel of `sample` (and of the warped image), the whole of `uv`,
  the column of dL/duva, and the whole of dL/dvirtual (of dL/dimg). The gradient of the sampled image is measured against
  the tensor's maximum because its elements are sums of up to thousands of signed terms that share one unit, and a channel
  may consist of a single cancelled sum: in `collapse_exact` channel 3 is one sum of 4096 terms that comes to -0.028 where
  the terms' magnitudes add up to 823, so 1e-4 of that channel's own maximum is below what any fp32 order of the sum
  keeps (the plain sequential fp32 sum is 3e-4 off). Channels that must be zero are asserted to be zero exactly by the
  tests. The reference's own fp32 ops on the CPU must stay within REF_TOL = 3e-5 of the float64 oracle under the same
  rule, so the bar is held by the reference alone.
* Lattice cases (`lattice=True`, and every flow case): coordinates are built so that fp32 and float64 agree exactly on cell
  and weight — Wv - 1 and Hv - 1 powers of two, u and v multiples of 2^-13 with dyadic cam2virt entries, flows multiples of
  1/8 (and H - 1, W - 1 powers of two where the reference's normalisation round trip would otherwise round). No element is
  left out.
* Seeded cases: only dL/duva may leave pixels out, and only where the float64 pixel coordinate ix or iy lies within NEAR =
  1e-3 of an integer along an axis with more than one cell: the sample is continuous there, its derivative is not, and two
  correct fp32 evaluations pick different cells. At most MAX_LEFT_OUT = 1 % of a case's pixels.
"""
import functools

import numpy as np
import torch

# restated from eogs2_amd/csrc/bucket_gather.h (OT, CHT, RB) and the launchers' tile choice in resample.hip / flow.hip
OT = 16                      # output tile edge: 256 pixels, one workgroup
BIG_CELLS = 1_500_000        # more virtual cells than this: 64 x 32 virtual tiles instead of 32 x 32
CHT = {1: 8, 4: 4}           # candidate output tiles per chunk, by planes held in registers (NACC)
RB = {1: 4096, 4: 1024}      # boxes per scan round
CAP = {k: v * OT * OT for k, v in CHT.items()}  # entries a chunk can park

TOL = 1e-4
REF_TOL = 3e-5
NEAR = 1e-3
MAX_LEFT_OUT = 0.01


def nacc(n_planes):
    return 1 if n_planes == 1 else 4


def virtual_tile(Hv, Wv):
    return (64, 32) if Hv * Wv > BIG_CELLS else (32, 32)


# ---- resample cases -------------------------------------------------------------------------------------------------
def _M(sx, sy, ax=0.0, ay=0.0):
    return torch.tensor([[sx, 0.0, ax], [0.0, sy, ay], [0.0, 0.0, 1.0]], dtype=torch.float32)


def _resample(guards, H, W, Hv, Wv, M, seed, C=5, n_out=4, fill_channel=3, lattice=False, U=None, V=None, alt=None):
    g = torch.Generator().manual_seed(seed)
    vr = torch.rand(C, Hv, Wv, generator=g)
    if C > 3:
        vr[3] = vr[3] * 40 - 10  # altitude-like channel
    a = torch.rand(H, W, generator=g) * 2 - 0.5
    gu, gv = torch.meshgrid(torch.linspace(-1, 1, W), torch.linspace(-1, 1, H), indexing="xy")
    w_s = torch.randn(n_out, H, W, generator=g)
    w_uv = torch.randn(H, W, 2, generator=g)
    if callable(alt):
        a = alt(a)
    if callable(U):
        gu, gv = U(gu, g), V(gv, g)
    return dict(guards=guards, vr=vr, U=gu.contiguous(), V=gv.contiguous(), alt=a, M=M, w_s=w_s, w_uv=w_uv, n_out=n_out,
                fill_channel=fill_channel, lattice=lattice)


def _dyadic(bits):
    return lambda t, g=None: torch.round(t * 2.0 ** bits) / 2.0 ** bits


def _big(n_out):
    C, fill = (5, 3) if n_out == 4 else (1, 0)
    return lambda: _resample(
        f"the 64x32-tile instantiation of ResampleSrc with {n_out} plane(s); magnification: most cells receive nothing and must be 0",
        96, 112, 1025, 2049, _M(1.0, 1.0, 2.0 ** -6, -(2.0 ** -7)), 11, C=C, n_out=n_out, fill_channel=fill, lattice=True,
        U=_dyadic(13), V=_dyadic(13), alt=_dyadic(6))


def _far(U, g):
    U = U.clone()
    U[:, U.shape[1] // 2] = 0.0
    return U


def _far_v(V, g):
    V = V.clone()
    V[V.shape[0] // 2, :] = 0.0
    return V


_RESAMPLE = {
    "collapse_exact": lambda: _resample(
        "a bucket of CAP entries in every chunk (cnt == CAP, s_start + cnt == CAP); the rank loop over CAP ids; half-cell weights",
        64, 64, 40, 40, _M(0.0, 0.0), 1, lattice=True),
    "collapse_alt": lambda: _resample("a few buckets holding all 4096 pixels; dL_duva[..., 2] non-trivial", 64, 64, 40, 40,
                                      _M(0.0, 0.0, 0.03, 0.02), 2),
    "minify8": lambda: _resample("tens of pixels per cell; a virtual tile partly outside the image", 128, 160, 17, 33,
                                 _M(1.0, 1.0, 0.05, -0.03), 3),
    "rounds4": lambda: _resample("1056 output tiles: two scan rounds of RB = 1024, every tile a candidate", 528, 512, 40, 40,
                                 _M(0.9, 0.9, 0.02, -0.015), 4),
    "rounds1": lambda: _resample("4160 output tiles: two scan rounds of RB = 4096; uint16 list offsets up to 4095", 1040, 1024, 40, 40,
                                 _M(0.9, 0.9, 0.02, -0.015), 5, C=1, n_out=1, fill_channel=0),
    "big4": _big(4),
    "big1": _big(1),
    "partly_out": lambda: _resample("x0 = -1 / y0 = -1 buckets; the fill channel; `outside` zeroing g", 48, 48, 33, 65,
                                    _M(1.5, 1.5, 0.3, 0.3), 6),
    "all_out": lambda: _resample("empty boxes everywhere: dL_dvirtual == 0 must still be written; sample channel 3 == -100, rgb == 0",
                                 40, 56, 40, 40, _M(1.0, 1.0), 7,
                                 U=lambda U, g: 1.5 + 1.5 * torch.rand(U.shape, generator=g).clamp(1e-3, 1 - 1e-3),
                                 V=lambda V, g: 1.5 + 1.5 * torch.rand(V.shape, generator=g).clamp(1e-3, 1 - 1e-3)),
    "far": lambda: _resample("the float clamp before the int conversion in make_taps; no cell touched outside the centre row and column",
                             40, 40, 40, 40, _M(1e6, -1e6), 8, U=_far, V=_far_v),
    "far_e12": lambda: _resample("as `far` with pixel coordinates beyond the int range (2e13): without the clamp the conversion is undefined",
                                 40, 40, 40, 40, _M(1e12, -1e12), 8, U=_far, V=_far_v),
    "edge_pm1": lambda: _resample("lattice weights 0; x0 = Wv - 1 with no east cell; `outside` false at exactly +-1", 33, 65, 33, 65,
                                  _M(1.0, 1.0), 9, lattice=True),
    "half_cell": lambda: _resample("dyadic fractional weights: a swapped east / west weight shows cleanly", 33, 65, 33, 65,
                                   _M(1.0, 1.0, 2.0 ** -6, 2.0 ** -5), 10, lattice=True, alt=_dyadic(6)),
    "thin_w": lambda: _resample("Wv - 1 = 0: one column, the coordinate gradient along x is exactly 0", 48, 48, 40, 1, _M(1.0, 1.0, 0.02, -0.015), 12),
    "thin_h": lambda: _resample("Hv - 1 = 0: one row, the coordinate gradient along y is exactly 0", 48, 48, 1, 40, _M(1.0, 1.0, 0.02, -0.015), 13),
    "one_tile": lambda: _resample("a virtual image of exactly one tile: tile edge against image edge", 48, 48, 32, 32,
                                  _M(0.95, 0.95, 0.02, -0.015), 14),
    "one_past": lambda: _resample("a virtual image one cell past a tile: a second tile row and column of one cell", 48, 48, 33, 33,
                                  _M(0.95, 0.95, 0.02, -0.015), 15),
}
BASE_RESAMPLE = tuple(_RESAMPLE)

# (C, n_out, fill_channel) on `minify8` and `partly_out`: the `ch < n_out` masks of the four-plane kernel, no fill channel or
# the first one, several trailing channels that must receive zeros, and n_out = 5: the global-atomic fallback
CHANNEL_MATRIX = ((5, 2, 1), (5, 3, -1), (5, 4, 0), (5, 4, -1), (4, 4, 3), (5, 5, 3), (6, 5, -1), (3, 1, 0))


def channel_name(base, C, n_out, fill):
    return f"{base}-c{C}-n{n_out}-f{'none' if fill < 0 else fill}"


def _channel_case(base, C, n_out, fill):
    def build():
        b = _RESAMPLE[base]()
        H, W = b["alt"].shape
        c = _resample(f"(C, n_out, fill_channel) = ({C}, {n_out}, {fill}) on {base}: " + b["guards"], H, W, *b["vr"].shape[1:], b["M"],
                      100 + 10 * C + n_out, C=C, n_out=n_out, fill_channel=fill)
        return c
    return build


for _base_name in ("minify8", "partly_out"):
    for _cnf in CHANNEL_MATRIX:
        _RESAMPLE[channel_name(_base_name, *_cnf)] = _channel_case(_base_name, *_cnf)
CHANNEL_RESAMPLE = tuple(n for n in _RESAMPLE if n not in BASE_RESAMPLE)
RESAMPLE = BASE_RESAMPLE + CHANNEL_RESAMPLE


@functools.lru_cache(maxsize=None)
def resample_case(name):
    """The case `name`; shared, so nobody writes into its tensors."""
    return _RESAMPLE[name]()


def reference_resample_ops(vr, M, uva, n_out=4, fill_channel=3):
    """renderer_cc_shadow.py:32-50 as the reference runs it (torch ops in the tensors' precision, autograd), with the channel
    count and the filled channel as parameters."""
    uv = torch.einsum("...ij,...j->...i", M, uva)[..., :2]
    s = torch.nn.functional.grid_sample(vr.unsqueeze(0), uv.unsqueeze(0), align_corners=True).squeeze(0)[:n_out]
    if fill_channel >= 0:
        outside = (uv.abs() > 1).any(-1)
        s = torch.cat([torch.where(outside, torch.full_like(c, -100.0), c)[None] if k == fill_channel else c[None]
                       for k, c in enumerate(s)], 0)
    return s, uv


def run_resample(fn, case, dev):
    """`fn(vr, M, uva, n_out, fill_channel) -> (sample, uv)` forward and backward on `dev`; CPU tensors back."""
    vr = case["vr"].to(dev).clone().requires_grad_(True)  # (a copy: the case's own tensors stay as they are)
    uva = torch.stack((case["U"], case["V"], case["alt"]), dim=-1).to(dev).requires_grad_(True)
    s, uv = fn(vr, case["M"].to(dev), uva, case["n_out"], case["fill_channel"])
    ((s * case["w_s"].to(dev)).sum() + (uv * case["w_uv"].to(dev)).sum()).backward()
    return dict(sample=s.detach().cpu(), uv=uv.detach().cpu(), g_virtual=vr.grad.cpu(), g_uva=uva.grad.cpu())


@functools.lru_cache(maxsize=None)
def oracle_resample(name):
    """The float64 oracle's result for a case, computed once per process."""
    from oracle import resample_oracle

    return run_resample(lambda vr, M, uva, n, f: resample_oracle.resample(vr, M, uva, n_keep=n, fill_channel=f), resample_case(name),
                        torch.device("cpu"))


def pixel_coords(case):
    """(u, v, ix, iy) of every output pixel in float64: the coordinates and where they fall in the virtual image."""
    uva = torch.stack((case["U"], case["V"], case["alt"]), dim=-1).double()
    uv = torch.einsum("ij,hwj->hwi", case["M"].double(), uva)
    Hv, Wv = case["vr"].shape[1:]
    u, v = uv[..., 0].numpy(), uv[..., 1].numpy()
    return u, v, (u + 1) * 0.5 * (Wv - 1), (v + 1) * 0.5 * (Hv - 1)


def left_out(case):
    """(H, W) bool: the pixels whose dL/duva may be left out of the comparison (see the rule above)."""
    _, _, ix, iy = pixel_coords(case)
    m = np.zeros(ix.shape, dtype=bool)
    if case["lattice"]:
        return m
    Hv, Wv = case["vr"].shape[1:]
    if Wv > 1:
        m |= np.abs(ix - np.round(ix)) <= NEAR
    if Hv > 1:
        m |= np.abs(iy - np.round(iy)) <= NEAR
    return m


def _rel(a, b, dims):
    a, b = torch.as_tensor(a).cpu().double(), torch.as_tensor(b).cpu().double()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    scale = b.abs().amax(dim=dims, keepdim=True).clamp_min(1e-30) if dims else b.abs().max().clamp_min(1e-30)
    return (a - b).abs() / scale


def resample_errors(got, ref, case):
    """{quantity: largest error relative to the quantity's scale} under the rule, and the fraction of pixels left out."""
    mask = torch.from_numpy(left_out(case))
    e_uva = _rel(got["g_uva"], ref["g_uva"], (0, 1)).amax(-1)
    e_uva[mask] = 0.0
    err = dict(sample=float(_rel(got["sample"], ref["sample"], (1, 2)).max()), uv=float(_rel(got["uv"], ref["uv"], None).max()),
               g_virtual=float(_rel(got["g_virtual"], ref["g_virtual"], None).max()), g_uva=float(e_uva.max()))
    return err, float(mask.double().mean())


def compare_resample(got, ref, case, tol, what):
    err, frac = resample_errors(got, ref, case)
    assert frac <= MAX_LEFT_OUT, f"{what}: {frac:.3%} of the pixels left out"
    for k, e in err.items():
        assert e <= tol, f"{what}: {k} {e:.3e} of its maximum (bound {tol:g}); all: {err}"
    return err


def tap_cells(case):
    """North-west tap cell (x0, y0) of every output pixel, float64, clamped to [-2, size + 1] (far away is far away)."""
    _, _, ix, iy = pixel_coords(case)
    Hv, Wv = case["vr"].shape[1:]
    return (np.clip(np.floor(ix), -2, Wv + 1).astype(np.int64), np.clip(np.floor(iy), -2, Hv + 1).astype(np.int64))


def reached_cells(x0, y0, Hv, Wv, dilate=1):
    """(Hv, Wv) bool: the cells of [x0, x0 + 1] x [y0, y0 + 1] inside the image, grown by `dilate` cells each way."""
    m = np.zeros((Hv, Wv), dtype=bool)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = (x >= 0) & (x < Wv) & (y >= 0) & (y < Hv)
            m[y[ok], x[ok]] = True
    for _ in range(dilate):
        p = np.pad(m, 1)
        m = np.zeros_like(m)
        for dy in range(3):
            for dx in range(3):
                m |= p[dy:dy + Hv, dx:dx + Wv]
    return m


def output_tiles(H, W):
    return -(-H // OT) * -(-W // OT)


def max_bucket_fill(x0, y0, has_tap, Hv, Wv, n_planes):
    """The gather's fullest bucket: output tiles whose box meets a virtual tile are its candidates in tile order, taken CHT
    at a time; every pixel of a chunk whose north-west cell lies in [vx0 - 1, vx0 + VX) x [vy0 - 1, vy0 + VY) is parked in the
    bucket of that cell. Returns the largest number of pixels one (virtual tile, chunk, bucket) holds."""
    H, W = x0.shape
    VX, VY = virtual_tile(Hv, Wv)
    cht = CHT[nacc(n_planes)]
    ntx, nty = -(-W // OT), -(-H // OT)
    tiles = []
    for ty in range(nty):
        for tx in range(ntx):
            sl = (slice(ty * OT, min((ty + 1) * OT, H)), slice(tx * OT, min((tx + 1) * OT, W)))
            tx0, ty0, ok = x0[sl].ravel(), y0[sl].ravel(), has_tap[sl].ravel()
            box = (tx0[ok].min(), ty0[ok].min(), tx0[ok].max() + 1, ty0[ok].max() + 1) if ok.any() else None
            tiles.append((box, tx0, ty0))
    best = 0
    for vy0 in range(0, Hv, VY):
        for vx0 in range(0, Wv, VX):
            cand = [t for t in tiles if t[0] is not None and t[0][0] <= vx0 + VX - 1 and t[0][2] >= vx0 and t[0][1] <= vy0 + VY - 1
                    and t[0][3] >= vy0]
            for k in range(0, len(cand), cht):
                lx = np.concatenate([t[1] for t in cand[k:k + cht]]) - vx0
                ly = np.concatenate([t[2] for t in cand[k:k + cht]]) - vy0
                lands = (lx >= -1) & (lx < VX) & (ly >= -1) & (ly < VY)
                if lands.any():
                    best = max(best, int(np.bincount(((ly[lands] + 1) * (VX + 1) + lx[lands] + 1)).max()))
    return best


# ---- flow cases -----------------------------------------------------------------------------------------------------
def _grid(H, W):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack((xx, yy))[None]


def _flow(guards, C, H, W, seed, flow):
    g = torch.Generator().manual_seed(seed)
    img, up = torch.rand(C, H, W, generator=g), torch.randn(C, H, W, generator=g)
    return dict(guards=guards, img=img, up=up, flow=flow(g).contiguous())


def _converge(tx, ty):
    return lambda g: torch.tensor([tx, ty]).view(1, 2, 1, 1) - _grid(64, 80)


def _eighths(H, W):
    return lambda g: torch.randint(-48, 49, (1, 2, H, W), generator=g).float() / 8.0  # integer + k/8, |flow| <= 6


# H - 1 and W - 1 are powers of two in the large cases: the reference normalises the position to [-1, 1] and grid_sample
# takes it back to pixels, which rounds unless the divisions are exact (flow_cases.py states the warp in pixels). With the
# same flows at 1232 x 1280 and 1040 x 1024 the reference's fp32 ops on the CPU sat 1.04e-4 / 6.3e-5 (out / g_img) and
# 5.9e-5 / 3.7e-5 from float64, past REF_TOL with no kernel involved; at these shapes they sit at 1.2e-7.
BIG_FLOW = (1025, 2049)
ROUNDS_FLOW = (1025, 1025)
_FLOW = {
    "flow_converge": lambda: _flow("every pixel samples one point: a full bucket with FlowSrc", 3, 64, 80, 21, _converge(40.5, 31.25)),
    "flow_converge_corner": lambda: _flow("everything clamped onto pixel (0, 0): a full bucket on the image corner", 3, 64, 80, 22,
                                          _converge(-50.0, -50.0)),
    "flow_big1": lambda: _flow("the one-plane 64x32-tile FlowSrc instantiation", 1, *BIG_FLOW, 23, _eighths(*BIG_FLOW)),
    "flow_big3": lambda: _flow("the four-plane 64x32-tile FlowSrc instantiation, three planes live", 3, *BIG_FLOW, 24, _eighths(*BIG_FLOW)),
    "flow_big5": lambda: _flow("five planes at 64x32 tiles: a four-plane and a one-plane pass", 5, *BIG_FLOW, 25, _eighths(*BIG_FLOW)),
    "flow_rounds1": lambda: _flow("more than 4096 output tiles: two scan rounds of RB = 4096 with one plane", 1, *ROUNDS_FLOW, 26,
                                  _eighths(*ROUNDS_FLOW)),
    "flow_strided": lambda: _flow("FlowField strides: the field as a slice of a wider tensor and as channels-last memory", 3, 48, 64, 27,
                                  _eighths(48, 64)),
}
FLOW = tuple(_FLOW)


@functools.lru_cache(maxsize=None)
def flow_case(name):
    return _FLOW[name]()


def strided_views(flow):
    """The same (1, 2, H, W) field as non-contiguous views: sliced from a wider tensor, and channels-last."""
    H, W = flow.shape[2:]
    wide = torch.zeros(1, 2, H + 3, W + 16, dtype=flow.dtype, device=flow.device)
    wide[:, :, 2:2 + H, 8:8 + W] = flow
    last = flow.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # strides (., 1, 2 W, 2)
    assert not wide[:, :, 2:2 + H, 8:8 + W].is_contiguous() and last.stride()[1:] == (1, 2 * W, 2)
    return {"sliced": wide[:, :, 2:2 + H, 8:8 + W], "channels_last": last}


def reference_flow_ops(img, flow, upstream):
    """flow_matching.py:225-253 as the reference runs it (fp32 torch ops and autograd), on the tensors' device."""
    x = img.clone().requires_grad_(True)
    C, H, W = x.shape
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid = torch.stack((xx, yy), dim=0).float().to(x.device).unsqueeze(0)
    flow_grid = grid + flow
    flow_grid[:, 0] = 2.0 * flow_grid[:, 0] / (W - 1) - 1.0
    flow_grid[:, 1] = 2.0 * flow_grid[:, 1] / (H - 1) - 1.0
    flow_grid = flow_grid.permute(0, 2, 3, 1)
    out = torch.nn.functional.grid_sample(x.unsqueeze(0), flow_grid.detach(), mode="bilinear", padding_mode="border",
                                          align_corners=True).squeeze(0)
    out.backward(upstream)
    return out.detach(), x.grad


@functools.lru_cache(maxsize=None)
def oracle_flow(name):
    """(out, g_img) of the float64 statement for a flow case, computed once per process."""
    import flow_cases as FC

    c = flow_case(name)
    return FC.warp(c["img"].numpy(), c["flow"].numpy()), FC.warp_adjoint(c["up"].numpy(), c["flow"].numpy())


def flow_errors(got, ref):
    return dict(out=float(_rel(got[0], ref[0], (1, 2)).max()), g_img=float(_rel(got[1], ref[1], None).max()))


def compare_flow(got, ref, tol, what):
    err = flow_errors(got, ref)
    for k, e in err.items():
        assert e <= tol, f"{what}: {k} {e:.3e} of its maximum (bound {tol:g})"
    return err


def flow_tap_cells(flow):
    """First tap (x0, y0) of every pixel, float64 (flow_cases.taps)."""
    import flow_cases as FC

    H, W = flow.shape[2:]
    x0, _, _, y0, _, _ = FC.taps(flow.numpy().reshape(2, H, W), H, W)
    return x0, y0
