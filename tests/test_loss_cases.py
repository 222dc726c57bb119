"""CPU: the photometric-loss edge cases (tests/loss_cases.py) are what they claim to be, the oracle's new pieces are pinned,
and the bound of loss_cases is reachable by fp32 arithmetic of the kernel's shape — shown without a GPU by a transcription of
csrc/loss.hip's sums in torch (run with -s for the error / bound of every family; DESIGN.md 5 keeps the table)."""
from math import exp

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as lc
from util import GOLDEN_LOSS, assert_close, load_golden

from oracle import loss_oracle as lo


# ---- 1. the fp32 path of the oracle ----
@pytest.mark.parametrize("name", GOLDEN_LOSS)
def test_fp32_oracle_path_matches_float64_and_the_reference_vectors(name):
    c = load_golden(name)
    img, gt = torch.from_numpy(c["img"]), torch.from_numpy(c["gt"])
    lam = float(c["lambda_dssim"])
    fns = {"l1": lo.l1_loss, "ssim": lo.ssim, "lphotom": lambda a, b, dtype: lo.lphotom(a, b, lam, dtype=dtype)}
    for key, fn in fns.items():
        v32, g32 = lc.val_grad(lambda a, b: fn(a, b, dtype=torch.float32), img, gt)
        v64, g64 = lc.val_grad(lambda a, b: fn(a, b, dtype=torch.float64), img, gt)
        assert v32.dtype == torch.float32 and v64.dtype == torch.float64
        for what, v, g in (("float64", v64, g64), ("reference", c[key], torch.from_numpy(c["g_" + key]))):
            assert abs(float(v32) - float(v)) <= 1e-5 * max(abs(float(v)), 1e-3), (key, what)
            assert_close(g32, g, f"{name}:g_{key} fp32 path vs {what}", rtol=1e-4, allow_flips=False)
    if "ssim_per_image" in c:
        w = torch.arange(1, img.shape[0] + 1, dtype=torch.float32)
        v32, g32 = lc.val_grad(lambda a, b: lo.ssim(a, b, size_average=False, dtype=torch.float32), img, gt, w)
        v64, g64 = lc.val_grad(lambda a, b: lo.ssim(a, b, size_average=False), img, gt, w.double())
        assert np.allclose(v32.numpy(), v64.numpy(), rtol=1e-5) and np.allclose(v32.numpy(), c["ssim_per_image"], rtol=1e-5)
        assert_close(g32, g64, f"{name}:g_ssim_per_image fp32 path", rtol=1e-4, allow_flips=False)


# ---- 2. the addends ----
@pytest.mark.parametrize("name", list(lc.CONDITIONING) + ["near4d"])
def test_ssim_addends_sum_to_the_gradient(name):
    img, gt = lc.near((2, 3, 24, 37)) if name == "near4d" else lc.case(name)
    add = lo.ssim_addends(img, gt)
    assert add.dtype == torch.float64 and tuple(add.shape) == (3,) + tuple(img.shape)
    x = img.double().requires_grad_(True)
    lo.ssim_map(x, gt).sum().backward()
    # ~300 float64 operations per element from the same window sums: 1e-12 of the largest addend is rounding, nothing else
    assert float((add.sum(0) - x.grad).abs().max()) <= 1e-12 * float(add.abs().max())


# ---- 3. a transcription of the kernel's arithmetic reaches the bound ----
WIN, HALO = 11, 5
f32 = np.float32


def kernel_window():
    """loss_window(): exp in double, stored as fp32, normalised by their exact sum rounded once to fp32."""
    g = [f32(exp(-((i - WIN // 2) ** 2) / (2.0 * 1.5 * 1.5))) for i in range(WIN)]
    s = f32(sum(float(v) for v in g))
    return [float(f32(v / s)) for v in g]


def test_kernel_window_is_the_references_window(hip_lib):
    """The library's taps are the reference's gaussian(11, 1.5) bit for bit, `gauss / gauss.sum()` in fp32. (An fp32 running
    sum is one ulp below torch's: every tap 6e-8 too heavy, the window's sum 1.6e-7 above the reference's, and the mean SSIM
    of flat_0.95_0.01 1.3e-5 = 36 x the bound from float64. The kernel normalised that way before these tests.)"""
    import ctypes

    g = torch.tensor([exp(-((x - WIN // 2) ** 2) / float(2 * 1.5**2)) for x in range(WIN)], dtype=torch.float32)
    ref = g / g.sum()
    taps = (ctypes.c_float * WIN)()
    hip_lib.check(hip_lib.loss_window(taps))
    assert list(taps) == [float(v) for v in ref] == kernel_window()
    assert torch.equal(ref[:, None].mm(ref[None, :]).double(), lo.window_2d())
    assert hip_lib.loss_window(None) == -1


def _taps(t, k_dim):
    """The 11 zero-padded shifts of t along one axis: what a window at each pixel reads, in k order."""
    pad = (HALO, HALO) if k_dim == -1 else (0, 0, HALO, HALO)
    p = F.pad(t, pad)
    n = t.shape[k_dim]
    return [p.narrow(k_dim, k, n) for k in range(WIN)]


def _window_1d(t, k_dim, w):
    acc = torch.zeros_like(t)
    for k, s in enumerate(_taps(t, k_dim)):
        acc = acc + w[k] * s
    return acc


def reference_window_sum():
    """The sum of the reference's 2-D window (fp32 products of the taps), as loss_window() hands it to the kernel."""
    w = np.array(kernel_window(), dtype=f32)
    return float(np.outer(w, w).astype(f32).astype(np.float64).sum())


def pivot_map(gt, tile):
    """Per pixel, the pivot of its tile: the median of the ground truth at the four corners and the centre of the tile's part
    inside the image (fmin / fmax pass over a NaN sample), 0 if that is not finite."""
    th, tw = tile
    H, W = gt.shape[-2:]
    out = torch.zeros_like(gt)
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            h, w = min(th, H - y0), min(tw, W - x0)
            a, b, c, d = (gt[..., y0 + r, x0 + q] for r in (0, h - 1) for q in (0, w - 1))
            e = gt[..., y0 + h // 2, x0 + w // 2]
            f, g = torch.fmax(torch.fmin(a, b), torch.fmin(c, d)), torch.fmin(torch.fmax(a, b), torch.fmax(c, d))
            m = torch.fmax(torch.fmin(f, g), torch.fmin(torch.fmax(f, g), e))
            out[..., y0:y0 + h, x0:x0 + w] = torch.where(torch.isfinite(m), m, torch.zeros_like(m))[..., None, None]
    return out


def _tile_moments(x, y, w, tile):
    """The five window sums of u = x - p, v = y - p per tile (p: pivot_map; the zero padding shifted like the image)."""
    th, tw = tile
    P, H, W = x.shape
    piv = pivot_map(y, tile)
    out = [torch.zeros_like(x) for _ in range(5)]
    xp, yp = F.pad(x, (HALO, HALO, HALO, HALO)), F.pad(y, (HALO, HALO, HALO, HALO))
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            h, wd = min(th, H - y0), min(tw, W - x0)
            p = piv[:, y0:y0 + 1, x0:x0 + 1]
            u, v = xp[:, y0:y0 + h + 2 * HALO, x0:x0 + wd + 2 * HALO] - p, yp[:, y0:y0 + h + 2 * HALO, x0:x0 + wd + 2 * HALO] - p
            m = [torch.zeros_like(u[..., :wd]) for _ in range(5)]
            for k in range(WIN):
                a, b = u[..., k:k + wd], v[..., k:k + wd]
                wa, wb = w[k] * a, w[k] * b
                m = [m[0] + wa, m[1] + wb, m[2] + wa * a, m[3] + wb * b, m[4] + wa * b]
            for i in range(5):
                acc = torch.zeros_like(m[i][:, :h])
                for k in range(WIN):
                    acc = acc + w[k] * m[i][:, k:k + h]
                out[i][:, y0:y0 + h, x0:x0 + wd] = acc
    return piv, out


def transcription(img, gt, mode, tile=(16, 32)):
    """(value, gradient) as csrc/loss.hip computes them, one fp32 torch op per operation and no fused multiply-add: per tile
    the moments about the tile's pivot — the horizontal window with w*u, (w*u)*u, (w*u)*v, the vertical window over the five
    sums — the reference's means and variances from them, _ssim and its three derivative maps, the same separable window over
    the maps, and the last line. Not the kernel's reduction order (torch's fp32 sum) and not its contraction: what is shown
    is that arithmetic of this shape sits inside the bound. The tile sums are of S - 1, the means and out[0] formed in double."""
    assert img.dtype == gt.dtype == torch.float32
    w = kernel_window()
    planes, n = img.numel() // (img.shape[-2] * img.shape[-1]), img.numel()
    x, y = img.reshape((planes,) + tuple(img.shape[-2:])), gt.reshape((planes,) + tuple(img.shape[-2:]))
    inv_n = float(f32(1.0 / n))
    w_l1, w_ss, bias = {"l1": (1.0, 0.0, 0.0), "ssim": (0.0, 1.0, 0.0),
                        "photometric": tuple(float(f32(v)) for v in (1.0 - lc.LAMBDA, -lc.LAMBDA, lc.LAMBDA))}[mode]
    one = lambda v: torch.tensor(v, dtype=torch.float32)
    l1m, sm = one(0.0).double(), one(0.0).double()  # the means are formed in double from the fp32 sums
    g = torch.zeros_like(x)
    if mode != "ssim":
        d = x - y
        l1m = d.abs().sum().double() / n
        g = g + (one(w_l1) * inv_n) * torch.sign(d)
    if mode != "l1":
        piv, (U, V, Uu, Vv, Uv) = _tile_moments(x, y, w, tile)
        ws = reference_window_sum()
        ws, c1, c0 = float(f32(ws)), float(f32(1.0 - ws)), float(f32(ws * (1.0 - ws)))
        mu1, mu2 = piv * ws + U, piv * ws + V
        pp, p1 = c0 * piv * piv, c1 * piv
        C1, C2 = float(f32(0.01) * f32(0.01)), float(f32(0.03) * f32(0.03))
        mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s11, s22 = (Uu - U * U) + (p1 * (2.0 * U) + pp), (Vv - V * V) + (p1 * (2.0 * V) + pp)
        s12 = (Uv - U * V) + (p1 * (U + V) + pp)
        A1, A2 = 2.0 * mu12 + C1, 2.0 * s12 + C2
        B1, B2 = mu1_sq + mu2_sq + C1, s11 + s22 + C2
        inv = 1.0 / (B1 * B2)
        S = (A1 * A2) / (B1 * B2)
        sm = 1.0 + (S - 1.0).sum().double() / n  # the sums are of S - 1
        d11 = -S / B2
        d12 = 2.0 * A1 * inv
        dm = 2.0 * mu2 * A2 * inv - 2.0 * mu1 * S / B1 - 2.0 * mu1 * d11 - mu2 * d12
        cm, c11, c12 = (_window_1d(_window_1d(t, -1, w), -2, w) for t in (dm, d11, d12))
        g = g + (one(w_ss) * inv_n) * (cm + 2.0 * x * c11 + y * c12)
    # (out[0] is combined in double from the unrounded means; every output is rounded once)
    value = {"l1": l1m, "ssim": sm, "photometric": w_l1 * l1m + (w_ss * sm + bias)}[mode].float()
    assert value.dtype == g.dtype == torch.float32
    return value, g.reshape(img.shape)


@pytest.mark.parametrize("name", lc.CONDITIONING)
def test_transcription_of_the_kernel_reaches_the_bound(hip_lib, name):
    """Every family at most 0.47 of the bound (DESIGN.md 5 has every figure beside the kernel's own)."""
    img, gt = lc.case(name)
    for mode in lc.MODES:
        v, g = transcription(img, gt, mode, lc.tile_shape())
        lc.reference(name, mode).check(f"transcription:{name}", v, g)


def test_transcription_is_the_same_function_on_ordinary_images():
    """On well-conditioned content the transcription is held to the suite's ordinary bar: it is the kernel's formulas, not
    something that merely happens to be near on flat images."""
    img, gt = lc.near((3, 48, 42))
    for mode in lc.MODES:
        v, g = transcription(img, gt, mode)
        v64, g64 = lc.val_grad(lc.oracle_fn(mode), img.double(), gt)
        assert abs(float(v) - float(v64)) <= 1e-5 * max(abs(float(v64)), 1e-3), mode
        assert_close(g, g64, f"transcription:{mode}", allow_flips=False)


# ---- 4. the cases meet the conditions they name ----
def test_patches_have_bit_equal_pixels_and_only_there():
    img, gt = lc.case("patches")
    tied = lc.patches_tied_mask()
    assert torch.equal(img == gt, tied)
    frac = float(tied.double().mean())
    assert 0.4 < frac < 0.6
    # constant 8 x 8 blocks of gt, several levels
    C, H, W = lc.COND_SHAPE
    blocks = gt.reshape(C, H // lc.PATCH, lc.PATCH, W // lc.PATCH, lc.PATCH)
    assert torch.equal(blocks, blocks[:, :, :1, :, :1].expand_as(blocks)) and gt.unique().numel() == C * (H // lc.PATCH) * (W // lc.PATCH)
    # the untied pixels are off by about 1e-3
    d = (img - gt)[~tied].abs()
    assert 0 < float(d.min()) and 5e-4 < float(d.mean()) < 1.5e-3


def test_conditioning_families_are_what_they_say():
    assert len(lc.CONDITIONING) == 19
    th, tw = lc.tile_shape()
    for name, lv, out in (("origins_bright", 0.02, 1.0), ("origins_bright_fine", 0.02, 1.0), ("origins_dark", 0.95, 0.0)):
        img, gt = lc.case(name)
        at = torch.zeros(lc.COND_SHAPE, dtype=torch.bool)
        at[..., ::th, ::tw] = True
        assert int(at.sum()) == 3 * lc.tiles_per_plane(lc.COND_SHAPE)  # one per tile
        assert bool((img[at] == out).all()) and bool((gt[at] == out).all()) and float((gt[~at] - lv).abs().max()) < 0.01
    for name in lc.CONDITIONING:
        img, gt = lc.case(name)
        assert tuple(img.shape) == tuple(gt.shape) == lc.COND_SHAPE and img.dtype == gt.dtype == torch.float32
    for lv in lc.LEVELS:
        img, gt = lc.case(f"flat_{lv:g}_0")
        assert torch.equal(img, gt) and bool((gt == f32(lv)).all())
        for a in lc.AMPS[1:]:
            img, gt = lc.case(f"flat_{lv:g}_{a:g}")
            assert 0.8 * a < float((gt - lv).std()) < 1.2 * a and 0.8 * a < float((img - gt).std()) < 1.2 * a
    img, gt = lc.case("step")
    assert bool((gt[..., :36] == f32(0.9)).all()) and bool((gt[..., 36:] == f32(0.1)).all())
    img, gt = lc.case("wide")
    assert -1.0 <= float(gt.min()) < -0.9 and 2.9 < float(gt.max()) <= 3.0 and float(img.min()) < -1.0
    img, gt = lc.case("bright")
    assert float(gt.max()) > 990 and float(img.max()) > 1000  # not clamped
    for name in lc.SINGLE_PIXEL:
        img, gt = lc.case(name)
        t = gt if name.startswith("gt_") else img
        at = (0, th, tw) if name.startswith("gt_") else lc.NONFINITE_AT  # a tile's origin / inside a tile
        bad = ~torch.isfinite(t)
        assert int(bad.sum()) == 1 and bool(bad[at]) and bool(torch.isfinite(img if t is gt else gt).all())
        assert min(at[1], t.shape[1] - 1 - at[1]) > 2 * HALO and min(at[2], t.shape[2] - 1 - at[2]) > 2 * HALO
        assert (at[1] % th == 0 and at[2] % tw == 0) == name.startswith("gt_")
    img, gt = lc.case("gt_inf_corners")
    assert tuple(gt.shape) == (1, th, tw) and int((~torch.isfinite(gt)).sum()) == 3 and bool(torch.isfinite(img).all())
    assert int(torch.isfinite(lc.reference("gt_inf_corners", "ssim").g32).sum()) > 0  # pixels out of the three windows' reach


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def test_reduction_shapes_have_the_stated_tile_and_plane_counts(hip_lib):
    th, tw = lc.tile_shape()
    for shape, tiles in lc.REDUCTION_TILES.items():
        assert lc.tiles_per_plane(shape) == tiles == -(-shape[-2] // th) * -(-shape[-1] // tw), shape
    for shape, planes in lc.REDUCTION_PLANES.items():
        assert int(np.prod(shape[:-2])) == planes and lc.tiles_per_plane(shape) == 1, shape
    assert lc.tiles_per_plane(lc.COND_SHAPE) == 9 and lc.COND_SHAPE[-2] % th and lc.COND_SHAPE[-1] % tw  # 3 x 3, partial in both
    # every tile of a ramp plane has its own partial: no two L1 or SSIM sums of the 257 tiles coincide
    img, gt = lc.ramp((1, 4112, 32))
    l1 = (img.double() - gt.double()).abs().reshape(257, -1).sum(1)
    ss = lo.ssim_map(img, gt).reshape(257, -1).sum(1)
    assert l1.unique().numel() == ss.unique().numel() == 257
    assert float(l1[-1] / l1.sum()) > 5e-3 and float(ss.min() / ss.sum()) > 1e-3  # against the 1e-5 value bar


def test_loss_row_limit_is_the_tile_rows_of_one_grid_dimension(hip_lib):
    """loss_check counts rows in the launch's own tile height (it kept the 32-row tile's count once the tile had 16 rows, and
    passed heights whose launch asked for up to 131070 rows of workgroups). Answered before anything touches a device."""
    import ctypes

    th, _ = lc.tile_shape()
    one = ctypes.c_void_p(256)  # never dereferenced
    assert hip_lib.loss_forward(1, th * 65535 + 1, 1, one, one, 1, 1.0, 0.0, 0.0, one, None, one, 1 << 40, None) == -1
    assert b"rows" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.loss_backward(1, th * 65535 + 1, 1, one, one, 1, 1.0, 0.0, None, None, one, 1 << 40, one, None) == -1
    assert b"rows" in hip_lib.cdll.eogs_rast_last_error()
    if th < 32:  # (what the 32-row count let through; with a tile of 32 rows it is a valid size, and these pointers are not)
        assert hip_lib.loss_forward(1, 32 * 65535, 1, one, one, 1, 1.0, 0.0, 0.0, one, None, one, 1 << 40, None) == -1
    assert hip_lib.loss_tile_shape(None, None) == -1
