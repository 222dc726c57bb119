"""Seeded inputs of the photometric-loss edge tests and the bound they are held to (no GPU import).

Used by tests/test_loss_cases.py (CPU: the cases meet the conditions they name, an fp32 transcription of the kernel's
arithmetic reaches the bound) and tests/test_gpu_loss_edges.py (MI355X: eogs2_amd.losses against oracle/loss_oracle.py).

Every generator returns (img, gt) as fp32 CPU tensors; img is the render (differentiated), gt the ground truth.

The bound. Where SSIM is ill-conditioned — flat areas rendered to 1e-3, where sigma^2 = E[x^2] - mu^2 cancels in fp32 against
C2 = 9e-4 — no fp32 evaluation is within 1e-4 of float64, the reference's own included. There the project's rule
(optim_cases._computed_close) applies: the kernel may sit no further from float64 than 4 x the reference's own fp32 run does,

    |hip - f64|.max() <= max(4 * |ref32 - f64|.max(), floor)

per plane for gradients, per scalar for values. ref32 is oracle/loss_oracle.py with dtype=float32 on the CPU (so the bound does
not depend on a device's convolution library). The floors are what fp32 can resolve at all:
  values                     4 ulp of |f64|
  gradients with SSIM        4 ulp of the plane's largest g_ss-scaled addend (oracle ssim_addends): the gradient is an fp32 sum
                             of three such addends, and where they cancel (img == gt: a true gradient of 1e-18) the sum cannot
                             be finer than their ulp
  gradients of L1 alone      1 ulp of g_l1 = 1/N: the sign of an fp32 difference is exact
"""
import functools

import numpy as np
import torch

from oracle import loss_oracle as lo

LAMBDA = 0.2
MODES = ("l1", "ssim", "photometric")
FACTOR = 4  # optim_cases._computed_close


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- conditioning families: three tile rows and three tile columns, partial in both ----
COND_SHAPE = (3, 40, 72)
LEVELS = (0.02, 0.5, 0.95)
AMPS = (0.0, 1e-4, 1e-3, 1e-2)


def flat(level, amp, seed=11):
    g = _gen(seed)
    gt = level + amp * torch.randn(COND_SHAPE, generator=g)
    return gt + amp * torch.randn(COND_SHAPE, generator=g), gt


def step(seed=12):
    gt = torch.full(COND_SHAPE, 0.9)
    gt[..., 36:] = 0.1
    return gt + 1e-3 * torch.randn(COND_SHAPE, generator=_gen(seed)), gt


PATCH = 8


def patches_tied_mask():
    """True where `patches` renders gt bit for bit: every other 8 x 8 block, as a chessboard."""
    _, H, W = COND_SHAPE
    by, bx = torch.arange(H)[:, None] // PATCH, torch.arange(W)[None, :] // PATCH
    return (((by + bx) % 2) == 0).expand(COND_SHAPE)


def patches(seed=13):
    g = _gen(seed)
    C, H, W = COND_SHAPE
    lv = torch.rand(C, H // PATCH, W // PATCH, generator=g)
    gt = lv.repeat_interleave(PATCH, 1).repeat_interleave(PATCH, 2).contiguous()
    img = torch.where(patches_tied_mask(), gt, gt + 1e-3 * torch.randn(COND_SHAPE, generator=g))
    return img, gt


def wide(seed=14):
    g = _gen(seed)
    gt = 4.0 * torch.rand(COND_SHAPE, generator=g) - 1.0  # [-1, 3]: negative means, products of either sign
    return gt + 0.1 * torch.randn(COND_SHAPE, generator=g), gt


def bright(seed=15):
    g = _gen(seed)
    gt = 1e3 * torch.rand(COND_SHAPE, generator=g)  # C1 and C2 vanish against the moments; renders are not clamped
    return gt + 30.0 * torch.randn(COND_SHAPE, generator=g), gt


def origins(level, amp, outlier, seed=17):
    """A flat image with one unrepresentative pixel, in render and ground truth alike, at the origin of EVERY tile of the
    kernel (a glint on dark water, a dark pixel on a bright roof): a kernel that conditions its sums on one pixel of the tile
    — its first — is as ill-conditioned here as one that does not condition them at all."""
    th, tw = tile_shape()
    img, gt = flat(level, amp, seed)
    img[..., ::th, ::tw] = outlier
    gt[..., ::th, ::tw] = outlier
    return img, gt


CONDITIONING = {f"flat_{lv:g}_{a:g}": functools.partial(flat, lv, a) for lv in LEVELS for a in AMPS}
CONDITIONING.update(step=step, patches=patches, wide=wide, bright=bright,
                    origins_bright=functools.partial(origins, 0.02, 1e-3, 1.0),
                    origins_bright_fine=functools.partial(origins, 0.02, 1e-4, 1.0),
                    origins_dark=functools.partial(origins, 0.95, 1e-3, 0.0))


# ---- geometry: well-conditioned content at the tile's and the window's edges ----
def near(shape, seed=None):
    g = _gen(100 + sum(shape) if seed is None else seed)
    gt = torch.rand(shape, generator=g)
    return gt + 0.03 * torch.randn(shape, generator=g), gt


GEOMETRY_SHAPES = ((1, 1, 1), (1, 1, 37), (1, 37, 1), (2, 5, 5), (1, 6, 6), (1, 11, 11), (1, 15, 31), (1, 16, 32), (1, 17, 33),
                   (1, 32, 64), (3, 48, 42), (1, 43, 75))


# ---- reduction: more tiles than the plane reduce has threads, more planes than any other checked case ----
# Values are held to 1e-5 of the value (test_gpu_loss._close_val). The render's noise grows with the row, so the partials of
# a plane's tiles all differ: in the 4096-row planes the L1 partial of tile t is ~ (t + 1/2) / tiles^2 of the plane's sum with
# 3 % of noise of its own (512 pixels), the SSIM partial 1/tiles of it. A dropped or doubled partial moves the SSIM mean by
# 4e-3 and the L1 mean by up to 8e-3 (the last tile, the one a stride off by one loses); only the first tile's L1 partial
# (1.5e-5 of the sum) is near the bar. In the many-plane cases one tile is one plane: a dropped plane moves either mean by
# 1/planes >= 7e-3, and the per-image values of size_average=False (weights 1..33) tell swapped planes apart.
REDUCTION_TILES = {(1, 4080, 32): 255, (1, 4096, 32): 256, (1, 4112, 32): 257}
REDUCTION_PLANES = {(65, 5, 7): 65, (33, 4, 5, 7): 132}
REDUCTION_SHAPES = tuple(REDUCTION_TILES) + tuple(REDUCTION_PLANES)


def ramp(shape, seed=None):
    g = _gen(200 + sum(shape) if seed is None else seed)
    H = shape[-2]
    gt = torch.rand(shape, generator=g)
    row = (torch.arange(H, dtype=torch.float32) / H)[:, None]
    return gt + 0.1 * row * torch.randn(shape, generator=g), gt


# ---- one non-finite pixel, away from the border ----
NONFINITE_SHAPE = (1, 40, 72)
NONFINITE_AT = (0, 19, 35)


def nonfinite(value, seed=16):
    img, gt = near(NONFINITE_SHAPE, seed)
    img[NONFINITE_AT] = value
    return img, gt


def nonfinite_gt(value, seed=18):
    """The ground truth's pixel at a tile origin of the kernel, where a per-tile pivot would be read."""
    th, tw = tile_shape()
    img, gt = near(NONFINITE_SHAPE, seed)
    gt[0, th, tw] = value
    return img, gt


def gt_inf_corners(seed=19):
    """One tile whose ground truth is +inf at three of its corners: most of what a per-tile statistic could sample. The
    pixels further than the window's reach from all three must stay finite."""
    th, tw = tile_shape()
    img, gt = near((1, th, tw), seed)
    gt[0, 0, 0] = gt[0, 0, tw - 1] = gt[0, th - 1, 0] = float("inf")
    return img, gt


NONFINITE = {"nan_pixel": functools.partial(nonfinite, float("nan")), "inf_pixel": functools.partial(nonfinite, float("inf")),
             "gt_nan_origin": functools.partial(nonfinite_gt, float("nan")), "gt_inf_origin": functools.partial(nonfinite_gt, float("inf")),
             "gt_inf_corners": gt_inf_corners}
SINGLE_PIXEL = ("nan_pixel", "inf_pixel", "gt_nan_origin", "gt_inf_origin")  # one non-finite pixel, 2 x the halo from every border


# ---- the two sides and the bound ----
def oracle_fn(mode, dtype=torch.float64):
    return {"l1": lambda a, b: lo.l1_loss(a, b, dtype=dtype),
            "ssim": lambda a, b: lo.ssim(a, b, dtype=dtype),
            "photometric": lambda a, b: lo.lphotom(a, b, LAMBDA, dtype=dtype)}[mode]


def hip_fn(mode):
    from eogs2_amd import losses

    return {"l1": losses.l1_loss, "ssim": losses.ssim,
            "photometric": lambda a, b: losses.photometric_loss(a, b, LAMBDA)[0]}[mode]


def val_grad(fn, img, gt, weights=None):
    x = img.clone().requires_grad_(True)
    v = fn(x, gt)
    (v if v.ndim == 0 else (v * weights).sum()).backward()
    return v.detach(), x.grad


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def grad_floor(img, gt, mode):
    """Per plane, float64 [planes]."""
    n = img.numel()
    planes = n // (img.shape[-2] * img.shape[-1])
    if mode == "l1":
        return torch.full((planes,), ulp32(1.0 / n), dtype=torch.float64)
    g_ss = (1.0 if mode == "ssim" else LAMBDA) / n
    add = torch.nan_to_num(lo.ssim_addends(img, gt).abs(), nan=0.0, posinf=0.0)  # (a non-finite pixel's neighbourhood: no part)
    top = add.reshape(3, planes, -1).amax(dim=(0, 2)) * g_ss
    return torch.tensor([FACTOR * ulp32(t) for t in top], dtype=torch.float64)


def bound(f64, ref32, floor):
    """The project's rule on one quantity (a scalar, or the elements of one plane): the larger of FACTOR x the reference's
    own fp32-to-float64 distance and the floor. Non-finite elements (of either side) take no part."""
    d = (ref32.double() - f64.double()).abs()
    d = d[torch.isfinite(d)]
    return max(FACTOR * (float(d.max()) if d.numel() else 0.0), float(floor))


class Reference:
    """Both CPU sides of one (img, gt, mode): float64 and the reference's fp32 run, values and gradients, and the floors."""

    def __init__(self, img, gt, mode):
        self.mode, self.shape = mode, tuple(img.shape)
        self.planes = img.numel() // (img.shape[-2] * img.shape[-1])
        self.v64, self.g64 = val_grad(oracle_fn(mode), img.double(), gt)  # a float64 leaf: the gradient is not rounded to fp32
        self.v32, self.g32 = val_grad(oracle_fn(mode, torch.float32), img, gt)
        assert self.g64.dtype == self.v64.dtype == torch.float64 and self.g32.dtype == self.v32.dtype == torch.float32
        self.floor_g = grad_floor(img, gt, mode)
        self.floor_v = FACTOR * ulp32(self.v64) if bool(torch.isfinite(self.v64)) else 0.0

    def value_ratio(self, v):
        """error / bound of a value."""
        return abs(float(v) - float(self.v64)) / bound(self.v64, self.v32, self.floor_v)

    def grad_ratios(self, g):
        """error / bound per plane over the elements that are finite in float64 and in `g`'s own run."""
        g = g.detach().cpu().double().reshape(self.planes, -1)
        g64, g32 = self.g64.reshape(self.planes, -1), self.g32.reshape(self.planes, -1)
        out = []
        for p in range(self.planes):
            ok = torch.isfinite(g64[p]) & torch.isfinite(g[p])
            err = (g[p] - g64[p]).abs()[ok]
            out.append((float(err.max()) if err.numel() else 0.0) / bound(g64[p], g32[p], self.floor_g[p]))
        return out

    def check(self, what, v, g, log=print):
        rv, rg = self.value_ratio(v), max(self.grad_ratios(g))
        log(f"{what}:{self.mode}: value error / bound {rv:.3f}, gradient error / bound {rg:.3f}")
        assert rv <= 1.0, f"{what}:{self.mode}: value {float(v)!r} vs float64 {float(self.v64)!r}: {rv:.3f} x bound"
        assert rg <= 1.0, f"{what}:{self.mode}: gradient {rg:.3f} x bound (per plane {['%.3f' % r for r in self.grad_ratios(g)]})"
        return rv, rg


@functools.lru_cache(maxsize=None)
def case(name):
    img, gt = {**CONDITIONING, **NONFINITE}[name]()
    return img, gt


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    return Reference(*case(name), mode)


def tile_shape():
    """(tile_h, tile_w) of the built library: the loss kernels' own constants, asked through the C-ABI."""
    import ctypes

    from eogs2_amd import _lib

    h, w = ctypes.c_int(), ctypes.c_int()
    abi = _lib.get()
    abi.check(abi.loss_tile_shape(ctypes.byref(h), ctypes.byref(w)))
    return h.value, w.value


def tiles_per_plane(shape):
    """Through eogs_loss_bytes: the L1 workspace is one 8-byte pair per tile and plane plus what does not depend on the image's
    size. This leans on loss_layout carving in multiples of 256 bytes (32 planes x 8 bytes: no padding between tile counts) and
    asserts as much; it is the workspace's own count, which tests/test_loss_cases.py sets beside the one from tile_shape()."""
    import ctypes

    from eogs2_amd import _lib
    from eogs2_amd._abi import LOSS_L1

    abi = _lib.get()

    def nbytes(H, W):
        n = ctypes.c_size_t()
        abi.check(abi.loss_bytes(32, H, W, LOSS_L1, ctypes.byref(n)))
        return n.value

    per_tile = 32 * 2 * 4
    one = nbytes(1, 1)  # one tile
    assert (nbytes(shape[-2], shape[-1]) - one) % per_tile == 0
    return 1 + (nbytes(shape[-2], shape[-1]) - one) // per_tile
