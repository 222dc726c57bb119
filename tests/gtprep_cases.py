"""Inputs and references of the ground-truth preparation tests (eogs2_amd.pansharp, eogs2_amd.rescaler,
include/eogs_gtprep.h): a float64 restatement of every piece, the histogram rule in integers, and the per-element rounding
bound of the dark pansharpening family.

What is restated (paths under the reference's src/gaussiansplatting/):
  upsample        torch's F.interpolate(size=(H, W), align_corners=False), bicubic (A = -0.75) and bilinear. The tap positions
                  are part of the rule and are computed in float32 as torch does (scale = in / out, src = fma(scale, dst + 0.5,
                  -0.5), see _src); weights and sums from there on in float64.
  brovey, simple_brovey, ihs                  pansharpening/algorithm/brovey.py, ihs.py
  pansharp_l2, pan_l2, pan_gradient_l2        loss/pansharp_loss.py, loss/PAN_loss.py, with their gradients
  clamp, rescale                              utils/rescaler/rescaler.py, in numpy float32: bit for bit torch's fp32 result
  equalize                                    torchvision's documented per-channel rule of transforms.functional.equalize,
                                              restated in integers (torchvision itself is never imported or compared against)

The dark family and its bound
-----------------------------
`dark` inputs hold a zero corner block and a 0 -> 1 step edge: bicubic undershoot makes W sum_c u_c negative or tiny, the
clamp at 1e-8 decides, and the reference's own brovey_pansharp returns values up to 1e7. A bar relative to the maximum would
hide every other pixel, so brovey on dark inputs is compared per element, none left out, against K * 2^-24 * B_i with

  B_i = |pan| (E_u(c) / d + |u_c| E_d / d^2) + |out_i|
  E_u(c) = sum over the 16 taps of (|wy_j| |wx_i| + |wy_j| ax_i + ay_j |wx_i|) |m_c,ji|
  E_d = W sum_c E_u(c) where the clamp is clearly inactive or undecided, 0 where W S <= 1e-8 - 64 * 2^-24 * W sum_c E_u(c)
        (d is then the constant 1e-8 in float32 too)

all from the float64 restatement. a_k is the sum of the absolute values of the terms of weight k's polynomial in expanded
form (|A| x^3 + 5 |A| x^2 + 8 |A| x + 4 |A| for the outer taps, (A + 2) x^3 + (A + 3) x^2 + 1 for the inner ones): the outer
weights vanish by cancellation at t -> 0 and t -> 1, so their float32 error is absolute (a few 2^-24 of terms of size ~1-30), not
relative to the weight. The last term of B_i covers the roundings of the product, the quotient and the final multiply.

K was measured on the CPU as the smallest integer at which every element of every dark brovey fixture (the reference's own
float32 output, tests/golden/gtprep/) lies inside K * 2^-24 * B_i: see DARK_K below (tests/test_gtprep_reference.py measures it
again and holds it to that value; the lit brovey fixtures, where one channel's undershoot also reaches 1e6 in places, lie
inside the same bound at a largest ratio of 0.125 and are held to it as well). The GPU test uses 4 * DARK_K: the factor 4 is a margin for a different association of the
16-tap sum, not a measurement.
"""
import zlib

import numpy as np

PAIRS = (((1, 1), (1, 1)), ((1, 1), (3, 5)), ((2, 3), (7, 9)), ((5, 7), (20, 28)), ((17, 9), (70, 33)), ((9, 9), (4, 5)),
         ((33, 65), (129, 257)))
CHANNELS = (1, 3, 4, 8)
FAMILIES = ("lit", "dark")
METHODS = ("brovey", "simple_brovey", "ihs")
BROVEY_W = 0.1
LOSS_PAIRS = (((5, 7), (20, 28)), ((33, 65), (129, 257)))
GRADIENT_SHAPES = ((2, 2), (2, 9), (3, 3), (65, 130), (3, 5, 7))
RESCALE_SHAPES = ((3, 1, 1), (3, 5, 7), (1, 33, 17), (3, 129, 257))
RESCALE_KINDS = ("plain", "constant", "inf", "nan")
HIST_SHAPES = ((3, 5, 7), (1, 16, 17), (3, 64, 48))
UPSTREAM = 0.75  # (exact in float32)
REL_BAR = 2e-5  # of max |ref|: the bar of tests/test_shade_oracle.py
EPS32 = 2.0 ** -24
DARK_K = 1  # measured on the CPU: the largest ratio |fixture - restatement| / (2^-24 B_i) over every dark brovey fixture is 0.214
# (at (17, 9) -> (70, 33)); a B_i with relative weight error had needed K ~ 85 there
FIXTURE_STRIDE = 4  # fixtures of the (129, 257) images keep every 4th row and column


def channels_of(method):
    return (3,) if method == "ihs" else CHANNELS


def fixture_channels(method, pair):
    """The channel counts a fixture exists for: all of them at the small sizes, C = 3 at the two large ones."""
    big = pair[1][0] * pair[1][1] > 1000
    return tuple(c for c in channels_of(method) if c == 3 or not big)


def stride_of(shape):
    return FIXTURE_STRIDE if shape[-1] * shape[-2] > 20000 else 1


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def pansharp_inputs(family, C, pair):
    """(msi f32[C,h,w], pan f32[H,W]). lit: both in [0.05, 1]. dark: the MSI image's upper-left block is 0 and its lower rows
    are a 0 -> 1 step edge."""
    (h, w), (H, W) = pair
    r = _rng("pansharp", family, C, pair)
    msi = (0.05 + 0.95 * r.random_sample((C, h, w))).astype(np.float32)
    pan = (0.05 + 0.95 * r.random_sample((H, W))).astype(np.float32)
    if family == "dark":
        msi[:, :(h + 1) // 2, :(w + 1) // 2] = 0.0
        msi[:, h // 2:, :w // 2] = 0.0
        msi[:, h // 2:, w // 2:] = 1.0
    return msi, pan


# ---- upsampling ----------------------------------------------------------------------------------------------------------
def _src(n_in, n_out):
    """The float32 source coordinate of every destination index: scale = in / out rounded to float32, then scale (dst + 0.5) -
    0.5 with ONE rounding (a fused multiply-add; exact in float64 before the cast). The reference's fixtures decide this: with
    the product rounded on its own they miss simple_brovey's dark pixels by up to 0.8 of the maximum, fused they agree to 2e-7."""
    scale = np.float64(np.float32(n_in) / np.float32(n_out))
    return (scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5).astype(np.float32)


def cubic_axis(n_in, n_out):
    """(idx int[n_out,4], weights f64[n_out,4], a f64[n_out,4]): `a` = the absolute sums of the weights' expanded terms."""
    A = -0.75
    src = _src(n_in, n_out)
    fl = np.floor(src)
    t = (src - fl).astype(np.float64)
    i = fl.astype(np.int64)
    inner = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1  # noqa: E731
    outer = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A  # noqa: E731
    a_inner = lambda x: (A + 2) * x ** 3 + (A + 3) * x ** 2 + 1  # noqa: E731
    a_outer = lambda x: -A * (x ** 3 + 5 * x ** 2 + 8 * x + 4)  # noqa: E731
    wt = np.stack([outer(t + 1), inner(t), inner(1 - t), outer(2 - t)], axis=1)
    a = np.stack([a_outer(t + 1), a_inner(t), a_inner(1 - t), a_outer(2 - t)], axis=1)
    idx = np.clip(i[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, wt, a


def linear_axis(n_in, n_out):
    src = np.maximum(_src(n_in, n_out), np.float32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    lam = np.clip(src.astype(np.float64) - i0, 0.0, 1.0)
    idx = np.stack([i0, np.minimum(i0 + 1, n_in - 1)], axis=1)
    wt = np.stack([1 - lam, lam], axis=1)
    return idx, wt, np.abs(wt)


def upsample(msi, H, W, cubic, with_bound=False):
    """f64[C,H,W]; with_bound: also E_u f64[C,H,W] of the module docstring."""
    C, h, w = msi.shape
    axis = cubic_axis if cubic else linear_axis
    iy, wy, ay = axis(h, H)
    ix, wx, ax = axis(w, W)
    m = msi.astype(np.float64)[:, iy[:, :, None, None], ix[None, None, :, :]]  # [C, H, Ty, W, Tx]
    u = np.einsum("cyjxi,yj,xi->cyx", m, wy, wx)
    if not with_bound:
        return u
    awy, awx = np.abs(wy), np.abs(wx)
    am = np.abs(m)
    e = np.einsum("cyjxi,yj,xi->cyx", am, awy, awx) + np.einsum("cyjxi,yj,xi->cyx", am, awy, ax) + np.einsum("cyjxi,yj,xi->cyx", am, ay, awx)
    return u, e


def pansharp(method, msi, pan, W=BROVEY_W, with_bound=False):
    """The float64 restatement of the three methods: f64[C,H,W] (brovey with_bound: also B f64[C,H,W])."""
    H, Wd = pan.shape
    p = pan.astype(np.float64)[None]
    if method == "brovey":
        u, e = upsample(msi, H, Wd, True, with_bound=True)
        Wf = float(np.float32(W))
        S = u.sum(axis=0, keepdims=True)
        d = np.maximum(Wf * S, float(np.float32(1e-8)))
        out = p / d * u
        if not with_bound:
            return out
        e_s = Wf * e.sum(axis=0, keepdims=True)
        clamped = Wf * S <= float(np.float32(1e-8)) - 64 * EPS32 * e_s
        e_d = np.where(clamped, 0.0, e_s)
        return out, np.abs(p) * (e / d + np.abs(u) * e_d / d ** 2) + np.abs(out)
    u = upsample(msi, H, Wd, False)
    S = u.sum(axis=0, keepdims=True)
    if method == "simple_brovey":
        return u * (p / (S + float(np.float32(1e-8))))
    if method == "ihs":
        return np.clip(u + (p - S / 3.0), 0.0, 1.0)
    raise ValueError(method)


def reference_shapes(method, msi, pan):
    """The shapes the reference's function of that name takes."""
    if method == "simple_brovey":
        return pan, msi[None]
    if method == "ihs":
        return pan[None], msi
    return pan, msi


# ---- losses ----------------------------------------------------------------------------------------------------------------
def l2(image, target, upstream=1.0):
    """(mean((image - target)^2), its gradient times upstream) in float64."""
    d = image.astype(np.float64) - target.astype(np.float64)
    return float((d ** 2).mean()), 2.0 * d / d.size * upstream


def loss_inputs(method, pair):
    """(syn f32[3,H,W], msi, pan) of a Pansharploss case: lit inputs and a synthesised image drawn on its own."""
    msi, pan = pansharp_inputs("lit", 3, pair)
    syn = _rng("loss", method, pair).random_sample((3,) + pair[1]).astype(np.float32)
    return syn, msi, pan


def gradient_inputs(shape):
    r = _rng("gradient", shape)
    return r.random_sample(shape).astype(np.float32), r.random_sample(shape).astype(np.float32)


def _grad_matrix(n):
    """G f64[n,n]: torch.gradient along one axis (unit spacing, edge order 1) as a matrix."""
    G = np.zeros((n, n))
    G[0, 0], G[0, 1] = -1, 1
    G[n - 1, n - 2], G[n - 1, n - 1] = -1, 1
    for i in range(1, n - 1):
        G[i, i - 1], G[i, i + 1] = -0.5, 0.5
    return G


def gradient_l2(pan, gt, upstream=1.0):
    """Lgradient_pan and its gradient with respect to `pan`, in float64."""
    d = pan.astype(np.float64) - gt.astype(np.float64)
    Gy, Gx = _grad_matrix(d.shape[-2]), _grad_matrix(d.shape[-1])
    gy = np.einsum("ij,...jx->...ix", Gy, d)
    gx = np.einsum("ij,...yj->...yi", Gx, d)
    loss = float((gy ** 2).mean() + (gx ** 2).mean())
    g = 2.0 / d.size * (np.einsum("ij,...ix->...jx", Gy, gy) + np.einsum("ij,...yi->...yj", Gx, gx))
    return loss, g * upstream


# ---- rescalers -------------------------------------------------------------------------------------------------------------
def rescale_input(shape, kind):
    r = _rng("rescale", shape, kind)
    x = (3.0 * r.standard_normal(shape)).astype(np.float32)
    n = shape[1] * shape[2]
    flat = x.reshape(shape[0], n)
    if kind == "constant":
        flat[0] = np.float32(0.3)
    elif kind == "inf":
        flat[0, 0] = np.inf
        flat[-1, n - 1] = -np.inf
    elif kind == "nan":
        flat[-1, n // 2] = np.nan
    return x


def minmax(x):
    """f32[C,2] with torch.min / torch.max's rule (numpy's min / max also hand a NaN on)."""
    f = x.reshape(x.shape[0], -1)
    with np.errstate(invalid="ignore"):
        return np.stack([f.min(axis=1), f.max(axis=1)], axis=1)


def rescale(x, mm):
    """(x - min) / ((max - min) + 1e-8) in float32, operation by operation as torch evaluates the reference's expression."""
    lo, hi = mm[:, 0][:, None, None], mm[:, 1][:, None, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return ((x - lo) / ((hi - lo) + np.float32(1e-8))).astype(np.float32)


def clamp(x, lo=0.0, hi=1.0):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.minimum(np.maximum(x, np.float32(lo)), np.float32(hi))).astype(np.float32)


def same_bits(a, b):
    """Equal float32 bits; two NaNs count as equal whatever their sign and payload (0 * inf has no canonical one)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan))


# ---- histogram equalisation ----------------------------------------------------------------------------------------------
def to_levels(x):
    """uint8(x * 255): the product in float32, a NaN becomes 0, clamped to [0, 255], truncated."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = x.astype(np.float32) * np.float32(255.0)
    y = np.where(np.isnan(y), np.float32(0), y)
    return np.clip(y, 0, 255).astype(np.int64)


def equalize(x):
    """The restated per-channel rule, in integers; f32[C,H,W] = lut[level] / 255."""
    v = to_levels(x)
    out = np.empty(x.shape, np.float32)
    for c in range(x.shape[0]):
        hist = np.bincount(v[c].reshape(-1), minlength=256)
        nonzero = hist[hist != 0]
        step = int(nonzero[:-1].sum()) // 255
        if step == 0:
            lut = np.arange(256)
        else:
            cum = np.cumsum(hist)
            lut = np.zeros(256, np.int64)
            lut[1:] = np.clip((cum[:-1] + step // 2) // step, 0, 255)
        out[c] = lut[v[c]].astype(np.float32) / np.float32(255.0)
    return out


def hist_input(shape, kind):
    """plain: (3,5,7) has 35 pixels a channel, so step == 0 there; single: one level only; all: every one of the 256 levels;
    edges: 0, 1, just outside both, NaN and infinities among ordinary values."""
    r = _rng("hist", shape, kind)
    x = r.random_sample(shape).astype(np.float32)
    n = shape[1] * shape[2]
    flat = x.reshape(shape[0], n)
    if kind == "single":
        flat[0] = np.float32(0.4)
    elif kind == "all":
        if n >= 256:
            flat[0, :256] = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255.0)
    elif kind == "edges":
        special = np.array([0.0, 1.0, -1e-7, np.nextafter(np.float32(1), np.float32(2)), -3.0, 7.0, np.nan, np.inf, -np.inf, 1.0 / 255.0,
                            np.nextafter(np.float32(1.0 / 255.0), np.float32(0))], np.float32)
        k = min(n, special.size)
        flat[-1, :k] = special[:k]
    return x
