"""Shared by the regulariser tests (tests/test_reg_cases.py on the CPU, tests/test_gpu_reg.py on the GPU) and by
tests/golden/make_golden_reg.py: seeded inputs, a plain-torch restatement of the reference's five regularisers
(src/gaussiansplatting/loss/opacity.py:14-17,30-35,44-45, loss/main_loss.py:26-34,46-50) on the RAW parameters, the derived
error bounds of their fp32 formulas, and the comparison helpers.

The bounds are not chosen, they are a first-order running error analysis of the fp32 formula, evaluated in float64 beside
the float64 value of every intermediate (`gauss_bounds`, `image_bounds`):

  * every fp32 +, -, *, / and sqrt rounds once: relative error U = 2^-24;
  * exp, log, expm1 are taken as accurate to 2 ulp: relative error FN = 4 U (torch's vectorised CPU functions and the device
    library document 1 ulp);
  * an error d_x of an input passes through an operation with the operation's derivative (log: d_x / x, sqrt: d_x / 2 sqrt x,
    a product: |a| d_b + |b| d_a, ...), so the ill-conditioned spots of the formulas - 1 - sigmoid for large logits,
    log(q + 1e-6) of a needle's q ~ 1, -log(e + 1e-5) where e ~ 1e-5 - widen the bound exactly where fp32 loses digits;
  * a sum of n addends carries SUM_DEPTH(n) U times the sum of their magnitudes: torch's CPU sum is a cascade of four levels
    of at most 2^max(4, ceil(log2 n / 4)) sequential additions each, plus at most 16 additions to combine levels, unrolled
    accumulators and vector lanes (the HIP kernels sum in float64 and stay far inside this part).

Scalars: the bound is absolute; it is reported relative to sum |term_i| / denominator. Gradients: one bound per element, which
stays at the scale of the cancelling parts where the element itself cancels (an isotropic row's entropy gradient is 0 = a - a).
The reference's own fp32 run must stay inside factor 1 of every bound on every fixture (tests/test_reg_cases.py); the HIP
kernels get KERNEL_FACTOR = 2, the factor the optimizer tests use.

Decisions. erank's gradient jumps where t = -log(e + 1e-5) crosses 0 (the clip) and where the two smallest s2 swap (amin).
A row may be excused from the g_scaling comparison only if the float64 run puts it inside the derived fp32 error of that
decision (|t| <= d_t, or two distinct smallest s2 closer than the sum of their errors), and at most MAX_EXCUSED of the rows
of a case. The scalar terms are continuous there and get no excusal.
"""
import math
import os

import numpy as np
import torch

U = 2.0 ** -24
FN = 4 * U
KERNEL_FACTOR = 2.0
MAX_EXCUSED = 1e-3
RETIRED_LOGIT = -1.0e30  # eogs2_amd.optim.RETIRED_LOGIT (asserted equal in tests/test_reg_api.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reg")
GAUSS_FIXTURES = ("gauss_mix", "gauss_radii_all_zero", "gauss_isotropic_init")
IMAGE_FIXTURES = ("image_24x37", "image_2x2", "image_flat_9x16")
MUTANTS_GAUSS = ("no_log_eps", "no_s2_eps", "amin_first", "clip_drop_equal", "P_for_N0")
MUTANTS_IMAGE = ("sign0_is_1", "tv_denominators_swapped")


def sum_depth(n):
    n = max(int(n), 2)
    return 4 * 2 ** max(4, -(-math.ceil(math.log2(n)) // 4)) + 16


# ---- seeded inputs --------------------------------------------------------------------------------------------------
def log_scales(kind, n, gen):
    """[n, 3] float32 log-scales of one population."""
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    if kind == "isotropic":  # the kNN initialisation: three equal scales, exact ties of amin
        l = u(-7.0, -1.5, n, 1).repeat(1, 3)
    elif kind == "two_small":  # one long axis, the two short ones exactly equal
        big = u(-3.0, -1.0, n, 1)
        small = big - u(0.3, 4.0, n, 1)
        l = torch.cat([big, small, small], 1)
    elif kind == "disk":  # two long axes of similar length, one thin: the effective rank is near 2, where the clip sits
        a = u(-3.5, -1.0, n, 1)
        l = torch.cat([a + u(-0.6, 0.6, n, 1), a + u(-0.6, 0.6, n, 1), a - u(1.5, 6.0, n, 1)], 1)
    elif kind == "needle":  # one long axis, two distinct short ones, down to where the +1e-5 of s2 dominates
        a = u(-3.0, -0.5, n, 1)
        l = torch.cat([a, a - u(2.5, 6.0, n, 1), a - u(2.5, 6.0, n, 1)], 1)
    elif kind == "loguniform":
        l = u(-8.0, 0.0, n, 3)
    else:
        raise ValueError(kind)
    if kind != "isotropic":
        idx = (torch.arange(3)[None, :] + torch.arange(n)[:, None]) % 3  # no axis is special
        l = torch.gather(l, 1, idx)
    return l.to(torch.float32)


def opacity_logits(n, gen):
    """[n, 1] float32 logits spread over +-12, every 16th exactly 0."""
    o = (24.0 * torch.rand(n, 1, generator=gen, dtype=torch.float64) - 12.0).to(torch.float32)
    o[::16] = 0.0
    if n >= 4:
        o[1], o[2] = 12.0, -12.0
    return o


def radii_mix(n, gen):
    r = torch.randint(0, 40, (n,), generator=gen, dtype=torch.int32)
    r[torch.rand(n, generator=gen) < 0.4] = 0
    return r


def altitude_image(H, W, gen, flat=True):
    """An altitude render: smooth relief plus noise, with patches that are exactly flat (the background value wherever
    nothing is listed) and a plateau."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    a = 30.0 * torch.sin(x / 7.0) * torch.cos(y / 5.0) + 2.0 * torch.randn(H, W, generator=gen, dtype=torch.float64)
    a = a.to(torch.float32)
    if flat and H >= 8 and W >= 8:
        a[: H // 3, : W // 2] = -12.5
        a[H // 2: H // 2 + 3, W // 2:] = 7.25
        a[-1, :] = a[-2, :]
    return a


def accumulated_image(H, W, gen):
    a = torch.rand(H, W, generator=gen, dtype=torch.float64).to(torch.float32)
    a.view(-1)[::7] = 1.0
    a.view(-1)[3::11] = 0.0
    return a


# ---- the restatement ------------------------------------------------------------------------------------------------
def erank_rows(l, mutant=None):
    """main_loss.py:27-32 on log-scales: (per-row term, t) with t the clipped quantity -log(e + 1e-5)."""
    s2 = torch.exp(l).square()
    if mutant != "no_s2_eps":
        s2 = s2 + 1e-5
    S = s2.sum(dim=1, keepdim=True)
    q = s2 / S
    erankm1 = torch.expm1(-(q * torch.log(q if mutant == "no_log_eps" else q + 1e-6)).sum(dim=1))
    t = torch.log(erankm1 + 1e-5).mul(-1)
    clipped = torch.where(t > 0, t, torch.zeros_like(t)) if mutant == "clip_drop_equal" else t.clip(min=0.0)
    mn = s2.min(dim=1).values if mutant == "amin_first" else s2.amin(1)  # (min(dim) hands its gradient to one index)
    return clipped + mn.sqrt(), t


def restate_gauss(opacity, log_scales_, radii, n_init, upstream, dtype, mutant=None):
    """The three Gaussian-space terms and the gradient of upstream[k] * term_k with respect to the raw parameters, by
    autograd over the reference's torch ops in `dtype`. Rows at RETIRED_LOGIT are taken out first (the reference is run
    on the model without them) and get zero gradient. Returns numpy arrays under the fixture's keys."""
    alive = opacity.reshape(-1) > 0.5 * RETIRED_LOGIT
    o = opacity[alive].to(dtype).requires_grad_(True)
    l = log_scales_[alive].to(dtype).requires_grad_(True)
    vis = radii[alive] > 0
    den = o.shape[0] if mutant == "P_for_N0" else n_init
    sig = torch.sigmoid(o).squeeze(1)
    L_op = sig.sum() / den
    L_rad = sig[vis].sum() / den
    L_er = erank_rows(l, mutant)[0].mean()
    up = [float(v) for v in upstream]
    g_op, = torch.autograd.grad(up[0] * L_op, o, retain_graph=True)
    g_rad, = torch.autograd.grad(up[1] * L_rad, o)
    g_sc, = torch.autograd.grad(up[2] * L_er, l)

    def full(g):
        out = torch.zeros((opacity.shape[0],) + tuple(g.shape[1:]), dtype=dtype)
        out[alive] = g
        return out.numpy()

    return {"L_opacity": L_op.detach().numpy(), "L_opacity_radii": L_rad.detach().numpy(), "L_erank": L_er.detach().numpy(),
            "g_opacity_op": full(g_op), "g_opacity_radii": full(g_rad), "g_scaling": full(g_sc)}


def restate_image(alt, acc, upstream, dtype, mutant=None):
    a = alt.to(dtype).requires_grad_(True)
    c = acc.to(dtype).requires_grad_(True)
    H, W = a.shape
    d1 = a[..., 1:, :] - a[..., :-1, :]
    d2 = a[..., :, 1:] - a[..., :, :-1]
    ab = (lambda d: torch.where(d >= 0, d, -d)) if mutant == "sign0_is_1" else torch.abs
    if mutant == "tv_denominators_swapped":
        tv = 0.5 * (ab(d1).sum() / (H * (W - 1)) + ab(d2).sum() / ((H - 1) * W))
    else:
        tv = 0.5 * (ab(d1).mean() + ab(d2).mean())
    ao = (1.0 - c).mean()
    g_a, = torch.autograd.grad(float(upstream[0]) * tv, a)
    g_c, = torch.autograd.grad(float(upstream[1]) * ao, c)
    return {"L_TV_altitude": tv.detach().numpy(), "L_accumulated_opacity": ao.detach().numpy(), "g_altitude": g_a.numpy(),
            "g_accumulated_opacity": g_c.numpy()}


# ---- the derived bounds ---------------------------------------------------------------------------------------------
def gauss_bounds(opacity, log_scales_, radii, n_init, upstream):
    """Bounds on |fp32 - float64| of every output of restate_gauss (same keys; scalars and per-element arrays, float64),
    "scale:<key>" = sum |term_i| / denominator of the scalars, and "excusable" = the rows whose clip or amin decision the
    float64 run puts inside its fp32 error."""
    f8 = torch.float64
    alive = opacity.reshape(-1) > 0.5 * RETIRED_LOGIT
    n = int(alive.sum())
    D = sum_depth(n)
    up = [abs(float(v)) for v in upstream]
    o = opacity[alive].to(f8).reshape(-1)
    vis = (radii[alive] > 0).to(f8)
    # sigmoid = 1 / (1 + exp(-o))
    z = torch.exp(-o)
    dz = FN * z
    d = 1 + z
    dd = dz + U * d
    sg = 1 / d
    dsg = sg * (dd / d + U)
    out = {}
    for key, m in (("L_opacity", torch.ones_like(vis)), ("L_opacity_radii", vis)):
        scale = float((sg * m).sum()) / n_init
        out["scale:" + key] = scale
        out[key] = float((dsg * m).sum()) / n_init + (D + 1) * U * scale  # the sum, the division by n_init
    # d/do = c (1 - sg) sg, c = upstream / n_init (one rounding); 1 - sg cancels for large logits
    w = 1 - sg
    dw = dsg + U * w
    for key, m, u_ in (("g_opacity_op", torch.ones_like(vis), up[0]), ("g_opacity_radii", vis, up[1])):
        c = u_ / n_init
        g = c * w * sg
        b = m * (c * (dw * sg + w * dsg) + 3 * U * g)
        out[key] = _full(b, alive).reshape(-1, 1)
    # erank, forward (main_loss.py:27-32)
    l = log_scales_[alive].to(f8)
    s = torch.exp(l)
    ds = FN * s
    sq = s * s
    s2 = sq + 1e-5
    ds2 = 2 * s * ds + U * sq + U * s2
    S = s2.sum(1, keepdim=True)
    dS = ds2.sum(1, keepdim=True) + 2 * U * S
    q = s2 / S
    dq = q * (ds2 / s2 + dS / S + U)
    a = q + 1e-6
    da = dq + U * a
    lq = torch.log(a)
    dlq = da / a + FN * lq.abs()
    p = q * lq
    dp = lq.abs() * dq + q * dlq + U * p.abs()
    h = p.sum(1)
    dh = dp.sum(1) + 2 * U * p.abs().sum(1)
    e = torch.expm1(-h)
    de = (e + 1) * dh + FN * e.abs()
    x = e + 1e-5
    dx = de + U * x
    t = -torch.log(x)
    dt = dx / x + FN * t.abs()
    active = t >= 0
    dc = torch.where(t > -dt, dt, torch.zeros_like(dt))
    mn, arg = s2.min(1)
    dmn = ds2.gather(1, arg[:, None]).squeeze(1)
    r = mn.sqrt()
    dr = dmn / (2 * r) + U * r
    row = t.clamp(min=0) + r
    drow = dc + dr + U * row
    scale = float(row.abs().sum()) / n
    out["scale:L_erank"] = scale
    out["L_erank"] = float(drow.sum()) / n + (D + 1) * U * scale
    # erank, backward, in autograd's order: c = upstream / n
    c = up[2] / n
    dcu = U * c
    ge = c / x
    dge = ge * (dx / x + U) + dcu / x
    gh = ge * (e + 1)
    dgh = (e + 1) * dge + ge * (de + U * (e + 1)) + U * gh
    dk = q / a
    ddk = dk * (dq / q + da / a + U)
    b = lq + dk
    db = dlq + ddk + U * b.abs()
    gq = gh[:, None] * b
    dgq = b.abs() * dgh[:, None] + gh[:, None] * db + 3 * U * gq.abs()
    tau = gq * s2
    dtau = s2 * dgq + gq.abs() * ds2 + U * tau.abs()
    T = tau.sum(1, keepdim=True)
    dT = dtau.sum(1, keepdim=True) + 2 * U * tau.abs().sum(1, keepdim=True)
    gS = -T / (S * S)
    dgS = dT / (S * S) + gS.abs() * (2 * dS / S + 2 * U)
    A = gq / S
    dA = dgq / S + A.abs() * (dS / S + U)
    gs2 = torch.where(active[:, None], A + gS, torch.zeros_like(A))
    dgs2 = torch.where(active[:, None], dA + dgS + U * (A.abs() + gS.abs()), torch.zeros_like(A))
    tie = s2 == mn[:, None]
    ties = tie.sum(1, keepdim=True).to(f8)
    gm = c * 0.5 / r[:, None] / ties
    dgm = gm * (dr / r)[:, None] + 4 * U * gm
    gs2 = gs2 + tie * gm
    dgs2 = dgs2 + tie * (dgm + U * gs2.abs())
    gl = gs2 * 2 * s * s
    dgl = 2 * sq * dgs2 + gl.abs() * (2 * ds / s + 2 * U)
    out["g_scaling"] = _full(dgl, alive)
    # decisions inside their fp32 error
    srt, order = s2.sort(1)
    gap = srt[:, 1] - srt[:, 0]
    dsrt = ds2.gather(1, order)
    near_tie = (gap > 0) & (gap <= dsrt[:, 0] + dsrt[:, 1])
    out["excusable"] = _full((t.abs() <= dt) | near_tie, alive).astype(bool)
    out["t"] = _full(t, alive)
    return out


def _full(v, alive):
    full = torch.zeros((alive.shape[0],) + tuple(v.shape[1:]), dtype=v.dtype)
    full[alive] = v
    return full.numpy()


def image_bounds(alt, acc, upstream):
    f8 = torch.float64
    a, c = alt.to(f8), acc.to(f8)
    H, W = a.shape
    up = [abs(float(v)) for v in upstream]
    sv = float((a[1:, :] - a[:-1, :]).abs().sum()) / ((H - 1) * W)
    sh = float((a[:, 1:] - a[:, :-1]).abs().sum()) / (H * (W - 1))
    tv = 0.5 * (sv + sh)
    D = sum_depth(H * W)
    out = {"scale:L_TV_altitude": tv, "L_TV_altitude": (1 + D + 1 + 1 + 1) * U * tv}  # difference, sum, division, add, halving
    ao = float((1 - c).abs().sum()) / (H * W)
    out["scale:L_accumulated_opacity"] = ao
    out["L_accumulated_opacity"] = (1 + D + 1) * U * ao
    cv, ch = 0.5 * up[0] / ((H - 1) * W), 0.5 * up[0] / (H * (W - 1))
    # each of the at most four +-cv / +-ch parts carries the three roundings of its coefficient, three additions join them
    out["g_altitude"] = np.full((H, W), 6 * U * (2 * cv + 2 * ch))
    out["g_accumulated_opacity"] = np.full((H, W), 3 * U * up[1] / (H * W))
    return out


# ---- fixtures and comparison ----------------------------------------------------------------------------------------
GAUSS_KEYS = ("L_opacity", "L_opacity_radii", "L_erank", "g_opacity_op", "g_opacity_radii", "g_scaling")
IMAGE_KEYS = ("L_TV_altitude", "L_accumulated_opacity", "g_altitude", "g_accumulated_opacity")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def gauss_inputs(fx):
    return (torch.from_numpy(fx["opacity"]), torch.from_numpy(fx["log_scales"]), torch.from_numpy(fx["radii"]), float(fx["n_init"]),
            fx["upstream"])


def image_inputs(fx):
    return torch.from_numpy(fx["altitude"]), torch.from_numpy(fx["accumulated_opacity"]), fx["upstream"]


def compare(got, want64, bounds, keys, factor, what, excuse_rows=False, log=None):
    """Asserts |got[k] - want64[k]| <= factor * bounds[k] for every key (every element of an array); rows of g_scaling
    flagged `excusable` are left out when `excuse_rows`, at most MAX_EXCUSED of them. Returns {key: worst error / bound}."""
    worst = {}
    for k in keys:
        g = np.asarray(got[k], dtype=np.float64)
        w = np.asarray(want64[k], dtype=np.float64)
        b = factor * np.asarray(bounds[k], dtype=np.float64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.isfinite(g).all(), (what, k, "non-finite")
        err = np.abs(g - w)
        if k == "g_scaling" and excuse_rows:
            ex = bounds["excusable"]
            assert ex.mean() <= MAX_EXCUSED, (what, "excused rows", int(ex.sum()), ex.size)
            err, b = err[~ex], b[~ex]
        ratio = np.where(err > 0, err / np.maximum(b, 1e-300), 0.0)
        worst[k] = float(ratio.max()) if ratio.size else 0.0
        line = f"{what} {k}: worst error {float(err.max()) if err.size else 0.0:.3e} = {worst[k]:.3f} x the bound (factor {factor:g})"
        if ("scale:" + k) in bounds:
            line += f"; bound {float(b):.3e} = {float(b) / max(bounds['scale:' + k], 1e-300) / U:.1f} U of the term's scale"
        if log is not None:
            log.append(line)
        print(line)
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, (what, bad)
    return worst


def rejects(mut, want64, bounds, keys, factor=KERNEL_FACTOR):
    """True if the mutant's outputs leave factor x the bound somewhere (no rows excused)."""
    for k in keys:
        err = np.abs(np.asarray(mut[k], dtype=np.float64) - np.asarray(want64[k], dtype=np.float64))
        if (err > factor * np.asarray(bounds[k], dtype=np.float64)).any():
            return True
    return False
