"""Shared helpers and the case module of the shade tests (include/eogs_shade.h: render pipeline, masked resample losses,
translucent-shadow regulariser): fixture loading, one driver that runs either implementation, the named edge cases as
seeded numpy inputs, and the per-element criterion.

The criterion (DESIGN.md §8, f2 image chain). Every output element is held to

    |got - ref64| <= HI * (k * 2^-24 * (sum of the magnitudes of the terms the element is formed from)) + half an ulp of ref64

computed in float64 from the inputs. `ref64` is oracle/shade_oracle.py in float64, whose constants (0.4, -1e-2, 0.30,
0.05, 0.95) are the fp32 values torch uses on an fp32 tensor, so it is the exact value of the fp32 program's formula. `k`
counts the roundings on the longest path of the kernel's formula as csrc/shade.hip writes it (-ffp-contract=off: every
product and sum rounds once, 2^-24 relative each); each derivation stands next to its bound. HI = 1 + 2^-10 covers the
products of two such errors (24 * 2^-24 squared is below 2^-38). expf and log2f: ROCm ships no statement of the device
library's error on this installation, so E_EXP / E_LOG2 come from a measurement on the CPU (torch's fp32 exp / log2
against float64 over the cases' argument ranges: 0.56 and 0.50 ulp, `measured_libm_ulp`, asserted in
tests/test_shade_oracle.py), rounded up to 1 ulp. No bound was fitted to the kernels' results.
NaN, +inf and -inf must sit at exactly the reference's elements; where asked, a zero carries the reference's sign.
"""
import glob
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixtures(prefix):
    return sorted(glob.glob(os.path.join(GOLD, f"shade_{prefix}*.npz")))


def load(path):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def matrix_of(fx, dtype, dev):
    kind = str(fx["kind"])
    if kind == "cc":
        M = np.concatenate([fx["weight"].reshape(3, 3), fx["bias"].reshape(3, 1)], axis=1)
    elif kind == "exposure":
        M = fx["exposure"][0]
    else:
        M = np.eye(3, 4, dtype=np.float32)
    return torch.tensor(M, dtype=dtype, device=dev)


def expected_matrix_grad(fx):
    kind = str(fx["kind"])
    if kind == "cc":
        return np.concatenate([fx["g_weight"].reshape(3, 3), fx["g_bias"].reshape(3, 1)], axis=1)
    if kind == "exposure":
        return fx["g_exposure"][0]
    return None


def run_shade(fn, fx, dtype, dev):
    """fn(raw, alt_diff|None, M, inshadow) -> (cc, shaded, shadow); returns outputs and gradients as float64 numpy."""
    t = lambda a: torch.tensor(a, dtype=dtype, device=dev)
    raw = t(fx["raw"]).requires_grad_(True)
    M = matrix_of(fx, dtype, dev).requires_grad_(True)
    has = "alt_diff" in fx
    alt = t(fx["alt_diff"]).requires_grad_(True) if has else None
    ins = t(fx["inshadow"]).requires_grad_(True)
    cc, shaded, shadow = fn(raw, alt, M, ins if has else None)
    loss = (shaded * t(fx["g_shaded"])).sum() + (cc * t(fx["g_cc"])).sum()
    if has:
        loss = loss + (shadow * t(fx["g_shadow"])).sum()
    loss.backward()
    n = lambda x: None if x is None else x.detach().double().cpu().numpy()
    out = dict(cc=n(cc), shaded=n(shaded), g_raw=n(raw.grad), g_M=n(M.grad))
    if has:
        out.update(shadow=n(shadow), g_alt_diff=n(alt.grad), g_inshadow=n(ins.grad))
    return out


def close(a, b, tol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max() / scale
    assert err <= tol, f"{what}: max |diff| / max |ref| = {err:.3e} > {tol}"


# ---- the per-element criterion ---------------------------------------------------------------------------------------
U = 2.0 ** -24  # one fp32 rounding, relative
HI = 1.0 + 2.0 ** -10  # products of two rounding errors
E_EXP = 1.0  # ulp, expf: measured_libm_ulp() rounded up
E_LOG2 = 1.0  # ulp, log2f: likewise
F04 = float(np.float32(0.4))  # the constants as the fp32 program holds them
CLIP_LO, CLIP_HI = float(np.float32(0.05)), float(np.float32(0.95))
ST, SMAXBLK = 256, 1024  # csrc/shade.hip: threads per workgroup, workgroups per launch


def measured_libm_ulp(n=400_001):
    """Largest error, in fp32 ulps, of torch's fp32 exp over [-104, 0] (0.4 * alt_diff down to where s underflows) and log2
    over [0.05, 0.95] (the clip range, which 1 - b shares), against float64 on this CPU."""
    out = {}
    for name, f32, f64, lo, hi in (("exp", torch.exp, np.exp, -104.0, 0.0), ("log2", torch.log2, np.log2, CLIP_LO, CLIP_HI)):
        x = np.linspace(lo, hi, n).astype(np.float32)
        ref = f64(x.astype(np.float64))
        got = f32(torch.tensor(x)).numpy().astype(np.float64)
        out[name] = float((np.abs(got - ref) / spacing32(ref)).max())
    return out


def spacing32(x):
    """fp32 ulp at |x| (2^-149 at and below the subnormals), as float64; NaN / inf where x is."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def chain(n):
    """Longest serial chain of fp32 additions a term of a sum over n pixels passes through, read off csrc/shade.hip: a lane's
    grid-stride trips ceil(n / (blocks * 256)); wg_sum = 6 butterfly steps + 3 adds over the four waves; then
    shade_reduce_kernel: ceil(blocks / 256) trips per lane, 6 + 3 again."""
    blocks = min(SMAXBLK, max(1, -(-n // ST)))
    return -(-n // (blocks * ST)) + 9 + -(-blocks // ST) + 9


def check(got, ref, bound, what, signed_zero=False):
    """Non-finite elements exactly where the reference has them (NaN, +inf, -inf each); every other element inside its own
    bound; with signed_zero, an exact zero of the reference is a zero of the same sign."""
    got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    for name, f in (("NaN", np.isnan), ("+inf", lambda x: x == np.inf), ("-inf", lambda x: x == -np.inf)):
        a, b = f(got), f(ref)
        assert np.array_equal(a, b), (f"{what}: {name} pattern differs at {np.argwhere(a != b)[:5].tolist()} "
                                      f"({int(a.sum())} got, {int(b.sum())} expected)")
    fin = np.isfinite(ref)
    assert np.isfinite(bound[fin]).all(), f"{what}: no finite bound for a finite reference element"
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    over = err > np.where(fin, bound, 0.0)
    if over.any():
        i = np.unravel_index(np.argmax(np.where(over, err / np.maximum(np.where(fin, bound, 1.0), 1e-300), 0.0)), ref.shape)
        raise AssertionError(f"{what}: {int(over.sum())} of {ref.size} elements outside their bound; worst at {tuple(int(x) for x in i)}: "
                             f"got {got[i]!r}, ref {ref[i]!r}, |diff| {err[i]:.3e} > bound {bound[i]:.3e}")
    if signed_zero:
        z = ref == 0.0
        assert (got[z] == 0.0).all(), f"{what}: nonzero where the reference is exactly zero"
        bad = np.signbit(got) != np.signbit(ref)
        assert not (bad & z).any(), f"{what}: sign of zero differs at {np.argwhere(bad & z)[:5].tolist()}"


def _half(ref):
    return 0.5 * spacing32(ref)


def shade_bounds(fx, ref):
    """Bounds of every output of run_shade, from the inputs in float64. Names as in shade_fwd_kernel / shade_bwd_kernel."""
    f = lambda k: np.asarray(fx[k], np.float64)
    M = matrix_of(fx, torch.float64, "cpu").numpy()
    raw = f("raw").reshape(3, -1)
    n = raw.shape[1]
    g, gc = f("g_shaded").reshape(3, -1), f("g_cc").reshape(3, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        # c = ((M0 r0 + M1 r1) + M2 r2) + M3: the first product is rounded once and passes three additions -> k = 4
        T_cc = sum(np.abs(M[:, k : k + 1] * raw[k]) for k in range(3)) + np.abs(M[:, 3:4])
        B = {"cc": 4 * U * T_cc}
        if "alt_diff" in fx:
            d = f("alt_diff").reshape(-1)
            ins = f("inshadow").reshape(3, 1)
            a = F04 * np.where(d > 0, 0.0, d)  # NaN kept
            s = np.exp(a)
            # s = expf(fl(0.4f d)): the product's rounding moves s by |a| 2^-24 s, expf itself by E_EXP ulp of s
            es = np.where(s > 0, np.abs(a) * U * s, 0.0) + E_EXP * spacing32(s)
            es = np.where(np.isnan(d), np.nan, es)
            oms = np.abs(1.0 - s)
            # shaded = s c + ((1 - s) ins) c, terms T_A = s T_cc, T_B = |1 - s| |ins| T_cc, and s's error reaches both:
            #   s c:             es |c| + (product, final sum: 2) |s c| + s (4 T_cc)                  <= es T_cc + 6 T_A
            #   ((1-s) ins) c:   es |ins c| + (1 - s, two products, final sum: 4) |B| + |(1-s) ins| (4 T_cc) <= es |ins| T_cc + 8 T_B
            B["shadow"] = es
            B["shaded"] = es * (1 + np.abs(ins)) * T_cc + U * (6 * s * T_cc + 8 * oms * np.abs(ins) * T_cc)
            # f = s + (1 - s) ins: es; (es + 2^-24 |1-s|) |ins| and the product's rounding; the sum's rounding
            Tf = s + oms * np.abs(ins)
            Ef = es * (1 + np.abs(ins)) + U * (s + 3 * oms * np.abs(ins))
            # gcc = g f + g_cc: f's error, the product's rounding, the sum's rounding
            Tgcc = np.abs(g) * Tf + np.abs(gc)
            Egcc = np.abs(g) * Ef + U * np.abs(g) * Tf + U * Tgcc
            # gs = ((g_shadow + t0) + t1) + t2, t_k = (g_k c_k)(1 - ins_k), T_k = |g_k| T_cc_k |1 - ins_k|: c's 4, three roundings in
            # t_k, at most three additions -> 10 per term; g_shadow passes three additions
            gsh = np.abs(f("g_shadow").reshape(-1))
            Tk = (np.abs(g) * T_cc * np.abs(1.0 - ins)).sum(0)
            Tgs, Egs = Tk + gsh, U * (10 * Tk + 3 * gsh)
            # g_alt = (gs 0.4f) s where d <= 0: gs's error, s's error, two products; exactly 0 elsewhere (d > 0 and NaN)
            B["g_alt_diff"] = np.where(d <= 0, F04 * (np.where(s > 0, s * Egs, 0.0) + Tgs * es + 2 * U * Tgs * s), 0.0)
            # sum_p (g (1 - s)) c: (1 - s) carries es + 2^-24 |1-s|, two products, c's 4 -> |g| T_cc (es + 7 2^-24 |1-s|) per term
            B["g_inshadow"] = (np.abs(g) * T_cc * (es + 7 * U * oms)).sum(1) + chain(n) * U * (np.abs(g) * oms * T_cc).sum(1)
        else:
            B["shaded"] = B["cc"]
            Tgcc = np.abs(g) + np.abs(gc)  # gcc = g + g_cc: one rounding
            Egcc = U * Tgcc
        # g_raw_k = (M0k gcc0 + M1k gcc1) + M2k gcc2: each gcc's error times |M|; a product and two additions -> 3
        B["g_raw"] = np.stack([sum(np.abs(M[c, k]) * (Egcc[c] + 3 * U * Tgcc[c]) for c in range(3)) for k in range(3)])
        # g_M[c][j] = sum_p gcc_c r_j (j < 3: one more product), g_M[c][3] = sum_p gcc_c; every term then passes chain(n) additions
        r1 = np.concatenate([np.abs(raw), np.ones((1, n))])
        prod = np.concatenate([np.ones((3, 1)), np.zeros((1, 1))])  # the product's rounding, absent in column 3
        B["g_M"] = np.stack([[(Egcc[c] * r1[j] + prod[j, 0] * U * Tgcc[c] * r1[j]).sum() + chain(n) * U * (Tgcc[c] * r1[j]).sum()
                              for j in range(4)] for c in range(3)])
        out = {}
        for k, b in B.items():
            out[k] = HI * b.reshape(np.shape(ref[k])) + _half(ref[k])
    return out


def check_shade(got, ref, fx, what):
    B = shade_bounds(fx, ref)
    for k in ref:
        check(got[k], ref[k], B[k], f"{what}: {k}", signed_zero=(k == "g_alt_diff"))


# ---- shadow pipeline cases -------------------------------------------------------------------------------------------
# 513 x 513 = 263,169 pixels: one more than 1024 workgroups x 256 lanes and then some, the last 1,025 take a second trip
SIZES = [(1, 1), (1, 257), (255, 1), (513, 513)]
PIPE_CASES = [(kind, H, W, sh) for kind in ("cc", "exposure", "identity") for sh in (True, False) for H, W in SIZES]
# 0, -0, the subnormals next to 0, ordinary shadow, s subnormal (e^-100), s == 0, both infinities
PLANTS = np.array([0.0, -0.0, -1e-45, 1e-45, -30.0, -250.0, -1e4, np.inf, -np.inf], np.float32)
NPLANT = len(PLANTS) + 2  # + a NaN altitude difference, + a NaN in one channel of raw
# the ones the reference's own modules ran (tests/golden/make_golden_shade.py -> shade_edgepipe_*.npz), a few KB each
GOLDEN_PIPE = [("cc", 3, 11, True, dict(nan=True)), ("exposure", 1, 33, True, dict(nan=True)), ("identity", 31, 1, True, dict(nan=False)),
               ("cc", 1, 29, False, dict(nan=True)), ("exposure", 1, 1, True, dict(plant=5)), ("identity", 1, 1, True, dict(plant=9)),
               ("cc", 1, 1, True, dict(plant=6))]


def pipeline_case(kind, H, W, shadow, nan=False, plant=None):
    """Inputs in the fixtures' layout. Sizes with room carry every planted altitude difference in their first and their last
    pixels (the last ones ride the second grid-stride trip at 513 x 513) and, with `nan`, a NaN altitude difference and a
    NaN in raw's channel 1 at two more pixels; a 1 x 1 image carries plant number `plant` (< NPLANT) alone.
    cc: row 1 of the matrix is zero, bias included; exposure: the in-shadow tint lies outside [0, 1]."""
    rng = np.random.default_rng([("cc", "exposure", "identity").index(kind), H, W, int(shadow)])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    n = H * W
    fx = dict(kind=np.array(kind), raw=rng.random((3, H, W), dtype=np.float32), g_shaded=f(3, H, W), g_cc=f(3, H, W))
    if kind == "cc":
        w = (np.eye(3, dtype=np.float32) + 0.2 * f(3, 3))
        b = 0.1 * f(3)
        w[1], b[1] = 0.0, 0.0
        fx.update(weight=w.reshape(3, 3, 1, 1), bias=b)
    elif kind == "exposure":
        fx["exposure"] = (np.eye(3, 4, dtype=np.float32) + 0.2 * f(3, 4))[None]
    fx["inshadow"] = np.array([-0.3, 1.7, 0.4], np.float32) if kind == "exposure" else (0.05 + 0.3 * rng.random(3)).astype(np.float32)
    alt = 2.0 * f(H, W)
    raw = fx["raw"]
    if n == 1:
        assert plant is not None and not nan
        if plant < len(PLANTS):
            alt.flat[0] = PLANTS[plant]
        elif plant == len(PLANTS):
            alt.flat[0] = np.nan
        else:
            raw[1].flat[0] = np.nan
    else:
        assert n >= 2 * len(PLANTS) + 4
        alt.flat[: len(PLANTS)] = PLANTS
        alt.flat[n - len(PLANTS) :] = PLANTS
        if nan:
            alt.flat[n // 2] = np.nan
            raw[1].flat[n // 2 + 1] = np.nan
    if shadow:
        fx.update(alt_diff=alt, g_shadow=f(H, W))
    return fx


# ---- masked resample losses ------------------------------------------------------------------------------------------
MLOSS_CASES = ["thresholds", "one_pixel", "empty", "full513", "nonfinite_out", "alt_inf_in", "rgb_nan_in", "rgb_inf_in", "uv_nan",
               "image_1x1_in", "image_1x1_out"]
MLOSS_MODES = ["sun", "random"]


def mloss_mask(fx):
    """The mask as the fp32 program takes it (shadow.py:40, main_loss.py:153-155)."""
    d, uv = fx["alt_diff"].astype(np.float32), fx["uv"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        ok = d > np.float32(-1e-2) if str(fx["mode"]) == "sun" else np.abs(d) < np.float32(0.30)
        return ok & (np.abs(uv) < 1).all(-1)


def _nbrs(t):
    t = np.float32(t)
    return [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))]


def mloss_case(name, mode):
    """The upstream pair has a negative entry: the reference's `grad * mask` then leaves -0 outside the mask."""
    H, W = (513, 513) if name == "full513" else (1, 1) if name.startswith("image_1x1") else (7, 9)
    rng = np.random.default_rng([MLOSS_CASES.index(name), MLOSS_MODES.index(mode)])
    a, b = rng.random((3, H, W), dtype=np.float32), rng.random((3, H, W), dtype=np.float32)
    alt = (0.2 * rng.standard_normal((H, W))).astype(np.float32)
    uv = (1.3 * (2 * rng.random((H, W, 2)) - 1)).astype(np.float32)
    inside = np.array([0.25, -0.5], np.float32)
    ok_alt = np.float32(0.001)
    if name == "thresholds":
        # the altitude decision at its constant and the fp32 neighbours (both signs for |d| < 0.30f)
        ts = _nbrs(-1e-2) if mode == "sun" else _nbrs(0.30) + [-x for x in _nbrs(0.30)]
        for i, t in enumerate(ts):
            alt[0, i], uv[0, i] = t, inside
        # |uv.x|, |uv.y| at 1 and its neighbours, both signs
        for i, t in enumerate(_nbrs(1.0)):
            for r, (sign, comp) in enumerate(((1, 0), (-1, 0), (1, 1), (-1, 1))):
                alt[1 + r, i] = ok_alt
                uv[1 + r, i] = inside
                uv[1 + r, i, comp] = sign * t
        # exact rgb ties and a zero altitude difference inside the mask: sign(0) = 0
        alt[5, :5], uv[5, :5] = ok_alt, inside
        alt[5, 0] = 0.0
        alt[5, 1] = -0.0
        b[:, 5, :5] = a[:, 5, :5]
    elif name in ("one_pixel", "empty"):
        uv = np.abs(uv) + 1.0
        if name == "one_pixel":
            alt[3, 4], uv[3, 4] = ok_alt, inside
    elif name == "full513":
        uv = (0.9 * (2 * rng.random((H, W, 2)) - 1)).astype(np.float32)
        alt = np.abs(alt) if mode == "sun" else (0.25 * (2 * rng.random((H, W)) - 1)).astype(np.float32)
    elif name == "nonfinite_out":
        out = np.array([1.5, 0.0], np.float32)
        for i, v in enumerate((np.nan, np.inf, -np.inf)):
            alt[0, i], uv[0, i] = v, out  # outside the view
            a[i, 1, i], uv[1, i] = v, out
            b[i, 2, i], uv[2, i] = v, out
        # masked out by the altitude test itself, inside the view
        for i, v in enumerate((np.nan, -np.inf) if mode == "sun" else (np.nan, np.inf, -np.inf)):
            alt[3, i], uv[3, i] = v, inside
    elif name == "alt_inf_in":  # sun only: +inf > -1e-2
        alt[2, 2], uv[2, 2] = np.inf, inside
    elif name in ("rgb_nan_in", "rgb_inf_in"):
        alt[2, 2], uv[2, 2] = ok_alt, inside
        a[1, 2, 2] = np.nan if name == "rgb_nan_in" else np.inf
        if name == "rgb_inf_in":
            alt[4, 4], uv[4, 4] = ok_alt, inside
            b[0, 4, 4] = np.inf
    elif name.startswith("image_1x1"):  # the whole image is one pixel, inside the mask or (an empty mask) outside the view
        alt[0, 0], uv[0, 0] = np.float32(-0.004), inside if name.endswith("_in") else np.array([0.25, 1.5], np.float32)
    elif name == "uv_nan":
        alt[2, 2], alt[2, 3] = ok_alt, ok_alt
        uv[2, 2], uv[2, 3] = (np.nan, 0.0), (0.0, np.nan)
    return dict(mode=np.array(mode), rgb_a=a, rgb_b=b, alt_diff=alt, uv=uv, upstream=np.array([0.7, -1.3], np.float32))


def mloss_case_list():
    return [(n, m) for n in MLOSS_CASES for m in MLOSS_MODES if not (n == "alt_inf_in" and m == "random")]


def masked_out_zeroed(fx):
    """The same inputs with every non-finite altitude difference or rgb value at a masked-out pixel replaced by 0. Such a
    pixel is moved outside the view, so that the mask stays the one of the original inputs (a NaN altitude difference that
    masks itself out would be let in as a 0)."""
    m = mloss_mask(fx)
    out = {k: np.array(v, copy=True) for k, v in fx.items()}
    bad = ~np.isfinite(fx["alt_diff"]) | ~np.isfinite(fx["rgb_a"]).all(0) | ~np.isfinite(fx["rgb_b"]).all(0)
    sel = bad & ~m
    out["alt_diff"][sel & ~np.isfinite(fx["alt_diff"])] = 0.0
    for k in ("rgb_a", "rgb_b"):
        out[k][:, sel] = np.where(np.isfinite(fx[k][:, sel]), fx[k][:, sel], 0.0)
    out["uv"][sel] = 2.0
    assert np.array_equal(mloss_mask(out), m)
    return out


def check_mloss_elementwise(got, ref, fx, what):
    """L_alt = (sum |d|) / N: the terms are exact, each passes chain(n) additions and the division -> k = chain + 1.
    L_rgb's term (|a0-b0| + |a1-b1|) + |a2-b2|: a difference and two additions more -> k = chain + 4. The count is exact.
    Gradients are fl(upstream / N) times -1, 0 or 1: half an ulp, zeros with the reference's sign."""
    n = fx["alt_diff"].size
    for k, extra in (("L_alt", 1), ("L_rgb", 4)):
        r = np.float64(ref[k])
        check(np.float64(got[k]), r, HI * (chain(n) + extra) * U * np.abs(r) + _half(r), f"{what}: {k}")
    for k in ("g_alt_diff", "g_rgb_a", "g_rgb_b"):
        check(got[k], ref[k], _half(ref[k]), f"{what}: {k}", signed_zero=True)


# ---- translucent-shadow regulariser --------------------------------------------------------------------------------
TSHADOW_CASES = ["edges", "nan", "one", "big"]


def tshadow_case(name):
    rng = np.random.default_rng(TSHADOW_CASES.index(name))
    if name == "one":
        x = np.array([0.3], np.float32)
    elif name == "big":
        x = (1.2 * rng.random(262_145) - 0.1).astype(np.float32)  # one more than 1024 workgroups x 256 lanes
    else:
        x = np.array(_nbrs(0.05) + _nbrs(0.95) + [0.0, -0.0, 1.0, -0.5, 1.5, -1e-45, 0.5, 3e4] + list(rng.random(21)), np.float32)
        if name == "nan":
            x[17] = np.nan
    return dict(a=x, upstream=np.float32(2.5))


def run_tshadow(fn, fx, dtype, dev):
    a = torch.tensor(fx["a"], dtype=dtype, device=dev).requires_grad_(True)
    L = fn(a)
    (float(fx["upstream"]) * L).backward()
    return dict(L=float(L), g_a=a.grad.detach().double().cpu().numpy())


def check_tshadow(got, ref, fx, what):
    """term = x log2f(b) + (1 - x) log2f(1 - b), b = clip(x, 0.05f, 0.95f), so |log2| <= 4.33:
      x log2f(b):           log2f's E_LOG2 ulp (2 E_LOG2 2^-24 relative), the product                      -> (2 E_LOG2 + 1) |x log2 b|
      (1-x) log2f(1-b):     the same, 1 - x's rounding, and 1 - b's rounding, which moves log2 by 2^-24 / ln 2  -> (2 E_LOG2 + 2) |..| + |1-x| 2^-24 / ln 2
      their sum:            one more rounding on both
    then chain(n) additions, the product with fl(1 / n) (two roundings) and the sign.
    g = w (log2f(b) - log2f(1 - b)), w = fl(-upstream / n): the same errors of the two logarithms, their difference, w's rounding and
    the product -> |w| ((2 E_LOG2 + 3)(|log2 b| + |log2(1-b)|) + 1 / ln 2) 2^-24. (The clip's own derivative term is
    x/b - (1-x)/(1-b) = 1 - 1 exactly inside the range and is not taken outside it.)"""
    x = np.asarray(fx["a"], np.float64).reshape(-1)
    n, up = x.size, float(fx["upstream"])
    with np.errstate(invalid="ignore", over="ignore"):
        b = np.where(x < CLIP_LO, CLIP_LO, np.where(x > CLIP_HI, CLIP_HI, x))
        l1, l2 = np.abs(np.log2(b)), np.abs(np.log2(1 - b))
        t1, t2 = np.abs(x) * l1, np.abs(1 - x) * l2
        e_term = U * ((2 * E_LOG2 + 2) * t1 + (2 * E_LOG2 + 3) * t2 + np.abs(1 - x) / np.log(2))
        bl = (e_term.sum() + (chain(n) + 2) * U * (t1 + t2).sum()) / n
        bg = np.abs(up / n) * U * ((2 * E_LOG2 + 3) * (l1 + l2) + 1 / np.log(2))
    r = np.float64(ref["L"])
    check(np.float64(got["L"]), r, HI * bl + _half(r), f"{what}: L")
    rg = np.asarray(ref["g_a"], np.float64).reshape(-1)
    # no signed zero here: at x = 0.5 the reference adds two opposite terms (+0), the kernel multiplies w by a zero (sign of w)
    check(np.asarray(got["g_a"]).reshape(-1), rg, HI * bg + _half(rg), f"{what}: g_a")
