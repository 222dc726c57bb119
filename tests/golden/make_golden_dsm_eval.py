"""Generates tests/golden/dsm_eval/*.npz by running the REFERENCE's own `eval/dsmr.py` and the `mask_dsm` /
`dsm_pointwise_diff` / `Mae_Computer._compute_mae` of its `eval/eval_dsm.py` on seeded inputs. Only inputs and outputs are
stored; nothing of the reference is restated here.

    python tests/golden/make_golden_dsm_eval.py [case ...]

`numba` is a stub in sys.modules whose `jit` hands the function back, and the modules eval_dsm.py imports for its file I/O
and command line (hydra, iio, rasterio, tyro, clearml) are empty stubs: the functions driven here touch none of them.
numba types the reference's accumulators float64 whatever the image type, plain numpy would keep a float32 sum in float32:
so the reference's loops are always handed float64 copies of the images (an exact conversion), while every array they
store into keeps the image's own type.

Condition on the inputs: at every pyramid level of every registration the best NCC exceeds the runner-up by >= 1e-6, else
no fixture is written. Float64 sums in another order move an NCC by ~1e-12, so the integer shift cannot depend on the
summation order and the tests demand it exactly.

Registration cases store one float32 base terrain, two crop rectangles, the affine map of the second image's heights and
bit-packed NaN masks (tests/dsm_eval_cases.py `rebuild` makes the two images from them, here and in the tests).
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/: dsm_eval_cases, util
from make_golden_tsdf import REFROOT  # noqa: E402  (where the reference's sources are read from)

import dsm_eval_cases as C  # noqa: E402  (rebuild() and the seeded terrain only)

OUT = os.path.join(HERE, "dsm_eval")
MIN_GAP = 1e-6
MAX_BYTES = 314810  # the largest fixture committed before these


def load_ref():
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (a[0] if a and callable(a[0]) and not k else (lambda f: f))
    sys.modules["numba"] = numba
    for name in ("hydra", "iio", "rasterio", "tyro", "tyro.conf", "clearml", "clearml_utils", "utils", "utils.clearml_utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["tyro.conf"].FlagConversionOff = None
    sys.modules["tyro"].conf = sys.modules["tyro.conf"]
    sys.modules["hydra"].main = lambda **k: (lambda f: f)
    mods = []
    for name in ("dsmr", "eval_dsm"):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REFROOT, "eval", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod  # eval_dsm.py does `from dsmr import ...`
        spec.loader.exec_module(mod)
        mods.append(mod)
    dsmr, ev = mods
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    # what eval_dsm calls: the reference's own functions, handed float64 copies; apply_shift stores in the image's type
    ev.compute_shift = lambda ref, sec, scaling=True: dsmr.compute_shift(f64(ref), f64(sec), scaling)
    ev.apply_shift = lambda in_dsm, dx=0, dy=0, a=1, b=0, c=0, d=0: dsmr.apply_shift_(
        f64(in_dsm), np.zeros_like(np.asarray(in_dsm)), dx, dy, a, b, c, d)
    return dsmr, ev


def record_levels(dsmr):
    """Wraps dsmr.ncc and dsmr.compute_ncc (looked up in the module at call time) to keep every NCC of every level."""
    levels = []
    ncc0, cncc0 = dsmr.ncc, dsmr.compute_ncc

    def ncc(u, v, dx=0, dy=0):
        val = ncc0(u, v, dx, dy)
        levels[-1]["values"].append(val)
        return val

    def compute_ncc(u, v, irange, initdx, initdy):
        levels.append({"shape_u": u.shape, "shape_v": v.shape, "centre": (initdx, initdy), "irange": irange, "values": []})
        best = cncc0(u, v, irange, initdx, initdy)
        levels[-1]["winner"] = best
        return best

    dsmr.ncc, dsmr.compute_ncc = ncc, compute_ncc

    def restore():
        dsmr.ncc, dsmr.compute_ncc = ncc0, cncc0

    return levels, restore


def save(name, **arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez(path, **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{name}: {size} bytes"
    print(f"{name}: {size} bytes", flush=True)


def registration_inputs(H, W, shift, seed, extra=(0, 0), scale=0.97, offset=2.5, nan_share=0.05, nan_border=False):
    dx, dy = shift
    m = max(abs(dx), abs(dy)) + 2
    base = C.terrain(H + 2 * m + extra[0], W + 2 * m + extra[1], seed).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    un = rng.random((H, W)) < nan_share
    vn = rng.random((H + extra[0], W + extra[1])) < nan_share
    if nan_border:
        un[0, :] = True
        un[:, -1] = True
    # v[j + dy][i + dx] pairs with u[j][i]
    return {"base": base, "u_rect": np.array([m, m, H, W]), "v_rect": np.array([m - dy, m - dx, H + extra[0], W + extra[1]]),
            "v_scale": np.float32(scale), "v_offset": np.float32(offset), "u_nan": np.packbits(un), "v_nan": np.packbits(vn),
            "true_shift": np.array([dx, dy])}


def registration_case(dsmr, name, **kw):
    z = registration_inputs(**kw)
    u32, v32 = C.rebuild(z)
    u, v = u32.astype(np.float64), v32.astype(np.float64)
    levels, restore = record_levels(dsmr)
    try:
        dx, dy, a, b = dsmr.compute_shift(u, v, scaling=True)
    finally:
        restore()
    dx0, dy0, a0, b0 = dsmr.compute_shift(u, v, scaling=False)
    muu, muv, sigu, sigv, xcorr = dsmr.mean_std_base(u, v, dx, dy)
    assert (dx0, dy0) == (dx, dy)
    n = 2 * levels[0]["irange"] + 1
    gaps = []
    for lv in levels:
        t = np.array(lv["values"], dtype=np.float64)
        assert t.size == n * n
        s = np.sort(t[np.isfinite(t)])
        gaps.append(float(s[-1] - s[-2]))
        lv["table"] = t.reshape(n, n)
    print(f"{name}: shift ({dx}, {dy}), levels {[lv['shape_u'] for lv in levels]}, gaps {gaps}", flush=True)
    assert min(gaps) >= MIN_GAP, f"{name}: NCC gap {min(gaps)} below {MIN_GAP}: choose other inputs"
    save(name, **z, irange=np.int64(levels[0]["irange"]),
         levels_shape_u=np.array([lv["shape_u"] for lv in levels]), levels_shape_v=np.array([lv["shape_v"] for lv in levels]),
         levels_centre=np.array([lv["centre"] for lv in levels]), levels_winner=np.array([lv["winner"] for lv in levels]),
         levels_table=np.stack([lv["table"] for lv in levels]), gaps=np.array(gaps),
         shift=np.array([dx, dy]), moments=np.array([muu, muv, sigu, sigv, xcorr]),
         ab_scaling=np.array([a, b], dtype=np.float64), ab_noscale=np.array([a0, b0], dtype=np.float64))


def downsample_cases(dsmr):
    rng = np.random.default_rng(7)
    out = {}
    for H, W in ((5, 6), (7, 7), (6, 9), (1, 5)):
        u = 500.0 + rng.normal(size=(H, W)) * 5
        u[rng.random((H, W)) < 0.3] = np.nan
        if H > 4:
            u[H - 2:, W - 2:] = np.nan  # a block with no finite pixel
        out[f"in_{H}x{W}"] = u
        out[f"out_{H}x{W}"] = dsmr.downsample2x(u)
    u32 = (500.0 + rng.normal(size=(9, 10)) * 5).astype(np.float32)
    u32[rng.random(u32.shape) < 0.2] = np.nan
    out["in_f32_9x10"] = u32
    out["out_f32_9x10"] = dsmr.downsample2x(u32.astype(np.float64))
    save("downsample", **out)


def apply_shift_cases(ev):
    rng = np.random.default_rng(11)
    out = {}
    coefs = [(-3, 2, 1, 0.0, 0.0, 0.0), (4, -5, 0.98, 2.5, 0.0, 0.0), (30, 1, 1.0, -1.25, 0.01, -0.02), (-1, -40, 1.03, 7.0, 0.003, 0.004),
             (0, 0, 1, 0.1, 0.0, 0.0)]
    for dt in (np.float32, np.float64):
        v = (500.0 + rng.normal(size=(21, 26)) * 5).astype(dt)
        v[rng.random(v.shape) < 0.1] = np.nan
        tag = np.dtype(dt).name
        out[f"in_{tag}"] = v
        for k, (dx, dy, a, b, c, d) in enumerate(coefs):
            a_ = a if isinstance(a, int) else np.float64(a)
            out[f"out_{tag}_{k}"] = ev.apply_shift(v, dx, dy, a_, np.float64(b), np.float64(c), np.float64(d))
    out["coefs"] = np.array(coefs, dtype=np.float64)
    save("apply_shift", **out)


class _FiniteBounds(np.ndarray):
    """A ground truth whose .min() / .max() skip NaN: the reference's own dsm_pointwise_diff then clips with the bounds of
    `clip="finite"` (OURS, not the reference's behaviour)."""

    def min(self, *a, **k):
        return np.nanmin(np.asarray(self))

    def max(self, *a, **k):
        return np.nanmax(np.asarray(self))


def mae_cases(dsmr, ev):
    from eval_dsm import Mae_Computer

    def run(pred, gt):
        diff, pred_r = ev.dsm_pointwise_diff(pred_dsm=pred, gt_dsm=gt)
        try:
            mae = Mae_Computer._compute_mae(None, diff)
        except ValueError:
            mae = np.nan
        return np.asarray(diff), np.asarray(pred_r), np.float64(mae)

    gt, pred = C.shifted_pair(44, 40, (2, -1), seed=21, extra=(6, 6), scale=1.0, offset=1.5)
    rng = np.random.default_rng(22)
    k = rng.random(pred.shape) < 0.03
    lo, hi = np.nanmin(gt), np.nanmax(gt)
    pred[k] = np.where(rng.random(int(k.sum())) < 0.5, lo - 50, hi + 50).astype(np.float32)  # beyond the clip bounds
    pred = pred + rng.normal(size=pred.shape).astype(np.float32) * np.float32(0.3)
    gt_clean = np.where(np.isnan(gt), np.float32(lo), gt)  # the reference's bounds need a ground truth without NaN
    transform = ev.compute_shift(gt_clean, pred, scaling=False)
    diff, pred_r, mae = run(pred.copy(), gt_clean.copy())
    assert np.isfinite(mae) and (np.asarray(pred_r) == lo - 10).any() and (np.asarray(pred_r) == hi + 10).any()
    save("mae_plain", pred=pred, gt=gt_clean, diff=diff, pred_r=pred_r, mae=mae, transform=np.array(transform, dtype=np.float64))

    diff_n, pred_rn, mae_n = run(pred.copy(), gt.copy())
    assert np.isnan(diff_n).all() and np.isnan(mae_n)
    diff_f, pred_rf, mae_f = run(pred.copy(), gt.copy().view(_FiniteBounds))
    assert np.isfinite(mae_f)
    save("mae_gt_nan", pred=pred, gt=gt, diff=diff_n, pred_r=pred_rn, ours_finite_diff=np.asarray(diff_f),
         ours_finite_pred_r=np.asarray(pred_rf), ours_finite_mae=mae_f,
         transform=np.array(ev.compute_shift(gt, pred, scaling=False), dtype=np.float64))

    water = rng.random((50, 47)) < 0.08  # larger than the DSM
    vis = rng.random(gt_clean.shape) < 0.06
    tree = rng.random((41, 38)) < 0.9  # smaller than the DSM: the DSM is cropped; NaN where the tree mask is False
    masked = ev.mask_dsm(gt_clean.copy(), water.copy(), vis.copy(), tree.copy())
    only_water = ev.mask_dsm(gt_clean.copy(), water.copy(), None, None)
    diff_m, pred_rm, mae_m = run(pred.copy(), np.array(masked).view(_FiniteBounds))
    save("mae_masks", gt=gt_clean, pred=pred, water=water, vis=vis, tree=tree, masked=np.asarray(masked), only_water=np.asarray(only_water),
         ours_finite_diff=np.asarray(diff_m), ours_finite_pred_r=np.asarray(pred_rm), ours_finite_mae=mae_m)


CASES = {
    "single_40x37": dict(H=40, W=37, shift=(2, -1), seed=1, nan_border=True),
    "two_levels_118x131": dict(H=118, W=131, shift=(4, -3), seed=2),
    "three_levels_202x206": dict(H=202, W=206, shift=(7, -9), seed=3),
    "odd_101x203": dict(H=101, W=203, shift=(-3, 5), seed=4),
    "sec_larger": dict(H=52, W=45, shift=(1, 3), seed=5, extra=(3, 2)),
}


def main():
    dsmr, ev = load_ref()
    want = sys.argv[1:] or list(CASES) + ["downsample", "apply_shift", "mae"]
    for name in want:
        if name in CASES:
            registration_case(dsmr, name, **CASES[name])
    if "downsample" in want:
        downsample_cases(dsmr)
    if "apply_shift" in want:
        apply_shift_cases(ev)
    if "mae" in want:
        mae_cases(dsmr, ev)


if __name__ == "__main__":
    main()
