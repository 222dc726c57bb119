"""TEST INFRASTRUCTURE — vectorised restatement of the reference's DSM registration and scoring (checker for
eogs2_amd.dsm_eval / the eogs_tsdf_dsm_* entries of include/eogs_tsdf.h, and the CPU baseline of tools/dsm_eval_probe.py):
  valnan / downsample2x / mean_std_base / ncc / compute_ncc / recursive_ncc / compute_shift / apply_shift
                                                                  src/gaussiansplatting/eval/dsmr.py
  mask_dsm / dsm_pointwise_diff / Mae_Computer._compute_mae       src/gaussiansplatting/eval/eval_dsm.py:35-69, 334-341
Pinned against vectors the reference's own modules produced (tests/golden/make_golden_dsm_eval.py,
tests/test_dsm_eval_oracle.py). All arithmetic is float64, as numba types the reference's accumulators; the sums run in
numpy's / torch's order, not the reference's row-major one, which moves a result by at most `eps(N)` below.

Also here: `rebuild(z)`, which makes a registration case's two images from the stored base terrain, crop rectangles and
bit-packed NaN masks (fixtures stay small), and the error bound the tests share.
"""
import math
import os

import numpy as np
import torch

from util import GOLDEN_DIR

IRANGE = 5


# ---------------------------------------------------------------------------------------------------------------------
# the bound (derived from N, the pixel count of `u` at the level in question)
def eps(n):
    """Two correct float64 evaluations of a sum of n terms in different orders differ by at most n 2^-53 sum|term|; the
    factor 8 covers the dependent operations after the sums (two square roots, a product, a quotient)."""
    return 8.0 * n * 2.0 ** -53


def mae_margin_f32(n, mae):
    """np.nanmean over a float32 diff sums pairwise in float32: good to ceil(log2 n) 2^-24 mae."""
    return math.ceil(math.log2(max(n, 2))) * 2.0 ** -24 * abs(mae)


# ---------------------------------------------------------------------------------------------------------------------
# fixtures
def rebuild(z):
    """(u, v) float32 of a registration fixture: u = base[u_rect]; v = f32(v_scale) * base[v_rect] + f32(v_offset),
    evaluated in float32; then the packed NaN masks."""
    base = np.asarray(z["base"], dtype=np.float32)

    def crop(rect):
        y0, x0, h, w = (int(t) for t in rect)
        return base[y0:y0 + h, x0:x0 + w].copy()

    u = crop(z["u_rect"])
    v = crop(z["v_rect"]) * np.float32(z["v_scale"]) + np.float32(z["v_offset"])
    for img, key in ((u, "u_nan"), (v, "v_nan")):
        m = np.unpackbits(np.asarray(z[key], dtype=np.uint8))[: img.size].reshape(img.shape).astype(bool)
        img[m] = np.nan
    return u, v.astype(np.float32)


def level_shapes(hu, wu, hv, wv):
    """Shapes of the pyramid the recursion visits, full resolution first."""
    out = [((hu, wu), (hv, wv))]
    while min(hu, wu) > 100:
        hu, wu, hv, wv = (hu + 1) // 2, (wu + 1) // 2, (hv + 1) // 2, (wv + 1) // 2
        out.append(((hu, wu), (hv, wv)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# dsmr.py
def downsample2x(u):
    """out[J][I] = mean over the finite pixels of the 2 x 2 block whose top-left corner is (min(2J+1, H-1), min(2I+1, W-1)),
    clipped to the image (the reference writes out[j // 2][i // 2] for every source pixel: the last writer wins)."""
    u = np.asarray(u, dtype=np.float64)
    H, W = u.shape
    jj = np.minimum(2 * np.arange((H + 1) // 2) + 1, H - 1)
    ii = np.minimum(2 * np.arange((W + 1) // 2) + 1, W - 1)
    s = np.zeros((jj.size, ii.size))
    cnt = np.zeros((jj.size, ii.size))
    for dj, di in ((0, 0), (1, 0), (0, 1), (1, 1)):  # the reference's order: k (columns) outer, l (rows) inner
        r, c = jj + dj, ii + di
        inb = (r < H)[:, None] & (c < W)[None, :]
        t = u[np.minimum(r, H - 1)][:, np.minimum(c, W - 1)]
        ok = inb & np.isfinite(t)
        s = s + np.where(ok, t, 0.0)
        cnt = cnt + ok
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, s / cnt, np.nan)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def mean_std(u, v, dx=0, dy=0):
    """mean_std_base in its centred two-pass form: (count, muu, muv, sigu, sigv, xcorr); NaN moments if no finite pair."""
    u = u if torch.is_tensor(u) else _t64(u)
    v = v if torch.is_tensor(v) else _t64(v)
    H, W = u.shape
    if v.shape[0] < H or v.shape[1] < W:
        raise ValueError("the image to register is smaller than the reference image")
    i0, i1, j0, j1 = max(0, -dx), min(W, W - dx), max(0, -dy), min(H, H - dy)  # the bounds test uses u's size
    nan = float("nan")
    if i1 <= i0 or j1 <= j0:
        return 0, nan, nan, nan, nan, nan
    uu, vv = u[j0:j1, i0:i1], v[j0 + dy:j1 + dy, i0 + dx:i1 + dx]
    ok = torch.isfinite(uu) & torch.isfinite(vv)
    count = int(ok.sum())
    if count == 0:
        return 0, nan, nan, nan, nan, nan
    zero = torch.zeros((), dtype=torch.float64)
    muu = float(torch.where(ok, uu, zero).sum()) / count
    muv = float(torch.where(ok, vv, zero).sum()) / count
    du, dv = torch.where(ok, uu - muu, zero), torch.where(ok, vv - muv, zero)
    sigu = math.sqrt(float((du * du).sum()) / count)
    sigv = math.sqrt(float((dv * dv).sum()) / count)
    xcorr = float((du * dv).sum()) / count
    return count, muu, muv, sigu, sigv, xcorr


def ncc(u, v, dx=0, dy=0):
    _, _, _, sigu, sigv, xcorr = mean_std(u, v, dx, dy)
    return xcorr / (sigu * sigv + 1e-8)


def ncc_table(u, v, irange, initdx, initdy):
    """[2 irange + 1][2 irange + 1] float64, rows = dy, columns = dx (the reference's scan order)."""
    u, v = _t64(u), _t64(v)
    n = 2 * irange + 1
    t = np.empty((n, n))
    for a, y in enumerate(range(initdy - irange, initdy + irange + 1)):
        for b, x in enumerate(range(initdx - irange, initdx + irange + 1)):
            t[a, b] = ncc(u, v, x, y)
    return t


def argmax_scan(table, irange, initdx, initdy):
    """compute_ncc's winner: strict `>`, the first of equal values wins, a NaN never wins; starts from the centre."""
    best, maxv = (initdx, initdy), -np.inf
    for a in range(table.shape[0]):
        for b in range(table.shape[1]):
            if table[a, b] > maxv:
                best, maxv = (initdx - irange + b, initdy - irange + a), table[a, b]
    return best


def compute_ncc(u, v, irange, initdx, initdy):
    t = ncc_table(u, v, irange, initdx, initdy)
    if not np.isfinite(t).any():
        raise ValueError("no candidate shift has a finite NCC")
    return argmax_scan(t, irange, initdx, initdy), t


def recursive_ncc(u, v, irange=IRANGE, dx=0, dy=0, record=None):
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if min(u.shape) > 100:
        dx, dy = recursive_ncc(downsample2x(u), downsample2x(v), irange, dx // 2, dy // 2, record)
        dx, dy = dx * 2, dy * 2
    (bx, by), t = compute_ncc(u, v, irange, dx, dy)
    if record is not None:
        record.append({"shape_u": u.shape, "shape_v": v.shape, "centre": (dx, dy), "table": t, "winner": (bx, by)})
    return bx, by


def compute_shift(dsm_ref, dsm_sec, scaling=True, record=None):
    dx, dy = recursive_ncc(dsm_ref, dsm_sec, record=record)
    _, muu, muv, sigu, sigv, _ = mean_std(dsm_ref, dsm_sec, dx, dy)
    a = sigu / sigv if scaling else 1
    b = muu - muv * a
    return dx, dy, a, b


def apply_shift(in_dsm, dx=0, dy=0, a=1, b=0, c=0, d=0):
    v = np.asarray(in_dsm)
    H, W = v.shape
    J, I = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    jj, ii = J + dy, I + dx
    inb = (ii >= 0) & (jj >= 0) & (ii < W) & (jj < H)
    val = np.where(inb, v.astype(np.float64)[np.clip(jj, 0, H - 1), np.clip(ii, 0, W - 1)], np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.float64(a) * val + np.float64(b) + np.float64(c) * I + np.float64(d) * J
        return out.astype(v.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# eval_dsm.py
def mask_dsm(dsm, water_mask, vis_mask, tree_mask):
    dsm = np.array(dsm, copy=True)
    if water_mask is not None:
        dsm[water_mask[: dsm.shape[0], : dsm.shape[1]]] = np.nan
    if vis_mask is not None:
        dsm[vis_mask] = np.nan
    if tree_mask is not None:
        if dsm.shape != tree_mask.shape:
            dsm = dsm[: tree_mask.shape[0], : tree_mask.shape[1]]
        dsm[np.logical_not(tree_mask)] = np.nan
    return dsm


def dsm_pointwise_diff(pred_dsm, gt_dsm, clip="reference"):
    """`clip="reference"`: bounds gt.min() - 10, gt.max() + 10 (NaN bounds if the ground truth holds a NaN: everything
    becomes NaN); `clip="finite"`: np.nanmin / np.nanmax (ours)."""
    transform = compute_shift(gt_dsm, pred_dsm, scaling=False)
    pred_r = apply_shift(pred_dsm, *transform)
    h, w = min(pred_r.shape[0], gt_dsm.shape[0]), min(pred_r.shape[1], gt_dsm.shape[1])
    with np.errstate(invalid="ignore"):
        lo, hi = (gt_dsm.min(), gt_dsm.max()) if clip == "reference" else (np.nanmin(gt_dsm), np.nanmax(gt_dsm))
        pred_r = np.clip(pred_r, lo - 10, hi + 10)
        diff = pred_r[:h, :w] - gt_dsm[:h, :w]
    return diff, pred_r, transform


def mae_of(diff):
    """float64 mean of |diff| over its non-NaN entries; ValueError if there is none (eval_dsm.py:334-341)."""
    d = np.abs(np.asarray(diff, dtype=np.float64).ravel())
    ok = ~np.isnan(d)
    if not ok.any():
        raise ValueError("The computed MAE is NaN: the diff array contains only NaN values")
    return float(d[ok].sum() / ok.sum())


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs larger than a fixture may be
def terrain(H, W, seed, mean=500.0):
    """Smooth field + random-walk relief + boxes, mean ~ 100 x its standard deviation (a UTM-like altitude), float64."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    z = 2.0 * np.sin(3.1 * x + 1.0) * np.cos(2.3 * y) + 1.5 * x * y
    walk = np.cumsum(rng.normal(size=(H, W)), axis=1) / math.sqrt(W) + np.cumsum(rng.normal(size=(H, W)), axis=0) / math.sqrt(H)
    z = z + 1.2 * walk
    for _ in range(max(6, H * W // 900)):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        hh, hw = rng.integers(2, max(3, H // 8)), rng.integers(2, max(3, W // 8))
        z[max(0, cy - hh):cy + hh, max(0, cx - hw):cx + hw] = z[cy, cx] + rng.uniform(2.0, 9.0)
    z = z - z.mean()
    return mean + z * (mean / 100.0 / z.std())


def shifted_pair(H, W, shift, seed, extra=(0, 0), scale=0.97, offset=2.5, nan_share=0.05, dtype=np.float32):
    """(u [H][W], v [H + extra[0]][W + extra[1]]) with v[j + dy][i + dx] = scale u[j][i] + offset, 5 % NaN in each."""
    dx, dy = shift
    m = max(abs(dx), abs(dy)) + 2
    base = terrain(H + 2 * m + extra[0], W + 2 * m + extra[1], seed)
    u = base[m:m + H, m:m + W].astype(dtype)
    v = (scale * base[m - dy:m - dy + H + extra[0], m - dx:m - dx + W + extra[1]] + offset).astype(dtype)
    rng = np.random.default_rng(seed + 1)
    u[rng.random(u.shape) < nan_share] = np.nan
    v[rng.random(v.shape) < nan_share] = np.nan
    return u, v


# ---------------------------------------------------------------------------------------------------------------------
# what the CPU and the GPU tests share: fixtures and the checks against them
DSM_DIR = os.path.join(GOLDEN_DIR, "dsm_eval")
REGISTRATION = ["single_40x37", "two_levels_118x131", "three_levels_202x206", "odd_101x203", "sec_larger"]


def load(name):
    z = np.load(os.path.join(DSM_DIR, f"{name}.npz"))
    return {k: z[k] for k in z.files}


def same_bits(a, b):
    """Equal bit for bit outside the NaNs, and NaN in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return a[ok].tobytes() == b[ok].tobytes()


def check_moments(got, z, n, what):
    """(muu, muv, sigu, sigv, xcorr) against the fixture's mean_std_base tuple under the bound of an n-pixel level."""
    e = eps(n)
    muu, muv, sigu, sigv, xcorr = (float(t) for t in z["moments"])
    print(f"{what}: eps {e:.3e}  dmuu {abs(got[0] - muu):.3e}  dmuv {abs(got[1] - muv):.3e}  dsigu/sigu {abs(got[2] - sigu) / sigu:.3e}  "
          f"dsigv/sigv {abs(got[3] - sigv) / sigv:.3e}  dxcorr {abs(got[4] - xcorr):.3e} (bound {e * sigu * sigv:.3e})")
    assert abs(got[0] - muu) <= e * abs(muu) and abs(got[1] - muv) <= e * abs(muv)  # mean|u| >= |mean u|
    assert abs(got[2] - sigu) <= e * sigu and abs(got[3] - sigv) <= e * sigv
    assert abs(got[4] - xcorr) <= e * sigu * sigv


def check_ab(a, b, z, key, n, what):
    """a: relative error <= eps; b: absolute error <= eps (mean|u| + mean|v|) over the counted pixels (the fixtures' heights are
    positive, so the means of the absolute values are |muu| and |muv|)."""
    e = eps(n)
    ra, rb = (float(t) for t in z[key])
    muu, muv = float(z["moments"][0]), float(z["moments"][1])
    print(f"{what} {key}: da/a {abs(a - ra) / ra:.3e}  db {abs(b - rb):.3e}  (eps {e:.3e}, bound on b {e * (abs(muu) + abs(muv)):.3e})")
    assert abs(a - ra) <= e * ra
    assert abs(b - rb) <= e * (abs(muu) + abs(muv))


def b_bound(gt, pred):
    """The bound on b of a registration of `pred` on `gt`: eps (mean|gt| + mean|pred|) with N the ground truth's pixel count
    (the means over each image's finite pixels: within a border's width of the counted ones)."""
    gt, pred = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    return eps(gt.size) * (float(np.nanmean(np.abs(gt))) + float(np.nanmean(np.abs(pred[np.isfinite(pred)]))))


def diff_tol(gt, pred, ref_pred_r):
    """diff and pred_rdsm through the whole dsm_pointwise_diff: a is the integer 1 there, so only b moves them: the bound
    on b plus one ulp of the storage type at the registered DSM's largest magnitude."""
    ref_pred_r = np.asarray(ref_pred_r)
    return b_bound(gt, pred) + float(np.spacing(ref_pred_r.dtype.type(np.nanmax(np.abs(ref_pred_r)))))


def check_mae(mae, ref_mae, ref_diff, n, what):
    """Against the recorded np.nanmean (which ran in the diff's dtype: a float32 pairwise sum is good to ceil(log2 N) 2^-24
    mae) and against the float64 mean of the recorded diff under eps mae."""
    m64 = mae_of(ref_diff)
    margin = mae_margin_f32(ref_diff.size, float(ref_mae)) if ref_diff.dtype == np.float32 else eps(n) * m64
    print(f"{what}: mae {mae!r} recorded {float(ref_mae)!r} (margin {margin:.3e}) float64 mean of the recorded diff {m64!r} "
          f"(|d| {abs(mae - m64):.3e}, bound {eps(n) * m64:.3e})")
    assert abs(mae - float(ref_mae)) <= margin
    assert abs(mae - m64) <= eps(n) * m64
