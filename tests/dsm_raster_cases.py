"""Shared by the DSM raster tests (eogs2_amd.dsm_raster, include/eogs_dsm.h): the float64 numpy restatement of the raster's
stated semantics, an independent brute-force loop, the value bound, the seeded cloud cases and the fixture loader.

The semantics (include/eogs_dsm.h), for sigma = inf: home cell i = floor((x - xoff) / res),
j = floor((yoff - y) / res); the point contributes float32(z) to every cell within `radius` of the home cell that lies
inside the raster (only the target is range-checked); a cell holds the mean of its contributions, NaN without one; a
non-finite z or |z| > Z_MAX makes its footprint NaN; a non-finite x or y is skipped and counted.
"""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dsm_raster")
Z_QUANTUM = 2.0 ** -20  # EOGS_DSM_Z_QUANTUM: the issue requires <= 2^-20 m
Z_MAX = 32768.0  # EOGS_DSM_Z_MAX
MAX_FIXTURE_BYTES = 400 * 1024


def restate(cloud, xoff, yoff, res, xsize, ysize, radius=1):
    """(mean float64 [ysize, xsize], counts int32 [ysize, xsize], skipped): the stated semantics, accumulated with np.add.at
    in float64. counts is -1 under a poisoned footprint."""
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    x, y = cloud[:, 0], cloud[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        z = cloud[:, 2].astype(np.float32)
        ok = np.isfinite(x) & np.isfinite(y)
        i = np.floor((x - xoff) / res)
        j = np.floor((yoff - y) / res)
        bad = ~(np.isfinite(z) & (np.abs(z) <= np.float32(Z_MAX)))
    total = np.zeros((ysize, xsize), dtype=np.float64)
    cnt = np.zeros((ysize, xsize), dtype=np.int64)
    poison = np.zeros((ysize, xsize), dtype=bool)
    z64 = z.astype(np.float64)
    for dj in range(-radius, radius + 1):
        for di in range(-radius, radius + 1):
            ii, jj = i + di, j + dj
            with np.errstate(invalid="ignore"):
                m = ok & (ii >= 0) & (ii < xsize) & (jj >= 0) & (jj < ysize)
            g, b = m & ~bad, m & bad
            np.add.at(total, (jj[g].astype(np.int64), ii[g].astype(np.int64)), z64[g])
            np.add.at(cnt, (jj[g].astype(np.int64), ii[g].astype(np.int64)), 1)
            poison[jj[b].astype(np.int64), ii[b].astype(np.int64)] = True
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where((cnt > 0) & ~poison, total / cnt, np.nan)
    return mean, np.where(poison, -1, cnt).astype(np.int32), int((~ok).sum())


def brute_force(cloud, xoff, yoff, res, xsize, ysize, radius=1):
    """The same result from a plain loop that walks every point's CLIPPED footprint, sums kept as exact Python fractions of
    the float32 values (math.fsum): independent of np.add.at and of the home-cell-plus-stencil formulation."""
    import math

    cells = {}
    poison = set()
    skipped = 0
    for x, y, z in np.asarray(cloud, dtype=np.float64).reshape(-1, 3).tolist():
        if not (math.isfinite(x) and math.isfinite(y)):
            skipped += 1
            continue
        i, j = math.floor((x - xoff) / res), math.floor((yoff - y) / res)
        with np.errstate(over="ignore"):
            zf = float(np.float32(z))
        bad = not (math.isfinite(zf) and abs(zf) <= Z_MAX)
        for jj in range(max(j - radius, 0), min(j + radius, ysize - 1) + 1):
            for ii in range(max(i - radius, 0), min(i + radius, xsize - 1) + 1):
                if bad:
                    poison.add((jj, ii))
                else:
                    cells.setdefault((jj, ii), []).append(zf)
    mean = np.full((ysize, xsize), np.nan)
    cnt = np.zeros((ysize, xsize), dtype=np.int32)
    for (jj, ii), zs in cells.items():
        mean[jj, ii] = math.fsum(zs) / len(zs)
        cnt[jj, ii] = len(zs)
    for jj, ii in poison:
        mean[jj, ii] = np.nan
        cnt[jj, ii] = -1
    return mean, cnt, skipped


def ulp32(m):
    """The spacing of float32 at |m| (m float64), 2^(e - 24) for |m| in [2^(e-1), 2^e); the smallest subnormal at 0."""
    m = np.abs(np.asarray(m, dtype=np.float64))
    _, e = np.frexp(m)
    return np.where(m > 0, np.ldexp(1.0, np.maximum(e - 24, -149)), 2.0 ** -149)


def value_bound(m, ulps=1):
    """The issue's bar |out - m| <= q / 2 + ulps * ulp32(m): q / 2 the worst mean of the per-point quantisation, half an ulp
    the final narrowing, the rest slack for the double division (ulps = 2 where z itself may differ by an ulp)."""
    return Z_QUANTUM / 2 + ulps * ulp32(m)


def check_raster(out, count_out, mean, counts, ulps=1, what=""):
    """Exact NaN pattern, exact counts, values within the bound. `out` float32 [ysize, xsize, 1] or [ysize, xsize]."""
    out = np.asarray(out)
    assert out.dtype == np.float32, out.dtype
    if out.ndim == 3:
        assert out.shape[2] == 1
        out = out[:, :, 0]
    assert out.shape == mean.shape, (what, out.shape, mean.shape)
    if count_out is not None:
        assert np.array_equal(np.asarray(count_out), counts), f"{what}: counts differ in {(np.asarray(count_out) != counts).sum()} cells"
    assert np.array_equal(np.isnan(out), np.isnan(mean)), f"{what}: NaN pattern differs"
    assert np.array_equal(np.isnan(mean), counts <= 0), f"{what}: the expectation contradicts itself"
    f = ~np.isnan(mean)
    err = np.abs(out[f].astype(np.float64) - mean[f])
    bound = value_bound(mean[f], ulps)
    worst = float((err / bound).max()) if err.size else 0.0
    print(f"{what}: {int(f.sum())} cells, worst error / bound = {worst:.3f}, max error {float(err.max()) if err.size else 0.0:.3e}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} cells beyond q/2 + {ulps} ulp32, worst ratio {worst:.3f}"


X0, Y0 = 5e5, 4.3e6  # UTM-sized offsets


def _uniform_cloud(g, n, xoff, yoff, res, xsize, ysize):
    x = xoff + g.random(n) * xsize * res
    y = yoff - g.random(n) * ysize * res
    z = 30.0 + 15.0 * g.standard_normal(n)
    return np.stack([x, y, z], axis=1)


def cloud_cases():
    """name -> (cloud float64 [N, 3], xoff, yoff, res, xsize, ysize, radius): the inputs of the issue's GPU test 1."""
    g = np.random.default_rng(20251018)
    cases = {"n1_on_1x1": (np.array([[X0 + 0.2, Y0 - 0.1, 12.3456789]]), X0, Y0, 0.5, 1, 1, 1)}
    for res in (0.3, 0.5):
        xoff, yoff = np.floor(X0 / res) * res, np.ceil(Y0 / res) * res
        cloud = _uniform_cloud(g, 5000, xoff, yoff, res, 37, 23)
        for radius in (0, 1, 2):
            cases[f"uniform_37x23_res{res}_r{radius}"] = (cloud, xoff, yoff, res, 37, 23, radius)
        # explicit geometry smaller than the cloud on all four sides, by 1.5 and by 4 cells: home cells outside the raster
        # reach in, points beyond the padding are dropped
        for cut, radius in ((1.5, 1), (4.0, 2), (4.0, 0)):
            cases[f"cropped_by{cut}_res{res}_r{radius}"] = (cloud, xoff + cut * res, yoff - cut * res, res, 37 - 2 * int(np.ceil(cut)),
                                                            23 - 2 * int(np.ceil(cut)), radius)
    # lattice points exactly on cell edges at res 0.5 (every quotient is an exact integer), the last row and column one cell
    # outside the raster
    kx, ky = np.meshgrid(np.arange(-1, 13), np.arange(-1, 9))
    lattice = np.stack([X0 + 0.5 * kx.ravel(), Y0 - 0.5 * ky.ravel(), 20.0 + 0.37 * kx.ravel() - 0.11 * ky.ravel()], axis=1)
    for radius in (0, 1):
        cases[f"lattice_res0.5_r{radius}"] = (lattice, X0, Y0, 0.5, 12, 8, radius)
    # 20 000 points in one cell of a 3 x 3 raster: one contended home cell, a long sum (and one with |z| near Z_MAX)
    pile = np.stack([X0 + 0.5 + 0.5 * g.random(20000), Y0 - 0.5 - 0.5 * g.random(20000), 100.0 * g.standard_normal(20000)], axis=1)
    cases["pile_20000_in_one_cell"] = (pile, X0, Y0, 0.5, 3, 3, 1)
    high = pile.copy()
    high[:, 2] = 32000.0 + 700.0 * g.random(20000)
    cases["pile_near_zmax"] = (high, X0, Y0, 0.5, 3, 3, 1)
    cases["empty"] = (np.zeros((0, 3)), X0, Y0, 0.5, 5, 4, 1)
    return cases


def fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))


def fixture_names(kind=None):
    """Case names: every <name>.npz that is not the <name>_xy.npz half (the cloud's x and y, split off to keep files small)."""
    names = [os.path.basename(p)[:-4] for p in fixture_files() if not p.endswith("_xy.npz")]
    return [n for n in names if kind is None or n.startswith(kind)]


def load(name):
    """One case as a dict; `cloud` float64 [N, 3] is put together from its two halves."""
    d = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    xy = np.load(os.path.join(GOLDEN, f"{name}_xy.npz"))["cloud_xy"]
    d["cloud"] = np.concatenate([xy, d.pop("cloud_z")[:, None]], axis=1)
    d["geometry"] = (np.float64(d["xoff"]), np.float64(d["yoff"]), int(d["xsize"]), int(d["ysize"]))
    return d


def emulate_kernel(cloud, xoff, yoff, res, xsize, ysize, radius=1):
    """The kernels' own formulation in numpy integers (eogs2_amd/csrc/dsm_raster.hip): every point goes to its HOME cell
    only, on a grid padded by `radius`, as round-to-even(float32(z) * 2^20) into an int64 sum and a count; a stencil pass
    adds the (2 radius + 1)^2 neighbourhood and divides once in double. Returns (float32 raster, int32 counts, skipped)."""
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    x, y = cloud[:, 0], cloud[:, 1]
    pw, ph = xsize + 2 * radius, ysize + 2 * radius
    with np.errstate(over="ignore", invalid="ignore"):
        z = cloud[:, 2].astype(np.float32)
        ok = np.isfinite(x) & np.isfinite(y)
        fi = np.floor((x - xoff) / res) + radius
        fj = np.floor((yoff - y) / res) + radius
        keep = ok & (fi >= 0) & (fi < pw) & (fj >= 0) & (fj < ph)
        bad = ~(np.abs(z) <= np.float32(Z_MAX))
    pi, pj = fi[keep].astype(np.int64), fj[keep].astype(np.int64)
    zk, bk = z[keep].astype(np.float64), bad[keep]
    sums = np.zeros((ph, pw), dtype=np.int64)
    cnts = np.zeros((ph, pw), dtype=np.int64)
    poison = np.zeros((ph, pw), dtype=np.int64)
    np.add.at(sums, (pj[~bk], pi[~bk]), np.rint(zk[~bk] / Z_QUANTUM).astype(np.int64))
    np.add.at(cnts, (pj[~bk], pi[~bk]), 1)
    poison[pj[bk], pi[bk]] = 1
    n = 2 * radius + 1
    window = lambda a: sum(a[dj:dj + ysize, di:di + xsize] for dj in range(n) for di in range(n))  # noqa: E731
    s, c, p = window(sums), window(cnts), window(poison)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where((p == 0) & (c > 0), (s.astype(np.float64) * Z_QUANTUM) / c, np.nan).astype(np.float32)
    return out, np.where(p > 0, -1, c).astype(np.int32), int((~ok).sum())
