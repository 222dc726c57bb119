"""The two-stage sum of csrc/reduce.h restated in numpy, and seeded inputs for the masked L1 loss that goes through it.

The restatement follows the header comment of reduce.h word for word, in float32, vectorised over lanes:
  Stage 1. 256 threads per workgroup, the grid capped at 1024. Thread t of workgroup g adds its elements g * 256 + t,
           + grid * 256, ... in that order; the 64 lanes of a wave combine by the xor butterfly (offsets 32 .. 1); the four
           wave sums are added left to right; one partial per workgroup.
  Stage 2. One workgroup per column: thread t adds partials t, t + 256, ... in that order, the same butterfly, the same
           four waves.
  Epilogue of the masked loss: {S_alt / N, S_rgb / N, N}, zeros for N = 0.
Every value on the path is a float32 add, subtract, abs or divide (IEEE, no contraction), so the restatement is exact: the
GPU test compares bits. A pixel outside the mask contributes +0 here where the kernel skips it: x + 0 = x for the
non-negative sums of this loss.

`column_stride` and `waves_right_to_left` give two deliberately WRONG orders; with `float64_once` they are what the CPU test
uses to show that the seeds below discriminate.
"""
import numpy as np

THREADS, CAP = 256, 1024  # csrc/shade.hip: ST (the four waves csrc/reduce.h asserts), SMAXBLK
MODE_SUN, MODE_RANDOM = 0, 1  # include/eogs_shade.h
f32 = np.float32

# (H, W): one lane; two workgroups and a partial wave; 301 workgroups (the column sum's second trip for lanes < 45); the grid
# at its cap and a second grid-stride trip for 300 lanes
SHAPES = [(1, 1), (1, 257), (1, 76_837), (1, 262_444)]
LARGE = SHAPES[2:]
# Seeds for which the restated order differs in bits from each wrong order (test_reduce_cases.py holds them to it):
# "alt" seeds alt_diff and uv, "ab"[C] seeds the two images of C planes.
SEEDS = {
    1: dict(alt=0, ab={1: 0, 2: 0, 3: 0, 4: 0}),
    257: dict(alt=0, ab={1: 0, 2: 0, 3: 0, 4: 0}),
    76_837: dict(alt=8, ab={1: 0, 2: 0, 3: 0, 4: 2}),
    262_444: dict(alt=61, ab={1: 4, 2: 33, 3: 659, 4: 19}),
}


def blocks(n):
    return min(CAP, max(1, -(-n // THREADS)))


def _lanes_in_order(x, lanes):
    """x[(n,) + cols] -> [(lanes,) + cols]: lane l adds x[l], x[l + lanes], ... in that order, from +0."""
    trips = -(-x.shape[0] // lanes)
    pad = np.zeros((trips * lanes,) + x.shape[1:], f32)
    pad[: x.shape[0]] = x
    pad = pad.reshape((trips, lanes) + x.shape[1:])
    acc = np.zeros((lanes,) + x.shape[1:], f32)
    for j in range(trips):
        acc = acc + pad[j]
    return acc


def _workgroup(v, waves_right_to_left=False):
    """v[(groups, 256) + cols] -> [(groups,) + cols]: the butterfly over each wave's 64 lanes, then the four waves."""
    v = v.reshape((v.shape[0], 4, 64) + v.shape[2:])
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]  # (every lane holds the same bits: a + b == b + a)
    if waves_right_to_left:
        return ((w[:, 3] + w[:, 2]) + w[:, 1]) + w[:, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def two_stage_sum(x, column_stride=THREADS, waves_right_to_left=False):
    """Sum over axis 0 of float32 x[(n,) + cols] in reduce.h's order; float32[cols]."""
    x = np.asarray(x, f32)
    g = blocks(x.shape[0])
    lanes = _lanes_in_order(x, g * THREADS)
    partial = _workgroup(lanes.reshape((g, THREADS) + x.shape[1:]), waves_right_to_left)
    col = np.zeros((THREADS,) + x.shape[1:], f32)
    col[:column_stride] = _lanes_in_order(partial, column_stride)
    return _workgroup(col[None], waves_right_to_left)[0]


def float64_once(x):
    return np.asarray(x, np.float64).sum(axis=0).astype(f32)


# ---- the masked L1 loss ------------------------------------------------------------------------------------------------
def inputs(H, W, C):
    """alt_diff (H, W), uv (H, W, 2), a and b (C, H, W), float32. About one pixel in 16 fails each of |alt| < 0.30,
    |u| < 1 and |v| < 1; values inside the mask lie in [0, 0.29) in magnitude (alt_diff of either sign)."""
    n = H * W
    s = SEEDS[n]
    r = np.random.default_rng([n, s["alt"]])
    alt = (r.uniform(0.0, 0.29, n) * r.choice([-1.0, 1.0], n)).astype(f32)
    uv = r.uniform(-0.98, 0.98, (n, 2)).astype(f32)
    if n > 1:  # (the single lane stays inside the mask)
        out = r.integers(0, 16, (3, n))
        alt[out[0] == 0] = f32(0.31) * np.sign(alt[out[0] == 0])
        uv[out[1] == 0, 0] = f32(1.0)
        uv[out[2] == 0, 1] = f32(-1.25)
    else:
        alt = np.abs(alt)  # (inside mode SUN's mask too)
    r = np.random.default_rng([n, C, s["ab"][C]])
    a, b = r.uniform(0.0, 0.29, (2, C, n)).astype(f32)
    return alt.reshape(H, W), uv.reshape(H, W, 2), a.reshape(C, H, W), b.reshape(C, H, W)


def mask(mode, alt, uv):
    alt_ok = alt > f32(-1e-2) if mode == MODE_SUN else np.abs(alt) < f32(0.30)
    return alt_ok & (np.abs(uv[..., 0]) < f32(1.0)) & (np.abs(uv[..., 1]) < f32(1.0))


def terms(mode, alt, uv, a, b):
    """Per pixel, float32 [n, 3]: |alt|, t = |a0 - b0|; t += |a1 - b1|; ..., and 1 — inside the mask, +0 outside."""
    m = mask(mode, alt, uv).reshape(-1)
    t = np.abs(a[0] - b[0])
    for k in range(1, a.shape[0]):
        t = t + np.abs(a[k] - b[k])
    x = np.stack([np.abs(alt).reshape(-1), t.reshape(-1), np.ones(m.size, f32)], axis=1).astype(f32)
    return np.where(m[:, None], x, f32(0.0)), m


def epilogue(tot):
    n = tot[2]
    if not n > 0:
        return np.array([0.0, 0.0, n], f32)
    return np.array([tot[0] / n, tot[1] / n, n], f32)


def masked_l1(mode, alt, uv, a, b, sum_fn=two_stage_sum, **order):
    """out[3] = {S_alt / N, S_rgb / N, N} as the kernels form it (or through a wrong order), and the mask."""
    x, m = terms(mode, alt, uv, a, b)
    return epilogue(sum_fn(x, **order)), m


def g_alt(upstream_alt, n_mask, m, alt):
    """(upstream / N * mask) * sgn(alt_diff), float32, with the signed zeros the product leaves outside the mask."""
    if not n_mask > 0:  # an empty mask: +0 everywhere
        return np.zeros(alt.shape, f32)
    w = f32(upstream_alt) / f32(n_mask)
    return ((w * m.astype(f32)) * np.sign(alt)).astype(f32)
