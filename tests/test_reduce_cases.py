"""CPU: the numpy restatement of csrc/reduce.h's two-stage sum (tests/reduce_cases.py) and the seeds of its inputs.

The GPU test compares the kernels with the restatement bit for bit; that shows the ORDER only if another order gives other
bits on the same inputs. So for the two larger shapes the seeds must make the restated S_alt / N and S_rgb / N differ from
the float64 sum rounded once, from the column sum taken with stride 64 and from the four waves added right to left. This is
a condition on the seeds (a sum of 76 837 terms in two orders agrees in float32 now and then), not a measurement.
"""
import numpy as np
import pytest

import reduce_cases as RC

WRONG = {"float64 once": dict(sum_fn=RC.float64_once), "column stride 64": dict(column_stride=64),
         "waves right to left": dict(waves_right_to_left=True)}


def bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def test_restatement_is_a_sum():
    """Against float64 within the roundings of the longest path, and exact where every order is exact (small integers)."""
    r = np.random.default_rng(3)
    for n in (1, 63, 257, 76_837, 262_444):
        k = r.integers(0, 4, (n, 2)).astype(np.float32)
        assert np.array_equal(RC.two_stage_sum(k), k.sum(axis=0, dtype=np.float64).astype(np.float32)), n
        x = r.uniform(0.0, 0.29, (n, 2)).astype(np.float32)
        want = x.sum(axis=0, dtype=np.float64)
        # a lane's trips, 6 butterfly steps and 3 wave adds, twice
        path = -(-n // (RC.blocks(n) * RC.THREADS)) + 9 + -(-RC.blocks(n) // RC.THREADS) + 9
        assert (np.abs(RC.two_stage_sum(x) - want) <= path * 2.0 ** -24 * want).all(), n


def test_grid_and_trips_of_the_shapes():
    """What each shape is there for."""
    g = [RC.blocks(h * w) for h, w in RC.SHAPES]
    assert g == [1, 2, 301, 1024]
    assert 257 % 64 == 1  # a partial wave in the second workgroup
    assert 256 < g[2] < 512  # lanes 0 .. 44 of the column sum make a second trip
    assert 262_444 - 1024 * 256 == 300  # 300 lanes make a second grid-stride trip


@pytest.mark.parametrize("H,W", RC.LARGE)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_seeds_discriminate(H, W, C):
    alt, uv, a, b = RC.inputs(H, W, C)
    for mode in (RC.MODE_SUN, RC.MODE_RANDOM) if C == 3 else (RC.MODE_RANDOM,):
        good, m = RC.masked_l1(mode, alt, uv, a, b)
        assert 0 < good[2] < H * W and good[2] == m.sum()
        for name, order in WRONG.items():
            bad, _ = RC.masked_l1(mode, alt, uv, a, b, **order)
            assert bad[2] == good[2]
            assert bits(bad[1]) != bits(good[1]), f"S_rgb / N, mode {mode}: {name} gives the same bits"
            if C == 3:  # (S_alt does not depend on the planes: once per mode)
                assert bits(bad[0]) != bits(good[0]), f"S_alt / N, mode {mode}: {name} gives the same bits"


@pytest.mark.parametrize("H,W", RC.SHAPES)
def test_inputs_mask_every_condition(H, W):
    alt, uv, a, b = RC.inputs(H, W, 3)
    n = H * W
    for mode in (RC.MODE_SUN, RC.MODE_RANDOM):
        assert RC.mask(mode, alt, uv).any()
    if n > 256:
        assert (np.abs(alt) >= 0.30).any() and (np.abs(uv[..., 0]) >= 1).any() and (np.abs(uv[..., 1]) >= 1).any()
        assert (alt < -1e-2).any() and (alt > 0).any()
