"""CPU: the float64 oracle of the correlation lookup and the flow upsampling (tests/raft_cases.py) pinned against itself:
its two statements of the lookup — RAFT's materialised volume read through grid_sample, and pooled features with
(2r+2)^2 dots and a shared-fraction blend — agree within 1e-12 on every map and flow family, the convex upsampling equals
its unfold statement, and the plain-torch forms the package keeps for its CPU path (eogs2_amd.raft.volume_*) are the same
functions."""
import pytest
import torch

import raft_cases as rc


@pytest.mark.parametrize("shape", rc.MAPS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_two_statements_of_the_lookup_agree(shape, family):
    N, h, w = shape
    C, r = rc.CPU_CONFIG
    f1, f2 = rc.features(N, C, h, w, seed=3)
    c = rc.coords(family, N, h, w)
    vol = rc.lookup_volume(f1, f2, c, r)
    pooled, all_outside = rc.lookup_pooled(f1, f2, c, r)
    assert vol.shape == pooled.shape == (N, rc.LEVELS * (2 * r + 1) ** 2, h, w)
    assert float((vol - pooled).abs().max()) <= 1e-12
    assert float(pooled[all_outside].abs().max() if all_outside.any() else 0.0) == 0.0  # exactly 0 where every corner is outside
    mag, _ = rc.lookup_pooled(f1, f2, c, r, magnitude=True)
    assert bool((pooled.abs() <= mag * (1 + 1e-12) + 1e-300).all())  # M bounds the value it scales the error of
    if family in ("zero", "smooth"):
        assert float(pooled.abs().max()) > 0.1  # (the cases are not vacuous)
    if family == "far":
        assert float(all_outside.double().mean()) > 0.5  # most windows lie outside


def test_radius_four_and_the_families_cover_what_they_claim():
    N, h, w = 1, 17, 19
    f1, f2 = rc.features(N, 8, h, w, seed=4)
    for family in rc.FAMILIES:
        c = rc.coords(family, N, h, w)
        assert c.dtype == torch.float32 and c.shape == (N, 2, h, w)
        assert float((rc.lookup_volume(f1, f2, c, 4) - rc.lookup_pooled(f1, f2, c, 4)[0]).abs().max()) <= 1e-12
    assert torch.equal(rc.coords("integers", N, h, w), rc.coords("integers", N, h, w).round())
    e = rc.coords("edges", N, h, w)
    assert set(e[:, 0].unique().tolist()) == {0.0, w - 1.0} and set(e[:, 1].unique().tolist()) == {0.0, h - 1.0}
    d = rc.coords("checker", N, h, w) - rc.coords("zero", N, h, w)
    assert float((d[..., :, 1:] - d[..., :, :-1]).abs().min()) == 2.0 * h  # neighbours differ by 2 h
    o = rc.coords("outlier", N, h, w) - rc.coords("smooth", N, h, w)
    assert int((o.abs().sum(1) > 0).sum()) == N


def test_pooling_drops_the_odd_row_and_column():
    x = torch.arange(17 * 19, dtype=torch.float64).view(1, 1, 17, 19)
    assert [tuple(rc.pool(x, l).shape[-2:]) for l in range(4)] == [(17, 19), (8, 9), (4, 4), (2, 2)]  # noqa: E741
    assert float(rc.pool(x, 1)[0, 0, 0, 0]) == (0 + 1 + 19 + 20) / 4


@pytest.mark.parametrize("shape", rc.UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_convex_upsampling_equals_its_unfold_statement(shape):
    flow, mask = rc.upsample_inputs(*shape, seed=1)
    assert torch.equal(flow, flow.float().double()) and torch.equal(mask, mask.float().double())
    a = rc.convex_unfold(flow, mask)
    b, wsum = rc.convex_direct(flow, mask)
    assert a.shape == b.shape == (shape[0], 2, 8 * shape[1], 8 * shape[2])
    assert float((a - b).abs().max()) <= 1e-13
    assert float((wsum - 1).abs().max()) <= 1e-14
    mag, _ = rc.convex_direct(flow, mask, magnitude=True)
    assert bool((b.abs() <= mag * (1 + 1e-12)).all())


def test_package_keeps_the_same_plain_torch_forms():
    """eogs2_amd.raft's volume path (its CPU path, and the float64 arbiter of the network test) is the oracle's volume
    statement; its convex upsampling the unfold statement."""
    from eogs2_amd import raft

    N, h, w = 2, 24, 40
    f1, f2 = rc.features(N, 8, h, w, seed=5)
    for family in ("smooth", "far"):
        c = rc.coords(family, N, h, w).double()
        got = raft.volume_lookup(raft.volume_pyramid(f1, f2, rc.LEVELS), c, 3)
        assert float((got - rc.lookup_volume(f1, f2, c, 3)).abs().max()) <= 1e-13
    flow, mask = rc.upsample_inputs(1, 5, 7, seed=2)
    assert float((raft.convex_upsample_torch(flow, mask) - rc.convex_unfold(flow, mask)).abs().max()) <= 1e-14
