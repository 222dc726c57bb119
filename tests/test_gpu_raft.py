"""GPU (MI355X): the flow network's three HIP operators (eogs2_amd.raft over eogs2_amd/csrc/raft.hip) against the float64
oracle of tests/raft_cases.py, element by element and under derived bounds; the staged and the direct path of the lookup
bit for bit; the whole network against its own float64 run, with the plain-torch float32 volume path as the yardstick;
and the network behind performOpticalmatching."""
import pytest
import torch

import raft_cases as rc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # half an ulp of 1: the unit of every bound below


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def ids(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("config", rc.CONFIGS, ids=ids)
@pytest.mark.parametrize("shape", rc.MAPS, ids=ids)
def test_pyramid_against_float64(dev, shape, config):
    """Level l within 3 l 2^-24 pool_l(|fmap2|) per element: three roundings per pooling step ((a + b) + (c + d), the
    quarter is exact). Level 0 is a copy: exact."""
    from eogs2_amd import raft

    (N, h, w), (C, _r) = shape, config
    f2 = rc.features(N, C, h, w, seed=7)[1].float().to(dev)
    pyr = raft.corr_pyramid(f2, rc.LEVELS)
    worst = 0.0
    for l in range(rc.LEVELS):  # noqa: E741
        got = pyr.level(l).double()
        want = rc.pool(f2.double(), l).permute(0, 2, 3, 1)
        bound = 3 * l * U * rc.pool(f2.double().abs(), l).permute(0, 2, 3, 1)
        assert got.shape == want.shape == (N, h >> l, w >> l, C)
        err = (got - want).abs()
        assert bool((err <= bound).all()), f"level {l}: {float((err - bound).max()):.3e} over the bound"
        if l:
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    one = raft.corr_pyramid(f2, 1)
    assert torch.equal(one.level(0), f2.permute(0, 2, 3, 1))
    again = raft.corr_pyramid(f2, rc.LEVELS, out=pyr)
    assert again is pyr
    print(f"pyramid {shape} C={C}: largest multiple of the bound {worst:.3f}")


@pytest.mark.parametrize("config", rc.CONFIGS, ids=ids)
@pytest.mark.parametrize("shape", rc.MAPS, ids=ids)
def test_lookup_against_float64(dev, shape, config):
    """Every element of every family: |hip - f64| <= (C + 3 l + 8) 2^-24 M, M the same blend of sum_c |fmap1_c|
    pool_l(|fmap2|)_c / sqrt(C) in float64: the standard bound of a length-C float32 dot product, the pooling's three
    roundings per level, and the blend and the scale. Exactly 0 where all four corners lie outside. The direct path
    (EOGS_RAFT_NO_STAGE) and a second run give the same bits."""
    from eogs2_amd import raft

    (N, h, w), (C, r) = shape, config
    f1, f2 = (t.float().to(dev) for t in rc.features(N, C, h, w, seed=11))
    f1cl, pyr = raft.corr_pyramid(f1, 1), raft.corr_pyramid(f2, rc.LEVELS)
    K = 2 * r + 1
    level = rc.lookup_level_of_channel(r).to(dev)
    factor = ((C + 3 * level + 8).double() * U).view(1, -1, 1, 1)
    worst = {}
    for family in rc.FAMILIES:
        c = rc.coords(family, N, h, w).to(dev)
        got = raft.corr_lookup(f1cl, pyr, c, r)
        assert got.shape == (N, rc.LEVELS * K * K, h, w) and got.dtype == torch.float32
        want, all_outside = rc.lookup_pooled(f1.double(), f2.double(), c, r)
        mag, _ = rc.lookup_pooled(f1.double(), f2.double(), c, r, magnitude=True)
        err = (got.double() - want).abs()
        bound = factor * mag
        assert bool((err <= bound).all()), f"{family}: {float((err - bound).max()):.3e} over the bound"
        assert bool((got[all_outside] == 0).all()), f"{family}: an element with every corner outside is not exactly 0"
        worst[family] = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
        direct = raft.corr_lookup(f1cl, pyr, c, r, no_stage=True)
        assert torch.equal(got, direct), f"{family}: the staged and the direct path differ"
        assert torch.equal(got, raft.corr_lookup(f1cl, pyr, c, r)), f"{family}: two runs differ"
    print(f"lookup {shape} C={C} r={r}: largest multiple of the bound per family " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


def test_lookup_zeroes_what_is_not_a_coordinate(dev):
    """NaN and +-inf coordinates: every tap outside, weight 0, the pixel's outputs exactly 0; its neighbours untouched."""
    from eogs2_amd import raft

    N, h, w, C, r = 1, 16, 16, 128, 3
    f1, f2 = (t.float().to(dev) for t in rc.features(N, C, h, w, seed=13))
    f1cl, pyr = raft.corr_pyramid(f1, 1), raft.corr_pyramid(f2, rc.LEVELS)
    c = rc.coords("smooth", N, h, w).to(dev)
    clean = raft.corr_lookup(f1cl, pyr, c, r)
    bad = c.clone()
    bad[0, 0, 3, 4], bad[0, 1, 5, 6], bad[0, 0, 7, 8], bad[0, 1, 9, 10] = float("nan"), float("inf"), float("-inf"), 1e30
    for no_stage in (False, True):
        got = raft.corr_lookup(f1cl, pyr, bad, r, no_stage=no_stage)
        hit = torch.zeros(h, w, dtype=torch.bool, device=dev)
        for y, x in ((3, 4), (5, 6), (7, 8), (9, 10)):
            assert bool((got[0, :, y, x] == 0).all())
            hit[y, x] = True
        assert torch.equal(got[0][:, ~hit], clean[0][:, ~hit])


@pytest.mark.parametrize("shape", rc.UP_SHAPES, ids=ids)
def test_upsampling_against_float64(dev, shape):
    """In units of 2^-24 sum_k w_k |u_k| (u = 8 flow, exact).

    Convex, 32 units, for mask logits in [-4, 4]: v - max lies in [-8, 0], its rounding is at most half an ulp of 8 = 4
    units of 2^-24 absolute, which is the relative error it leaves in e_k; expf is documented at 1 ulp = 2 units; so e_k
    carries 6. The numerator sum_k e_k u_k adds 1 per product and 8 for its eight additions: 15. The denominator, a sum of
    nine positive terms, carries 6 + 8 = 14. The division adds 1: 30, rounded up to 32.

    Bilinear, 8 units: the source position is split into integer and fraction in integer arithmetic, so each of the four
    1-D weights is one rounded division (1); hx v (+1), the row's addition (+1), hy row (+1 for hy, +1), the final addition
    (+1): 6, rounded up to 8; the factor 8 is exact.

    The convex weights sum to 1: with 8 flow = 1 everywhere the interior outputs are 1 within the convex bound."""
    from eogs2_amd import raft

    N, h, w = shape
    flow, mask = rc.upsample_inputs(N, h, w, seed=5)
    f32, m32 = flow.float().to(dev), mask.float().to(dev)
    got = raft.upsample_flow(f32, m32)
    want, _ = rc.convex_direct(flow.to(dev), mask.to(dev))
    mag, _ = rc.convex_direct(flow.to(dev), mask.to(dev), magnitude=True)
    assert got.shape == want.shape == (N, 2, 8 * h, 8 * w)
    err = (got.double() - want).abs()
    assert bool((err <= 32 * U * mag).all()), f"convex: {float((err / mag.clamp_min(1e-300)).max() / U):.2f} units"
    worst_c = float((err / mag.clamp_min(1e-300))[mag > 0].max() / U)
    assert torch.equal(got, raft.upsample_flow(f32, m32))

    got = raft.upsample_flow(f32)
    want, mag = rc.bilinear(flow.to(dev)), rc.bilinear(flow.to(dev), magnitude=True)
    err = (got.double() - want).abs()
    # (float64's own coordinate arithmetic: a relative 2^-52 of the position, times the largest slope)
    slack = 1e-12 * float(flow.abs().max()) * 8
    assert bool((err <= 8 * U * mag + slack).all()), f"bilinear: {float(((err - slack) / mag.clamp_min(1e-300)).max() / U):.2f} units"
    worst_b = float((err / mag.clamp_min(1e-300))[mag > 1e-6].max() / U) if bool((mag > 1e-6).any()) else 0.0
    print(f"upsampling {shape}: convex {worst_c:.2f} of 32 units, bilinear {worst_b:.2f} of 8 units")

    ones = raft.upsample_flow(torch.full_like(f32, 0.125), m32)
    if h > 2 and w > 2:
        inner = ones[:, :, 8:-8, 8:-8]
        assert float((inner.double() - 1).abs().max()) <= 32 * U


@pytest.mark.parametrize("size", [(128, 128), (128, 136)], ids=ids)
@pytest.mark.parametrize("name", ["small", "large"])
def test_network_against_its_float64_run(dev, name, size):
    """Seeded random weights, eval mode, 4 updates, three runs on the device: on-demand (the HIP operators), the plain-torch
    volume path in float32, and the volume path in float64, which arbitrates. The on-demand flow's largest deviation from
    float64 may be at most 16 x the float32 volume path's own: the margin this project gives a float32 reference's error."""
    from eogs2_amd import raft

    torch.manual_seed(20)
    model = raft.RAFT(name, corr="volume").eval().to(dev)
    g = torch.Generator().manual_seed(21)
    H, W = size
    base = torch.rand(1, 3, H + 8, W + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev)  # the second image: the first, shifted
    with torch.inference_mode():
        model.corr = "ondemand"
        od = model(a, b, num_flow_updates=4, return_all=True)
        od_last = model(a, b, num_flow_updates=4)
        model.corr = "volume"
        v32 = model(a, b, num_flow_updates=4, return_all=True)
        m64 = model.double()
        v64 = m64(a.double(), b.double(), num_flow_updates=4, return_all=True)
    assert len(od) == len(v32) == len(v64) == 4 and len(od_last) == 1
    for f in od:
        assert f.shape == (1, 2, H, W) and f.dtype == torch.float32 and bool(torch.isfinite(f).all())
    dev_od = float((od[-1].double() - v64[-1]).abs().max())
    dev_vol = float((v32[-1].double() - v64[-1]).abs().max())
    print(f"network {name} {size}: |ondemand - f64| {dev_od:.3e}, |volume32 - f64| {dev_vol:.3e}, ratio {dev_od / max(dev_vol, 1e-300):.3f}, "
          f"largest |flow| {float(v64[-1].abs().max()):.3f}")
    assert dev_od <= 16 * dev_vol
    assert float((od_last[-1].double() - v64[-1]).abs().max()) <= 16 * dev_vol


@pytest.mark.parametrize("mode", ["downscale", "upscale"])
def test_network_behind_perform_optical_matching(dev, mode):
    from eogs2_amd import flow as F
    from eogs2_amd import raft

    torch.manual_seed(30)
    model = raft.raft_small().eval().to(dev)
    g = torch.Generator().manual_seed(31)
    gt, img = torch.rand(3, 130, 150, generator=g).to(dev), torch.rand(3, 130, 150, generator=g).to(dev)
    warper = F.performOpticalmatching(False, mode=mode, model_name="small", num_flow_updates=2, model=model)
    flow, gt2, img2 = warper.get_flow(gt, img)
    assert gt2.shape == img2.shape == ((3, 128, 144) if mode == "downscale" else (3, 130, 150))
    assert flow.shape == (1, 2) + tuple(gt2.shape[1:]) and flow.dtype == torch.float32 and bool(torch.isfinite(flow).all())
    cst = F.performOpticalmatching(True, mode=mode, model_name="small", num_flow_updates=2, model=model)
    flow_c, _, _ = cst.get_flow(gt, img)
    assert flow_c.shape == flow.shape and flow_c.stride()[2:] == (0, 0)
    warped = warper.apply_flow(img2, flow)
    assert warped.shape == img2.shape


def test_example_flow_network(dev):
    """examples/train_synthetic.py --flow-matching --flow-network small: the network takes the stand-in's place behind the same
    performOpticalmatching. With random weights this is the plumbing alone (the criterion decides about random flows): the
    run finishes with finite losses."""
    import math
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    first, last = train_synthetic.main(["--gaussians", "5000", "--size", "128", "--iters", "6", "--quiet", "--flow-matching",
                                        "--flow-network", "small"])[:2]
    assert math.isfinite(first) and math.isfinite(last)
