"""CPU: the float64 oracle of the fused encoders (tests/flowenc_cases.py) against raft.FeatureEncoder.forward, and the
condition under which the statistics' bound of tests/test_gpu_flowenc.py holds, on the case generator's own maps."""
import copy

import pytest
import torch

import flowenc_cases as ec


@pytest.mark.parametrize("image", ec.ENCODER_IMAGES + ((1, 3, 9, 9), (2, 3, 16, 16)), ids=lambda s: "x".join(map(str, s)))
def test_encoder_oracle_is_the_module_in_float64(image):
    """The header's statement, unit by unit (conv -> statistics -> (v - mean) rstd -> ReLU; relu(S + y) with the three
    shortcut forms; the head), is what the torch modules compute: within 1e-12 relative for both encoders of raft_small()."""
    from eogs2_amd import raft

    torch.manual_seed(70)
    model = raft.raft_small(corr="volume", update="torch").eval()
    g = torch.Generator().manual_seed(71)
    x = (torch.rand(*image, generator=g) * 2 - 1).double()
    with torch.inference_mode():
        for enc, norm in ((model.feature_encoder, True), (model.context_encoder, False)):
            e64 = copy.deepcopy(enc).double()
            want, got = e64(x), ec.encoder_oracle(e64, x, norm)
            assert got.shape == want.shape
            diff, scale = float((got - want).abs().max()), float(want.abs().max())
            print(f"encoder oracle {image} norm={norm}: largest difference {diff:.3e} on values up to {scale:.3f}")
            assert diff <= 1e-12 * scale


def test_strided_oracle_reads_what_a_strided_convolution_reads():
    """out(y, x) reads in(s y + ky - p, s x + kx - p): a unit impulse at the last input position of an odd map reaches the
    last output through the tap (p, p) under stride 2, and an impulse at an odd position is not read by a 1 x 1 at all."""
    w = torch.arange(9, dtype=torch.float64).view(1, 1, 3, 3)
    x = torch.zeros(1, 5, 7, 1, dtype=torch.float64)
    x[0, 4, 6, 0] = 1.0
    out = ec.strided_oracle(x, w, None, stride=2)
    assert out.shape == (1, 3, 4, 1) and float(out[0, 2, 3, 0]) == 4.0 and float(out.abs().sum()) == 4.0
    x = torch.zeros(1, 5, 7, 1, dtype=torch.float64)
    x[0, 1, 1, 0] = 1.0
    assert float(ec.strided_oracle(x, torch.ones(1, 1, 1, 1, dtype=torch.float64), None, stride=2).abs().sum()) == 0.0
    assert float(ec.strided_oracle(x, w, None, stride=2)[0, 0, 0, 0]) == 8.0  # in(1, 1) = out(0, 0)'s tap (2, 2)


@pytest.mark.parametrize("config", ec.CONFIGS, ids=ec.config_id)
def test_statistics_cases_meet_the_condition_of_their_bound(config):
    """|mean - mean64| <= U |mean64| + 2^-31 mean|v| and |rstd - rstd64| <= 4 U rstd64 are derived for maps with
    var >= 2^-8 E[v^2] and at most 2^22 positions. The maps the GPU test takes statistics of are the
    generator's: asserted here on the float64 side, as a condition on the inputs."""
    for shape in ec.STATS_SHAPES + (ec.tile_input(config, 16, 8),):
        x, weight, bias, _, _ = ec.conv_case(config, shape, seed=500 + shape[1])
        v = ec.strided_oracle(x.double(), weight.double(), bias.double(), stride=config[3], in_nchw=config[4])
        assert v.shape[1] * v.shape[2] <= 2 ** 22
        if v.shape[1] * v.shape[2] == 1:
            continue  # (a single position has no variance: the GPU test takes no statistics there)
        ratio = ec.stats_condition(v.float())
        assert ratio >= 2.0 ** -8, (shape, ratio)
