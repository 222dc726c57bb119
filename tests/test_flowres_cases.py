"""CPU: the case table and the float64 oracles of RAFT-large's fused encoders (tests/flowres_cases.py) against the module tree
and the modules' own forward, and the magnitude of the outputs the GPU ratio tests compare against."""
import copy

import pytest
import torch
import torch.nn.functional as F

import flowres_cases as rc


def ids(s):
    return "x".join(map(str, s))


def large(seed=90):
    from eogs2_amd import raft

    torch.manual_seed(seed)
    model = raft.raft_large(corr="volume", update="torch").eval()
    assert rc.randomise_batchnorms(model, seed + 1) == 15
    return model


def test_the_case_table_is_every_convolution_of_the_two_encoders():
    model = large()
    feature, context = rc.encoder_convs(model.feature_encoder), rc.encoder_convs(model.context_encoder)
    assert len(feature) == len(context) == 16 and feature == context
    assert set(feature) == set(rc.CASES) and len(set(rc.CASES)) == len(rc.CASES) == 9


def test_randomised_batchnorms_are_no_identity():
    model = large()
    norms = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(norms) == 15 and not any(m.training for m in norms)
    for m in norms:
        g = m.weight.detach()
        C = g.numel()
        assert int((g == 0).sum()) == C // 16 and int((g < 0).sum()) == C // 4
        assert float(g.abs().max()) <= 1.5 and float(g.abs()[g != 0].min()) >= 0.5
        assert 0.5 <= float(m.running_var.min()) and float(m.running_var.max()) <= 2.0
        assert float(m.bias.detach().abs().max()) > 0 and float(m.running_mean.abs().max()) > 0


@pytest.mark.parametrize("config", rc.CASES, ids=lambda c: f"{c[0]}to{c[1]}k{c[2]}s{c[3]}")
def test_statistics_cases_meet_the_condition_of_their_bound(config):
    """tests/test_flowenc_cases.py's condition (var >= 2^-8 E[v^2], at most 2^22 positions) on the maps the GPU test of this
    table takes statistics of."""
    from test_flowenc_cases import test_statistics_cases_meet_the_condition_of_their_bound as check

    check(config)


@pytest.mark.parametrize("shape", rc.FOLD_SHAPES, ids=ids)
def test_fold_oracle_is_the_batch_norm_of_the_convolution(shape):
    """conv(x, w', b') with the folded parameters is norm(conv(x, w, b)) of an eval-mode BatchNorm2d: in float64 up to the two
    float32 roundings of the statement (s and w'), 2^-22 of the terms' magnitude."""
    cout, per_out = shape
    weight, bias, gamma, beta, mean, var = rc.fold_case(cout, per_out, seed=400 + cout)
    s, w2, b2 = rc.fold_oracle(weight, bias, gamma, beta, mean, var)
    assert s.dtype == w2.dtype == torch.float32 and b2.dtype == torch.float64
    assert bool((s[::16] == 0).all()) and bool((w2[::16] == 0).all()) and torch.equal(b2[::16], beta.double()[::16])
    g = torch.Generator().manual_seed(401)
    x = torch.randn(2, per_out, 3, 4, generator=g, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(cout).double().eval()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(mean)
        bn.running_var.copy_(var)
        want = bn(F.conv2d(x, weight.double(), bias.double()))
        got = F.conv2d(x, w2.double(), b2)
        mag = F.conv2d(x.abs(), w2.double().abs(), b2.abs()) + (bias.double().abs() + mean.double().abs()).view(1, -1, 1, 1) * s.double().abs().view(1, -1, 1, 1)
    assert bool(((got - want).abs() <= 2.0 ** -22 * mag + 1e-300).all())


@pytest.mark.parametrize("kind", ["feature", "context"])
@pytest.mark.parametrize("where", ["layer1.1", "layer2.0", "layer3.0"])
def test_block_oracle_is_the_module_in_float64(where, kind):
    model = large()
    block = copy.deepcopy(getattr(model, f"{kind}_encoder").get_submodule(where)).double()
    g = torch.Generator().manual_seed(91)
    cin = block.convnormrelu1[0].in_channels
    x = torch.relu(torch.randn(2, cin, 17, 23, generator=g)).double()
    with torch.inference_mode():
        want, got = block(x.clone()), rc.residual_block_oracle(block, x)
    diff, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"block oracle {kind} {where}: largest difference {diff:.3e} on values up to {scale:.3f}")
    assert got.shape == want.shape and diff <= 1e-12 * scale


@pytest.mark.parametrize("image", rc.ENCODER_IMAGES + ((1, 3, 9, 9),), ids=ids)
def test_encoder_oracle_is_the_module_in_float64_and_its_output_is_of_order_ten(image):
    """The header's statement, unit by unit, is what the torch modules compute, within 1e-12 relative for both encoders of
    raft_large() with randomised batch norms in eval mode. The outputs stay between 1 and 100 in magnitude: the GPU tests'
    ratios to torch float32's own deviation compare against something."""
    model = large()
    g = torch.Generator().manual_seed(92)
    x = (torch.rand(*image, generator=g) * 2 - 1).double()
    with torch.inference_mode():
        for kind in ("feature", "context"):
            e64 = copy.deepcopy(getattr(model, f"{kind}_encoder")).double()
            want, got = e64(x), rc.encoder_oracle(e64, x)
            diff, scale = float((got - want).abs().max()), float(want.abs().max())
            print(f"encoder oracle {kind} {image}: largest difference {diff:.3e} on values up to {scale:.3f}")
            assert got.shape == want.shape == (image[0], 256, -(-image[2] // 8), -(-image[3] // 8))
            assert diff <= 1e-12 * scale and 1.0 <= scale <= 100.0
