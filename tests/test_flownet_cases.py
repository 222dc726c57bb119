"""CPU: the float64 oracle of the fused update (tests/flownet_cases.py) against raft.UpdateBlock.forward in float64. Float64
rounding is the only difference, so this proves the hoisting identity (the context's share of the GRU convolutions as a plane)
and the channel slices of convz / convr / convq before any kernel is involved."""
import pytest
import torch

import flownet_cases as fc


@pytest.mark.parametrize("shape", fc.STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_update_oracle_is_the_update_block(shape):
    from eogs2_amd import raft

    torch.manual_seed(50)
    block = raft.raft_small().double().eval().update_block
    hidden, context, corr, flow = (t.double() for t in fc.update_inputs(*shape, seed=51))
    with torch.inference_mode():
        want_h, want_d = block(hidden, context, corr, flow)
        got_h, got_d = fc.update_oracle(block, hidden, context, corr, flow)
    for name, got, want in (("hidden", got_h, want_h), ("delta", got_d, want_d)):
        assert got.shape == want.shape
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"update oracle {shape} {name}: {err:.3e} of {scale:.3e}")
        assert scale > 0 and err <= 1e-12 * scale


def test_conv_oracle_concatenates_and_bounds():
    cfg = fc.CONFIGS[5]
    inputs, weight, bias, add = fc.conv_case(cfg, (2, 5, 7), seed=52)
    d = [t.double() for t in inputs]
    out = fc.conv_oracle(d, weight.double(), bias.double(), "none", add.double())
    mag = fc.conv_oracle(d, weight.double(), bias.double(), "none", add.double(), magnitude=True)
    assert out.shape == mag.shape == (2, 5, 7, cfg[1]) and bool((out.abs() <= mag).all())
    # the second segment's channels meet the weight's channels 96.. : zeroing them equals dropping the segment
    w0 = weight.double().clone()
    w0[:, 96:] = 0
    assert torch.allclose(fc.conv_oracle(d, w0, None), fc.conv_oracle(d[:1], weight.double()[:, :96], None), rtol=0, atol=1e-12)
    assert bool((fc.conv_oracle(d, weight.double(), bias.double(), "relu") >= 0).all())
