"""CPU: the float64 oracles of RAFT-large's fused update (tests/flownet_large_cases.py) before any kernel is involved.
update_large_oracle against raft.UpdateBlock.forward and raft.MaskPredictor.forward in float64: float64 rounding is the only
difference, so this proves the hoisting identity for both GRUs (the context's share of their six convolutions as four
planes), the channel slices of [h | context | motion | flow] and the 0.25 on the mask. conv_rect_oracle against F.conv2d with
the rectangular padding. And the rectangular general cases reach what their comments name, by the library's packing sizes."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import flownet_cases as fc
import flownet_large_cases as lc


@pytest.mark.parametrize("shape", lc.STEP_SHAPES + ((1, 3, 9), (1, 7, 3)), ids=lambda s: "x".join(map(str, s)))
def test_update_large_oracle_is_the_update_block_and_the_mask_predictor(shape):
    from eogs2_amd import raft

    torch.manual_seed(70)
    model = raft.raft_large().double().eval()
    block, predictor = model.update_block, model.mask_predictor
    hidden, context, corr, flow = (t.double() for t in lc.update_large_inputs(*shape, seed=71))
    with torch.inference_mode():
        want_h, want_d = block(hidden, context, corr, flow)
        want_m = predictor(want_h)
        got_h, got_d, got_m = lc.update_large_oracle(block, predictor, hidden, context, corr, flow)
    N, h, w = shape
    assert got_m.shape == (N, lc.MASK, h, w) and got_h.shape == (N, lc.HIDDEN, h, w) and got_d.shape == (N, 2, h, w)
    for name, got, want in (("hidden", got_h, want_h), ("delta", got_d, want_d), ("mask", got_m, want_m)):
        assert got.shape == want.shape
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"update_large oracle {shape} {name}: {err:.3e} of {scale:.3e}")
        assert scale > 0 and err <= 1e-12 * scale
    assert not torch.equal(got_h, hidden)


@pytest.mark.parametrize("config", lc.CONFIGS + lc.GENERAL, ids=lc.config_id)
def test_conv_rect_oracle_is_conv2d(config):
    segs, cout, (kh, kw), with_add, act, _ = config
    inputs, weight, bias, add = lc.conv_rect_case(config, (2, 5, 7), seed=72)
    d = [t.double() for t in inputs]
    got = lc.conv_rect_oracle(d, weight.double(), bias.double(), act, None if add is None else add.double())
    x = torch.cat(d, dim=3).permute(0, 3, 1, 2)
    want = F.conv2d(x, weight.double(), bias.double(), stride=1, padding=((kh - 1) // 2, (kw - 1) // 2))
    assert want.shape == (2, cout, 5, 7)  # the padding keeps the map's size
    if add is not None:
        want = want + add.double().permute(0, 3, 1, 2)
    want = torch.relu(want) if act == "relu" else 0.25 * want if act == "quarter" else want
    assert torch.equal(got, want.permute(0, 2, 3, 1))
    mag = lc.conv_rect_oracle(d, weight.double(), bias.double(), act, None if add is None else add.double(), magnitude=True)
    plain = lc.conv_rect_oracle(d, weight.double(), bias.double(), "none", None if add is None else add.double())
    assert mag.shape == got.shape and bool((plain.abs() <= mag * (1 + 1e-12)).all())
    if kh == kw:  # a square weight: the square oracle
        assert torch.equal(plain, fc.conv_oracle(d, weight.double(), bias.double(), "none", None if add is None else add.double()))


def test_conv_rect_oracle_orients_its_taps():
    """A 1 x 5 weight that is 1 at tap kx shifts the map by kx - 2 columns, a 5 x 1 by ky - 2 rows, zeros shifted in."""
    g = torch.Generator().manual_seed(73)
    x = torch.randn(1, 6, 7, 1, generator=g).double()
    for t in range(5):
        wt = torch.zeros(1, 1, 1, 5, dtype=torch.float64)
        wt[0, 0, 0, t] = 1
        want = torch.zeros_like(x)
        s = t - 2  # out(y, x) = in(y, x + s)
        want[:, :, max(0, -s):7 - max(0, s)] = x[:, :, max(0, s):7 - max(0, -s)]
        assert torch.equal(lc.conv_rect_oracle([x], wt, None), want), t
        want = torch.zeros_like(x)
        want[:, max(0, -s):6 - max(0, s)] = x[:, max(0, s):6 - max(0, -s)]
        assert torch.equal(lc.conv_rect_oracle([x], wt.permute(0, 1, 3, 2).contiguous(), None), want), t


@pytest.fixture(scope="module")
def lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def rect_floats(lib, segs, cout, kh, kw):
    n = ctypes.c_size_t()
    lib.check(lib.flowrect_pack_bytes(kh, kw, len(segs), (ctypes.c_int * len(segs))(*segs), cout, ctypes.byref(n)))
    assert n.value % 4 == 0
    return n.value // 4


def test_the_cases_reach_what_they_claim(lib):
    """The tables' comments as assertions. A rectangular packing is [chunk][workgroup along Cout][kh kw taps][8][row]: its size
    is a square packing's with kh kw in place of k k, so the plan (blocks per workgroup, workgroups) is the square one's."""
    for c in lc.CONFIGS + lc.GENERAL + lc.GATE_CONFIGS:
        segs, cout, (kh, kw) = c[:3]
        assert (kh, kw) in lc.TAP_SHAPES
        chunks, blocks = sum(-(-s // fc.CHUNK) for s in segs), -(-cout // fc.BLOCK)
        floats = rect_floats(lib, segs, cout, kh, kw)
        row = 16 if blocks == 1 else 48
        assert floats % (chunks * kh * kw * fc.CHUNK * row) == 0
        workgroups = floats // (chunks * kh * kw * fc.CHUNK * row)
        assert workgroups in (1,) if blocks == 1 else workgroups in (-(-blocks // 2), -(-blocks // 3)), c
        if kh == kw:  # the square entry's size
            n = ctypes.c_size_t()
            lib.check(lib.flownet_conv_pack_bytes(kh, len(segs), (ctypes.c_int * len(segs))(*segs), cout, ctypes.byref(n)))
            assert n.value == 4 * floats
    g = lc.GENERAL
    assert g[0][0] == g[1][0] == (5, 9, 1) and g[0][1] == g[1][1] == 33 and (g[0][2], g[1][2]) == ((1, 5), (5, 1))
    assert rect_floats(lib, *g[0][:2], 1, 5) == 4 * 1 * 5 * 8 * 48  # four chunks, one workgroup of three blocks (15 padded columns)
    assert g[2][:3] == ((4,), 1, (5, 1)) and rect_floats(lib, (4,), 1, 5, 1) == 5 * 8 * 16
    assert g[3][0] == (12,) and g[3][2] == (1, 5) and -(-g[3][1] // 16) == 7
    assert rect_floats(lib, (12,), 112, 1, 5) == 2 * 4 * 5 * 8 * 48  # two chunks, four workgroups of two blocks: the eighth block is padding
    assert {c[2] for c in lc.CONFIGS} == {(1, 1), (3, 3), (7, 7), (1, 5), (5, 1)}
    assert sum(c[5] for c in lc.CONFIGS) == 2 and [c[4] for c in lc.CONFIGS].count("quarter") == 1
    for c in lc.GATE_CONFIGS:
        assert c[4] in ("gates", "gru") and c[2] in ((1, 5), (5, 1)) and (c[1] % 2 == 0 or c[4] == "gru")
    assert any(s[2] < 5 for s in lc.SHAPES) and any(s[1] < 5 for s in lc.SHAPES)  # narrower than 1 x 5, shorter than 5 x 1
