"""GPU (MI355X): RAFT-large's fused update block (eogs2_amd.raft.conv2d_rect_cl / FusedUpdateLarge / RAFT(update="fused_large")
over eogs2_amd/csrc/flownet.hip, the entries of include/eogs_resample.h) against the float64 oracles of
tests/flownet_large_cases.py: every convolution of RAFT-large's update and mask head per element under the bound of a float32
fma sum, the rectangular kernel's exact cases bit for bit (a square pair is the square entry, an impulse weight is a shift, a
NaN reaches the kernel's own footprint), the gate epilogues at 1 x 5 and 5 x 1, one update and three chained updates and the
whole network against their float64 runs with torch's float32 modules as the yardstick, and the example."""
import copy
import math
import os
import sys

import pytest
import torch

import flownet_large_cases as lc
from test_gpu_flownet import U, dev, ids, run_conv, seg_array, tile_shape  # noqa: F401
from test_gpu_flownet_general import HIGHER, guarded, ulp_of

pytestmark = pytest.mark.gpu

shape_id = lambda s: s if isinstance(s, str) else ids(s)  # noqa: E731
EPILOGUES = {"none": "FLOWNET_EPI_BIAS", "relu": "FLOWNET_EPI_RELU", "gates": "FLOWNET_EPI_GATES", "gru": "FLOWNET_EPI_GRU",
             "quarter": "FLOWRECT_EPI_QUARTER"}


def resolve(shape):
    return tile_shape() if shape == "tile" else shape


def new_rect_packing(dev, chans, cout, kh, kw):
    """A packing of the library's size with every byte 0xFF (a NaN in every float): what a call does not write shows."""
    from eogs2_amd import _lib
    from eogs2_amd._host import query_bytes

    size = query_bytes(_lib.get(), "flowrect_pack_bytes", kh, kw, len(chans), seg_array(chans), cout)
    return torch.full((size,), 0xFF, dtype=torch.uint8, device=dev)


def rect_pack_into(packed, chans, cout, weight, cout_off=0, offsets=None):
    from eogs2_amd._host import call

    weight = weight.contiguous()
    call("eogs_flowrect_pack", packed.device, weight.shape[2], weight.shape[3], len(chans), seg_array(chans),
         None if offsets is None else seg_array(offsets), weight.shape[1], cout, cout_off, weight.shape[0], weight.data_ptr(),
         packed.data_ptr(), packed.numel())
    return packed


def run_rect(inputs, weight, bias, act="none", add=None, flags=0, aux=None, out=None, packed=None):
    """test_gpu_flownet.run_conv over the rectangular entries: `out` and the packing filled with NaN before the call; `packed`
    = (a packing made by the caller, Cout, (kh, kw)) stands in for `weight`."""
    from eogs2_amd import _abi
    from eogs2_amd._host import call

    dev = inputs[0].device
    nchw = [bool(flags >> s & 1) for s in range(len(inputs))]
    N, h, w = (inputs[0].shape[0],) + tuple(inputs[0].shape[2:] if nchw[0] else inputs[0].shape[1:3])
    chans = [t.shape[1] if f else t.shape[3] for t, f in zip(inputs, nchw)]
    for t, f, c in zip(inputs, nchw, chans):
        assert tuple(t.shape) == ((N, c, h, w) if f else (N, h, w, c))
    if packed is None:
        cout, kh, kw = weight.shape[0], weight.shape[2], weight.shape[3]
        packed = rect_pack_into(new_rect_packing(dev, chans, cout, kh, kw), chans, cout, weight)
        assert not bool((packed.view(torch.int32) == -1).any())
    else:
        packed, cout, (kh, kw) = packed
    if out is None:
        shape = (2, N, h, w, cout // 2) if act == "gates" else (N, cout, h, w) if flags & _abi.FLOWNET_OUT_NCHW else (N, h, w, cout)
        out = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    xs = [t.contiguous() for t in inputs] + [None] * (3 - len(inputs))
    call("eogs_flowrect_conv", dev, N, h, w, kh, kw, len(chans), seg_array(chans), *(None if x is None else x.data_ptr() for x in xs),
         cout, packed.data_ptr(), packed.numel(), None if bias is None else bias.data_ptr(), None if add is None else add.data_ptr(),
         None if aux is None else aux.data_ptr(), out.data_ptr(), getattr(_abi, EPILOGUES[act]), flags)
    return out


def case_on(dev, config, shape, seed):
    inputs, weight, bias, add = lc.conv_rect_case(config, shape, seed)
    return [t.to(dev) for t in inputs], weight.to(dev), bias.to(dev), None if add is None else add.to(dev)


def cl(t, out_nchw):
    """A result as [N, h, w, Cout]."""
    return t.permute(0, 2, 3, 1) if out_nchw else t


# ---- per element against float64 ----

def check_against_float64(dev, shape, config):
    """Every element: |hip - f64| <= (K + 2) 2^-24 M with K = kh kw sum C_i (+ 1 with `add`) and M = |add| + |bias| +
    conv(|x|, |W|) in float64: the standard bound of a length-K float32 fma sum in any fixed order, the bias and the plane.
    ReLU is exact given its argument, and so is the 0.25 (both sides of the bound scale by it). The wrapper gives the bits of
    the entries called by hand, a second run the same bits."""
    from eogs2_amd import _abi, raft

    shape = resolve(shape)
    segs, cout, (kh, kw), with_add, act, out_nchw = config
    inputs, weight, bias, add = case_on(dev, config, shape, seed=100 + 7 * shape[1] + shape[2])
    flags = _abi.FLOWNET_OUT_NCHW if out_nchw else 0
    raw = run_rect(inputs, weight, bias, act, add, flags=flags)
    assert raw.shape == ((shape[0], cout) + shape[1:] if out_nchw else shape + (cout,)) and raw.dtype == torch.float32 and raw.is_contiguous()
    got = cl(raw, out_nchw)
    d = [t.double() for t in inputs]
    add64 = None if add is None else add.double()
    want = lc.conv_rect_oracle(d, weight.double(), bias.double(), act, add64)
    mag = lc.conv_rect_oracle(d, weight.double(), bias.double(), act, add64, magnitude=True) * (0.25 if act == "quarter" else 1.0)
    K = kh * kw * sum(segs) + (1 if with_add else 0)
    assert bool(torch.isfinite(got).all())
    err, bound = (got.double() - want).abs(), (K + 2) * U * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"conv {lc.config_id(config)} {shape}: largest multiple of the bound {worst:.4f}")
    assert bool((err <= bound).all()), f"{float((err - bound).max()):.3e} over the bound"
    assert torch.equal(run_rect(inputs, weight, bias, act, add, flags=flags), raw)
    if act != "quarter":  # (the wrapper has the square one's two activations; it writes channel-last)
        assert torch.equal(raft.conv2d_rect_cl(inputs, weight, bias, act, add), got)
    else:
        assert torch.equal(got, 0.25 * raft.conv2d_rect_cl(inputs, weight, bias, "none", add))  # an exact scaling


@pytest.mark.parametrize("config", lc.CONFIGS, ids=lc.config_id)
@pytest.mark.parametrize("shape", lc.SHAPES + ("tile",), ids=shape_id)
def test_convolution_against_float64(dev, shape, config):
    check_against_float64(dev, shape, config)


@pytest.mark.parametrize("config", lc.GENERAL, ids=lc.config_id)
@pytest.mark.parametrize("shape", lc.GENERAL_SHAPES + ((1, 7, 3), (1, 3, 9), "tile"), ids=shape_id)
def test_general_rectangular_convolution_against_float64(dev, shape, config):
    check_against_float64(dev, shape, config)


# ---- bit for bit ----

@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_a_square_pair_is_the_square_entry(dev, k):
    """eogs_flowrect_conv with kh == kw gives eogs_flownet_conv's bits, and its packing that entry's bytes; either packing
    serves either entry. Ragged segments, a plane, ReLU; both layouts of the output."""
    from eogs2_amd import _abi, raft
    from test_gpu_flownet import new_packing, pack_into

    config = ((5, 9, 1), 33, (k, k), True, "relu", False)
    inputs, weight, bias, add = case_on(dev, config, resolve("tile"), seed=110 + k)
    segs, cout = config[0], config[1]
    sq = pack_into(new_packing(dev, segs, cout, k), segs, cout, k, weight)
    rc = rect_pack_into(new_rect_packing(dev, segs, cout, k, k), segs, cout, weight)
    assert torch.equal(sq, rc)
    for flags in (0, _abi.FLOWNET_OUT_NCHW, 5):
        xs = [t.permute(0, 3, 1, 2).contiguous() if flags >> s & 1 else t for s, t in enumerate(inputs)]
        want = run_conv(xs, weight, bias, "relu", add, flags=flags)
        assert bool(torch.isfinite(want).all())
        assert torch.equal(run_rect(xs, weight, bias, "relu", add, flags=flags), want)
        assert torch.equal(run_rect(xs, None, bias, "relu", add, flags=flags, packed=(sq, cout, (k, k))), want)
        assert torch.equal(run_conv(xs, None, bias, "relu", add, flags=flags, packed=(rc, cout, k)), want)
    assert torch.equal(raft.conv2d_rect_cl(inputs, weight, bias, "relu", add), raft.conv2d_cl(inputs, weight, bias, "relu", add))


@pytest.mark.parametrize("taps", [(1, 5), (5, 1)], ids=ids)
@pytest.mark.parametrize("shape", [(1, 7, 3), (1, 3, 9), "tile"], ids=shape_id)
def test_an_impulse_weight_is_a_shift(dev, shape, taps):
    """A weight that is 1.0 at one tap and one (input, output) channel pair reproduces the input shifted by that tap, bit for
    bit, zeros shifted in (every other product is an exact zero): the tap orientation (a cross-correlation, row-major over
    kh x kw) and the padding ((kh - 1) / 2, (kw - 1) / 2), at every tap, for a channel in each of a chunk's two instructions."""
    N, h, w = resolve(shape)
    kh, kw = taps
    g = torch.Generator().manual_seed(120)
    x = torch.randn(N, h, w, 13, generator=g).to(dev)
    for t, (ci, co) in ((t, p) for t in range(5) for p in ((2, 0), (12, 16))):
        weight = torch.zeros(17, 13, kh, kw, device=dev)
        weight.view(17, 13, 5)[co, ci, t] = 1.0
        got = run_rect([x], weight, None)
        s = t - 2
        want = torch.zeros(N, h, w, 17, device=dev)
        if kw == 5 and abs(s) < w:  # out(y, x) = in(y, x + s)
            want[:, :, max(0, -s):w - max(0, s), co] = x[:, :, max(0, s):w - max(0, -s), ci]
        if kh == 5 and abs(s) < h:
            want[:, max(0, -s):h - max(0, s), :, co] = x[:, max(0, s):h - max(0, -s), :, ci]
        assert torch.equal(got, want), (t, ci, co)


@pytest.mark.parametrize("config", [c for c in lc.CONFIGS + lc.GENERAL if c[2][0] != c[2][1]], ids=lc.config_id)
def test_a_nan_reaches_the_footprint_of_the_kernel_shape(dev, config):
    """One NaN at one input position gives NaN at exactly the output positions whose kh x kw window holds it: five in a row
    for 1 x 5, five in a column for 5 x 1 (clipped at the border), never a 5 x 5 block. In the last channel of every segment,
    at a corner and at the centre. And an all-zero input returns the bias (plus `add`) bit for bit."""
    segs, cout, (kh, kw), with_add, act, _ = config
    N, h, w = shape = resolve("tile")
    inputs, weight, bias, add = case_on(dev, config, shape, seed=200)
    zeros = [torch.zeros_like(t) for t in inputs]
    plain = bias.expand(N, h, w, cout) if add is None else bias.expand(N, h, w, cout) + add
    assert torch.equal(run_rect(zeros, weight, bias, act, add), torch.relu(plain) if act == "relu" else plain)
    for s, C in enumerate(segs):
        for y, x in ((0, 0), (h - 1, w - 1), (h // 2, w // 2)):
            xs = [t.clone() for t in inputs]
            xs[s][0, y, x, C - 1] = float("nan")
            nan = torch.isnan(run_rect(xs, weight, bias, act, add))
            foot = torch.zeros(h, w, dtype=torch.bool, device=dev)
            foot[max(0, y - kh // 2):y + kh // 2 + 1, max(0, x - kw // 2):x + kw // 2 + 1] = True
            assert int(foot.sum()) <= 5 and ((y, x) != (h // 2, w // 2) or int(foot.sum()) == 5)
            assert bool((nan == foot[None, :, :, None].expand_as(nan)).all()), (s, y, x)


@pytest.mark.parametrize("config", lc.CONFIGS + lc.GENERAL, ids=lc.config_id)
def test_a_batch_is_its_images_and_layouts_do_not_change_a_bit(dev, config):
    """A batch gives the bits of its single images; every segment read as [N, C, h, w] gives the bits of channel-last
    inputs, and `out` as [N, Cout, h, w] those of a channel-last `out`."""
    from eogs2_amd import _abi

    segs, cout, _, _, act, _ = config
    inputs, weight, bias, add = case_on(dev, config, (2, 17, 19), seed=300)
    both = run_rect(inputs, weight, bias, act, add)
    assert bool(torch.isfinite(both).all())
    for n in range(2):
        # (clones: a slice of the batch may start off a 16-byte boundary, which the library refuses)
        one = run_rect([t[n:n + 1].clone() for t in inputs], weight, bias, act, None if add is None else add[n:n + 1].clone())
        assert torch.equal(one[0], both[n]), n
    planar = [t.permute(0, 3, 1, 2).contiguous() for t in inputs]
    mask = (1 << len(segs)) - 1
    assert torch.equal(run_rect(planar, weight, bias, act, add, flags=mask), both)
    got = run_rect(planar, weight, bias, act, add, flags=mask | _abi.FLOWNET_OUT_NCHW)
    assert got.shape == (2, cout, 17, 19) and torch.equal(got.permute(0, 2, 3, 1), both)
    if len(segs) > 1:
        assert torch.equal(run_rect([planar[0]] + inputs[1:], weight, bias, act, add, flags=1), both)


# ---- the gate epilogues at 1 x 5 and 5 x 1 ----

def gate_case_on(dev, config, shape, seed):
    """lc.gate_rect_case on the device; the pairs at the update's sizes without a bias, as the update calls them."""
    inputs, weight, bias, add, aux, hid = lc.gate_rect_case(config, shape, seed)
    return [t.to(dev) for t in inputs], weight.to(dev), None if config[0][0] == lc.HIDDEN else bias.to(dev), add.to(dev), aux.to(dev), hid.to(dev)


@pytest.mark.parametrize("config", [c for c in lc.GATE_CONFIGS if c[4] == "gates"], ids=lc.config_id)
@pytest.mark.parametrize("shape", lc.GENERAL_SHAPES + ("tile",), ids=shape_id)
def test_gates_epilogue_given_its_argument(dev, shape, config):
    """tests/test_gpu_flownet_general.py's test of the gates and its bound, at 1 x 5 and 5 x 1: v from an EOGS_FLOWNET_EPI_BIAS
    run of the same operands (the sum does not depend on the epilogue), then |z - sigmoid(v)| <= 4 u sigmoid(v) and
    |r h - sigmoid(v) aux| <= 5 u |sigmoid(v) aux|, u = 2^-24, times 1 + 2^-20 (derived there)."""
    segs, cout, _, _, _ = config
    shape = resolve(shape)
    N, h, w = shape
    half = cout // 2
    inputs, weight, bias, add, aux, _ = gate_case_on(dev, config, shape, seed=800)
    v = run_rect(inputs, weight, bias, "none", add).double()
    buf, out = guarded(2 * N * h * w * half, lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=dev))
    out = out.view(2, N, h, w, half)
    assert run_rect(inputs, weight, bias, "gates", add, aux=aux, out=out) is out
    assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())
    assert bool(torch.isfinite(out).all())
    z, r = torch.sigmoid(v[..., :half]), torch.sigmoid(v[..., half:])
    want = torch.stack([z, r * aux.double()])
    bound = torch.stack([4 * U * z, 5 * U * (r * aux.double()).abs()]) * HIGHER
    err = (out.double() - want).abs()
    worst = [float((err[i] / bound[i].clamp_min(1e-300)).max()) for i in range(2)]
    print(f"gates {lc.config_id(config)} {shape}: largest multiple of the bound: z {worst[0]:.4f}, r h {worst[1]:.4f}")
    assert bool((err <= bound).all()), f"{float((err - bound).max()):.3e} over the bound"
    again = torch.full_like(out, float("nan"))
    assert torch.equal(run_rect(inputs, weight, bias, "gates", add, aux=aux, out=again), out)


@pytest.mark.parametrize("config", [c for c in lc.GATE_CONFIGS if c[4] == "gru"], ids=lc.config_id)
@pytest.mark.parametrize("shape", lc.GENERAL_SHAPES + ("tile",), ids=shape_id)
def test_gru_epilogue_given_its_argument(dev, shape, config):
    """tests/test_gpu_flownet_general.py's test of the blend and its bound, at 1 x 5 and 5 x 1: with u = 2^-24,
    3 u |1 - z| |h| + |z| (T ulp(tanh v) + 2 u |tanh v|), times 1 + 2^-20, T four times the largest error in ulps of
    torch.tanh in float32 on the device over the same arguments (derived and measured there; printed at every run)."""
    shape = resolve(shape)
    inputs, weight, bias, add, z, hid = gate_case_on(dev, config, shape, seed=900)
    v32 = run_rect(inputs, weight, bias, "none", add)
    v = v32.double()
    tanh = torch.tanh(v)
    measured = float(((torch.tanh(v32).double() - tanh).abs() / ulp_of(tanh)).max())
    assert 0 < measured < 16
    T = 4 * measured
    g = torch.Generator().manual_seed(901)
    buf, out = guarded(hid.numel(), lambda n: torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64)
                       .to(torch.int32).view(torch.float32).to(dev))
    out = out.view(hid.shape)
    out.copy_(hid)
    before = buf.view(torch.int32).clone()
    assert run_rect(inputs, weight, bias, "gru", add, aux=z, out=out) is out
    after = buf.view(torch.int32)
    assert torch.equal(after[:64], before[:64]) and torch.equal(after[-64:], before[-64:])
    assert bool(torch.isfinite(out).all())
    z64, h64 = z.double(), hid.double()
    want = (1 - z64) * h64 + z64 * tanh
    bound = (3 * U * (1 - z64) * h64.abs() + z64 * (T * ulp_of(tanh) + 2 * U * tanh.abs())) * HIGHER
    err = (out.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"gru {lc.config_id(config)} {shape}: torch.tanh float32 is within {measured:.3f} ulp, tanhf allowed {T:.3f} ulp; "
          f"largest multiple of the bound {worst:.4f}")
    assert bool((err <= bound).all()), f"{float((err - bound).max()):.3e} over the bound"
    again = hid.clone()
    assert torch.equal(run_rect(inputs, weight, bias, "gru", add, aux=z, out=again), out)
    assert not torch.equal(out, hid)


# ---- the update ----

@pytest.fixture(scope="module")
def large(dev):
    """RAFT-large with seeded default weights in float32 and its float64 copy, shared and left unchanged."""
    from eogs2_amd import raft

    torch.manual_seed(40)
    model = raft.raft_large(corr="volume", update="torch").eval().to(dev)
    return model, copy.deepcopy(model).double()


def test_step_before_begin_raises(dev, large):
    from eogs2_amd import raft

    f = raft.FusedUpdateLarge(large[0].update_block, large[0].mask_predictor)
    with pytest.raises(RuntimeError, match="begin"):
        f.step(torch.zeros(1, lc.CORR, 16, 16, device=dev), torch.zeros(1, 2, 16, 16, device=dev))
    with pytest.raises(RuntimeError, match="begin"):
        f.mask()
    with pytest.raises(RuntimeError, match="begin"):
        f.hidden()


@pytest.mark.parametrize("shape", lc.STEP_SHAPES, ids=ids)
def test_updates_against_their_float64_run(dev, large, shape):
    """FusedUpdateLarge (begin, then three chained steps, the mask after each) against raft.UpdateBlock and raft.MaskPredictor
    run by torch in float32 and in float64 on the same device, seeded default weights. For the hidden state, delta and the
    mask after each step (one update, and three chained: the hidden state advances in place) the largest deviation from
    float64 may be at most 16 x the torch float32 modules' own: the factor tests/test_gpu_flownet.py uses for RAFT-small's
    update. hidden() right after begin gives the hidden state back bit for bit, mask() leaves it as it is, a second run gives
    the same bits, the workspace is prefilled with 0xFF, and the header's statement in float64 (update_large_oracle) agrees
    with the modules on the device too."""
    from eogs2_amd import raft

    model, model64 = large
    block, predictor, block64, predictor64 = model.update_block, model.mask_predictor, model64.update_block, model64.mask_predictor
    hidden, context, corr, flow = (t.to(dev) for t in lc.update_large_inputs(*shape, seed=41))
    steps = [(corr, flow)] + [tuple(t.to(dev) for t in lc.update_large_inputs(*shape, seed=s)[2:]) for s in (42, 43)]
    N, h, w = shape
    with torch.inference_mode():
        def fused_run():
            f = raft.FusedUpdateLarge(block, predictor)
            f.begin(hidden, context)
            f._state[3].fill_(0xFF)  # the workspace as NaNs: begin, step and mask rely on nothing they did not write
            f.begin(hidden, context)
            assert torch.equal(f.hidden(), hidden)  # the round trip
            out = []
            for c, fl in steps:
                d = f.step(c, fl)
                hd = f.hidden()
                m = f.mask()
                assert torch.equal(f.hidden(), hd)
                out.append((hd, d, m))
            return out

        got = fused_run()
        h32, h64, want = hidden, hidden.double(), []
        for c, fl in steps:
            h32, d32 = block(h32, context, c, fl)
            m32 = predictor(h32)
            prev64 = h64
            h64, d64 = block64(h64, context.double(), c.double(), fl.double())
            m64 = predictor64(h64)
            want.append(((h32, h64), (d32, d64), (m32, m64)))
            oh, od, om = lc.update_large_oracle(block64, predictor64, prev64, context.double(), c.double(), fl.double())
            for a, b in ((oh, h64), (od, d64), (om, m64)):
                assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
        again = fused_run()
    for i, (g3, w3) in enumerate(zip(got, want)):
        assert g3[0].shape == (N, lc.HIDDEN, h, w) and g3[1].shape == (N, 2, h, w) and g3[2].shape == (N, lc.MASK, h, w)
        assert g3[1].is_contiguous() and g3[2].is_contiguous()
        for name, g, (t32, t64) in zip(("hidden", "delta", "mask"), g3, w3):
            assert g.dtype == torch.float32 and bool(torch.isfinite(g).all())
            mine, theirs = float((g.double() - t64).abs().max()), float((t32.double() - t64).abs().max())
            print(f"update large {shape} {name} {i + 1}: |fused - f64| {mine:.3e}, |torch32 - f64| {theirs:.3e}, "
                  f"factor {mine / max(theirs, 1e-300):.3f} of 16, largest |value| {float(t64.abs().max()):.3f}")
            assert mine <= 16 * theirs, (name, i + 1)
    assert all(torch.equal(a, b) for x, y in zip(got, again) for a, b in zip(x, y))
    assert not torch.equal(got[0][0], got[2][0])


@pytest.mark.parametrize("shape", lc.STEP_SHAPES, ids=ids)
def test_update_is_the_chain_of_its_convolutions(dev, large, shape):
    """begin, two steps and the masks of FusedUpdateLarge against the same work done by hand through
    eogs_flowrect_pack and eogs_flowrect_conv, as include/eogs_resample.h states it: the GRUs' weights split by
    channel offsets into the context's share and the rest with convz | convr sharing one packing by column ranges, the
    four hoisted planes, per step the eleven convolutions and per mask the two, with their flags and epilogues. Bit for bit."""
    from eogs2_amd import _abi, raft

    block, predictor = large[0].update_block, large[0].mask_predictor
    hidden, context, corr, flow = (t.to(dev) for t in lc.update_large_inputs(*shape, seed=44))
    _, _, corr2, flow2 = (t.to(dev) for t in lc.update_large_inputs(*shape, seed=45))
    H, C, M = lc.HIDDEN, lc.CONTEXT, lc.MOTION
    with torch.inference_mode():
        fused = raft.FusedUpdateLarge(block, predictor)
        fused.begin(hidden, context)
        got = []
        for c, f in ((corr, flow), (corr2, flow2)):
            delta = fused.step(c, f)
            got.append((fused.hidden(), delta, fused.mask()))

        def packing(segs, cout, parts, offsets=None):
            kh, kw = parts[0][1].shape[2:]
            buf = new_rect_packing(dev, segs, cout, kh, kw)
            for off, wt in parts:
                rect_pack_into(buf, segs, cout, wt.detach(), cout_off=off, offsets=offsets)
            assert not bool((buf.view(torch.int32) == -1).any())
            return buf, cout, (kh, kw)

        def plain(m, segs):
            return packing(segs, m.weight.shape[0], [(0, m.weight)]), m.bias.detach()

        me, rb, fh = block.motion_encoder, block.recurrent_block, block.flow_head
        cc1, cc2, cf1, cf2 = plain(me.convcorr1[0], (lc.CORR,)), plain(me.convcorr2[0], (256,)), plain(me.convflow1[0], (2,)), plain(me.convflow2[0], (128,))
        menc, fh1, fh2 = plain(me.conv[0], (192, 64)), plain(fh.conv1, (H,)), plain(fh.conv2, (256,))
        mk1, mk2 = plain(predictor.convrelu[0], (H,)), plain(predictor.conv, (256,))
        ctx, rest, segs = (H,), (0, H + C, H + C + M), (H, M, 2)
        grus = []
        for gru in (rb.convgru1, rb.convgru2):
            wz, wr, wq = (m.weight.detach() for m in (gru.convz, gru.convr, gru.convq))
            bz, br, bq = (m.bias.detach() for m in (gru.convz, gru.convr, gru.convq))
            assert wz.shape[1] == H + C + M + 2
            plane_zr = run_rect([context], None, torch.cat([bz, br]), "none", flags=1, packed=packing((C,), 2 * H, [(0, wz), (H, wr)], ctx))
            plane_q = run_rect([context], None, bq, "none", flags=1, packed=packing((C,), H, [(0, wq)], ctx))
            grus.append((plane_zr, plane_q, packing(segs, 2 * H, [(0, wz), (H, wr)], rest), packing(segs, H, [(0, wq)], rest)))
        hid = hidden.permute(0, 2, 3, 1).contiguous()
        for i, (c, f) in enumerate(((corr, flow), (corr2, flow2))):
            c1 = run_rect([c], None, cc1[1], "relu", flags=1, packed=cc1[0])
            c2 = run_rect([c1], None, cc2[1], "relu", packed=cc2[0])
            f1 = run_rect([f], None, cf1[1], "relu", flags=1, packed=cf1[0])
            f2 = run_rect([f1], None, cf2[1], "relu", packed=cf2[0])
            m = run_rect([c2, f2], None, menc[1], "relu", packed=menc[0])
            for plane_zr, plane_q, gates_p, q_p in grus:
                zr = run_rect([hid, m, f], None, None, "gates", add=plane_zr, aux=hid, flags=4, packed=gates_p)
                run_rect([zr[1], m, f], None, None, "gru", add=plane_q, aux=zr[0], out=hid, flags=4, packed=q_p)
            d = run_rect([hid], None, fh1[1], "relu", packed=fh1[0])
            delta = run_rect([d], None, fh2[1], "none", flags=_abi.FLOWNET_OUT_NCHW, packed=fh2[0])
            mh = run_rect([hid], None, mk1[1], "relu", packed=mk1[0])
            mask = run_rect([mh], None, mk2[1], "quarter", flags=_abi.FLOWNET_OUT_NCHW, packed=mk2[0])
            assert bool(torch.isfinite(delta).all()) and bool(torch.isfinite(hid).all()) and bool(torch.isfinite(mask).all())
            assert torch.equal(got[i][0], hid.permute(0, 3, 1, 2)), f"hidden state after step {i + 1}"
            assert torch.equal(got[i][1], delta), f"delta after step {i + 1}"
            assert torch.equal(got[i][2], mask), f"mask after step {i + 1}"
    assert not torch.equal(got[0][0], got[1][0])


# ---- the network and the example ----

@pytest.fixture(scope="module")
def network_runs(dev, large):
    """The shared reference of the whole network at 128 x 136, 3 updates, every flow: the float32 and the float64 run of the
    plain-torch volume path, the second arbitrating."""
    model, model64 = large
    g = torch.Generator().manual_seed(21)
    H, W = 128, 136
    base = torch.rand(1, 3, H + 8, W + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev)
    with torch.inference_mode():
        v32 = model(a, b, num_flow_updates=3, return_all=True)
        v64 = model64(a.double(), b.double(), num_flow_updates=3, return_all=True)
    return a, b, v32, v64


@pytest.mark.parametrize("return_all", [False, True], ids=["last", "all"])
def test_network_against_its_float64_run(dev, large, network_runs, return_all):
    """RAFT("large", corr="ondemand", update="fused_large") at 128 x 136 with 3 updates, seeded random weights, eval mode: the
    fused update and mask over the on-demand correlation against the plain-torch volume path in float64, at most 16 x the
    float32 volume path's own deviation, for every flow returned."""
    from eogs2_amd import raft

    a, b, v32, v64 = network_runs
    model = raft.RAFT("large", corr="ondemand", update="fused_large").eval().to(dev)
    model.load_state_dict(large[0].state_dict())
    assert model._fused is None and model._fused_large is not None
    with torch.inference_mode():
        fu = model(a, b, num_flow_updates=3, return_all=return_all)
    assert len(fu) == (3 if return_all else 1)
    for f, t32, t64 in zip(fu, v32[-len(fu):], v64[-len(fu):]):
        assert f.shape == (1, 2, 128, 136) and f.dtype == torch.float32 and bool(torch.isfinite(f).all())
        mine, theirs = float((f.double() - t64).abs().max()), float((t32.double() - t64).abs().max())
        print(f"network large return_all={return_all}: |fused - f64| {mine:.3e}, |volume32 - f64| {theirs:.3e}, "
              f"factor {mine / max(theirs, 1e-300):.3f} of 16, largest |flow| {float(t64.abs().max()):.3f}")
        assert mine <= 16 * theirs
    if return_all:
        assert not torch.equal(fu[0], fu[-1])


def test_example_with_the_fused_large_update():
    """examples/train_synthetic.py --flow-matching --flow-network large --flow-update fused_large runs to the end at the size
    tests/test_gpu_flownet_example.py uses, with finite losses."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    first, last = train_synthetic.main(["--gaussians", "5000", "--size", "128", "--iters", "6", "--quiet", "--flow-matching",
                                        "--flow-network", "large", "--flow-update", "fused_large"])[:2]
    assert math.isfinite(first) and math.isfinite(last)
