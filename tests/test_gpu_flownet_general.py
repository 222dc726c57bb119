"""GPU (MI355X): the convolution of eogs2_amd/csrc/flownet.hip across its public surface (eogs_flownet_conv and
eogs_flownet_conv_pack of include/eogs_resample.h), beyond the eight convolutions that RAFT-small's update runs through it
(tests/test_gpu_flownet.py): k = 5, k > 3 over several channel chunks, ragged segments and ragged Cout under every block
count per workgroup, the layout flags and a missing bias bit for bit, the packing by column ranges and channel offsets
byte for byte, the two gate epilogues per element given their float32 argument, and FusedUpdate's two steps as the chain of
these links bit for bit."""
import itertools

import pytest
import torch

import flownet_cases as fc
from test_gpu_flownet import (U, case_on, check_against_float64, check_batch_is_its_images, check_exact_cases, dev, ids,  # noqa: F401
                              new_packing, pack_into, run_conv, tile_shape)

pytestmark = pytest.mark.gpu

shape_id = lambda s: s if isinstance(s, str) else ids(s)  # noqa: E731
HIGHER = 1 + 2.0 ** -20  # the second-order terms of a product of a few (1 + d), |d| <= 2^-22, and the float64 reference's own error


def resolve(shape):
    return tile_shape() if shape == "tile" else shape


# ---- per element against float64, the exact cases, a batch ----

@pytest.mark.parametrize("config", fc.GENERAL, ids=fc.config_id)
@pytest.mark.parametrize("shape", fc.GENERAL_SHAPES + ("tile",), ids=shape_id)
def test_general_convolution_against_float64(dev, shape, config):
    check_against_float64(dev, shape, config)


@pytest.mark.parametrize("config", fc.GENERAL, ids=fc.config_id)
def test_general_convolution_exact_cases(dev, config):
    check_exact_cases(dev, config, lanes=True)


@pytest.mark.parametrize("config", fc.GENERAL, ids=fc.config_id)
def test_general_convolution_of_a_batch_is_its_images(dev, config):
    check_batch_is_its_images(dev, config, (2, 9, 17))


# ---- layouts ----

@pytest.mark.parametrize("config", fc.CONFIGS + fc.GENERAL, ids=fc.config_id)
@pytest.mark.parametrize("shape", fc.LAYOUT_SHAPES + ("tile",), ids=shape_id)
def test_layout_flags_do_not_change_a_bit(dev, shape, config):
    """Every subset of the segments read as [N, C, h, w], with `out` channel-last and as [N, Cout, h, w]: the order of an
    element's sum does not depend on a layout, so every run equals the all-channel-last one under torch.equal."""
    from eogs2_amd import _abi

    segs, cout, k, with_add, act = config
    inputs, weight, bias, add = case_on(dev, config, resolve(shape), seed=400)
    want = run_conv(inputs, weight, bias, act, add)
    assert bool(torch.isfinite(want).all())
    planar = [t.permute(0, 3, 1, 2).contiguous() for t in inputs]
    for mask, out_nchw in itertools.product(range(1 << len(segs)), (0, _abi.FLOWNET_OUT_NCHW)):
        xs = [planar[s] if mask >> s & 1 else inputs[s] for s in range(len(segs))]
        got = run_conv(xs, weight, bias, act, add, flags=mask | out_nchw)
        assert got.shape == ((want.shape[0], cout) + want.shape[1:3] if out_nchw else want.shape)
        assert torch.equal(got.permute(0, 2, 3, 1) if out_nchw else got, want), (mask, out_nchw)


@pytest.mark.parametrize("config", fc.CONFIGS + fc.GENERAL, ids=fc.config_id)
def test_no_bias_is_a_zero_bias(dev, config):
    inputs, weight, bias, add = case_on(dev, config, (2, 9, 17), seed=500)
    got = run_conv(inputs, weight, None, config[4], add)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, run_conv(inputs, weight, torch.zeros_like(bias), config[4], add))
    assert not torch.equal(got, run_conv(inputs, weight, bias, config[4], add))


# ---- packing ----

def columns_of(dev, segs, cout, k):
    """The packing's shape as the kernel's source states it, [chunk][workgroup along Cout][tap][8][row] with a row of 16
    floats for a single block and of 48 otherwise, and per (workgroup, row slot) the output column it holds or -1 for a
    padded one: read off a packing of a weight whose every element is its column's number + 1."""
    chunks, row = sum(-(-c // fc.CHUNK) for c in segs), 16 if cout <= fc.BLOCK else 48
    marker = (torch.arange(cout, dtype=torch.float32, device=dev) + 1)[:, None, None, None].expand(cout, sum(segs), k, k)
    packed = pack_into(new_packing(dev, segs, cout, k), segs, cout, k, marker).view(torch.float32)
    assert packed.numel() % (chunks * k * k * fc.CHUNK * row) == 0
    shape = (chunks, packed.numel() // (chunks * k * k * fc.CHUNK * row), k * k, fc.CHUNK, row)
    packed = packed.view(shape)
    col = packed.amax(dim=(0, 2, 3)).long() - 1  # (every column has a real channel lane in every chunk's first lane)
    assert sorted(col[col >= 0].tolist()) == list(range(cout))
    assert bool(((packed == 0) | (packed == (col + 1)[None, :, None, None, :])).all())
    return shape, col


@pytest.mark.parametrize("segs, cout, k, a", [((5, 9, 1), 33, 3, 20), ((3,), 17, 5, 7), ((96, 80, 2), 192, 3, 96)],
                         ids=lambda v: "+".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_packing_by_column_ranges(dev, segs, cout, k, a):
    """Columns [0, a) and [a, Cout) packed from two weight tensors, in either order, are the bytes of one call on their
    concatenation (a is no multiple of 16 in the first two; 96 of 192 is how the update shares convz | convr). After either
    call alone the other's real columns are still 0xFF and every padded column is already zero. No 0xFF float is left."""
    g = torch.Generator().manual_seed(600)
    weight = torch.randn(cout, sum(segs), k, k, generator=g).to(dev)
    lo, hi = weight[:a].clone(), weight[a:].clone()
    one = pack_into(new_packing(dev, segs, cout, k), segs, cout, k, weight)
    ones = one.view(torch.int32)
    assert not bool((ones == -1).any())
    shape, col = columns_of(dev, segs, cout, k)
    where = col[None, :, None, None, :].expand(shape)
    for first, second in (((lo, 0), (hi, a)), ((hi, a), (lo, 0))):
        buf = pack_into(new_packing(dev, segs, cout, k), segs, cout, k, first[0], cout_off=first[1])
        part = buf.view(torch.int32).view(shape)
        mine = (where >= first[1]) & (where < first[1] + first[0].shape[0])
        assert bool((part[where < 0] == 0).all())
        assert bool((part[(where >= 0) & ~mine] == -1).all())
        assert torch.equal(part[mine], ones.view(shape)[mine])
        pack_into(buf, segs, cout, k, second[0], cout_off=second[1])
        assert torch.equal(buf, one), first[1]
    # and the packed halves multiply as the whole does
    x = [torch.randn(1, 5, 7, c, generator=g).to(dev) for c in segs]
    assert torch.equal(run_conv(x, None, None, packed=(buf, cout, k)), run_conv(x, weight, None))


@pytest.mark.parametrize("cin, offsets", [(15, (10, 0, 9)), (20, (14, 2, 12))], ids=["15", "20gaps"])
def test_packing_by_channel_offsets(dev, cin, offsets):
    """Segments (5, 9, 1) read at `offsets` of a weight with Cin channels are the bytes of the gathered weight packed in
    order. The channels no segment covers hold NaN: they are never read."""
    segs, cout, k = (5, 9, 1), 33, 3
    g = torch.Generator().manual_seed(700)
    weight = torch.randn(cout, cin, k, k, generator=g)
    covered = torch.zeros(cin, dtype=torch.bool)
    for c, o in zip(segs, offsets):
        assert not bool(covered[o:o + c].any())
        covered[o:o + c] = True
    assert int((~covered).sum()) == cin - sum(segs)
    weight[:, ~covered] = float("nan")
    weight = weight.to(dev)
    gathered = torch.cat([weight[:, o:o + c] for c, o in zip(segs, offsets)], dim=1).contiguous()
    want = pack_into(new_packing(dev, segs, cout, k), segs, cout, k, gathered)
    got = pack_into(new_packing(dev, segs, cout, k), segs, cout, k, weight, offsets=offsets)
    assert torch.equal(got, want)
    assert not bool((got.view(torch.int32) == -1).any()) and bool(torch.isfinite(got.view(torch.float32)).all())
    # offsets and a column range together, as the update's GRU packings are composed
    both = new_packing(dev, segs, cout, k)
    pack_into(both, segs, cout, k, weight[20:].clone(), cout_off=20, offsets=offsets)
    pack_into(both, segs, cout, k, weight[:20].clone(), cout_off=0, offsets=offsets)
    assert torch.equal(both, want)


# ---- the gate epilogues ----

def ulp_of(x):
    """The spacing of float32 at the float64 values `x` (normal range)."""
    return torch.ldexp(torch.ones_like(x), torch.frexp(x.abs())[1] - 24)


def gate_case_on(dev, config, shape, seed):
    """fc.gate_case on the device; the pair at the update's sizes without a bias, as the update calls it."""
    inputs, weight, bias, add, aux, hid = fc.gate_case(config, shape, seed)
    return [t.to(dev) for t in inputs], weight.to(dev), None if config[0][0] == fc.HIDDEN else bias.to(dev), add.to(dev), aux.to(dev), hid.to(dev)


def guarded(numel, fill):
    """A buffer of `numel` floats between two guards of 64, and the view between them."""
    buf = fill(numel + 128)
    return buf, buf[64:64 + numel]


@pytest.mark.parametrize("config", [c for c in fc.GATE_CONFIGS if c[4] == "gates"], ids=fc.config_id)
@pytest.mark.parametrize("shape", fc.GENERAL_SHAPES + ("tile",), ids=shape_id)
def test_gates_epilogue_given_its_argument(dev, shape, config):
    """The sum under an epilogue is the sum under EOGS_FLOWNET_EPI_BIAS bit for bit (its order does not depend on the
    epilogue), so v is taken from such a run and the epilogue is held alone, every element against float64 formed from
    that float32 v: z = 1 / (1 + expf(-v)) in the first map, z * aux in the second at out + P Cout / 2.

    The bound, with u = 2^-24 (a rounding's relative error): expf is documented at 1 ulp, at most 2 u relative; 1 + e
    rounds once (u) and keeps e's error scaled by e / (1 + e) < 1; the division is correctly rounded (u; the library is
    built without fast-math, and HIP's float division is correctly rounded by default). So |z - sigmoid(v)| <= 4 u
    sigmoid(v), and the product with aux rounds once more: 5 u |sigmoid(v) aux|. Both times 1 + 2^-20 for the second-order
    terms. The update's own pair runs without a bias, as the update calls it. The slack around the two maps keeps its NaNs."""
    segs, cout, k, _, _ = config
    shape = resolve(shape)
    N, h, w = shape
    half = cout // 2
    inputs, weight, bias, add, aux, _ = gate_case_on(dev, config, shape, seed=800)
    v = run_conv(inputs, weight, bias, "none", add).double()
    buf, out = guarded(2 * N * h * w * half, lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=dev))
    out = out.view(2, N, h, w, half)
    assert run_conv(inputs, weight, bias, "gates", add, aux=aux, out=out) is out
    assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())
    assert bool(torch.isfinite(out).all())
    z, r = torch.sigmoid(v[..., :half]), torch.sigmoid(v[..., half:])
    want = torch.stack([z, r * aux.double()])
    bound = torch.stack([4 * U * z, 5 * U * (r * aux.double()).abs()]) * HIGHER
    err = (out.double() - want).abs()
    worst = [float((err[i] / bound[i].clamp_min(1e-300)).max()) for i in range(2)]
    print(f"gates {fc.config_id(config)} {shape}: largest multiple of the bound: z {worst[0]:.4f}, r h {worst[1]:.4f}")
    assert bool((err <= bound).all()), f"{float((err - bound).max()):.3e} over the bound"
    again = torch.full_like(out, float("nan"))
    assert torch.equal(run_conv(inputs, weight, bias, "gates", add, aux=aux, out=again), out)


@pytest.mark.parametrize("config", [c for c in fc.GATE_CONFIGS if c[4] == "gru"], ids=fc.config_id)
@pytest.mark.parametrize("shape", fc.GENERAL_SHAPES + ("tile",), ids=shape_id)
def test_gru_epilogue_given_its_argument(dev, shape, config):
    """As the gates: v from an EOGS_FLOWNET_EPI_BIAS run of the same operands, then every element of the blend
    h' = (1 - z) h + z tanhf(v), in place in `out`, against float64 formed from the float32 v, z = aux and h.

    The bound, with u = 2^-24: 1 - z, its product with h and the final sum round once each, 3 u |1 - z| |h| in all; z tanhf(v)
    carries tanhf's error T ulp(tanh v), the product's rounding and the sum's: |z| (T ulp(tanh v) + 2 u |tanh v|); times
    1 + 2^-20 for the second-order terms. (The library is built with -ffp-contract=off; a fused multiply-add would round
    less often, not more.) No accuracy table for tanhf ships with the ROCm installation, so T comes from MEASUREMENT:
    torch.tanh in float32 on the device against float64 over the same arguments v, and four times its largest error in
    ulps is allowed: another correct float32 tanh may differ by a small factor, not by an order of magnitude. Measured on
    an MI355X: torch.tanh within 0.648 to 1.312 ulp over the six cases' arguments (0.648 and 0.961 at the two single
    positions), so T is 2.6 to 5.2 ulp; the blend came to at most 0.72 of its bound. Both are printed at every run.
    Outside the map, `out`'s buffer keeps its bits."""
    segs, cout, k, _, _ = config
    shape = resolve(shape)
    N, h, w = shape
    inputs, weight, bias, add, z, hid = gate_case_on(dev, config, shape, seed=900)
    v32 = run_conv(inputs, weight, bias, "none", add)
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
    assert run_conv(inputs, weight, bias, "gru", add, aux=z, out=out) is out
    after = buf.view(torch.int32)
    assert torch.equal(after[:64], before[:64]) and torch.equal(after[-64:], before[-64:])
    assert bool(torch.isfinite(out).all())
    z64, h64 = z.double(), hid.double()
    want = (1 - z64) * h64 + z64 * tanh
    bound = (3 * U * (1 - z64) * h64.abs() + z64 * (T * ulp_of(tanh) + 2 * U * tanh.abs())) * HIGHER
    err = (out.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"gru {fc.config_id(config)} {shape}: torch.tanh float32 is within {measured:.3f} ulp, tanhf allowed {T:.3f} ulp; "
          f"largest multiple of the bound {worst:.4f}")
    assert bool((err <= bound).all()), f"{float((err - bound).max()):.3e} over the bound"
    again = hid.clone()
    assert torch.equal(run_conv(inputs, weight, bias, "gru", add, aux=z, out=again), out)
    assert not torch.equal(out, hid)


# ---- the update step as the chain of its convolutions ----

@pytest.mark.parametrize("shape", fc.STEP_SHAPES, ids=ids)
def test_update_is_the_chain_of_its_convolutions(dev, shape):
    """begin + two steps of FusedUpdate against the same work done by hand through eogs_flownet_conv_pack and
    eogs_flownet_conv, as include/eogs_resample.h states it: the six plain packings, the GRU's weights split by channel
    offsets into the context's share and the rest with convz | convr sharing one packing by column ranges, the two hoisted
    planes, and per step the eight convolutions with their flags and epilogues. The hidden state (read at
    eogs_flownet_update_hidden_offset) and delta after each step are the chain's bits."""
    from eogs2_amd import _abi, raft

    torch.manual_seed(40)
    block = raft.raft_small(update="torch").eval().to(dev).update_block
    hidden, context, corr, flow = (t.to(dev) for t in fc.update_inputs(*shape, seed=41))
    _, _, corr2, flow2 = (t.to(dev) for t in fc.update_inputs(*shape, seed=42))
    H, C = fc.HIDDEN, fc.CONTEXT
    with torch.inference_mode():
        fused = raft.FusedUpdate(block)
        fused.begin(hidden, context)
        got = []
        for c, f in ((corr, flow), (corr2, flow2)):
            delta = fused.step(c, f)
            got.append((fused.hidden(), delta))

        me, gru, fh = block.motion_encoder, block.recurrent_block.convgru1, block.flow_head
        conv = {"convcorr1": me.convcorr1[0], "convflow1": me.convflow1[0], "convflow2": me.convflow2[0], "conv": me.conv[0],
                "fh1": fh.conv1, "fh2": fh.conv2}
        wz, wr, wq = (m.weight.detach() for m in (gru.convz, gru.convr, gru.convq))
        bz, br, bq = (m.bias.detach() for m in (gru.convz, gru.convr, gru.convq))

        def packing(segs, cout, k, parts, offsets=None):
            buf = new_packing(dev, segs, cout, k)
            for off, wt in parts:
                pack_into(buf, segs, cout, k, wt.detach(), cout_off=off, offsets=offsets)
            assert not bool((buf.view(torch.int32) == -1).any())
            return buf, cout, k

        def plain(name, segs):
            m = conv[name]
            return packing(segs, m.weight.shape[0], m.weight.shape[2], [(0, m.weight)]), m.bias.detach()

        corr1, flow1, flow2_, menc = plain("convcorr1", (fc.CORR,)), plain("convflow1", (2,)), plain("convflow2", (64,)), plain("conv", (H, 32))
        fh1, fh2 = plain("fh1", (H,)), plain("fh2", (128,))
        motion = menc[0][1]
        assert motion == 80 and wz.shape[1] == H + C + motion + 2
        ctx, rest, segs = (H,), (0, H + C, H + C + motion), (H, motion, 2)
        hoist_zr = packing((C,), 2 * H, 3, [(0, wz), (H, wr)], ctx)
        hoist_q = packing((C,), H, 3, [(0, wq)], ctx)
        gates_p = packing(segs, 2 * H, 3, [(0, wz), (H, wr)], rest)
        q_p = packing(segs, H, 3, [(0, wq)], rest)
        hid = hidden.permute(0, 2, 3, 1).contiguous()
        plane_zr = run_conv([context], None, torch.cat([bz, br]), "none", flags=1, packed=hoist_zr)
        plane_q = run_conv([context], None, bq, "none", flags=1, packed=hoist_q)
        for i, (c, f) in enumerate(((corr, flow), (corr2, flow2))):
            c1 = run_conv([c], None, corr1[1], "relu", flags=1, packed=corr1[0])
            f1 = run_conv([f], None, flow1[1], "relu", flags=1, packed=flow1[0])
            f2 = run_conv([f1], None, flow2_[1], "relu", packed=flow2_[0])
            m = run_conv([c1, f2], None, menc[1], "relu", packed=menc[0])
            zr = run_conv([hid, m, f], None, None, "gates", add=plane_zr, aux=hid, flags=4, packed=gates_p)
            run_conv([zr[1], m, f], None, None, "gru", add=plane_q, aux=zr[0], out=hid, flags=4, packed=q_p)
            d = run_conv([hid], None, fh1[1], "relu", packed=fh1[0])
            delta = run_conv([d], None, fh2[1], "none", flags=_abi.FLOWNET_OUT_NCHW, packed=fh2[0])
            assert delta.shape == got[i][1].shape and bool(torch.isfinite(delta).all()) and bool(torch.isfinite(hid).all())
            assert torch.equal(got[i][0], hid.permute(0, 3, 1, 2)), f"hidden state after step {i + 1}"
            assert torch.equal(got[i][1], delta), f"delta after step {i + 1}"
    assert not torch.equal(got[0][0], got[1][0])
