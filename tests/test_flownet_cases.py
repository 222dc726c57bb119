"""CPU: the float64 oracle of the fused update (tests/flownet_cases.py) against raft.UpdateBlock.forward in float64. Float64
rounding is the only difference, so this proves the hoisting identity (the context's share of the GRU convolutions as a plane)
and the channel slices of convz / convr / convq before any kernel is involved. And the general cases of the convolution
(flownet_cases.GENERAL) reach the parts of the kernel their comments name, by the library's own packing sizes."""
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


@pytest.fixture(scope="module")
def lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def pack_floats(lib, segs, cout, k):
    import ctypes

    n = ctypes.c_size_t()
    lib.check(lib.flownet_conv_pack_bytes(k, len(segs), (ctypes.c_int * len(segs))(*segs), cout, ctypes.byref(n)))
    assert n.value % 4 == 0
    return n.value // 4


def pack_plan(lib, segs, cout, k):
    """(NB, workgroups along Cout, chunks) of a convolution from eogs_flownet_conv_pack_bytes alone, which answers without a
    device. The packing is [chunk of 8 channels per segment][workgroup along Cout][tap][8][row] floats (flownet_pack_kernel
    in csrc/flownet.hip), a row being 16 floats under one block per workgroup and 48 under two or three. One block per
    workgroup is the plan of a single block (Cout <= 16); test_the_one_block_row_belongs_to_a_single_block holds that by
    sizes. So the size gives the number of workgroups, and that number gives NB: where two and three blocks per workgroup
    need equally many workgroups the smaller has fewer padded blocks, which is what the plan minimises; equal padding with
    different workgroup counts the size itself tells apart."""
    chunks = sum(-(-c // fc.CHUNK) for c in segs)
    blocks = -(-cout // fc.BLOCK)
    floats = pack_floats(lib, segs, cout, k)
    per_workgroup = lambda row: chunks * k * k * fc.CHUNK * row  # noqa: E731
    if blocks == 1:
        assert floats == per_workgroup(16)
        return 1, 1, chunks
    assert floats % per_workgroup(48) == 0
    workgroups = floats // per_workgroup(48)
    fits = [nb for nb in (2, 3) if -(-blocks // nb) == workgroups]
    assert fits, (segs, cout, k, floats)
    return fits[0], workgroups, chunks


def test_the_one_block_row_belongs_to_a_single_block(lib):
    for blocks in range(2, 25):
        for cout in (blocks * 16 - 15, blocks * 16):
            floats = pack_floats(lib, (8,), cout, 3)
            assert floats % (9 * 8 * 48) == 0 and floats // (9 * 8 * 48) in (-(-blocks // 2), -(-blocks // 3)), cout
            if blocks % 3:  # (a multiple of three blocks has one size under either row)
                assert floats != blocks * 9 * 8 * 16, cout


def test_general_cases_reach_what_they_claim(lib):
    """The comments of flownet_cases.GENERAL as assertions, and the coverage the two tables owe together: every kernel size,
    a k >= 5 over more than one chunk for each of 5 and 7 (the hand-over from a chunk's last tap row to the next chunk), a
    ragged Cout under each of NB = 2 and 3, and the channel-lane boundaries 1, 4 and 5."""
    plans = {c: pack_plan(lib, c[0], c[1], c[2]) for c in fc.CONFIGS + fc.GENERAL}
    g = fc.GENERAL
    real_in_last = lambda c: c[1] - (-(-c[1] // 16) - 1) * 16  # noqa: E731
    padded_blocks = lambda c: plans[c][0] * plans[c][1] - -(-c[1] // 16)  # noqa: E731
    assert g[0][2] == 5 and plans[g[0]] == (2, 1, 1) and real_in_last(g[0]) == 1 and padded_blocks(g[0]) == 0
    assert g[1][2] == 7 and plans[g[1]] == (2, 2, 2) and len(g[1][0]) == 2 and real_in_last(g[1]) == 2 and padded_blocks(g[1]) == 0
    assert g[2][2] == 5 and plans[g[2]] == (2, 4, 2) and len(g[2][0]) == 1 and padded_blocks(g[2]) == 1 and g[2][1] % 16 == 0
    assert g[3][2] == 3 and plans[g[3]] == (3, 1, 4) and g[3][0] == (5, 9, 1) and 3 * 16 - g[3][1] == 15
    assert g[4][:3] == ((4,), 1, 1) and plans[g[4]] == (1, 1, 1)
    assert {c[2] for c in plans} == {1, 3, 5, 7}
    for k in (5, 7):
        assert any(c[2] == k and plans[c][2] > 1 for c in plans), k
    for nb in (2, 3):
        assert any(plans[c][0] == nb and c[1] % 16 for c in plans), nb
    assert all(c[4] in ("none", "relu") for c in g)
    lanes = {s % fc.CHUNK for c in g for s in c[0]}
    assert {1, 4, 5} <= lanes  # one real lane, the skipped instruction's boundary, one real lane in the second instruction
    assert any(len(c[0]) == 3 and all(s % fc.CHUNK for s in c[0]) for c in g)  # three segments, each ragged
    assert any(c[3] for c in g) and any(not c[3] for c in g)
    # the update's own plans, for the record of what the first table already reaches: ragged Cout under NB = 1 only
    assert [plans[c][0] for c in fc.CONFIGS if c[1] % 16] == [1]
    for c in fc.GATE_CONFIGS:
        assert c[4] in ("gates", "gru") and (c[1] % 2 == 0 or c[4] == "gru")


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
