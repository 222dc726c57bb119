"""Cases and the float64 oracle of RAFT-large's fused update block and of the convolution over rectangular taps
(eogs2_amd.raft.conv2d_rect_cl / FusedUpdateLarge, the entries of include/eogs_resample.h), shared by the CPU test of the oracle
itself (tests/test_flownet_large_cases.py) and the GPU tests (tests/test_gpu_flownet_large.py). Everything is computed from
seeds: no fixture, nothing outside the repository.

  conv_rect_oracle      F.conv2d(torch.cat(inputs)) with padding ((kh - 1) // 2, (kw - 1) // 2) on NCHW views, in the dtype of its
                        inputs (the tests pass float64); act "quarter" is the mask head's 0.25 v; with `magnitude=True`
                        |add| + |bias| + conv(|x|, |W|): the M of the error bound (before the 0.25, which scales both sides)
  update_large_oracle   one update and the mask as the header states them: per GRU the context's share of its three
                        convolutions as two planes formed from the context alone, z and r from ONE 256-wide convolution, the
                        blend; the mask head with its 0.25. tests/test_flownet_large_cases.py holds it against
                        raft.UpdateBlock.forward and raft.MaskPredictor.forward in float64, which proves the hoisting identity
                        for both GRUs and the channel slices.
"""
import math

import torch
import torch.nn.functional as F

# (input channel segments, Cout, (kh, kw), with add, activation, out as [N, Cout, h, w]): every distinct convolution of
# RAFT-large's update and mask head, and the hoisted planes' (z | r | q of one GRU as one 384-wide convolution)
CONFIGS = (
    ((324,), 256, (1, 1), False, "relu", False),          # convcorr1
    ((256,), 192, (3, 3), False, "relu", False),          # convcorr2
    ((2,), 128, (7, 7), False, "relu", False),            # convflow1
    ((128,), 64, (3, 3), False, "relu", False),           # convflow2
    ((192, 64), 126, (3, 3), False, "relu", False),       # conv of the motion encoder
    ((128,), 384, (1, 5), False, "none", False),          # the hoisted context planes of convgru1
    ((128,), 384, (5, 1), False, "none", False),          # and of convgru2
    ((128, 126, 2), 256, (1, 5), True, "none", False),    # convz | convr of convgru1 without the context's channels, the plane added
    ((128, 126, 2), 128, (1, 5), True, "none", False),    # convq of convgru1
    ((128, 126, 2), 256, (5, 1), True, "none", False),    # convgru2
    ((128, 126, 2), 128, (5, 1), True, "none", False),
    ((128,), 256, (3, 3), False, "relu", False),          # flow head conv1 (and the mask head's convrelu: the same shape)
    ((256,), 2, (3, 3), False, "none", True),             # flow head conv2, NCHW
    ((256,), 576, (1, 1), False, "quarter", True),        # the mask head's conv with the 0.25 epilogue, NCHW
)
# (N, h, w): a single position; odd sizes; narrower than a 1 x 5 kernel; shorter than a 5 x 1 kernel; a batch over several
# tiles. The tests add one column and one row beyond whole position tiles.
SHAPES = ((1, 1, 1), (1, 5, 7), (1, 7, 3), (1, 3, 9), (2, 17, 19))
STEP_SHAPES = ((1, 16, 16), (2, 17, 19))
# The rectangular kernel beyond the update's own, in the style of flownet_cases.GENERAL
GENERAL = (
    # three ragged segments (5: one real lane in the chunk's second instruction; 9: a second chunk of one channel; 1); NB = 3
    # with 15 padded columns
    ((5, 9, 1), 33, (1, 5), True, "relu", False),
    ((5, 9, 1), 33, (5, 1), True, "relu", False),
    # exactly four channels (a chunk's second instruction is skipped), Cout = 1, five taps in a column
    ((4,), 1, (5, 1), False, "none", False),
    # 1 x 5 over two chunks; seven blocks under NB = 2: the last workgroup's second block is padding throughout
    ((12,), 112, (1, 5), True, "none", False),
)
GENERAL_SHAPES = ((1, 1, 1), (2, 9, 17))
# (segments, Cout, (kh, kw), with add, epilogue): the gate epilogues at the update's sizes and at one ragged pair
GATE_CONFIGS = (
    ((128, 126, 2), 256, (1, 5), True, "gates"),
    ((128, 126, 2), 128, (1, 5), True, "gru"),
    ((128, 126, 2), 256, (5, 1), True, "gates"),
    ((128, 126, 2), 128, (5, 1), True, "gru"),
    ((5, 9, 1), 34, (1, 5), True, "gates"),
    ((5, 9, 1), 33, (5, 1), True, "gru"),
)
TAP_SHAPES = ((1, 1), (3, 3), (5, 5), (7, 7), (1, 5), (5, 1))
HIDDEN, CONTEXT, CORR, MOTION, MASK = 128, 128, 324, 126, 576


def config_id(c):
    return "+".join(map(str, c[0])) + f"to{c[1]}k{c[2][0]}x{c[2][1]}"


def conv_rect_case(config, shape, seed):
    """(inputs [N, h, w, C_i] float32, weight [Cout, sum C_i, kh, kw], bias, add or None): the weight scaled so that outputs are O(1)."""
    segs, cout, (kh, kw), with_add = config[:4]
    N, h, w = shape
    g = torch.Generator().manual_seed(seed)
    inputs = [torch.randn(N, h, w, c, generator=g) for c in segs]
    weight = torch.randn(cout, sum(segs), kh, kw, generator=g) / math.sqrt(sum(segs) * kh * kw)
    bias = torch.randn(cout, generator=g)
    add = torch.randn(N, h, w, cout, generator=g) if with_add else None
    return inputs, weight, bias, add


def gate_rect_case(config, shape, seed):
    """conv_rect_case and the operands of a gate epilogue, as flownet_cases.gate_case: (inputs, weight, bias, add, aux, h)."""
    segs, cout, _, _, epi = config
    inputs, weight, bias, add = conv_rect_case(config, shape, seed)
    g = torch.Generator().manual_seed(seed + 1)
    N, h, w = shape
    if epi == "gates":
        hid = torch.tanh(torch.randn(N, h, w, cout // 2, generator=g))
        return inputs, weight, bias, add, hid, hid
    return inputs, weight, bias, add, torch.sigmoid(torch.randn(N, h, w, cout, generator=g)), torch.tanh(torch.randn(N, h, w, cout, generator=g))


def conv_rect_oracle(inputs, weight, bias, act="none", add=None, magnitude=False):
    """[N, h, w, Cout] from channel-last inputs, in their dtype."""
    x = torch.cat([t.permute(0, 3, 1, 2) for t in inputs], dim=1)
    pad = ((weight.shape[2] - 1) // 2, (weight.shape[3] - 1) // 2)
    if magnitude:
        out = F.conv2d(x.abs(), weight.abs(), None, padding=pad).permute(0, 2, 3, 1)
        if bias is not None:
            out = out + bias.abs()
        return out if add is None else out + add.abs()
    out = F.conv2d(x, weight, bias, padding=pad).permute(0, 2, 3, 1)
    if add is not None:
        out = out + add
    return torch.relu(out) if act == "relu" else 0.25 * out if act == "quarter" else out


def update_large_inputs(N, h, w, seed):
    """(hidden, context, corr, flow) float32 NCHW: tanh(randn), relu(randn), randn, a flow within +-3 px."""
    g = torch.Generator().manual_seed(seed)
    return (torch.tanh(torch.randn(N, HIDDEN, h, w, generator=g)), torch.relu(torch.randn(N, CONTEXT, h, w, generator=g)),
            torch.randn(N, CORR, h, w, generator=g), (torch.rand(N, 2, h, w, generator=g) * 2 - 1) * 3)


def update_large_oracle(block, mask_predictor, hidden, context, corr, flow):
    """(new hidden, delta, mask of the new hidden) of one update of RAFT-large's `block` (a raft.UpdateBlock) and
    `mask_predictor` (a raft.MaskPredictor) as include/eogs_resample.h states them, in the dtype of the modules and the inputs."""
    me, rb, fh = block.motion_encoder, block.recurrent_block, block.flow_head
    c1 = torch.relu(F.conv2d(corr, me.convcorr1[0].weight, me.convcorr1[0].bias))
    c2 = torch.relu(F.conv2d(c1, me.convcorr2[0].weight, me.convcorr2[0].bias, padding=1))
    f1 = torch.relu(F.conv2d(flow, me.convflow1[0].weight, me.convflow1[0].bias, padding=3))
    f2 = torch.relu(F.conv2d(f1, me.convflow2[0].weight, me.convflow2[0].bias, padding=1))
    m = torch.relu(F.conv2d(torch.cat([c2, f2], dim=1), me.conv[0].weight, me.conv[0].bias, padding=1))
    assert m.shape[1] == MOTION
    # convz / convr / convq read [h | context | motion | flow]
    ctx = list(range(HIDDEN, HIDDEN + CONTEXT))
    rest = list(range(HIDDEN)) + list(range(HIDDEN + CONTEXT, HIDDEN + CONTEXT + MOTION + 2))
    h = hidden
    for gru, pad in ((rb.convgru1, (0, 2)), (rb.convgru2, (2, 0))):
        wzr, bzr = torch.cat([gru.convz.weight, gru.convr.weight]), torch.cat([gru.convz.bias, gru.convr.bias])
        plane_zr = F.conv2d(context, wzr[:, ctx], bzr, padding=pad)
        plane_q = F.conv2d(context, gru.convq.weight[:, ctx], gru.convq.bias, padding=pad)
        v = F.conv2d(torch.cat([h, m, flow], dim=1), wzr[:, rest], None, padding=pad) + plane_zr
        z, rh = torch.sigmoid(v[:, :HIDDEN]), torch.sigmoid(v[:, HIDDEN:]) * h
        q = torch.tanh(F.conv2d(torch.cat([rh, m, flow], dim=1), gru.convq.weight[:, rest], None, padding=pad) + plane_q)
        h = (1 - z) * h + z * q
    d = torch.relu(F.conv2d(h, fh.conv1.weight, fh.conv1.bias, padding=1))
    delta = F.conv2d(d, fh.conv2.weight, fh.conv2.bias, padding=1)
    mh = torch.relu(F.conv2d(h, mask_predictor.convrelu[0].weight, mask_predictor.convrelu[0].bias, padding=1))
    return h, delta, 0.25 * F.conv2d(mh, mask_predictor.conv.weight, mask_predictor.conv.bias)
