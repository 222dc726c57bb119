"""Cases and the float64 oracle of the flow network's update block (eogs2_amd.raft.conv2d_cl / FusedUpdate, the eogs_flownet_*
entries of include/eogs_resample.h), shared by the CPU test of the oracle itself (tests/test_flownet_cases.py) and the GPU
tests (tests/test_gpu_flownet.py; tests/test_gpu_flownet_general.py for GENERAL and GATE_CONFIGS, the kernel beyond the update's
own convolutions). Everything is computed from seeds: no fixture, nothing outside the repository.

  conv_oracle     F.conv2d(torch.cat(inputs)) on NCHW views, in the dtype of its inputs (the tests pass float64); with
                  `magnitude=True` |add| + |bias| + conv(|x|, |W|): the M of the error bound
  update_oracle   one update as the header states it: the context's share of the three GRU convolutions as a plane formed
                  from the context alone, z and r from ONE 192-wide convolution, the blend. tests/test_flownet_cases.py holds
                  it against raft.UpdateBlock.forward in float64, which proves the hoisting identity and the channel slices.
"""
import math

import torch
import torch.nn.functional as F

# (input channel segments, Cout, k, with add, activation): exactly the convolutions of RAFT-small's update
CONFIGS = (
    ((196,), 96, 1, False, "relu"),     # convcorr1
    ((2,), 64, 7, False, "relu"),       # convflow1
    ((64,), 32, 3, False, "relu"),      # convflow2
    ((96, 32), 80, 3, False, "relu"),   # conv of the motion encoder
    ((64,), 288, 3, False, "none"),     # the hoisted context planes
    ((96, 82), 192, 3, True, "none"),   # convz | convr without the context's channels, the plane added
    ((96,), 128, 3, False, "relu"),     # flow head, conv1
    ((128,), 2, 3, False, "none"),      # flow head, conv2
)
SHAPES = ((1, 1, 1), (1, 5, 7), (1, 16, 16), (2, 17, 19))  # (N, h, w); tests add one shape from the kernel's position tile
STEP_SHAPES = ((1, 16, 16), (2, 17, 19))
# The kernel beyond the update's eight, in the same form: what each line reaches of csrc/flownet.hip (a chunk is eight input
# channels, a block sixteen output channels, NB the blocks per workgroup; tests/test_flownet_cases.py holds these claims)
GENERAL = (
    # k = 5; NB = 2, the second block with one real column
    ((3,), 17, 5, False, "none"),
    # k = 7 over two chunks (the hand-over from a chunk's last tap row to the next chunk's input and first tap row), two
    # segments; NB = 2, two workgroups along Cout, the last block with two real columns
    ((8, 8), 50, 7, False, "relu"),
    # k = 5 over two chunks; seven blocks under NB = 2: the last workgroup's second block is padding throughout
    ((12,), 112, 5, True, "none"),
    # three ragged segments (5: one real lane in the chunk's second instruction; 9: a second chunk of one channel; 1);
    # NB = 3 with 15 padded columns
    ((5, 9, 1), 33, 3, True, "relu"),
    # exactly four channels (the boundary at which a chunk's second instruction is skipped), Cout = 1
    ((4,), 1, 1, False, "none"),
)
GENERAL_SHAPES = ((1, 1, 1), (2, 9, 17))  # and the position tile's shape, as above
LAYOUT_SHAPES = ((2, 9, 17),)             # and the position tile's shape
# (segments, Cout, k, with add, epilogue): the gate epilogues at the update's sizes and at one small ragged pair
GATE_CONFIGS = (
    ((96, 80, 2), 192, 3, True, "gates"),
    ((96, 80, 2), 96, 3, True, "gru"),
    ((5, 9, 1), 34, 3, True, "gates"),
    ((5, 9, 1), 33, 3, True, "gru"),
)
CHUNK, BLOCK = 8, 16  # input channels per staged chunk, output channels per block
HIDDEN, CONTEXT, CORR = 96, 64, 196


def config_id(c):
    return "+".join(map(str, c[0])) + f"to{c[1]}k{c[2]}"


def conv_case(config, shape, seed):
    """(inputs [N, h, w, C_i] float32, weight, bias, add or None): the weight scaled so that outputs are O(1)."""
    segs, cout, k, with_add, _ = config
    N, h, w = shape
    g = torch.Generator().manual_seed(seed)
    inputs = [torch.randn(N, h, w, c, generator=g) for c in segs]
    weight = torch.randn(cout, sum(segs), k, k, generator=g) / math.sqrt(sum(segs) * k * k)
    bias = torch.randn(cout, generator=g)
    add = torch.randn(N, h, w, cout, generator=g) if with_add else None
    return inputs, weight, bias, add


def gate_case(config, shape, seed):
    """conv_case and the operands of a gate epilogue: (inputs, weight, bias, add, aux, h). GATES: aux = h, tanh(randn) as
    [N, h, w, Cout / 2]. GRU: aux = z, sigmoid(randn), and h, tanh(randn), what `out` holds before the call, both
    [N, h, w, Cout]."""
    segs, cout, k, with_add, epi = config
    inputs, weight, bias, add = conv_case(config, shape, seed)
    g = torch.Generator().manual_seed(seed + 1)
    N, h, w = shape
    if epi == "gates":
        hid = torch.tanh(torch.randn(N, h, w, cout // 2, generator=g))
        return inputs, weight, bias, add, hid, hid
    return inputs, weight, bias, add, torch.sigmoid(torch.randn(N, h, w, cout, generator=g)), torch.tanh(torch.randn(N, h, w, cout, generator=g))


def conv_oracle(inputs, weight, bias, act="none", add=None, magnitude=False):
    """[N, h, w, Cout] from channel-last inputs, in their dtype."""
    x = torch.cat([t.permute(0, 3, 1, 2) for t in inputs], dim=1)
    k = weight.shape[-1]
    if magnitude:
        out = F.conv2d(x.abs(), weight.abs(), None, padding=(k - 1) // 2).permute(0, 2, 3, 1)
        if bias is not None:
            out = out + bias.abs()
        return out if add is None else out + add.abs()
    out = F.conv2d(x, weight, bias, padding=(k - 1) // 2).permute(0, 2, 3, 1)
    if add is not None:
        out = out + add
    return torch.relu(out) if act == "relu" else out


def update_inputs(N, h, w, seed):
    """(hidden, context, corr, flow) float32 NCHW: tanh(randn), relu(randn), randn, a flow within +-3 px."""
    g = torch.Generator().manual_seed(seed)
    return (torch.tanh(torch.randn(N, HIDDEN, h, w, generator=g)), torch.relu(torch.randn(N, CONTEXT, h, w, generator=g)),
            torch.randn(N, CORR, h, w, generator=g), (torch.rand(N, 2, h, w, generator=g) * 2 - 1) * 3)


def update_oracle(block, hidden, context, corr, flow):
    """(new hidden, delta) of one update of RAFT-small's `block` (a raft.UpdateBlock) as include/eogs_resample.h states it,
    in the dtype of the block and the inputs."""
    me, gru, fh = block.motion_encoder, block.recurrent_block.convgru1, block.flow_head
    c = torch.relu(F.conv2d(corr, me.convcorr1[0].weight, me.convcorr1[0].bias))
    f1 = torch.relu(F.conv2d(flow, me.convflow1[0].weight, me.convflow1[0].bias, padding=3))
    f2 = torch.relu(F.conv2d(f1, me.convflow2[0].weight, me.convflow2[0].bias, padding=1))
    m = torch.relu(F.conv2d(torch.cat([c, f2], dim=1), me.conv[0].weight, me.conv[0].bias, padding=1))
    # convz / convr / convq read [h | context | motion | flow]
    ctx = list(range(HIDDEN, HIDDEN + CONTEXT))
    rest = list(range(HIDDEN)) + list(range(HIDDEN + CONTEXT, gru.convz.weight.shape[1]))
    wzr, bzr = torch.cat([gru.convz.weight, gru.convr.weight]), torch.cat([gru.convz.bias, gru.convr.bias])
    plane_zr = F.conv2d(context, wzr[:, ctx], bzr, padding=1)
    plane_q = F.conv2d(context, gru.convq.weight[:, ctx], gru.convq.bias, padding=1)
    v = F.conv2d(torch.cat([hidden, m, flow], dim=1), wzr[:, rest], None, padding=1) + plane_zr
    z, rh = torch.sigmoid(v[:, :HIDDEN]), torch.sigmoid(v[:, HIDDEN:]) * hidden
    q = torch.tanh(F.conv2d(torch.cat([rh, m, flow], dim=1), gru.convq.weight[:, rest], None, padding=1) + plane_q)
    new = (1 - z) * hidden + z * q
    d = torch.relu(F.conv2d(new, fh.conv1.weight, fh.conv1.bias, padding=1))
    return new, F.conv2d(d, fh.conv2.weight, fh.conv2.bias, padding=1)
