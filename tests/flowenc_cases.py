"""Cases and the float64 oracle of the flow network's fused encoders (eogs2_amd.raft.conv2d_strided_cl / finish_cl / FusedEncoder,
the eogs_flowenc_* entries of include/eogs_resample.h), shared by the CPU test of the oracle itself
(tests/test_flowenc_cases.py) and the GPU tests (tests/test_gpu_flowenc.py). Everything is computed from seeds: no fixture,
nothing outside the repository.

  strided_oracle   F.conv2d with a stride on a channel-last map, in the dtype of its inputs (the tests pass float64), with
                   the on-load transform max((x - mean) rstd, 0) from the float32 (mean, rstd) table the kernel is given;
                   with `magnitude=True` the M of the error bound: |bias| + conv(|x|, |W|), x after the transform's
                   product and before its ReLU
  stats_oracle     float64 mean, biased variance and rstd = 1 / sqrt(var + 1e-5) of a stored float32 map, per image and channel
  finish_oracle    relu(S + relu((v - mean) rstd)) with the three shortcut forms, from float32 tables
  encoder_oracle   a whole encoder as the header states it, unit by unit; tests/test_flowenc_cases.py holds it against
                   raft.FeatureEncoder.forward in float64
"""
import math

import torch
import torch.nn.functional as F

# (Cin, Cout, k, stride, the input is NCHW): every distinct convolution of RAFT-small's two encoders
CONFIGS = (
    (3, 32, 7, 2, True),                                                        # the stem, on the image
    (32, 8, 1, 1, False), (8, 32, 1, 1, False), (32, 16, 1, 1, False), (16, 64, 1, 1, False), (64, 16, 1, 1, False),
    (64, 24, 1, 1, False), (24, 96, 1, 1, False), (96, 24, 1, 1, False),       # the bottlenecks' 1 x 1 units
    (96, 128, 1, 1, False), (96, 160, 1, 1, False),                             # the two heads
    (8, 8, 3, 1, False), (16, 16, 3, 1, False), (24, 24, 3, 1, False),          # the 3 x 3 units of the stride-1 blocks
    (16, 16, 3, 2, False), (24, 24, 3, 2, False),                               # ... of layer2.0 and layer3.0
    (32, 64, 1, 2, False), (64, 96, 1, 2, False),                               # the two downsamples
)
SHAPES = ((1, 1, 1), (1, 2, 2), (1, 5, 7), (2, 17, 19))  # (N, h, w) of the INPUT; tests add one from the kernel's position tile
STATS_SHAPES = ((1, 5, 7), (2, 17, 19))                   # maps of more than one position: the statistics' condition can hold
ENCODER_IMAGES = ((2, 3, 17, 23), (1, 3, 40, 56))
EPS = 1e-5


def config_id(c):
    return f"{c[0]}to{c[1]}k{c[2]}s{c[3]}" + ("nchw" if c[4] else "")


def out_size(h, w, stride):
    return (h + stride - 1) // stride, (w + stride - 1) // stride


def tile_input(config, tile_w, tile_h):
    """The input (N, h, w) whose OUTPUT is one row and one column more than whole position tiles; under stride 2 the sizes are
    odd, so the last output row and column have their windows half outside."""
    s = config[3]
    return (1, s * (tile_h + 1) - (s - 1), s * (2 * tile_w + 1) - (s - 1))


def conv_case(config, shape, seed):
    """(input, weight, bias, in_norm, res) in float32: the input [N, h, w, Cin] or [N, Cin, h, w], the weight scaled so that
    outputs are O(1), an (mean, rstd) table [N, Cin, 2] with rstd in [0.5, 2], res [N, h', w', Cout]."""
    cin, cout, k, s, nchw = config
    N, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, cin, h, w) if nchw else (N, h, w, cin), generator=g)
    weight = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    bias = torch.randn(cout, generator=g) * 0.5
    table = torch.stack([torch.randn(N, cin, generator=g) * 0.5, torch.rand(N, cin, generator=g) * 1.5 + 0.5], dim=-1)
    ho, wo = out_size(h, w, s)
    res = torch.randn(N, ho, wo, cout, generator=g)
    return x, weight, bias, table, res


def _normalised(x_nchw, in_norm):
    t = in_norm.to(x_nchw.dtype)
    return (x_nchw - t[:, :, 0, None, None]) * t[:, :, 1, None, None]


def strided_oracle(x, weight, bias, stride=1, in_norm=None, act="none", res=None, in_nchw=False, magnitude=False):
    """[N, h', w', Cout] in the dtype of `x`. `in_norm` is the float32 table the kernel reads; act "none" or "relu"; with `res`
    the result is relu(res + relu(v)). magnitude=True: M (+ |res| with `res`)."""
    xn = x if in_nchw else x.permute(0, 3, 1, 2)
    k = weight.shape[-1]
    if in_norm is not None:
        xn = _normalised(xn, in_norm)
    if magnitude:
        out = F.conv2d(xn.abs(), weight.abs(), None, stride=stride, padding=(k - 1) // 2).permute(0, 2, 3, 1)
        if bias is not None:
            out = out + bias.abs()
        return out if res is None else out + res.abs()
    if in_norm is not None:
        xn = torch.relu(xn)
    v = F.conv2d(xn, weight, bias, stride=stride, padding=(k - 1) // 2).permute(0, 2, 3, 1)
    if res is not None:
        return torch.relu(res + torch.relu(v))
    return torch.relu(v) if act == "relu" else v


def stats_oracle(stored):
    """(mean, var, rstd), each float64 [N, C], of a stored float32 channel-last map [N, h, w, C]."""
    v = stored.double().flatten(1, 2)
    mean = v.mean(dim=1)
    var = ((v - mean[:, None]) ** 2).mean(dim=1)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def stats_condition(stored):
    """The smallest var / E[v^2] over the (image, channel) pairs of a map: the statistics' bound holds from 2^-8 up."""
    v = stored.double().flatten(1, 2)
    _, var, _ = stats_oracle(stored)
    return float((var / (v ** 2).mean(dim=1).clamp_min(1e-300)).min())


def finish_oracle(v, norm_v, s=None, norm_s=None, magnitude=False):
    """relu(S + relu((v - mean) rstd)) on channel-last maps in the dtype of `v`, the tables float32 [N, C, 2]. magnitude=True:
    |S| + |(v - mean) rstd|."""
    def norm(x, t):
        t = t.to(x.dtype)
        return (x - t[:, None, None, :, 0]) * t[:, None, None, :, 1]

    y = norm(v, norm_v)
    sc = torch.zeros_like(v) if s is None else s if norm_s is None else norm(s, norm_s)
    if magnitude:
        return sc.abs() + y.abs()
    return torch.relu(sc + torch.relu(y))


def _unit(x, conv, norm, act=True):
    """conv -> statistics -> (v - mean) rstd -> ReLU, on NCHW in the dtype of x."""
    v = F.conv2d(x, conv.weight, conv.bias, stride=conv.stride, padding=conv.padding)
    if norm:
        mean = v.mean(dim=(2, 3), keepdim=True)
        var = ((v - mean) ** 2).mean(dim=(2, 3), keepdim=True)
        v = (v - mean) * (1.0 / torch.sqrt(var + EPS))
    return torch.relu(v) if act else v


def block_oracle(block, x, norm):
    """relu(S + y) of one raft.BottleneckBlock: S is x, or the (normalised, not rectified) 1 x 1 stride-2 downsample."""
    y = _unit(_unit(_unit(x, block.convnormrelu1[0], norm), block.convnormrelu2[0], norm), block.convnormrelu3[0], norm)
    s = x if isinstance(block.downsample, torch.nn.Identity) else _unit(x, block.downsample[0], norm, act=False)
    return torch.relu(s + y)


def encoder_oracle(enc, x, norm):
    """A raft.FeatureEncoder of bottleneck blocks as include/eogs_resample.h states it, in the dtype of `enc` and `x`
    [N, 3, H, W]; `norm`: whether every unit but the head normalises."""
    x = _unit(x, enc.convnormrelu[0], norm)
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for block in layer:
            x = block_oracle(block, x, norm)
    return F.conv2d(x, enc.conv.weight, enc.conv.bias)
