"""Cases and the float64 oracles of RAFT-large's fused encoders (eogs2_amd.raft.fold_batchnorm / FusedEncoderLarge, the
eogs_flowres_* entries of include/eogs_resample.h), shared by the CPU tests (tests/test_flowres_cases.py,
tests/test_flowres_api.py) and the GPU tests (tests/test_gpu_flowres.py). Everything is computed from seeds: no fixture,
nothing outside the repository.

  CASES                   every distinct convolution of RAFT-large's two encoders, in tests/flowenc_cases.py's form
  randomise_batchnorms    default-initialised batch norms are the identity and would hide a wrong fold: every test that
                          involves one randomises it first
  fold_oracle             the header's statement of eogs_flowres_fold: (s float32, w' float32, b' float64 before its rounding)
  residual_block_oracle   relu(S + relu(norm(conv2(relu(norm(conv1(x))))))) of one raft.ResidualBlock, in float64, the norm written out
  encoder_oracle          a whole encoder the same way; tests/test_flowres_cases.py holds both against the modules' forward
"""
import torch
import torch.nn.functional as F

# (Cin, Cout, k, stride, the input is NCHW)
CASES = (
    (3, 64, 7, 2, True),      # the stem, on the image
    (64, 64, 3, 1, False),    # layer1
    (64, 96, 3, 2, False),    # layer2.0's first convolution
    (96, 96, 3, 1, False),    # layer2
    (64, 96, 1, 2, False),    # layer2.0's downsample
    (96, 128, 3, 2, False),   # layer3.0's first convolution
    (128, 128, 3, 1, False),  # layer3
    (96, 128, 1, 2, False),   # layer3.0's downsample
    (128, 256, 1, 1, False),  # the head
)
ENCODER_IMAGES = ((2, 3, 17, 23), (1, 3, 40, 56))
FOLD_SHAPES = ((1, 1), (5, 27), (64, 147), (128, 1152))  # (Cout, per_out = Cin k k)
EPS = 1e-5


def encoder_convs(encoder):
    """(Cin, Cout, k, stride, NCHW) of every nn.Conv2d of a raft.FeatureEncoder, in module order."""
    out = []
    for name, m in encoder.named_modules():
        if isinstance(m, torch.nn.Conv2d):
            assert m.kernel_size[0] == m.kernel_size[1] and m.stride[0] == m.stride[1] and m.padding[0] == (m.kernel_size[0] - 1) // 2
            out.append((m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], name == "convnormrelu.0"))
    return out


def bn_values(C, generator):
    """(gamma, beta, running mean, running var) of C channels: gamma uniform in [0.5, 1.5] with a quarter of the values
    negated and every 16th exactly 0, beta and the mean N(0, 0.5^2), var uniform in [0.5, 2]."""
    gamma = torch.rand(C, generator=generator) + 0.5
    idx = torch.arange(C)
    gamma[idx % 4 == 1] *= -1.0
    gamma[idx % 16 == 0] = 0.0
    beta, mean = torch.randn(C, generator=generator) * 0.5, torch.randn(C, generator=generator) * 0.5
    var = torch.rand(C, generator=generator) * 1.5 + 0.5
    return gamma, beta, mean, var


def randomise_batchnorms(module, seed):
    """Fills every BatchNorm2d below `module` with bn_values, in module order from one seeded generator; returns how many."""
    g = torch.Generator().manual_seed(seed)
    count = 0
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                gamma, beta, mean, var = bn_values(m.num_features, g)
                m.weight.copy_(gamma)
                m.bias.copy_(beta)
                m.running_mean.copy_(mean)
                m.running_var.copy_(var)
                count += 1
    return count


def fold_case(cout, per_out, seed):
    """(weight [cout, per_out, 1, 1], bias, gamma, beta, mean, var) in float32."""
    g = torch.Generator().manual_seed(seed)
    weight = torch.randn(cout, per_out, 1, 1, generator=g) / per_out ** 0.5
    bias = torch.randn(cout, generator=g) * 0.5
    return (weight, bias) + bn_values(cout, g)


def fold_oracle(weight, bias, gamma, beta, mean, var, eps=EPS):
    """The statement of eogs_flowres_fold: s = float(gamma / sqrt(double(var) + eps)); w' = float(double(w) double(s)), which is
    the one float32 product (a product of two float32 values is exact in double); b' = (double(b) - double(mean)) double(s)
    + double(beta) in float64, BEFORE its rounding to float32. Returns (s, w', b')."""
    s = (gamma.double() / torch.sqrt(var.double() + eps)).float()
    shape = (-1,) + (1,) * (weight.ndim - 1)
    w2 = (weight.double() * s.double().view(shape)).float()
    b2 = (bias.double() - mean.double()) * s.double() + beta.double()
    return s, w2, b2


def _norm_of(unit):
    found = [m for m in list(unit)[1:] if not isinstance(m, torch.nn.ReLU)]
    assert len(found) == 1, unit
    return found[0]


def _unit(x, unit, act=True):
    """conv -> norm written out -> ReLU of one Conv2dNormActivation, on NCHW in the dtype of x: the instance norm with the
    map's own biased statistics, the batch norm with its running ones."""
    conv, norm = unit[0], _norm_of(unit)
    v = F.conv2d(x, conv.weight, conv.bias, stride=conv.stride, padding=conv.padding)
    if isinstance(norm, torch.nn.InstanceNorm2d):
        mean = v.mean(dim=(2, 3), keepdim=True)
        var = ((v - mean) ** 2).mean(dim=(2, 3), keepdim=True)
        v = (v - mean) * (1.0 / torch.sqrt(var + EPS))
    else:
        assert isinstance(norm, torch.nn.BatchNorm2d) and not norm.training
        c = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
        v = (v - c(norm.running_mean)) / torch.sqrt(c(norm.running_var) + EPS) * c(norm.weight) + c(norm.bias)
    return torch.relu(v) if act else v


def residual_block_oracle(block, x):
    """relu(S + y) of one raft.ResidualBlock: S is x, or the normalised, not rectified 1 x 1 stride-2 downsample."""
    y = _unit(_unit(x, block.convnormrelu1), block.convnormrelu2)
    s = x if isinstance(block.downsample, torch.nn.Identity) else _unit(x, block.downsample, act=False)
    return torch.relu(s + y)


def encoder_oracle(enc, x):
    """A raft.FeatureEncoder of residual blocks as include/eogs_resample.h states it, in the dtype of `enc` and `x` [N, 3, H, W]."""
    x = _unit(x, enc.convnormrelu)
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for block in layer:
            x = residual_block_oracle(block, x)
    return F.conv2d(x, enc.conv.weight, enc.conv.bias)
