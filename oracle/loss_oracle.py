"""CPU oracle of the photometric loss — TEST INFRASTRUCTURE ONLY (never imported by eogs2_amd/).

A float64 restatement of the reference's algorithm:
  l1_loss  src/gaussiansplatting/utils/loss_utils.py:18-19
  gaussian / create_window (sigma 1.5, 11 taps, fp32 outer product)  loss_utils.py:26-42
  ssim / _ssim (five depthwise conv2d, zero padding 5, C1=0.01^2, C2=0.03^2)  loss_utils.py:45-85
  lphotom  src/gaussiansplatting/utils/image_utils.py:27-28
Gradients come from torch autograd over this restatement. Pinned against the reference's own functions through
tests/golden/loss_*.npz (tests/golden/make_golden_loss.py imports the reference module to generate them).

Every function takes `dtype`. float64 (the default) is the oracle. float32 is the reference's own arithmetic: the same
operations in the same order on fp32 tensors (the fp32 2-D window, five depthwise conv2d, the elementwise map), which is what
the distance "the reference's fp32 run to float64" in tests/loss_cases.py is measured with.
"""
from math import exp

import torch
import torch.nn.functional as F

C1, C2 = 0.01**2, 0.03**2


def window_2d(window_size=11, sigma=1.5, dtype=torch.float64):
    g = torch.tensor([exp(-((x - window_size // 2) ** 2) / float(2 * sigma**2)) for x in range(window_size)],
                     dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).to(dtype)  # the reference builds the 2-D window in fp32 (loss_utils.py:36-38)


def l1_loss(x, y, dtype=torch.float64):
    return (x.to(dtype) - y.to(dtype)).abs().mean()


def _conv(t, window_size, dtype):
    C = t.shape[1]
    w = window_2d(window_size, dtype=dtype).expand(C, 1, window_size, window_size).contiguous()
    return F.conv2d(t, w, padding=window_size // 2, groups=C)


def _map(mu1, mu2, e11, e22, e12):
    """_ssim's elementwise part (loss_utils.py:60-80) from the five window sums."""
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    return ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s11 + s22 + C2))


def ssim_map(x, y, window_size=11, dtype=torch.float64):
    x, y = x.to(dtype), y.to(dtype)
    squeeze = x.ndim == 3
    if squeeze:
        x, y = x[None], y[None]
    conv = lambda t: _conv(t, window_size, dtype)
    m = _map(conv(x), conv(y), conv(x * x), conv(y * y), conv(x * y))
    return m[0] if squeeze else m


def ssim(x, y, window_size=11, size_average=True, dtype=torch.float64):
    m = ssim_map(x, y, window_size, dtype)
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def lphotom(x, y, lambda_dssim, dtype=torch.float64):
    return (1.0 - lambda_dssim) * l1_loss(x, y, dtype) + lambda_dssim * (1.0 - ssim(x, y, dtype=dtype))


def ssim_addends(x, y, window_size=11):
    """float64 [3, *x.shape]: the three addends of d sum(ssim_map) / dx per pixel, as csrc/loss.hip forms them,
        W*Dm,  2x . W*D11,  y . W*D12
    with Dm, D11, D12 the derivatives of the summed map with respect to the window sums mu1, E[x^2], E[xy] (autograd over
    `_map` with the sums as leaves) and W* the zero-padded window, which is symmetric and so its own adjoint. Their sum is the
    autograd gradient of ssim_map(x, y).sum() to float64 rounding; each alone is what one fp32 product of the kernel's last
    line carries, so their magnitudes say how small an fp32 sum of them can be told from zero."""
    dt = torch.float64
    x, y = x.detach().to(dt), y.detach().to(dt)
    shape = x.shape
    if x.ndim < 4:
        x, y = x.reshape((1, -1) + tuple(shape[-2:])), y.reshape((1, -1) + tuple(shape[-2:]))
    conv = lambda t: _conv(t, window_size, dt)
    mu1, e11, e12 = (conv(t).requires_grad_(True) for t in (x, x * x, x * y))
    dm, d11, d12 = torch.autograd.grad(_map(mu1, conv(y), e11, conv(y * y), e12).sum(), (mu1, e11, e12))
    return torch.stack([conv(dm), 2 * x * conv(d11), y * conv(d12)]).reshape((3,) + tuple(shape))
