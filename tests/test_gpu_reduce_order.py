"""GPU: the masked L1 loss against the numpy restatement of csrc/reduce.h's two-stage sum (tests/reduce_cases.py), bit for bit.

`shade.suncamera_l` / `shade.randomcam_l` (three planes, both mask modes) and `randomcam.cmloss` (one to four planes) run
one kernel pair and one reduce epilogue. At four shapes — one lane; two workgroups and a partial wave; 301 workgroups, so the
column sum makes a second trip; the grid at its cap with a second grid-stride trip — all three outputs {S_alt / N, S_rgb / N,
N} equal the restatement in every bit, and the backward's g_alt equals (upstream / N * mask) * sgn(d) formed from the restated
N. tests/test_reduce_cases.py shows that another order would give other bits on these inputs.
"""
import functools

import numpy as np
import pytest
import torch

import reduce_cases as RC

pytestmark = pytest.mark.gpu
UP = (0.7, -1.3)  # upstream gradients of the two losses


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(H, W, C, mode):
    """The inputs and what the restatement makes of them: computed once, shared, left unchanged."""
    alt, uv, a, b = RC.inputs(H, W, C)
    out, m = RC.masked_l1(mode, alt, uv, a, b)
    g = RC.g_alt(UP[0], out[2], m, alt)
    for x in (alt, uv, a, b, out, g):
        x.setflags(write=False)
    return alt, uv, a, b, out, g


def bits(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def run(fn, dev, alt, uv, a, b):
    """fn(alt, a, b, uv) -> out[3] on the device; returns out and d(UP . out[:2]) / d alt."""
    t = [torch.from_numpy(np.array(x)).to(dev) for x in (alt, a, b, uv)]
    t[0].requires_grad_(True)
    out = fn(*t)
    (g_alt,) = torch.autograd.grad(out, t[0], torch.tensor([UP[0], UP[1], 0.0], device=dev))
    return out, g_alt


def check(fn, dev, H, W, C, mode):
    alt, uv, a, b, want, want_g = case(H, W, C, mode)
    out, g_alt = run(fn, dev, alt, uv, a, b)
    print(f"{H}x{W} C={C} mode={mode}: got {out.tolist()}  restated {want.tolist()}")
    assert out.shape == (3,) and out.dtype == torch.float32
    assert np.array_equal(bits(out), bits(want)), (out.tolist(), want.tolist())
    assert g_alt.shape == (H, W) and np.array_equal(bits(g_alt), bits(want_g))


@pytest.mark.parametrize("H,W", RC.SHAPES)
@pytest.mark.parametrize("mode", [RC.MODE_SUN, RC.MODE_RANDOM])
def test_mloss_is_the_restated_order_bit_for_bit(dev, H, W, mode):
    from eogs2_amd.shade import _MaskedLoss

    check(lambda alt, a, b, uv: _MaskedLoss.apply(alt, a, b, uv, mode), dev, H, W, 3, mode)


@pytest.mark.parametrize("H,W", RC.SHAPES)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_cmloss_is_the_restated_order_bit_for_bit(dev, H, W, C):
    from eogs2_amd.randomcam import _CMLoss

    check(_CMLoss.apply, dev, H, W, C, RC.MODE_RANDOM)
