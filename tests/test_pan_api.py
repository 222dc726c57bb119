"""CPU: the C-ABI of include/eogs_pan.h and the host side of eogs2_amd.pan. No kernel is launched (every call here is
rejected, or answered, before a launch)."""
import ctypes
import os
import re
import types

import pytest
import torch

import abi_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    return sorted(set(re.findall(r"\b(eogs_pan_[a-z_0-9]+)\s*\(", AC.header_text("eogs_pan.h"))))


def test_header_and_binding_agree():
    from eogs2_amd._abi import HEADERS, HIP_ONLY

    assert header_symbols() == sorted(HEADERS["eogs_pan.h"]) == ["eogs_pan_backward", "eogs_pan_bytes", "eogs_pan_forward"]
    assert not set(HEADERS["eogs_pan.h"]) & AC.elsewhere("eogs_pan.h")
    assert set(HEADERS["eogs_pan.h"]) <= set(HIP_ONLY)


def test_header_constants_match_python():
    from eogs2_amd import _abi

    src = open(os.path.join(ROOT, "include", "eogs_pan.h")).read()
    defs = dict(re.findall(r"^#define EOGS_(PAN_[A-Z_]+) (\d+)$", src, flags=re.M))
    assert len(defs) == 10
    for name, value in defs.items():
        assert getattr(_abi, name) == int(value), name


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def test_library_exports_the_symbols_at_abi_8(hip_lib):
    assert hip_lib.backend == "hip-gfx950"
    assert hip_lib.cdll.eogs_rast_abi_version() == 8
    for name in header_symbols():
        assert hasattr(hip_lib.cdll, name), name
    assert hip_lib.pan_bytes.argtypes is not None  # bound through the "pan_" short name


def test_entry_points_reject_bad_arguments_before_any_launch(hip_lib):
    n = ctypes.c_size_t()
    hip_lib.check(hip_lib.pan_bytes(33, 65, ctypes.byref(n)))
    assert 20 * 4 <= n.value < (1 << 20)
    assert hip_lib.pan_bytes(0, 65, ctypes.byref(n)) == -1 and b"pan_bytes" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.pan_bytes(33, 65, None) == -1
    p = ctypes.c_void_p(4096)  # never dereferenced: each call below returns before a launch
    err = hip_lib.cdll.eogs_rast_last_error
    # forward: NULL images, unknown order / kind, a map kind without its parameters, shadow without alt_diff
    assert hip_lib.pan_forward(4, 4, 0, 2, None, None, p, None, p, p, p, None, None) == -1 and b"pan_forward" in err()
    assert hip_lib.pan_forward(4, 4, 0, 2, p, None, p, None, p, p, None, None, None) == -1 and b"pan_forward" in err()
    assert hip_lib.pan_forward(4, 4, 2, 2, p, None, p, None, p, p, p, None, None) == -1 and b"order" in err()
    assert hip_lib.pan_forward(4, 4, 0, 7, p, None, p, None, p, p, p, None, None) == -1 and b"kind" in err()
    assert hip_lib.pan_forward(4, 4, 0, 2, p, None, p, None, None, p, p, None, None) == -1 and b"map_params" in err()
    assert hip_lib.pan_forward(4, 4, 0, 0, p, None, p, None, None, p, p, p, None) == -1 and b"pan_forward" in err()
    assert hip_lib.pan_forward(4, 4, 0, 0, p, p, p, None, None, p, p, p, None) == -1 and b"inshadow" in err()
    assert hip_lib.pan_forward(4, 4, 1, 0, p, None, p, None, None, None, p, None, None) == -1  # order B needs cc
    assert hip_lib.pan_forward(0, 4, 0, 0, p, None, p, None, None, p, p, None, None) == -1 and b"sizes" in err()
    # backward: NULL workspace, too-small workspace, g_alt_diff without alt_diff
    args = (4, 4, 0, 0, p, None, p, None, None, p, None, None, p, None, p)
    assert hip_lib.pan_backward(*args, None, n.value, None) == -1
    assert b"pan_backward" in err() and b"NULL" in err()
    assert hip_lib.pan_backward(*args, p, n.value - 1, None) == -3
    assert b"pan_backward" in err() and b"workspace" in err()
    assert hip_lib.pan_backward(*args, p, 0, None) == -3
    assert hip_lib.pan_backward(4, 4, 0, 0, p, None, p, None, None, p, None, None, p, p, p, p, n.value, None) == -1
    assert b"pan_backward" in err()
    assert hip_lib.pan_backward(4, 4, 0, 0, p, None, p, None, None, p, None, None, None, None, p, p, n.value, None) == -1


# ---- duck-typed modules: the names and attributes of scene/msi_to_pan/transf_msi_to_pan.py --------------------------
def _module(name, **attrs):
    return type(name, (), attrs)()


def _conv(cin=3, k=1):
    return torch.nn.Conv2d(cin, 1, kernel_size=k, padding="same")


def test_pan_map_of_recognises_each_module():
    from eogs2_amd.pan import PanMap, pan_map_of

    assert pan_map_of(_module("msi_to_pan_identity")).kind == "identity"
    assert pan_map_of(_module("msi_to_pan_identity")).planes == 3
    assert pan_map_of(_module("only_one_channel", num_channel=0)).kind == "only_one_channel"
    assert pan_map_of(_module("average_msitopan")).kind == "average"
    p = torch.arange(5.0)
    m = pan_map_of(_module("base_msi_to_pan", pan_params=p))
    assert m.kind == "fixed" and m.params is p and m.planes == 1
    q = torch.nn.Parameter(torch.arange(5.0), requires_grad=False)
    m = pan_map_of(_module("learnable_base_msi_to_pan", pan_params=q))
    assert m.kind == "learnable_fixed" and m.params is q
    lin = _conv()
    m = pan_map_of(_module("MSI_TO_PAN", linear=lin, remove_sigm=True))
    assert m.kind == "base" and m.remove_sigm and m.weight is lin.weight and m.bias is lin.bias
    assert not pan_map_of(_module("MSI_TO_PAN", linear=lin, remove_sigm=False)).remove_sigm
    fw, fb = torch.ones(1, 3, 1, 1), torch.zeros(1)
    for learn in (False, True):
        m = pan_map_of(_module("msi_to_pan_fixedandtranslate", linear=lin, fixed_weights=fw, fixed_bias=fb, learn_conv2d=learn))
        assert m.kind == "fixedandtranslate" and m.learn_conv2d is learn and m.differentiable is learn
        assert m.fixed_weights is fw and m.weight is lin.weight
    own = PanMap("average")
    assert pan_map_of(own) is own
    with pytest.raises(RuntimeError, match="unknown MSI->PAN module"):
        pan_map_of(torch.nn.Identity())
    with pytest.raises(ValueError, match="Unknown MSI to PAN conversion type"):
        PanMap("brovey")
    with pytest.raises(RuntimeError, match="5 values"):
        PanMap("fixed", params=torch.zeros(4))


def test_convolutional_and_pooled_maps_stay_the_callers():
    from eogs2_amd.pan import pan_map_of

    with pytest.raises(NotImplementedError, match="kernel_size"):
        pan_map_of(_module("MSI_TO_PAN", linear=_conv(k=3), remove_sigm=False))
    with pytest.raises(NotImplementedError, match="use_avgpool"):
        pan_map_of(_module("MSI_TO_PAN", linear=torch.nn.AvgPool2d(kernel_size=1, ceil_mode=True), remove_sigm=False))
    with pytest.raises(NotImplementedError, match="kernel_size"):
        pan_map_of(_module("msi_to_pan_fixedandtranslate", linear=_conv(k=3), fixed_weights=torch.ones(1, 3, 1, 1),
                           fixed_bias=torch.zeros(1), learn_conv2d=True))


def test_identity_in_the_map_first_order_raises():
    from eogs2_amd.pan import PanMap, pan_shade, render_pipeline

    raw = torch.rand(3, 4, 4)
    with pytest.raises(RuntimeError, match="identity"):
        pan_shade(raw, None, torch.tensor([1.0, 0.0]), None, PanMap("identity"), "map_first")
    cam = types.SimpleNamespace(weird_pan_setup=True, use_shadow=False, color_correction=torch.nn.Conv2d(1, 1, 1),
                                msi_to_pan=_module("msi_to_pan_identity"))
    with pytest.raises(RuntimeError, match="identity"):
        render_pipeline(cam, raw)


def test_cpu_tensors_and_wrong_shapes_raise_before_any_launch():
    from eogs2_amd.pan import PanMap, pan_shade, render_pipeline

    avg, eye = PanMap("average"), torch.eye(3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pan_shade(torch.rand(3, 4, 4), None, eye, None, avg, "cc_first")
    cam = types.SimpleNamespace(weird_pan_setup=False, use_cc=False, use_exposure=False, use_shadow=False, msi_to_pan=avg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_pipeline(cam, torch.rand(3, 4, 4))
    with pytest.raises(RuntimeError, match=r"must be \(3, H, W\)"):
        pan_shade(torch.rand(4, 4), None, eye, None, avg, "cc_first")
    with pytest.raises(RuntimeError, match=r"must be \(3, H, W\)"):
        pan_shade(torch.rand(1, 4, 4), None, eye, None, avg, "cc_first")
    with pytest.raises(ValueError, match="unknown order"):
        pan_shade(torch.rand(3, 4, 4), None, eye, None, avg, "sideways")
    raw = torch.rand(3, 4, 5)
    with pytest.raises(RuntimeError, match=r"sun_altitude_diff must be \(4, 5\)"):
        pan_shade(raw, torch.zeros(5, 4), eye, torch.zeros(3), avg, "cc_first")
    with pytest.raises(RuntimeError, match="12 values"):
        pan_shade(raw, None, torch.tensor([1.0, 0.0]), None, avg, "cc_first")
    with pytest.raises(RuntimeError, match="2 values"):
        pan_shade(raw, None, eye, None, avg, "map_first")
    with pytest.raises(RuntimeError, match="inshadow must have 1 value"):
        pan_shade(raw, torch.zeros(4, 5), torch.tensor([1.0, 0.0]), torch.zeros(3), avg, "map_first")
    with pytest.raises(RuntimeError, match="inshadow must have 3 value"):
        pan_shade(raw, torch.zeros(4, 5), eye, None, avg, "cc_first")
