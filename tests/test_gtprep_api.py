"""CPU: the public interface of ground-truth preparation (eogs2_amd.pansharp, eogs2_amd.rescaler, include/eogs_gtprep.h):
the header, the binding table and the built library agree; the entries and the Python wrappers refuse bad arguments before
any device call (CPU tensors: there is no CPU fallback)."""
import ctypes
import os
import re
import types

import pytest
import torch

import abi_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def header():
    return AC.header_text("eogs_gtprep.h")


def test_header_and_binding_agree():
    from eogs2_amd import _abi

    names = sorted(set(re.findall(r"\b(eogs_gtprep_[a-z_0-9]+)\s*\(", header())))
    assert names == sorted(_abi.HEADERS["eogs_gtprep.h"]) and len(names) == 12
    assert set(names) <= set(_abi.HIP_ONLY)
    assert not set(names) & AC.elsewhere("eogs_gtprep.h")  # under this header alone
    for name, (res, args) in _abi.HEADERS["eogs_gtprep.h"].items():
        assert res is ctypes.c_int, name  # every entry returns a status
        decl = re.search(name + r"\s*\(([^)]*)\)", header()).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(args), name
        for p, a in zip(params, args):  # the C type of every parameter against its ctypes type
            want = (ctypes.c_void_p if "*" in p and "size_t*" not in p else ctypes.POINTER(ctypes.c_size_t) if "size_t*" in p else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_size_t if p.startswith("size_t") else
                    ctypes.c_float if p.startswith("float") else ctypes.c_int)
            assert a is want, (name, p)
        if name != "eogs_gtprep_bytes":
            assert args[-1] is ctypes.c_void_p and "void* stream" in decl  # the stream is passed in
    defines = dict(re.findall(r"#define\s+(EOGS_GTPREP_[A-Z_]+)\s+(\d+)", header()))
    assert (int(defines["EOGS_GTPREP_BROVEY"]), int(defines["EOGS_GTPREP_SIMPLE_BROVEY"]), int(defines["EOGS_GTPREP_IHS"])) == \
        (_abi.GTPREP_BROVEY, _abi.GTPREP_SIMPLE_BROVEY, _abi.GTPREP_IHS)
    assert int(defines["EOGS_GTPREP_MAX_CHANNELS"]) == _abi.GTPREP_MAX_CHANNELS == 8
    assert _abi.ABI_VERSION == 8  # additions only


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS

    for n in HEADERS["eogs_gtprep.h"]:
        assert hasattr(hip_lib.cdll, n), n
    assert hip_lib.cdll.eogs_rast_abi_version() == 8
    assert hip_lib.gtprep_pansharp is not None and hip_lib.gtprep_equalize is not None  # the short names resolve
    n = ctypes.c_size_t()
    assert hip_lib.gtprep_bytes(3, ctypes.byref(n)) == 0 and n.value >= 1024 * 2 * 8
    big = ctypes.c_size_t()
    assert hip_lib.gtprep_bytes(64, ctypes.byref(big)) == 0 and big.value >= 64 * 2048 and big.value > n.value


def test_package_exports_the_modules():
    import eogs2_amd
    from eogs2_amd import pansharp as P, rescaler as R

    assert eogs2_amd.pansharp is P and eogs2_amd.rescaler is R
    for name in ("brovey_pansharp", "simple_brovey", "ihs_fusion", "load_pansharp", "pan_l2", "pan_gradient_l2", "pansharp_l2", "Lpan",
                 "Lgradient_pan", "Pansharploss"):
        assert callable(getattr(P, name)) and name in P.__all__
    for name in ("clamper", "standard_rescaler", "rescale_wrt_firstimage", "histogram_equalizer", "identity_rescaler", "CLAHE_rescaler",
                 "load_rescaler", "perform_rescaling_listcam", "perform_rescaling"):
        assert callable(getattr(R, name)) and name in R.__all__


def test_entries_check_their_arguments_without_a_device(hip_lib):
    one, two, three = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(1024)
    err = lambda: hip_lib.cdll.eogs_rast_last_error()  # noqa: E731
    L = hip_lib
    assert L.gtprep_bytes(0, ctypes.byref(ctypes.c_size_t())) == -1 and L.gtprep_bytes(3, None) == -1
    assert L.gtprep_pansharp(3, 3, 2, 2, 4, 4, one, two, 0.1, three, None) == -1 and b"unknown method" in err()
    assert L.gtprep_pansharp(0, 9, 2, 2, 4, 4, one, two, 0.1, three, None) == -1 and b"1 to 8" in err()
    assert L.gtprep_pansharp(0, 0, 2, 2, 4, 4, one, two, 0.1, three, None) == -1
    assert L.gtprep_pansharp(2, 4, 2, 2, 4, 4, one, two, 0.1, three, None) == -1 and b"3 MSI channels" in err()
    assert L.gtprep_pansharp(0, 3, 0, 2, 4, 4, one, two, 0.1, three, None) == -1 and b"bad sizes" in err()
    assert L.gtprep_pansharp(0, 3, 2, 2, 4, -1, one, two, 0.1, three, None) == -1
    assert L.gtprep_pansharp(0, 3, 2, 2, 4, 4, None, two, 0.1, three, None) == -1 and b"NULL" in err()
    assert L.gtprep_pansharp(0, 3, 2, 2, 4, 4, one, two, 0.1, None, None) == -1
    assert L.gtprep_pansharp_l2_forward(0, 3, 2, 2, 4, 4, one, two, three, 0.1, one, two, 16, None) == -3 and b"workspace" in err()
    assert L.gtprep_pansharp_l2_forward(0, 3, 2, 2, 4, 4, None, two, three, 0.1, one, two, 1 << 20, None) == -1
    assert L.gtprep_pansharp_l2_forward(1, 9, 2, 2, 4, 4, one, two, three, 0.1, one, two, 1 << 20, None) == -1
    assert L.gtprep_pansharp_l2_backward(0, 3, 2, 2, 4, 4, one, two, three, 0.1, None, None, None) == -1
    assert L.gtprep_pansharp_l2_backward(5, 3, 2, 2, 4, 4, one, two, three, 0.1, None, one, None) == -1
    assert L.gtprep_l2_forward(0, one, two, three, one, 1 << 20, None) == -1 and b"bad size" in err()
    assert L.gtprep_l2_forward(10, one, None, three, one, 1 << 20, None) == -1
    assert L.gtprep_l2_forward(10, one, two, three, one, 8, None) == -3
    assert L.gtprep_l2_backward(10, one, two, None, None, None) == -1
    assert L.gtprep_l2_backward(-1, one, two, None, three, None) == -1
    assert L.gtprep_grad_l2_forward(1, 1, 5, one, two, three, one, 1 << 20, None) == -1 and b"at least 2" in err()
    assert L.gtprep_grad_l2_forward(1, 5, 1, one, two, three, one, 1 << 20, None) == -1
    assert L.gtprep_grad_l2_forward(0, 5, 5, one, two, three, one, 1 << 20, None) == -1
    assert L.gtprep_grad_l2_forward(1, 5, 5, one, two, three, one, 8, None) == -3
    assert L.gtprep_grad_l2_backward(1, 5, 1, one, two, None, three, None) == -1 and b"at least 2" in err()
    assert L.gtprep_grad_l2_backward(1, 5, 5, one, two, None, None, None) == -1
    assert L.gtprep_minmax(0, 10, one, two, three, 1 << 20, None) == -1
    assert L.gtprep_minmax(3, 0, one, two, three, 1 << 20, None) == -1
    assert L.gtprep_minmax(3, 10, one, two, three, 8, None) == -3
    assert L.gtprep_minmax(3, 10, one, None, three, 1 << 20, None) == -1
    assert L.gtprep_rescale(3, 10, one, None, three, None) == -1
    assert L.gtprep_rescale(3, 0, one, two, three, None) == -1
    assert L.gtprep_clamp(0, one, 0.0, 1.0, two, None) == -1
    assert L.gtprep_clamp(10, one, float("nan"), 1.0, two, None) == -1 and b"numbers" in err()
    assert L.gtprep_clamp(10, None, 0.0, 1.0, two, None) == -1
    assert L.gtprep_equalize(3, 1 << 31, one, two, three, 1 << 20, None) == -1 and b"2^31" in err()
    assert L.gtprep_equalize(3, 10, one, one, three, 1 << 20, None) == -1 and b"of its own" in err()
    assert L.gtprep_equalize(3, 10, one, two, three, 8, None) == -3
    assert L.gtprep_equalize(3, 10, one, two, None, 1 << 20, None) == -1


def test_pansharp_refuses_bad_arguments():
    from eogs2_amd import pansharp as P

    pan, msi = torch.rand(8, 8), torch.rand(3, 2, 2)
    for call in (lambda: P.brovey_pansharp(pan, msi), lambda: P.brovey_pansharp(pan[None], msi), lambda: P.brovey_pansharp(pan[:, :, None], msi),
                 lambda: P.simple_brovey(pan, msi[None]), lambda: P.ihs_fusion(pan[None], msi)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="at most 8"):  # C > 8
        P.brovey_pansharp(pan, torch.rand(9, 2, 2))
    with pytest.raises(ValueError, match=r"\(1, C, h, w\)"):
        P.simple_brovey(pan, msi)
    with pytest.raises(ValueError):
        P.brovey_pansharp(torch.rand(2, 8, 8), msi)
    with pytest.raises(ValueError):
        P.brovey_pansharp(pan, torch.rand(2, 2))
    with pytest.raises(ValueError):
        P.brovey_pansharp(torch.rand(0, 8), msi)
    with pytest.raises(AssertionError):  # the reference's two assertions
        P.ihs_fusion(pan, msi)
    with pytest.raises(AssertionError):
        P.ihs_fusion(pan[None], torch.rand(4, 2, 2))
    with pytest.raises(TypeError, match="float32"):
        P.brovey_pansharp(pan.double(), msi)
    with pytest.raises(TypeError):
        P.brovey_pansharp(pan.numpy(), msi)


def test_load_pansharp_follows_the_reference():
    from eogs2_amd import pansharp as P

    cfg = lambda m: types.SimpleNamespace(method=m)  # noqa: E731
    assert P.load_pansharp(cfg("brovey")) is P.brovey_pansharp and P.load_pansharp("brovey") is P.brovey_pansharp
    assert P.load_pansharp(cfg("simple_brovey")) is P.simple_brovey and P.load_pansharp(cfg("ihs")) is P.ihs_fusion
    assert P.load_pansharp(cfg("nopansharp")) is None and P.load_pansharp("nopansharp") is None
    with pytest.raises(ValueError, match="Unsupported pansharpening method: gram_schmidt"):
        P.load_pansharp(cfg("gram_schmidt"))
    with pytest.raises(ValueError, match="nopansharp"):  # at construction, not on the first step
        P.Pansharploss(0.1, cfg("nopansharp"))
    with pytest.raises(ValueError, match="Unsupported"):
        P.Pansharploss(0.1, cfg("pca"))
    loss = P.Pansharploss(0.25, cfg("brovey"))
    assert loss.lambda_L_pansharp == 0.25 and loss.pansharp_method is P.brovey_pansharp and loss.get_loss_name() == "Pansharploss"
    assert P.Lpan(0.5).lambda_Lpan == 0.5 and P.Lgradient_pan(0.125).lambda_lgradient_pan == 0.125


def test_losses_refuse_bad_arguments():
    from eogs2_amd import pansharp as P

    a, b = torch.rand(1, 6, 7, requires_grad=True), torch.rand(1, 6, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.Lpan(1.0)(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.Lgradient_pan(1.0)(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.Pansharploss(1.0, "brovey")(torch.rand(3, 8, 8), torch.rand(8, 8), torch.rand(3, 2, 2))
    for shape in ((1, 6), (6, 1), (3, 1, 5), (5,)):  # an axis shorter than 2: torch.gradient's error, as a ValueError, before any launch
        with pytest.raises(ValueError, match="at least 2"):
            P.pan_gradient_l2(torch.rand(shape), torch.rand(shape))
    with pytest.raises(ValueError, match="shape of the pansharpened image"):
        P.pansharp_l2(torch.rand(3, 8, 7), torch.rand(8, 8), torch.rand(3, 2, 2))
    with pytest.raises(ValueError, match="Unsupported"):
        P.pansharp_l2(torch.rand(3, 8, 8), torch.rand(8, 8), torch.rand(3, 2, 2), method="nopansharp")
    with pytest.raises(ValueError, match="at most 8"):
        P.pansharp_l2(torch.rand(9, 8, 8), torch.rand(8, 8), torch.rand(9, 2, 2))
    with pytest.raises(TypeError, match="float32"):
        P.pan_l2(a.double(), b)
    with pytest.raises(ValueError, match="empty"):
        P.pan_l2(torch.rand(0, 3), torch.rand(0, 3))


def test_rescalers_refuse_bad_arguments():
    from eogs2_amd import rescaler as R

    x = torch.rand(3, 5, 7)
    for name in ("clamper", "standard_rescaler", "histogram_equalizer"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            R.load_rescaler(name).forward(x)
    cams = [types.SimpleNamespace(is_reference_camera=k == 1, original_image=x) for k in range(2)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.load_rescaler("rescale_wrt_firstimage").setup(cams)
    with pytest.raises(AssertionError, match="reference camera"):
        R.rescale_wrt_firstimage().setup([types.SimpleNamespace(is_reference_camera=False, original_image=x)])
    with pytest.raises(AssertionError, match="setup"):
        R.rescale_wrt_firstimage().forward(x)
    with pytest.raises(ValueError, match="Unknown rescaler name: gamma"):
        R.load_rescaler("gamma")
    with pytest.raises(NotImplementedError, match="kornia"):
        R.load_rescaler("CLAHE_rescaler")
    with pytest.raises(NotImplementedError):
        R.CLAHE_rescaler()
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):
        R.standard_rescaler().forward(torch.rand(5, 7))
    with pytest.raises(TypeError, match="float32"):
        R.standard_rescaler().forward(x.double())
    assert R.load_rescaler("identity").forward(x) is x and isinstance(R.load_rescaler("clamper"), R.clamper)
    c = R.clamper(0.25, 0.5)
    assert (c.min_val, c.max_val) == (0.25, 0.5) and R.base_rescaler().setup([]) is not None
