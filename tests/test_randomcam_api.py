"""CPU: the public interface of the random-camera loss (eogs2_amd.randomcam, include/eogs_randomcam.h): the header, the binding
table and the built library agree; the entries refuse bad arguments before a device is touched; the constructor keeps the
reference's assertion; every shape and device error of the Python layer is raised before any launch."""
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
    return AC.header_text("eogs_randomcam.h")


def test_header_and_binding_agree():
    from eogs2_amd import _abi

    names = sorted(set(re.findall(r"\b(eogs_[a-z_0-9]+)\s*\(", header())))
    assert names == sorted(_abi.HEADERS["eogs_randomcam.h"]) == ["eogs_cmloss_backward", "eogs_cmloss_bytes", "eogs_cmloss_forward",
                                                         "eogs_randomcam_compose"]
    assert set(names) <= set(_abi.HIP_ONLY)
    assert not set(names) & AC.elsewhere("eogs_randomcam.h")  # under this header alone
    for name, (res, args) in _abi.HEADERS["eogs_randomcam.h"].items():
        assert res is ctypes.c_int, name
        decl = re.search(name + r"\s*\(([^)]*)\)", header()).group(1)
        assert len(decl.split(",")) == len(args), name
        if name != "eogs_cmloss_bytes":
            assert args[-1] is ctypes.c_void_p and "void* stream" in decl
    defines = dict(re.findall(r"#define\s+(EOGS_CMLOSS_[A-Z_]+)\s+(\d+)", header()))
    assert int(defines["EOGS_CMLOSS_MAX_CHANNELS"]) == _abi.CMLOSS_MAX_CHANNELS == 4
    assert _abi.ABI_VERSION == 8  # additions only
    # the existing entries stay as they are
    shade = open(os.path.join(ROOT, "include", "eogs_shade.h")).read()
    assert "eogs_cmloss" not in shade and "eogs_randomcam" not in shade


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS

    for n in HEADERS["eogs_randomcam.h"]:
        assert hasattr(hip_lib.cdll, n), n
    assert hip_lib.cdll.eogs_rast_abi_version() == 8
    assert hip_lib.randomcam_compose is not None and hip_lib.cmloss_forward is not None  # the short names resolve


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import randomcam as R

    assert eogs2_amd.randomcam is R
    for name in ("RandomcamRendering_Loss", "render_resample_virtual_camera_wshadowmapping", "virtual_to_sun", "cmloss"):
        assert callable(getattr(R, name)) and name in R.__all__


def test_entries_check_their_arguments_without_a_device(hip_lib):
    err = lambda: hip_lib.cdll.eogs_rast_last_error()  # noqa: E731
    p = ctypes.c_void_p
    assert hip_lib.randomcam_compose(None, p(4096), p(8192), None) == -1 and b"cam2virt" in err()
    assert hip_lib.randomcam_compose(p(4096), None, p(8192), None) == -1 and b"camera_to_sun" in err()
    assert hip_lib.randomcam_compose(p(4096), p(4224), None, None) == -1 and b"out" in err()
    for bad in ((4098, 4224, 8192), (4096, 4225, 8192), (4096, 4224, 8194)):
        assert hip_lib.randomcam_compose(p(bad[0]), p(bad[1]), p(bad[2]), None) == -1 and b"aligned" in err()
    assert hip_lib.randomcam_compose(p(4096), p(4224), p(4096 + 32), None) == -1 and b"overlaps" in err()
    assert hip_lib.randomcam_compose(p(4096), p(4224), p(4224 - 68), None) == -1 and b"overlaps" in err()
    n = ctypes.c_size_t()
    assert hip_lib.cmloss_bytes(0, 4, ctypes.byref(n)) == -1 and hip_lib.cmloss_bytes(4, 4, None) == -1
    assert hip_lib.cmloss_bytes(4, 4, ctypes.byref(n)) == 0 and n.value > 0
    a = [p(1 << 20)] * 6
    assert hip_lib.cmloss_forward(0, 4, 3, *a, n.value, None) == -1 and b"sizes" in err()
    for C in (0, 5, -1):
        assert hip_lib.cmloss_forward(4, 4, C, *a, n.value, None) == -1 and b"channels" in err()
        assert hip_lib.cmloss_backward(4, 4, C, *([p(1 << 20)] * 9), None) == -1 and b"channels" in err()
    for i in range(6):
        args = list(a)
        args[i] = None
        assert hip_lib.cmloss_forward(4, 4, 3, *args, n.value, None) == -1 and b"NULL" in err(), i
    assert hip_lib.cmloss_forward(4, 4, 3, *a, n.value - 1, None) == -3 and b"workspace" in err()
    for i in range(7):  # alt_diff, rgb_a, rgb_b, uv, out, upstream, g_alt_diff; the two colour gradients may be NULL
        args = [p(1 << 20)] * 9
        args[i] = None
        assert hip_lib.cmloss_backward(4, 4, 3, *args, None) == -1 and b"NULL" in err(), i


def test_constructor_keeps_the_reference_assertion(capsys):
    from eogs2_amd.randomcam import RandomcamRendering_Loss

    for ok in ("rawrender", "rawrender_wshadow"):
        fn = RandomcamRendering_Loss(1e-4, 1e-3, ok)
        assert fn.render_type == ok and fn.use_gt is False and fn.weight == 0
        assert fn.w_L_randomcam_rendering == 1e-4 and fn.w_L_new_rgb_resample == 1e-3
        assert fn.get_loss_name() == "RandomcamRendering_Loss"
    with pytest.raises(AssertionError, match="render type not implemented,got shaded"):
        RandomcamRendering_Loss(1.0, 1.0, "shaded")
    capsys.readouterr()
    assert RandomcamRendering_Loss(1.0, 1.0, "rawrender", use_gt=True).use_gt is True
    assert "gt image for random camera loss" in capsys.readouterr().out
    for name in ("forward", "_forward", "log_loss", "_rawrender_from_camera", "_rawrender_from_camera_wshadow"):
        assert callable(getattr(RandomcamRendering_Loss, name))
    logged = []
    RandomcamRendering_Loss(1.0, 1.0, "rawrender").log_loss(types.SimpleNamespace(add_scalar=lambda *a: logged.append(a)), 1.0, 2.0, 7)
    assert logged == [("loss/L_new_altitude_resample", 1.0, 7), ("loss/L_new_rgb_resample", 2.0, 7)]


def test_virtual_to_sun_refuses_before_any_launch():
    from eogs2_amd.randomcam import virtual_to_sun

    I = torch.eye(3)
    with pytest.raises(TypeError, match="cam2virt must be a tensor"):
        virtual_to_sun(I.numpy(), I)
    with pytest.raises(ValueError, match=r"camera_to_sun must have shape \(3, 3\)"):
        virtual_to_sun(I, torch.eye(4))
    with pytest.raises(ValueError, match="cam2virt must be float32"):
        virtual_to_sun(I.double(), I)
    with pytest.raises(ValueError, match="out must be 18 contiguous float32"):
        virtual_to_sun(I, I, out=torch.zeros(9))
    with pytest.raises(ValueError, match="out must be 18 contiguous float32"):
        virtual_to_sun(I, I, out=torch.zeros(36)[::2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        virtual_to_sun(I, I)
    with pytest.raises(RuntimeError, match="camera_to_sun on cpu, cam2virt on meta"):
        from eogs2_amd.randomcam import check_compose

        check_compose(I.to("meta"), I)


def test_cmloss_refuses_before_any_launch():
    from eogs2_amd.randomcam import cmloss

    H, W = 5, 7
    d, uv = torch.zeros(H, W), torch.zeros(H, W, 2)
    rgb = lambda c: torch.zeros(c, H, W)  # noqa: E731
    with pytest.raises(ValueError, match=r"new_altitude_diff must be \(H, W\)"):
        cmloss(torch.zeros(1, H, W), rgb(3), rgb(3), uv)
    for c in (0, 5):
        with pytest.raises(ValueError, match="1 <= C <= 4"):
            cmloss(d, rgb(c), rgb(c), uv)
    with pytest.raises(ValueError, match="new_rgb_sample must be"):
        cmloss(d, rgb(3), rgb(1), uv)
    with pytest.raises(ValueError, match="rgb_render must be"):
        cmloss(d, torch.zeros(3, H, W + 1), rgb(3), uv)
    with pytest.raises(ValueError, match="new_uv must be"):
        cmloss(d, rgb(3), rgb(3), torch.zeros(H, W, 3))
    with pytest.raises(TypeError, match="new_uv must be a tensor"):
        cmloss(d, rgb(3), rgb(3), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cmloss(d, rgb(1), rgb(1), uv)
    with pytest.raises(RuntimeError, match="new_uv on cpu"):
        from eogs2_amd.randomcam import check_cmloss

        check_cmloss(d.to("meta"), rgb(3).to("meta"), rgb(3).to("meta"), uv)


def test_wshadowmapping_refuses_before_any_launch():
    from eogs2_amd.randomcam import RandomcamRendering_Loss, render_resample_virtual_camera_wshadowmapping as fn

    cam = types.SimpleNamespace(get_sun_camera=lambda: (None, torch.eye(3)))
    uva = torch.zeros(4, 6, 3)
    with pytest.raises(RuntimeError, match="rendered_uva on 'cpu'.*no CPU fallback"):
        fn(None, cam, torch.eye(3), uva, None, None, None)
    with pytest.raises(TypeError, match="rendered_uva must be a tensor"):
        fn(None, cam, torch.eye(3), None, None, None, None)
    with pytest.raises(ValueError, match="sun_render belongs to"):
        RandomcamRendering_Loss(1.0, 1.0, "rawrender").forward(None, cam, torch.eye(3), uva, None, None, None, None, None, None, None,
                                                               sun_render=torch.zeros(5, 8, 12))
