"""CPU: the public interface of the DSM raster (eogs2_amd.dsm_raster, include/eogs_dsm.h): the header, the binding table
and the built library agree, the size queries and argument checks answer without a device, and the Python wrappers refuse
what they cannot run (CPU tensors: there is no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
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
    return AC.header_text("eogs_dsm.h")


def test_header_and_binding_agree():
    from eogs2_amd import _abi

    names = sorted(set(re.findall(r"\b(eogs_dsm_[a-z_0-9]+)\s*\(", header())))
    assert names == sorted(_abi.HEADERS["eogs_dsm.h"]) and len(names) == 4
    assert set(names) <= set(_abi.HIP_ONLY)
    assert not set(names) & AC.elsewhere("eogs_dsm.h")  # under this header alone
    for name, (res, args) in _abi.HEADERS["eogs_dsm.h"].items():
        assert res is ctypes.c_int, name  # every entry returns a status
    assert any(n.endswith("_bytes") for n in names)
    defines = dict(re.findall(r"#define\s+(EOGS_DSM_[A-Z_]+)\s+(\(?[-0-9./ ]+\)?)", header()))
    assert eval(defines["EOGS_DSM_Z_QUANTUM"]) == _abi.DSM_Z_QUANTUM <= 2.0 ** -20
    assert float(defines["EOGS_DSM_Z_MAX"]) == _abi.DSM_Z_MAX >= 32768
    assert int(defines["EOGS_DSM_MAX_RADIUS"]) == _abi.DSM_MAX_RADIUS >= 2
    assert [int(defines[f"EOGS_DSM_SRC_{k}"]) for k in ("CLOUD", "VIEW", "GRID")] == [_abi.DSM_SRC_CLOUD, _abi.DSM_SRC_VIEW, _abi.DSM_SRC_GRID]
    assert ctypes.sizeof(_abi.DsmSource) == 96 and ctypes.sizeof(_abi.DsmBounds) == 48
    assert _abi.DsmSource.N.offset == 16 and _abi.DsmSource.scale.offset == 64  # the C layout on LP64


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS

    for n in HEADERS["eogs_dsm.h"]:
        assert hasattr(hip_lib.cdll, n), n
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only
    assert hip_lib.dsm_raster is not None and hip_lib.dsm_bounds_bytes is not None  # the short names resolve


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import dsm_raster as D
    from eogs2_amd.tsdf import TSDFVolume

    assert eogs2_amd.dsm_raster is D
    for n in ("cloud_bounds", "raster_geometry", "plyflatten", "dsm_from_view", "dsm_from_surface", "make_profile", "clear_workspaces"):
        assert callable(getattr(D, n)), n
    assert callable(TSDFVolume.extract_dsm) and callable(TSDFVolume.surface_cloud)
    assert D.Z_QUANTUM <= 2.0 ** -20 and D.Z_MAX >= 32768 and D.MAX_RADIUS >= 2


def test_size_queries_and_argument_checks_need_no_device(hip_lib):
    from eogs2_amd._abi import DsmSource

    n = ctypes.c_size_t()
    hip_lib.check(hip_lib.dsm_bounds_bytes(ctypes.byref(n)))
    assert 0 < n.value < (1 << 20)
    assert hip_lib.dsm_bounds_bytes(None) == -1
    hip_lib.check(hip_lib.dsm_raster_bytes(37, 23, 1, ctypes.byref(n)))
    assert 39 * 25 * 12 <= n.value <= 39 * 25 * 12 + 2048  # an int64 sum and a uint32 count per cell of the padded grid
    hip_lib.check(hip_lib.dsm_raster_bytes(4096, 4096, 2, ctypes.byref(n)))
    assert 4100 * 4100 * 12 <= n.value <= 4100 * 4100 * 12 + 2048
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, -1), (5, 5, 5), (-3, 5, 1), (50000, 50000, 1)):
        assert hip_lib.dsm_raster_bytes(*bad, ctypes.byref(n)) == -1, bad
    assert b"dsm_raster_bytes" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.dsm_raster_bytes(5, 5, 1, None) == -1
    # NULL and malformed arguments are rejected before anything touches a device
    cloud = DsmSource(kind=0, N=10)  # ten points, no pointer
    one = ctypes.c_void_p(256)
    assert hip_lib.dsm_raster(None, 0.0, 0.0, 0.5, 4, 4, 1, one, None, None, one, 1 << 20, None) == -1
    assert hip_lib.dsm_raster(ctypes.byref(cloud), 0.0, 0.0, 0.5, 4, 4, 1, one, None, None, one, 1 << 20, None) == -1
    assert b"NULL cloud" in hip_lib.cdll.eogs_rast_last_error()
    empty = DsmSource(kind=0, N=0)
    for xoff, yoff, res, xs, ys, r in ((0.0, 0.0, 0.0, 4, 4, 1), (0.0, 0.0, -0.5, 4, 4, 1), (0.0, 0.0, float("nan"), 4, 4, 1),
                                       (float("inf"), 0.0, 0.5, 4, 4, 1), (0.0, float("nan"), 0.5, 4, 4, 1), (0.0, 0.0, 0.5, 0, 4, 1),
                                       (0.0, 0.0, 0.5, 4, 4, 9)):
        assert hip_lib.dsm_raster(ctypes.byref(empty), xoff, yoff, res, xs, ys, r, one, None, None, one, 1 << 20, None) == -1
    assert hip_lib.dsm_raster(ctypes.byref(empty), 0.0, 0.0, 0.5, 4, 4, 1, None, None, None, one, 1 << 20, None) == -1
    assert hip_lib.dsm_raster(ctypes.byref(empty), 0.0, 0.0, 0.5, 4, 4, 1, one, None, None, one, 16, None) == -3  # workspace
    assert hip_lib.dsm_bounds(ctypes.byref(cloud), one, one, 1 << 20, None) == -1
    assert hip_lib.dsm_bounds(ctypes.byref(empty), None, one, 1 << 20, None) == -1
    assert hip_lib.dsm_bounds(ctypes.byref(empty), one, one, 16, None) == -3
    assert hip_lib.dsm_bounds(ctypes.byref(DsmSource(kind=7)), one, one, 1 << 20, None) == -1
    assert hip_lib.dsm_bounds(ctypes.byref(DsmSource(kind=1, H=4, W=4)), one, one, 1 << 20, None) == -1  # no image


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import dsm_raster as D
    from eogs2_amd.tsdf import TSDFVolume

    cloud = torch.zeros(10, 3, dtype=torch.float64)
    alt = torch.zeros(8, 9)
    sp = [np.array([5e5, 4.3e6, 30.0]), 10.0, 17, "T"]
    cam = (torch.eye(3), torch.zeros(3))
    for call in (lambda: D.cloud_bounds(cloud), lambda: D.plyflatten(cloud, 0.0, 0.0, 0.5, 4, 4),
                 lambda: D.dsm_from_view(alt, cam, sp, 0.5), lambda: D.dsm_from_view(alt, cam, sp, 0.5, geometry=(0.0, 0.0, 4, 4)),
                 lambda: D.dsm_from_surface(alt, torch.zeros(8), torch.zeros(9), sp, 0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        D.plyflatten(cloud.numpy(), 0.0, 0.0, 0.5, 4, 4)
    for radius in (-1, D.MAX_RADIUS + 1, 1.5, True):
        with pytest.raises(ValueError, match="radius"):
            D.plyflatten(cloud, 0.0, 0.0, 0.5, 4, 4, radius=radius)
    for sigma in (1.0, 0.0, 100.0, -float("inf")):
        with pytest.raises(NotImplementedError, match="sigma"):
            D.plyflatten(cloud, 0.0, 0.0, 0.5, 4, 4, sigma=sigma)
    for xs, ys in ((0, 4), (4, 0), (-1, 4), (4.5, 4)):
        with pytest.raises(ValueError, match="xsize"):
            D.plyflatten(cloud, 0.0, 0.0, 0.5, xs, ys)
    for res in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="resolution"):
            D.plyflatten(cloud, 0.0, 0.0, res, 4, 4)
    with pytest.raises(ValueError, match="finite"):
        D.plyflatten(cloud, float("nan"), 0.0, 0.5, 4, 4)
    assert callable(TSDFVolume.extract_dsm)


def test_raster_geometry_is_host_float64():
    """The reference's four lines (utils/dsm_utils.py:20-25) on numbers chosen so that a reciprocal multiply would differ."""
    from eogs2_amd.dsm_raster import make_profile, raster_geometry

    xmin, xmax, ymin, ymax, res = 500000.3, 500011.09999, 4300000.0, 4300006.9, 0.3
    xoff, yoff, xsize, ysize = raster_geometry(xmin, xmax, ymin, ymax, res)
    assert xoff == np.floor(xmin / res) * res and yoff == np.ceil(ymax / res) * res
    assert xsize == int(1 + np.floor((xmax - xoff) / res)) and ysize == int(1 - np.floor((ymin - yoff) / res))
    assert isinstance(xoff, np.float64) and isinstance(xsize, int)
    p = make_profile(torch.zeros(ysize, xsize, 1), xoff, yoff, res)
    assert p == {"dtype": "float32", "height": ysize, "width": xsize, "count": 1, "nodata": p["nodata"],
                 "transform": (res, 0.0, float(xoff), 0.0, -res, float(yoff))} and p["nodata"] != p["nodata"]
