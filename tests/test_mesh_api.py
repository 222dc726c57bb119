"""CPU: the public interface of the mesh extraction (eogs2_amd.mesh, include/eogs_mesh.h): the header, the binding table
and the built library agree, the size query and the argument checks answer without a device, the Python wrappers refuse
what they cannot run (CPU tensors: there is no CPU fallback) and export_obj writes a file that reads back to the same mesh."""
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
    return AC.header_text("eogs_mesh.h")


def test_header_and_binding_agree():
    from eogs2_amd import _abi

    names = sorted(set(re.findall(r"\b(eogs_mesh_[a-z_0-9]+)\s*\(", header())))
    assert names == sorted(_abi.HEADERS["eogs_mesh.h"]) and len(names) == 4
    assert set(names) <= set(_abi.HIP_ONLY)
    assert not set(names) & AC.elsewhere("eogs_mesh.h")  # under this header alone
    for name, (res, args) in _abi.HEADERS["eogs_mesh.h"].items():
        assert res is ctypes.c_int, name  # every entry returns a status
    # the argument counts of the declarations
    for name, (_, args) in _abi.HEADERS["eogs_mesh.h"].items():
        decl = re.search(name + r"\s*\(([^)]*)\)", header()).group(1)
        assert len(decl.split(",")) == len(args), name
    defines = dict(re.findall(r"#define\s+(EOGS_MESH_[A-Z_]+)\s+(\S+)", header()))
    assert "#define EOGS_MESH_MAX_VERTICES (1u << 29)" in header() and _abi.MESH_MAX_VERTICES == 1 << 29
    assert int(defines["EOGS_MESH_WG_VOXELS"]) == _abi.MESH_WG_VOXELS and int(defines["EOGS_MESH_SCAN_ROUND"]) == _abi.MESH_SCAN_ROUND


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS

    for n in HEADERS["eogs_mesh.h"]:
        assert hasattr(hip_lib.cdll, n), n
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only
    assert hip_lib.mesh_count is not None and hip_lib.mesh_bytes is not None  # the short names resolve


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import mesh as M
    from eogs2_amd.tsdf import TSDFVolume

    assert eogs2_amd.mesh is M
    assert callable(M.marching_cubes) and callable(M.export_obj) and callable(TSDFVolume.extract_mesh)
    assert M.MAX_VERTICES == 1 << 29


def test_size_query_and_argument_checks_need_no_device(hip_lib):
    from eogs2_amd._abi import MESH_WG_VOXELS

    n = ctypes.c_size_t()
    for dims in ((5, 6, 7), (512, 512, 192), (1, 1, 1)):
        hip_lib.check(hip_lib.mesh_bytes(*dims, ctypes.byref(n)))
        voxels = dims[0] * dims[1] * dims[2]
        groups = -(-voxels // MESH_WG_VOXELS)
        chunks = -(-groups // 256)  # a word per voxel, three per workgroup, six per chunk of 256 workgroups
        assert 4 * voxels + 12 * groups + 24 * chunks <= n.value <= 4 * voxels + 12 * groups + 24 * chunks + 2048
    for bad in ((0, 5, 5), (5, -1, 5), (5, 5, 0), (2048, 2048, 512), (65536, 65536, 1), (1 << 30, 2, 1)):
        assert hip_lib.mesh_bytes(*bad, ctypes.byref(n)) == -1, bad
    assert b"mesh_bytes" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.mesh_bytes(5, 5, 5, None) == -1
    one = ctypes.c_void_p(256)
    # NULL and malformed arguments are rejected before anything touches a device
    assert hip_lib.mesh_count(5, 5, 5, None, 0.0, one, 1 << 20, one, None) == -1
    assert hip_lib.mesh_count(5, 5, 5, one, 0.0, None, 1 << 20, one, None) == -1
    assert hip_lib.mesh_count(5, 5, 5, one, 0.0, one, 1 << 20, None, None) == -1
    assert hip_lib.mesh_count(5, 5, 5, one, float("nan"), one, 1 << 20, one, None) == -1
    assert hip_lib.mesh_count(0, 5, 5, one, 0.0, one, 1 << 20, one, None) == -1
    assert hip_lib.mesh_count(2048, 2048, 512, one, 0.0, one, 1 << 20, one, None) == -1
    assert b"2^31" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.mesh_count(5, 5, 5, one, 0.0, one, 16, one, None) == -3  # workspace
    emit = lambda *a: hip_lib.mesh_emit(*a, None)  # noqa: E731
    assert emit(5, 5, 5, None, 0.0, None, None, None, None, one, 1 << 20, one, 3, one, 1) == -1
    assert emit(5, 5, 5, one, 0.0, one, None, None, None, one, 1 << 20, one, 3, one, 1) == -1  # one axis of three
    assert b"axes" in hip_lib.cdll.eogs_rast_last_error()
    assert emit(5, 5, 5, one, 0.0, None, None, None, None, one, 1 << 20, None, 3, one, 1) == -1  # vertices wanted, no array
    assert emit(5, 5, 5, one, 0.0, None, None, None, None, one, 1 << 20, one, 3, None, 1) == -1
    assert emit(5, 5, 5, one, 0.0, None, None, None, None, one, 1 << 20, one, -1, one, 1) == -1
    assert emit(5, 5, 5, one, 0.0, None, None, None, None, one, 1 << 20, one, 1 << 29, one, 1) == -5  # the vertex limit
    assert b"2^29" in hip_lib.cdll.eogs_rast_last_error()
    assert emit(5, 5, 5, one, 0.0, None, None, None, None, one, 16, one, 3, one, 1) == -3
    # the table accessor is host code
    row, k = (ctypes.c_int8 * 15)(), ctypes.c_int(-1)
    hip_lib.check(hip_lib.mesh_case(0, row, ctypes.byref(k)))
    assert k.value == 0 and list(row) == [-1] * 15
    hip_lib.check(hip_lib.mesh_case(1, row, ctypes.byref(k)))
    assert k.value == 1 and sorted(row[:3]) == [0, 4, 8] and list(row[3:]) == [-1] * 12  # corner 0: its x, y and z edge
    assert hip_lib.mesh_case(256, row, ctypes.byref(k)) == -1 and hip_lib.mesh_case(-1, row, ctypes.byref(k)) == -1
    assert hip_lib.mesh_case(3, None, ctypes.byref(k)) == -1


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import mesh as M
    from eogs2_amd.tsdf import TSDFVolume

    vol = torch.ones(4, 5, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.marching_cubes(vol)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.marching_cubes(vol, 0.25, axes=[torch.zeros(4), torch.zeros(5), torch.zeros(6)], shift=(1.0, 2.0, 3.0))
    with pytest.raises(TypeError):
        M.marching_cubes(vol.numpy())
    tv = TSDFVolume(np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 0.5]]), 0.1, 2.0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tv.extract_mesh()
    with pytest.raises(ValueError, match="coords"):
        tv.extract_mesh(coords="utm")


def parse_obj(path):
    v, f = [], []
    for line in open(path):
        p = line.split()
        if p and p[0] == "v":
            v.append([float(x) for x in p[1:]])
        elif p and p[0] == "f":
            f.append([int(x) - 1 for x in p[1:]])
    return np.array(v, dtype=np.float64).reshape(-1, 3), np.array(f, dtype=np.int64).reshape(-1, 3)


def test_export_obj_round_trips(tmp_path):
    from eogs2_amd.mesh import export_obj

    g = np.random.default_rng(0)
    v = np.concatenate([g.standard_normal((50, 3)) * 1e-3, g.random((50, 3)) + [512345.25, 4321987.75, 31.5], [[0.1, 1 / 3, -2.5e-300]]])
    f = g.integers(0, len(v), (70, 3)).astype(np.int32)
    p = tmp_path / "mesh.obj"
    export_obj(torch.as_tensor(v), torch.as_tensor(f), p)
    lines = open(p).read().splitlines()
    assert len(lines) == len(v) + len(f) and lines[0].startswith("v ") and lines[-1].startswith("f ")
    v2, f2 = parse_obj(p)
    assert v2.tobytes() == v.tobytes() and np.array_equal(f2, f)  # coordinates round-trip, indices are 1-based in the file
    assert min(int(x) for line in lines[len(v):] for x in line.split()[1:]) >= 1
    export_obj(torch.zeros((0, 3), dtype=torch.float64), torch.zeros((0, 3), dtype=torch.int32), p)
    assert open(p).read() == ""
    with pytest.raises(ValueError, match="vertex"):
        export_obj(torch.zeros((2, 3), dtype=torch.float64), torch.tensor([[0, 1, 2]], dtype=torch.int32), p)
