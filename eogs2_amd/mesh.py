"""Mesh extraction on the GPU over include/eogs_mesh.h: marching cubes over a TSDF volume, the last stage of the reference's
post-processing chain. The reference copies the volume to the host and hands it to the third-party `mcubes`
(tsdf.py:522-528, :719-723); here the volume stays on the device:

  marching_cubes(volume, iso=0.0, *, axes=None, shift=None)   -> (vertices f64 [NV, 3], triangles i32 [NT, 3]) on the device
  export_obj(vertices, triangles, path)                       mcubes.export_obj's file: `v x y z` / `f a b c`, 1-based
  TSDFVolume.extract_mesh(output_mesh_path=None, ...)         eogs2_amd.tsdf: the reference's method, mcubes-free

GPU tensors only; CPU tensors raise (no CPU fallback). The semantics are stated in include/eogs_mesh.h and DESIGN.md §8: a
voxel is inside when value < iso, one vertex per grid edge whose ends differ, at i + t (index coordinates, what mcubes
returns) or ax[i] + t (ax[i+1] - ax[i]) (world coordinates, `axes`), t = (iso - va) / (vb - va) in double, `shift` added
in double; vertices ordered by owning voxel (z fastest) then axis, triangles by cell then table order; the same bits on
every run. Deviations from mcubes: that ordering, the face rule on ambiguous cells, and a ValueError for a volume with
non-finite voxels (mcubes hands back NaN vertices).

Two phases with one host wait between them, for the sizes (four integers), as `density.densify_and_prune` has.
"""
import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._abi import MESH_MAX_VERTICES
from ._host import Ctx, on_device, ptr, query_bytes

MAX_VERTICES = MESH_MAX_VERTICES  # include/eogs_mesh.h EOGS_MESH_MAX_VERTICES


_on_device = functools.partial(on_device, "mesh", "the mesh extraction runs", non_tensor="not")


def _shift3(shift):
    c = np.asarray(shift.detach().cpu() if torch.is_tensor(shift) else shift, dtype=np.float64).reshape(-1)
    if c.shape != (3,):
        raise ValueError("mesh marching_cubes: shift is three numbers (scene_params[0])")
    return (ctypes.c_double * 3)(*c.tolist())


def marching_cubes(volume, iso=0.0, *, axes=None, shift=None):
    """(vertices float64 [NV, 3], triangles int32 [NT, 3]) of a float32 [nx, ny, nz] volume at level `iso`, on the volume's
    device. `axes` = (ax [nx], ay [ny], az [nz]) gives world coordinates from the fp32 axes, None index coordinates;
    `shift` (three numbers) is added in double. An empty surface returns two empty tensors. ValueError for non-finite
    voxels; a non-contiguous volume is copied, a dtype other than float32 raises TypeError."""
    _on_device(volume, "marching_cubes")
    if volume.dtype != torch.float32 or volume.ndim != 3 or volume.numel() == 0:
        raise TypeError(f"mesh marching_cubes: the volume is a non-empty float32 [nx, ny, nz], not {volume.dtype} {tuple(volume.shape)}")
    iso = float(iso)
    if iso != iso:
        raise ValueError("mesh marching_cubes: iso is NaN")
    vol = volume.detach().contiguous()
    dev = vol.device
    nx, ny, nz = vol.shape
    if nx * ny * nz >= 1 << 31:
        raise ValueError("mesh marching_cubes: the volume must hold fewer than 2^31 voxels")
    ax = ay = az = None
    if axes is not None:
        ax, ay, az = (a.detach().to(device=dev, dtype=torch.float32).contiguous() for a in axes)
        if (ax.numel(), ay.numel(), az.numel()) != (nx, ny, nz):
            raise ValueError("mesh marching_cubes: the axes do not match the volume")
    sh = None if shift is None else _shift3(shift)
    abi = _lib.get()
    ws = torch.empty(query_bytes(abi, "mesh_bytes", nx, ny, nz), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    with Ctx(abi, dev) as cx:
        abi.check(abi.mesh_count(nx, ny, nz, ptr(vol), iso, ptr(ws), ws.numel(), ptr(counts), cx.stream))
        nv, nt, bad, _ = (int(c) for c in counts.cpu().numpy().view(np.uint32))  # the one wait
        if bad:
            raise ValueError(f"mesh marching_cubes: {bad} of {nx * ny * nz} voxels are not finite")
        if nv >= MAX_VERTICES:
            raise ValueError(f"mesh marching_cubes: {nv} vertices or more, the limit is 2^29 - 1")
        vertices = torch.empty((nv, 3), dtype=torch.float64, device=dev)
        triangles = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        if nv:
            abi.check(abi.mesh_emit(nx, ny, nz, ptr(vol), iso, ptr(ax), ptr(ay), ptr(az), sh, ptr(ws), ws.numel(),
                                    ptr(vertices), nv, ptr(triangles), nt, cx.stream))
    return vertices, triangles


def export_obj(vertices, triangles, path):
    """mcubes.export_obj's file: one `v x y z` line per vertex, one `f a b c` line per triangle with 1-based indices.
    Coordinates are printed with 17 significant digits: reading them back gives the same float64."""
    v = np.asarray(vertices.detach().cpu() if torch.is_tensor(vertices) else vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(triangles.detach().cpu() if torch.is_tensor(triangles) else triangles).reshape(-1, 3).astype(np.int64)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("mesh export_obj: a triangle names a vertex that is not there")
    with open(path, "w") as out:
        np.savetxt(out, v, fmt="v %.17g %.17g %.17g")
        np.savetxt(out, f + 1, fmt="f %d %d %d")


__all__ = ["MAX_VERTICES", "export_obj", "marching_cubes"]
