"""TSDF fusion over the C-ABI of include/eogs_tsdf.h (second piece).

`TSDFVolume(vol_bounds, vox_size, trunc_margin_fact)` has the reference's constructor arithmetic and attributes
(src/gaussiansplatting/tsdf.py:374-456: `num_voxels_per_dimension`, `axes`, `_tsdf_vol` = ones, `_weight_vol` = zeros)
and `integrate(rangeimage)` (:459-498) runs ONE HIP kernel per range image instead of the reference's ~25 voxel-sized
PyTorch temporaries. `rangeimage` is duck-typed like `RangeImageEOGS` (:186-368): `affine_model = (coef[3,3],
intercept[3])`, `model_scale`, `altitude_img [1,1,H,W]`, `get_weights() [1,1,H,W]`.

The stages around integrate are HIP as well:
  RangeImage (alias RangeImageEOGS)  the reference's RangeImageEOGS (:186-323): normals, view angle and weights of one
                                     altitude image in one kernel, without the 5x5 unfold of the world-position image
  TSDFVolume.apply_prior()           tsdf.py:602-638, in place (two kernels, no voxel-sized index tensors)
  TSDFVolume.surface()               tsdf.py:530-536: the top-most voxel with t < 0 per column and its height
  TSDFVolume.surface_cloud(sp)       tsdf.py:538-556: the float64 point cloud the reference hands to plyflatten
  TSDFVolume.extract_dsm(sp, res)    tsdf.py:530-600 without the file write: the surface rasterised on the device
  TSDFVolume.extract_mesh(path)      tsdf.py:522-528 without mcubes: marching cubes on the device (eogs2_amd.mesh)
No CPU / eager fallback: CPU tensors raise.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, dsm_raster, mesh
from ._host import Ctx, on_device, ptr, query_bytes


def volume_axes(vol_bounds, vox_size, device):
    """tsdf.py:387-407: voxel counts and per-axis centre coordinates, the reference's own statements."""
    vb = torch.tensor(np.asarray(vol_bounds), dtype=torch.float32, device=device)
    assert vb.shape == (3, 2), "vol_bounds should be of shape (3,2)"
    n = (vb[:, 1] - vb[:, 0]) // vox_size + 1
    n = n.ceil().long()
    starts = vb[:, 0]
    ends = vb[:, 0] + n * vox_size
    dims = tuple(n.cpu().numpy().tolist())
    axes = [torch.linspace(starts[i], ends[i], dims[i], device=device) for i in range(3)]
    return dims, axes


class TSDFVolume:
    def __init__(self, vol_bounds, vox_size, trunc_margin_fact, device="cuda:0"):
        self.device = torch.device(device)
        self.vox_size = vox_size
        self._trunc_margin = trunc_margin_fact * self.vox_size
        self.num_voxels_per_dimension, self.axes = volume_axes(vol_bounds, vox_size, self.device)
        self._tsdf_vol = torch.ones(size=self.num_voxels_per_dimension, device=self.device, dtype=torch.float32)
        self._weight_vol = torch.zeros(size=self.num_voxels_per_dimension, device=self.device, dtype=torch.float32)

    def integrate(self, rangeimage):
        integrate(self._tsdf_vol, self._weight_vol, self.axes, rangeimage.affine_model[0], rangeimage.affine_model[1],
                  float(rangeimage.model_scale), float(self._trunc_margin), rangeimage.altitude_img,
                  rangeimage.get_weights())

    def apply_prior(self):
        """tsdf.py:602-638, in place."""
        apply_prior(self._tsdf_vol, self._weight_vol)

    def surface(self):
        """tsdf.py:530-536: (index int64 [nx, ny] = the top-most z with t < 0, 0 if none; height f32 [nx, ny] = axes[2][index])."""
        return surface(self._tsdf_vol, self.axes[2])

    def surface_cloud(self, scene_params):
        """tsdf.py:538-556: the array the reference's extract_dsm hands to plyflatten, float64 [nx * ny, 3]
        (x, y, height in fp32 on the device, then `+ scene_params[0]` on the host)."""
        _, height = self.surface()
        xy = torch.stack(torch.meshgrid([self.axes[0], self.axes[1]], indexing="ij"), dim=-1)
        cloud = torch.cat([xy, height.unsqueeze(-1)], dim=-1).detach().cpu().reshape(-1, 3).numpy()
        return cloud + scene_params[0]

    def extract_dsm(self, scene_params, resolution):
        """tsdf.py:530-600 without the file write: (profile, dsm float32 [ysize, xsize, 1]) on the device. x, y and the
        height go to the raster kernel as fp32, `+ scene_params[0]` happens there in double; the grid comes from the
        bounds of those points (the one host wait). The profile is dsm_raster.make_profile's plain dict."""
        _, height = self.surface()
        return dsm_raster.dsm_from_surface(height, self.axes[0], self.axes[1], scene_params, resolution)

    def extract_mesh(self, output_mesh_path=None, *, coords="index", scene_params=None, iso=0.0):
        """tsdf.py:522-528 without mcubes: (vertices float64 [NV, 3], triangles int32 [NT, 3]) on the device, and the OBJ
        file when a path is given. coords="index": voxel units, what `mcubes.marching_cubes(vol, 0)` returns;
        coords="world": interpolated between the volume's fp32 axes. `scene_params[0]` is added in double when given, as
        surface_cloud and extract_dsm add it. Semantics and ordering: include/eogs_mesh.h."""
        if coords not in ("index", "world"):
            raise ValueError(f"tsdf extract_mesh: coords is 'index' or 'world', not {coords!r}")
        vertices, triangles = mesh.marching_cubes(self._tsdf_vol, iso, axes=self.axes if coords == "world" else None,
                                                  shift=None if scene_params is None else scene_params[0])
        if output_mesh_path is not None:
            mesh.export_obj(vertices, triangles, output_mesh_path)
        return vertices, triangles


class RangeImage:
    """The reference's RangeImageEOGS (tsdf.py:186-323) on the GPU: `metadata` is its dict (`img`, `model.scale`,
    `model.coef_`, `model.intercept_`), `altitude_img` a numpy array or a tensor, [H, W] or [1, 1, H, W]. Attributes as in
    the reference: img_name, model_scale, affine_model, view_direction, altitude_img [1,1,H,W], height, width,
    pixels_normals [1,3,H,W], pixels_angle [1,1,H,W]. The weights come out of the same kernel: get_weights() returns
    clamp(pixels_angle, 0, 1) as computed at construction."""

    def __init__(self, metadata, altitude_img, device="cuda:0"):
        self.device = altitude_img.device if torch.is_tensor(altitude_img) else torch.device(device)
        self.img_name = metadata["img"]
        self.model_scale = metadata["model"]["scale"]
        self.affine_model = (torch.tensor(metadata["model"]["coef_"], dtype=torch.float32, device=self.device),
                             torch.tensor(metadata["model"]["intercept_"], dtype=torch.float32, device=self.device))
        self.view_direction = view_direction(self.affine_model[0])
        alt = torch.as_tensor(altitude_img).to(device=self.device, dtype=torch.float32)
        if alt.ndim == 2:
            alt = alt[None, None]
        if alt.ndim != 4 or alt.shape[:2] != (1, 1):
            raise RuntimeError("RangeImage: altitude_img must be [H, W] or [1, 1, H, W]")
        self.altitude_img = alt.contiguous()
        _, _, self.height, self.width = self.altitude_img.shape
        self.pixels_normals, self.pixels_angle, self._weights = normals(self.altitude_img, *self.affine_model,
                                                                        view_dir=self.view_direction)

    def get_weights(self):
        return self._weights


RangeImageEOGS = RangeImage


def _affine24(coef, intercept, dev):
    """f32[24] = coef, intercept, inv(coef), inv(coef) @ intercept (tsdf.py:234, :238-240): the layout of include/eogs_tsdf.h."""
    f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    A, b = f(coef).reshape(3, 3), f(intercept).reshape(3)
    Ainv = torch.linalg.inv(A)
    return torch.cat([A.reshape(-1), b, Ainv.reshape(-1), Ainv @ b])


def view_direction(coef):
    """tsdf.py:213-218: normalize(solve(coef, e3), eps=1e-6)."""
    v = torch.linalg.solve(coef, torch.tensor([0, 0, 1.0], device=coef.device))
    return F.normalize(v, dim=0, eps=1e-6)


_on_device = functools.partial(on_device, "tsdf", "the TSDF stages run")


def normals(altitude_img, coef, intercept, view_dir=None, with_normals=True, with_weights=True):
    """tsdf.py:213-231, 243-323 in one kernel: (pixels_normals [1,3,H,W] or None, pixels_angle [1,1,H,W],
    weights [1,1,H,W] = clamp(angle, 0, 1) or None) of an altitude image [H, W] or [1, 1, H, W]."""
    _on_device(altitude_img, "normals")
    abi = _lib.get()
    dev = altitude_img.device
    alt = altitude_img.detach().to(dtype=torch.float32).contiguous()
    H, W = alt.shape[-2:]
    if alt.numel() != H * W or H * W == 0:
        raise RuntimeError("tsdf normals: the altitude image must be a non-empty single-channel H x W")
    affine = _affine24(coef, intercept, dev)
    vd = (view_direction(coef.detach().to(device=dev, dtype=torch.float32).reshape(3, 3)) if view_dir is None else view_dir)
    vd = vd.detach().to(device=dev, dtype=torch.float32).contiguous()
    n = torch.empty((1, 3, H, W), device=dev, dtype=torch.float32) if with_normals else None
    angle = torch.empty((1, 1, H, W), device=dev, dtype=torch.float32)
    wgt = torch.empty((1, 1, H, W), device=dev, dtype=torch.float32) if with_weights else None
    with Ctx(abi, dev) as cx:
        abi.check(abi.tsdf_normals(H, W, ptr(alt), ptr(affine), ptr(vd), ptr(n), ptr(angle), ptr(wgt), cx.stream))
    return n, angle, wgt


def _check_volume(t, what):
    _on_device(t, what)
    if t.dtype != torch.float32 or not t.is_contiguous() or t.ndim != 3:
        raise RuntimeError(f"tsdf {what}: volumes must be contiguous float32 [nx, ny, nz]")


def apply_prior(tsdf_vol, weight_vol):
    """tsdf.py:602-638 in place on `tsdf_vol` / `weight_vol` (f32[nx,ny,nz], contiguous)."""
    for t in (tsdf_vol, weight_vol):
        _check_volume(t, "apply_prior")
    abi = _lib.get()
    if tsdf_vol.shape != weight_vol.shape or tsdf_vol.device != weight_vol.device:
        raise RuntimeError("tsdf apply_prior: the volumes differ in shape or device")
    nx, ny, nz = tsdf_vol.shape
    n = query_bytes(abi, "tsdf_prior_bytes", nx, ny, nz)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=tsdf_vol.device)
    with Ctx(abi, tsdf_vol.device) as cx:
        abi.check(abi.tsdf_prior(nx, ny, nz, ptr(tsdf_vol), ptr(weight_vol), ptr(ws), n, cx.stream))


def surface(tsdf_vol, z_axis):
    """tsdf.py:530-536: (index int64 [nx, ny], height f32 [nx, ny]) with index = argmax((t < 0) * arange(nz)) (the
    top-most voxel with t < 0; 0 if the column has none) and height = z_axis[index]."""
    _check_volume(tsdf_vol, "surface")
    abi = _lib.get()
    nx, ny, nz = tsdf_vol.shape
    az = z_axis.detach().to(device=tsdf_vol.device, dtype=torch.float32).contiguous()
    if az.numel() != nz:
        raise RuntimeError("tsdf surface: the z axis does not match the volume")
    index = torch.empty((nx, ny), dtype=torch.int64, device=tsdf_vol.device)
    height = torch.empty((nx, ny), dtype=torch.float32, device=tsdf_vol.device)
    with Ctx(abi, tsdf_vol.device) as cx:
        abi.check(abi.tsdf_surface(nx, ny, nz, ptr(tsdf_vol), ptr(az), ptr(index), ptr(height), cx.stream))
    return index, height


def integrate(tsdf_vol, weight_vol, axes, coef, intercept, model_scale, trunc_margin, altitude_img, weight_img):
    """In place on `tsdf_vol` / `weight_vol` (f32[nx,ny,nz], contiguous)."""
    abi = _lib.get()
    dev = tsdf_vol.device
    for t in (tsdf_vol, weight_vol):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.ndim != 3:
            raise RuntimeError("tsdf integrate: volumes must be contiguous float32 [nx, ny, nz]")
    if tsdf_vol.shape != weight_vol.shape:
        raise RuntimeError("tsdf integrate: volume shapes differ")
    nx, ny, nz = tsdf_vol.shape
    f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    ax, ay, az = (f(a) for a in axes)
    if (ax.numel(), ay.numel(), az.numel()) != (nx, ny, nz):
        raise RuntimeError("tsdf integrate: axes do not match the volume")
    affine = _affine24(coef, intercept, dev)  # tsdf.py:238-239
    alt, wgt = f(altitude_img), f(weight_img)
    H, W = alt.shape[-2:]
    if alt.numel() != H * W or wgt.numel() != H * W:
        raise RuntimeError("tsdf integrate: altitude and weight images must be single-channel H x W")
    with Ctx(abi, dev) as cx:
        abi.check(abi.tsdf_integrate(nx, ny, nz, ptr(ax), ptr(ay), ptr(az), ptr(affine), model_scale, trunc_margin,
                                     H, W, ptr(alt), ptr(wgt), ptr(tsdf_vol), ptr(weight_vol), cx.stream))


__all__ = ["RangeImage", "RangeImageEOGS", "TSDFVolume", "apply_prior", "integrate", "normals", "surface", "view_direction",
           "volume_axes"]
