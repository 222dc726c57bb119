"""Generates tests/golden/dsm_raster/*.npz by running the REFERENCE's own `compute_dsm_from_view` (utils/dsm_utils.py:7-51)
and `TSDFVolume.extract_dsm` (tsdf.py:530-600), unmodified, on seeded inputs. Only inputs and outputs are stored.

    python tests/golden/make_golden_dsm_raster.py

As in make_golden_tsdf_post.py, `plyflatten`, `plyflatten.utils`, `rasterio` and `affine` are stubs in sys.modules and
`tsdf.py` is loaded by make_golden_tsdf.load_ref; MKL runs its CPU-independent code path (MKL_CBWR=COMPATIBLE). The stub
`plyflatten` is third-party code that is not installed here: it RECORDS the cloud and the geometry it is handed — the
reference's own — and returns the float64 numpy restatement of the raster's stated semantics (tests/dsm_raster_cases.py
`restate`, accumulated with np.add.at; include/eogs_dsm.h) narrowed to float32.

  view   `view` is a namespace with the camera's `affine` (4 x 4, transposed) and `Ainv`, built by the statements of
         scene/cameras/affine_cameras.py:151-159, and the reference's `UVA_to_ECEF` (:440-447) bound to it; `rendered_uva`
         is stacked from the UV grid of :139-143 and a seeded altitude as train_pan.py:766-768 stacks it; `scene_name` holds
         "JAX" (resolution 0.5) or "IARPA" (0.3). 48 x 40 and 160 x 128, sheared cameras.
  tsdf   small built volumes (make_golden_tsdf_post.built_volume) through extract_dsm.

Stored per case: the inputs, the cloud (x and y in <name>_xy.npz, z in <name>.npz: every file stays under 400 KiB), the
geometry, the float64 mean per cell and the counts. The generator asserts two margins and takes the next seed otherwise:
no point's fractional cell coordinate and none of the four bound quotients is within 1e-6 of an integer, so that a 1-ulp
float64 difference in the matrix-vector product can move neither a point nor the grid.
"""
import importlib.util
import os
import sys
import types

os.environ["MKL_CBWR"] = "COMPATIBLE"  # before torch loads MKL

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from dsm_raster_cases import MAX_FIXTURE_BYTES, restate  # noqa: E402
from make_golden_tsdf import REFROOT, load_ref, view  # noqa: E402
from make_golden_tsdf_post import built_volume, small_volume, stub_dsm_writers  # noqa: E402

OUT = os.path.join(HERE, "dsm_raster")  # a directory of its own: tests/util.py takes every top-level golden/*.npz
MARGIN = 1e-6


def stub_plyflatten():
    """make_golden_tsdf_post's stubs, with a plyflatten that records what it is handed and answers with the restatement."""
    stub_dsm_writers()
    calls = []

    def plyflatten(cloud, xoff, yoff, resolution, xsize, ysize, radius=1, sigma=float("inf")):
        assert sigma == float("inf")
        mean, counts, skipped = restate(cloud, xoff, yoff, resolution, xsize, ysize, radius)
        assert skipped == 0
        calls.append(dict(cloud=np.array(cloud, dtype=np.float64, copy=True), xoff=np.float64(xoff), yoff=np.float64(yoff),
                          resolution=np.float64(resolution), xsize=np.int64(xsize), ysize=np.int64(ysize), radius=np.int64(radius),
                          raster=mean, counts=counts))
        return mean.astype(np.float32)[:, :, None]

    sys.modules["plyflatten"].plyflatten = plyflatten
    return calls


def load_module(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REFROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def away_from_integers(q):
    return bool((np.abs(q - np.round(q)) > MARGIN).all())


def margins_hold(rec):
    c, res = rec["cloud"], rec["resolution"]
    xmin, xmax, ymin, ymax = c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max()
    bounds = np.array([xmin / res, (xmax - rec["xoff"]) / res, ymax / res, (ymin - rec["yoff"]) / res])
    return (away_from_integers((c[:, 0] - rec["xoff"]) / res) and away_from_integers((rec["yoff"] - c[:, 1]) / res)
            and away_from_integers(bounds))


def save(name, rec, inputs):
    os.makedirs(OUT, exist_ok=True)
    cloud = rec.pop("cloud")
    main = dict(inputs, cloud_z=np.ascontiguousarray(cloud[:, 2]), **rec)
    for suffix, d in (("", main), ("_xy", dict(cloud_xy=np.ascontiguousarray(cloud[:, :2])))):
        path = os.path.join(OUT, f"{name}{suffix}.npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < MAX_FIXTURE_BYTES, (path, size)
        print(f"dsm_raster/{name}{suffix}: {size // 1024} KB")
    print(f"    {rec['ysize']} x {rec['xsize']} cells, {int((rec['counts'] > 0).sum())} filled, most contributions {rec['counts'].max()}")


def view_case(cams, dsm_utils, calls, name, H, W, shear, scene_name, scale, seed0):
    for seed in range(seed0, seed0 + 50):
        coef, intercept, alt = view(H, W, seed, shear)
        cam = types.SimpleNamespace()
        cam.affine = torch.eye(4, 4)  # affine_cameras.py:151-159
        cam.affine[:3, :3] = coef
        cam.affine[:3, -1] = intercept
        cam.affine = cam.affine.float().T
        cam.Ainv = torch.inverse(cam.affine[:3, :3].T)
        cam.UVA_to_ECEF = types.MethodType(cams.AffineCamera.UVA_to_ECEF, cam)
        u_axis, v_axis = torch.linspace(-1, 1, W), torch.linspace(-1, 1, H)  # :139-143
        uv_grid = torch.meshgrid(u_axis, v_axis, indexing="xy")
        rendered_uva = torch.stack(uv_grid + (alt,), dim=-1)  # train_pan.py:766-768
        g = np.random.default_rng(seed)
        center = np.array([512345.0, 4321987.0, 31.5]) + g.random(3)
        scene_params = [center, scale, 17, "T"]
        calls.clear()
        profile, dsm = dsm_utils.compute_dsm_from_view(cam, rendered_uva, scene_params, scene_name)
        (rec,) = calls
        if not margins_hold(rec):
            print(f"    {name}: seed {seed} misses a margin, next")
            continue
        assert (profile["height"], profile["width"]) == (rec["ysize"], rec["xsize"]) and dsm.dtype == np.float32
        save(name, rec, dict(altitude=alt.numpy(), affine=cam.affine.numpy(), Ainv=cam.Ainv.numpy(), u_axis=u_axis.numpy(),
                             v_axis=v_axis.numpy(), center=center, scale=np.float64(scale), seed=np.int64(seed)))
        return
    raise RuntimeError(f"{name}: no seed holds the margins")


def tsdf_case(ref, calls, name, dims, resolution, seed0):
    for seed in range(seed0, seed0 + 50):
        vol = small_volume(ref, dims)
        t, w = built_volume(dims, seed)
        vol._tsdf_vol, vol._weight_vol = torch.as_tensor(t).clone(), torch.as_tensor(w).clone()
        g = np.random.default_rng(seed)
        center = np.array([512345.0, 4321987.0, 31.5]) + g.random(3)
        calls.clear()
        dsm = ref.TSDFVolume.extract_dsm(vol, [center, 1.0, 17, "T"], resolution, OUT)  # the stub rasterio writes nothing
        (rec,) = calls
        if not margins_hold(rec):
            print(f"    {name}: seed {seed} misses a margin, next")
            continue
        assert dsm.shape == (rec["ysize"], rec["xsize"], 1)
        save(name, rec, dict(tsdf=t, axis0=vol.axes[0].numpy().copy(), axis1=vol.axes[1].numpy().copy(),
                             axis2=vol.axes[2].numpy().copy(), center=center, seed=np.int64(seed)))
        return
    raise RuntimeError(f"{name}: no seed holds the margins")


def main():
    calls = stub_plyflatten()
    ref = load_ref()
    dsm_utils = load_module("ref_dsm_utils", "utils/dsm_utils.py")
    cams = load_module("ref_affine_cameras", "scene/cameras/affine_cameras.py")
    torch.manual_seed(0)
    view_case(cams, dsm_utils, calls, "view_48x40", 48, 40, 0.15, "JAX_004", 7.0, 31)
    view_case(cams, dsm_utils, calls, "view_160x128", 160, 128, 0.3, "IARPA_001", 13.0, 41)
    tsdf_case(ref, calls, "tsdf_23x17x9", (23, 17, 9), 0.3, 300)
    tsdf_case(ref, calls, "tsdf_40x33x12", (40, 33, 12), 0.5, 310)


if __name__ == "__main__":
    main()
