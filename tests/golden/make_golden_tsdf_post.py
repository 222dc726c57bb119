"""Generates tests/golden/tsdf_post/*.npz by running the REFERENCE's own `tsdf.py` (loaded by make_golden_tsdf.load_ref,
which stubs its module-level imports and answers the CPU for its hard-wired cuda:0) on seeded inputs. Only inputs and
outputs are stored.

    python tests/golden/make_golden_tsdf_post.py

Stages (src/gaussiansplatting/tsdf.py):
  normals   RangeImageEOGS(metadata, altitude): view_direction, pixels_normals, pixels_angle, get_weights() (:186-323) on
            ragged images from 5 x 7 to 64 x 48, with a cliff, a shear and a NaN pixel; every image is small enough that
            every pixel within 2 of the border is stored (F.unfold's zero padding of the world-position image).
  prior     TSDFVolume.apply_prior() (:602-638): both volumes before and after, for volumes integrated from reference views
            and for built volumes that hit every rule (isolated voxels in the interior, on faces, edges and corners and at
            z = 0, NaN voxels, t == 0 and t == -0, t == 1 with w > 0, empty and full columns, untouched voxels under
            occupied ones).
  surface   TSDFVolume.extract_dsm() (:525-600) runs unmodified: `plyflatten`, `plyflatten.utils`, `rasterio` and `affine`
            are stubs in sys.modules, and the stub plyflatten keeps the cloud it is handed; the argmax indices are recorded
            on their way through the module's `torch`. scene_params[0] is UTM-sized (~5e5), so the float64 add matters.
  chain     RangeImageEOGS -> integrate -> apply_prior -> extract_dsm over three views.
MKL runs its CPU-independent code path (MKL_CBWR=COMPATIBLE, set before torch loads, as make_golden_tsdf.py does).
"""
import os
import sys
import types

os.environ["MKL_CBWR"] = "COMPATIBLE"  # before torch loads MKL

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_tsdf import load_ref, view  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tsdf_post")  # a directory of its own: the rasterizer's
# fixture list (tests/util.py) is every tests/golden/*.npz that is not a loss_ / shade_ / tsdf_ / resample_ case
CENTER = np.array([512345.25, 4321987.75, 31.5])  # scene_params[0]: a UTM centre


def stub_dsm_writers():
    """The modules extract_dsm imports after it has built the cloud; plyflatten records the cloud."""
    captured = {}

    def plyflatten(cloud, xoff, yoff, resolution, xsize, ysize, radius=1, sigma=float("inf")):
        captured["cloud"] = np.array(cloud, copy=True)
        return np.zeros((ysize, xsize, 1), dtype=np.float32)

    class _Raster:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def write(self, *a, **k):
            pass

    mods = {name: types.ModuleType(name) for name in ("plyflatten", "plyflatten.utils", "rasterio", "affine")}
    mods["plyflatten"].plyflatten = plyflatten
    mods["plyflatten"].utils = mods["plyflatten.utils"]
    mods["plyflatten.utils"].rasterio_crs = lambda x: x
    mods["plyflatten.utils"].crs_proj = lambda *a, **k: None
    mods["rasterio"].open = lambda *a, **k: _Raster()
    mods["affine"].Affine = lambda *a: a
    sys.modules.update(mods)
    return captured


def record_argmax(ref):
    """The module's forwarding `torch` (load_ref) gets an argmax that keeps its last result."""
    rec = {}

    def argmax(*a, **k):
        rec["last"] = torch.argmax(*a, **k)
        return rec["last"]

    ref.torch.argmax = argmax
    return rec


def meta(name, scale, coef, intercept):
    return {"img": name, "model": {"scale": scale, "coef_": coef.tolist(), "intercept_": intercept.tolist()}}


def normals_case(ref, name, H, W, seed, shear, nan_pixel=None, flat=False):
    coef, intercept, alt = view(H, W, seed, shear)
    if flat:  # a plane: many exact left / right ties
        alt = torch.full((H, W), 0.25)
    if nan_pixel is not None:
        alt[nan_pixel] = float("nan")
    ri = ref.RangeImageEOGS(meta(name, 1.0, coef, intercept), alt.numpy())
    return dict(altitude=alt.numpy(), coef=coef.numpy(), intercept=intercept.numpy(), view_direction=ri.view_direction.numpy(),
                pixels_normals=ri.pixels_normals.numpy(), pixels_angle=ri.pixels_angle.numpy(), weights=ri.get_weights().numpy())


def small_volume(ref, dims, vox=0.1):
    bounds = np.array([[0.0, (d - 0.5) * vox] for d in dims])
    vol = ref.TSDFVolume(bounds, vox, 2.0)
    assert tuple(vol.num_voxels_per_dimension) == tuple(dims), vol.num_voxels_per_dimension
    return vol


def built_volume(dims, seed):
    """Every rule of apply_prior and every comparison edge, on purpose."""
    g = np.random.default_rng(seed)
    nx, ny, nz = dims
    vals = np.array([1.0, 1.0, 1.0, 0.6, 0.2, -0.3, -1.0, 0.0, -0.0, np.nan], dtype=np.float32)
    t = vals[g.integers(0, len(vals), size=dims)]
    w = np.where(g.random(dims) < 0.5, 0.0, g.choice([0.25, 1.0, 2.5], size=dims)).astype(np.float32)
    t[g.random(dims) < 0.35] = 1.0  # sparse occupancy leaves isolated voxels
    t[t > 0.5] = np.where(g.random(np.count_nonzero(t > 0.5)) < 0.8, 1.0, 0.6)
    w[(t == 1.0) & (g.random(dims) < 0.3)] = 0.7  # t == 1 with w > 0: not untouched
    # explicit cases: clear a block, then place isolated voxels in the interior, on faces, edges, corners and at z = 0
    t[:, :, :] = np.where(g.random(dims) < 0.5, t, 1.0)
    for (x, y, z) in ((nx // 2, ny // 2, nz // 2), (0, ny // 2, nz // 2), (nx - 1, 1, 2), (0, 0, 0), (nx - 1, ny - 1, nz - 1),
                      (0, ny - 1, nz // 2), (nx // 2, 0, 0), (nx // 3, ny // 3, 0), (nx - 1, ny - 1, 0)):
        sl = tuple(slice(max(c - 1, 0), c + 2) for c in (x, y, z))
        t[sl], w[sl] = 1.0, 0.0
        t[x, y, z], w[x, y, z] = -0.5, 1.0
    t[1, 2, :], w[1, 2, :] = 1.0, 0.0            # an empty column (untouched throughout)
    t[2, 1, :], w[2, 1, :] = -1.0, 1.0           # a full column
    t[3, 3, :], w[3, 3, :] = 1.0, 0.0            # untouched under an occupied voxel, with a NaN and t == 0 in the column
    t[3, 3, nz - 2], t[3, 3, nz - 3], t[3, 3, 1] = -0.25, np.nan, 0.0
    t[4, 2, :], w[4, 2, :] = np.nan, 0.0         # a NaN column
    t[2, 4, :], w[2, 4, :] = -0.0, 0.0           # -0.0 is occupied (<= 0) but not below the surface (< 0)
    return t, w


def prior_case(ref, vol, t, w):
    vol._tsdf_vol = torch.as_tensor(t).clone()
    vol._weight_vol = torch.as_tensor(w).clone()
    before_t, before_w = vol._tsdf_vol.numpy().copy(), vol._weight_vol.numpy().copy()
    vol.apply_prior()
    return dict(tsdf_before=before_t, weight_before=before_w, tsdf_after=vol._tsdf_vol.numpy().copy(),
                weight_after=vol._weight_vol.numpy().copy())


def surface_case(ref, vol, captured, rec):
    captured.clear()
    vol.extract_dsm([CENTER, 1.0, 17, "T"], 0.5, OUT)  # the stub rasterio writes nothing
    return dict(tsdf=vol._tsdf_vol.numpy().copy(), axis0=vol.axes[0].numpy().copy(), axis1=vol.axes[1].numpy().copy(),
                axis2=vol.axes[2].numpy().copy(), center=CENTER, indices=rec["last"].numpy().copy(), cloud=captured["cloud"])


def save(name, d):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **d)
    print(f"tsdf_post/{name}: {os.path.getsize(path) // 1024} KB")


def main():
    ref = load_ref()
    captured = stub_dsm_writers()
    rec = record_argmax(ref)
    torch.manual_seed(0)

    # normals
    d = {}
    for i, (H, W, seed, shear, nan_px, flat) in enumerate([
            (5, 7, 11, 0.15, None, False), (7, 5, 12, 0.0, (3, 2), False), (17, 23, 13, 0.3, None, False),
            (33, 17, 14, 0.15, (16, 0), False), (64, 48, 15, 0.4, (10, 30), False), (48, 64, 16, 0.15, None, False),
            (9, 11, 17, 0.15, None, True)]):
        for k, v in normals_case(ref, f"n{i}", H, W, seed, shear, nan_px, flat).items():
            d[f"c{i}_{k}"] = v
    d["n_cases"] = np.int64(7)
    save("normals", d)

    # prior on built volumes
    d = {}
    for i, dims in enumerate([(7, 6, 5), (9, 8, 70), (12, 11, 130)]):
        vol = small_volume(ref, dims)
        for k, v in prior_case(ref, vol, *built_volume(dims, 100 + i)).items():
            d[f"c{i}_{k}"] = v
    d["n_cases"] = np.int64(3)
    save("prior_built", d)

    # surface on built volumes (the prior's outputs and raw built volumes)
    d = {}
    for i, dims in enumerate([(7, 6, 5), (9, 8, 70), (12, 11, 130)]):
        vol = small_volume(ref, dims)
        t, w = built_volume(dims, 200 + i)
        vol._tsdf_vol, vol._weight_vol = torch.as_tensor(t).clone(), torch.as_tensor(w).clone()
        for k, v in surface_case(ref, vol, captured, rec).items():
            d[f"c{i}_{k}"] = v
    d["n_cases"] = np.int64(3)
    save("surface_built", d)

    # the chain over reference views
    H, W, scale, fact, vox = 48, 64, 1.7, 3.0, 0.06
    bounds = np.array([[-1.4, 1.4], [-1.3, 1.3], [-0.3, 0.45]], dtype=np.float64)
    vol = ref.TSDFVolume(bounds, vox, fact)
    d = dict(vol_bounds=bounds, vox_size=np.float64(vox), trunc_margin_fact=np.float64(fact), model_scale=np.float64(scale),
             n_views=np.int64(3))
    for v, seed in enumerate((21, 22, 23)):
        coef, intercept, alt = view(H, W, seed)
        ri = ref.RangeImageEOGS(meta(f"view{v}", scale, coef, intercept), alt.numpy())
        vol.integrate(ri)
        d.update({f"v{v}_coef": coef.numpy(), f"v{v}_intercept": intercept.numpy(), f"v{v}_altitude": alt.numpy(),
                  f"v{v}_weights": ri.get_weights().numpy()})
    d["tsdf_integrated"], d["weight_integrated"] = vol._tsdf_vol.numpy().copy(), vol._weight_vol.numpy().copy()
    vol.apply_prior()
    d["tsdf_prior"], d["weight_prior"] = vol._tsdf_vol.numpy().copy(), vol._weight_vol.numpy().copy()
    for k, v in surface_case(ref, vol, captured, rec).items():
        if k != "tsdf":
            d[k] = v
    save("chain_48x64", d)


if __name__ == "__main__":
    main()
