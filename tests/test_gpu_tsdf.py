"""GPU (MI355X): TSDF integration (include/eogs_tsdf.h, eogs2_amd/tsdf.py) through the C-ABI against the restatement of
the reference's statements (oracle/tsdf_oracle.py) in float64 on the CPU and in fp32 on the GPU (the op sequence the
reference executes), plus size-independent properties on a 4M-voxel volume."""
import glob
import os
import types

import numpy as np
import pytest
import torch

import tsdf_cases as tc
from oracle import tsdf_oracle as O
from tsdf_cases import assert_attributed, scene
from util import GOLDEN_DIR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def references(vol_axes, views, scale, trunc):
    return tc.reference([a.cpu() for a in vol_axes], views, scale, trunc)


@pytest.mark.parametrize("H,W,bounds,vox", [
    (48, 64, [[-1.4, 1.4], [-1.3, 1.3], [-0.3, 0.4]], 0.06),
    (33, 17, [[-0.5, 0.5], [-0.5, 0.5], [-0.2, 0.3]], 0.031),
    (64, 64, [[-4.0, -3.5], [-0.2, 0.2], [0.0, 0.1]], 0.05),  # entirely outside the view: nothing changes
])
def test_integrate_matches_restatement(dev, H, W, bounds, vox):
    from eogs2_amd.tsdf import TSDFVolume

    scale, fact = 1.7, 3.0
    vol = TSDFVolume(np.array(bounds), vox, fact, device=dev)
    t_ref = torch.ones(vol.num_voxels_per_dimension, dtype=torch.float64)
    w_ref = torch.zeros(vol.num_voxels_per_dimension, dtype=torch.float64)
    t32 = torch.ones(vol.num_voxels_per_dimension, device=dev)
    w32 = torch.zeros(vol.num_voxels_per_dimension, device=dev)
    axes64 = [a.double().cpu() for a in vol.axes]
    views = [scene(H, W, seed) for seed in (1, 2, 3)]
    for coef, intercept, alt, wgt in views:  # three views accumulated
        ri = types.SimpleNamespace(affine_model=(coef.to(dev), intercept.to(dev)), model_scale=scale, altitude_img=alt.to(dev),
                                   get_weights=lambda wgt=wgt: wgt.to(dev))
        vol.integrate(ri)
        t_ref, w_ref = O.integrate(t_ref, w_ref, axes64, coef.double(), intercept.double(), scale, fact * vox, alt.double(), wgt.double())
        t32, w32 = O.integrate(t32, w32, vol.axes, coef.to(dev), intercept.to(dev), scale, fact * vox, alt.to(dev), wgt.to(dev))
    # an outlier only where the restatement's own fp32 and float64 runs place a decision within their margin (tests/tsdf_cases.py)
    ref = references(vol.axes, views, scale, fact * vox)
    assert_attributed(vol._tsdf_vol, t_ref, 2e-4, ref, "tsdf vs float64 restatement")
    assert_attributed(vol._weight_vol, w_ref, 2e-4, ref, "weights vs float64 restatement")
    assert_attributed(vol._tsdf_vol, t32, 2e-5, ref, "tsdf vs fp32 op sequence")
    assert_attributed(vol._weight_vol, w32, 2e-5, ref, "weights vs fp32 op sequence")
    if bounds[0][1] < -3.0:
        assert torch.equal(vol._tsdf_vol, torch.ones_like(vol._tsdf_vol)) and float(vol._weight_vol.abs().max()) == 0.0


def test_full_size_properties(dev):
    """256 x 256 x 64 voxels, 1024^2 image: determinism; integrating the same image twice leaves the TSDF where it was
    and doubles the weights; untouched voxels keep their initial values."""
    from eogs2_amd.tsdf import TSDFVolume

    coef, intercept, alt, wgt = scene(1024, 1024, 5)
    wgt = wgt.clamp(min=0.05)
    ri = types.SimpleNamespace(affine_model=(coef.to(dev), intercept.to(dev)), model_scale=1.0, altitude_img=alt.to(dev),
                               get_weights=lambda: wgt.to(dev))
    bounds = np.array([[-1.2, 1.2], [-1.2, 1.2], [-0.3, 0.35]])
    a = TSDFVolume(bounds, 2.4 / 255, 4.0, device=dev)
    b = TSDFVolume(bounds, 2.4 / 255, 4.0, device=dev)
    assert a._tsdf_vol.numel() >= 4_000_000
    a.integrate(ri)
    b.integrate(ri)
    assert torch.equal(a._tsdf_vol, b._tsdf_vol) and torch.equal(a._weight_vol, b._weight_vol)
    touched = a._weight_vol > 0
    assert 0.05 < float(touched.float().mean()) < 0.95
    assert torch.equal(a._tsdf_vol[~touched], torch.ones_like(a._tsdf_vol[~touched]))
    b.integrate(ri)
    assert torch.allclose(b._weight_vol, 2 * a._weight_vol, rtol=1e-6, atol=0)
    assert torch.allclose(b._tsdf_vol, a._tsdf_vol, rtol=0, atol=2e-6)
    assert float(a._tsdf_vol.max()) <= 1.0 and float(a._tsdf_vol[touched].min()) >= -1.0 - 1e-6


# ---- vectors from the REFERENCE's own tsdf.py (tests/golden/make_golden_tsdf.py; tests/test_tsdf_oracle.py pins the restatement) ----
TSDF_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "tsdf_*.npz")))


@pytest.mark.parametrize("path", TSDF_FIXTURES, ids=lambda p: os.path.basename(p)[5:-4])
def test_integrate_matches_reference_vectors(dev, path):
    """eogs2_amd.tsdf.TSDFVolume (constructor + one HIP kernel per view) against the volumes the reference's
    TSDFVolume.integrate produced after every accumulated view, NaN voxels of the zero-weight region included."""
    from eogs2_amd.tsdf import TSDFVolume

    z = np.load(path)
    c = {k: z[k] for k in z.files}
    vol = TSDFVolume(c["vol_bounds"], float(c["vox_size"]), float(c["trunc_margin_fact"]), device=dev)
    assert tuple(vol.num_voxels_per_dimension) == tuple(int(x) for x in c["num_voxels"])
    for i in range(3):
        assert torch.equal(vol.axes[i].cpu(), torch.as_tensor(c[f"axis{i}"]))
    t = lambda k: torch.as_tensor(c[k]).to(dev)
    views = [tuple(torch.as_tensor(c[f"v{v}_{k}"]) for k in ("coef", "intercept", "altitude", "weights")) for v in range(int(c["n_views"]))]
    for v in range(int(c["n_views"])):
        ri = types.SimpleNamespace(affine_model=(t(f"v{v}_coef"), t(f"v{v}_intercept")), model_scale=float(c["model_scale"]),
                                   altitude_img=t(f"v{v}_altitude"), get_weights=lambda v=v: t(f"v{v}_weights"))
        vol.integrate(ri)
        ref = tc.reference([a.cpu() for a in vol.axes], views[: v + 1], float(c["model_scale"]), float(c["trunc_margin"]))
        assert_attributed(vol._tsdf_vol, torch.as_tensor(c[f"v{v}_tsdf_vol"]), 2e-5, ref, f"view {v}: tsdf vs the reference's volume")
        assert_attributed(vol._weight_vol, torch.as_tensor(c[f"v{v}_weight_vol"]), 2e-5, ref, f"view {v}: weights vs the reference's volume")
    if "outside" in path:
        assert torch.equal(vol._tsdf_vol, torch.ones_like(vol._tsdf_vol)) and float(vol._weight_vol.abs().max()) == 0.0


# ---- shapes, exact lattices and planted non-finite pixels (tests/tsdf_cases.py) ----
def run_hip(dev, axes, views, scale, trunc, t0=None, w0=None):
    from eogs2_amd.tsdf import integrate

    dims = tuple(int(a.numel()) for a in axes)
    t = (torch.ones(dims) if t0 is None else t0.clone()).to(dev)
    w = (torch.zeros(dims) if w0 is None else w0.clone()).to(dev)
    ax = [a.to(dev) for a in axes]
    for coef, intercept, alt, wgt in views:
        integrate(t, w, ax, coef.to(dev), intercept.to(dev), scale, trunc, alt.to(dev), wgt.to(dev))
    return t, w


@pytest.mark.parametrize("name", list(tc.SHAPES))
def test_integrate_shapes_attributed(dev, name):
    axes, views = tc.shape_case(name)
    ref = tc.reference(axes, views, tc.SCALE, tc.TRUNC)
    t, w = run_hip(dev, axes, views, tc.SCALE, tc.TRUNC)
    for got, k in ((t, "t"), (w, "w")):
        tc.assert_attributed(got, ref[k + "64"], 2e-4, ref, f"{name}: {k} vs float64 restatement")
        tc.assert_attributed(got, ref[k + "32"], 2e-5, ref, f"{name}: {k} vs fp32 op sequence")


@pytest.mark.parametrize("scale", tc.LATTICE_SCALES)
def test_integrate_exact_lattice_bit_for_bit(dev, scale):
    """Nothing rounds (tests/test_tsdf_cases.py shows it for the restatement): the float64 result, bit for bit, with |u| = 1 and
    |v| = 1 valid, one step outside untouched (pre-filled NaN and -0 keep their bits), sdf == -trunc included."""
    axes, views, t0, w0 = tc.lattice_case(scale)
    ref = tc.reference(axes, views, scale, tc.LATTICE_TRUNC, t0, w0)
    for n_views in (1, 2):
        r = ref if n_views == 2 else tc.reference(axes, views[:1], scale, tc.LATTICE_TRUNC, t0, w0)
        t, w = run_hip(dev, axes, views[:n_views], scale, tc.LATTICE_TRUNC, t0, w0)
        assert torch.equal(tc.bits(t), tc.bits(r["t64"].float())), f"tsdf after {n_views} view(s)"
        assert torch.equal(tc.bits(w), tc.bits(r["w64"].float())), f"weights after {n_views} view(s)"


@pytest.mark.parametrize("plant", tc.PLANTS, ids=lambda p: f"{p[0]}_{p[1]}")
def test_integrate_one_non_finite_pixel(dev, plant):
    """One planted pixel on the exact lattice: the fp32 op sequence's NaN / +inf / -inf pattern and finite values exactly, the
    untouched voxels' bits; a weight of 0 gives the reference's 0 / 0."""
    axes, views, t0, w0 = tc.lattice_case(1.0, plant)
    ref = tc.reference(axes, views, 1.0, tc.LATTICE_TRUNC, t0, w0)
    for n_views in (1, 2):
        r = ref if n_views == 2 else tc.reference(axes, views[:1], 1.0, tc.LATTICE_TRUNC, t0, w0)
        t, w = run_hip(dev, axes, views[:n_views], 1.0, tc.LATTICE_TRUNC, t0, w0)
        for got, exp, k in ((t, r["t32"], "tsdf"), (w, r["w32"], "weights")):
            got = got.cpu()
            for what, f in (("NaN", torch.isnan), ("+inf", lambda x: x == float("inf")), ("-inf", lambda x: x == float("-inf"))):
                assert torch.equal(f(got), f(exp)), f"{k} after {n_views} view(s): {what} pattern differs"
            fin = torch.isfinite(exp)
            assert torch.equal(tc.bits(got)[fin], tc.bits(exp)[fin]), f"{k} after {n_views} view(s): finite voxels differ"
    if plant == ("weight", 0.0):
        assert int(torch.isnan(t[1:]).sum()) > 0  # 0 / 0 under the pixel (x index 0 is the pre-filled NaN)


@pytest.mark.parametrize("row,col", [(1, 0), (2, 2)])
def test_integrate_nan_in_coef_updates_nothing(dev, row, col):
    """The kernel itself, through the C ABI. The affine block is the one the product's host set-up builds (coef, intercept,
    inv(coef), inv(coef) @ intercept), built here on the CPU, where torch.linalg.inv of a matrix with a NaN is NaN throughout:
    a NaN in a row of u or v fails the view test; a NaN in the altitude row leaves u and v valid and is stopped by the NaN sdf
    that the NaN inverse gives, which fails `sdf >= -trunc`."""
    from eogs2_amd import _lib
    from eogs2_amd._host import Ctx, ptr
    from eogs2_amd.tsdf import _affine24

    axes, views, t0, w0 = tc.lattice_case(1.0)
    coef, intercept, alt, wgt = views[0]
    bad = coef.clone()
    bad[row, col] = float("nan")
    affine = _affine24(bad, intercept, torch.device("cpu"))
    assert int(torch.isnan(affine[:9]).sum()) == 1 and bool(torch.isnan(affine[12:]).all())
    affine = affine.to(dev)
    t, w = t0.clone().to(dev), w0.clone().to(dev)
    ax = [a.to(dev).contiguous() for a in axes]
    a_img, w_img = alt.to(dev).contiguous(), wgt.to(dev).contiguous()
    abi = _lib.get()
    with Ctx(abi, dev) as cx:
        abi.check(abi.tsdf_integrate(*t.shape, ptr(ax[0]), ptr(ax[1]), ptr(ax[2]), ptr(affine), 1.0, tc.LATTICE_TRUNC, 9, 9,
                                     ptr(a_img), ptr(w_img), ptr(t), ptr(w), cx.stream))
    torch.cuda.synchronize()
    assert torch.equal(tc.bits(t), tc.bits(t0)) and torch.equal(tc.bits(w), tc.bits(w0))
    # the same call with the clean matrix does update: the block above reached the kernel's decision, not an early return
    affine = _affine24(coef, intercept, torch.device("cpu")).to(dev)
    with Ctx(abi, dev) as cx:
        abi.check(abi.tsdf_integrate(*t.shape, ptr(ax[0]), ptr(ax[1]), ptr(ax[2]), ptr(affine), 1.0, tc.LATTICE_TRUNC, 9, 9,
                                     ptr(a_img), ptr(w_img), ptr(t), ptr(w), cx.stream))
    ref = tc.reference(axes, views[:1], 1.0, tc.LATTICE_TRUNC, t0, w0)
    assert torch.equal(tc.bits(t), tc.bits(ref["t64"].float())) and torch.equal(tc.bits(w), tc.bits(ref["w64"].float()))
