"""CPU: the restatement of the TSDF stages around integrate (tests/tsdf_post_cases.py) against vectors produced by the
REFERENCE's own tsdf.py (tests/golden/make_golden_tsdf_post.py: RangeImageEOGS, TSDFVolume.apply_prior and extract_dsm
executed unmodified on the CPU), bit for bit in fp32; and the product's TSDF stages refuse CPU tensors (no fallback)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tsdf_post_cases as P
from util import GOLDEN_DIR

POST_DIR = os.path.join(GOLDEN_DIR, "tsdf_post")
FIXTURES = sorted(glob.glob(os.path.join(POST_DIR, "*.npz")))
STAGES = ("normals", "prior_built", "surface_built", "chain_48x64")


def load(name):
    z = np.load(os.path.join(POST_DIR, f"{name}.npz"))
    return {k: z[k] for k in z.files}


def bits(a, b):
    """Equal bit for bit, NaN pattern included (a NaN's payload aside)."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(-1).view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                                               b[~nb].view(-1).view(torch.int32 if b.dtype == torch.float32 else torch.int64))


def test_fixtures_present():
    assert sorted(os.path.basename(p)[:-4] for p in FIXTURES) == sorted(STAGES)
    for p in FIXTURES:
        assert os.path.getsize(p) < 400 * 1024


def in_child(stage):
    """fp32 bit for bit holds on the MKL code path the vectors were made on (MKL_CBWR=COMPATIBLE, read once at start: the
    case runs in a child process), as tests/test_tsdf_oracle.py does."""
    node = f"{os.path.abspath(__file__)}::test_restatement_matches_reference_vectors[{stage}]"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", node],
                       env=dict(os.environ, MKL_CBWR="COMPATIBLE"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("stage", STAGES)
def test_restatement_matches_reference_vectors(stage):
    if os.environ.get("MKL_CBWR") != "COMPATIBLE":
        in_child(stage)
        return
    c = load(stage)
    t = lambda k: torch.as_tensor(c[k])
    if stage == "normals":
        for i in range(int(c["n_cases"])):
            vd, n, angle, wgt = P.reconstruct(t(f"c{i}_altitude"), t(f"c{i}_coef"), t(f"c{i}_intercept"))
            assert bits(vd, c[f"c{i}_view_direction"]), f"case {i}: view_direction"
            assert bits(n, c[f"c{i}_pixels_normals"]), f"case {i}: pixels_normals"
            assert bits(angle, c[f"c{i}_pixels_angle"]), f"case {i}: pixels_angle"
            assert bits(wgt, c[f"c{i}_weights"]), f"case {i}: weights"
        nan_cases = [i for i in range(int(c["n_cases"])) if np.isnan(c[f"c{i}_altitude"]).any()]
        assert len(nan_cases) >= 2 and all(np.isnan(c[f"c{i}_pixels_angle"]).any() for i in nan_cases)
        # float64: the same statements agree with the fp32 vectors to rounding, except where a branch comparison is a near-tie
        for i in range(int(c["n_cases"])):
            _, n64, a64, _ = P.reconstruct(t(f"c{i}_altitude").double(), t(f"c{i}_coef").double(), t(f"c{i}_intercept").double())
            d = (a64 - t(f"c{i}_pixels_angle").double()).abs()
            ok = (d <= 1e-4) | torch.isnan(d)
            assert float((~ok).double().mean()) <= 0.05, f"case {i}: {int((~ok).sum())} pixels"
    elif stage == "prior_built":
        for i in range(int(c["n_cases"])):
            tv, wv = P.apply_prior(t(f"c{i}_tsdf_before"), t(f"c{i}_weight_before"))
            assert bits(tv, c[f"c{i}_tsdf_after"]) and bits(wv, c[f"c{i}_weight_after"]), f"case {i}"
    elif stage == "surface_built":
        for i in range(int(c["n_cases"])):
            idx, z = P.surface(t(f"c{i}_tsdf"), t(f"c{i}_axis2"))
            assert torch.equal(idx, t(f"c{i}_indices")), f"case {i}: indices"
            cloud = P.surface_cloud([t(f"c{i}_axis0"), t(f"c{i}_axis1")], z, c[f"c{i}_center"])
            assert cloud.dtype == np.float64 and np.array_equal(cloud, c[f"c{i}_cloud"]), f"case {i}: cloud"
    else:  # the chain: the integrated volume (pinned by tests/test_tsdf_oracle.py) through the prior and the surface
        for v in range(int(c["n_views"])):
            _, _, _, wgt = P.reconstruct(t(f"v{v}_altitude"), t(f"v{v}_coef"), t(f"v{v}_intercept"))
            assert bits(wgt, c[f"v{v}_weights"]), f"view {v}: weights"
        tv, wv = P.apply_prior(t("tsdf_integrated"), t("weight_integrated"))
        assert bits(tv, c["tsdf_prior"]) and bits(wv, c["weight_prior"])
        idx, z = P.surface(tv, t("axis2"))
        assert torch.equal(idx, t("indices"))
        assert np.array_equal(P.surface_cloud([t("axis0"), t("axis1")], z, c["center"]), c["cloud"])


def test_surface_is_the_top_most_negative_voxel():
    """The reference's docstring says "first voxel with a TSDF value < 0"; its code takes the top-most one. Pinned on the
    vectors: every stored index is the largest z with t < 0 (0 if none)."""
    c = load("surface_built")
    for i in range(int(c["n_cases"])):
        neg = c[f"c{i}_tsdf"] < 0
        nz = neg.shape[-1]
        top = np.where(neg.any(-1), nz - 1 - np.argmax(neg[..., ::-1], axis=-1), 0)
        assert np.array_equal(top, c[f"c{i}_indices"])
        assert (neg.sum(-1) > 1).any()  # columns where first and top-most differ


def test_api_refuses_cpu_tensors():
    """eogs2_amd.tsdf's new stages run on the GPU only: CPU tensors raise before any library call."""
    from eogs2_amd import tsdf

    c = load("normals")
    meta = {"img": "v", "model": {"scale": 1.0, "coef_": c["c0_coef"].tolist(), "intercept_": c["c0_intercept"].tolist()}}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.RangeImage(meta, torch.as_tensor(c["c0_altitude"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.RangeImageEOGS(meta, c["c0_altitude"], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.normals(torch.as_tensor(c["c0_altitude"]), torch.as_tensor(c["c0_coef"]), torch.as_tensor(c["c0_intercept"]))
    vol = tsdf.TSDFVolume(np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 0.5]]), 0.1, 2.0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.apply_prior()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.surface()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.surface_cloud([np.zeros(3)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.surface(vol._tsdf_vol, vol.axes[2])
    assert torch.equal(vol._tsdf_vol, torch.ones_like(vol._tsdf_vol)) and float(vol._weight_vol.abs().max()) == 0.0
