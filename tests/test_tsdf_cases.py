"""CPU: the cases of tests/tsdf_cases.py checked on the restatement alone. The fp32 run of oracle/tsdf_oracle.py against its
float64 run stays inside the attributed criterion and its cap on every case (so the criterion asks nothing of the kernel
that the reference's own arithmetic does not meet), and the lattice cases are exact and hold the situations they name."""
import glob
import os

import numpy as np
import pytest
import torch

import tsdf_cases as tc
from util import GOLDEN_DIR

EXISTING = [(48, 64, [[-1.4, 1.4], [-1.3, 1.3], [-0.3, 0.4]], 0.06), (33, 17, [[-0.5, 0.5], [-0.5, 0.5], [-0.2, 0.3]], 0.031),
            (64, 64, [[-4.0, -3.5], [-0.2, 0.2], [0.0, 0.1]], 0.05)]


def _fp32_inside_the_cap(axes, views, scale, trunc, what):
    ref = tc.reference(axes, views, scale, trunc)
    for a, b, k in ((ref["t32"], ref["t64"], "tsdf"), (ref["w32"], ref["w64"], "weights")):
        tc.assert_attributed(a, b, 2e-4, ref, f"{what}: fp32 restatement against float64, {k}")
    assert all(0 <= d < 1e-4 and 0 <= dv < 1e-4 for d, dv in ref["margins"]), ref["margins"]


@pytest.mark.parametrize("name", list(tc.SHAPES))
def test_fp32_restatement_stays_inside_the_cap(name):
    axes, views = tc.shape_case(name)
    _fp32_inside_the_cap(axes, views, tc.SCALE, tc.TRUNC, name)


@pytest.mark.parametrize("H,W,bounds,vox", EXISTING)
def test_fp32_restatement_stays_inside_the_cap_on_the_volume_cases(H, W, bounds, vox):
    from eogs2_amd.tsdf import volume_axes

    _, axes = volume_axes(np.array(bounds), vox, torch.device("cpu"))
    _fp32_inside_the_cap(axes, [tc.scene(H, W, seed) for seed in (1, 2, 3)], 1.7, 3.0 * vox, f"{H}x{W}")


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN_DIR, "tsdf_*.npz"))), ids=lambda p: os.path.basename(p)[5:-4])
def test_fp32_restatement_stays_inside_the_cap_on_the_reference_vector_cases(path):
    """The cases tests/test_gpu_tsdf.py::test_integrate_matches_reference_vectors holds to the attributed check, after every view."""
    z = np.load(path)
    axes = [torch.as_tensor(z[f"axis{i}"]) for i in range(3)]
    views = [tuple(torch.as_tensor(z[f"v{v}_{k}"]) for k in ("coef", "intercept", "altitude", "weights")) for v in range(int(z["n_views"]))]
    for v in range(len(views)):
        _fp32_inside_the_cap(axes, views[: v + 1], float(z["model_scale"]), float(z["trunc_margin"]), f"{os.path.basename(path)} view {v}")


def test_a_nan_that_moves_is_never_attributed():
    axes, views = tc.shape_case("nz_65")
    ref = tc.reference(axes, views, tc.SCALE, tc.TRUNC)
    t = ref["t32"].clone()
    t[tuple(torch.nonzero(~torch.isnan(t))[0])] = float("nan")
    ref["near"][:] = True  # even at a decision
    with pytest.raises(AssertionError, match="NaN pattern differs"):
        tc.assert_attributed(t, ref["t64"], 2e-4, ref, "moved NaN")


def test_one_corrupted_voxel_is_not_attributed():
    """What the old share accepted: a wrong interior voxel away from every decision."""
    axes, views = tc.shape_case("nz_65")
    ref = tc.reference(axes, views, tc.SCALE, tc.TRUNC)
    free = torch.nonzero(~ref["near"] & ~torch.isnan(ref["t64"]))
    assert free.numel()
    t = ref["t32"].clone()
    t[tuple(free[len(free) // 2])] += 0.5
    with pytest.raises(AssertionError, match="away from every decision"):
        tc.assert_attributed(t, ref["t64"], 2e-4, ref, "corrupted")


@pytest.mark.parametrize("scale", tc.LATTICE_SCALES)
def test_lattice_case_is_exact_and_holds_its_situations(scale):
    axes, views, t0, w0 = tc.lattice_case(scale)
    ref = tc.reference(axes, views, scale, tc.LATTICE_TRUNC, t0, w0)
    for k in ("t", "w"):  # nothing rounds: float64 holds fp32 values and the fp32 sequence gives the same bits
        a64, a32 = ref[k + "64"], ref[k + "32"]
        assert torch.equal(tc.bits(a64.float()), tc.bits(a32)), k
        fin = ~torch.isnan(a64)
        assert torch.equal(a64.float().double()[fin], a64[fin]), k
    uv, sdf, upd = tc.lattice_facts(axes, views[0], scale)
    T = tc.LATTICE_TRUNC
    on_edge = ((uv.abs() == 1.0).any(1)) & (uv.abs() <= 1.0).all(1)
    assert int((on_edge & upd).sum()) > 0  # |u| = 1 or |v| = 1 exactly: valid
    for comp in (0, 1):
        for sign in (1.0, -1.0):
            assert int((uv[:, comp] == sign).sum()) > 0 and int((uv[:, comp] == sign * 1.125).sum()) > 0  # and one step outside
    inside = (uv.abs() <= 1.0).all(1)
    assert int((inside & (sdf == -T)).sum()) > 0 and int((inside & (sdf == -T) & ~upd).sum()) == 0  # included, t = -1
    step = scale / 16.0
    assert int((inside & (sdf == -T - step)).sum()) > 0 and int((inside & (sdf == -T - step) & upd).sum()) == 0  # one step below
    assert int((inside & (sdf == 0)).sum()) > 0 and int((inside & (sdf >= T)).sum()) > 0
    t64 = ref["t64"].reshape(-1)
    first = tc.reference(axes, views[:1], scale, T, t0, w0)["t64"].reshape(-1)
    assert bool((first[inside & (sdf == -T)] == -1.0).all()) and bool((first[inside & (sdf == 0)] == 0.0).all())
    assert bool((first[inside & (sdf >= T)] == 1.0).all())
    assert torch.equal(tc.bits(t64.float())[~inside], tc.bits(t0.reshape(-1))[~inside])  # untouched: NaN and -0 keep their bits
    one_out = ~inside & (uv.abs() <= 1.125).all(1)  # one lattice step outside: pre-filled with both
    pre = t0.reshape(-1)[one_out]
    assert int(torch.isnan(pre).sum()) > 0 and int((tc.bits(pre) == tc.bits(torch.tensor(-0.0))).sum()) > 0


@pytest.mark.parametrize("plant", tc.PLANTS, ids=lambda p: f"{p[0]}_{p[1]}")
def test_planted_pixel_reaches_voxels_in_the_restatement(plant):
    """The planted pixel changes some voxels of the fp32 restatement and only voxels under it."""
    axes, views, t0, w0 = tc.lattice_case(1.0, plant)
    plain = tc.lattice_case(1.0)
    a = tc.reference(axes, views, 1.0, tc.LATTICE_TRUNC, t0, w0)
    b = tc.reference(plain[0], plain[1], 1.0, tc.LATTICE_TRUNC, t0, w0)
    changed = (tc.bits(a["t32"]) != tc.bits(b["t32"])) | (tc.bits(a["w32"]) != tc.bits(b["w32"]))
    # the pixel is a tap (a NaN or an infinity even at weight 0) of the voxels with fx in [4, 6) and fy in [3, 5): 4 x 4 columns
    assert 0 < int(changed.sum()) <= 16 * 17
