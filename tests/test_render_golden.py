"""CPU: the raw-parameter front end against vectors from the REFERENCE's own `render()`
(tests/golden/make_golden_render.py: gaussian_renderer/renderer.py and scene/gaussian_model.py executed unmodified, the
rasterizer below the reference's wrapper being the oracle over activated inputs).

Pinned here: the oracle's RAW mode (its C restatement of the activations and their backward, reached through
`eogs2_amd.render.render` over the oracle library) and `util.render_unfused` (the PyTorch ops the other raw-path tests compare
with). Both through the full parity bar (parity_cases.compare): per-column, support and per-Gaussian checks. The GPU
counterpart is tests/test_gpu_render_golden.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from parity_cases import compare
from util import RENDER, RENDER_DIR, load_render, run_render_case

GEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_render.py")
CASES = ("aa_learn_61x83", "noaa_fixed_47x70", "modifier0p7_55x38", "affine_tilted_50x66", "offscreen_45x77", "edges_41x53",
         "subeps_29x23")


def test_fixtures_present():
    assert RENDER == sorted(CASES)
    for n in RENDER:
        assert os.path.getsize(os.path.join(RENDER_DIR, n + ".npz")) < 400 * 1024


def test_fixtures_cover_the_edges():
    """What each case is there for is in its inputs: both antialiasing settings, a learned and a fixed last row, a scale
    modifier, an altitude axis apart from the view matrix, culled Gaussians, and the edge rows."""
    cases = {n: load_render(n) for n in RENDER}
    assert {bool(c["antialiasing"]) for c, _ in cases.values()} == {False, True}
    assert {bool(c["learn_wv_only_lastparam"]) for c, _ in cases.values()} == {False, True}
    assert any(float(c["scaling_modifier"]) == np.float32(0.7) for c, _ in cases.values())
    c, _ = cases["affine_tilted_50x66"]
    assert np.abs(c["affine"][:3, 2] - c["viewmatrix"][:3, 2]).max() > 0.01
    c, e = cases["offscreen_45x77"]
    assert (e["out_radii"] == 0).sum() > 0 and (e["out_radii"] > 0).sum() > 0
    assert all(not (H % 8 == 0 or W % 8 == 0) for H, W in ((int(c["H"]), int(c["W"])) for c, _ in cases.values()))
    c, e = cases["edges_41x53"]
    logit, n = c["opacity_logit"].ravel(), np.linalg.norm(c["raw_rotation"].astype(np.float64), axis=1)
    assert logit.max() >= 20 and logit.min() <= -90
    assert c["log_scaling"].max() - np.median(c["log_scaling"]) > 2.5 and np.median(c["log_scaling"]) - c["log_scaling"].min() > 6
    assert n.min() < 1e-3 and n.max() >= 1e3 and ((n > 5e-4) & (n < 2e-3)).any() and (c["raw_rotation"][:, 0] < 0).any()
    c, e = cases["subeps_29x23"]
    n = np.linalg.norm(c["raw_rotation"].astype(np.float64), axis=1)
    assert (n < 1e-12).sum() == 4 and (c["raw_rotation"][n < 1e-12, 0] < 0).any()
    assert (e["out_radii"][n < 1e-12] > 0).all()  # (the sub-eps rows are drawn: their gradient is not zero)
    assert (np.abs(e["g_raw_rotation"][n < 1e-12]).max(axis=1) > 0).all()
    for c, e in cases.values():
        if bool(c["learn_wv_only_lastparam"]):
            assert np.array_equal(e["_g_last_row"], e["g_viewmatrix"][3]) and np.abs(e["_g_last_row"]).max() > 0


def test_fixtures_regenerate_bit_for_bit(tmp_path):
    """The generator, run again, writes the committed arrays bit for bit (where the reference's sources are present)."""
    sys.path.insert(0, os.path.dirname(GEN))
    try:
        import make_golden_render as gen
    finally:
        sys.path.remove(os.path.dirname(GEN))
    if not os.path.isdir(gen.REFROOT):
        pytest.skip("the reference's sources are not on this machine")
    subprocess.run([sys.executable, GEN, "--out", str(tmp_path)], check=True, timeout=600)
    for n in RENDER:
        a, b = np.load(os.path.join(RENDER_DIR, n + ".npz")), np.load(tmp_path / (n + ".npz"))
        assert sorted(a.files) == sorted(b.files), n
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{n}:{k}"


def _check(got, expected, case, name):
    assert torch.equal(got["_visibility_filter"], torch.from_numpy(expected["_visibility_filter"])), f"{name}: visibility_filter"
    if "_g_last_row" in expected:
        assert torch.equal(got["_g_last_row"], got["g_viewmatrix"][3]), f"{name}: last_row"
    compare(got, expected, name, case, ref_is_oracle=False)


@pytest.mark.parametrize("name", RENDER)
def test_oracle_raw_mode_matches_reference_render(oracle_backend, name):
    """`eogs2_amd.render.render` over the oracle library (its RAW mode) == the reference's render()."""
    case, expected = load_render(name)
    _check(run_render_case(case, torch.device("cpu")), expected, case, f"oracle_raw:{name}")


@pytest.mark.parametrize("name", RENDER)
def test_render_unfused_matches_reference_render(oracle_backend, name):
    """util.render_unfused (the PyTorch activations + the drop-in rasterizer over the oracle) == the reference's render()."""
    case, expected = load_render(name)
    _check(run_render_case(case, torch.device("cpu"), fused=False), expected, case, f"unfused:{name}")
