"""GPU (MI355X): `eogs2_amd.render.render` — the HIP raw-parameter path — against the REFERENCE's own
render() (tests/golden/render/*.npz, tests/golden/make_golden_render.py), through the full parity bar: radii and
visibility_filter exact; the image and every raw-parameter gradient through parity_cases.compare (column check, support check,
per-Gaussian pass), with attribution re-running the oracle's RAW mode on the same inputs; the camera gradient (whole view matrix
and last_row) by the magnitude-sum rule. The CPU counterpart (the oracle's RAW mode, util.render_unfused) is
tests/test_render_golden.py."""
import pytest
import torch

from parity_cases import compare
from util import RENDER, load_render, run_render_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", RENDER)
def test_hip_render_matches_reference_render(dev, name):
    case, expected = load_render(name)
    got = run_render_case(case, dev)
    assert torch.equal(got["_visibility_filter"].cpu(), torch.from_numpy(expected["_visibility_filter"])), f"{name}: visibility_filter"
    if "_g_last_row" in expected:
        assert torch.equal(got["_g_last_row"], got["g_viewmatrix"][3]), f"{name}: last_row"
    compare(got, expected, f"hip_render:{name}", case, ref_is_oracle=False)
