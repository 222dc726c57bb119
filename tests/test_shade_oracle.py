"""CPU: the float64 restatement (oracle/shade_oracle.py) against the vectors the reference's own modules produced
(tests/golden/make_golden_shade.py): render pipeline, masked resample losses, translucent-shadow regulariser."""
import os

import numpy as np
import pytest
import torch

import shade_cases as sc
from oracle import shade_oracle as O
from shade_cases import close, expected_matrix_grad, fixtures, load, run_shade

TOL = 2e-5  # the vectors are fp32 results of the reference


@pytest.mark.parametrize("path", fixtures("cc_") + fixtures("exposure_") + fixtures("identity_"), ids=lambda p: p.split("shade_")[-1][:-4])
def test_render_pipeline_matches_reference_vectors(path):
    fx = load(path)
    got = run_shade(O.render_pipeline, fx, torch.float64, "cpu")
    for k in ("cc", "shaded", "g_raw"):
        close(got[k], fx[k], TOL, k)
    if "alt_diff" in fx:
        for k in ("shadow", "g_alt_diff", "g_inshadow"):
            close(got[k], fx[k], TOL, k)
    gM = expected_matrix_grad(fx)
    if gM is not None:
        close(got["g_M"], gM, TOL, "g_M")


def run_mloss(fn_sun, fn_random, fx, dtype, dev):
    t = lambda a: torch.tensor(a, dtype=dtype, device=dev)
    a, b = t(fx["rgb_a"]).requires_grad_(True), t(fx["rgb_b"]).requires_grad_(True)
    alt, uv, up = t(fx["alt_diff"]).requires_grad_(True), t(fx["uv"]), t(fx["upstream"])
    L = fn_sun(a, b, alt, uv) if str(fx["mode"]) == "sun" else fn_random(alt, a, b, uv)
    total = up[0] * L[0] + up[1] * L[1]
    if total.requires_grad:  # an empty mask gives constants: no path to any input
        total.backward()
    n = lambda x, like: (torch.zeros_like(like) if x is None else x).detach().double().cpu().numpy()  # None: no path = zero
    return dict(L_alt=float(L[0]), L_rgb=float(L[1]), g_alt_diff=n(alt.grad, alt), g_rgb_a=n(a.grad, a), g_rgb_b=n(b.grad, b))


def check_mloss(got, fx, tol):
    assert abs(got["L_alt"] - float(fx["L_alt"])) <= tol * max(abs(float(fx["L_alt"])), 1e-30) + 1e-30
    assert abs(got["L_rgb"] - float(fx["L_rgb"])) <= tol * max(abs(float(fx["L_rgb"])), 1e-30) + 1e-30
    for k in ("g_alt_diff", "g_rgb_a", "g_rgb_b"):
        if np.abs(fx[k]).max() == 0:
            assert np.abs(got[k]).max() == 0, k
        else:
            close(got[k], fx[k], tol, k)


@pytest.mark.parametrize("path", fixtures("mloss_"), ids=lambda p: p.split("shade_")[-1][:-4])
def test_masked_losses_match_reference_vectors(path):
    fx = load(path)
    check_mloss(run_mloss(O.suncamera_l, O.randomcam_l, fx, torch.float64, "cpu"), fx, TOL)


@pytest.mark.parametrize("path", fixtures("tshadow_"), ids=lambda p: p.split("shade_")[-1][:-4])
def test_translucent_shadows_matches_reference_vectors(path):
    fx = load(path)
    a = torch.tensor(fx["a"], dtype=torch.float64).requires_grad_(True)
    L = O.translucentshadows_l(a)
    (float(fx["upstream"]) * L).backward()
    assert abs(float(L) - float(fx["L"])) <= TOL * abs(float(fx["L"]))
    close(a.grad.numpy(), fx["g_a"], TOL, "g_a")


# ---- the edge cases of tests/shade_cases.py, as the reference's own modules ran them (shade_edge*.npz) ----


def pin(got, vec, tol, what, signed_zero=False):
    """The float64 oracle against an fp32 vector of the reference: NaN, +inf and -inf at the same elements, the finite ones
    within tol of the largest finite |vector| (the reference's own fp32 rounding; its autograd forms some gradients from
    other terms than the kernels do, so the kernels' per-element bounds do not apply to it), zeros with the same sign."""
    vec = np.asarray(vec, np.float64)
    fin = np.isfinite(vec)
    scale = max(float(np.abs(vec[fin]).max()) if fin.any() else 0.0, 1e-30)
    sc.check(got, vec, np.full(vec.shape, tol * scale), what, signed_zero=signed_zero)


def same_inputs(fx, case, what):
    for k, v in case.items():
        a, b = np.asarray(fx[k]), np.asarray(v)
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=(b.dtype.kind == "f")), f"{what}: {k}"


def test_libm_error_constants_cover_the_cpu_measurement():
    m = sc.measured_libm_ulp()
    assert m["exp"] <= sc.E_EXP and m["log2"] <= sc.E_LOG2, m


@pytest.mark.parametrize("kind,H,W,shadow,kw", sc.GOLDEN_PIPE, ids=lambda v: str(v))
def test_render_pipeline_edges_match_reference_vectors(kind, H, W, shadow, kw):
    tag = "_".join(f"{k}{int(v)}" for k, v in kw.items())
    fx = load(os.path.join(sc.GOLD, f"shade_edgepipe_{kind}_{'shadow' if shadow else 'noshadow'}_{H}x{W}_{tag}.npz"))
    same_inputs(fx, sc.pipeline_case(kind, H, W, shadow, **kw), "fixture inputs are the case's")
    got = run_shade(O.render_pipeline, fx, torch.float64, "cpu")
    vec = {k: fx[k] for k in got if k != "g_M"}
    gM = expected_matrix_grad(fx)
    if gM is not None:
        vec["g_M"] = gM
    for k, v in vec.items():
        pin(got[k], v, TOL, k, signed_zero=(k == "g_alt_diff"))
    if "alt_diff" in fx and np.isnan(fx["alt_diff"]).any():  # the reference keeps a NaN altitude difference; its own gradient is 0
        p = np.isnan(fx["alt_diff"])
        assert np.isnan(fx["shadow"][p]).all() and np.isnan(fx["shaded"][:, p]).all() and (fx["g_alt_diff"][p] == 0).all()
        assert np.isnan(fx["g_inshadow"]).all() and np.isnan(fx["g_raw"][:, p]).all()


@pytest.mark.parametrize("name,mode", [c for c in sc.mloss_case_list() if c[0] != "full513"], ids=lambda v: str(v))
def test_masked_loss_edges_match_reference_vectors(name, mode):
    """Also the stated deviation: with a non-finite value at a masked-out pixel the reference's loss is NaN
    (`NaN * 0` in its masked sum) with finite gradients; on the same inputs with those values zeroed it is finite, and that
    is what the kernels return (tests/test_gpu_shade_edges.py)."""
    fx = load(os.path.join(sc.GOLD, f"shade_edgemloss_{name}_{mode}.npz"))
    case = sc.mloss_case(name, mode)
    same_inputs(fx, case, "fixture inputs are the case's")
    got = run_mloss(O.suncamera_l, O.randomcam_l, fx, torch.float64, "cpu")
    for k in ("L_alt", "L_rgb"):
        pin(np.float64(got[k]), np.float64(fx[k]), TOL, k)
    for k in ("g_alt_diff", "g_rgb_a", "g_rgb_b"):
        pin(got[k], fx[k], 2.0 ** -23, k, signed_zero=True)
        assert np.isfinite(fx[k]).all(), k
    zeroed = run_mloss(O.suncamera_l, O.randomcam_l, sc.masked_out_zeroed(case), torch.float64, "cpu")
    if name == "nonfinite_out":
        assert np.isnan(float(fx["L_alt"])) and np.isnan(float(fx["L_rgb"])) and np.isnan(got["L_alt"]) and np.isnan(got["L_rgb"])
        assert np.isfinite(zeroed["L_alt"]) and np.isfinite(zeroed["L_rgb"])
        for k in ("g_alt_diff", "g_rgb_a", "g_rgb_b"):
            assert np.array_equal(zeroed[k], got[k]), k  # a zeroed -inf or NaN changes no more than the sign of a zero
    else:  # nothing to zero: a non-finite value inside the mask reaches the loss in both
        for k in got:
            assert np.array_equal(zeroed[k], got[k], equal_nan=True), k
    if name in ("alt_inf_in", "rgb_nan_in", "rgb_inf_in"):
        assert not np.isfinite(float(fx["L_alt" if name == "alt_inf_in" else "L_rgb"]))


@pytest.mark.parametrize("name", [n for n in sc.TSHADOW_CASES if n != "big"])
def test_translucent_shadow_edges_match_reference_vectors(name):
    fx = load(os.path.join(sc.GOLD, f"shade_edgetshadow_{name}.npz"))
    case = sc.tshadow_case(name)
    same_inputs(fx, case, "fixture inputs are the case's")
    got = sc.run_tshadow(O.translucentshadows_l, case, torch.float64, "cpu")
    pin(np.float64(got["L"]), np.float64(fx["L"]), TOL, "L")
    pin(got["g_a"], fx["g_a"], TOL, "g_a")
    if name == "nan":  # the reference's gradient at a NaN is NaN
        assert np.isnan(fx["g_a"][np.isnan(fx["a"])]).all() and np.isnan(float(fx["L"]))
