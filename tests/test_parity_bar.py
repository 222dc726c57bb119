"""CPU: the parity bar itself (tests/parity_cases.py compare) against errors planted into the oracle's own output, and against the
valid fp32 evaluations it must keep accepting. Every render and backward kernel is judged by compare; these tests say what it can
see. Planted errors must raise AssertionError; the negative controls (the oracle, its FMA build, its fp32-summing mode, the oracle
on inputs perturbed by a few ulp) must pass.

Cases: seeded row 12 (long lists, early termination: the 64 / 32 / 14 Gaussians whose largest gradient entry is below 1e-3 /
3e-4 / 1e-4 of its column's scale are what a per-column scale could not see), the dense_termination golden, an antialiased
seeded row with an inverse-depth gradient, and sweep seed 4249 (ill-conditioned covariance backward: the arbiter decides)."""
import ctypes

import numpy as np
import pytest
import torch

from parity_cases import (ARB_ABS, ARB_FACTOR, PAIR_NOISE_DRAWS, SENS_ULPS, ULP, VIEW_ABS, arbiter, compare, fp32_variants, gaussian_grad_keys,
                          oracle_run, perturbed, quantity_scale, row_magnitude, seeded_case, sweep_case)
from util import load_golden, load_render

CASES = {
    "seed12": lambda: seeded_case(3000, 64, 64, 12, 0.7, 8.0, False, False)[0],
    "dense_termination": lambda: {k: v for k, v in load_golden("dense_termination").items() if not k.startswith(("out_", "g_"))},
    "seed11_aa_depth": lambda: seeded_case(5000, 160, 208, 11, "trained", 2.0, True, True)[0],
    "sweep4249": lambda: sweep_case(4249)[0],
    # raw-parameter cases (the inputs of tests/golden/render/*.npz through eogs2_amd.render.render over the oracle's RAW mode)
    "raw_aa_learn": lambda: load_render("aa_learn_61x83")[0],
    "raw_edges": lambda: load_render("edges_41x53")[0],
}
_STATE = {}


def _case(name):
    if name not in _STATE:
        case = CASES[name]()
        _STATE[name] = (case, oracle_run(case))
    return _STATE[name]


@pytest.fixture(scope="module")
def cache_dir(tmp_path_factory):
    """File prefix per case for the arbiter's arrays (they depend on the case alone: computed once per module)."""
    d = tmp_path_factory.mktemp("bar_cache")
    return lambda name: str(d / name)


def _as_out(ref):
    return {k: torch.from_numpy(np.array(v, copy=True)) for k, v in ref.items()}


def _rows(ref, case, below):
    P = case["means3D"].shape[0]
    rel = row_magnitude(ref, P).numpy()
    return (rel > 0) & (rel < below)


def _rejects(out, ref, name, case, cache):
    with pytest.raises(AssertionError) as e:
        compare(out, ref, name, case, cache=cache)
    return str(e.value)


# ---- planted errors: every gradient column of the rows whose largest entry is below `below` of its column's scale -------------
# (rows, factor, expected row count on seed 12): the first four passed the column-scale bar before the per-Gaussian pass and the
# support check existed, the last one did not
ROW_ERRORS = [(1e-3, 1.1, 64), (1e-3, 1.05, 64), (1e-4, 0.0, 14), (1e-4, 2.0, 14), (3e-4, 0.0, 32)]


@pytest.mark.parametrize("below,factor,nrows", ROW_ERRORS, ids=[f"{b:g}x{f:g}" for b, f, _ in ROW_ERRORS])
def test_small_rows_wrong_are_rejected(cache_dir, below, factor, nrows):
    case, ref = _case("seed12")
    sel = _rows(ref, case, below)
    assert int(sel.sum()) == nrows  # (the case the table was measured on)
    out = _as_out(ref)
    for k in gaussian_grad_keys(ref, case["means3D"].shape[0]):
        out[k][torch.from_numpy(sel)] *= factor
    msg = _rejects(out, ref, "seed12", case, cache_dir("seed12"))
    if below < 3e-4:  # (the rows the column check cannot see: rejected by the support check or the per-Gaussian pass)
        assert ("gradient support" in msg) if factor == 0.0 else (":row" in msg), msg


@pytest.mark.parametrize("name", ["dense_termination", "seed11_aa_depth"])
def test_small_rows_wrong_are_rejected_other_cases(cache_dir, name):
    case, ref = _case(name)
    P = case["means3D"].shape[0]
    for below, factor in ((1e-3, 1.05), (3e-4, 0.0)):
        sel = _rows(ref, case, below)
        assert sel.any()
        out = _as_out(ref)
        for k in gaussian_grad_keys(ref, P):
            out[k][torch.from_numpy(sel)] *= factor
        _rejects(out, ref, name, case, cache_dir(name))


def _nudged_thresholds(case, sign, k4):
    """The oracle with its blend / stop thresholds moved uniformly by `sign` x k4's margins (rast_oracle.c
    eogs_oracle_threshold_nudge: alpha_min = (1/255)(1 + s (k0 + k1 M) 2^-23), T_min = 1e-4 (1 + s (k2 + k3 n) 2^-23))."""
    import oracle

    lib = oracle.abi().cdll
    lib.eogs_oracle_threshold_nudge.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    k = (ctypes.c_float * 4)(*k4)
    lib.eogs_oracle_threshold_nudge(sign, None, 0, ctypes.cast(k, ctypes.c_void_p))
    try:
        return oracle_run(case)
    finally:  # the margins are process-global, and Attribution's own nudged runs pass none: restore them
        d = (ctypes.c_float * 4)(16.0, 8.0, 16.0, 4.0)
        lib.eogs_oracle_threshold_nudge(0, None, 0, ctypes.cast(d, ctypes.c_void_p))


@pytest.mark.parametrize("name", ["seed12", "dense_termination"])
@pytest.mark.parametrize("what,sign,k4", [
    ("stop at 0.95e-4", -1, (0.0, 0.0, 0.05 / ULP, 0.0)),
    ("stop at 1.05e-4", 1, (0.0, 0.0, 0.05 / ULP, 0.0)),
    ("blend threshold +1 %", 1, (0.01 / ULP, 0.0, 0.0, 0.0)),
])
def test_moved_thresholds_are_rejected(cache_dir, name, what, sign, k4):
    case, ref = _case(name)
    moved = _nudged_thresholds(case, sign, k4)
    assert any(not np.array_equal(moved[k], ref[k]) for k in ref), f"{what}: no output moved"
    _rejects(_as_out(moved), ref, name, case, cache_dir(name))
    # (and the margins are back: a plain nudged run equals the default one)
    assert np.array_equal(oracle_run(case)["out_color"], ref["out_color"])


def test_arbiter_has_an_absolute_bound(cache_dir):
    """0.2 of the column's scale on the worst-conditioned Gaussian (the largest spread of the valid fp32 evaluations around the
    float64 arbiter) is rejected even where ARB_FACTOR x that spread would cover it."""
    case, ref = _case("sweep4249")
    f64, spread, _, same = arbiter(case, ref)
    P = case["means3D"].shape[0]
    key, row, worst = None, None, -1.0
    for k in gaussian_grad_keys(ref, P):
        s = (spread[k] / quantity_scale(ref[k]).numpy()).reshape(P, -1).max(axis=1)
        if s.max() > worst:
            key, row, worst = k, int(s.argmax()), float(s.max())
    # (0.2 lies within ARB_FACTOR x the spread there, and beyond the absolute bound: the same-input evaluations sit closer than 0.1)
    assert ARB_ABS < 0.2 < ARB_FACTOR * worst
    assert float((same[key][row] / quantity_scale(ref[key]).numpy()[0]).max()) < ARB_ABS
    out = _as_out(ref)
    col = quantity_scale(ref[key]).numpy()[0]
    away = np.where(ref[key][row] >= f64[key][row], 1.0, -1.0)  # away from f64: |HIP - f64| >= 0.2 of the scale
    out[key][row] += torch.from_numpy((0.2 * col * away).astype(np.float32))
    msg = _rejects(out, ref, "sweep4249", case, cache_dir("sweep4249"))
    assert key in msg, msg


def test_camera_gradient_has_an_absolute_bound(cache_dir):
    case, ref = _case("sweep4249")
    g2 = np.abs(ref["g_means2D"]).astype(np.float64)
    m3 = np.abs(case["means3D"]).astype(np.float64)
    msum = max(float((m3.T @ g2).max()), float(g2.sum(0).max()), float(np.abs(ref["g_viewmatrix"]).max()))
    out = _as_out(ref)
    out["g_viewmatrix"][0, 0] += 2.0 * VIEW_ABS * msum
    msg = _rejects(out, ref, "sweep4249", case, cache_dir("sweep4249"))
    assert "g_viewmatrix" in msg, msg


# ---- negative controls: valid fp32 evaluations of the reference's algorithm pass -------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_valid_fp32_evaluations_pass(cache_dir, name):
    import oracle

    case, ref = _case(name)
    compare(_as_out(ref), ref, name, case, cache=cache_dir(name))  # the oracle's own output
    variants = {k: v for k, v in fp32_variants(case).items() if k in ("fp32 sums", "fma")}
    assert "fp32 sums" in variants
    if oracle.abi_fma() is None:
        print("no FMA on this host: the FMA build is not compared")
    for label, res in variants.items():
        compare(_as_out(res), ref, f"{name} ({label})", case, cache=cache_dir(name))
    assert PAIR_NOISE_DRAWS >= 1


# (sweep 4249's covariance backward is ill-conditioned: 4 ulp on its Gaussians' parameters move g_rotations by 6 % of its scale on
# 68 elements — the column check without the row pass rejects that too; arbiter() counts only evaluations of the SAME inputs. There
# the upstream gradient alone is perturbed: what the rounding of every pixel's term of a cancelling per-Gaussian sum does.)
GAUSSIAN_INPUTS = ("means3D", "scales", "rotations", "opacities", "colors", "cov3D_precomp")
RAW_INPUTS = ("means3D", "f_dc", "opacity_logit", "log_scaling", "raw_rotation")
UPSTREAM = ("dL_dcolor", "dL_dinvdepth")


@pytest.mark.parametrize("name,keys", [("seed12", GAUSSIAN_INPUTS + UPSTREAM), ("dense_termination", GAUSSIAN_INPUTS + UPSTREAM),
                                       ("seed11_aa_depth", GAUSSIAN_INPUTS + UPSTREAM), ("sweep4249", UPSTREAM),
                                       ("raw_aa_learn", RAW_INPUTS + UPSTREAM), ("raw_edges", RAW_INPUTS + UPSTREAM)],
                         ids=lambda v: v if isinstance(v, str) else len(v))
def test_oracle_on_perturbed_inputs_passes(cache_dir, name, keys):
    """The oracle on inputs moved by SENS_ULPS ulp, drawn as arbiter() draws them (an fp32 evaluation is the exact result for
    inputs perturbed by a few ulp)."""
    case, ref = _case(name)
    res = oracle_run(perturbed(case, keys, np.random.default_rng(1000)))
    assert np.array_equal(res["out_radii"], ref["out_radii"])
    compare(_as_out(res), ref, f"{name} (inputs +-{SENS_ULPS:g} ulp)", case, cache=cache_dir(name))


# ---- the raw-parameter path: its own gradient columns, planted into the oracle's RAW output -----------------
# Rows whose largest entry is below 1e-4 of the column scales, restricted to those where the planted column carries at least 5 % of the
# row's largest entry: every factor moves an element by at least 5e-5 of the row scale ... and by less than 1e-4 of its column's scale,
# so only the per-Gaussian pass (":row") sees it. Before that pass the raw path was judged by util.assert_close alone.
RAW_ROW_ERRORS = [(k, f) for k in ("g_log_scaling", "g_raw_rotation", "g_opacity_logit") for f in (1.05, 2.0, 0.0)]


@pytest.mark.parametrize("key,factor", RAW_ROW_ERRORS, ids=[f"{k}x{f:g}" for k, f in RAW_ROW_ERRORS])
def test_small_raw_rows_wrong_are_rejected(cache_dir, key, factor):
    case, ref = _case("raw_aa_learn")
    P = case["means3D"].shape[0]
    rel = row_magnitude(ref, P).numpy()
    own = (np.abs(ref[key]).reshape(P, -1) / quantity_scale(ref[key]).numpy().reshape(1, -1)).max(axis=1)
    sel = (rel > 0) & (rel < 1e-4) & (own >= 0.05 * rel)
    assert int(sel.sum()) >= 100
    out = _as_out(ref)
    out[key][torch.from_numpy(sel)] *= factor
    msg = _rejects(out, ref, "raw_aa_learn", case, cache_dir("raw_aa_learn"))
    assert f"{key}:row" in msg or "gradient support" in msg, msg


def _activated_rotation_grad(case):
    """dL/d(normalised quaternion) of a render case: the oracle on the activated inputs (what the reference's rasterizer sees)."""
    t = lambda k: torch.from_numpy(np.asarray(case[k], dtype=np.float32))
    xyz, A = t("means3D"), t("affine")
    alt = (xyz @ A[:3, 2] + A[3, 2])[:, None]
    vm = t("viewmatrix").clone()
    if bool(case["learn_wv_only_lastparam"]):
        vm[3] += t("last_row")
    act = dict(means3D=xyz, scales=torch.exp(t("log_scaling")), rotations=torch.nn.functional.normalize(t("raw_rotation")),
               opacities=torch.sigmoid(t("opacity_logit")),
               colors=torch.cat([t("f_dc").squeeze(1) * 0.28209479177387814 + 0.5, alt, torch.ones_like(alt)], 1), viewmatrix=vm)
    act = {k: v.contiguous().numpy() for k, v in act.items()}
    act.update(bg=case["bg"], dL_dcolor=case["dL_dcolor"], H=case["H"], W=case["W"], antialiasing=case["antialiasing"],
               scale_modifier=case["scaling_modifier"])
    return oracle_run(act)["g_rotations"].astype(np.float64)


def test_dropped_normalize_projection_is_rejected(cache_dir):
    """On the edges case's quaternions of norm 3e-4 to 3e3 (rows 9-14, make_golden_render.EDGE_QUAT_NORM): dL/dq / |q| without the
    projection (dL/dq - q^ (q^ . dL/dq)) / |q| that F.normalize's backward applies."""
    case, ref = _case("raw_edges")
    dq = _activated_rotation_grad(case)
    r = np.asarray(case["raw_rotation"], dtype=np.float64)
    n = np.linalg.norm(r, axis=1, keepdims=True)
    rows = np.arange(9, 15)
    assert np.all(np.abs(np.log10(n[rows, 0])) > 2.9)
    qh = r / n
    proj = (dq - qh * (qh * dq).sum(1, keepdims=True)) / n
    # (the oracle's RAW gradient is the projected one on those rows)
    assert np.allclose(ref["g_raw_rotation"][rows], proj[rows], rtol=1e-3, atol=1e-3 * np.abs(proj[rows]).max())
    out = _as_out(ref)
    out["g_raw_rotation"][torch.from_numpy(rows)] = torch.from_numpy((dq / n)[rows].astype(np.float32))
    msg = _rejects(out, ref, "raw_edges", case, cache_dir("raw_edges"))
    assert "g_raw_rotation" in msg, msg
