"""CPU: the vectorised restatement of the reference's DSM registration and scoring (tests/dsm_eval_cases.py) pinned to the
vectors the reference's own eval/dsmr.py and eval/eval_dsm.py produced (tests/golden/dsm_eval/,
tests/golden/make_golden_dsm_eval.py): downsample2x and apply_shift bit for bit, (dx, dy) equal at every pyramid level,
NCC tables / moments / a / b / MAE within the bound derived from the pixel count (dsm_eval_cases.eps)."""
import numpy as np
import pytest

import dsm_eval_cases as C

from dsm_eval_cases import REGISTRATION, check_ab, check_mae, check_moments, load, same_bits


def test_fixtures_satisfy_the_gap_condition():
    for name in REGISTRATION:
        z = load(name)
        assert z["gaps"].min() >= 1e-6, name
        for t, w, c in zip(z["levels_table"], z["levels_winner"], z["levels_centre"]):
            assert C.argmax_scan(t, int(z["irange"]), int(c[0]), int(c[1])) == (int(w[0]), int(w[1]))


def test_downsample_is_bit_exact():
    z = load("downsample")
    for k in z:
        if k.startswith("in_"):
            assert same_bits(C.downsample2x(z[k]), z["out_" + k[3:]]), k


def test_apply_shift_is_bit_exact():
    z = load("apply_shift")
    for tag in ("float32", "float64"):
        for k, (dx, dy, a, b, c, d) in enumerate(z["coefs"]):
            got = C.apply_shift(z[f"in_{tag}"], int(dx), int(dy), a, b, c, d)
            assert same_bits(got, z[f"out_{tag}_{k}"]), (tag, k)


@pytest.mark.parametrize("name", REGISTRATION)
def test_registration(name):
    z = load(name)
    u, v = C.rebuild(z)
    shapes = C.level_shapes(*u.shape, *v.shape)[::-1]  # coarsest first, as recorded
    assert [tuple(s) for s in z["levels_shape_u"]] == [s[0] for s in shapes]
    assert [tuple(s) for s in z["levels_shape_v"]] == [s[1] for s in shapes]
    rec = []
    dx, dy, a, b = C.compute_shift(u, v, scaling=True, record=rec)
    assert len(rec) == len(z["levels_table"])
    for lv, t, c, w in zip(rec, z["levels_table"], z["levels_centre"], z["levels_winner"]):
        n = lv["shape_u"][0] * lv["shape_u"][1]
        assert lv["centre"] == (int(c[0]), int(c[1])) and lv["winner"] == (int(w[0]), int(w[1]))
        assert np.array_equal(np.isnan(lv["table"]), np.isnan(t))
        err = np.nanmax(np.abs(lv["table"] - t))
        print(f"{name} level {lv['shape_u']}: max NCC error {err:.3e} (eps {C.eps(n):.3e})")
        assert err <= C.eps(n)
    assert (dx, dy) == tuple(int(t) for t in z["shift"])
    if name != "sec_larger":
        assert (dx, dy) == tuple(int(t) for t in z["true_shift"])
    _, *m = C.mean_std(u, v, dx, dy)
    check_moments(m, z, u.size, name)
    check_ab(a, b, z, "ab_scaling", u.size, name)
    _, _, a0, b0 = C.compute_shift(u, v, scaling=False)
    assert a0 == 1 and float(z["ab_noscale"][0]) == 1.0
    assert abs(b0 - float(z["ab_noscale"][1])) <= C.eps(u.size) * (abs(m[0]) + abs(m[1]))


def test_mae_plain():
    z = load("mae_plain")
    diff, pred_r, tr = C.dsm_pointwise_diff(z["pred"], z["gt"])
    assert tr[:3] == (int(z["transform"][0]), int(z["transform"][1]), 1)
    assert diff.dtype == z["diff"].dtype and diff.shape == z["diff"].shape == z["gt"].shape
    assert np.array_equal(np.isnan(diff), np.isnan(z["diff"])) and np.array_equal(np.isnan(pred_r), np.isnan(z["pred_r"]))
    tol = C.diff_tol(z["gt"], z["pred"], z["pred_r"])
    assert np.nanmax(np.abs(pred_r.astype(np.float64) - z["pred_r"])) <= tol
    assert np.nanmax(np.abs(diff.astype(np.float64) - z["diff"])) <= tol
    check_mae(C.mae_of(diff), z["mae"], z["diff"], z["gt"].size, "mae_plain")


def test_mae_gt_nan():
    z = load("mae_gt_nan")
    diff, pred_r, _ = C.dsm_pointwise_diff(z["pred"], z["gt"])
    assert np.isnan(diff).all() and np.isnan(z["diff"]).all() and np.isnan(pred_r).all() and np.isnan(z["pred_r"]).all()
    with pytest.raises(ValueError):
        C.mae_of(diff)
    diff, pred_r, _ = C.dsm_pointwise_diff(z["pred"], z["gt"], clip="finite")
    assert np.array_equal(np.isnan(diff), np.isnan(z["ours_finite_diff"]))
    check_mae(C.mae_of(diff), z["ours_finite_mae"], z["ours_finite_diff"], z["gt"].size, "mae_gt_nan finite")


def test_mae_masks():
    z = load("mae_masks")
    assert same_bits(C.mask_dsm(z["gt"], z["water"], z["vis"], z["tree"]), z["masked"])
    assert same_bits(C.mask_dsm(z["gt"], z["water"], None, None), z["only_water"])
    assert z["masked"].shape == z["tree"].shape != z["gt"].shape
    diff, _, _ = C.dsm_pointwise_diff(z["pred"], z["masked"], clip="finite")
    assert np.array_equal(np.isnan(diff), np.isnan(z["ours_finite_diff"]))
    check_mae(C.mae_of(diff), z["ours_finite_mae"], z["ours_finite_diff"], z["masked"].size, "mae_masks finite")
