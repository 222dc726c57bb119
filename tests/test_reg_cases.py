"""CPU: the fixtures of the regularisers (tests/golden/reg/*.npz, written by the reference's own classes in float32 and in
float64), the plain-torch restatement of tests/reg_cases.py and the derived error bounds, against one another:

  * the restatement replays the reference's torch ops: its float32 run reproduces the fixture's float32 run bit for bit,
    its float64 run the float64 run;
  * the reference's own float32 run stays inside factor 1 of every derived bound against its float64 run;
  * the bounds, at the kernels' factor, reject each planted mutant of the restatement on some output of some fixture;
  * the fixtures hold what they are meant to hold (ties, both sides of the clip, a row on the clip, retired rows, flat
    patches, H != W, 2 x 2).
"""
import numpy as np
import pytest
import torch

import reg_cases as rc


def _runs(fx, keys):
    return {k: fx[k + "@32"] for k in keys}, {k: fx[k + "@64"] for k in keys}


@pytest.mark.parametrize("name", rc.GAUSS_FIXTURES)
def test_restatement_reproduces_the_gaussian_fixtures(name):
    fx = rc.load(name)
    ref32, ref64 = _runs(fx, rc.GAUSS_KEYS)
    o, l, r, n0, up = rc.gauss_inputs(fx)
    got32 = rc.restate_gauss(o, l, r, n0, up, torch.float32)
    got64 = rc.restate_gauss(o, l, r, n0, up, torch.float64)
    for k in rc.GAUSS_KEYS:
        assert got32[k].dtype == np.float32 and np.array_equal(got32[k], ref32[k]), (name, k)  # the same torch ops: the same bits
        assert got64[k].dtype == np.float64 and np.array_equal(got64[k], ref64[k]), (name, k)


@pytest.mark.parametrize("name", rc.IMAGE_FIXTURES)
def test_restatement_reproduces_the_image_fixtures(name):
    fx = rc.load(name)
    ref32, ref64 = _runs(fx, rc.IMAGE_KEYS)
    a, c, up = rc.image_inputs(fx)
    got32, got64 = rc.restate_image(a, c, up, torch.float32), rc.restate_image(a, c, up, torch.float64)
    for k in rc.IMAGE_KEYS:
        assert np.array_equal(got32[k], ref32[k]) and np.array_equal(got64[k], ref64[k]), (name, k)


@pytest.mark.parametrize("name", rc.GAUSS_FIXTURES)
def test_reference_fp32_stays_inside_the_derived_bounds_gaussian(name):
    fx = rc.load(name)
    ref32, ref64 = _runs(fx, rc.GAUSS_KEYS)
    b = rc.gauss_bounds(*rc.gauss_inputs(fx))
    # the fixtures need no excusal except the one row that was put ON the clip in float32 (gauss_mix)
    assert int(b["excusable"].sum()) == (1 if name == "gauss_mix" else 0)
    rc.compare(ref32, ref64, b, rc.GAUSS_KEYS, 1.0, name + " reference fp32", excuse_rows=True)
    for k in ("L_opacity", "L_opacity_radii"):  # well conditioned: sigmoid's 6 roundings, the sum's depth, one division
        assert b[k] <= (8 + rc.sum_depth(fx["opacity"].shape[0])) * rc.U * b["scale:" + k], (name, k, b[k], b["scale:" + k])
    # (L_erank's bound is wider on needles, whose e + 1e-5 ~ 2e-5 carries the absolute error of log(q + 1e-6) at q ~ 1;
    # what it still rejects is asserted mutant by mutant below)


@pytest.mark.parametrize("name", rc.IMAGE_FIXTURES)
def test_reference_fp32_stays_inside_the_derived_bounds_image(name):
    fx = rc.load(name)
    ref32, ref64 = _runs(fx, rc.IMAGE_KEYS)
    rc.compare(ref32, ref64, rc.image_bounds(*rc.image_inputs(fx)), rc.IMAGE_KEYS, 1.0, name + " reference fp32")


@pytest.mark.parametrize("mutant", rc.MUTANTS_GAUSS)
def test_bounds_reject_the_gaussian_mutants(mutant):
    """Each mutant, run in float64 (no rounding to hide behind), leaves the kernels' bound on some fixture. The mutant of the
    clip at equality differs from the reference only where t == 0 exactly, which happens in float32 arithmetic alone: it
    is run in float32 and judged, with the same bound, against the reference's float32 gradients at the row that
    make_golden_reg.py put on the clip."""
    hit = []
    for name in rc.GAUSS_FIXTURES:
        fx = rc.load(name)
        ref32, ref64 = _runs(fx, rc.GAUSS_KEYS)
        o, l, r, n0, up = rc.gauss_inputs(fx)
        b = rc.gauss_bounds(o, l, r, n0, up)
        if mutant == "clip_drop_equal":
            got = rc.restate_gauss(o, l, r, n0, up, torch.float32, mutant=mutant)
            rows = np.flatnonzero(b["excusable"])
            for i in rows:
                err = np.abs(got["g_scaling"][i].astype(np.float64) - ref32["g_scaling"][i].astype(np.float64))
                hit.append(bool((err > rc.KERNEL_FACTOR * b["g_scaling"][i]).any()))
        else:
            hit.append(rc.rejects(rc.restate_gauss(o, l, r, n0, up, torch.float64, mutant=mutant), ref64, b, rc.GAUSS_KEYS))
            assert not rc.rejects(rc.restate_gauss(o, l, r, n0, up, torch.float64), ref64, b, rc.GAUSS_KEYS)
    assert any(hit), mutant


@pytest.mark.parametrize("mutant", rc.MUTANTS_IMAGE)
def test_bounds_reject_the_image_mutants(mutant):
    hit = []
    for name in rc.IMAGE_FIXTURES:
        fx = rc.load(name)
        _, ref64 = _runs(fx, rc.IMAGE_KEYS)
        a, c, up = rc.image_inputs(fx)
        hit.append(rc.rejects(rc.restate_image(a, c, up, torch.float64, mutant=mutant), ref64, rc.image_bounds(a, c, up), rc.IMAGE_KEYS))
    assert any(hit), mutant


def test_fixtures_hold_what_they_are_for():
    fx = rc.load("gauss_mix")
    o, l, r, n0, up = rc.gauss_inputs(fx)
    alive = o.reshape(-1) > 0.5 * rc.RETIRED_LOGIT
    assert int((~alive).sum()) == 64 and bool((o[~alive] == rc.RETIRED_LOGIT).all())
    assert float(o[alive].min()) == -12.0 and float(o[alive].max()) == 12.0 and int((o == 0).sum()) > 50
    assert n0 != int(alive.sum()) and n0 != o.shape[0]  # init_number_of_gaussians is a constant, not P
    la = l[alive]
    iso = (la[:, 0] == la[:, 1]) & (la[:, 1] == la[:, 2])
    srt = la.sort(1).values
    two = (srt[:, 0] == srt[:, 1]) & (srt[:, 1] < srt[:, 2])
    assert int(iso.sum()) == 512 and int(two.sum()) == 512
    t = rc.gauss_bounds(o, l, r, n0, up)["t"][alive.numpy()]
    assert int((t > 1e-3).sum()) > 500 and int((t < -1e-3).sum()) > 500  # clearly on both sides of the clip
    t32 = rc.erank_rows(la)[1]
    assert int((t32 == 0).sum()) == 1  # and one row on it, in float32
    assert bool((r[alive] > 0).any()) and bool((r[alive] == 0).any())
    # retired rows: zero gradient in every column of both runs
    for k in ("g_opacity_op", "g_opacity_radii", "g_scaling"):
        for tag in ("@32", "@64"):
            assert not fx[k + tag][~alive.numpy()].any(), k
    # the amin tie: an isotropic row's gradient is the same on its three axes
    g = fx["g_scaling@64"][alive.numpy()][iso.numpy()]
    assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 1], g[:, 2]) and (g[:, 0] != 0).all()
    z = rc.load("gauss_radii_all_zero")
    assert not z["radii"].any() and float(z["L_opacity_radii@32"]) == 0.0 and not z["g_opacity_radii@32"].any()
    im = rc.load("image_24x37")["altitude"]
    assert im.shape == (24, 37) and int((np.diff(im, axis=0) == 0).sum()) > 100 and int((np.diff(im, axis=1) == 0).sum()) > 100
    assert rc.load("image_2x2")["altitude"].shape == (2, 2)
    f = rc.load("image_flat_9x16")
    assert float(f["L_TV_altitude@32"]) == 0.0 and not f["g_altitude@32"].any()  # sign(0) = 0
