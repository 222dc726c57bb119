"""CPU: the fixtures of the DSM raster (tests/golden/dsm_raster, written by tests/golden/make_golden_dsm_raster.py from the
reference's own compute_dsm_from_view and TSDFVolume.extract_dsm) and the statement of its semantics agree with an
independent brute-force loop over each point's clipped footprint; the kernels' home-cell-plus-stencil formulation, emulated
in numpy integers, gives the same cells, the same counts and values inside the issue's bound; the host geometry equals the
reference's bit for bit."""
import os

import numpy as np
import pytest

import dsm_raster_cases as K

CASES = K.cloud_cases()


def same(a, b):
    (ma, ca, sa), (mb, cb, sb) = a, b
    assert sa == sb
    assert np.array_equal(ca, cb)
    assert np.array_equal(np.isnan(ma), np.isnan(mb))
    f = ~np.isnan(ma)
    # two float64 summation orders of at most a few ten thousand float32 values: far below the bar of the kernels
    assert np.allclose(ma[f], mb[f], rtol=1e-12, atol=1e-12)


def test_fixtures_exist_and_are_small():
    names = K.fixture_names()
    assert {"view_48x40", "view_160x128"} <= set(names) and len(K.fixture_names("tsdf")) >= 2
    for p in K.fixture_files():
        assert os.path.getsize(p) < K.MAX_FIXTURE_BYTES, p
    for n in names:
        assert os.path.exists(os.path.join(K.GOLDEN, f"{n}_xy.npz")), n


@pytest.mark.parametrize("name", K.fixture_names())
def test_stored_raster_is_the_brute_force_raster(name):
    d = K.load(name)
    assert float(d["resolution"]) in (0.3, 0.5) and int(d["radius"]) == 1
    got = K.brute_force(d["cloud"], *d["geometry"][:2], float(d["resolution"]), *d["geometry"][2:], 1)
    same(got, (d["raster"], d["counts"], 0))
    assert d["raster"].dtype == np.float64 and d["raster"].shape == (d["geometry"][3], d["geometry"][2])
    assert (d["counts"] > 0).any() and not (d["counts"] < 0).any()


@pytest.mark.parametrize("name", K.fixture_names())
def test_fixture_margins(name):
    """What lets the GPU tests demand exact counts: no point within 1e-6 of a cell edge, no bound quotient within 1e-6 of an
    integer."""
    d = K.load(name)
    c, res, (xoff, yoff, _, _) = d["cloud"], float(d["resolution"]), d["geometry"]
    q = np.concatenate([(c[:, 0] - xoff) / res, (yoff - c[:, 1]) / res,
                        [c[:, 0].min() / res, (c[:, 0].max() - xoff) / res, c[:, 1].max() / res, (c[:, 1].min() - yoff) / res]])
    assert (np.abs(q - np.round(q)) > 1e-6).all()


@pytest.mark.parametrize("name", K.fixture_names())
def test_raster_geometry_is_the_reference_geometry(name):
    from eogs2_amd.dsm_raster import raster_geometry

    d = K.load(name)
    c = d["cloud"]
    xoff, yoff, xsize, ysize = raster_geometry(c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max(), float(d["resolution"]))
    assert isinstance(xsize, int) and isinstance(ysize, int)
    assert (xsize, ysize) == d["geometry"][2:]
    assert np.float64(xoff).tobytes() == d["xoff"].tobytes() and np.float64(yoff).tobytes() == d["yoff"].tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_is_the_brute_force_raster(name):
    """Clipping: only the target cell is range-checked (the cropped cases), lattice points fall where floor puts them."""
    same(K.restate(*CASES[name]), K.brute_force(*CASES[name]))


def test_cases_cover_what_they_claim():
    cloud, xoff, yoff, res, xsize, ysize, radius = CASES["cropped_by4.0_res0.5_r2"]
    i, j = np.floor((cloud[:, 0] - xoff) / res), np.floor((yoff - cloud[:, 1]) / res)
    outside = (i < 0) | (i >= xsize) | (j < 0) | (j >= ysize)
    reach = outside & (i >= -radius) & (i < xsize + radius) & (j >= -radius) & (j < ysize + radius)
    beyond = (i < -radius) | (i >= xsize + radius) | (j < -radius) | (j >= ysize + radius)
    assert reach.sum() > 100 and beyond.sum() > 100
    for side in (i < -radius, i >= xsize + radius, j < -radius, j >= ysize + radius):
        assert side.sum() > 10
    lattice = CASES["lattice_res0.5_r1"]
    q = (lattice[0][:, 0] - lattice[1]) / lattice[3]
    assert np.array_equal(q, np.round(q))  # exactly on the edges
    pile = CASES["pile_20000_in_one_cell"]
    assert K.restate(*pile)[1].max() == 20000
    assert K.restate(*CASES["empty"])[1].max() == 0 and np.isnan(K.restate(*CASES["empty"])[0]).all()


@pytest.mark.parametrize("name", sorted(CASES) + K.fixture_names())
def test_home_cell_plus_stencil_is_the_footprint_scatter(name):
    """The formulation of the kernels: same NaN pattern, same counts, values within q / 2 + ulp32(m)."""
    if name in CASES:
        args = CASES[name]
    else:
        d = K.load(name)
        args = (d["cloud"], *d["geometry"][:2], float(d["resolution"]), *d["geometry"][2:], 1)
    mean, counts, skipped = K.restate(*args)
    out, cnt, sk = K.emulate_kernel(*args)
    assert sk == skipped
    K.check_raster(out, cnt, mean, counts, ulps=1, what=name)


def test_poison_and_skips_in_the_statement():
    cloud, *geom = CASES["uniform_37x23_res0.5_r1"]
    cloud = cloud[:200].copy()
    cloud[3, 2], cloud[50, 2], cloud[70, 2], cloud[90, 2] = np.nan, np.inf, -np.inf, 2 * K.Z_MAX
    cloud[120, 0], cloud[130, 1] = np.nan, np.inf
    for f in (K.restate, K.brute_force, K.emulate_kernel):
        mean, counts, skipped = f(cloud, *geom)
        assert skipped == 2
        assert (counts == -1).sum() >= 4 and np.isnan(np.asarray(mean)[counts == -1]).all()
    same(K.restate(cloud, *geom), K.brute_force(cloud, *geom))
    assert np.array_equal(K.emulate_kernel(cloud, *geom)[1], K.restate(cloud, *geom)[1])


def test_bound_is_the_issues_bound():
    assert K.Z_QUANTUM <= 2.0 ** -20 and K.Z_MAX >= 32768
    assert K.ulp32(1.0) == 2.0 ** -23 and K.ulp32(1.5) == 2.0 ** -23 and K.ulp32(0.99) == 2.0 ** -24 and K.ulp32(30.0) == 2.0 ** -19
    assert K.value_bound(30.0) == 2.0 ** -21 + 2.0 ** -19 and K.value_bound(30.0, 2) == 2.0 ** -21 + 2.0 ** -18
