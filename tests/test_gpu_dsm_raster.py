"""GPU (MI355X): the DSM raster (eogs2_amd.dsm_raster, include/eogs_dsm.h) against the float64 restatement of its stated
semantics (tests/dsm_raster_cases.py, pinned on the CPU by tests/test_dsm_raster_cases.py) and against the vectors the
reference's own compute_dsm_from_view and TSDFVolume.extract_dsm produced (tests/golden/dsm_raster/). The bar is the
issue's: exact NaN pattern, exact counts, |out - m| <= q / 2 + ulp32(m) for clouds, q / 2 + 2 ulp32(m) where the kernel
forms z itself (a 1-ulp float64 difference in the matrix-vector product before narrowing); bit-identical under permutation
and from run to run."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import dsm_raster_cases as K

pytestmark = pytest.mark.gpu
CASES = K.cloud_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def expected():
    """The restatement of every cloud case, computed once."""
    return {name: K.restate(*args) for name, args in CASES.items()}


def gpu_cloud(cloud, dev):
    return torch.as_tensor(np.ascontiguousarray(cloud), dtype=torch.float64).reshape(-1, 3).to(dev)


def bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.mark.parametrize("name", sorted(CASES))
def test_cloud_against_the_restatement(dev, expected, name):
    from eogs2_amd.dsm_raster import plyflatten

    cloud, xoff, yoff, res, xsize, ysize, radius = CASES[name]
    mean, counts, _ = expected[name]
    skipped = torch.full((1,), -1, dtype=torch.int64, device=dev)
    out, cnt = plyflatten(gpu_cloud(cloud, dev), xoff, yoff, res, xsize, ysize, radius=radius, return_count=True, skipped_out=skipped)
    assert out.shape == (ysize, xsize, 1) and out.dtype == torch.float32 and out.device.type == "cuda"
    assert cnt.shape == (ysize, xsize) and cnt.dtype == torch.int32
    K.check_raster(out.cpu().numpy(), cnt.cpu().numpy(), mean, counts, ulps=1, what=name)
    assert int(skipped) == 0
    plain = plyflatten(gpu_cloud(cloud, dev), xoff, yoff, res, xsize, ysize, radius=radius)  # plyflatten's own signature
    assert bits(plain, out)


def test_bounds_and_geometry(dev):
    from eogs2_amd.dsm_raster import cloud_bounds, raster_geometry

    for name in ("uniform_37x23_res0.3_r1", "uniform_37x23_res0.5_r1", "lattice_res0.5_r1", "n1_on_1x1", "pile_20000_in_one_cell"):
        cloud, res = CASES[name][0], CASES[name][3]
        got = cloud_bounds(gpu_cloud(cloud, dev))
        want = (cloud[:, 0].min(), cloud[:, 0].max(), cloud[:, 1].min(), cloud[:, 1].max())
        assert all(isinstance(g, np.float64) for g in got)
        assert [g.tobytes() for g in got] == [np.float64(w).tobytes() for w in want], name  # a min is exact in any order
        xoff = np.floor(want[0] / res) * res  # utils/dsm_utils.py:20-25
        xsize = int(1 + np.floor((want[1] - xoff) / res))
        yoff = np.ceil(want[3] / res) * res
        ysize = int(1 - np.floor((want[2] - yoff) / res))
        assert raster_geometry(*got, res) == (xoff, yoff, xsize, ysize)
    big = np.random.default_rng(5).random((300_001, 3)) * 1e3  # more points than one pass of the grid: the strided loop
    got = cloud_bounds(gpu_cloud(big, dev))
    assert got == (big[:, 0].min(), big[:, 0].max(), big[:, 1].min(), big[:, 1].max())
    with pytest.raises(ValueError, match="empty"):
        cloud_bounds(gpu_cloud(np.zeros((0, 3)), dev))


def test_bad_z_poisons_its_footprint_and_bad_xy_is_skipped(dev):
    from eogs2_amd.dsm_raster import Z_MAX, cloud_bounds, plyflatten

    cloud, *geom = CASES["uniform_37x23_res0.5_r1"]
    xoff, yoff, res, xsize, ysize, _ = geom
    clean = K.restate(cloud, *geom)
    for radius in (0, 1, 2):
        for bad in (np.nan, np.inf, -np.inf, Z_MAX * (1 + 2.0 ** -20), -2 * Z_MAX, 1e300):
            c = cloud.copy()
            c[[17, 1234, 4999], 2] = bad
            mean, counts, _ = K.restate(c, xoff, yoff, res, xsize, ysize, radius)
            poisoned = counts == -1
            assert 3 <= poisoned.sum() <= 3 * (2 * radius + 1) ** 2  # exactly the three footprints (clipped, overlapping)
            out, cnt = plyflatten(gpu_cloud(c, dev), xoff, yoff, res, xsize, ysize, radius=radius, return_count=True)
            K.check_raster(out.cpu().numpy(), cnt.cpu().numpy(), mean, counts, what=f"z = {bad}, radius {radius}")
    c = cloud.copy()
    c[5, 2] = Z_MAX  # the largest z that is still a height
    out, cnt = plyflatten(gpu_cloud(c, dev), *geom[:5], radius=1, return_count=True)
    mean, counts, _ = K.restate(c, *geom)
    assert not (counts == -1).any()
    K.check_raster(out.cpu().numpy(), cnt.cpu().numpy(), mean, counts, what="z = Z_MAX")
    # a non-finite x or y: skipped and counted with explicit geometry, an error where the grid would come from it
    c = cloud.copy()
    c[3, 0], c[40, 1], c[41, 0], c[42, 1] = np.nan, np.nan, np.inf, -np.inf
    mean, counts, sk = K.restate(c, *geom)
    assert sk == 4 and not np.array_equal(counts, clean[1])
    skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    out, cnt = plyflatten(gpu_cloud(c, dev), *geom[:5], radius=1, return_count=True, skipped_out=skipped)
    K.check_raster(out.cpu().numpy(), cnt.cpu().numpy(), mean, counts, what="non-finite x, y")
    assert int(skipped) == 4
    with pytest.raises(ValueError, match="non-finite"):
        cloud_bounds(gpu_cloud(c, dev))


def test_permutation_and_rerun_give_the_same_bits(dev):
    from eogs2_amd.dsm_raster import plyflatten

    g = torch.Generator().manual_seed(3)
    for name in ("uniform_37x23_res0.3_r1", "uniform_37x23_res0.5_r2", "pile_20000_in_one_cell", "pile_near_zmax"):
        cloud, xoff, yoff, res, xsize, ysize, radius = CASES[name]
        t = gpu_cloud(cloud, dev)
        first, c1 = plyflatten(t, xoff, yoff, res, xsize, ysize, radius=radius, return_count=True)
        again, c2 = plyflatten(t, xoff, yoff, res, xsize, ysize, radius=radius, return_count=True)
        assert bits(first, again) and torch.equal(c1, c2), f"{name}: two runs differ"
        for _ in range(2):
            perm = torch.randperm(t.shape[0], generator=g).to(dev)
            shuffled, c3 = plyflatten(t[perm].contiguous(), xoff, yoff, res, xsize, ysize, radius=radius, return_count=True)
            assert bits(first, shuffled) and torch.equal(c1, c3), f"{name}: a permutation changes the raster"
        assert bits(first, plyflatten(t.flip(0).contiguous(), xoff, yoff, res, xsize, ysize, radius=radius))


def _camera(d, dev):
    return types.SimpleNamespace(affine=torch.as_tensor(d["affine"]).to(dev), Ainv=torch.as_tensor(d["Ainv"]).to(dev))


@pytest.mark.parametrize("name", K.fixture_names("view"))
def test_view_fixtures(dev, name):
    """dsm_from_view on the reference's inputs against what its compute_dsm_from_view handed to plyflatten."""
    from eogs2_amd.dsm_raster import cloud_bounds, dsm_from_view, plyflatten, view_axes

    d = K.load(name)
    res = float(d["resolution"])
    alt = torch.as_tensor(d["altitude"]).to(dev)
    axes = (torch.as_tensor(d["u_axis"]).to(dev), torch.as_tensor(d["v_axis"]).to(dev))  # the camera's own UV grid
    sp = [d["center"], float(d["scale"]), 17, "T"]
    profile, dsm, cnt = dsm_from_view(alt, _camera(d, dev), sp, res, uv_axes=axes, return_count=True)
    xoff, yoff, xsize, ysize = d["geometry"]
    assert profile == {"dtype": "float32", "height": ysize, "width": xsize, "count": 1, "nodata": profile["nodata"],
                       "transform": (res, 0.0, float(xoff), 0.0, -res, float(yoff))} and math.isnan(profile["nodata"])
    K.check_raster(dsm.cpu().numpy(), cnt.cpu().numpy(), d["raster"], d["counts"].astype(np.int32), ulps=2, what=name)
    # the same grid handed over: no wait, the same bits; (Ainv, b) in place of the camera: the same bits
    _, fixed = dsm_from_view(alt, _camera(d, dev), sp, res, uv_axes=axes, geometry=d["geometry"])
    assert bits(fixed, dsm)
    cam = _camera(d, dev)
    _, pair = dsm_from_view(alt[None], (cam.Ainv, cam.affine[3, :3]), sp, res, uv_axes=axes, geometry=d["geometry"])
    assert bits(pair, dsm)
    # the bounds pass of the cloud path on the reference's own points
    cb = cloud_bounds(gpu_cloud(d["cloud"], dev))
    assert cb == (d["cloud"][:, 0].min(), d["cloud"][:, 0].max(), d["cloud"][:, 1].min(), d["cloud"][:, 1].max())
    # the stored cloud through plyflatten: the cloud path on the reference's own points, one ulp32 as for every cloud
    out, c2 = plyflatten(gpu_cloud(d["cloud"], dev), xoff, yoff, res, xsize, ysize, return_count=True)
    K.check_raster(out.cpu().numpy(), c2.cpu().numpy(), d["raster"], d["counts"].astype(np.int32), ulps=1, what=name + " (cloud)")
    # the default UV grid is torch.linspace on the image's device
    H, W = alt.shape
    u, v = view_axes(H, W, dev)
    assert torch.equal(u, torch.linspace(-1, 1, W, device=dev)) and torch.equal(v, torch.linspace(-1, 1, H, device=dev))
    _, default = dsm_from_view(alt, _camera(d, dev), sp, res, geometry=d["geometry"])
    _, explicit = dsm_from_view(alt, _camera(d, dev), sp, res, uv_axes=(u, v), geometry=d["geometry"])
    assert bits(default, explicit)


@pytest.mark.parametrize("name", K.fixture_names("tsdf"))
def test_tsdf_fixtures(dev, name):
    """TSDFVolume.extract_dsm against what the reference's extract_dsm handed to plyflatten; surface_cloud -> plyflatten
    gives the same bits."""
    from eogs2_amd.dsm_raster import plyflatten
    from eogs2_amd.tsdf import TSDFVolume

    d = K.load(name)
    res = float(d["resolution"])
    vol = TSDFVolume.__new__(TSDFVolume)  # the stored axes and volume in place of the constructor's
    vol.device = dev
    vol.axes = [torch.as_tensor(d[f"axis{k}"]).to(dev) for k in range(3)]
    vol._tsdf_vol = torch.as_tensor(d["tsdf"]).to(dev)
    sp = [d["center"], 1.0, 17, "T"]
    profile, dsm = vol.extract_dsm(sp, res)
    xoff, yoff, xsize, ysize = d["geometry"]
    assert (profile["height"], profile["width"]) == (ysize, xsize)
    assert profile["transform"] == (res, 0.0, float(xoff), 0.0, -res, float(yoff))
    assert dsm.device.type == "cuda" and dsm.shape == (ysize, xsize, 1)
    K.check_raster(dsm.cpu().numpy(), None, d["raster"], d["counts"].astype(np.int32), ulps=2, what=name)
    cloud = vol.surface_cloud(sp)
    assert np.array_equal(cloud, d["cloud"])  # unchanged: the reference's cloud
    flat, cnt = plyflatten(gpu_cloud(cloud, dev), xoff, yoff, res, xsize, ysize, return_count=True)
    assert np.array_equal(cnt.cpu().numpy(), d["counts"])
    assert bits(flat, dsm)


def test_graph_replay_equals_eager(dev):
    from eogs2_amd.dsm_raster import plyflatten

    cloud, xoff, yoff, res, xsize, ysize, radius = CASES["uniform_37x23_res0.3_r1"]
    other = CASES["uniform_37x23_res0.3_r2"][0].copy()
    other[:, 2] = other[::-1, 2] * 0.5 + 3.0
    other[:, 0] += 0.07
    t = gpu_cloud(cloud, dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        plyflatten(t, xoff, yoff, res, xsize, ysize, radius=radius, return_count=True)  # warm-up: the workspace of this shape
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out, cnt = plyflatten(t, xoff, yoff, res, xsize, ysize, radius=radius, return_count=True)
    for c in (other, cloud):
        t.copy_(gpu_cloud(c, dev))  # refill
        graph.replay()
        torch.cuda.synchronize(dev)
        eager, ecnt = plyflatten(gpu_cloud(c, dev), xoff, yoff, res, xsize, ysize, radius=radius, return_count=True)
        assert bits(out, eager) and torch.equal(cnt, ecnt)
    mean, counts, _ = K.restate(cloud, xoff, yoff, res, xsize, ysize, radius)
    K.check_raster(out.cpu().numpy(), cnt.cpu().numpy(), mean, counts, what="replayed")


def test_chain_view_to_registered_mae(dev):
    """render altitude -> DSM on the target's geometry -> dsm_eval.dsm_mae, nothing leaves the device in between."""
    from eogs2_amd.dsm_eval import dsm_mae
    from eogs2_amd.dsm_raster import dsm_from_view

    d = K.load("view_160x128")
    res = float(d["resolution"])
    alt = torch.as_tensor(d["altitude"]).to(dev)
    axes = (torch.as_tensor(d["u_axis"]).to(dev), torch.as_tensor(d["v_axis"]).to(dev))
    sp = [d["center"], float(d["scale"]), 17, "T"]
    profile, target = dsm_from_view(alt, _camera(d, dev), sp, res, uv_axes=axes)
    geometry = (profile["transform"][2], profile["transform"][5], profile["width"], profile["height"])
    g = torch.Generator().manual_seed(1)
    noisy = alt + 0.01 * torch.randn(alt.shape, generator=g).to(dev)
    _, pred = dsm_from_view(noisy, _camera(d, dev), sp, res, uv_axes=axes, geometry=geometry)
    assert pred.shape == target.shape and pred.device.type == "cuda"
    mae, diff, _, (dx, dy, _, _) = dsm_mae(pred[:, :, 0], target[:, :, 0], clip="finite")
    assert math.isfinite(mae) and 0.0 < mae < 0.01 * float(d["scale"]) * 3 and abs(dx) <= 1 and abs(dy) <= 1
    same, _, _, shift = dsm_mae(target[:, :, 0], target[:, :, 0], clip="finite")
    assert same < 1e-9 and shift[:2] == (0, 0)  # (the registration's offset b = muu - muv need not be an exact 0)


def test_example_scores_dsms():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    args = ["--gaussians", "20000", "--size", "160", "--iters", "20", "--quiet"]
    plain = train_synthetic.main(args)
    scored = train_synthetic.main(args + ["--dsm-mae-every", "10", "--dsm-resolution", "6"])
    assert scored == plain  # rasterising and scoring read the render, they change nothing
    scores = train_synthetic.main.last_dsm_mae
    assert [s[0] for s in scores] == [10, 20]
    for it, dx, dy, mae in scores:
        assert isinstance(dx, int) and isinstance(dy, int) and math.isfinite(mae) and mae >= 0.0
    print("DSM MAE over the run (iteration, dx, dy, mae):", scores)
    with pytest.raises(SystemExit):
        train_synthetic.main(args + ["--dsm-resolution", "6"])  # needs --dsm-mae-every
