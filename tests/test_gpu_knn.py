"""GPU (MI355X): `distCUDA2` (include/eogs_knn.h) against an exact k-d tree (scipy.spatial.cKDTree) — the quantity the
reference computes is the exact mean squared distance to the three nearest neighbours (simple_knn.cu:147-185).

rtol = 2e-5 throughout, by derivation: the difference of two fp32 coordinates is one rounding whatever their offset from the
origin, so a squared distance carries a few 2^-24 relative, and a mis-ordered near-tie between the third and the fourth
neighbour changes the mean by no more than that.

A cliff that is NOT tested on purpose: the exact scan is quadratic in the size of a cluster of coincident points (every
point of the cluster has rejection radius 0 and scans every box that holds the cluster), in the reference as well. The
20,000 coincident points below cost 4e8 distance evaluations; hundreds of thousands would run for minutes."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def _exact(pts):
    d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4, workers=16)
    return (d[:, 1:] ** 2).mean(1)


def _check(dev, pts, ref=None):
    """distCUDA2 on fp32 points [P, 3] against the exact tree; also: a second call returns the same bits and the input is
    left as it was."""
    from eogs2_amd.knn import distCUDA2

    pts = np.ascontiguousarray(pts, dtype=np.float32)
    t = torch.from_numpy(pts).to(dev)
    before = t.clone()
    got = distCUDA2(t)
    again = distCUDA2(t)
    assert torch.equal(t, before) and got.dtype == torch.float32 and got.shape == (pts.shape[0],)
    assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    got = got.cpu().numpy()
    ref = _exact(pts) if ref is None else ref
    assert np.isfinite(got).all()
    assert np.allclose(got, ref, rtol=2e-5, atol=1e-12), float(np.abs(got - ref).max())
    return got


@pytest.mark.parametrize("P,kind", [(4, "uniform"), (1000, "uniform"), (100_003, "uniform"), (60_000, "scene"),
                                    (30_000, "clustered"), (5000, "planar")])
def test_dist2_matches_exact_knn(dev, P, kind):
    from simple_knn._C import distCUDA2  # the import path of the reference

    g = np.random.default_rng(P)
    if kind == "uniform":
        pts = g.random((P, 3))
    elif kind == "scene":   # the normalised EOGS scene box: thin in z
        pts = g.random((P, 3)) * [1.8, 1.8, 0.2] - [0.9, 0.9, 0.05]
    elif kind == "clustered":
        pts = g.normal(size=(P, 3)) * 0.01 + g.integers(0, 5, (P, 1)) * 3.0
    else:                    # one flat axis: the Morton normalisation of that axis is degenerate
        pts = np.concatenate([g.random((P, 2)), np.zeros((P, 1))], 1)
    pts = pts.astype(np.float32)
    got = distCUDA2(torch.from_numpy(pts).to(dev)).cpu().numpy()
    ref = _exact(pts)
    assert got.shape == (P,) and got.dtype == np.float32
    assert np.allclose(got, ref, rtol=2e-5, atol=1e-12), float(np.abs(got - ref).max())


def test_duplicates_and_tiny_inputs(dev):
    from eogs2_amd.knn import distCUDA2

    pts = torch.tensor([[0.0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 0]], device=dev)
    got = distCUDA2(pts).cpu().numpy()
    assert np.allclose(got, [1 / 3, 1 / 3, 1.0, 4.0, 1 / 3])  # coincident points are neighbours at distance 0
    assert distCUDA2(torch.zeros(0, 3, device=dev)).shape == (0,)
    with pytest.raises(RuntimeError):
        distCUDA2(torch.zeros(5, 2, device=dev))


def _scene_box(P, seed):
    g = np.random.default_rng(seed)
    return (g.random((P, 3)) * [1.8, 1.8, 0.2] - [0.9, 0.9, 0.05]).astype(np.float32)


def _surface(P, seed):
    from eogs2_amd.synthetic import make_scene

    return make_scene(P, 64, 64, seed=seed, kind="surface")["means3D"].numpy()


@pytest.mark.parametrize("P,kind", [(1_048_576, "scene"), (1_048_576, "surface"), (2_097_152, "scene")])
def test_dist2_at_the_headline_sizes(dev, P, kind):
    """1,048,576 points (the headline) in the normalised scene box and on a surface-shaped cloud; 2,097,152 (BASELINE's
    config 4; 1.3 s with its tree, so not behind the `slow` marker)."""
    _check(dev, _scene_box(P, 1) if kind == "scene" else _surface(P, 2))


@pytest.mark.parametrize("P", [1, 2, 3])
def test_fewer_than_four_points_give_the_reference_sentinel_value(dev, P):
    """simple_knn.cu:156-184 with fewer than three neighbours: the kept-3 list starts at the 1e37 sentinel, what is found
    replaces its head, and the three entries are summed in fp32 in list order and divided by 3: finite, not inf or nan."""
    from eogs2_amd.knn import distCUDA2

    pts = np.array([[0.25, -1.0, 2.0], [1.25, -1.0, 2.0], [0.25, 1.0, 2.0]], dtype=np.float32)[:P]
    got = distCUDA2(torch.from_numpy(pts).to(dev)).cpu().numpy()
    want = []
    for i in range(P):
        d = sorted(np.float32(((pts[i].astype(np.float64) - pts[j]) ** 2).sum()) for j in range(P) if j != i)
        best = (d + [np.float32(1e37)] * 3)[:3]
        want.append((np.float32(best[0] + best[1]) + best[2]) / np.float32(3.0))
    assert got.dtype == np.float32 and np.isfinite(got).all() and got.tobytes() == np.array(want, dtype=np.float32).tobytes()


def test_scene_far_from_the_origin(dev):
    """The scene box translated by (3e3, -7e3, 5e2), spacing unchanged: coordinates carry 12 bits of offset."""
    pts = (_scene_box(200_000, 3).astype(np.float64) + [3e3, -7e3, 5e2]).astype(np.float32)
    got = _check(dev, pts)
    assert got.max() < 1.0  # neighbours, not the 1e37 sentinel or the offset


@pytest.mark.parametrize("kind", ["diagonal", "axis"])
def test_collinear_points(dev, kind):
    """All points on one line: general direction, and axis-aligned (two flat axes: 1024 distinct Morton cells for 20,000 points)."""
    g = np.random.default_rng(5)
    t = g.random(20_000)
    pts = np.outer(t, [1.0, 0.0, 0.0] if kind == "axis" else [0.6, -1.1, 0.3]) + ([0.2, 0.3, -0.4] if kind == "axis" else [0, 0, 0])
    _check(dev, pts)


def test_regular_grid_of_ties(dev):
    """64^3 exact grid: six equidistant nearest neighbours everywhere inside (ties in the keep-3 list, equal Morton cells)."""
    a = np.arange(64, dtype=np.float32) * np.float32(0.125)
    pts = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    got = _check(dev, pts)
    assert (got == np.float32(0.125 ** 2)).all()  # every distance is exact in fp32: no tolerance needed


def test_coincident_points(dev):
    """20,000 coincident points inside a 100,000-point scene (rejection radius 0 for each of them), and 5,000 points that are
    all one point: exactly 0."""
    from eogs2_amd.knn import distCUDA2

    rest = _scene_box(80_000, 7)
    c = np.array([[0.123, -0.456, 0.05]], dtype=np.float32)
    pts = np.concatenate([rest[:30_000], np.repeat(c, 20_000, 0), rest[30_000:]])
    # the same quantity without a 20,000-point leaf in the tree: four copies of the cluster stand for all of it
    small = np.concatenate([rest, np.repeat(c, 4, 0)])
    r = _exact(small)
    ref = np.concatenate([r[:30_000], np.zeros(20_000), r[30_000:80_000]])
    got = _check(dev, pts, ref)
    assert (got[30_000:50_000] == 0).all()
    same = distCUDA2(torch.from_numpy(np.repeat(c, 5_000, 0)).to(dev)).cpu().numpy()
    assert (same == 0).all()


@pytest.mark.parametrize("P", [256, 257, 1024, 1025])
def test_box_edges_of_the_search_kernel(dev, P):
    _check(dev, np.random.default_rng(P).random((P, 3)))


def test_float64_and_strided_inputs(dev):
    from eogs2_amd.knn import distCUDA2

    pts = _scene_box(30_000, 9)
    want = _check(dev, pts)
    got64 = distCUDA2(torch.from_numpy(pts.astype(np.float64)).to(dev))
    wide = torch.from_numpy(np.concatenate([pts, np.ones((30_000, 3), np.float32)], 1)).to(dev)
    view = wide[:, :3]
    assert not view.is_contiguous()
    got_view = distCUDA2(view)
    assert got64.dtype == torch.float32 and got64.cpu().numpy().tobytes() == want.tobytes()
    assert got_view.cpu().numpy().tobytes() == want.tobytes() and bool((wide[:, 3:] == 1).all())
