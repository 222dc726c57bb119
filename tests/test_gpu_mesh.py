"""GPU (MI355X): the mesh extraction (eogs2_amd.mesh, include/eogs_mesh.h) against its stated semantics restated in numpy
float64 (tests/mesh_cases.py): the vertices bit for bit in the stated order, in index and world coordinates, with and
without the shift; every triangle inside its cell, cells ascending, the count the cases give; closed, outward-oriented
surfaces on padded volumes, boundary-only open edges on an unpadded one; the same bits from run to run; empty and
non-finite volumes; and TSDFVolume.extract_mesh end to end with its OBJ file."""
import ctypes
import types

import numpy as np
import pytest
import torch

import mesh_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def table():
    return K.load_table()


def run(vol, iso, dev, axes=None, shift=None):
    from eogs2_amd.mesh import marching_cubes

    v, t = marching_cubes(torch.as_tensor(vol).to(dev), iso, axes=None if axes is None else [torch.as_tensor(a).to(dev) for a in axes],
                          shift=shift)
    assert v.dtype == torch.float64 and t.dtype == torch.int32 and v.device == dev and t.device == dev
    assert v.ndim == 2 and v.shape[1] == 3 and t.ndim == 2 and t.shape[1] == 3
    return v.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize("name", list(K.VOLUMES))
def test_volume(dev, table, name):
    vol, iso, closed = K.VOLUMES[name]()
    edges, ntris = table
    axes = K.axes_for(vol.shape)
    first = None
    for ax, sh in ((None, None), (None, K.SHIFT), (axes, None), (axes, K.SHIFT)):
        want, keys = K.expected_vertices(vol, iso, ax, sh)
        got, tri = run(vol, iso, dev, ax, sh)
        assert len(want) > 0 and got.shape == want.shape, (got.shape, want.shape)
        assert got.tobytes() == want.tobytes(), f"{name}: {int((got != want).any(axis=1).sum())} of {len(want)} vertices differ"
        if first is None:
            first = (got, keys, tri)
        else:
            assert np.array_equal(tri, first[2])  # the coordinates do not touch the triangles
    got, keys, tri = first
    K.check_triangles_in_cells(vol, iso, keys, tri, ntris)
    assert np.array_equal(tri, K.expected_triangles(vol, iso, keys, edges, ntris))  # cell by cell in table order
    if closed:
        K.check_closed(tri, len(keys))
        assert K.signed_volume(got, tri) > 0
    else:
        assert K.check_open(vol, keys, tri) > 0
    if name == "random_48x48x40":
        from eogs2_amd._abi import MESH_SCAN_ROUND, MESH_WG_VOXELS

        assert vol.size > MESH_SCAN_ROUND * MESH_WG_VOXELS  # more workgroups than one chunk of the scan covers
    if name == "exact_iso":
        v = got[tri]
        assert (np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) == 0).any()  # degenerate triangles exist


def test_repeat_runs_give_the_same_bits(dev):
    vol, iso, _ = K.VOLUMES["random_48x48x40"]()
    axes = K.axes_for(vol.shape)
    a, b = run(vol, iso, dev, axes, K.SHIFT), run(vol, iso, dev, axes, K.SHIFT)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_more_chunks_than_one_round_of_the_top_scan(dev):
    """260 x 256 x 256 voxels are 66 560 workgroups, 260 chunks of 256: the top level of the scan takes two rounds and carries
    from one to the next (a chunk is one x plane here). Isolated inside voxels in an outside volume, in the first chunks, at
    the end of the first round (x = 254, 255) and in the second (x = 256, 257): each gives an octahedron of six vertices and
    eight triangles, written down here without touching the other 17 million voxels."""
    from eogs2_amd._abi import MESH_SCAN_ROUND, MESH_WG_VOXELS
    from eogs2_amd.mesh import marching_cubes

    shape = (260, 256, 256)
    assert shape[0] * shape[1] * shape[2] > MESH_SCAN_ROUND * MESH_SCAN_ROUND * MESH_WG_VOXELS
    seeds = np.array([[1, 1, 1], [4, 200, 77], [100, 3, 250], [252, 254, 254], [255, 1, 1], [257, 128, 9]])  # x apart: cells in order
    values = -np.linspace(0.1, 0.9, len(seeds)).astype(np.float32)
    vol = torch.ones(shape, dtype=torch.float32, device=dev)
    vol[tuple(torch.as_tensor(seeds.T).to(dev))] = torch.as_tensor(values).to(dev)
    v, t = marching_cubes(vol)
    a, one = values.astype(np.float64), np.float64(1.0)
    t_lo, t_hi = (0.0 - one) / (a - one), (0.0 - a) / (one - a)  # the edge ending at the seed, the edge starting there
    pos, keys = [], []
    lin = lambda q: (q[:, 0] * shape[1] + q[:, 1]) * shape[2] + q[:, 2]  # noqa: E731
    for axis in range(3):
        e = np.eye(3, dtype=np.int64)[axis]
        for owner, tt in ((seeds - e, t_lo), (seeds, t_hi)):
            p = owner.astype(np.float64)
            p[:, axis] = owner[:, axis].astype(np.float64) + tt
            pos.append(p)
            keys.append(lin(owner) * 3 + axis)
    pos, keys = np.concatenate(pos), np.concatenate(keys)
    order = np.argsort(keys)
    assert v.cpu().numpy().tobytes() == pos[order].tobytes()
    tri = t.cpu().numpy()
    assert tri.shape == (8 * len(seeds), 3)
    K.check_closed(tri, len(keys))
    assert K.signed_volume(pos[order], tri) > 0
    # a triangle stays at its seed: its cell's lowest corner is the seed or one step below it on every axis
    sorted_keys = keys[order]
    owner = sorted_keys[tri] // 3
    ox, oy, oz = owner // (shape[1] * shape[2]), (owner // shape[2]) % shape[1], owner % shape[2]
    which = np.repeat(np.arange(len(seeds)), 8)  # the seeds are in linear order, so are their cells
    for o, k in ((ox, 0), (oy, 1), (oz, 2)):
        assert (np.abs(o - seeds[which, k][:, None]) <= 1).all()


def test_non_contiguous_and_wrong_dtype(dev):
    from eogs2_amd.mesh import marching_cubes

    vol, iso, _ = K.VOLUMES["random_7x5x67"]()
    t = torch.as_tensor(np.ascontiguousarray(vol.transpose(2, 1, 0))).to(dev).permute(2, 1, 0)
    assert not t.is_contiguous()
    v, _ = marching_cubes(t, iso)
    assert v.cpu().numpy().tobytes() == K.expected_vertices(vol, iso)[0].tobytes()
    with pytest.raises(TypeError, match="float32"):
        marching_cubes(torch.as_tensor(vol).double().to(dev))
    with pytest.raises(TypeError, match="float32"):
        marching_cubes(torch.as_tensor(vol[0]).to(dev))


def test_degenerate_inputs(dev):
    from eogs2_amd.mesh import marching_cubes

    for vol in (np.ones((5, 6, 7), dtype=np.float32), -np.ones((5, 6, 7), dtype=np.float32),  # all outside, all inside
                np.random.default_rng(0).standard_normal((1, 9, 70)).astype(np.float32),  # nx = 1: no cell
                np.random.default_rng(1).standard_normal((6, 1, 5)).astype(np.float32),
                np.random.default_rng(2).standard_normal((6, 5, 1)).astype(np.float32)):
        v, t = marching_cubes(torch.as_tensor(vol).to(dev))
        assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and v.dtype == torch.float64 and t.dtype == torch.int32
    vol, iso, _ = K.VOLUMES["random_7x5x67"]()
    for bad in (np.nan, np.inf, -np.inf):
        planted = vol.copy()
        planted[3, 2, 65] = bad
        planted[8, 6, 68] = bad  # the last voxel
        with pytest.raises(ValueError, match="2 of .* voxels are not finite"):
            marching_cubes(torch.as_tensor(planted).to(dev), iso)


def test_mismatched_counts_are_an_error(dev):
    """eogs_mesh_emit with other sizes than eogs_mesh_count found returns an error and writes nothing."""
    from eogs2_amd import _lib

    abi = _lib.get()
    vol, iso, _ = K.VOLUMES["random_3x3x3"]()
    nv, nt = len(K.expected_vertices(vol, iso)[0]), int(K.triangle_cells(vol, iso, K.load_table()[1])[0].shape[0])
    t = torch.as_tensor(vol).to(dev)
    nb = ctypes.c_size_t()
    abi.check(abi.mesh_bytes(*vol.shape, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    abi.check(abi.mesh_count(*vol.shape, p(t), iso, p(ws), ws.numel(), p(counts), stream))
    assert counts.cpu().tolist() == [nv, nt, 0, 0]
    verts = torch.full((nv + 1, 3), -7.0, dtype=torch.float64, device=dev)
    tris = torch.full((nt + 1, 3), -7, dtype=torch.int32, device=dev)
    for a, b in ((nv - 1, nt), (nv, nt - 1), (nv + 1, nt), (nv, nt + 1), (0, 0)):
        assert abi.mesh_emit(*vol.shape, p(t), iso, None, None, None, None, p(ws), ws.numel(), p(verts), a, p(tris), b, stream) == -1
        assert b"counts of mesh_count" in abi.cdll.eogs_rast_last_error()
    torch.cuda.synchronize()
    assert bool((verts == -7.0).all()) and bool((tris == -7).all())
    abi.check(abi.mesh_emit(*vol.shape, p(t), iso, None, None, None, None, p(ws), ws.numel(), p(verts), nv, p(tris), nt, stream))
    torch.cuda.synchronize()
    assert bool((verts[nv] == -7.0).all()) and bool((tris[nt] == -7).all())  # nothing past either array
    assert verts[:nv].cpu().numpy().tobytes() == K.expected_vertices(vol, iso)[0].tobytes()


def parse_obj(path):
    v, f = [], []
    for line in open(path):
        p = line.split()
        if p and p[0] == "v":
            v.append([float(x) for x in p[1:]])
        elif p and p[0] == "f":
            f.append([int(x) - 1 for x in p[1:]])
    return np.array(v, dtype=np.float64).reshape(-1, 3), np.array(f, dtype=np.int64).reshape(-1, 3)


def test_tsdf_volume_end_to_end(dev, table, tmp_path):
    """integrate of one synthetic range image + apply_prior, then the reference's line `extract_mesh(output_mesh_path=p)`."""
    from eogs2_amd.tsdf import TSDFVolume

    H, W = 48, 64
    g = torch.Generator().manual_seed(1)
    coef = torch.tensor([[0.0, 0.9, 0.0], [0.9, 0.0, 0.0], [0.0, 0.0, 1.0]])
    coef[:2, 2] = 0.15 * torch.randn(2, generator=g)
    intercept = torch.tensor([0.02, -0.03, 0.1])
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    alt = (0.15 * torch.sin(3 * xx) * torch.cos(2 * yy))[None, None]
    wgt = 0.05 + 0.95 * torch.rand((1, 1, H, W), generator=g)
    ri = types.SimpleNamespace(affine_model=(coef.to(dev), intercept.to(dev)), model_scale=1.7, altitude_img=alt.to(dev),
                               get_weights=lambda: wgt.to(dev))
    vol = TSDFVolume(np.array([[-1.4, 1.4], [-1.3, 1.3], [-0.3, 0.4]]), 0.06, 3.0, device=dev)
    vol.integrate(ri)
    vol.apply_prior()
    path = tmp_path / "mesh.obj"
    v, t = vol.extract_mesh(output_mesh_path=path)
    assert v.shape[0] > 100 and t.shape[0] > 100 and v.dtype == torch.float64 and t.dtype == torch.int32
    host = vol._tsdf_vol.cpu().numpy()
    want, keys = K.expected_vertices(host, 0.0)
    assert v.cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(t.cpu().numpy(), K.expected_triangles(host, 0.0, keys, *table))
    K.check_open(host, keys, t.cpu().numpy())
    v2, f2 = parse_obj(path)
    assert v2.tobytes() == want.tobytes() and np.array_equal(f2, t.cpu().numpy())
    sp = [K.SHIFT, 1.0, 17, "T"]
    vw, tw = vol.extract_mesh(coords="world", scene_params=sp)
    assert vw.cpu().numpy().tobytes() == K.expected_vertices(host, 0.0, [a.cpu().numpy() for a in vol.axes], K.SHIFT)[0].tobytes()
    assert torch.equal(tw, t)
