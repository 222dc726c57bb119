"""Shared by the mesh tests (tests/test_mesh_table.py, tests/test_gpu_mesh.py): the volumes of the issue, the stated semantics
of include/eogs_mesh.h restated in vectorised numpy float64 (the vertices, bit for bit; the triangle list that the table
gives), and the checks on a finished mesh. No per-cell Python loop anywhere."""
import ctypes

import numpy as np

SHIFT = np.array([512345.25, 4321987.75, 31.5])  # UTM-sized: the float64 add matters


def load_table():
    """(edges int [256, 15], ntris int [256]) through the host accessor of the built library."""
    from eogs2_amd import _lib, build

    build.build(verbose=False)
    abi = _lib.get()
    edges, ntris = np.zeros((256, 15), dtype=np.int64), np.zeros(256, dtype=np.int64)
    row, n = (ctypes.c_int8 * 15)(), ctypes.c_int()
    for c in range(256):
        abi.check(abi.mesh_case(c, row, ctypes.byref(n)))
        edges[c], ntris[c] = list(row), n.value
    return edges, ntris


# ---- volumes ----------------------------------------------------------------------------------------------------------
def padded(interior, outside=1.0):
    out = np.full(tuple(s + 2 for s in interior.shape), outside, dtype=np.float32)
    out[1:-1, 1:-1, 1:-1] = interior
    return out


def all_cases_volume(seed=0):
    """64 x 64 x 4: case c = 16 i + j alone in the 4 x 4 x 4 block (i, j), its cell in the middle, outside values around."""
    g = np.random.default_rng(seed)
    vol = (0.1 + 0.9 * g.random((64, 64, 4))).astype(np.float32)
    c = np.arange(256).reshape(16, 16)
    for b in range(8):
        dx, dy, dz = b & 1, (b >> 1) & 1, b >> 2
        sub = vol[1 + dx::4, 1 + dy::4, 1 + dz]
        vol[1 + dx::4, 1 + dy::4, 1 + dz] = np.where((c >> b) & 1, -sub, sub)
    return vol


def random_padded(dims, seed):
    return padded(np.random.default_rng(seed).standard_normal(dims).astype(np.float32), 1.0)


def exact_iso_volume(seed=5):
    """values in {-1, 0, 1}: many voxels sit exactly on iso = 0 (outside), so t is exactly 0 or 1"""
    return padded(np.random.default_rng(seed).integers(-1, 2, (5, 6, 7)).astype(np.float32), 1.0)


def axes_for(shape, seed=11):
    """increasing, unevenly spaced fp32 axes"""
    g = np.random.default_rng(seed)
    return [np.cumsum(0.05 + g.random(n)).astype(np.float32) - np.float32(3.0) for n in shape]


VOLUMES = {  # name -> (volume, iso, closed)
    "all_cases": lambda: (all_cases_volume(), 0.0, True),
    "random_3x3x3": lambda: (random_padded((3, 3, 3), 1), 0.0, True),
    "random_7x5x67": lambda: (random_padded((7, 5, 67), 2), 0.0, True),      # a z run longer than a wave
    "random_48x48x40": lambda: (random_padded((48, 48, 40), 3), 0.0, True),  # 411 workgroups: two chunks of the scan
    "exact_iso": lambda: (exact_iso_volume(), 0.0, True),
    "iso_0.25": lambda: (random_padded((6, 5, 9), 4), 0.25, True),
    "unpadded": lambda: (np.random.default_rng(6).standard_normal((6, 7, 9)).astype(np.float32), 0.0, False),
}


# ---- the stated semantics ---------------------------------------------------------------------------------------------
def expected_vertices(vol, iso, axes=None, shift=None):
    """(vertices float64 [NV, 3] in the stated order, keys int64 [NV] = 3 * owner's linear index + axis)."""
    if min(vol.shape) < 2:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int64)
    v64 = vol.astype(np.float64)
    iso = np.float64(iso)
    ins = v64 < iso
    lin = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    a64 = None if axes is None else [np.asarray(a, dtype=np.float32).astype(np.float64) for a in axes]
    pos, keys = [], []
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = ins[lo] != ins[hi]
        idx = np.argwhere(cross)  # the lower ends, in C order
        va, vb = v64[lo][cross], v64[hi][cross]
        t = (iso - va) / (vb - va)
        cols = []
        for k in range(3):
            i = idx[:, k]
            if k == axis:
                c = (i.astype(np.float64) + t) if a64 is None else (a64[k][i] + t * (a64[k][i + 1] - a64[k][i]))
            else:
                c = i.astype(np.float64) if a64 is None else a64[k][i]
            if shift is not None:
                c = c + np.float64(shift[k])
            cols.append(c)
        pos.append(np.stack(cols, axis=1))
        keys.append(lin[lo][cross] * 3 + axis)
    pos, keys = np.concatenate(pos), np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    return pos[order], keys[order]


def cell_cases(vol, iso):
    """int [nx-1, ny-1, nz-1]: bit dx + 2 dy + 4 dz = that corner is inside"""
    ins = vol.astype(np.float64) < np.float64(iso)
    nx, ny, nz = vol.shape
    c = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for b in range(8):
        dx, dy, dz = b & 1, (b >> 1) & 1, b >> 2
        c |= ins[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << b
    return c


def edge_owner_offset(e):
    """(axis, dx, dy, dz) of table edge(s) e = 4 axis + u + 2 v"""
    axis, u, v = e >> 2, e & 1, (e >> 1) & 1
    dx = np.where(axis == 0, 0, u)
    dy = np.where(axis == 0, u, np.where(axis == 1, 0, v))
    dz = np.where(axis == 2, 0, v)
    return axis, dx, dy, dz


def triangle_cells(vol, iso, ntris):
    """Per expected triangle: the linear index of its cell's lowest corner and its rank in the cell; cells ascending."""
    if min(vol.shape) < 2:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    nx, ny, nz = vol.shape
    cases = cell_cases(vol, iso)
    lin = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)[:-1, :-1, :-1]
    n = ntris[cases].ravel()
    cell = np.repeat(lin.ravel(), n)
    case = np.repeat(cases.ravel(), n)
    start = np.repeat(np.cumsum(n) - n, n)
    return cell, case, np.arange(len(cell), dtype=np.int64) - start


def expected_triangles(vol, iso, keys, edges, ntris):
    """The triangle list the table gives: int64 [NT, 3] vertex indices."""
    cell, case, rank = triangle_cells(vol, iso, ntris)
    nx, ny, nz = vol.shape
    vid = np.full(vol.size * 3, -1, dtype=np.int64)
    vid[keys] = np.arange(len(keys))
    tri = np.zeros((len(cell), 3), dtype=np.int64)
    for j in range(3):
        axis, dx, dy, dz = edge_owner_offset(edges[case, 3 * rank + j])
        tri[:, j] = vid[(cell + dx * ny * nz + dy * nz + dz) * 3 + axis]
    return tri


# ---- checks on a finished mesh ----------------------------------------------------------------------------------------
def check_triangles_in_cells(vol, iso, keys, tri, ntris):
    """NT = sum of ntris[case]; triangle k lies in the k-th expected cell (so cells never decrease): the owner of each of
    its three vertices is a corner of that cell with offset 0 along the edge's own axis."""
    cell, _, _ = triangle_cells(vol, iso, ntris)
    assert len(tri) == len(cell), f"{len(tri)} triangles, the cases give {len(cell)}"
    if not len(tri):
        return
    assert tri.min() >= 0 and tri.max() < len(keys)
    nx, ny, nz = vol.shape
    owner, axis = keys[tri] // 3, keys[tri] % 3  # [NT, 3]
    cx, cy, cz = cell // (ny * nz), (cell // nz) % ny, cell % nz
    d = np.stack([owner // (ny * nz) - cx[:, None], (owner // nz) % ny - cy[:, None], owner % nz - cz[:, None]], axis=-1)  # [NT, 3, 3]
    assert ((d == 0) | (d == 1)).all(), "a triangle vertex lies outside the triangle's cell"
    assert (np.take_along_axis(d, axis[..., None], axis=-1) == 0).all(), "a triangle vertex lies on no edge of the triangle's cell"
    assert (np.diff(cell) >= 0).all()


def directed_edges(tri, nv):
    t = np.asarray(tri, dtype=np.int64)
    a, b = t.ravel(), np.roll(t, -1, axis=1).ravel()
    return a * nv + b, b * nv + a


def check_closed(tri, nv):
    fwd, rev = directed_edges(tri, nv)
    assert len(np.unique(fwd)) == len(fwd), "a directed edge occurs twice"
    assert np.array_equal(np.sort(fwd), np.sort(rev)), "a directed edge has no reverse"


def signed_volume(vertices, tri):
    v = vertices[np.asarray(tri, dtype=np.int64)]
    return float(np.einsum("ni,ni->", v[:, 0], np.cross(v[:, 1], v[:, 2])) / 6.0)


def check_open(vol, keys, tri):
    """No directed edge twice; an edge without its reverse lies in a boundary face of the volume."""
    nv = len(keys)
    fwd, rev = directed_edges(tri, nv)
    assert len(np.unique(fwd)) == len(fwd), "a directed edge occurs twice"
    lone = fwd[~np.isin(fwd, rev)]
    a, b = lone // nv, lone % nv
    dims = np.array(vol.shape)
    in_face = np.zeros(len(lone), dtype=bool)
    for k in range(3):
        stride = int(np.prod(dims[k + 1:]))
        ca, cb = (keys[a] // 3 // stride) % dims[k], (keys[b] // 3 // stride) % dims[k]
        off_axis = (keys[a] % 3 != k) & (keys[b] % 3 != k)  # an edge along k leaves the face
        for side in (0, dims[k] - 1):
            in_face |= off_axis & (ca == side) & (cb == side)
    assert in_face.all(), "an unpaired edge lies inside the volume"
    return len(lone)
