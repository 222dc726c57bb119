"""CPU: the committed marching-cubes case table (eogs2_amd/csrc/mesh_table.h, read through eogs_mesh_case) against the face
rule of include/eogs_mesh.h, derived here from the cube's geometry, independently of tools/gen_mesh_table.py; and the
table run through the numpy restatement of tests/mesh_cases.py gives closed, outward-oriented meshes."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CORNERS = [np.array([b & 1, (b >> 1) & 1, b >> 2]) for b in range(8)]  # b = dx + 2 dy + 4 dz


def edge_ends(e):
    """the two corner numbers of edge e = 4 axis + u + 2 v"""
    axis, uv = e // 4, [e & 1, (e >> 1) & 1]
    lo = [0, 0, 0]
    for k in range(3):
        if k != axis:
            lo[k] = uv.pop(0)
    hi = list(lo)
    hi[axis] = 1
    return lo[0] + 2 * lo[1] + 4 * lo[2], hi[0] + 2 * hi[1] + 4 * hi[2]


ENDS = [edge_ends(e) for e in range(12)]
EDGE_OF = {frozenset(p): e for e, p in enumerate(ENDS)}
FACES = [(k, s) for k in range(3) for s in (0, 1)]


def faces_of_edge(e):
    a, b = ENDS[e]
    return {(k, s) for k, s in FACES if CORNERS[a][k] == s and CORNERS[b][k] == s}


def ccw_corners(face):
    """The four corners of a face, counter-clockwise for a viewer outside the cube: sorted by the angle in a right-handed
    frame (p, q, n) whose n is the face's outward normal."""
    k, s = face
    n = np.zeros(3)
    n[k] = 1.0 if s else -1.0
    p = np.zeros(3)
    p[(k + 1) % 3] = 1.0
    q = np.cross(n, p)
    centre = np.full(3, 0.5)
    centre[k] = s
    on = [b for b in range(8) if CORNERS[b][k] == s]
    return sorted(on, key=lambda b: np.arctan2((CORNERS[b] - centre) @ q, (CORNERS[b] - centre) @ p))


def rule_segments(case, face):
    """{(from edge, to edge)}: one per maximal run of inside corners on the walk, from where it is entered to where it is left"""
    ring = ccw_corners(face)
    ins = [(case >> b) & 1 for b in ring]
    out = set()
    if all(ins) or not any(ins):
        return out
    for i in range(4):
        if ins[i] and not ins[i - 1]:
            j = i
            while ins[(j + 1) % 4]:
                j += 1
            out.add((EDGE_OF[frozenset((ring[i - 1], ring[i]))], EDGE_OF[frozenset((ring[j % 4], ring[(j + 1) % 4]))]))
    return out


@pytest.fixture(scope="module")
def table():
    return K.load_table()


def triangles_of(table, case):
    edges, ntris = table
    return [tuple(int(e) for e in edges[case, 3 * k:3 * k + 3]) for k in range(int(ntris[case]))]


def directed(tris):
    return [(t[j], t[(j + 1) % 3]) for t in tris for j in range(3)]


def test_rows_are_well_formed(table):
    edges, ntris = table
    assert ntris.max() == 5 and ntris.sum() == 820 and ntris[0] == ntris[255] == 0
    for c in range(256):
        n = int(ntris[c])
        assert (edges[c, :3 * n] >= 0).all() and (edges[c, :3 * n] < 12).all() and (edges[c, 3 * n:] == -1).all(), c


def test_every_crossing_edge_and_no_other(table):
    for c in range(256):
        crossing = {e for e in range(12) if ((c >> ENDS[e][0]) ^ (c >> ENDS[e][1])) & 1}
        used = {e for t in triangles_of(table, c) for e in t}
        assert used == crossing, c
        assert all(len(set(t)) == 3 for t in triangles_of(table, c)), c


def test_face_edges_are_the_rule_segments_and_diagonals_pair_up(table):
    """A triangle edge whose two crossings share a cube face is a segment of the face rule, with its direction, and every
    segment occurs once (so no fan diagonal lies in a face); every other triangle edge occurs once in each direction."""
    for c in range(256):
        segs = [s for f in FACES for s in rule_segments(c, f)]
        assert len(set(segs)) == len(segs), c
        on_face, interior = [], []
        for a, b in directed(triangles_of(table, c)):
            (on_face if faces_of_edge(a) & faces_of_edge(b) else interior).append((a, b))
        assert sorted(on_face) == sorted(segs), c
        assert len(set(interior)) == len(interior), c
        assert sorted(interior) == sorted((b, a) for a, b in interior), c


def test_neighbours_agree_on_the_shared_face(table):
    """The cell across face (k, 1) sees the same four corners on its face (k, 0): whatever its other four corners are, its
    triangle edges in that face are this case's, reversed."""
    for k in range(3):
        mirror = {e: EDGE_OF[frozenset(b - (1 << k) for b in ENDS[e])] for e in range(12) if (k, 1) in faces_of_edge(e)}
        far = [b for b in range(8) if CORNERS[b][k] == 1]
        for c in range(256):
            mine = sorted((a, b) for a, b in directed(triangles_of(table, c)) if (k, 1) in faces_of_edge(a) & faces_of_edge(b))
            shared = sum(((c >> b) & 1) << (b - (1 << k)) for b in far)
            for rest in itertools.product((0, 1), repeat=4):
                n = shared + sum(bit << b for bit, b in zip(rest, far))
                theirs = sorted((b, a) for a, b in directed(triangles_of(table, n)) if (k, 0) in faces_of_edge(a) & faces_of_edge(b))
                assert theirs == sorted((mirror[a], mirror[b]) for a, b in mine), (k, c, n)


def mesh_of(vol, iso, table):
    vertices, keys = K.expected_vertices(vol, iso)
    return vertices, keys, K.expected_triangles(vol, iso, keys, *table)


def test_every_case_alone_closes_with_positive_volume(table):
    vol = K.all_cases_volume()
    vertices, keys, tri = mesh_of(vol, 0.0, table)
    K.check_triangles_in_cells(vol, 0.0, keys, tri, table[1])
    K.check_closed(tri, len(keys))
    # per 4 x 4 x 4 block: the blocks are separate surfaces, each encloses its inside corners
    block = (keys[tri[:, 0]] // 3 // (64 * 4) // 4) * 16 + ((keys[tri[:, 0]] // 3 // 4) % 64) // 4
    v = vertices[tri]
    vol6 = np.einsum("ni,ni->n", v[:, 0], np.cross(v[:, 1], v[:, 2]))
    per_block = np.bincount(block, weights=vol6, minlength=256) / 6.0
    assert (per_block[1:] > 0).all() and per_block[0] == 0


def test_random_volumes_close(table):
    g = np.random.default_rng(0)
    for trial in range(200):
        dims = tuple(int(d) for d in g.integers(2, 8, 3))
        vol = K.padded(g.standard_normal(dims).astype(np.float32))
        vertices, keys, tri = mesh_of(vol, 0.0, table)
        ins = vol < 0
        assert len(keys) == sum(int((np.diff(ins.astype(np.int8), axis=a) != 0).sum()) for a in range(3))
        assert (tri >= 0).all()
        K.check_closed(tri, len(keys))
        assert K.signed_volume(vertices, tri) > 0, trial
    vol, iso, _ = K.VOLUMES["unpadded"]()
    vertices, keys, tri = mesh_of(vol, iso, table)
    assert K.check_open(vol, keys, tri) > 0


def test_committed_header_is_the_generators_output():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mesh_table.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
