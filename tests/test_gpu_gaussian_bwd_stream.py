"""GPU (MI355X): the streaming build of the per-Gaussian backward (csrc/preprocess.hip gaussian_bwd_kernel, WIDE = 3: each
workgroup's records pass through a two-stage LDS ring in chunks of GB_CHUNK = 256, fetched as consecutive 16-byte-per-lane
loads) against the three gather builds. Every build adds the same records in the same order, so every gradient tensor and
grad_viewmatrix must be the same BITS (compared as integers: no tolerance, which would hide a wrong order). EOGS_GB_WIDE is
read once per process: one child process per forced value 0, 1, 2, 3 runs all cases, one child at a time
(tests/gb_stream_child.py); the cases are built here once, and the scenes whose workgroup regions must end on, one short of
and one past a chunk boundary are put together from per-Gaussian record counts measured by forwards of this process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK, COOP, STAGES = 256, 64, 2  # csrc/common.h GB_CHUNK, csrc/preprocess.hip GB_COOP, the ring's stages
PER_G = ("means3D", "scales", "rotations", "opacities", "colors")
BOUNDARY = {"chunk_exact": 4 * CHUNK, "chunk_short": 4 * CHUNK - 1, "chunk_past": 4 * CHUNK + 1}
CASES = ("odd_p_interleaved", "empty_region", *BOUNDARY, "opaque", "altitude_only", "raw_params", "range_split", "nofit")


def _scene(P, H, W, seed, opacity, **kw):
    from eogs2_amd.synthetic import make_scene

    return {k: v.numpy() for k, v in make_scene(P, H, W, seed=seed, opacity=opacity, **kw).items()}


def _cull(sc, idx):
    sc["means3D"][idx, :2] = 40.0  # far outside the image: radii 0, no listed tile


def _take(sc, idx):
    return {k: (v[idx] if k in PER_G else v) for k, v in sc.items()}


def _cat(parts):
    return {k: (np.concatenate([p[k] for p in parts]) if k in PER_G else parts[0][k]) for k in parts[0]}


def _slots(sc, H, W, dev):
    """record slots (listed (tile, Gaussian) pairs) of a forward of `sc`: the count the library reads back"""
    from eogs2_amd import GaussianRasterizer
    from eogs2_amd.rasterizer import last_exact_token
    from eogs2_amd.synthetic import settings_for

    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sc.items()}
    P = t["means3D"].shape[0]
    with torch.no_grad():
        GaussianRasterizer(settings_for(t, H, W))(t["means3D"], torch.zeros(P, 3, device=dev), t["opacities"],
                                                  colors_precomp=t["colors"], scales=t["scales"], rotations=t["rotations"])
    torch.cuda.synchronize()
    return int(last_exact_token(dev)) & 0x7FFFFFFF


def _boundary_cases(dev):
    """Three scenes of 256 + 256 + 4133 Gaussians on 192 x 192 whose SECOND workgroup's region of record slots is exactly
    4 x 256, one fewer and one more: more chunks than the ring has stages, ending on, one short of and one past a chunk
    boundary. The workgroup holds three Gaussians beyond GB_COOP listed tiles, culled Gaussians in between, and is followed
    by a crowd that makes the last workgroup partial and, by its opacity, decides flags (0.9: mean list depth x opacity far
    beyond NOFLAG_K = 24, csrc/common.h noflag_scene) or flag-free records (0.01). Which tiles a Gaussian lists depends on
    its opacity (the box of alpha >= 1/255), so the counts are measured at the opacity of the case."""
    H = W = 192
    g = np.random.default_rng(5)
    npool, nbig, nord = 330, 6, 204  # big, ordinary, within one tile
    px = 2.0 / W  # one pixel in the units of `scales`
    cases = {}
    for (name, target), opacity in zip(BOUNDARY.items(), (0.01, 0.9, 0.3)):
        reach = min(3.0, float(np.sqrt(2.0 * np.log(255.0 * opacity))))  # footprint half-width in sigmas
        pool = _scene(npool, H, W, 11, opacity)
        sig = np.concatenate([np.full(nbig, 50.0 / reach), np.full(nord, 6.0 / reach), np.full(npool - nbig - nord, 0.15)])
        pool["scales"] = (px * sig[:, None] * np.exp(0.2 * g.standard_normal((npool, 3)))).astype(np.float32)
        n = np.array([_slots(_take(pool, [i]), H, W, dev) for i in range(npool)])
        big = sorted((i for i in range(nbig) if n[i] > COOP), key=lambda i: n[i])[:3]
        assert len(big) == 3, n[:nbig]
        ones = [i for i in range(nbig + nord, npool) if n[i] == 1]
        shared = {k: v for k, v in pool.items() if k not in PER_G}  # one camera, background and upstream gradient for all parts
        head = dict(_scene(256, H, W, 12, opacity, scale_mult=0.25), **shared)
        crowd = dict(_scene(4133, H, W, 13, opacity, scale_mult=0.6), **shared)
        chosen, total = list(big), int(n[big].sum())
        for i in range(nbig, nbig + nord):
            if n[i] and total + n[i] <= target - 8 and len(chosen) < 200:
                chosen.append(i)
                total += int(n[i])
        fill = ones[:target - total]
        chosen, total = [int(i) for i in g.permutation(chosen + fill)], total + len(fill)
        assert total == target and len(chosen) <= 240, (name, total, len(chosen), n[:nbig])
        order = g.permutation(256)  # where the chosen Gaussians stand among the workgroup's 256: the rest are culled
        live_at, dead = np.sort(order[:len(chosen)]), np.sort(order[len(chosen):])
        mid = _take(pool, np.resize(np.array(chosen), 256))
        for k in PER_G:
            mid[k][live_at] = pool[k][chosen]
        _cull(mid, dead)
        sc = _cat([head, mid, crowd])
        # from the counts: the middle workgroup alone lists `target` slots, and the whole scene those of its three parts
        assert _slots(mid, H, W, dev) == target, name
        total_all = _slots(sc, H, W, dev)
        assert total_all == _slots(head, H, W, dev) + target + _slots(crowd, H, W, dev), name
        assert (target + CHUNK - 1) // CHUNK > STAGES and sc["means3D"].shape[0] % 256 != 0
        ntiles = ((H + 7) // 8) * ((W + 7) // 8)
        if opacity == 0.9:
            assert round(64 * 0.9) * total_all > 64 * 24 * ntiles, "flags on"
        if opacity == 0.01:
            assert round(64 * 0.01) * total_all <= 64 * 24 * ntiles, "flag-free"
        cases[name] = (sc, H, W)
    return cases


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda:0")
    d = tmp_path_factory.mktemp("gb_stream")
    case_dir = os.path.join(str(d), "cases")
    os.makedirs(case_dir)
    cases = {}
    sc = _scene(3001, 160, 192, 1, "init", scale_mult=2.0)  # P no multiple of 256; every third Gaussian culled; flag-free
    _cull(sc, np.arange(0, 3001, 3))
    cases["odd_p_interleaved"] = ("plain", sc, 160, 192)
    sc = _scene(805, 128, 128, 2, "init", scale_mult=2.0)  # an empty region between two full ones
    _cull(sc, np.arange(256, 512))
    cases["empty_region"] = ("plain", sc, 128, 128)
    bound = _boundary_cases(dev)
    for name, (sc, H, W) in bound.items():
        cases[name] = ("plain", sc, H, W)
    cases["opaque"] = ("plain", _scene(6000, 128, 128, 3, "trained", scale_mult=2.0), 128, 128)  # flags on, dead pairs
    cases["altitude_only"] = ("alt", _scene(5000, 160, 136, 4, "trained", scale_mult=2.0), 160, 136)
    cases["raw_params"] = ("raw", _scene(3001, 136, 160, 5, "init", scale_mult=2.0), 136, 160)
    cases["range_split"] = ("range", bound["chunk_short"][0], 192, 192)
    small = _scene(3000, 128, 128, 6, "trained", scale_mult=0.4)
    cases["nofit"] = ("nofit", _scene(3000, 128, 128, 7, "trained", scale_mult=3.0), 128, 128)
    assert set(cases) == set(CASES)
    for name, (kind, sc, H, W) in cases.items():
        extra = {"small_" + k: v for k, v in small.items()} if kind == "nofit" else {}
        np.savez(os.path.join(case_dir, name + ".npz"), kind=kind, H=H, W=W, **sc, **extra)
    out = {}
    for wide in (0, 1, 2, 3):  # one child at a time
        o = os.path.join(str(d), f"wide{wide}")
        os.makedirs(o)
        r = subprocess.run([sys.executable, os.path.join(HERE, "gb_stream_child.py"), case_dir, o],
                           env=dict(os.environ, EOGS_GB_WIDE=str(wide)), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"EOGS_GB_WIDE={wide}: {r.stderr[-3000:]}"
        out[wide] = {}
        for name in CASES:
            z = np.load(os.path.join(o, name + ".npz"))
            out[wide][name] = {k: z[k] for k in z.files}
    return out, {name: c[1] for name, c in cases.items()}


@pytest.mark.parametrize("name", CASES)
def test_streaming_build_adds_the_same_bits(results, name):
    out, scenes = results
    stream = out[3][name]
    grads = [k for k in stream if k.startswith("g_")]
    assert "g_viewmatrix" in grads and len(grads) >= 6, grads
    if name != "raw_params":  # (the raw-parameter entry hands no token back to ask with)
        assert all(int(out[w][name]["_build"]) == w for w in out), "each child ran its forced build"
    radii = stream["out_radii"]
    if name == "odd_p_interleaved":
        assert not radii[0::3].any() and radii[1::3].any() and radii[2::3].any() and radii.shape[0] % 256 != 0
    if name == "empty_region":
        assert not radii[256:512].any() and radii[:256].any() and radii[512:].any()
    if name != "nofit":  # (an altitude-only render has no gradient for the other colours; everything else is nonzero)
        assert sum(bool(np.abs(stream[k]).max() > 0) for k in grads) >= len(grads) - 1, grads
    for k in grads:
        bits = stream[k].view(np.uint32)
        if name == "nofit":
            assert not (stream[k] != 0).any(), f"{k}: a forward that did not fit its capacity token has zero gradients"
        for w in (0, 1, 2):
            d = out[w][name][k].view(np.uint32) != bits
            print(f"{name}: {k}: build 3 against build {w}: {int(d.sum())} of {d.size} elements differ in bits")
            assert not d.any(), f"{k}: the streaming build differs from build {w} in {int(d.sum())} of {d.size} elements"
