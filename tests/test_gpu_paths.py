"""GPU (MI355X): (1) every render kernel variant against the ORACLE — the library picks list granularity and render
kernel per forward, so the golden, seeded and randomised cases are replayed in child processes
with each path forced through the tuning switches, the path actually taken is read back (eogs_rast_path_info) and the
test asserts that every kernel x {forward, backward} was oracle-compared; (2) BASELINE.json's configurations at their
own sizes: the headline 1 M / 1024^2 and config 2 (300 k / 800^2) against the C oracle in full, config 3 (learnable
camera + a grid_sample-warped loss gradient) against the oracle, config 4's per-rank workload (2 M / 1024^2) through
size-independent properties."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from parity_cases import SEEDED, compare, seeded_case, sweep_case
from util import GOLDEN, load_golden, run_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# name -> environment. The switches are thresholds in listed tiles per Gaussian (csrc/api.hip, csrc/render.hip).
FORCED = {  # (the default switches run in-process: tests/test_gpu_parity.py, same cases, same comparison)
    # (EOGS_TILE_SCHED=0 here: the band mapping of rounds 1-3 instead of the tile schedule — no descriptors, and block_lists_kernel
    # finds its block's start by summing the counts of the blocks before it instead of reading the schedule workgroup's prefixes)
    "tile": {"EOGS_BLOCK_SWITCH": "1000", "EOGS_DEPTH_SWITCH": "0", "EOGS_QUAD_SWITCH": "0", "EOGS_QUAD_BWD_SWITCH": "0",
             "EOGS_TILE_SCHED": "0"},
    "block": {"EOGS_BLOCK_SWITCH": "0.5", "EOGS_DEPTH_SWITCH": "0.001"},
    # (EOGS_NOFLAG=0: the quad backward with live flags on every case; the next entry forces its flag-free records on every case —
    # correct for any scene, chosen by default only where no tile comes near saturation: csrc/common.h noflag_scene)
    "quad": {"EOGS_BLOCK_SWITCH": "1000", "EOGS_DEPTH_SWITCH": "0", "EOGS_QUAD_SWITCH": "1000", "EOGS_QUAD_BWD_SWITCH": "1000",
             "EOGS_NOFLAG": "0"},
    "quad_noflag": {"EOGS_BLOCK_SWITCH": "1000", "EOGS_DEPTH_SWITCH": "0", "EOGS_QUAD_SWITCH": "1000", "EOGS_QUAD_BWD_SWITCH": "1000",
                    "EOGS_NOFLAG": "2", "EOGS_PLAIN_TRIPS": "0"},
    # A forward of one per-tile kernel with the backward of the other: the two read separate switches (EOGS_QUAD_SWITCH,
    # EOGS_QUAD_BWD_SWITCH), and n_contrib means something different per kernel — 1 + the last blended position (tile forward),
    # the position of the stop entry or 0xFFFFFFFF (quad forward); both backwards read it as "positions >= n_contrib take no part",
    # which both values satisfy (csrc/render.hip). The quad backward after a tile forward finds its quad masks itself.
    "tile_fwd_quad_bwd": {"EOGS_BLOCK_SWITCH": "1000", "EOGS_DEPTH_SWITCH": "0", "EOGS_QUAD_SWITCH": "0", "EOGS_QUAD_BWD_SWITCH": "1000"},
    "quad_fwd_tile_bwd": {"EOGS_BLOCK_SWITCH": "1000", "EOGS_DEPTH_SWITCH": "0", "EOGS_QUAD_SWITCH": "1000", "EOGS_QUAD_BWD_SWITCH": "0"},
}
# (Rounds 2-5 also forced two matrix-pipe variants of the quad backward and, for image-sized Gaussians, a separate back-to-front
# kernel; since round 6 every backward kernel walks back to front — the reference's recursion — and the variants are gone.)
KERNEL_NAMES = {0: "tile", 1: "block", 2: "quad", 6: "quad_alt"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def _oracle(case):
    from parity_cases import oracle_run

    return oracle_run(case)


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    """Inputs + oracle results of the golden fixtures, the seeded table and the 24-seed sweep, one .npz each."""
    d = tmp_path_factory.mktemp("path_cases")
    cases = []
    for name in GOLDEN:
        c = load_golden(name)
        ins = {k: v for k, v in c.items() if not k.startswith(("out_", "g_"))}
        cases.append((f"golden_{name}", name, ins, {k: v for k, v in c.items() if k.startswith(("out_", "g_"))}))
    for row in SEEDED:
        c, label = seeded_case(*row)
        cases.append((f"seeded_{label}", label, c, None))
    # (every second seed of the 24-seed sweep unless EOGS_FULL=1: the default path runs all 24 in tests/test_gpu_parity.py; the forced
    # paths' share of the suite was 60-90 s of 300, box to box)
    for seed in (range(200, 224) if os.environ.get("EOGS_FULL") == "1" else range(200, 224, 2)):
        c, label = sweep_case(seed)
        cases.append((f"sweep_{seed}", label, c, None))
    from parity_cases import oracle_cached

    for fname, label, ins, ref in cases:
        ref = ref if ref is not None else oracle_cached(fname, ins)  # (shared with tests/test_gpu_parity.py in this process)
        np.savez(os.path.join(str(d), fname + ".npz"), label=label, **{"in_" + k: v for k, v in ins.items()},
                 **{"ref_" + k: v for k, v in ref.items()})
    return str(d), len(cases)


def test_every_kernel_path_matches_oracle(dev, case_dir, tmp_path):
    d, ncases = case_dir
    seen_fwd, seen_bwd, report = set(), set(), {}
    # One child first, then the others together (each is one process on the card and mostly CPU-side comparison; the GPU box
    # allows six processes on its card and has 16 cores): what the float64 arbiter needs for a case depends on the case alone
    # and is cached in files the children share, so the first child pays for it and the others read it (all four at once
    # computed it four times: 95 s against 78 s two by two). Exactly the processes started here are waited for.
    tags, procs = list(FORCED), {}
    for group in (tags[:1], tags[1:]):
        for tag in group:
            out = os.path.join(str(tmp_path), f"{tag}.json")
            procs[tag] = (subprocess.Popen([sys.executable, os.path.join(HERE, "path_child.py"), d, out],
                                           env=dict(os.environ, **FORCED[tag]), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), out)
        for tag in group:
            try:
                _, err = procs[tag][0].communicate(timeout=1500)
            except subprocess.TimeoutExpired:
                for q, _o in procs.values():
                    if q.poll() is None:
                        q.kill()
                raise
            assert procs[tag][0].returncode == 0, f"{tag}: {err[-2000:]}"
    for tag, env_extra in FORCED.items():
        out = procs[tag][1]
        res = json.load(open(out))
        assert len(res) == ncases
        bad = {k: v["error"] for k, v in res.items() if not v["ok"]}
        assert not bad, f"path '{tag}': {len(bad)} of {ncases} cases differ from the oracle: {json.dumps(bad)[:3000]}"
        paths = [tuple(v["path"]) for v in res.values() if v["path"][1] >= 0]
        report[tag] = {"fwd": sorted({KERNEL_NAMES[p[1]] for p in paths}), "bwd": sorted({KERNEL_NAMES[p[2]] for p in paths}),
                       "flips": sum(v["flips"] for v in res.values())}
        # a forced configuration really takes its path on every non-empty case
        if tag == "tile":
            assert all(p == (8, 0, 0) for p in paths), report[tag]
        if tag == "block":
            assert all(p[1] == 1 and p[2] == 1 for p in paths if p[0] == 32), report[tag]
            assert sum(p[0] == 32 for p in paths) >= len(paths) * 0.8, report[tag]
        if tag in ("quad", "quad_noflag"):  # (quad_noflag also switches the forward's plain chunks off: its general loop on every case)
            assert all(p == (8, 2, 2) for p in paths), report[tag]
        if tag == "tile_fwd_quad_bwd":
            assert all(p == (8, 0, 2) for p in paths), report[tag]
        if tag == "quad_fwd_tile_bwd":
            assert all(p == (8, 2, 0) for p in paths), report[tag]
        seen_fwd |= {p[1] for p in paths}
        seen_bwd |= {p[2] for p in paths}
    print("kernel paths compared with the oracle:", json.dumps(report))
    assert seen_fwd == {0, 1, 2}, report
    assert seen_bwd == {0, 1, 2}, report


def _full_size_case(P, H, W, seed, opacity, **kw):
    from eogs2_amd.synthetic import make_scene

    sc = make_scene(P, H, W, seed=seed, opacity=opacity, **kw)
    case = {k: v.numpy() for k, v in sc.items()}
    case.update(H=H, W=W, antialiasing=False)
    return case


def test_headline_1M_1024_matches_oracle(dev):
    """BASELINE.json's headline configuration, every output and every gradient against the C oracle (16 s of CPU)."""
    from eogs2_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib

    import time

    from parity_cases import prefetch_nudges

    case = _full_size_case(1 << 20, 1024, 1024, 0, "init")
    prefetch_nudges(case)  # the two uniform nudged runs beside the un-nudged one: 100 s -> 50 s of wall time
    got = run_case(case, dev, GaussianRasterizer, GaussianRasterizationSettings)
    assert _lib.get().path_info(1 << 20, got["_num_rendered"]) == (8, 2, 2)  # the bench's kernels
    t0 = time.perf_counter()
    ref = _oracle(case)
    print(f"oracle at 1M / 1024^2: {time.perf_counter() - t0:.1f} s")
    flips = compare(got, ref, "headline", case)
    print("headline 1M/1024^2: attributed out-of-tolerance elements:", flips)


@pytest.mark.parametrize("name,P,S,opacity", [
    ("trained_1M_1024", 1 << 20, 1024, "trained"),
    ("opacity0.1_1M_1024", 1 << 20, 1024, 0.1),
    ("opacity0.01_1M_2048", 1 << 20, 2048, "init"),  # the sun camera's size (row-span listing)
    ("opacity0.1_2M_1024", 2_000_000, 1024, 0.1),
    ("config4_2M_1024", 2_000_000, 1024, "trained"),
    # the trained-scene SHAPE (synthetic.py kind="surface": flat disks on a terrain, log-normal sizes, bimodal opacities)
    ("surface_300k_800", 300_000, 800, "surface"),
    ("surface_1M_1024", 1 << 20, 1024, "surface"),
    ("surface_2M_1024", 2_000_000, 1024, "surface")])
def test_regimes_of_the_bench_line_match_oracle(dev, name, P, S, opacity):
    """Every regime bench.py reports beside the headline (bench.regime_scan), at its own size, in full against the C oracle:
    trained opacities (tiles saturate, most listed pairs dead: the backward's flags-first record sum), opacity 0.1 (lists twice
    as long, nothing saturates), the 2048^2 sun-camera size (row-span listing), 2 M Gaussians at opacity 0.1 — and configs[3]'s
    per-rank workload (IARPA_001 class: 2 M Gaussians, trained opacities, one 1024^2 view). In the default suite since the
    oracle's per-pixel loops use the host's cores (8-33 s each; minutes before); outcomes in profiles/r04_sweeps.txt."""
    from eogs2_amd import GaussianRasterizationSettings, GaussianRasterizer
    from parity_cases import prefetch_nudges

    case = _full_size_case(P, S, S, 8 if name.startswith("config4") else 0, opacity)
    prefetch_nudges(case)
    got = run_case(case, dev, GaussianRasterizer, GaussianRasterizationSettings)
    flips = compare(got, _oracle(case), name, case)
    print(f"{name}: attributed out-of-tolerance elements: {flips}")


def test_mixed_scale_scene(dev):
    """A million-small-Gaussians scene that ALSO holds a few hundred image-sized opaque ones (ground splats of a trained scene):
    300 k Gaussians at the synthetic statistics, trained opacities, 800 x 800, plus 200 Gaussians of sigma = 5-30 % of the image
    with opacity 0.9-0.99 at altitudes throughout the box — deep lists under opaque fronts in EVERY tile while the per-forward
    averages (listed tiles per Gaussian, list depth) stay those of an ordinary scene. Rounds 3-5 chose the backward's dL/dalpha
    formulation by such an average and would have missed this composition; every backward kernel is the reference's
    back-to-front recursion now (csrc/render.hip). Full compare with the oracle, on the kernels the defaults pick."""
    from eogs2_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib
    from parity_cases import prefetch_nudges

    P, S, big = 300_000, 800, 200
    case = _full_size_case(P, S, S, 5, "trained")
    g = np.random.default_rng(55)
    idx = g.choice(P, big, replace=False)
    sig_px = S * g.uniform(0.05, 0.30, (big, 1))
    case["scales"][idx] = (sig_px / (0.5 * S) * np.exp(0.2 * g.standard_normal((big, 3)))).astype(np.float32)
    case["opacities"][idx] = g.uniform(0.9, 0.99, (big, 1)).astype(np.float32)
    prefetch_nudges(case)
    got = run_case(case, dev, GaussianRasterizer, GaussianRasterizationSettings)
    info = _lib.get().path_info(P, got["_num_rendered"])
    print("mixed-scale scene: pairs", got["_num_rendered_exact"] & 0x7FFFFFFF, "path", info)
    flips = compare(got, _oracle(case), "mixed_scale", case)
    print(f"mixed_scale: attributed out-of-tolerance elements: {flips}")


def test_config2_300k_800_matches_oracle(dev):
    """configs[1] (JAX_004 class): ~300 k Gaussians, 800 x 800, trained opacities, in full against the oracle."""
    from eogs2_amd import GaussianRasterizationSettings, GaussianRasterizer

    from parity_cases import prefetch_nudges

    case = _full_size_case(300_000, 800, 800, 4, "trained")
    prefetch_nudges(case)
    got = run_case(case, dev, GaussianRasterizer, GaussianRasterizationSettings)
    compare(got, _oracle(case), "config2", case)


def test_config3_camera_gradient_with_warped_loss(dev):
    """configs[2] (JAX_068 class): the view matrix is a leaf (camera refinement, renderer.py:47-53) and the loss reaches
    the render through a grid_sample warp (flowmatching/flow_matching.py:225-253), so dL/dcolor is a resampled field
    rather than white noise. 300 k Gaussians / 800^2, HIP vs oracle through the same autograd graph."""
    import torch.nn.functional as F

    import oracle
    from eogs2_amd import GaussianRasterizer, _lib
    from eogs2_amd.synthetic import make_scene, settings_for

    P, H, W = 300_000, 800, 800
    sc = make_scene(P, H, W, seed=6, opacity="trained")
    g = torch.Generator().manual_seed(6)
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    flow = 0.02 * torch.randn(2, 8, 8, generator=g)
    flow = F.interpolate(flow[None], size=(H, W), mode="bilinear", align_corners=True)[0]
    grid = torch.stack([xs + flow[0], ys + flow[1]], dim=-1)[None]
    target = torch.rand(3, H, W, generator=g)

    def run(device):
        to = lambda t: t.to(device)
        leaves = {k: to(sc[k]).clone().requires_grad_(True) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
        vm = to(sc["viewmatrix"]).clone().requires_grad_(True)
        rs = settings_for({k: to(v) for k, v in sc.items()}, H, W)._replace(viewmatrix=vm, projmatrix=vm.detach())
        m2 = torch.zeros(P, 3, device=device, requires_grad=True)
        color, radii, _ = GaussianRasterizer(rs)(leaves["means3D"], m2, leaves["opacities"], colors_precomp=leaves["colors"],
                                                 scales=leaves["scales"], rotations=leaves["rotations"])
        warped = F.grid_sample(color[None, :3], to(grid), mode="bilinear", padding_mode="border", align_corners=True)[0]
        loss = (warped - to(target)).abs().mean() + 1e-3 * color[3:].mean()
        loss.backward()
        out = dict(out_color=color.detach(), out_radii=radii, out_invdepth=torch.zeros(1, H, W),
                   g_means2D=m2.grad, g_viewmatrix=vm.grad)
        out.update({"g_" + k: v.grad for k, v in leaves.items()})
        return out

    got = run(dev)
    hip = _lib.get
    _lib.get = oracle.abi
    try:
        ref = run(torch.device("cpu"))
    finally:
        _lib.get = hip
    case = {k: v.numpy() for k, v in sc.items()}
    case.update(H=H, W=W, antialiasing=False)
    got.pop("out_invdepth"), ref.pop("out_invdepth")
    assert float(ref["g_viewmatrix"].abs().max()) > 0
    compare(got, {k: v.cpu().numpy() for k, v in ref.items()}, "config3", case)


@pytest.mark.slow  # (round 4: the same workload is compared with the oracle in full by the default suite —
#                     test_regimes_of_the_bench_line_match_oracle[config4_2M_1024]; these properties run with EOGS_FULL=1)
def test_config4_2M_1024_properties(dev):
    """configs[3]'s per-rank workload (IARPA_001 class: 2 M Gaussians, one 1024^2 view per rank): finite outputs,
    backward linear in dL/dcolor, zero gradient for invisible Gaussians, accumulated opacity in [0, 1], and a 64 x 64
    crop of the image against the dense renderer."""
    from eogs2_amd import GaussianRasterizer
    from eogs2_amd.synthetic import make_scene, settings_for
    from oracle.torch_dense import render_dense
    from util import assert_close

    P, H, W = 2_000_000, 1024, 1024
    sc = make_scene(P, H, W, seed=8, opacity="trained", device=dev)
    rs = settings_for(sc, H, W)

    def fwd_bwd(scale):
        leaves = {k: sc[k].clone().requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "colors")}
        color, radii, _ = GaussianRasterizer(rs)(leaves["means3D"], torch.zeros(P, 3, device=dev), leaves["opacities"],
                                                 colors_precomp=leaves["colors"], scales=leaves["scales"],
                                                 rotations=leaves["rotations"])
        torch.autograd.backward([color], [scale * sc["dL_dcolor"]])
        return color.detach(), radii, {k: v.grad for k, v in leaves.items()}

    c1, radii, g1 = fwd_bwd(1.0)
    _, _, g3 = fwd_bwd(3.0)
    assert torch.isfinite(c1).all()
    for k in g1:
        assert torch.isfinite(g1[k]).all()
        assert_close(g3[k], 3.0 * g1[k], f"2M linearity:{k}", allow_flips=False)
        assert float(g1[k][radii == 0].abs().sum()) == 0.0, k
    assert float(c1[4].min()) >= -1e-6 and float(c1[4].max()) <= 1 + 1e-5
    c = {k: v.cpu() for k, v in sc.items()}
    y0, x0, S = 512, 256, 64
    crop = render_dense(c["means3D"], c["opacities"], c["colors"], c["bg"], c["viewmatrix"], H, W, scales=c["scales"],
                        rotations=c["rotations"], block=64, crop=(y0, x0, S, S))[0]
    assert_close(c1[:, y0:y0 + S, x0:x0 + S], crop, "2M crop")


def test_image_sized_gaussians_take_the_same_kernels_as_everything_else(dev):
    """Rounds 3-5 switched forwards whose Gaussians list a few per cent of the image's tiles each to a separate back-to-front
    backward (a tuned threshold on a per-forward average; token bit 60). Every backward kernel now IS the reference's
    back-to-front recursion (csrc/render.hip), so such a forward takes the ordinary kernels — block lists here — and holds
    1e-4 against the oracle with them; so does the quad backward forced onto it (tests/test_gpu_paths.py FORCED, every case)."""
    from eogs2_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib
    from parity_cases import compare, oracle_run, seeded_case

    abi = _lib.get()
    big, label = seeded_case(400, 200, 168, 15, "trained", 14.0, False, False)   # rects > 64 internal tiles each
    got = run_case(big, dev, GaussianRasterizer, GaussianRasterizationSettings)
    assert abi.path_info(400, got["_num_rendered"]) == (32, 1, 1)
    compare(got, oracle_run(big), label, big)
    small, label = seeded_case(5000, 160, 208, 10, "init", 2.0, False, False)
    got = run_case(small, dev, GaussianRasterizer, GaussianRasterizationSettings)
    assert abi.path_info(5000, got["_num_rendered"]) == (8, 2, 2)
    compare(got, oracle_run(small), label, small)
