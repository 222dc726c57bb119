"""The per-iteration draws on one GPU (eogs2_amd.draw) against what they replace, on the same card:

  draw      one `IterationDraws.draw()` for two cameras, each with a random background and a sampled virtual camera: one
            launch, no wait, against
  torch     the same two cameras by the reference's recipe as torch operations (train_pan.py:272-277 and
            affine_cameras.py:403-430 restated: `torch.rand(5)`, the altitude bound through `.item()`, the sheared affine put
            together in a CPU tensor from device operands and sent back): about twenty small launches and two waits per camera;
  graph     16 draws in ONE recorded graph, per draw: the launch without the host.

  example   examples/train_synthetic.py at `--gaussians` / `--size` with --views 8 --graph --optimizer-in-graph --random-camera:
            `plain` (no new flag), `background` (--random-background alone), `draws_small` (--random-background
            --virtual-camera-extent 0.0003: a shear of the size of the fixed camera's, 0.1 over this example's altitude scale of
            350), `draws` (--random-background --virtual-camera-extent 0.02: a shear of up to 7, which widens and moves every
            footprint of the third render) and, with --parent-root DIR (a built checkout of the commit before the feature),
            `parent`: the plain command there. Every run is a child process.

    python tools/draw_probe.py [--out profiles/draw_probe.json] [--rounds 7] [--iters 200] [--gaussians 1000000] [--size 1024]
                               [--parent-root DIR]

Times: after a warm-up the paths alternate, `rounds` turns each. A turn of draw / torch is `iters` iterations on the host's
clock between two device synchronisations (the torch path waits for the device inside, so device events would not see its
cost); a turn of graph is between device events; a turn of the example is one run (main.last_ms_per_iter: the last half).
Reported per path: the median turn and the spread of the turns (min, max). The kernel is one wave and nothing here is
bandwidth-bound: the expectation for the example is "inside the spread between turns", and no speed ratio is an acceptance
condition of this feature. The file records what was measured and what was not.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd.build import source_hash  # noqa: E402
from eogs2_amd.draw import DrawStream, IterationDraws  # noqa: E402

IN_GRAPH = 16
EXTENT = 0.02
EXTENT_SMALL = 0.0003  # x 350 (synthetic.ALT_SCALE) = 0.105: the standard deviation of the fixed cameras' shear (make_camera)


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def host_timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def event_timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def draw_paths(dev, rounds, iters):
    g = torch.Generator().manual_seed(0)
    cams = []
    for _ in range(2):
        affine = torch.eye(4)
        affine[:3, :3] += 0.3 * torch.randn(3, 3, generator=g)
        affine[3, :3] = torch.randn(3, generator=g) * 1e6
        cams.append(dict(affine=affine.to(dev), center=(torch.randn(3, generator=g) * 1e5).to(dev),
                         altitude_bounds=torch.tensor([-31.5, 80.0], device=dev), bg=torch.zeros(5, device=dev),
                         virt=torch.zeros(4, 4, device=dev), c2v=torch.zeros(3, 3, device=dev)))
    stream = DrawStream(1, device=dev)
    draws = IterationDraws(stream)
    for c in cams:
        draws.add_camera(c["affine"], c["center"], c["altitude_bounds"][:1], bg=c["bg"], virt_affine=c["virt"], cam2virt=c["c2v"], extent=EXTENT)

    def with_draw():
        draws.draw()

    def with_torch():  # the reference's recipe, restated
        for c in cams:
            bg = torch.rand(5, device=dev)
            bg[3] = c["altitude_bounds"][0].item()
            bg[4] = 0
            A, b = c["affine"][:3, :3].T, c["affine"][3, :3]
            m = torch.eye(3, device=dev)
            m[:2, 2] = m[:2, 2] + torch.randn(2, device=dev).clip(-1, 1) * EXTENT
            new_A = m @ A
            new_b = (torch.eye(3, device=dev) - m) @ A @ c["center"] + b
            new_affine = torch.eye(4, 4)
            new_affine[:3, :3] = new_A
            new_affine[:3, -1] = new_b
            c["ref"] = (bg, new_affine.to(dev).float().T, m)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(IN_GRAPH):
            draws.draw()

    paths = {"draw": (host_timed, with_draw), "torch": (host_timed, with_torch), "graph_16_draws": (event_timed, graph.replay)}
    turns = {k: [] for k in paths}
    for r in range(rounds + 2):  # two warm-up turns
        for name, (clock, fn) in paths.items():
            ms = clock(fn, iters)
            if r >= 2:
                turns[name].append(ms)
    out = {k: summary(v) for k, v in turns.items()}
    out["spread_ms"] = max(out[k]["max_ms"] - out[k]["min_ms"] for k in paths)
    out["torch_over_draw"] = out["torch"]["median_ms"] / out["draw"]["median_ms"]
    out["device_ms_per_draw"] = out["graph_16_draws"]["median_ms"] / IN_GRAPH
    out["what"] = ("two cameras per iteration, background and sampled virtual camera each; draw and torch: host clock per iteration between "
                   "two device synchronisations (the torch path's own waits included); graph_16_draws: device events around one replay")
    return out


def example_run(root, args):
    code = ("import sys; sys.path.insert(0, 'examples'); import train_synthetic as t; t.main(sys.argv[1:]); "
            "print('MS_PER_ITER', t.main.last_ms_per_iter, t.main.last_recordings)")
    run = subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, cwd=root, timeout=900)
    if run.returncode != 0:
        raise RuntimeError(run.stdout[-2000:] + run.stderr[-3000:])
    line = [x for x in run.stdout.splitlines() if x.startswith("MS_PER_ITER")][-1].split()
    return float(line[1]), int(line[2])


def example_runs(gaussians, size, iters, rounds, parent_root):
    base = ["--gaussians", str(gaussians), "--size", str(size), "--iters", str(iters), "--quiet", "--views", "8", "--graph",
            "--optimizer-in-graph", "--random-camera"]
    configs = [("plain", ROOT, []), ("background", ROOT, ["--random-background"]),
               ("draws_small", ROOT, ["--random-background", "--virtual-camera-extent", str(EXTENT_SMALL)]),
               ("draws", ROOT, ["--random-background", "--virtual-camera-extent", str(EXTENT)])]
    if parent_root:
        configs.append(("parent", os.path.abspath(parent_root), []))
    turns, recordings = {name: [] for name, _, _ in configs}, {}
    for r in range(rounds + 1):  # one warm-up turn
        for name, root, extra in configs:
            ms, recordings[name] = example_run(root, base + extra)
            if r >= 1:
                turns[name].append(ms)
            print(name, f"{ms:.3f} ms/iter", flush=True)
    out = {k: summary(v) for k, v in turns.items()}
    out["recordings_of_the_last_run"] = recordings
    out["spread_ms"] = max(v["max_ms"] - v["min_ms"] for v in [out[name] for name, _, _ in configs])
    for name in ("background", "draws_small", "draws"):
        out[name + "_over_plain"] = out[name]["median_ms"] / out["plain"]["median_ms"]
    if parent_root:
        out["plain_over_parent"] = out["plain"]["median_ms"] / out["parent"]["median_ms"]
        out["draws_over_parent"] = out["draws"]["median_ms"] / out["parent"]["median_ms"]
    else:
        out["parent"] = "not measured: no --parent-root given"
    out["what"] = (f"{gaussians} Gaussians, {size}^2, --views 8 --graph --optimizer-in-graph --random-camera, {iters} iterations per run, ms "
                   f"per iteration over the last {max(1, iters // 2)} (host clock around a device synchronise), {rounds} alternating runs "
                   "each, every run a child process")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--example-iters", type=int, default=60)
    ap.add_argument("--example-rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit before the feature: its plain run joins the turns")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    out = {"what": f"the paths alternate, {a.rounds} turns each of {a.iters} iterations; ms per iteration", "source_hash": source_hash(),
           "device": torch.cuda.get_device_name(0)}
    out["draw"] = draw_paths(dev, a.rounds, a.iters)
    print("draw", json.dumps(out["draw"]), flush=True)
    torch.cuda.empty_cache()
    out["example"] = example_runs(a.gaussians, a.size, a.example_iters, a.example_rounds, a.parent_root)
    print("example", json.dumps(out["example"]), flush=True)
    out["not_measured"] = ("the kernel's own time under a profiler; more than two cameras; an eager multi-view loop with the reference's "
                           "host-side draws against the recorded one; whether the drawn backgrounds change what the model learns")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
