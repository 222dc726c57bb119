"""The random-camera loss in full on one GPU (eogs2_amd.randomcam) against what it replaces and against what it adds, on the same card:

  chain     everything of `rawrender_wshadow` around the renders, forward and backward, with both renders handed in as leaf tensors at
            `--size`: `hip` — virtual_to_sun, the sun lookup, the render pipeline, the resample, cmloss (this package's kernels) — against
            `torch` — the reference's non-render lines restated as torch operations (renderer_cc_shadow.py:85-137, affine_cameras.py:
            303-348, main_loss.py:149-164: two einsums, torch.inverse, two grid_samples with their index_puts, the elementwise pipeline,
            the masked means with their `.any()` wait);
  example   examples/train_synthetic.py at `--gaussians` / `--size` with --views 8 --graph --optimizer-in-graph --random-camera: `plain`
            (the `--random-camera` iteration as it was: render type rawrender through shade.randomcam_l), `wshadow_shared`
            (--random-camera-type rawrender_wshadow: the iteration's sun render handed to the loss), `wshadow_twice`
            (... --no-share-sun-render: the reference's protocol, the sun camera rendered a second time) and, with --parent-root DIR (a
            built checkout of the commit before the feature), `parent`: the plain command there. Every run is a child process.

    python tools/randomcam_probe.py [--out profiles/randomcam_probe.json] [--rounds 7] [--iters 50] [--gaussians 1000000] [--size 1024]
                                    [--parent-root DIR]

Times: after a warm-up the paths alternate, `rounds` turns each. A turn of the chain is `iters` iterations on the host's clock between
two device synchronisations (the torch path waits for the device inside); a turn of the example is one run (main.last_ms_per_iter: the
last half). Reported per path: the median turn and the spread of the turns (min, max). No ratio is an acceptance condition; the file
records what was measured and what was not.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd.build import source_hash  # noqa: E402
from eogs2_amd.randomcam import RandomcamRendering_Loss  # noqa: E402


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def host_timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def chain_paths(dev, size, rounds, iters):
    H = W = size
    g = torch.Generator().manual_seed(0)
    rand = lambda *s: torch.rand(*s, generator=g).to(dev)  # noqa: E731
    U, V = torch.meshgrid(torch.linspace(-0.95, 0.95, W, device=dev), torch.linspace(-0.95, 0.95, H, device=dev), indexing="xy")
    leaves = dict(virtual=rand(5, H, W), sun=rand(5, 2 * H, 2 * W), altitude=0.5 + 0.1 * rand(H, W), raw=rand(3, H, W), shaded=rand(3, H, W))
    for t in leaves.values():
        t.requires_grad_(True)
    cam2virt = torch.eye(3, device=dev)
    cam2virt[:2, 2] = torch.tensor([0.03, -0.02], device=dev)
    camera_to_sun = torch.diag(torch.tensor([0.5, 0.5, 1.0], device=dev))
    camera_to_sun[:2, 2] = torch.tensor([0.04, -0.03], device=dev)
    cam = types.SimpleNamespace(use_cc=True, use_exposure=False, use_shadow=True)
    cam.color_correction = torch.nn.Conv2d(3, 3, 1, bias=True).to(dev)
    cam.inshadow_color_correction = torch.nn.Parameter(torch.full((3, 1, 1), 0.05, device=dev))
    cam.get_sun_camera = lambda: (None, camera_to_sun)
    params = [*cam.color_correction.parameters(), cam.inshadow_color_correction]
    loss_fn = RandomcamRendering_Loss(1e-4, 1e-3, "rawrender_wshadow")

    def clear():
        for t in (*leaves.values(), *params):
            t.grad = None

    def with_hip():
        clear()
        uva = torch.stack((U, V, leaves["altitude"]), dim=-1)
        L_alt, L_rgb = loss_fn(None, cam, cam2virt, uva, None, None, None, leaves["altitude"], leaves["raw"], None, leaves["shaded"],
                               virtual_render=leaves["virtual"], sun_render=leaves["sun"])
        (1e-4 * L_alt + 1e-3 * L_rgb).backward()

    def resample_ref(render, M, uva):  # renderer_cc_shadow.py:32-46
        uv = torch.einsum("...ij,...j->...i", M, uva)[..., :2]
        smp = torch.nn.functional.grid_sample(render.unsqueeze(0), uv.unsqueeze(0), align_corners=True).squeeze(0)
        return smp, uv

    def with_torch():  # the reference's lines, restated
        clear()
        uva = torch.stack((U, V, leaves["altitude"]), dim=-1)
        vr = leaves["virtual"]
        virtual_uva = torch.einsum("...ij,...j->...i", cam2virt, uva)
        virt_to_sun = torch.matmul(torch.inverse(cam2virt), camera_to_sun)
        smp, sun_uv = resample_ref(leaves["sun"], virt_to_sun, virtual_uva)
        sun_alt = smp[3]
        sun_alt[(sun_uv.abs() > 1).any(-1)] = -100
        diff = vr[3] - sun_alt
        cc = cam.color_correction(vr[:3].unsqueeze(0))
        shadow = torch.exp(0.4 * diff.clip(max=0.0))
        shaded = (shadow * cc + (1 - shadow) * cam.inshadow_color_correction * cc).squeeze(0)
        source = torch.cat([shaded, vr[3:]], dim=0)
        uv = virtual_uva[..., :2]
        sample = torch.nn.functional.grid_sample(source.unsqueeze(0), uv.unsqueeze(0), align_corners=True).squeeze(0)
        alt_s = sample[3]
        alt_s[(uv.abs() > 1).any(-1)] = -100
        d = leaves["altitude"] - alt_s
        rgb = leaves["shaded"] - sample[:3]
        occ = ((d.abs() < 0.30) * (uv.abs() < 1).all(-1)).detach()
        if occ.any():
            L_alt, L_rgb = (d.abs() * occ).sum() / occ.sum(), (rgb.abs() * occ).sum() / occ.sum()
            (1e-4 * L_alt + 1e-3 * L_rgb).backward()

    paths = {"hip": with_hip, "torch": with_torch}
    turns = {k: [] for k in paths}
    for r in range(rounds + 2):  # two warm-up turns
        for name, fn in paths.items():
            ms = host_timed(fn, iters)
            if r >= 2:
                turns[name].append(ms)
    out = {k: summary(v) for k, v in turns.items()}
    out["spread_ms"] = max(out[k]["max_ms"] - out[k]["min_ms"] for k in paths)
    out["torch_over_hip"] = out["torch"]["median_ms"] / out["hip"]["median_ms"]
    out["what"] = (f"{size}^2, renders handed in as leaves ([5,H,W] and [5,2H,2W]), forward and backward of everything else of rawrender_wshadow; "
                   "host clock per iteration between two device synchronisations")
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
    wshadow = ["--random-camera-type", "rawrender_wshadow"]
    configs = [("plain", ROOT, []), ("wshadow_shared", ROOT, wshadow), ("wshadow_twice", ROOT, wshadow + ["--no-share-sun-render"])]
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
    for name in ("wshadow_shared", "wshadow_twice"):
        out[name + "_over_plain"] = out[name]["median_ms"] / out["plain"]["median_ms"]
    out["twice_minus_shared_ms"] = out["wshadow_twice"]["median_ms"] - out["wshadow_shared"]["median_ms"]
    if parent_root:
        out["plain_over_parent"] = out["plain"]["median_ms"] / out["parent"]["median_ms"]
    else:
        out["parent"] = "not measured: no --parent-root given"
    out["what"] = (f"{gaussians} Gaussians, {size}^2, --views 8 --graph --optimizer-in-graph --random-camera, {iters} iterations per run, ms "
                   f"per iteration over the last {max(1, iters // 2)} (host clock around a device synchronise), {rounds} alternating runs "
                   "each, every run a child process")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randomcam_probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
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
    out["chain"] = chain_paths(dev, a.size, a.rounds, a.iters)
    print("chain", json.dumps(out["chain"]), flush=True)
    torch.cuda.empty_cache()
    out["example"] = example_runs(a.gaussians, a.size, a.example_iters, a.example_rounds, a.parent_root)
    print("example", json.dumps(out["example"]), flush=True)
    out["not_measured"] = ("the kernels' own times under a profiler; the eager and --parallel-renders forms of the example; a panchromatic "
                           "camera; --random-camera-gt; what the option changes in what the model learns")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
