"""The report module on one GPU (eogs2_amd.report) against the reference's own lines restated as torch operations, on the same card:

  fetch     one view's products at `--size` (render_set's thirteen images: eight of three planes, five of one) to the host in file
            layout: `hip` — fetch_products: one packing launch, one copy into page-locked memory — against `torch` — the reference's
            `permute(1, 2, 0).cpu().numpy()` (a one-plane image: `.cpu().numpy()`) per product (render_pan.py:346-399);
  rows      normalize_before_saving's colour pass over `--rows` Gaussians: `hip` — the in-place row kernel and the one-wave camera
            kernel — against `torch` — utils/save_utils.py:18-33 as it stands, torch.linalg.inv included, for the same five cameras;
  metrics   one view's L1 and PSNR at 3 x `--size`^2: `hip` — ReportAccumulator.accumulate, nothing read back — against `torch` —
            train_pan.py:917,942-943 with their two `.double()` results read back by `float()`, which is where the reference's
            `+=` on Python floats waits.

    python tools/report_probe.py [--out profiles/report_probe.json] [--rounds 7] [--iters 20] [--size 1024] [--rows 1000000]

Times: after two warm-up turns the paths alternate, `rounds` turns each; a turn is `iters` calls on the host's clock between two
device synchronisations. Reported per path: the median turn and the spread of the turns (min, max). No ratio is an acceptance
condition; the file records what was measured and what was not.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd.build import source_hash  # noqa: E402
from eogs2_amd.report import ReportAccumulator, fetch_products, normalize_colors_  # noqa: E402

C0 = 0.28209479177387814


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def host_timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(paths, rounds, iters, what):
    turns = {k: [] for k in paths}
    for r in range(rounds + 2):  # two warm-up turns
        for name, fn in paths.items():
            ms = host_timed(fn, iters)
            if r >= 2:
                turns[name].append(ms)
    out = {k: summary(v) for k, v in turns.items()}
    out["spread_ms"] = max(out[k]["max_ms"] - out[k]["min_ms"] for k in paths)
    out["torch_over_hip"] = out["torch"]["median_ms"] / out["hip"]["median_ms"]
    out["what"] = what
    return out


def fetch_paths(dev, size, rounds, iters):
    g = torch.Generator().manual_seed(0)
    three = ("rawrender", "sunpovsampled", "nadirpov", "nadirpovsampled", "shaded", "cc", "final", "gt")
    one = ("altitude", "accumulated_opacity", "nadiraltitudesampled", "nadir_altitude_diff", "shadowmap")
    products = {k: torch.rand(3, size, size, generator=g).to(dev) for k in three}
    products.update({k: torch.rand(size, size, generator=g).to(dev) for k in one})

    def with_hip():
        fetch_products(products)

    def with_torch():
        for v in products.values():
            (v.permute(1, 2, 0) if v.ndim == 3 else v).cpu().numpy()

    return alternate({"hip": with_hip, "torch": with_torch}, rounds, iters,
                     f"{len(three)} images of 3 planes and {len(one)} of one at {size}^2 to numpy arrays in file layout, per view")


def rows_paths(dev, rows, rounds, iters):
    g = torch.Generator().manual_seed(1)
    V = 5
    weights = [(torch.eye(3) + 0.05 * torch.randn(3, 3, generator=g)).reshape(3, 3, 1, 1).to(dev) for _ in range(V)]
    biases = [(0.02 * torch.randn(3, generator=g)).to(dev) for _ in range(V)]
    f_dc = torch.randn(rows, 1, 3, generator=g).to(dev)
    holder = {"f": f_dc.clone()}

    def with_hip():
        normalize_colors_(holder["f"], weights[0], biases[0], weights, biases)

    def with_torch():  # utils/save_utils.py:18-33
        A1, b1 = weights[0].squeeze(), biases[0].squeeze()
        A1inv = torch.linalg.inv(A1.double()).float()
        rgb = holder["f"] * C0 + 0.5
        holder["f"] = (torch.einsum("ij,...j->...i", A1, rgb) + b1 - 0.5) / C0
        for i in range(V):
            Ai, bi = weights[i].squeeze(), biases[i].squeeze()
            weights[i] = (Ai @ A1inv).reshape(3, 3, 1, 1)
            biases[i] = -(Ai @ A1inv @ b1) + bi

    # (both paths keep transforming the same data: corrections near the identity keep it finite over the probe's calls)
    return alternate({"hip": with_hip, "torch": with_torch}, rounds, iters, f"{rows} rows and {V} cameras per call")


def metrics_paths(dev, size, rounds, iters):
    g = torch.Generator().manual_seed(2)
    image, gt = torch.rand(3, size, size, generator=g).to(dev), (1.2 * torch.rand(3, size, size, generator=g) - 0.1).to(dev)
    acc = ReportAccumulator(dev)
    acc.reset()
    sums = {"l1": 0.0, "psnr": 0.0}

    def with_hip():
        acc.accumulate(image, gt, "msi")

    def with_torch():  # train_pan.py:917,942-943
        gt_image = torch.clamp(gt, 0.0, 1.0)
        sums["l1"] += float(torch.abs(image - gt_image).mean().mean().double())
        mse = ((image - gt_image) ** 2).view(image.shape[0], -1).mean(1, keepdim=True)
        sums["psnr"] += float((20 * torch.log10(1.0 / torch.sqrt(mse))).mean().double())

    return alternate({"hip": with_hip, "torch": with_torch}, rounds, iters, f"one view of 3 x {size}^2 per call; the torch path reads two scalars back per view")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    out = {"what": f"the paths alternate, {a.rounds} turns each of {a.iters} calls; ms per call on the host's clock between two device "
                   "synchronisations", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0)}
    for name, fn, arg in (("fetch", fetch_paths, a.size), ("rows", rows_paths, a.rows), ("metrics", metrics_paths, a.size)):
        out[name] = fn(dev, arg, a.rounds, a.iters)
        print(name, json.dumps(out[name]), flush=True)
    out["not_measured"] = ("the kernels' own times under a profiler; the converters (a few hundred bytes, no speed is claimed); evaluate_views and "
                           "view_products, whose time is their renders'; the 8-bit modes and the video frame; PAN images")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
