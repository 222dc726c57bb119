"""The per-iteration cost of watching the training: the reference's monitoring lines against the device monitor, on one GPU,
same commit, at 3 x 1024^2 images and 1 048 576 Gaussians.

    python tools/monitor_probe.py [--out profiles/monitor_probe.json] [--iters 200] [--warmup 30] [--rounds 5]

  baseline   what train_pan.py:423-429, 471-495, 534 does per camera per iteration BESIDE the loss it needs anyway, written
             here in torch ops: `Ll1.item()`, `Lphotometric.item()`, psnr(image, gt).mean().item(), a SECOND full SSIM as five
             grouped 11x11 convolutions plus its elementwise kernels and `.item()`, `loss.item()`, `Lphotometric.item()` for the
             two moving averages, and sigmoid(opacity).mean() (the reference reads that one every tenth iteration; here every
             iteration, `.item()` every tenth)
  monitor    TrainingMonitor.observe(loss_out=...) + observe_model + end_iteration every iteration, close_interval + fetch()
             every tenth

Both run after the same `photometric_loss` forward, which is not part of either figure: a run of the loss alone is timed and
subtracted. A run is `iters` iterations between two device synchronisations, on a host clock; the figure of a run is
(run - loss-only run) / iters. The three variants alternate, `rounds` runs each; reported: the median over the runs and the
spread (max - min). No ratio is promised or asserted; the file records what was measured and what was not.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd.build import source_hash  # noqa: E402
from eogs2_amd.losses import photometric_loss  # noqa: E402
from eogs2_amd.monitor import TrainingMonitor  # noqa: E402

PLANES, SIZE, P, LAM, INTERVAL = 3, 1024, 1 << 20, 0.2, 10


def _window(dev):
    g = torch.tensor([np.exp(-((x - 5) ** 2) / (2 * 1.5**2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t())[None, None].expand(PLANES, 1, 11, 11).contiguous().to(dev)


def torch_ssim(x, y, w):
    """utils/loss_utils.py:45-85 in torch ops: five grouped convolutions and the elementwise map."""
    conv = lambda t: F.conv2d(t, w, padding=5, groups=PLANES)  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu12
    return (((2 * mu12 + 0.01**2) * (2 * s12 + 0.03**2)) / ((mu1_sq + mu2_sq + 0.01**2) * (s11 + s22 + 0.03**2))).mean()


def torch_psnr(x, y):
    mse = ((x - y) ** 2).view(x.shape[0], -1).mean(1, keepdim=True)  # utils/image_utils.py:19-21
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def run(variant, img, gt, opacity, window, iters):
    dev = img.device
    mon = TrainingMonitor(dev) if variant == "monitor" else None
    sink = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(1, iters + 1):
        loss, Ll1, out = photometric_loss(img, gt, LAM, return_out=True)
        if variant == "baseline":
            sink += Ll1.item() + loss.item()  # train_pan.py:424,428
            sink += torch_psnr(img, gt).mean().float().item()  # :472
            sink += torch_ssim(img[None], gt[None], window).item()  # :476
            mean_opacity = torch.sigmoid(opacity).mean()  # :331
            sink += loss.item() + loss.item()  # :492-495
            if it % INTERVAL == 0:
                sink += mean_opacity.item()  # :534
        elif variant == "monitor":
            mon.observe(img, gt, "msi", loss_out=out, lambda_dssim=LAM)
            mon.observe_model(opacity)
            mon.end_iteration(loss.detach())
            if it % INTERVAL == 0:
                mon.close_interval()
                sink += mon.fetch()["photometric"]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitor_probe.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("monitor_probe: needs a GPU (a timing taken elsewhere says nothing about it)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(PLANES, SIZE, SIZE, generator=g).to(dev)
    img = (gt + 0.05 * torch.randn(PLANES, SIZE, SIZE, generator=g).to(dev)).clamp(0, 1)
    opacity = (torch.rand(P, 1, generator=g) * 8 - 4).to(dev)
    window = _window(dev)
    variants = ("loss_only", "baseline", "monitor")
    for v in variants:  # every shape and code path once before the clock
        run(v, img, gt, opacity, window, a.warmup)
    ms = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            ms[v].append(run(v, img, gt, opacity, window, a.iters))
    med = {v: float(np.median(ms[v])) for v in variants}
    res = {
        "what": "per-iteration cost of the monitoring lines beside the photometric loss, one camera per iteration",
        "device": torch.cuda.get_device_name(0), "source_hash": source_hash(), "torch": torch.__version__,
        "shape": {"planes": PLANES, "H": SIZE, "W": SIZE, "gaussians": P, "interval": INTERVAL},
        "iters_per_run": a.iters, "warmup_iters": a.warmup, "rounds": a.rounds,
        "ms_per_iter_runs": ms,
        "ms_per_iter_median": med,
        "spread_ms": {v: float(max(ms[v]) - min(ms[v])) for v in variants},
        "baseline_monitoring_ms": med["baseline"] - med["loss_only"],
        "monitor_monitoring_ms": med["monitor"] - med["loss_only"],
        "not_measured": ["kernel times (no rocprofv3 run)", "the monitor inside a recorded graph (eager launches here)",
                         "more than one camera per iteration", "fetch_async/poll in place of fetch"],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("ms_per_iter_median", "spread_ms", "baseline_monitoring_ms", "monitor_monitoring_ms")}))


if __name__ == "__main__":
    main()
