"""Ground-truth preparation on one GPU: eogs2_amd.pansharp / eogs2_amd.rescaler against the reference's lines as PyTorch ops
(pansharpening/algorithm/brovey.py:31-49, loss/pansharp_loss.py, loss/PAN_loss.py:16-30, utils/rescaler/rescaler.py:76-99 with
torchvision's documented equalize rule written as torch ops) on the same card:

  brovey_pansharp, MSI 3 x 512^2 -> PAN 2048^2;  Pansharploss forward + backward at the same size;
  Lgradient_pan forward + backward at 2048^2;  standard_rescaler at 3 x 2048^2;  histogram equalisation at 3 x 2048^2

    python tools/gtprep_probe.py [--out profiles/gtprep_probe.json] [--rounds 10] [--iters 200]

Times: after a warm-up of every shape the two paths alternate, `rounds` times; each turn is `iters` calls between a device
synchronise and a host clock read after the next device synchronise. Reported per path: the median turn in ms per call and the
spread of the turns (min, max). No ratio is promised: where the difference of the medians is inside the spread the row says so.
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

from eogs2_amd import pansharp as P, rescaler as R  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402


def torch_brovey(pan, msi, W=0.1):
    up = F.interpolate(msi[None], mode="bicubic", align_corners=False, size=pan.shape)[0]
    return pan / (W * up.sum(dim=0, keepdim=True)).clamp(min=1e-8) * up


def torch_gradient_loss(a, b):
    ga, gb = torch.gradient(a, dim=(-2, -1)), torch.gradient(b, dim=(-2, -1))
    return torch.mean((ga[0] - gb[0]) ** 2) + torch.mean((ga[1] - gb[1]) ** 2)


def torch_standard(x):
    lo = x.view(x.shape[0], -1).min(dim=1)[0][:, None, None]
    hi = x.view(x.shape[0], -1).max(dim=1)[0][:, None, None]
    return (x - lo) / (hi - lo + 1e-8)


def torch_equalize(x):
    v = (x * 255.0).to(torch.uint8)
    out = []
    for ch in v:  # the documented per-channel rule, with its wait for `step`
        hist = torch.bincount(ch.reshape(-1).long(), minlength=256)
        nonzero = hist[hist != 0]
        step = torch.div(nonzero[:-1].sum(), 255, rounding_mode="floor")
        if step == 0:
            out.append(ch)
            continue
        lut = torch.div(torch.cumsum(hist, 0) + torch.div(step, 2, rounding_mode="floor"), step, rounding_mode="floor")
        lut = F.pad(lut, [1, 0])[:-1].clamp(0, 255)
        out.append(lut[ch.long()].to(torch.uint8))
    return torch.stack(out) / 255.0


def turn(step, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def case(name, hip_step, ref_step, compare, rounds, iters):
    for _ in range(5):  # warm-up of every shape, both paths
        got, want = hip_step(), ref_step()
    err = compare(got, want)
    hip, ref = [], []
    for _ in range(rounds):  # alternating turns
        hip.append(turn(hip_step, iters))
        ref.append(turn(ref_step, iters))
    h, r = summary(hip), summary(ref)
    spread = max(h["max_ms"] - h["min_ms"], r["max_ms"] - r["min_ms"])
    row = {"hip": h, "torch_sequence": r, "spread_ms": spread, "torch_over_hip": r["median_ms"] / h["median_ms"],
           "difference_inside_spread": abs(h["median_ms"] - r["median_ms"]) <= spread, "max_difference_of_results": err}
    print(name, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtprep_probe.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--msi", type=int, default=512)
    ap.add_argument("--pan", type=int, default=2048)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    msi = (0.05 + 0.95 * torch.rand(3, a.msi, a.msi, generator=g)).to(dev)
    pan = (0.05 + 0.95 * torch.rand(a.pan, a.pan, generator=g)).to(dev)
    syn = torch.rand(3, a.pan, a.pan, generator=g).to(dev).requires_grad_(True)
    img, gt = torch.rand(1, a.pan, a.pan, generator=g).to(dev).requires_grad_(True), torch.rand(1, a.pan, a.pan, generator=g).to(dev)
    x = (3.0 * torch.randn(3, a.pan, a.pan, generator=g)).to(dev)
    u = torch.rand(3, a.pan, a.pan, generator=g).to(dev)
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max())  # noqa: E731
    term = P.Pansharploss(0.1, "brovey")

    def with_grad(fn, leaf):
        def step():
            leaf.grad = None
            v = fn()
            v.backward()
            return v.detach(), leaf.grad
        return step

    both = lambda p, q: [rel(p[0], q[0]), rel(p[1], q[1])]  # noqa: E731
    # largest |difference|: 0 for the rescaler; the histogram's last step differs by an ulp where torch on the GPU multiplies by
    # the reciprocal of 255 instead of dividing (the kernel divides, as torch does on the CPU)
    absdiff = lambda p, q: float((p - q).abs().max())  # noqa: E731
    out = {"what": f"HIP path and the reference's PyTorch op sequence alternating, {a.rounds} turns of {a.iters} calls each; host clock "
                   "from a device synchronise to the next; ms per call, fp32",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "cases": {}}
    c = out["cases"]
    c[f"brovey_pansharp, MSI 3x{a.msi}^2 -> PAN {a.pan}^2"] = case(
        "brovey", lambda: P.brovey_pansharp(pan, msi), lambda: torch_brovey(pan, msi), rel, a.rounds, a.iters)
    c[f"Pansharploss forward + backward, MSI 3x{a.msi}^2 -> PAN {a.pan}^2"] = case(
        "pansharploss", with_grad(lambda: term(syn, pan, msi), syn), with_grad(lambda: torch.mean((syn - torch_brovey(pan, msi)) ** 2), syn),
        both, a.rounds, a.iters)
    c[f"Lgradient_pan forward + backward, {a.pan}^2"] = case(
        "lgradient", with_grad(lambda: P.pan_gradient_l2(img, gt), img), with_grad(lambda: torch_gradient_loss(img, gt), img), both,
        a.rounds, a.iters)
    std = R.standard_rescaler()
    c[f"standard_rescaler, 3x{a.pan}^2"] = case(
        "standard_rescaler", lambda: std.forward(x), lambda: torch_standard(x), absdiff, a.rounds, a.iters)
    heq = R.histogram_equalizer()
    c[f"histogram equalisation, 3x{a.pan}^2"] = case(
        "histogram", lambda: heq.forward(u), lambda: torch_equalize(u), absdiff, a.rounds, a.iters)
    out["not_measured"] = "simple_brovey and ihs; other sizes and channel counts; the rescalers inside a data loader; more than one GPU"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
