"""The panchromatic camera pipeline on one GPU: forward + backward of eogs2_amd.pan.pan_shade against what a user had
before it, on the same card, at 1024^2 and 2048^2:

  order A (colour correction, shadow, then the map) with the `fixed` map
    (a) fused            eogs2_amd.pan.pan_shade
    (b) shade + torch    eogs2_amd.shade.shade (the affine camera's fused pipeline) followed by the map as PyTorch ops
    (c) torch            the whole chain as PyTorch ops (1x1 convolution, exp / clip, the tint, the map)
  order B (`weird_pan_setup`: the map, a 1->1 colour correction, then shadow) with the `learnable_fixed` map, unfrozen
    (a) fused            eogs2_amd.pan.pan_shade
    (b) torch            the whole chain as PyTorch ops

    python tools/pan_probe.py [--out profiles/pan_probe.json] [--sizes 1024 2048] [--rounds 20] [--iters 20]

Every path computes the same thing: outputs cc, shaded, shadow; one backward from upstream gradients of shaded and shadow to
raw, the altitude difference, the colour correction, the in-shadow tint and (order B) the map's five parameters. After a
warm-up of every shape the paths alternate, `rounds` times; each turn is `iters` forward + backward calls between two device
events. Reported per path: the median turn in ms per call and the spread of the turns (min, max). Acceptance: (a) is not
slower than (b) at either size; a gain is claimed only where the medians differ by more than the spread.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd import _lib, pan, shade  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402


def torch_map(p, x):
    return p[3] * (torch.sum(p[None, :3, None, None] * x, dim=-3, keepdim=True) + p[4])


def torch_shadow(d):
    return torch.exp(0.4 * d.clip(max=0.0))


def make_paths(order):
    """{name: step(t) -> (cc, shaded, shadow)}; t holds raw, d, the parameters and the upstream gradients."""
    if order == "A":
        def fused(t):
            return pan.pan_shade(t.raw, t.d, t.M, t.ins, t.pan_map, "cc_first")

        def shade_then_torch(t):
            cc, shaded3, shadow = shade.shade(t.raw, t.d, t.M, t.ins)
            return cc, torch_map(t.p, shaded3.unsqueeze(0)).squeeze(0), shadow

        def plain(t):
            cc = torch.nn.functional.conv2d(t.raw.unsqueeze(0), t.M[:, :3].reshape(3, 3, 1, 1), t.M[:, 3])
            shadow = torch_shadow(t.d)
            shaded3 = shadow * cc + (1 - shadow) * t.ins.reshape(3, 1, 1) * cc
            return cc.squeeze(0), torch_map(t.p, shaded3).squeeze(0), shadow
        return {"fused": fused, "shade_then_torch_map": shade_then_torch, "torch": plain}

    def fused(t):
        return pan.pan_shade(t.raw, t.d, t.M, t.ins, t.pan_map, "map_first")

    def plain(t):
        p0 = torch_map(t.p, t.raw.unsqueeze(0))
        cc = torch.nn.functional.conv2d(p0, t.M[0].reshape(1, 1, 1, 1), t.M[1].reshape(1))
        shadow = torch_shadow(t.d)
        shaded = shadow * cc + (1 - shadow) * t.ins.reshape(1, 1, 1) * cc
        return cc.squeeze(0), shaded.squeeze(0), shadow
    return {"fused": fused, "torch": plain}


def leaves(t):
    return [x for x in (t.raw, t.d, t.M, t.ins, t.p) if x.requires_grad]


def call(step, t):
    for x in leaves(t):
        x.grad = None
    cc, shaded, shadow = step(t)
    torch.autograd.backward([shaded, shadow], [t.g_shaded, t.g_shadow])
    return cc, shaded, shadow


def turn(step, t, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        call(step, t)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "turns": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pan_probe.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.rounds >= 20, "the median of at least 20 timed repeats"
    dev = torch.device("cuda:0")
    assert _lib.get().backend == "hip-gfx950"
    out = {"what": "PAN camera render pipeline, forward + backward, fp32; the paths alternate, "
                   f"{a.rounds} turns of {a.iters} calls each between device events; ms per call",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "cases": {}}
    g = torch.Generator().manual_seed(0)
    for size in a.sizes:
        H = W = size
        for order, kind in (("A", "fixed"), ("B", "learnable_fixed")):
            t = argparse.Namespace()
            t.raw = torch.rand((3, H, W), generator=g).to(dev).requires_grad_(True)
            t.d = (1.5 * torch.randn((H, W), generator=g)).to(dev).requires_grad_(True)
            if order == "A":
                t.M = (torch.eye(3, 4) + 0.2 * torch.randn((3, 4), generator=g)).to(dev).requires_grad_(True)
                t.ins = (0.05 + 0.5 * torch.rand(3, generator=g)).to(dev).requires_grad_(True)
            else:
                t.M = torch.tensor([0.9, 0.05], device=dev, requires_grad=True)
                t.ins = torch.tensor([0.2], device=dev, requires_grad=True)
            t.p = torch.tensor(pan.FIXED_PARAMS, device=dev).requires_grad_(kind == "learnable_fixed")
            t.pan_map = pan.PanMap(kind, params=t.p)
            t.g_shaded = torch.randn((1, H, W), generator=g).to(dev)
            t.g_shadow = torch.randn((H, W), generator=g).to(dev)
            paths = make_paths(order)
            results = {}
            for name, step in paths.items():  # warm-up of every shape, every path; and the results of each
                for _ in range(5):
                    o = call(step, t)
                results[name] = [x.detach().clone() for x in o] + [x.grad.clone() for x in leaves(t)]
            diff = {}
            for name in paths:
                if name != "torch":
                    diff[name] = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(results[name], results["torch"]))
                    assert diff[name] <= 2e-4, (name, diff)  # faster and different is not faster
            ts = {name: [] for name in paths}
            for _ in range(a.rounds):
                for name, step in paths.items():
                    ts[name].append(turn(step, t, a.iters))
            row = {name: summary(v) for name, v in ts.items()}
            before = "shade_then_torch_map" if order == "A" else "torch"
            spread = max(r["max_ms"] - r["min_ms"] for r in row.values())
            row.update(spread_ms=spread, before=before,
                       before_over_fused=row[before]["median_ms"] / row["fused"]["median_ms"],
                       torch_over_fused=row["torch"]["median_ms"] / row["fused"]["median_ms"],
                       fused_not_slower_than_before=row["fused"]["median_ms"] <= row[before]["median_ms"],
                       gain_exceeds_spread=row[before]["median_ms"] - row["fused"]["median_ms"] > spread,
                       max_difference_from_torch_over_array_max=diff)
            out["cases"][f"{H}x{W} order {order} {kind}"] = row
            print(H, order, kind, json.dumps(row), flush=True)
    out["not_measured"] = "kernel times on their own (the library's 32 profile slots are taken); more than one GPU"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
