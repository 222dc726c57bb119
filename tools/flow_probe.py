"""The flow warp on one GPU: forward + backward of eogs2_amd.flow.apply_flow against the reference's PyTorch op sequence
(flowmatching/flow_matching.py:225-253: cached grid + flow, two in-place normalisations, permute, grid_sample(border,
align_corners=True), autograd's backward) on the same card, at 3 x 1024^2 and 1 x 1024^2, for a flow field and for a
constant displacement; and ms/iter of examples/train_synthetic.py with and without --flow-matching.

    python tools/flow_probe.py [--out profiles/flow_probe.json] [--size 1024] [--rounds 10] [--iters 40]

Times: after a warm-up of every shape the two paths alternate, `rounds` times; each turn is `iters` forward + backward calls
between two device events (rounds x iters >= 200 calls per path). Reported per path: the median turn in ms per call, and the
spread of the turns (min, max). The constant displacement is handed to the PyTorch sequence as the filled (1, 2, H, W) tensor
the reference's set_cst_displacement returns, to the HIP path as the stride-0 view this package returns; building either is
outside the timed region. Kernel times are the library's profile slots (HIP events around each kernel group), in a separate
pass. Acceptance (per case): the HIP path is not slower than the PyTorch sequence by more than the measured spread.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from eogs2_amd import _lib, flow as F  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402


def torch_sequence(grid):
    def step(x, flow, up):
        C, H, W = x.shape
        flow_grid = grid + flow
        flow_grid[:, 0] = 2.0 * flow_grid[:, 0] / (W - 1) - 1.0
        flow_grid[:, 1] = 2.0 * flow_grid[:, 1] / (H - 1) - 1.0
        flow_grid = flow_grid.permute(0, 2, 3, 1)
        out = torch.nn.functional.grid_sample(x.unsqueeze(0), flow_grid.detach(), mode="bilinear", padding_mode="border",
                                              align_corners=True).squeeze(0)
        out.backward(up)
        return out
    return step


def hip_step(x, flow, up):
    out = F.apply_flow(x, flow)
    out.backward(up)
    return out


def turn(step, x, flow, up, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        x.grad = None
        step(x, flow, up)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_probe.json"))
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--no-example", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.rounds * a.iters >= 200
    dev = torch.device("cuda:0")
    abi = _lib.get()
    abi.profile_select(0xFFFFFFFF)
    H = W = a.size
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid = torch.stack((xx, yy), dim=0).float().to(dev).unsqueeze(0)  # the reference's cached grid
    ref_step = torch_sequence(grid)
    field = (3.0 * torch.randn(1, 2, H, W, generator=g)).to(dev)
    two = torch.tensor([1.37, -0.62], device=dev).view(1, 2, 1, 1)
    out = {"what": f"apply_flow forward + backward at {H} x {W}, fp32; HIP path and the reference's PyTorch op sequence alternating, "
                   f"{a.rounds} turns of {a.iters} calls each between device events; ms per call",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "cases": {}}
    for C in (3, 1):
        for kind in ("field", "constant"):
            x = torch.rand(C, H, W, generator=g).to(dev).requires_grad_(True)
            up = torch.randn(C, H, W, generator=g).to(dev)
            hip_flow = field if kind == "field" else two.expand(1, 2, H, W)
            ref_flow = field if kind == "field" else two.expand(1, 2, H, W).contiguous()
            for _ in range(10):  # warm-up of every shape, both paths
                o1 = hip_step(x, hip_flow, up)
                g1 = x.grad.clone()
                x.grad = None
                o2 = ref_step(x, ref_flow, up)
                g2 = x.grad.clone()
                x.grad = None
            err = (float((o1 - o2).abs().max() / o2.abs().max()), float((g1 - g2).abs().max() / g2.abs().max()))
            assert max(err) <= 2e-4, err  # faster and different is not faster
            hip, ref = [], []
            for _ in range(a.rounds):
                hip.append(turn(hip_step, x, hip_flow, up, a.iters))
                ref.append(turn(ref_step, x, ref_flow, up, a.iters))
            # kernel times, in a pass of their own
            fwd, bwd = [], []
            for _ in range(25):
                abi.profile_reset()
                torch.cuda.synchronize()
                abi.profile_enable(1)
                x.grad = None
                hip_step(x, hip_flow, up)
                torch.cuda.synchronize()
                abi.profile_enable(0)
                prof = abi.profile()
                fwd.append(prof["flow_fwd"][0])
                bwd.append(prof["flow_bwd"][0])
            h, r = summary(hip), summary(ref)
            spread = max(h["max_ms"] - h["min_ms"], r["max_ms"] - r["min_ms"])
            row = {"hip": h, "torch_sequence": r, "spread_ms": spread, "torch_over_hip": r["median_ms"] / h["median_ms"],
                   "hip_not_slower_beyond_spread": h["median_ms"] <= r["median_ms"] + spread,
                   "hip_kernels_ms": {"flow_fwd": float(np.median(fwd)), "flow_bwd": float(np.median(bwd))},
                   "max_difference_of_channel_max": {"out": err[0], "g_img": err[1]}}
            out["cases"][f"{C}x{H}x{W} {kind}"] = row
            print(C, kind, json.dumps(row), flush=True)
    if not a.no_example:
        import train_synthetic

        base = ["--quiet", "--no-prune"]
        ms = {"plain": [], "flow_matching": []}
        for _ in range(3):  # alternating
            train_synthetic.main(base)
            ms["plain"].append(train_synthetic.main.last_ms_per_iter)
            train_synthetic.main(base + ["--flow-matching"])
            ms["flow_matching"].append(train_synthetic.main.last_ms_per_iter)
        out["example_ms_per_iter"] = {"what": "examples/train_synthetic.py --quiet --no-prune (200 000 Gaussians, 512 x 512, 200 iterations, "
                                              "steady-state half), three runs each, alternating; with --flow-matching the iteration adds "
                                              "the stand-in network, flow_stats, the gate and the warp each way",
                                      "plain": summary(ms["plain"]), "flow_matching": summary(ms["flow_matching"])}
        print(json.dumps(out["example_ms_per_iter"]), flush=True)
    out["not_measured"] = "RAFT itself (the caller's); 2048^2; more than one GPU"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
