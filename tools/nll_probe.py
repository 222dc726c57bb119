"""The transient-uncertainty term on one GPU: forward + backward of eogs2_amd.uncertainty.transient_nll against the
reference's two statements as PyTorch ops (train_pan.py:434-440: clip, add, square, unsqueeze + repeat, gaussian_nll_loss with
its `torch.any(var < 0)` wait, autograd's backward) on the same card, at 3 x 1024^2, 3 x 2048^2 and 1 x 4096^2.

    python tools/nll_probe.py [--out profiles/nll_probe.json] [--rounds 7] [--iters 30]

Times: after a warm-up of every shape the two paths alternate, `rounds` times (at least five); each turn is `iters` forward +
backward calls between two device events. Reported per path: the median turn in ms per call and the spread of the turns (min,
max). Per kernel: `iters` back-to-back calls of eogs_nll_forward (the streaming kernel plus the one-workgroup combine) and of
eogs_nll_backward straight through the C-ABI between two device events, in turns of their own, and the bytes per second they
reach on the byte counts of include/eogs_nll.h: the forward reads (2 C + 1) H W 4 bytes, the backward reads the same and
writes (C + 1) H W 4. A call that takes less than ~10 microseconds is at the launch floor, and is reported as such: its
bytes per second say how often a launch can be queued, not what the kernel reaches.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd import _lib, uncertainty as U  # noqa: E402
from eogs2_amd._abi import NLL_MASK  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402

LAUNCH_FLOOR_MS = 0.010


def torch_statements(image, gt_image, transient_mask):
    betaprime = (transient_mask.clip(0, 1) + 1e-3).square()
    return torch.nn.functional.gaussian_nll_loss(input=image, target=gt_image, var=betaprime.unsqueeze(0).repeat(image.shape[0], 1, 1))


def between_events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def case(C, H, W, rounds, iters, dev):
    g = torch.Generator().manual_seed(C * H + W)
    gt = torch.rand(C, H, W, generator=g).to(dev)
    image = (gt + 0.2 * torch.randn(C, H, W, generator=g).to(dev)).requires_grad_(True)
    mask = (1.2 * torch.rand(H, W, generator=g) - 0.1).to(dev).requires_grad_(True)
    leaves = (image, mask)

    def run(step):
        for x in leaves:
            x.grad = None
        v = step()
        v.backward()
        return v

    hip_step = lambda: U.transient_nll(image, gt, mask)[1]  # noqa: E731
    ref_step = lambda: torch_statements(image, gt, mask)  # noqa: E731
    for _ in range(5):  # warm-up of the shape, both paths
        v1 = float(run(hip_step).detach())
        g1 = [x.grad.clone() for x in leaves]
        v2 = float(run(ref_step).detach())
        g2 = [x.grad.clone() for x in leaves]
    # faster and different is not faster: a guard, not the parity bar (tests/test_gpu_nll.py holds that, against float64)
    err = [abs(v1 - v2) / abs(v2)] + [float((p - q).abs().max() / q.abs().max()) for p, q in zip(g1, g2)]
    assert max(err) <= 1e-4, err
    hip, ref = [], []
    for _ in range(rounds):
        hip.append(between_events(lambda: run(hip_step), iters))
        ref.append(between_events(lambda: run(ref_step), iters))
    # the two launch groups on their own, straight through the C-ABI
    lib = _lib.get()
    n = ctypes.c_size_t()
    lib.check(lib.nll_bytes(C, H, W, ctypes.byref(n)))
    ws, out = torch.empty(n.value, dtype=torch.uint8, device=dev), torch.zeros(6, device=dev)
    g_loss, g_x, g_m = torch.ones(1, device=dev), torch.empty_like(image), torch.empty_like(mask)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, m = image.detach(), mask.detach()
    fwd_call = lambda: lib.check(lib.nll_forward(C, H, W, NLL_MASK, p(x), p(gt), p(m), 1, 1e-3, 1e-6, None, p(out), p(ws), n.value, stream))  # noqa: E731
    bwd_call = lambda: lib.check(lib.nll_backward(C, H, W, NLL_MASK, p(x), p(gt), p(m), 1, 1e-3, 1e-6, None, p(g_loss), None, p(g_x), p(g_m), stream))  # noqa: E731
    fwd_call()
    bwd_call()
    fwd, bwd = [], []
    for _ in range(rounds):
        fwd.append(between_events(fwd_call, iters))
        bwd.append(between_events(bwd_call, iters))
    plane = H * W * 4
    kernels = {}
    for name, ts, nbytes in (("forward", fwd, (2 * C + 1) * plane), ("backward", bwd, (2 * C + 1) * plane + (C + 1) * plane)):
        s = summary(ts)
        s.update(bytes=nbytes, achieved_TB_per_s=nbytes / (s["median_ms"] * 1e-3) / 1e12, at_launch_floor=s["median_ms"] < LAUNCH_FLOOR_MS)
        kernels[name] = s
    h, r = summary(hip), summary(ref)
    spread = max(h["max_ms"] - h["min_ms"], r["max_ms"] - r["min_ms"])
    row = {"hip": h, "torch_statements": r, "spread_ms": spread, "torch_over_hip": r["median_ms"] / h["median_ms"],
           "difference_inside_spread": abs(h["median_ms"] - r["median_ms"]) <= spread, "launch_groups": kernels,
           "max_relative_difference": {"value": err[0], "gradients": err[1:]}}
    print(f"{C} x {H} x {W}", json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nll_probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.rounds >= 5, "medians of at least five turns"
    dev = torch.device("cuda:0")
    out = {"what": f"forward + backward of the transient NLL term, fp32; eogs2_amd.uncertainty.transient_nll and the reference's two "
                   f"statements as torch ops (with gaussian_nll_loss's any() wait) alternating, {a.rounds} turns of {a.iters} calls each "
                   "between device events; ms per call. launch_groups: the same number of back-to-back C-ABI calls of the forward "
                   "(streaming kernel + one-workgroup combine) and of the backward between device events, turns of their own; bytes "
                   f"as counted in include/eogs_nll.h; at_launch_floor: under {LAUNCH_FLOOR_MS * 1e3:g} microseconds per call",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "cases": {}}
    for C, H, W in ((3, 1024, 1024), (3, 2048, 2048), (1, 4096, 4096)):
        out["cases"][f"{C} x {H} x {W}"] = case(C, H, W, a.rounds, a.iters, dev)
    out["not_measured"] = ("the direct-variance modes; sizes that are no multiple of four (the scalar-load path); the term inside the example's "
                           "iteration; kernel times from a profiler trace (the launch-group times above are event brackets around "
                           "back-to-back calls); more than one GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
