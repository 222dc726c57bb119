"""The flow network on one GPU: eogs2_amd.raft's RAFT-small and RAFT-large at 1024^2 and 2048^2, 12 updates, seeded random
weights, with the on-demand correlation (the HIP operators) and the materialised volume (plain torch: matmul, avg_pool2d,
grid_sample) ALTERNATING.

    python tools/raft_probe.py [--out profiles/raft_probe.json] [--rounds 5] [--sizes 1024 2048] [--names small large]

Per configuration and back end: the whole forward between two device events (median and min - max of the turns, one forward
per turn after a warm-up of both back ends), its split by device events at the phase boundaries of one more forward
(encoders; pyramid or volume build; lookup x 12; update convolutions x 12; upsampling), and torch.cuda.max_memory_allocated
of a forward. Per configuration: the lookup kernel alone, staged against EOGS_RAFT_NO_STAGE, for a smooth flow (registration
errors of a few pixels, what this application sees) and a rough one (+-20 px per pixel, independent), `iters` back-to-back
calls between device events, with the bytes a call has to move at least (both maps' pyramids once, coords, the output).
The file is rewritten after every configuration, so an interrupted run keeps what it measured. A back end that fails
(out of memory) is recorded as failed, not skipped in silence.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd import raft  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402

PHASES = ("encoders", "correlation_build", "lookup", "update", "upsampling")


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "turns": len(ts)}


def between_events(fn, iters=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def phased_forward(model, image1, image2, updates, ondemand):
    """RAFT.forward (eogs2_amd/raft.py) with a device event at every phase boundary; returns ({phase: ms}, flow)."""
    marks = []

    def mark(phase):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((phase, e))

    N, _, H, W = image1.shape
    h, w = H // 8, W // 8
    mark(None)
    fmap1, fmap2 = torch.chunk(model.feature_encoder(torch.cat([image1, image2], dim=0)), 2, dim=0)
    context_out = model.context_encoder(image1)
    hidden, context = torch.split(context_out, [model.update_block.hidden_state_size, model.context_size], dim=1)
    hidden, context = torch.tanh(hidden), F.relu(context)
    mark("encoders")
    if ondemand:
        f1cl, pyramid = raft.corr_pyramid(fmap1, 1), raft.corr_pyramid(fmap2, model.corr_levels)
    else:
        pyramid = raft.volume_pyramid(fmap1, fmap2, model.corr_levels)
    mark("correlation_build")
    ys, xs = torch.meshgrid(torch.arange(h, dtype=image1.dtype, device=image1.device),
                            torch.arange(w, dtype=image1.dtype, device=image1.device), indexing="ij")
    coords0 = torch.stack([xs, ys], dim=0)[None].repeat(N, 1, 1, 1)
    coords1 = coords0.clone()
    for _ in range(updates):
        corr = raft.corr_lookup(f1cl, pyramid, coords1, model.corr_radius) if ondemand else raft.volume_lookup(pyramid, coords1, model.corr_radius)
        mark("lookup")
        hidden, delta = model.update_block(hidden, context, corr, coords1 - coords0)
        coords1 = coords1 + delta
        mark("update")
    mask = None if model.mask_predictor is None else model.mask_predictor(hidden)
    flow = coords1 - coords0
    up = raft.upsample_flow(flow, mask) if ondemand else raft._upsample_torch(flow, mask)
    mark("upsampling")
    torch.cuda.synchronize()
    ms = dict.fromkeys(PHASES, 0.0)
    for (_, a), (phase, b) in zip(marks[:-1], marks[1:]):
        ms[phase] += a.elapsed_time(b)
    return ms, up


def lookup_alone(model, h, w, iters, rounds, dev):
    C, r, L = model.feature_encoder.conv.out_channels, model.corr_radius, model.corr_levels
    g = torch.Generator().manual_seed(h + w)
    f1, f2 = torch.randn(1, C, h, w, generator=g).to(dev), torch.randn(1, C, h, w, generator=g).to(dev)
    f1cl, pyr = raft.corr_pyramid(f1, 1), raft.corr_pyramid(f2, L)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None]
    flows = {"smooth": torch.stack([2.5 * torch.sin(0.011 * xs + 0.007 * ys) + 0.3, 1.5 * torch.cos(0.009 * xs - 0.013 * ys)])[None],
             "rough": (torch.rand(1, 2, h, w, generator=g) * 2 - 1) * 20}
    K = 2 * r + 1
    nbytes = f1cl.buffer.numel() + pyr.buffer.numel() + 2 * h * w * 4 + L * K * K * h * w * 4
    flops = 2 * h * w * L * (K + 1) ** 2 * C
    out = {"bytes_at_least": nbytes, "flop": flops}
    for name, fl in flows.items():
        c = (grid + fl).to(dev)
        a, b = raft.corr_lookup(f1cl, pyr, c, r), raft.corr_lookup(f1cl, pyr, c, r, no_stage=True)
        assert torch.equal(a, b)  # faster and different is not faster
        ts = {"staged": [], "no_stage": []}
        for _ in range(rounds):
            ts["staged"].append(between_events(lambda: raft.corr_lookup(f1cl, pyr, c, r), iters))
            ts["no_stage"].append(between_events(lambda: raft.corr_lookup(f1cl, pyr, c, r, no_stage=True), iters))
        row = {k: summary(v) for k, v in ts.items()}
        for v in row.values():
            v["GB_per_s_at_least"] = nbytes / (v["median_ms"] * 1e-3) / 1e9
            v["TFLOP_per_s"] = flops / (v["median_ms"] * 1e-3) / 1e12
        row["no_stage_over_staged"] = row["no_stage"]["median_ms"] / row["staged"]["median_ms"]
        out[name] = row
    return out


def configuration(name, size, updates, rounds, iters, dev):
    torch.manual_seed(7)
    model = raft.RAFT(name).eval().to(dev)
    g = torch.Generator().manual_seed(size)
    base = torch.rand(1, 3, size + 8, size + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev).contiguous(), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev).contiguous()
    row = {"feature_positions": (size // 8) ** 2}
    alive = {}
    with torch.inference_mode():
        for backend in ("ondemand", "volume"):  # warm-up of both back ends, and their memory
            model.corr = backend
            try:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                flow = model(a, b, num_flow_updates=updates)[-1]
                torch.cuda.synchronize()
                alive[backend] = flow
                row[backend] = {"max_memory_allocated_bytes": torch.cuda.max_memory_allocated(), "allocated_before_bytes": before}
            except torch.OutOfMemoryError as e:
                row[backend] = {"failed": "out of memory: " + str(e).splitlines()[0]}
                torch.cuda.empty_cache()
        if len(alive) == 2:
            row["largest_flow_difference_px"] = float((alive["ondemand"] - alive["volume"]).abs().max())
            row["largest_flow_px"] = float(alive["volume"].abs().max())
        ts = {k: [] for k in alive}
        for _ in range(rounds):
            for backend in alive:
                model.corr = backend
                ts[backend].append(between_events(lambda: model(a, b, num_flow_updates=updates)))
        for backend in alive:
            row[backend]["forward"] = summary(ts[backend])
            row[backend]["split_ms"] = phased_forward(model, a, b, updates, backend == "ondemand")[0]
        if len(alive) == 2:
            row["volume_over_ondemand"] = row["volume"]["forward"]["median_ms"] / row["ondemand"]["forward"]["median_ms"]
        del alive
        torch.cuda.empty_cache()
        row["lookup_kernel"] = lookup_alone(model, size // 8, size // 8, iters, rounds, dev)
    print(name, size, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raft_probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--updates", type=int, default=12)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--names", nargs="+", default=["small", "large"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.rounds >= 5, "medians of at least five turns"
    dev = torch.device("cuda:0")
    tw, th, pos = raft.stage_info()
    out = {"what": f"eogs2_amd.raft RAFT forward, fp32, batch 1, {a.updates} updates, seeded random weights, inference_mode; the on-demand "
                   f"correlation (HIP) and the materialised volume (plain torch) alternating, {a.rounds} turns of one forward each between "
                   "device events after a warm-up of both; split_ms: device events at the phase boundaries of one further forward; "
                   f"lookup_kernel: {a.iters} back-to-back calls per turn, staged and EOGS_RAFT_NO_STAGE alternating",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "lookup_tile": [tw, th], "staged_positions": pos,
           "configurations": {}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.names:
        for size in a.sizes:
            out["configurations"][f"{name} {size}x{size}"] = configuration(name, size, a.updates, a.rounds, a.iters, dev)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    out["not_measured"] = ("pretrained weights (none at hand: the flows of random weights are not those of a trained network, which "
                           "moves the lookup's windows); batches above 1; kernel times from a profiler trace; more than one GPU")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
