"""RAFT-small's update block on one GPU: eogs2_amd.raft's fused update (the eogs_flownet_* convolutions) against the torch
modules of the same checkout, ALTERNATING, at 1024^2 and 2048^2, batch 1, 12 updates, seeded random weights, inference_mode,
over the on-demand correlation.

    python tools/raft_update_probe.py [--out profiles/raft_update_probe.json] [--rounds 5] [--sizes 1024 2048]

Per size and path, medians and min - max of `rounds` turns after a warm-up of both paths: the update phase alone (device
events around each of the 12 updates of a forward, the lookups excluded, summed), the whole forward between two device events,
and for the fused path `begin` alone (the repacking of the weights, the hidden state's layout and the hoisted context
planes; it is part of the fused forward, not of its update phase, and is reported beside it and added in
`update_plus_begin`). Also torch.cuda.max_memory_allocated of a forward, the fused workspace's bytes, and the largest
difference between the two paths' flows. The verdict is the rule RAFT(update="auto") follows: fused only if at every size
the slowest fused turn of the update phase PLUS begin is faster than the fastest torch turn. The file is rewritten after
every size, so an interrupted run keeps what it measured.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from raft_probe import between_events, summary  # noqa: E402

from eogs2_amd import _lib, raft  # noqa: E402
from eogs2_amd._host import query_bytes  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402

LAUNCHES_PER_FUSED_UPDATE = 8  # include/eogs_resample.h, eogs_flownet_update_step: one per convolution


def phased_forward(model, image1, image2, updates, fused):
    """RAFT.forward (eogs2_amd/raft.py, on-demand correlation) with device events around `begin` and around every update;
    returns ({"begin": ms, "update": ms over all updates}, flow)."""
    pairs = {"begin": [], "update": []}

    def timed(phase, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        pairs[phase].append((a, b))
        return out

    N, _, H, W = image1.shape
    h, w = H // 8, W // 8
    fmap1, fmap2 = torch.chunk(model.feature_encoder(torch.cat([image1, image2], dim=0)), 2, dim=0)
    hidden, context = torch.split(model.context_encoder(image1), [model.update_block.hidden_state_size, model.context_size], dim=1)
    hidden, context = torch.tanh(hidden), F.relu(context)
    f1cl, pyramid = raft.corr_pyramid(fmap1, 1), raft.corr_pyramid(fmap2, model.corr_levels)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=image1.dtype, device=image1.device),
                            torch.arange(w, dtype=image1.dtype, device=image1.device), indexing="ij")
    coords0 = torch.stack([xs, ys], dim=0)[None].repeat(N, 1, 1, 1)
    coords1 = coords0.clone()
    if fused:
        timed("begin", lambda: model._fused.begin(hidden, context))
    for _ in range(updates):
        corr = raft.corr_lookup(f1cl, pyramid, coords1, model.corr_radius)
        flow = coords1 - coords0
        if fused:
            delta = timed("update", lambda: model._fused.step(corr, flow))
        else:
            hidden, delta = timed("update", lambda: model.update_block(hidden, context, corr, flow))
        coords1 = coords1 + delta
    up = raft.upsample_flow(coords1 - coords0, None)
    torch.cuda.synchronize()
    return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in pairs.items()}, up


def configuration(size, updates, rounds, dev):
    torch.manual_seed(7)
    model = raft.raft_small(corr="ondemand").eval().to(dev)
    g = torch.Generator().manual_seed(size)
    base = torch.rand(1, 3, size + 8, size + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev).contiguous(), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev).contiguous()
    h = w = size // 8
    row = {"feature_positions": h * w, "fused_workspace_bytes": query_bytes(_lib.get(), "flownet_update_bytes", 1, h, w),
           "launches_per_update": {"fused": LAUNCHES_PER_FUSED_UPDATE, "torch": "not measured"}}
    paths = ("fused", "torch")
    flows = {}
    with torch.inference_mode():
        for path in paths:  # warm-up of both paths, and their memory
            model.update = path
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            flows[path] = model(a, b, num_flow_updates=updates)[-1]
            phased_forward(model, a, b, updates, path == "fused")
            torch.cuda.synchronize()
            row[path] = {"max_memory_allocated_bytes": torch.cuda.max_memory_allocated(), "allocated_before_bytes": before}
        row["largest_flow_difference_px"] = float((flows["fused"] - flows["torch"]).abs().max())
        row["largest_flow_px"] = float(flows["torch"].abs().max())
        ts = {p: {"forward": [], "update": [], "begin": []} for p in paths}
        for _ in range(rounds):
            for path in paths:
                model.update = path
                ts[path]["forward"].append(between_events(lambda: model(a, b, num_flow_updates=updates)))
                ms, _ = phased_forward(model, a, b, updates, path == "fused")
                ts[path]["update"].append(ms["update"])
                ts[path]["begin"].append(ms["begin"])
    for path in paths:
        row[path]["forward"] = summary(ts[path]["forward"])
        row[path]["update_phase"] = summary(ts[path]["update"])
    row["fused"]["begin"] = summary(ts["fused"]["begin"])
    row["fused"]["update_plus_begin"] = summary([u + b for u, b in zip(ts["fused"]["update"], ts["fused"]["begin"])])
    row["torch_over_fused_update_phase"] = row["torch"]["update_phase"]["median_ms"] / row["fused"]["update_plus_begin"]["median_ms"]
    row["torch_over_fused_forward"] = row["torch"]["forward"]["median_ms"] / row["fused"]["forward"]["median_ms"]
    row["fused_outside_the_spread"] = row["fused"]["update_plus_begin"]["max_ms"] < row["torch"]["update_phase"]["min_ms"]
    print(size, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raft_update_probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=12)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.rounds >= 5, "medians of at least five turns"
    dev = torch.device("cuda:0")
    out = {"what": f"eogs2_amd.raft RAFT-small forward, fp32, batch 1, {a.updates} updates, seeded random weights, inference_mode, on-demand "
                   f"correlation; update='fused' (HIP) and update='torch' alternating, {a.rounds} turns after a warm-up of both; update_phase: "
                   "device events around each update of one forward per turn, summed (lookups excluded); begin: the fused path's once-per-"
                   "forward repacking and hoisted planes; forward: one whole forward per turn between device events",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "conv_tile": list(raft.conv_info()),
           "auto_rule": "fused only if at every size fused update_plus_begin max_ms < torch update_phase min_ms", "configurations": {}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for size in a.sizes:
        out["configurations"][f"small {size}x{size}"] = configuration(size, a.updates, a.rounds, dev)
        out["auto_selects_fused"] = all(c["fused_outside_the_spread"] for c in out["configurations"].values())
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    out["not_measured"] = ("batches above 1; pretrained weights (none at hand); the kernels under a profiler (per-kernel times, launch "
                           "gaps); the torch path's launches per update; more than one GPU")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
