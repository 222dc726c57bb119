"""RAFT-large's update block and mask predictor on one GPU: eogs2_amd.raft's fused path (update="fused_large", the
eogs_flowlarge_* entries of include/eogs_resample.h) against the torch modules of the same checkout, ALTERNATING,
at 1024^2 and 2048^2, batch 1, 12 updates, seeded random weights, inference_mode, over the on-demand correlation. The
protocol is tools/raft_update_probe.py's.

    python tools/raft_large_update_probe.py [--out profiles/raft_large_update_probe.json] [--rounds 5] [--sizes 1024 2048]

Per size and path, medians and min - max of `rounds` turns after a warm-up of both paths: the update phase alone (device
events around each of the 12 updates of a forward and around the mask predictor's one call after the last, the lookups
excluded, summed; the mask's share is also given alone), the whole forward between two device events, and for the fused path
`begin` alone (the repacking of the weights, the hidden state's layout and the four hoisted context planes; it is part of
the fused forward, not of its update phase, and is reported beside it and added in `update_plus_begin`). Also
torch.cuda.max_memory_allocated of a forward, the fused workspace's bytes, and the largest difference between the two paths'
flows. The verdict is the rule used for RAFT-small: fused wins only if at every size the slowest fused turn of the update
phase PLUS begin is faster than the fastest torch turn. RAFT(update="auto") does not follow it for RAFT-large (it stays the
torch modules); raft.AUTO_UPDATE_LARGE_IS_FUSED records it. The file is rewritten after every size, so an interrupted run
keeps what it measured.
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

from eogs2_amd import raft  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402

LAUNCHES_PER_FUSED_UPDATE, LAUNCHES_PER_FUSED_MASK = 11, 2  # include/eogs_resample.h: one per convolution


def multiply_adds_per_position():
    """Multiply-adds per feature position and update of the twelve convolutions of one update (the mask head excluded), as
    torch runs them and as the fused path does with the context's 128 channels of the six GRU convolutions hoisted."""
    plain = 324 * 256 + 256 * 9 * 192 + 2 * 49 * 128 + 128 * 9 * 64 + 256 * 9 * 126 + 128 * 9 * 256 + 256 * 9 * 2
    return {"torch": plain + 6 * 384 * 5 * 128, "fused": plain + 6 * 256 * 5 * 128, "fused_begin_once": 6 * 128 * 5 * 128,
            "mask_once": 128 * 9 * 256 + 256 * 576}


def phased_forward(model, image1, image2, updates, fused):
    """RAFT.forward (eogs2_amd/raft.py, on-demand correlation) with device events around `begin`, around every update and
    around the mask; returns ({"begin": ms, "update": ms over all updates, "mask": ms}, flow)."""
    pairs = {"begin": [], "update": [], "mask": []}

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
        timed("begin", lambda: model._fused_large.begin(hidden, context))
    for _ in range(updates):
        corr = raft.corr_lookup(f1cl, pyramid, coords1, model.corr_radius)
        flow = coords1 - coords0
        if fused:
            delta = timed("update", lambda: model._fused_large.step(corr, flow))
        else:
            hidden, delta = timed("update", lambda: model.update_block(hidden, context, corr, flow))
        coords1 = coords1 + delta
    mask = timed("mask", (lambda: model._fused_large.mask()) if fused else (lambda: model.mask_predictor(hidden)))
    up = raft.upsample_flow(coords1 - coords0, mask)
    torch.cuda.synchronize()
    return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in pairs.items()}, up


def configuration(size, updates, rounds, dev):
    torch.manual_seed(7)
    model = raft.raft_large(corr="ondemand").eval().to(dev)
    g = torch.Generator().manual_seed(size)
    base = torch.rand(1, 3, size + 8, size + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev).contiguous(), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev).contiguous()
    h = w = size // 8
    row = {"feature_positions": h * w, "fused_workspace_bytes": raft.FusedUpdateLarge.workspace_bytes(1, h, w),
           "launches": {"fused_per_update": LAUNCHES_PER_FUSED_UPDATE, "fused_per_mask": LAUNCHES_PER_FUSED_MASK, "torch": "not measured"}}
    paths = {"fused": "fused_large", "torch": "torch"}
    flows = {}
    with torch.inference_mode():
        for path, update in paths.items():  # warm-up of both paths, and their memory (the fused workspace is made here, inside the peak)
            model.update = update
            model._fused_large._ws.clear()
            model._fused_large._state = None  # (no workspace is held when a path's peak is taken)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            flows[path] = model(a, b, num_flow_updates=updates)[-1]
            torch.cuda.synchronize()
            row[path] = {"max_memory_allocated_bytes": torch.cuda.max_memory_allocated(), "allocated_before_bytes": before}
            _, same = phased_forward(model, a, b, updates, path == "fused")
            row[path]["phased_forward_gives_the_forward_s_bits"] = bool(torch.equal(same, flows[path]))
        row["largest_flow_difference_px"] = float((flows["fused"] - flows["torch"]).abs().max())
        row["largest_flow_px"] = float(flows["torch"].abs().max())
        ts = {p: {"forward": [], "update": [], "begin": [], "mask": []} for p in paths}
        for _ in range(rounds):
            for path, update in paths.items():
                model.update = update
                ts[path]["forward"].append(between_events(lambda: model(a, b, num_flow_updates=updates)))
                ms, _ = phased_forward(model, a, b, updates, path == "fused")
                ts[path]["update"].append(ms["update"] + ms["mask"])
                ts[path]["mask"].append(ms["mask"])
                ts[path]["begin"].append(ms["begin"])
    for path in paths:
        row[path]["forward"] = summary(ts[path]["forward"])
        row[path]["update_phase"] = summary(ts[path]["update"])
        row[path]["mask_alone"] = summary(ts[path]["mask"])
    row["fused"]["begin"] = summary(ts["fused"]["begin"])
    row["fused"]["update_plus_begin"] = summary([u + b for u, b in zip(ts["fused"]["update"], ts["fused"]["begin"])])
    row["torch_over_fused_update_phase"] = row["torch"]["update_phase"]["median_ms"] / row["fused"]["update_plus_begin"]["median_ms"]
    row["torch_over_fused_forward"] = row["torch"]["forward"]["median_ms"] / row["fused"]["forward"]["median_ms"]
    row["fused_outside_the_spread"] = row["fused"]["update_plus_begin"]["max_ms"] < row["torch"]["update_phase"]["min_ms"]
    row["torch_outside_the_spread"] = row["torch"]["update_phase"]["max_ms"] < row["fused"]["update_plus_begin"]["min_ms"]
    ma = multiply_adds_per_position()
    per_update_ms = (row["fused"]["update_phase"]["median_ms"] - row["fused"]["mask_alone"]["median_ms"]) / updates
    row["fused_tflops_over_its_update_kernels"] = 2 * ma["fused"] * h * w / (per_update_ms * 1e-3) / 1e12  # (launch gaps included)
    per_update_ms = (row["torch"]["update_phase"]["median_ms"] - row["torch"]["mask_alone"]["median_ms"]) / updates
    row["torch_tflops_over_its_update_modules"] = 2 * ma["torch"] * h * w / (per_update_ms * 1e-3) / 1e12
    print(size, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raft_large_update_probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=12)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.rounds >= 5, "medians of at least five turns"
    dev = torch.device("cuda:0")
    out = {"what": f"eogs2_amd.raft RAFT-large forward, fp32, batch 1, {a.updates} updates, seeded random weights, inference_mode, on-demand "
                   f"correlation; update='fused_large' (HIP) and update='torch' alternating, {a.rounds} turns after a warm-up of both; "
                   "update_phase: device events around each update of one forward per turn and around the mask predictor's one call, "
                   "summed (lookups excluded); mask_alone: that one call; begin: the fused path's once-per-forward repacking and hoisted "
                   "planes; forward: one whole forward per turn between device events",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "conv_tile": list(raft.conv_info()),
           "multiply_adds_per_position": multiply_adds_per_position(),
           "rule": "fused wins only if at every size fused update_plus_begin max_ms < torch update_phase min_ms; update='auto' stays the "
                   "torch modules for RAFT-large either way", "configurations": {}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for size in a.sizes:
        out["configurations"][f"large {size}x{size}"] = configuration(size, a.updates, a.rounds, dev)
        out["fused_wins"] = all(c["fused_outside_the_spread"] for c in out["configurations"].values())
        out["torch_wins"] = all(c["torch_outside_the_spread"] for c in out["configurations"].values())
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    out["not_measured"] = ("batches above 1; pretrained weights (none at hand); the kernels under a profiler (per-kernel times, launch "
                           "gaps: the TFLOP/s figures divide by event time, gaps included); the torch path's launches per update; more "
                           "than one GPU")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
