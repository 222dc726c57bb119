"""RAFT-small's two encoders on one GPU: eogs2_amd.raft's fused encoders (the eogs_flowenc_* entries) against the torch modules
of the same checkout, ALTERNATING, at 1024^2 and 2048^2, batch 1, seeded random weights, inference_mode.

    python tools/raft_encoder_probe.py [--out profiles/raft_encoder_probe.json] [--rounds 5] [--sizes 1024 2048]

Per size and path, medians and min - max of `rounds` turns after a warm-up of both paths: the encoder phase alone (device
events around the feature encoder on the two images followed by the context encoder, what RAFT.forward runs), each encoder
alone, and the whole forward with update="fused" between two device events. Also torch.cuda.max_memory_allocated of one
forward per path, each measured after every kept workspace was released and the cache emptied (the fused encoders keep
their workspaces between forwards: measured after the other path, one path's peak would hold the other's memory), the two
fused workspaces' bytes, the largest difference between the two paths' flows, and the bytes the fused
launches move by the shapes of their operands (an estimate from the launch list of include/eogs_resample.h, NOT a counter
reading) with the bandwidth that implies. The verdict is the rule RAFT(encoder="auto") follows: fused only if at every size
the slowest fused turn of the encoder phase is faster than the fastest torch turn. The file is rewritten after every size, so
an interrupted run keeps what it measured.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from raft_probe import between_events, summary  # noqa: E402

from eogs2_amd import raft  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402


def estimated_bytes(N, H, W, normed, head):
    """Bytes the fused launches read and write, from their operands' shapes: each convolution its input once and its output
    once (the stride-2 1 x 1 downsample a quarter of its input's positions, rounded up to whole 64-byte lines: all of it), each
    finish its two or three maps; weights, partials and norm tables left out (well under 1 %)."""
    widths = (32, 32, 64, 96)
    h, w = (H + 1) // 2, (W + 1) // 2
    total = 4 * N * (3 * H * W + 32 * h * w)  # the stem
    if normed:
        total += 4 * N * 2 * 32 * h * w  # finish: read, write
    for L in (1, 2, 3):
        for B in (0, 1):
            cin, cout = (widths[L - 1] if B == 0 else widths[L]), widths[L]
            down = B == 0 and L > 1
            ho, wo = ((h + 1) // 2, (w + 1) // 2) if down else (h, w)
            P, Po, mid = N * h * w, N * ho * wo, cout // 4
            total += 4 * (P * cin + P * mid)        # conv1
            total += 4 * (P * mid + Po * mid)       # conv2
            total += 4 * (Po * mid + Po * cout)     # conv3
            if down:
                total += 4 * (P * cin + Po * cout)  # the downsample
            if normed:
                total += 4 * 3 * Po * cout          # finish: v, the shortcut, out
            else:
                total += 4 * Po * cout              # the residual epilogue reads its shortcut
            h, w = ho, wo
    return total + 4 * N * h * w * (96 + head)


def encoder_phase(model, image1, image2, fused):
    feature, context = model._fused_enc if fused else (model.feature_encoder, model.context_encoder)
    feature(torch.cat([image1, image2], dim=0))
    context(image1)


def drop_workspaces(model):
    """Releases what the fused paths keep between forwards (the encoders' workspaces, the update block's), so that one path's
    peak memory is not counted into the other's."""
    for e in model._fused_enc:
        e._ws.clear()
    model._fused._ws.clear()
    model._fused._state = None


def configuration(size, updates, rounds, dev):
    torch.manual_seed(7)
    model = raft.raft_small(corr="ondemand", update="fused").eval().to(dev)
    g = torch.Generator().manual_seed(size)
    base = torch.rand(1, 3, size + 8, size + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev).contiguous(), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev).contiguous()
    both = torch.cat([a, b], dim=0)
    fe, ce = model._fused_enc
    est = estimated_bytes(2, size, size, True, 128) + estimated_bytes(1, size, size, False, 160)
    row = {"fused_workspace_bytes": {"feature (batch 2)": fe.workspace_bytes(2, size, size), "context": ce.workspace_bytes(1, size, size)},
           "estimated_bytes_moved_by_the_fused_launches": est}
    paths = ("fused", "torch")
    flows = {}
    with torch.inference_mode():
        for path in paths:  # warm-up of both paths, and their memory: each from a state in which no workspace is held
            model.encoder = path
            drop_workspaces(model)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            flows[path] = model(a, b, num_flow_updates=updates)[-1]
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            held = sum(ws.numel() for e in model._fused_enc for ws in e._ws.values())
            row[path] = {"max_memory_allocated_bytes": peak, "allocated_before_bytes": before, "forward_peak_above_before_bytes": peak - before,
                         "encoder_workspaces_held_after_bytes": held}
            encoder_phase(model, a, b, path == "fused")
            torch.cuda.synchronize()
        row["largest_flow_difference_px"] = float((flows["fused"] - flows["torch"]).abs().max())
        row["largest_flow_px"] = float(flows["torch"].abs().max())
        ts = {p: {"forward": [], "encoders": [], "feature": [], "context": []} for p in paths}
        for _ in range(rounds):
            for path in paths:
                model.encoder = path
                fused = path == "fused"
                feature, context = model._fused_enc if fused else (model.feature_encoder, model.context_encoder)
                ts[path]["forward"].append(between_events(lambda: model(a, b, num_flow_updates=updates)))
                ts[path]["encoders"].append(between_events(lambda: encoder_phase(model, a, b, fused)))
                ts[path]["feature"].append(between_events(lambda: feature(both)))
                ts[path]["context"].append(between_events(lambda: context(a)))
    for path in paths:
        row[path]["forward"] = summary(ts[path]["forward"])
        row[path]["encoder_phase"] = summary(ts[path]["encoders"])
        row[path]["feature_encoder_two_images"] = summary(ts[path]["feature"])
        row[path]["context_encoder"] = summary(ts[path]["context"])
    row["fused_estimated_bandwidth_TB_s"] = est / (row["fused"]["encoder_phase"]["median_ms"] * 1e-3) / 1e12
    row["torch_over_fused_encoder_phase"] = row["torch"]["encoder_phase"]["median_ms"] / row["fused"]["encoder_phase"]["median_ms"]
    row["torch_over_fused_forward"] = row["torch"]["forward"]["median_ms"] / row["fused"]["forward"]["median_ms"]
    row["fused_outside_the_spread"] = row["fused"]["encoder_phase"]["max_ms"] < row["torch"]["encoder_phase"]["min_ms"]
    print(size, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raft_encoder_probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=12)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.rounds >= 5, "medians of at least five turns"
    dev = torch.device("cuda:0")
    out = {"what": f"eogs2_amd.raft RAFT-small, fp32, batch 1, seeded random weights, inference_mode; encoder='fused' (HIP) and encoder='torch' "
                   f"alternating, {a.rounds} turns after a warm-up of both; encoder_phase: device events around the feature encoder on the two "
                   f"images followed by the context encoder; forward: one whole forward ({a.updates} updates, on-demand correlation, update="
                   "'fused' either way) per turn between device events",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "conv_tile": list(raft.conv_info()),
           "auto_rule": "fused only if at every size fused encoder_phase max_ms < torch encoder_phase min_ms", "configurations": {}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for size in a.sizes:
        out["configurations"][f"small {size}x{size}"] = configuration(size, a.updates, a.rounds, dev)
        out["auto_selects_fused"] = all(c["fused_outside_the_spread"] for c in out["configurations"].values())
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    out["not_measured"] = ("the bytes the kernels move (estimated_bytes_moved_by_the_fused_launches is computed from operand shapes, no counter "
                           "was read); batches above 1 (beyond the feature encoder's pair of images); pretrained weights (none at hand); the "
                           "kernels under a profiler (per-kernel times, launch gaps, LDS conflicts); more than one GPU")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
