"""RAFT-large's two encoders on one GPU: eogs2_amd.raft's fused encoders (the eogs_flowres_* entries) against the torch modules
of the same checkout, ALTERNATING, at 1024^2 and 2048^2, batch 1, seeded random weights with the batch norms randomised
(default ones are the identity), eval mode, inference_mode.

    python tools/raft_large_encoder_probe.py [--out profiles/raft_large_encoder_probe.json] [--rounds 5] [--sizes 1024 2048]

Per size and path, medians and min - max of `rounds` turns after a warm-up of both paths: the encoder phase alone (device
events around the feature encoder on the two images followed by the context encoder, what RAFT.forward runs), each encoder
alone, and the whole forward with update="fused_large" on both sides between two device events. Also
torch.cuda.max_memory_allocated of one forward per path, each measured after every kept workspace was released and the
cache emptied, the two fused workspaces' bytes, and the largest difference between the two paths' flows. The verdict is the
rule of AUTO_ENCODER_LARGE_IS_FUSED: fused only if at every size the slowest fused turn of the encoder phase is faster than
the fastest torch turn. The file is rewritten after every size, so an interrupted run keeps what it measured.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from flowres_cases import randomise_batchnorms  # noqa: E402  (the tests' recipe: one copy of it)
from raft_probe import between_events, summary  # noqa: E402

from eogs2_amd import raft  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402


def encoder_phase(model, image1, image2, fused):
    feature, context = model._fused_enc_large if fused else (model.feature_encoder, model.context_encoder)
    feature(torch.cat([image1, image2], dim=0))
    context(image1)


def drop_workspaces(model):
    """Releases what the fused paths keep between forwards (the encoders' workspaces, the update block's), so that one path's
    peak memory is not counted into the other's."""
    for e in model._fused_enc_large:
        e._ws.clear()
    model._fused_large._ws.clear()
    model._fused_large._state = None


def configuration(size, updates, rounds, dev):
    torch.manual_seed(7)
    model = raft.raft_large(corr="ondemand", update="fused_large").eval()
    randomise_batchnorms(model, 8)
    model = model.to(dev)
    g = torch.Generator().manual_seed(size)
    base = torch.rand(1, 3, size + 8, size + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev).contiguous(), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev).contiguous()
    both = torch.cat([a, b], dim=0)
    fe, ce = model._fused_enc_large
    row = {"fused_workspace_bytes": {"feature (batch 2)": fe.workspace_bytes(2, size, size), "feature (per image)": fe.workspace_bytes(1, size, size),
                                     "context": ce.workspace_bytes(1, size, size)}}
    paths = {"fused": "fused_large", "torch": "torch"}
    flows = {}
    with torch.inference_mode():
        for path, encoder in paths.items():  # warm-up of both paths, and their memory: each from a state in which no workspace is held
            model.encoder = encoder
            drop_workspaces(model)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            flows[path] = model(a, b, num_flow_updates=updates)[-1]
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            held = sum(ws.numel() for e in model._fused_enc_large for ws in e._ws.values())
            row[path] = {"max_memory_allocated_bytes": peak, "allocated_before_bytes": before, "forward_peak_above_before_bytes": peak - before,
                         "encoder_workspaces_held_after_bytes": held}
            encoder_phase(model, a, b, path == "fused")
            torch.cuda.synchronize()
        row["largest_flow_difference_px"] = float((flows["fused"] - flows["torch"]).abs().max())
        row["largest_flow_px"] = float(flows["torch"].abs().max())
        ts = {p: {"forward": [], "encoders": [], "feature": [], "context": []} for p in paths}
        for _ in range(rounds):
            for path, encoder in paths.items():
                model.encoder = encoder
                fused = path == "fused"
                feature, context = model._fused_enc_large if fused else (model.feature_encoder, model.context_encoder)
                ts[path]["forward"].append(between_events(lambda: model(a, b, num_flow_updates=updates)))
                ts[path]["encoders"].append(between_events(lambda: encoder_phase(model, a, b, fused)))
                ts[path]["feature"].append(between_events(lambda: feature(both)))
                ts[path]["context"].append(between_events(lambda: context(a)))
    for path in paths:
        row[path]["forward"] = summary(ts[path]["forward"])
        row[path]["encoder_phase"] = summary(ts[path]["encoders"])
        row[path]["feature_encoder_two_images"] = summary(ts[path]["feature"])
        row[path]["context_encoder"] = summary(ts[path]["context"])
    row["torch_over_fused_encoder_phase"] = row["torch"]["encoder_phase"]["median_ms"] / row["fused"]["encoder_phase"]["median_ms"]
    row["torch_over_fused_forward"] = row["torch"]["forward"]["median_ms"] / row["fused"]["forward"]["median_ms"]
    row["fused_outside_the_spread"] = row["fused"]["encoder_phase"]["max_ms"] < row["torch"]["encoder_phase"]["min_ms"]
    print(size, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raft_large_encoder_probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=12)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.rounds >= 5, "medians of at least five turns"
    dev = torch.device("cuda:0")
    out = {"what": f"eogs2_amd.raft RAFT-large, fp32, batch 1, seeded random weights, randomised batch norms, eval mode, inference_mode; "
                   f"encoder='fused_large' (HIP) and encoder='torch' alternating, {a.rounds} turns after a warm-up of both; encoder_phase: device "
                   f"events around the feature encoder on the two images followed by the context encoder; forward: one whole forward "
                   f"({a.updates} updates, on-demand correlation, update='fused_large' either way) per turn between device events",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "conv_tile": list(raft.conv_info()),
           "launches": {"feature": "16 convolutions + 15 norms + 7 pointwise passes + 16 packings", "context": "16 convolutions + 15 folds + 16 packings"},
           "auto_rule": "fused only if at every size fused encoder_phase max_ms < torch encoder_phase min_ms", "configurations": {}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for size in a.sizes:
        out["configurations"][f"large {size}x{size}"] = configuration(size, a.updates, a.rounds, dev)
        out["auto_selects_fused"] = all(c["fused_outside_the_spread"] for c in out["configurations"].values())
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    out["not_measured"] = ("pretrained weights (none at hand); batches above 1 (beyond the feature encoder's pair of images); the kernels "
                           "under a profiler (per-kernel times, launch gaps, LDS conflicts); the bytes the kernels move; more than one GPU")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
