"""The optimizer step inside the recorded graph against the optimizers outside it, on one GPU, same commit:

    examples/train_synthetic.py --graph --random-camera                         (both optimizers and the host walk outside)
    examples/train_synthetic.py --graph --random-camera --optimizer-in-graph    (FusedAdam(capturable=True) behind the gate)

at 100 000 Gaussians / 512^2 and 1 048 576 Gaussians / 1024^2.

    python tools/step_probe.py [--out profiles/step_probe.json] [--iters 320] [--warmup 100] [--rounds 3]

Per size the two variants alternate, `rounds` runs each. From the example's host stamps (before / after each iteration's
replay; the replay's fit check waits for that replay's counts, so the host cannot run ahead of the device by more than one
iteration) a run yields: ms per iteration = the median distance between the starts of consecutive iterations after `warmup`
(at least 200 of them), and the host time between two replays = the median time from a replay's return to the next replay's
call. Reported: the median over the runs and their spread (max - min of the run medians). The number of graph nodes comes from
a short run of its own with the graph's debug dump (null where the runtime gives none). The last block replays a captured
capturable step 3000 times and compares the prologue's fp32 scalars of every replay with the host's.

No speed ratio is asserted here; the file records what was measured and what was not.
"""
import argparse
import json
import math
import os
import re
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from eogs2_amd.build import source_hash  # noqa: E402
from eogs2_amd.optim import FusedAdam  # noqa: E402

SIZES = ((100_000, 512), (1_048_576, 1024))


def run(train_synthetic, P, size, iters, warmup, inside):
    args = ["--gaussians", str(P), "--size", str(size), "--iters", str(iters), "--quiet", "--graph", "--random-camera"]
    first, last, n = train_synthetic.main(args + (["--optimizer-in-graph"] if inside else []))
    st = train_synthetic.main.last_stamps[warmup:]
    starts = np.array([a for a, _ in st])
    per_iter = np.diff(starts) * 1e3
    between = np.array([st[i + 1][0] - st[i][1] for i in range(len(st) - 1)]) * 1e6
    step = train_synthetic.main.last_step
    return {"ms_per_iter_median": float(np.median(per_iter)), "iterations": int(per_iter.size),
            "host_between_replays_us_median": float(np.median(between)), "recordings_outgrown": int(step.recaptures),
            "first_loss": first, "last_loss": last, "gaussians_left": n}


def graph_nodes(train_synthetic, P, size, inside):
    """Nodes of the recorded step from the graph's debug dump, in a short run of its own (the debug mode keeps the graph)."""
    orig = torch.cuda.CUDAGraph.capture_begin

    def capture_begin(self, *a, **k):
        self.enable_debug_mode()
        return orig(self, *a, **k)

    torch.cuda.CUDAGraph.capture_begin = capture_begin
    try:
        args = ["--gaussians", str(P), "--size", str(size), "--iters", "4", "--quiet", "--graph", "--random-camera", "--no-prune"]
        train_synthetic.main(args + (["--optimizer-in-graph"] if inside else []))
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "graph.dot")
            train_synthetic.main.last_step.graph.debug_dump(path)
            dot = open(path).read()
        return len(re.findall(r"^\s*\"?[A-Za-z_0-9]+\"?\s*\[", dot, flags=re.M)) or None
    except Exception as e:  # the runtime has no dump: recorded as not measured
        print("graph nodes not available:", repr(e), flush=True)
        return None
    finally:
        torch.cuda.CUDAGraph.capture_begin = orig


def ulp_share(dev, replays=3000):
    """Share of replays of a captured capturable step whose prologue scalars differ from the host's double expressions rounded
    to fp32 (what eogs_adam_step passes): one tensor, betas (0.9, 0.999), t = 1 .. replays."""
    p = torch.nn.Parameter(torch.zeros(64, device=dev))
    p.grad = torch.ones(64, device=dev)
    opt = FusedAdam([{"params": [p], "lr": 1e-3, "name": "x"}], lr=0.0, eps=1e-15, capturable=True)
    opt.step()
    opt.state[p]["step"].zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    rows = torch.empty((replays, 4), device=dev)
    for t in range(replays):
        g.replay()
        rows[t].copy_(opt.step_scalars(p))
    got = rows.cpu().numpy()
    t = np.arange(1, replays + 1, dtype=np.float64)
    want1 = np.array([np.float32(1.0 / (1.0 - 0.9 ** int(k))) for k in t])
    want2 = np.array([np.float32(math.sqrt(1.0 - 0.999 ** int(k))) for k in t])
    d1, d2 = got[:, 1] != want1, got[:, 2] != want2
    ulps = max(float(np.max(np.abs(got[:, 1].astype(np.float64) - want1) / np.spacing(want1))),
               float(np.max(np.abs(got[:, 2].astype(np.float64) - want2) / np.spacing(want2))))
    assert int(opt.state[p]["step"]) == replays
    return {"replays": replays, "share_inv_bc1_differs": float(d1.mean()), "share_sqrt_bc2_differs": float(d2.mean()),
            "share_any_differs": float((d1 | d2).mean()), "largest_difference_ulp": ulps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_probe.json"))
    ap.add_argument("--iters", type=int, default=320)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default=None, help="P:size,P:size (default: the two of the module docstring)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.iters - a.warmup - 1 >= 200, "at least 200 timed iterations"
    import train_synthetic

    dev = torch.device("cuda:0")
    sizes = SIZES if not a.sizes else tuple(tuple(int(x) for x in s.split(":")) for s in a.sizes.split(","))
    out = {"what": "examples/train_synthetic.py --graph --random-camera, optimizers outside the recorded step against "
                   f"--optimizer-in-graph; the variants alternate, {a.rounds} runs each of {a.iters} iterations, the first {a.warmup} "
                   "dropped; host clock stamps around every replay (the fit check ties the host to the device within one iteration)",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "sizes": []}
    for P, size in sizes:
        runs = {"outside": [], "inside": []}
        for r in range(a.rounds):
            for name in ("outside", "inside"):
                runs[name].append(run(train_synthetic, P, size, a.iters, a.warmup, name == "inside"))
                print(P, size, name, json.dumps(runs[name][-1]), flush=True)
        row = {"gaussians": P, "size": size}
        for name in runs:
            ms = [x["ms_per_iter_median"] for x in runs[name]]
            row[name] = {"ms_per_iter": float(np.median(ms)), "ms_per_iter_runs": ms, "spread_ms": float(max(ms) - min(ms)),
                         "host_between_replays_us": float(np.median([x["host_between_replays_us_median"] for x in runs[name]])),
                         "timed_iterations_per_run": runs[name][0]["iterations"],
                         "recordings_outgrown": [x["recordings_outgrown"] for x in runs[name]],
                         "losses": [(x["first_loss"], x["last_loss"], x["gaussians_left"]) for x in runs[name]]}
        row["inside_minus_outside_ms"] = row["inside"]["ms_per_iter"] - row["outside"]["ms_per_iter"]
        row["inside_not_slower_than_outside_spread"] = bool(row["inside_minus_outside_ms"] <= row["outside"]["spread_ms"])
        for name in runs:
            row[name]["graph_nodes"] = graph_nodes(train_synthetic, P, size, name == "inside")
        out["sizes"].append(row)
        print(json.dumps(row), flush=True)
    out["prologue_scalars_against_host"] = ulp_share(dev)
    print(json.dumps(out["prologue_scalars_against_host"]), flush=True)
    out["not_measured"] = ("per-kernel times of the prologue and the element kernel (no profiler run); other scene sizes and flag "
                           "mixes (--parallel-renders, --defer-prune, --densify-every); more than one GPU (the in-graph step is "
                           "single-rank); a host under load from other processes beyond what the runs' spread shows")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
