"""The device-side view bank on one GPU (eogs2_amd.views) against what it replaces, on the same card:

  bank      per iteration `bank.load()` + `bank.store()` + `schedule.advance()` (three launches) over one ground truth of
            3 x S^2 fp32 (S = 1024 and 2048, LOAD only) plus twelve small state slots (a colour camera's weight [3,3,1,1], bias
            [3] and in-shadow tint [3,1,1], their two Adam moments each and three step counts), against
  copy_     the same bytes moved by per-tensor `copy_` calls — 13 into the working tensors, 12 back into the view's rows: the
            alternative a user has today — and against
  single    ONE device `copy_` of the large slot alone, which the load can at best equal; beside them
  load      `bank.load()` alone (one launch, all thirteen slots), the figure to hold against `single`, and
  graph     load + store + advance recorded into a HIP graph and replayed, one iteration per replay;
  device    the kernels without the host: 16 x (load, advance) in ONE recorded graph, minus 16 x advance in another, per load,
            against 16 `copy_` of the large slot in a third (each on the next view): eager calls of the bank are bound by the
            host's Python and launch path, which a recorded step does not pay;

  example   examples/train_synthetic.py at `--gaussians` / `--size` with --graph --optimizer-in-graph: --views 8 against
            --views 1, steady-state ms per iteration (main.last_ms_per_iter: the last half of the run).

    python tools/views_probe.py [--out profiles/views_probe.json] [--rounds 7] [--iters 50] [--gaussians 1000000] [--size 1024]

Times: after a warm-up the paths alternate, `rounds` turns each; a turn of the copy paths is `iters` iterations between two
device events, each iteration on the next of 8 views (8 x 50 MB of rows: more than the caches keep); a turn of the example is
one run. Reported per path: the median turn and the spread of the turns (min, max), and the ratios of the medians. No speed
ratio is an acceptance condition of this feature; the file records what was measured and what was not.
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

from eogs2_amd.build import source_hash  # noqa: E402
from eogs2_amd.views import ViewBank, ViewSchedule  # noqa: E402

V = 8
IN_GRAPH = 16  # loads (or copies) per recorded graph of the device-side comparison
SMALL = [(3, 3, 1, 1), (3,), (3, 1, 1)] * 3 + [(), (), ()]  # parameters, exp_avg, exp_avg_sq, step counts


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for k in range(iters):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def copy_paths(S, dev, rounds, iters):
    g = torch.Generator().manual_seed(S)
    gt = torch.empty(3, S, S, device=dev)
    gt_rows = [torch.rand(3, S, S, generator=g).to(dev) for _ in range(V)]
    small = [torch.randn(s, generator=g).to(dev) for s in SMALL]
    small_rows = [[torch.randn(s, generator=g).to(dev) for s in SMALL] for _ in range(V)]
    sched = ViewSchedule(list(range(V)), V, dev)
    bank = ViewBank(sched)
    bank.add_input("gt", gt, gt_rows)
    for i, t in enumerate(small):
        bank.add_state(f"s{i}", t, [small_rows[v][i] for v in range(V)])

    def with_bank(k):
        bank.load()
        bank.store()
        sched.advance()

    def with_copies(k):
        v = k % V
        gt.copy_(gt_rows[v])
        for t, r in zip(small, small_rows[v]):
            t.copy_(r)
        for t, r in zip(small, small_rows[v]):
            r.copy_(t)

    def single(k):
        gt.copy_(gt_rows[k % V])

    def load_only(k):
        bank.load()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        with_bank(0)

    def graphed(k):
        graph.replay()

    def record(body):
        g_ = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_, stream=side):
            for j in range(IN_GRAPH):
                body(j)
        return lambda k: g_.replay()

    def load_advance(j):
        bank.load()
        sched.advance()

    # the bank moves what the copies move: faster and different is not faster
    sched.seek(3)
    bank.load()
    torch.cuda.synchronize()
    assert torch.equal(gt, gt_rows[3]) and all(torch.equal(t, r) for t, r in zip(small, small_rows[3])) and int(sched.current) == 3
    sched.seek(0)
    paths = {"bank": with_bank, "copy_": with_copies, "single": single, "load": load_only, "graph": graphed,
             "graph_16_load_advance": record(load_advance), "graph_16_advance": record(lambda j: sched.advance()),
             "graph_16_single": record(single)}
    turns = {k: [] for k in paths}
    for r in range(rounds + 2):  # two warm-up turns
        for name, fn in paths.items():
            ms = timed(fn, iters)
            if r >= 2:
                turns[name].append(ms)
    out = {k: summary(v) for k, v in turns.items()}
    gt_bytes = gt.numel() * 4
    small_bytes = sum(t.numel() * 4 for t in small)
    out["bytes"] = {"ground_truth": gt_bytes, "small_slots_each_way": small_bytes, "launches": {"bank": 3, "copy_": 25, "single": 1}}
    out["spread_ms"] = max(out[k]["max_ms"] - out[k]["min_ms"] for k in paths)
    out["copy_over_bank"] = out["copy_"]["median_ms"] / out["bank"]["median_ms"]
    out["bank_over_single"] = out["bank"]["median_ms"] / out["single"]["median_ms"]
    out["load_over_single"] = out["load"]["median_ms"] / out["single"]["median_ms"]
    out["copy_over_graph"] = out["copy_"]["median_ms"] / out["graph"]["median_ms"]
    load_dev = (out["graph_16_load_advance"]["median_ms"] - out["graph_16_advance"]["median_ms"]) / IN_GRAPH
    single_dev = out["graph_16_single"]["median_ms"] / IN_GRAPH
    out["device"] = {"load_ms": load_dev, "single_copy_ms": single_dev, "load_over_single": load_dev / single_dev,
                     "load_ground_truth_GBps": 2.0 * gt.numel() * 4 / (load_dev * 1e-3) / 1e9,
                     "single_copy_GBps": 2.0 * gt.numel() * 4 / (single_dev * 1e-3) / 1e9}
    # bytes the load reads and writes for the large slot, over the whole bank iteration: a floor on the copy's own rate
    out["ground_truth_GBps_over_bank_iteration"] = 2.0 * gt_bytes / (out["bank"]["median_ms"] * 1e-3) / 1e9
    out["ground_truth_GBps_load_alone"] = 2.0 * gt_bytes / (out["load"]["median_ms"] * 1e-3) / 1e9
    out["ground_truth_GBps_single_copy"] = 2.0 * gt_bytes / (out["single"]["median_ms"] * 1e-3) / 1e9
    return out


def example_runs(gaussians, size, iters, rounds):
    import train_synthetic

    base = ["--gaussians", str(gaussians), "--size", str(size), "--iters", str(iters), "--quiet", "--graph", "--optimizer-in-graph"]
    turns, recordings = {"views_1": [], "views_8": []}, {}
    for r in range(rounds + 1):  # one warm-up turn
        for name, extra in (("views_1", ["--views", "1"]), ("views_8", ["--views", "8"])):
            train_synthetic.main(base + extra)
            recordings[name] = train_synthetic.main.last_recordings
            if r >= 1:
                turns[name].append(train_synthetic.main.last_ms_per_iter)
            print(name, f"{train_synthetic.main.last_ms_per_iter:.3f} ms/iter", flush=True)
    out = {k: summary(v) for k, v in turns.items()}
    out["recordings_of_the_last_run"] = recordings
    out["spread_ms"] = max(v["max_ms"] - v["min_ms"] for v in (out["views_1"], out["views_8"]))
    out["views_8_over_views_1"] = out["views_8"]["median_ms"] / out["views_1"]["median_ms"]
    out["what"] = (f"{gaussians} Gaussians, {size}^2, --graph --optimizer-in-graph, {iters} iterations per run, ms per iteration over "
                   f"the last {max(1, iters // 2)} (host clock around a device synchronise), {rounds} alternating runs each")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--example-iters", type=int, default=60)
    ap.add_argument("--example-rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    out = {"what": f"{V} views; the paths alternate, {a.rounds} turns each of {a.iters} iterations between device events, every iteration "
                   "on the next view; ms per iteration", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0)}
    for S in (1024, 2048):
        out[f"copy_3x{S}x{S}"] = copy_paths(S, dev, a.rounds, a.iters)
        print(f"copy_3x{S}x{S}", json.dumps(out[f"copy_3x{S}x{S}"]), flush=True)
        torch.cuda.empty_cache()
    out["example"] = example_runs(a.gaussians, a.size, a.example_iters, a.example_rounds)
    print("example", json.dumps(out["example"]), flush=True)
    out["not_measured"] = ("the kernels' own times (a profiler run); other view counts and sizes; views of several sizes (one bank per "
                           "size); the bank under data parallelism; an eager multi-view loop against the recorded one")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
