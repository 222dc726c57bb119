"""GPU (MI355X, one card): rehearsal of the N-rank data-parallel bench path. RCCL refuses two ranks on one device, so the
ranks share cuda:0 and exchange over gloo (`--backend gloo --share-gpu`): not a measurement, but everything else is the
code the driver's `--gpus N` run executes — bench.py starting its own ranks, the overlapped gradient exchange driven by
the rasterizer's backward (eogs_rast_backward_range), the warmup measurement of the number of ranges, the JSON line."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_rank_bench_rehearsal():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu",
                        "--steps", "4", "--warmup", "1", "--gaussians", "30000", "--size", "160", "--full"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["config"]["parallelism"] == "view-dp2"
    ex = line["exchange"]
    assert ex["rccl_ranks"] == 2 and ex["bytes_per_gaussian"] == 56 and ex["chunks"] in (1, 4)
    # (reduce-scatter + all-gather is an RCCL candidate only: over gloo the all-reduce with 1 and 4 ranges is measured)
    assert set(ex["candidates_tried_ms_per_step"]) == {"all_reduce/1", "all_reduce/4"} and ex["algo"] == "all_reduce"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # the iteration that scales: three renders, ONE synchronous exchange of the raw-parameter gradients, the optimizer step
    ti = line["train_iter_fused"]
    assert ti["n_gpus"] == 2 and ti["renders_per_iter"] == 3 and ti["exchange"]["bytes_per_gaussian"] == 56
    # (no ordering between the two clocks is asserted: at this size an iteration is a few hundred microseconds of kernels, and a
    # stall of the box's host in either window decides which number is larger)
    assert ti["ms_per_iter"] > 0 and ti["compute_only_ms"] > 0 and ti["exchange_alone_ms"] > 0


def test_four_rank_bench_rehearsal():
    """The same with four ranks on the one card (gloo; four ranks and this process: five of the six processes the box allows
    on its GPU): bench.py's own launcher, the per-rank view seeds, the exchange among more than two partners, the line's
    whole-job value."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--backend", "gloo", "--share-gpu",
                        "--steps", "3", "--warmup", "1", "--gaussians", "20000", "--size", "128", "--no-train-iter"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 4 and line["scaling"] == "weak" and line["config"]["parallelism"] == "view-dp4"
    assert line["exchange"]["rccl_ranks"] == 4 and line["exchange"]["bytes_per_gaussian"] == 56
    # whole-job throughput: the four ranks' views over the slowest rank's clock
    assert abs(line["value"] - 4 * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]


def test_two_rank_bench_under_torchrun():
    """The driver's own launch style for N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1 --master-port P bench.py --gpus N ...` — bench.py is then a rank (RANK / LOCAL_RANK / WORLD_SIZE from the
    launcher) and must not start ranks of its own; rank 0 prints the one JSON line."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    port = 29600 + os.getpid() % 300
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--backend", "gloo", "--share-gpu", "--steps", "4", "--warmup", "1",
                        "--gaussians", "30000", "--size", "160"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # one line, from rank 0
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["exchange"]["rccl_ranks"] == 2 and line["config"]["parallelism"] == "view-dp2"


def test_one_gpu_bench_line_and_its_graph_extras():
    """The driver's own command at a small size with --full: ONE JSON line with the contract's keys, `roofline` and `host`,
    and — from the child process bench.py starts after its own measurements — the graph-replay figures beside the eager ones."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--gaussians", "30000", "--size", "160", "--no-cpu-baseline", "--full"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["steps"] == 5 and line["dtype"] == "f32" and line["vs_baseline"] is None
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] < 1
    # HBM traffic of the dominant kernel observed in THIS run (two rocprofv3 --pmc children, bench.live_traffic)
    assert str(line["roofline"]["traffic_source"]).startswith("live"), line["roofline"]
    assert line["roofline"]["traffic"] > 0
    te = line["train_example"]
    assert te["eager"]["ms_per_iter"] > 0 and te["graphed"]["ms_per_iter"] > 0, te
    host = line["host"]
    assert host["kernel_sum_ms"] > 0 and host["count_readback"]["hit"] == 0  # the eager headline waits for its counts
    gs = line["graphed_step"]
    assert "error" not in gs, gs
    assert gs["ms_per_step"] > 0 and gs["recaptures"] == 0
    tg = line["train_iter_fused_graphed"]
    assert tg["graph"]["forwards_per_replay"] == 3 and tg["ms_per_iter"] > 0
    # at this size the eager step is host-bound: the replayed graph must not be slower than it
    # (measured 0.15 against 0.3 ms; the bound is loose because both numbers are clocks of a few milliseconds on a shared host)
    assert gs["ms_per_step"] <= 1.5 * line["ms_per_step"], (gs["ms_per_step"], line["ms_per_step"])


def test_two_rank_training_iteration_with_the_compute_as_a_graph():
    """Opt-in (`--graph-train-iter`): on every rank the three renders, the loss and their backward passes are one replayed
    HIP graph whose gradients accumulate inside the GradBucket buffer (GradBucket.zero_()); the exchange and FusedAdam stay
    outside. Rehearsal over gloo with both ranks on one GPU: the line carries both iterations."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu",
                        "--steps", "4", "--warmup", "1", "--gaussians", "30000", "--size", "160", "--graph-train-iter", "--full"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    eager, graphed = line["train_iter_fused"], line["train_iter_fused_graphed"]
    assert graphed["n_gpus"] == 2 and graphed["graph"]["forwards_per_replay"] == 3 and graphed["graph"]["recaptures"] == 0
    assert graphed["exchange"]["bytes_per_gaussian"] == 56 and graphed["ms_per_iter"] > 0 and eager["ms_per_iter"] > 0
