#!/usr/bin/env python3
"""bench.py — rasterizer fwd+bwd throughput at BASELINE.json's headline configuration.

A "step" = one forward + backward pass of the drop-in rasterizer for ONE training view (the unit the
reference's training loop repeats, GS/train_pan.py:278,469) over synthetic inputs already resident in
HBM: 1,048,576 Gaussians rendered to 1024x1024, 5 channels. With N>1 GPUs each rank renders its own
view of the same Gaussians (view-sharded data parallelism) and a step additionally
all-reduces the 56 B/Gaussian parameter-gradient buffer over RCCL. value = views/s over the whole job.

A plain run sets up, warms up, times exactly --steps steps and prints the line: value, ms_per_step, config, pipeline
(algorithmic bytes over the step time), host (per-step host intervals of the timed region) and, with N ranks, exchange.
--dump-outputs DIR writes what the last timed step returned to its caller (see dump_outputs).

Extra objects in the JSON line, measured only with --full:
  roofline      — dominant kernel (render_bwd): algorithmic bytes (52 B/pair + 32 B/pixel)
                  / its mean HIP-event duration on the launch stream, vs the 8 TB/s HBM peak; `traffic` = its HBM bytes per
                  launch counted IN THIS RUN by two `rocprofv3 --pmc` child runs (live_traffic; --no-live-traffic skips them,
                  the committed profile of the same kernel sources is the fallback)
  host          — kernel sum against step time (the per-step host intervals of the timed region are in every run)
  regimes       — the same step at trained opacities, opacity 0.1, 2048^2 and 2 M Gaussians (median of three 20-step windows)
  train_iter*   — the synthetic 3-render training iteration (torch ops / fused / graphs / parallel branches / altitude-only sun)
  train_example — examples/train_synthetic.py at this size: the reference's whole iteration with its shipped configuration
  pipeline      — the whole fwd+bwd: (432 P + 268 R + 64 HW) bytes / step time, same peak
  kernels_ms    — mean device ms per kernel group (HIP events inside the library)
  cpu_baseline  — the pure-PyTorch dense alpha-blend (oracle/torch_dense.py, fwd+bwd through autograd) on a
                  bounded 1/64-area crop of the same workload, all host cores; rank 0, N=1 only; `scalar_c`: the
                  single-threaded C restatement (oracle/rast_oracle.c) on the same crop
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
# what a plain streaming kernel reaches on the driver's box class (tools/hbm_stream.hip, profiles/r03_hbm_stream.txt): reported
# beside the peak, never used as the denominator of `frac`
HBM_ACHIEVABLE_GBS = {"read": 6500.0, "copy": 5700.0, "write": 4800.0, "source": "profiles/r03_hbm_stream.txt (tools/hbm_stream.hip)"}


def median_window_ms(run, iters, windows=3):
    """ms per call of `run`: `windows` timed windows of `iters` calls each, bracketed by synchronize, the MEDIAN window reported
    — the extra sections below time a few milliseconds of host-driven work each, and one stall of the box's host thread
    (profiles/r04_experiments/ab_session2_summary.txt: 4 ms once per ~500 steps on some boxes) would otherwise be a section's
    whole number (the same section read 0.36, 0.52 and 0.93 ms on three boxes before this)."""
    ws = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        torch.cuda.synchronize()
        ws.append((time.perf_counter() - t0) / iters * 1e3)
    return sorted(ws)[len(ws) // 2]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--gaussians", type=int, default=1 << 20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--opacity", default="init", help="init (0.01, gs_config/train.yaml:55) | trained | float | surface (the trained-scene shape, synthetic.py)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: per-kernel groups and rooflines, the training "
                         "iterations, graph replays, regimes, the other workloads' comparisons and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (image, radii, gradients) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-train-iter", action="store_true", help="skip the extra synthetic training-iteration measurement")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed (RCCL) and run the gradient all-reduce even with one rank (self-test)")
    ap.add_argument("--ar-chunks", type=int, default=0,
                    help="Gaussian ranges of the overlapped gradient exchange (eogs_rast_backward_range); 0 = pick the "
                         "faster of 1 and 4 during warmup")
    ap.add_argument("--ar-algo", default="auto", choices=("auto", "all_reduce", "rs_ag"),
                    help="gradient exchange: one all-reduce, or reduce-scatter + all-gather of the same buffer; auto = "
                         "measure both (with --ar-chunks candidates) during warmup and time the fastest")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"),
                    help="collective backend; gloo + --share-gpu rehearses the N-rank path on a one-GPU box (not a measurement)")
    ap.add_argument("--share-gpu", action="store_true", help="rehearsal only: every rank uses cuda:0")
    ap.add_argument("--graph-extras", action="store_true", help="child mode: the graph-replay measurements only")
    ap.add_argument("--traffic-child", action="store_true",
                    help="child mode (run under rocprofv3 --pmc by live_traffic()): a few steps of the headline workload, nothing else")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="skip the two rocprofv3 --pmc child runs that observe the dominant kernel's HBM traffic in this run "
                         "(roofline.traffic then comes from the committed profile of the same kernel sources, or is null)")
    ap.add_argument("--graph-train-iter", action="store_true",
                    help="N ranks: also report the training iteration with its compute recorded into a HIP graph (opt-in)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher self-test: ranks rendezvous over gloo, all-reduce one number and exit before any GPU call")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


def graph_extras(a):
    """Child mode (--graph-extras): fwd+bwd of the bench step, and the fused training iteration, as replayed HIP graphs."""
    from eogs2_amd import GaussianRasterizer
    from eogs2_amd.graph import GraphedStep
    from eogs2_amd.synthetic import make_scene, settings_for

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    P, H, W = a.gaussians, a.size, a.size
    op = a.opacity if a.opacity in ("init", "trained", "surface") else float(a.opacity)
    sc = make_scene(P, H, W, seed=0, opacity=op, device=dev)
    rast = GaussianRasterizer(settings_for(sc, H, W))
    names = ("means3D", "colors", "opacities", "scales", "rotations")
    params = {k: sc[k].clone().requires_grad_(True) for k in names}
    means2D = torch.zeros(P, 3, device=dev, requires_grad=True)

    def step():
        means2D.grad = None
        for p in params.values():
            p.grad = None
        color, _, _ = rast(params["means3D"], means2D, params["opacities"], colors_precomp=params["colors"],
                           scales=params["scales"], rotations=params["rotations"])
        torch.autograd.backward([color], [sc["dL_dcolor"]])
        return color.detach()  # (a result that kept the autograd graph alive would tie the next backward to this stream)

    t_ramp = time.perf_counter()
    while time.perf_counter() - t_ramp < 1.5:
        step()
    gs = GraphedStep(step, warmup=2)
    for _ in range(max(a.warmup, 10)):
        gs()
    g_ms = median_window_ms(gs, a.steps)  # (three windows of a.steps replays, the median: an extra beside the headline)
    out = {"graphed_step": {"ms_per_step": g_ms, "views_per_s": 1e3 / g_ms, "recaptures": gs.recaptures,
                            "what": "GraphedStep: fwd+bwd of the bench step as one hipGraph replay, list capacity checked "
                                    "per replay while it runs"}}
    del gs
    if not a.no_train_iter:
        out["train_iter_fused_graphed"] = train_iteration(sc, P, H, W, dev, fused=True, graphed=True, iters=20)
        try:  # the same graph with its three renders as parallel branches (eogs2_amd.graph.Branches)
            out["train_iter_fused_graphed_parallel"] = train_iteration(sc, P, H, W, dev, fused=True, graphed=True, parallel=True, iters=20)
            out["train_iter_fused_graphed_parallel_sun_altitude_only"] = train_iteration(
                sc, P, H, W, dev, fused=True, graphed=True, parallel=True, iters=20, sun_altitude_only=True)
        except Exception as e:  # noqa: BLE001 (an extra must never cost the line)
            out["train_iter_fused_graphed_parallel"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    print(json.dumps(out), flush=True)


def graph_extras_from_child(a, kernel_sum_ms):
    import subprocess

    cmd = [sys.executable, os.path.abspath(__file__), "--graph-extras", "--gaussians", str(a.gaussians), "--size", str(a.size),
           "--opacity", str(a.opacity), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        rows = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not rows:
            return {"graphed_step": {"error": f"child exited {r.returncode}: {r.stderr[-300:]}"}}
        out = json.loads(rows[-1])
        if kernel_sum_ms and "ms_per_step" in out.get("graphed_step", {}):
            out["graphed_step"]["step_over_kernel_sum"] = out["graphed_step"]["ms_per_step"] / kernel_sum_ms
        return out
    except Exception as e:  # noqa: BLE001 (an extra must never cost the bench line)
        return {"graphed_step": {"error": repr(e)[:300]}}


def _free_port():
    import socket

    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(a, argv):
    """`python3 bench.py --gpus N` without a launcher: this process starts the N ranks itself (one process per GPU,
    LOCAL_RANK = GPU index) BEFORE anything touches the GPU here, forwards rank 0's JSON line, and exits with the worst
    return code. The parent never initialises HIP: a process that did must not start other programs on this pool."""
    import subprocess

    port = _free_port()
    threads = max(1, (os.cpu_count() or 8) // a.gpus)
    procs = []
    try:
        for r in range(a.gpus):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0",
                       EOGS_BENCH_CHILD="1")
            env.setdefault("OMP_NUM_THREADS", str(threads))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env,
                                          stdout=subprocess.PIPE if r == 0 else sys.stderr, text=True))
        # rank 0's stdout is drained by a thread; the ranks are polled, and if one of them dies the others (which would wait
        # for it inside a collective forever) are ended: exactly the PIDs started above, nothing by pattern
        import threading

        chunks = []
        reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
        reader.start()
        while True:
            rcs = [p.poll() for p in procs]
            if all(rc is not None for rc in rcs):
                break
            if any(rc not in (None, 0) for rc in rcs):
                time.sleep(2.0)  # let the failing rank's traceback reach stderr
                for p in procs:
                    if p.poll() is None:
                        p.kill()
                rcs = [p.wait() for p in procs]
                break
            time.sleep(0.2)
        reader.join(timeout=10)
        out = "".join(chunks)
    except BaseException:
        for p in procs:  # exactly the PIDs started above
            if p.poll() is None:
                p.kill()
        raise
    sys.stdout.write(out)
    sys.stdout.flush()
    bad = [rc for rc in rcs if rc != 0]
    if bad:
        print(f"bench.py: rank return codes {rcs}", file=sys.stderr)
        sys.exit(bad[0] if bad[0] > 0 else 1)


def dry_run(a, rank, world):
    """Stops before any GPU call: proves that the launcher's ranks find each other (gloo over 127.0.0.1)."""
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.ones(1)
    dist.all_reduce(t)
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": a.gpus, "world_size": world, "ranks_seen": int(t.item()),
                          "launcher": "self" if os.environ.get("EOGS_BENCH_CHILD") else "external"}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def measured_traffic(kernel, a):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes (tools/prof.sh: FETCH_SIZE and
    WRITE_SIZE collected in separate --pmc runs of this same command). gfx950 correction per MI355X_MICROARCH.md:
    FETCH_SIZE counts 128-byte requests as 64 bytes -> doubled; both counters are in KiB. None when no profile of
    the default workload is committed (PMC counters cannot be read from inside this process)."""
    import glob

    if a.gaussians != (1 << 20) or a.size != 1024 or a.opacity != "init":
        return None, None
    import re

    def ver(path):  # profiles/r01_v12/...: (round, version), numeric
        m = re.search(r"r(\d+)_v(\d+)", path)
        return (int(m.group(1)), int(m.group(2))) if m else (-1, -1)

    for d in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_v*", "pmc_mean_per_dispatch.json")), key=ver, reverse=True):
        if not _profile_is_current(d):
            continue  # counters of other kernels: never replayed
        try:
            pm = json.load(open(d))
        except Exception:
            continue
        # a launch group of the library (kernels_ms key) -> the kernels it launches once per step
        group = {"depth_sort": ("block_lists_kernel",),
                 "binning": ("pblock_scan_kernel", "expand_entries_kernel", "entry_hist_kernel", "entry_colscan_kernel",
                             "entry_scatter_kernel")}.get(kernel, (kernel + "_kernel", kernel + "_quad_kernel"))
        total, hit = 0.0, False
        for name, c in pm.items():
            if name.startswith(group) and "FETCH_SIZE" in c and "WRITE_SIZE" in c:
                total += (2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024
                hit = True
                if kernel not in ("depth_sort", "binning"):
                    break
        if hit:
            return int(total), os.path.relpath(d, ROOT)
    return None, None


def live_traffic(a, kernels=("render_bwd", "render_fwd", "gaussian_bwd", "preprocess_fwd", "depth_sort", "binning")):
    """HBM bytes per launch OBSERVED IN THIS RUN: two child runs of this script under `rocprofv3 --pmc` (FETCH_SIZE and
    WRITE_SIZE do not fit one pass; counters only, no trace domain beside them), a few steps of the same workload each, the
    mean counter value per dispatch of each kernel. Corrections per MI355X_MICROARCH.md (its HBM / rocprofv3 section): both
    counters are in KiB, FETCH_SIZE counts 128-byte requests as 64 bytes on gfx950 -> doubled. The children are started as
    child processes from /tmp (the profiler writes there), the program itself after `--`. Returns ({kernel group: bytes},
    note); ({}, reason) when the profiler is not there or a pass fails — the caller falls back to the committed profile."""
    import collections
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {}, "rocprofv3 not found"
    means = {}
    t0 = time.perf_counter()
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        out = None
        try:
            out = tempfile.mkdtemp(prefix="eogs_pmc_", dir="/tmp")
            cmd = [exe, "--pmc", counter, "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
                   "--traffic-child", "--gaussians", str(a.gaussians), "--size", str(a.size), "--opacity", str(a.opacity)]
            r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, timeout=90)
            if r.returncode != 0:
                return {}, f"rocprofv3 --pmc {counter}: exit {r.returncode}"
            agg = collections.defaultdict(list)
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row["Counter_Name"] == counter:
                        agg[row["Kernel_Name"]].append(float(row["Counter_Value"]))
            if not agg:
                return {}, f"rocprofv3 --pmc {counter}: no counter rows"
            means[counter] = {k: sum(v) / len(v) for k, v in agg.items()}
        except Exception as e:
            return {}, f"rocprofv3 --pmc {counter}: {type(e).__name__}: {e}"[:160]
        finally:
            if out:
                shutil.rmtree(out, ignore_errors=True)
    res = {}
    groups = {"depth_sort": ("block_lists_kernel",),  # a launch group of the library (kernels_ms key) -> its kernels, once per step each
              "binning": ("pblock_scan_kernel", "expand_entries_kernel", "entry_hist_kernel", "entry_colscan_kernel", "entry_scatter_kernel")}
    for g in kernels:
        names = groups.get(g, (g + "_kernel", g + "_quad_kernel"))
        tot, hit = 0.0, 0
        for nm in names:
            pick = lambda c: [v for k, v in means[c].items() if k.replace("void ", "").startswith(nm)]
            f, w = pick("FETCH_SIZE"), pick("WRITE_SIZE")
            if f and w:  # (one variant of a kernel runs per workload)
                tot += (2.0 * max(f) + max(w)) * 1024
                hit += 1
        if hit and (g in groups or hit == 1):
            res[g] = int(tot)
    return res, f"live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, two child runs of this command's workload ({time.perf_counter() - t0:.0f} s)"


def traffic_child(a):
    """The workload of live_traffic()'s children: 2 + 4 steps of the bench step, no clock ramp (counters, not time)."""
    from eogs2_amd import GaussianRasterizer
    from eogs2_amd.synthetic import make_camera, make_scene, settings_for

    dev = torch.device("cuda", 0)
    P, H, W = a.gaussians, a.size, a.size
    try:
        opacity = float(a.opacity)
    except ValueError:
        opacity = a.opacity
    sc = make_scene(P, H, W, seed=0, opacity=opacity, device=dev)
    sc["viewmatrix"] = make_camera(H, W, seed=0, device=dev)
    rast = GaussianRasterizer(settings_for(sc, H, W))
    params = {k: sc[k].clone().requires_grad_(True) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    for _ in range(6):
        for p in params.values():
            p.grad = None
        m2.grad = None
        c, _, _ = rast(params["means3D"], m2, params["opacities"], colors_precomp=params["colors"], scales=params["scales"],
                       rotations=params["rotations"])
        torch.autograd.backward([c], [sc["dL_dcolor"]])
    torch.cuda.synchronize()
    return 0


def _profile_is_current(pmc_json):
    """A committed PMC profile counts only if it was taken (1) on the kernel sources this process runs (meta.json written by
    tools/prof_summary.py holds their sha256): traffic / instruction counts of older kernels are not printed — and (2) on
    the DEFAULT workload: directories with a workload suffix (r02_v19_trained: other opacities run other kernels,
    r02_v19_lds: other counters) or a non-empty BENCH_ARGS in their meta.json are never replayed."""
    import re

    from eogs2_amd.build import source_hash

    d = os.path.dirname(pmc_json)
    if not re.fullmatch(r"r\d+_v\d+", os.path.basename(d)):
        return False
    try:
        meta = json.load(open(os.path.join(d, "meta.json")))
    except Exception:
        return False
    return meta.get("kernel_source_sha256") == source_hash() and not meta.get("bench_args", "").strip()


def measured_valu(kernel, a, counter=None):
    """VALU wave-instructions per launch of `kernel` from the same committed PMC passes (SQ_INSTS_VALU), for the
    instruction-issue bound the render kernels actually sit at; `counter`: another counter of that kernel
    from the same passes (None when the profile does not hold it)."""
    import glob
    import re

    if a.gaussians != (1 << 20) or a.size != 1024 or a.opacity != "init":
        return None

    def ver(path):
        m = re.search(r"r(\d+)_v(\d+)", path)
        return (int(m.group(1)), int(m.group(2))) if m else (-1, -1)

    for d in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_v*", "pmc_mean_per_dispatch.json")), key=ver, reverse=True):
        if not _profile_is_current(d):
            continue
        try:
            pm = json.load(open(d))
        except Exception:
            continue
        for name, c in pm.items():
            if name.startswith((kernel + "_kernel", kernel + "_quad_kernel")) and "SQ_INSTS_VALU" in c:
                if counter is not None:
                    return float(c[counter]) if counter in c else None
                return float(c["SQ_INSTS_VALU"])
    return None


def _torch_photometric(img, gt, win, lam=0.2):
    """The reference's op sequence for (1-l) L1 + l (1-SSIM) (GS/utils/loss_utils.py:18-19,45-85, image_utils.py:27-28)
    in PyTorch on the GPU: what the loss costs a user of the reference after the drop-in."""
    import torch.nn.functional as F

    C = img.shape[0]
    conv = lambda t: F.conv2d(t[None], win[:C], padding=5, groups=C)[0]
    mu1, mu2 = conv(img), conv(gt)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11, s22, s12 = conv(img * img) - mu1_sq, conv(gt * gt) - mu2_sq, conv(img * gt) - mu12
    m = ((2 * mu12 + 0.01**2) * (2 * s12 + 0.03**2)) / ((mu1_sq + mu2_sq + 0.01**2) * (s11 + s22 + 0.03**2))
    return (1.0 - lam) * torch.abs(img - gt).mean() + lam * (1.0 - m.mean())


def _ssim_window(dev, C=3):
    w1 = torch.tensor([math.exp(-((x - 5) ** 2) / (2 * 1.5**2)) for x in range(11)])
    w1 = (w1 / w1.sum()).unsqueeze(1)
    return w1.mm(w1.t()).float().expand(C, 1, 11, 11).contiguous().to(dev)


def train_iteration(sc, P, H, W, dev, fused, iters=5, dist=None, view_seed=0, algo="all_reduce", graphed=False, parallel=False,
                    sun_altitude_only=False):
    """Extra, reported beside the headline: one synthetic EOGS++ training iteration as the reference schedules it after
    iteration 1000 (GS/train_pan.py:278,305-316,375-391): three renders of the same Gaussians — the view (H x W), the
    sun camera (2H x 2W, affine_cameras.py:366-367) and a random virtual camera (H x W) — each forward + backward,
    the photometric loss (1-l) L1 + l (1-SSIM), l = 0.2, on the view's RGB against a synthetic ground truth, fixed
    upstream gradients for everything else (resampling / shadow / regularisers are out of scope), then
    one Adam step on the five raw parameter tensors (torch.optim.Adam as the reference configures it, or FusedAdam).
    fused=False: the reference's PyTorch ops around the drop-in GaussianRasterizer (activations, feature assembly,
    SSIM as five depthwise conv2d) — what a user of the reference gets after the drop-in alone.
    fused=True: `eogs2_amd.fused.rasterize_raw` (§8 f1) + `eogs2_amd.losses.photometric_loss` (§8 f2).
    dist: the initialised torch.distributed module of an N-rank run. Every rank then renders ITS three views (`view_seed`)
    of the same Gaussians and the iteration ends with ONE synchronous exchange of the 56 B/Gaussian raw-parameter gradients
    (`GradBucket.all_reduce()`: the three backward passes accumulate first, so the exchange cannot start earlier) before the
    optimizer step — the reference's iteration (train_pan.py:278,308,469,664-690) under view-sharded data parallelism.
    Reported: ms per iteration (max over ranks), the same without the exchange, and the exchange alone.
    graphed (one rank, fused): the three renders, the loss and their backward passes are recorded once into a HIP graph
    (eogs2_amd.graph.GraphedStep) and replayed; the optimizer step stays outside (its bias correction is host arithmetic).
    parallel (with graphed): the three renders are independent branches of that graph (eogs2_amd.graph.Branches).
    sun_altitude_only (fused): the 2H x 2W sun-camera render blends its altitude channel alone (EOGS_FLAG_ALT_ONLY) — what the
    reference's shipped configuration consumes of it (train_pan.py:305-324, gs_config/train.yaml:123)."""
    from eogs2_amd import GaussianRasterizer
    from eogs2_amd.fused import rasterize_raw
    from eogs2_amd.losses import photometric_loss
    from eogs2_amd.synthetic import make_camera, settings_for

    C0 = 0.28209479177387814
    op = sc["opacities"].double()
    raw = dict(xyz=sc["means3D"].clone(), f_dc=((sc["colors"][:, :3] - 0.5) / C0).reshape(P, 1, 3).contiguous(),
               opacity=torch.log(op / (1 - op)).float(), scaling=torch.log(sc["scales"]), rotation=sc["rotations"] * 1.5)
    params = {k: v.requires_grad_(True) for k, v in raw.items()}
    if fused:
        from eogs2_amd.optim import FusedAdam

        opt = FusedAdam([{"params": [v], "lr": 1e-4, "name": k} for k, v in params.items()], lr=0.0, eps=1e-15)
    else:  # the reference's optimizer (gaussian_model.py:262)
        opt = torch.optim.Adam([{"params": [v], "lr": 1e-4, "name": k} for k, v in params.items()], lr=0.0, eps=1e-15)
    win = _ssim_window(dev)
    bucket = None
    if dist is not None:
        from eogs2_amd.parallel import GradBucket

        bucket = GradBucket(list(params.values()), algo=algo)
    views = []
    for seed, (h, w) in ((11, (H, W)), (12, (2 * H, 2 * W)), (13, (H, W))):
        vm = make_camera(h, w, seed=seed + 100 * view_seed, device=dev)
        g = torch.Generator().manual_seed(seed)
        dL = (torch.randn(5, h, w, generator=g) / (h * w)).to(dev)
        views.append((settings_for(dict(sc, viewmatrix=vm), h, w), vm[:, 2].contiguous(), torch.zeros(P, 3, device=dev), dL))
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)

    branches = None
    if parallel:
        from eogs2_amd.graph import Branches

        branches = Branches(len(views), device=dev)

    def it(exchange=True, step=True):
        if graphed and bucket is not None:
            bucket.zero_()  # the gradients live in the exchange buffer: the same tensors in every replay
        else:
            opt.zero_grad(set_to_none=True)
        if branches is not None:
            # the largest render (the 2H x 2W sun camera) is queued first: its long kernels start at once and the two small
            # renders fill in beside them, instead of the sun camera finishing alone (2.73-2.76 -> 2.58-2.63 ms with the
            # altitude-only sun render; tools/branch_order_probe.py). The shared parameters' gradients are summed after the join,
            # in the order queued (eogs2_amd.graph.Branches).
            order = [int(x) for x in os.environ["EOGS_BRANCH_ORDER"].split(",")] if "EOGS_BRANCH_ORDER" in os.environ else \
                sorted(range(len(views)), key=lambda vi: -(views[vi][3].shape[-1] * views[vi][3].shape[-2]))
            branches.run([lambda vi=vi: one_view(vi) for vi in order], shared=list(params.values()))
        else:
            for vi in range(len(views)):
                one_view(vi)
        if bucket is not None and exchange:
            bucket.all_reduce()
        if step:
            opt.step()

    def one_view(vi):
        rs, alt, m2, dL = views[vi]
        if fused and sun_altitude_only and vi == 1:
            color, _, _ = rasterize_raw(params["xyz"], m2, params["f_dc"], params["opacity"], params["scaling"],
                                        params["rotation"], alt, rs, altitude_only=True)
            torch.autograd.backward([color], [dL[3:4]])
            return
        if fused:
            color, _, _ = rasterize_raw(params["xyz"], m2, params["f_dc"], params["opacity"], params["scaling"],
                                        params["rotation"], alt, rs)
        else:
            rgb = (params["f_dc"] * C0 + 0.5).squeeze(1)
            altitude = (params["xyz"] @ rs.viewmatrix[:3, :3] + rs.viewmatrix[3, :3])[..., 2].unsqueeze(-1)
            colors = torch.cat([rgb, altitude, torch.ones_like(altitude)], dim=-1)
            color, _, _ = GaussianRasterizer(rs)(
                params["xyz"], m2, torch.sigmoid(params["opacity"]), colors_precomp=colors,
                scales=torch.exp(params["scaling"]), rotations=torch.nn.functional.normalize(params["rotation"]))
        if vi == 0:
            loss = photometric_loss(color[:3], gt, 0.2)[0] if fused else _torch_photometric(color[:3], gt, win)
            (loss + (color[3:] * dL[3:]).sum()).backward()
        else:
            torch.autograd.backward([color], [dL])

    graph_info = {}
    if graphed:
        from eogs2_amd.graph import GraphedStep

        assert fused
        eager_it = it
        gs = GraphedStep(lambda: eager_it(exchange=False, step=False), warmup=2)

        def it(exchange=True):  # noqa: F811
            gs()
            if bucket is not None and exchange:
                bucket.all_reduce()  # (outside the graph; finds the gradients already in its buffer)
            opt.step()

    def timed(fn, n):
        fn()
        if dist is None:  # one rank: the median of three windows (a stall of the host thread is not the iteration's time)
            return median_window_ms(fn, n) * 1e-3
        # N ranks: three windows, each bracketed by a barrier + synchronize on both sides and clocked by the slowest rank
        # (MAX over ranks); the median window is reported — every rank sees the same three numbers, so the same median
        ws = []
        for _ in range(3):
            dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            dist.barrier()
            torch.cuda.synchronize()
            tt = torch.tensor([(time.perf_counter() - t0) / n], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            ws.append(float(tt.item()))
        return sorted(ws)[1]

    dt = timed(it, iters)
    extra = {}
    if bucket is not None:
        world = dist.get_world_size()
        extra = {"n_gpus": world, "iters_per_s_all_ranks": world / dt, "views_per_s_all_ranks": 3 * world / dt,
                 "compute_only_ms": timed(lambda: it(exchange=False), iters) * 1e3,
                 "exchange_alone_ms": timed(lambda: bucket._exchange_whole(async_op=False), 10) * 1e3,
                 "exchange": {"algo": bucket.algo, "bytes": int(bucket.flat.numel() * 4),
                              "bytes_per_gaussian": bucket.bytes_per_gaussian,
                              "how": "GradBucket.all_reduce() after the iteration's three backward passes, before the optimizer step"}}
        bucket.close()
    if graphed:
        graph_info = {"graph": {"replays": gs.replays, "recaptures": gs.recaptures, "forwards_per_replay": len(gs.forwards)}}
    return {"iters_per_s": 1.0 / dt, "ms_per_iter": dt * 1e3, "renders_per_iter": 3, **extra, **graph_info,
            "what": f"3 renders ({H}x{W}, {2 * H}x{2 * W} sun camera, {H}x{W}) fwd+bwd + L1/DSSIM loss on the view + Adam "
                    f"on raw parameters; activations, loss and optimizer " + ("inside HIP kernels (EOGS_FLAG_RAW_PARAMS, "
                    "eogs_loss_*, eogs_adam_step)" if fused else "as the reference's PyTorch ops")}


def photometric_loss_bench(abi, dev, H, W, iters=20):
    """Extra: `(1-l) L1 + l (1-SSIM)` forward + backward on a 3 x H x W render, l = 0.2
    (GS/utils/image_utils.py:27-28, arguments/__init__.py:257). `fused` = eogs2_amd.losses.photometric_loss (one HIP
    kernel each way); `torch_ops` = the reference's op sequence (5 depthwise 11x11 conv2d + elementwise,
    GS/utils/loss_utils.py:18-19,45-85) in PyTorch on the same GPU, i.e. what the reference's loss costs after the drop-in."""
    from eogs2_amd.losses import photometric_loss

    g = torch.Generator().manual_seed(3)
    gt = torch.rand(3, H, W, generator=g).to(dev)
    img = (gt + 0.05 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)
    win = _ssim_window(dev)

    def torch_ops():
        return _torch_photometric(img, gt, win)

    def timed(fn):
        def run():
            img.grad = None
            fn().backward()

        for _ in range(3):
            run()
        return median_window_ms(run, iters)

    t_ref = timed(torch_ops)
    v_ref = float(torch_ops())
    abi.profile_reset()
    abi.profile_enable(1)
    t_fused = timed(lambda: photometric_loss(img, gt, 0.2)[0])
    abi.profile_enable(0)
    kern = {k: ms / n for k, (ms, n) in abi.profile().items() if n and k.startswith("loss_")}
    v_fused = float(photometric_loss(img, gt, 0.2)[0])
    alg = {"loss_fwd": 20 * 3 * H * W, "loss_bwd": 24 * 3 * H * W}  # B: fwd reads 2 images, writes 3 maps; bwd reads 5, writes 1
    return {"workload": f"3x{H}x{W}, lambda_dssim=0.2, fwd+bwd", "fused_ms": t_fused, "torch_ops_ms": t_ref,
            "value_fused": v_fused, "value_torch_ops": v_ref, "kernels_ms": kern,
            "roofline": {k: {"algorithmic_bytes": alg[k], "achieved_GBps": alg[k] / (kern[k] * 1e-3) / 1e9,
                             "frac": alg[k] / (kern[k] * 1e-3) / 1e9 / HBM_PEAK_GBS} for k in kern}}


def resample_bench(abi, dev, H, W, iters=20):
    """Extra: the virtual-camera resample of GS/gaussian_renderer/renderer_cc_shadow.py:32-50 (einsum,
    grid_sample, out-of-view fill) forward + backward for the sun camera (2H x 2W render sampled on the H x W grid) and a
    random virtual camera (H x W): the reference's PyTorch ops on the same GPU vs eogs2_amd.resample.resample."""
    from eogs2_amd.resample import resample

    def ref_ops(vr, M, uva):
        uv = torch.einsum("...ij,...j->...i", M, uva)[..., :2]
        s = torch.nn.functional.grid_sample(vr.unsqueeze(0), uv.unsqueeze(0), align_corners=True).squeeze(0)
        rgb, a = s[:3], s[3]
        a[(uv.abs() > 1).any(-1)] = -100
        return torch.cat([rgb, a[None]], 0), uv

    out = {}
    U, V = torch.meshgrid(torch.linspace(-1, 1, W, device=dev), torch.linspace(-1, 1, H, device=dev), indexing="xy")
    M = torch.eye(3, device=dev)
    M[:2, 2] = torch.tensor([0.01, -0.02], device=dev)
    for name, f in (("sun_2x", 2), ("random_1x", 1)):
        vr = torch.rand(5, H * f, W * f, device=dev, requires_grad=True)
        alt = torch.rand(H, W, device=dev, requires_grad=True)
        w = torch.randn(4, H, W, device=dev)
        for tag, fn in (("torch_ops_ms", ref_ops), ("fused_ms", resample)):
            def run():
                vr.grad = alt.grad = None
                s, uv = fn(vr, M, torch.stack((U, V, alt), dim=-1))
                ((s * w).sum() + uv.sum()).backward()
            for _ in range(3):
                run()
            out[f"{name}_{tag}"] = median_window_ms(run, iters)
            if tag == "fused_ms":
                abi.profile_reset()
                abi.profile_enable(1)
                for _ in range(5):
                    run()
                abi.profile_enable(0)
                out[f"{name}_kernels_ms"] = {k: ms / n for k, (ms, n) in abi.profile().items()
                                             if n and k.startswith("resample_")}
    out["what"] = f"true camera {H}x{W}; timings include the small PyTorch ops around the call (stack, weighted sum)"
    return out


def shade_bench(abi, dev, H, W, iters=20):
    """Extra: the per-pixel chain after the raw render — AffineCamera.render_pipeline
    (scene/cameras/affine_cameras.py:303-348), Suncamera_L (loss/shadow.py:37-51) and Translucentshadows_L (:13-17) —
    forward + backward on one H x W view: the reference's PyTorch ops on the same GPU vs eogs2_amd.shade."""
    import types

    from eogs2_amd import shade as S

    torch.manual_seed(5)
    raw = torch.rand(3, H, W, device=dev, requires_grad=True)
    sample = torch.rand(3, H, W, device=dev)
    alt = (torch.randn(H, W, device=dev) * 0.5).requires_grad_(True)
    uv = (torch.rand(H, W, 2, device=dev) * 2.2 - 1.1)
    gt = torch.rand(3, H, W, device=dev)
    cam = types.SimpleNamespace(use_cc=True, use_exposure=False, use_shadow=True)
    cam.color_correction = torch.nn.Conv2d(3, 3, 1, bias=True).to(dev)
    cam.inshadow_color_correction = torch.nn.Parameter(torch.full((3, 1, 1), 0.05, device=dev))

    def ref_ops():
        cc = cam.color_correction(raw.unsqueeze(0))
        shadow = torch.exp(0.4 * alt.clip(max=0.0))
        shaded = (shadow * cc + (1 - shadow) * cam.inshadow_color_correction * cc).squeeze(0)
        diff = raw - sample
        vis = ((alt > -1e-2) * (uv.abs() < 1).all(-1)).detach()
        l_alt = (alt.abs() * vis).sum() / vis.sum()
        l_rgb = (diff.abs() * vis).sum() / vis.sum()
        b = shadow.clip(0.05, 0.95)
        l_ts = -(shadow * torch.log2(b) + (1 - shadow) * torch.log2(1 - b)).mean()
        return (shaded - gt).abs().mean() + l_alt + l_rgb + 0.1 * l_ts

    def fused():
        out = S.render_pipeline(cam, raw, alt)
        l_alt, l_rgb = S.suncamera_l(raw, sample, alt, uv)
        return (out["final"] - gt).abs().mean() + l_alt + l_rgb + 0.1 * S.translucentshadows_l(out["shadowmap"])

    res = {}
    params = [raw, alt, cam.inshadow_color_correction, *cam.color_correction.parameters()]
    for tag, fn in (("torch_ops_ms", ref_ops), ("fused_ms", fused)):
        def run():
            for q in params:
                q.grad = None
            v = fn()
            v.backward()
            return v
        for _ in range(3):
            v = run()
        res[tag] = median_window_ms(run, iters)
        res["value_" + tag[:-3]] = float(v.detach())
        if tag == "fused_ms":
            abi.profile_reset()
            abi.profile_enable(1)
            for _ in range(5):
                run()
            abi.profile_enable(0)
            res["kernels_ms"] = {k: ms / n for k, (ms, n) in abi.profile().items() if n and k.startswith(("shade_", "mloss_"))}
    npx = H * W
    k = res.get("kernels_ms", {})
    # algorithmic bytes per pixel: shade fwd reads 16 (raw, alt_diff) writes 28 (cc, shaded, shadow); bwd reads 16 + 28
    # upstream, writes 16
    if "shade_fwd" in k:
        res["roofline"] = {"shade_fwd": {"algorithmic_bytes": 44 * npx, "achieved_GBps": 44 * npx / (k["shade_fwd"] * 1e-3) / 1e9},
                           "shade_bwd": {"algorithmic_bytes": 60 * npx, "achieved_GBps": 60 * npx / (k["shade_bwd"] * 1e-3) / 1e9}}
    res["what"] = (f"{H}x{W} view: colour correction + shadow map + in-shadow tint, sun-camera masked L1 pair, translucent-shadow "
                   "regulariser, fwd+bwd incl. the L1 on the shaded image (PyTorch in both variants)")
    return res


def tsdf_bench(abi, dev, iters=10):
    """Extra: TSDF integration of one 1024^2 altitude image into a 256 x 256 x 64 volume
    (src/gaussiansplatting/tsdf.py:325-368,459-520): the reference's PyTorch op sequence on the same GPU vs
    eogs2_amd.tsdf.integrate (one kernel)."""
    import torch.nn.functional as F

    from eogs2_amd.tsdf import integrate, volume_axes

    dims, axes = volume_axes([[-1.2, 1.2], [-1.2, 1.2], [-0.3, 0.35]], 2.4 / 255, dev)
    torch.manual_seed(9)
    coef = torch.tensor([[0.0, 0.9, 0.05], [0.9, 0.0, -0.08], [0.0, 0.0, 1.0]], device=dev)
    intercept = torch.tensor([0.02, -0.03, 0.1], device=dev)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 1024, device=dev), torch.linspace(-1, 1, 1024, device=dev), indexing="ij")
    alt = (0.15 * torch.sin(3 * xx) * torch.cos(2 * yy))[None, None]
    wgt = torch.rand((1, 1, 1024, 1024), device=dev).clamp(min=0.05)
    trunc = 4.0 * 2.4 / 255
    world = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    vox = torch.stack(torch.meshgrid(*[torch.arange(d, device=dev) for d in dims], indexing="ij"), dim=-1).reshape(-1, 3)

    def ref_ops(t, w):
        view = F.linear(world / 1.0, coef, intercept)
        sampled = F.grid_sample(torch.cat([alt, wgt], dim=1), view[None, :, None, :2], mode="bilinear", align_corners=True).squeeze()
        a_s, w_s = sampled[0], sampled[1]
        mask = (view[:, :2].abs() <= 1.0).all(dim=1)
        vn = view.clone()
        vn[:, 2] = a_s
        Ainv = torch.linalg.inv(coef)
        d = torch.linalg.norm(F.linear(vn, Ainv, -(Ainv @ intercept)) - world, dim=1) * torch.sign(view[:, 2] - a_s)
        mask &= d >= -trunc
        tv = torch.minimum(torch.ones_like(d), d / trunc)[mask]
        x, y, z = vox[mask, 0], vox[mask, 1], vox[mask, 2]
        w_old, t_old = w[x, y, z], t[x, y, z]
        obs = w_s.reshape(*w.shape)[x, y, z]
        w_new = w_old + obs
        t[x, y, z] = (w_old * t_old + obs * tv) / w_new
        w[x, y, z] = w_new

    def fused(t, w):
        integrate(t, w, axes, coef, intercept, 1.0, trunc, alt, wgt)

    res = {}
    vols = {}
    for tag, fn in (("torch_ops_ms", ref_ops), ("fused_ms", fused)):
        t, w = torch.ones(dims, device=dev), torch.zeros(dims, device=dev)
        fn(t, w)
        vols[tag] = (t.clone(), w.clone())
        res[tag] = median_window_ms(lambda: fn(t, w), iters)
    res["max_abs_diff_tsdf"] = float((vols["torch_ops_ms"][0] - vols["fused_ms"][0]).abs().max())
    abi.profile_reset()
    abi.profile_enable(1)
    t, w = torch.ones(dims, device=dev), torch.zeros(dims, device=dev)
    for _ in range(5):
        fused(t, w)
    abi.profile_enable(0)
    k = {n: ms / c for n, (ms, c) in abi.profile().items() if c and n == "tsdf"}
    nvox = dims[0] * dims[1] * dims[2]
    if "tsdf" in k:  # algorithmic bytes: both volumes read and written once = 16 B/voxel (the image is 8 MB, cache-served)
        res["kernel_ms"] = k["tsdf"]
        res["roofline"] = {"algorithmic_bytes": 16 * nvox, "achieved_GBps": 16 * nvox / (k["tsdf"] * 1e-3) / 1e9,
                           "frac": 16 * nvox / (k["tsdf"] * 1e-3) / 1e9 / HBM_PEAK_GBS}
    res["what"] = f"{dims[0]}x{dims[1]}x{dims[2]} voxels, 1024x1024 altitude + weight image, one integrate() call"
    return res


def optimizer_bench(abi, dev, P, iters=20):
    """Extra: the reference's optimizer step — torch.optim.Adam over six single-tensor groups
    (GS/scene/gaussian_model.py:228-262) — and its prune (`_prune_optimizer` + `prune_points`, :466-505: 21 boolean-mask
    gathers) against eogs2_amd.optim.FusedAdam / prune_optimizer (one launch / one scan + one gather)."""
    from eogs2_amd.optim import FusedAdam, prune_optimizer

    shapes = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (0, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}

    def groups():
        g = torch.Generator().manual_seed(0)
        return [{"params": [torch.nn.Parameter(torch.randn((P,) + s, generator=g).to(dev))], "lr": 1e-3, "name": n}
                for n, s in shapes.items()]

    def timed(fn, n=iters):
        fn()
        return median_window_ms(fn, n)

    out = {}
    for name, ctor in (("torch_adam_ms", lambda l: torch.optim.Adam(l, lr=0.0, eps=1e-15)),
                       ("fused_adam_ms", lambda l: FusedAdam(l, lr=0.0, eps=1e-15))):
        opt = ctor(groups())
        for gr in opt.param_groups:
            gr["params"][0].grad = torch.randn_like(gr["params"][0])
        out[name] = timed(opt.step)
    # prune 10 % of the Gaussians: parameters, both moments, three statistics
    keep = torch.rand(P, generator=torch.Generator().manual_seed(1)).to(dev) < 0.9
    stats = [torch.rand(P, 1, device=dev), torch.rand(P, 1, device=dev), torch.rand(P, device=dev)]

    def ref_prune():
        for gr in opt.param_groups:  # what _prune_optimizer does per group, without replacing anything
            p = gr["params"][0]
            st = opt.state[p]
            _ = (st["exp_avg"][keep], st["exp_avg_sq"][keep], p.data[keep])
        _ = [t[keep] for t in stats]

    def fused_prune():
        from eogs2_amd.optim import compact_rows

        flat = []
        for gr in opt.param_groups:
            p = gr["params"][0]
            flat += [p.data, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]]
        compact_rows(keep, flat + stats)

    out["torch_prune_ms"] = timed(ref_prune, 10)
    out["fused_prune_ms"] = timed(fused_prune, 10)
    out["what"] = f"{P} Gaussians, six parameter groups (59 floats of state per Gaussian incl. moments + 3 statistics); prune keeps 90 %"
    return out


def cpu_baseline(P_full, S_full):
    """The reported CPU baselines (never the thing measured). `value`: the C restatement of the reference's algorithm
    (oracle/rast_oracle.c) on the FULL workload with its per-pixel loops on all host cores (at most 16), fwd+bwd, median of three,
    nothing extrapolated. `scalar_c`: the same on one core, once. `torch_dense`: the dense pure-PyTorch alpha-blend with autograd
    (oracle/torch_dense.py) on bounded crops — 1/16 of the area (scaled x16) and 1/64 (x64) — the line's `value` until round 4
    and what it falls back to when the checker library cannot be loaded."""
    from eogs2_amd.synthetic import make_scene
    from oracle.torch_dense import render_dense

    # many small dense ops: more than ~16 intra-op threads only adds fork/join overhead (256 threads on the
    # GPU box ran 250x slower than 8); `cores` in the JSON is what was actually used
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)

    def dense_crop(frac, budget_s, max_n):
        side = int(round(math.sqrt(frac)))
        P, S = P_full // frac, S_full // side
        # same sigma in pixels as the full workload: s0 ~ P^(-1/3), pixels per unit ~ S
        mult = (S_full / S) * (P / P_full) ** (1.0 / 3.0)
        sc = make_scene(P, S, S, seed=0, opacity="init", scale_mult=mult)

        def once():
            leaves = [sc[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "colors", "scales", "rotations")]
            c, _, _ = render_dense(leaves[0], leaves[1], leaves[2], sc["bg"], sc["viewmatrix"], S, S, scales=leaves[3],
                                   rotations=leaves[4], block=32)
            (c * sc["dL_dcolor"]).sum().backward()

        once()
        ts = []
        t_end = time.perf_counter() + budget_s
        while len(ts) < max_n and (time.perf_counter() < t_end or not ts):
            t0 = time.perf_counter()
            once()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2], len(ts), P, S

    t64, n64, P64, S64 = dense_crop(64, 8.0, 11)
    t16, n16, P16, S16 = dense_crop(16, 12.0, 7)
    # Scaling by area is NOT linear for the dense PyTorch path: the larger crop amortises per-op overhead over bigger
    # tensors (measured on the GPU box: x16 of the 1/16 crop is about half of x64 of the 1/64 crop), so the reported value
    # comes from the larger crop and the smaller one is kept beside it.
    out = {
        "value": 1.0 / (t16 * 16), "unit": "views/s", "cores": torch.get_num_threads(), "kind": "port",
        "sample": f"1/16-area crop of the workload ({P16} Gaussians / {S16}x{S16}, same pixel density and footprint), "
                  f"dense PyTorch fwd+bwd via autograd, median of {n16} = {t16 * 1e3:.0f} ms, scaled x16",
        "smaller_crop": {"sample": f"1/64-area crop ({P64} Gaussians / {S64}x{S64}), median of {n64} = {t64 * 1e3:.0f} ms, scaled x64",
                         "value": 1.0 / (t64 * 64), "x16_over_x64_time_estimate": (t16 * 16) / (t64 * 64)},
    }
    # second reference point: the scalar C restatement of the reference algorithm, one thread, on the FULL
    # workload, driven through the same host wrapper over host pointers (checker library: never on the product path)
    try:
        import oracle
        from eogs2_amd import GaussianRasterizer, _lib
        from eogs2_amd.synthetic import settings_for

        sc = make_scene(P_full, S_full, S_full, seed=0, opacity="init")
        hip = _lib.get
        _lib.get = oracle.abi
        # ONE core: the checker's per-pixel loops are threaded for the tests' sake (oracle/rast_oracle.c eogs_oracle_set_threads)
        old_threads = oracle.abi().cdll.eogs_oracle_set_threads(1)
        try:
            rast = GaussianRasterizer(settings_for(sc, S_full, S_full))
            lv = {k: sc[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "colors", "scales", "rotations")}
            m2 = torch.zeros(P_full, 3, requires_grad=True)
            t0 = time.perf_counter()
            c, _, _ = rast(lv["means3D"], m2, lv["opacities"], colors_precomp=lv["colors"], scales=lv["scales"],
                           rotations=lv["rotations"])
            torch.autograd.backward([c], [sc["dL_dcolor"]])
            tc = time.perf_counter() - t0
            out["scalar_c"] = {"value": 1.0 / tc, "unit": "views/s", "cores": 1,
                               "sample": f"oracle/rast_oracle.c, one fwd+bwd of the full workload ({P_full} Gaussians / "
                                         f"{S_full}x{S_full}) = {tc:.1f} s, not extrapolated"}
            # the same restatement with its per-pixel loops on all cores (OpenMP, at most 16 threads; projection, sort and the
            # per-Gaussian passes stay serial): the strongest CPU number this repository can produce for the full workload
            oracle.abi().cdll.eogs_oracle_set_threads(0)
            tms = []
            for _ in range(3):
                for p in lv.values():
                    p.grad = None
                t0 = time.perf_counter()
                c, _, _ = rast(lv["means3D"], m2, lv["opacities"], colors_precomp=lv["colors"], scales=lv["scales"],
                               rotations=lv["rotations"])
                torch.autograd.backward([c], [sc["dL_dcolor"]])
                tms.append(time.perf_counter() - t0)
            tm = sorted(tms)[1]
            # This is the line's CPU baseline: the restatement of the REFERENCE's algorithm on the FULL workload, nothing
            # extrapolated; the dense PyTorch crops (a different algorithm, scaled by area) stay beside it.
            out = {"value": 1.0 / tm, "unit": "views/s", "cores": min(os.cpu_count() or 1, 16), "kind": "port",
                   "sample": f"oracle/rast_oracle.c (C restatement of the reference's forward.cu / backward.cu), fwd+bwd of the FULL "
                             f"workload ({P_full} Gaussians / {S_full}x{S_full}), per-pixel loops on all cores (OpenMP; projection, "
                             f"sort and per-Gaussian passes serial), median of 3 = {tm:.2f} s, not extrapolated",
                   "scalar_c": out["scalar_c"],
                   "torch_dense": {k: out[k] for k in ("value", "unit", "cores", "sample", "smaller_crop")}}
        finally:
            _lib.get = hip
            oracle.abi().cdll.eogs_oracle_set_threads(old_threads)
    except Exception as e:  # the checker library is optional for the bench line
        out["scalar_c"] = {"error": str(e)[:200]}
    return out


def regime_scan(dev, steps=20):
    """The step in the regimes the headline does not show: same pipeline, same timing rule (steps
    bracketed by synchronize, HBM-resident inputs), the median of three windows of 20 steps each after 5 untimed ones. `frac` is the pipeline's algorithmic
    bytes (432 P + 268 R + 64 HW) over the step time against the 8 TB/s HBM peak, R = the library's own pair count."""
    from eogs2_amd import GaussianRasterizer
    from eogs2_amd.synthetic import make_scene, settings_for

    from eogs2_amd import _lib

    abi = _lib.get()
    out = {}
    # surface_*: the trained-scene SHAPE (eogs2_amd/synthetic.py kind="surface": flat disks on a terrain with buildings, log-normal
    # in-plane sizes with sigma 1, bimodal opacities) at configs[1]'s, the headline's and configs[3]'s sizes; the others keep the
    # reference's initialisation statistics (uniform in the box, near-isotropic) and vary opacity / image size alone
    for name, P, S, op in (("trained_1M_1024", 1 << 20, 1024, "trained"), ("opacity0.1_1M_1024", 1 << 20, 1024, 0.1),
                           ("opacity0.01_1M_2048", 1 << 20, 2048, "init"), ("opacity0.1_2M_1024", 2_000_000, 1024, 0.1),
                           ("surface_300k_800", 300_000, 800, "surface"), ("surface_1M_1024", 1 << 20, 1024, "surface"),
                           ("surface_2M_1024", 2_000_000, 1024, "surface")):
        try:
            sc = make_scene(P, S, S, seed=0, opacity=op, device=dev)
            rast = GaussianRasterizer(settings_for(sc, S, S))
            params = {k: sc[k].clone().requires_grad_(True) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
            m2 = torch.zeros(P, 3, device=dev, requires_grad=True)

            def step():
                for p in params.values():
                    p.grad = None
                m2.grad = None
                c, _, _ = rast(params["means3D"], m2, params["opacities"], colors_precomp=params["colors"],
                               scales=params["scales"], rotations=params["rotations"])
                torch.autograd.backward([c], [sc["dL_dcolor"]])
                return c

            t_ramp = time.perf_counter()  # the scene was built on the host: the GPU's clocks have dropped meanwhile
            while time.perf_counter() - t_ramp < 0.4:
                step()
                torch.cuda.synchronize()
            for _ in range(5):
                step()
            # three windows of `steps` steps, the median reported: one host hiccup (the eager forward blocks on its count
            # readback, so a 10 ms stall of the host is 10 ms of idle GPU) would otherwise be a regime's whole number
            windows = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    c = step()
                torch.cuda.synchronize()
                windows.append((time.perf_counter() - t0) / steps * 1e3)
            ms = sorted(windows)[1]
            nr = int(getattr(c.grad_fn, "num_rendered_exact", getattr(c.grad_fn, "num_rendered", -1)))
            R = nr & 0x7FFFFFFF
            by = 432 * P + 268 * R + 64 * S * S
            # which kernels the library chose for this forward, and the step's kernel groups (a window of its own: every
            # bracket costs two event records, so the timed windows above run without them)
            block_px, fwd_k, bwd_k = abi.path_info(P, nr)
            names = {0: "tile", 1: "block", 2: "quad", 6: "quad_alt"}
            abi.profile_select(0xFFFFFFFF)
            abi.profile_reset()
            abi.profile_enable(1)
            for _ in range(steps):
                c = step()
            torch.cuda.synchronize()
            abi.profile_enable(0)
            # (per STEP, not per bracket: `binning` is two brackets a step — the count scan, then the entry sort)
            kern = {k: t / steps for k, (t, n) in abi.profile().items() if n and k in ("preprocess_fwd", "depth_sort", "binning", "render_fwd", "render_bwd", "gaussian_bwd")}
            out[name] = {"gaussians": P, "size": S, "opacity": op, "steps": steps, "ms_per_step": ms, "views_per_s": 1e3 / ms,
                         "num_rendered": R, "list_entries": (nr >> 32) & 0x07FFFFFF, "list_block_px": block_px, "fwd_kernel": names.get(fwd_k, fwd_k), "bwd_kernel": names.get(bwd_k, bwd_k),
                         "gaussian_bwd_wide": abi.backward_info(P, nr), "kernels_ms": kern, "algorithmic_bytes": by,
                         "frac": by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "windows_ms": windows}
            del sc, rast, params, m2, c
        except Exception as e:  # a regime must never cost the line
            out[name] = {"error": f"{type(e).__name__}: {e}"[:200]}
    return out


def train_example_bench(P, S, iters=24):
    """Extra (SURVEY.md §8 f, BASELINE's "train iters/s"): examples/train_synthetic.py at the headline size — the reference's
    whole iteration with the shipped configuration (train_pan.py:262-400,663-690): view render, sun camera at 2H x 2W consumed
    through its altitude alone, random virtual camera, both resampled onto the view, colour correction + shadow map + tint,
    photometric loss, masked consistency pair, translucent-shadow regulariser, FusedAdam on the Gaussians + Adam on the camera —
    eager and as a replayed HIP graph. ms per iteration over the last half of `iters` iterations (no prune inside)."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic

    out = {"gaussians": P, "size": S, "iters_timed": max(1, iters // 2),
           "what": "3 renders (view, 2x sun altitude-only, random camera) + 2 resamples + render pipeline + losses + FusedAdam + camera Adam"}
    for tag, extra in (("eager", []), ("graphed", ["--graph"]), ("graphed_parallel_renders", ["--graph", "--parallel-renders"])):
        try:
            train_synthetic.main(["--gaussians", str(P), "--size", str(S), "--iters", str(iters), "--quiet", "--no-prune",
                                  "--sun-altitude-only", "--random-camera"] + extra)
            ms = train_synthetic.main.last_ms_per_iter
            out[tag] = {"ms_per_iter": ms, "iters_per_s": 1e3 / ms}
        except Exception as e:  # an extra must never cost the line
            out[tag] = {"error": f"{type(e).__name__}: {e}"[:200]}
    return out


DUMP_ROWS = 1 << 18     # per-Gaussian arrays: at most this many rows (20 floats each over the six arrays)
DUMP_PIXELS = 1 << 20   # images: at most this many pixels per channel (1024 x 1024 whole)


def _dump_sample(n, k, seed):
    """Sorted indices of a fixed, seeded sample of k of range(n) (all of it when n <= k)."""
    if n <= k:
        return None
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].sort().values


def dump_outputs(path, color, radii, invdepth, grads):
    """--dump-outputs: what the caller of the timed step received from its last step, as float32 .npy files: the image
    [5, H, W], the inverse-depth image [1, H, W], radii [P] and the gradients of the six inputs (means2D included). At
    most 44 MiB in all: beyond DUMP_PIXELS pixels the images keep a fixed, seeded sample of pixel positions ([C, DUMP_PIXELS],
    the same positions in every channel), beyond DUMP_ROWS Gaussians the per-Gaussian arrays a fixed, seeded sample of
    rows (the same rows in every array). The inputs are seeded, so two runs with the same arguments can be compared."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    P = radii.shape[0]
    rows = _dump_sample(P, DUMP_ROWS, 1)
    pix = _dump_sample(color.shape[-2] * color.shape[-1], DUMP_PIXELS, 2)
    out = {"color": color, "invdepth": invdepth, "radii": radii}
    out.update({"grad_" + k: g for k, g in grads.items()})
    for name, t in out.items():
        if t is None:
            continue
        t = t.detach().to("cpu", torch.float32)
        if t.dim() == 3 and pix is not None:  # an image
            t = t.reshape(t.shape[0], -1)[:, pix]
        elif t.dim() != 3 and rows is not None:  # per Gaussian
            t = t[rows]
        np.save(os.path.join(path, name + ".npy"), t.numpy())


def main():
    a = parse()
    # read by the HSA runtime when it initialises: must be in the environment before the first torch.cuda call
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if a.gpus > 1 and "RANK" not in os.environ:
        return launch_ranks(a, sys.argv[1:])  # no launcher around us: start the ranks, never touch the GPU here
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29511")
    if a.dry_run:
        return dry_run(a, rank, world)
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP path has no CPU fallback)"
    if a.graph_extras:
        return graph_extras(a)
    if a.traffic_child:
        return traffic_child(a)
    dev = torch.device("cuda", 0 if a.share_gpu else local_rank)
    torch.cuda.set_device(dev)
    dist = None
    use_dist = world > 1 or a.force_dist
    if use_dist:
        import torch.distributed as dist

        if a.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    from eogs2_amd import GaussianRasterizer, _lib
    from eogs2_amd.parallel import GradBucket
    from eogs2_amd.synthetic import make_camera, make_scene, settings_for

    abi = _lib.get()
    P, H, W = a.gaussians, a.size, a.size
    try:
        opacity = float(a.opacity)
    except ValueError:
        opacity = a.opacity
    sc = make_scene(P, H, W, seed=0, opacity=opacity, device=dev)  # same Gaussians on every rank
    vm = make_camera(H, W, seed=rank, device=dev)                  # one view per rank
    sc["viewmatrix"] = vm
    rs = settings_for(sc, H, W)
    params = {k: sc[k].clone().requires_grad_(True) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
    dL = sc["dL_dcolor"]
    names = ("means3D", "colors", "opacities", "scales", "rotations")
    bucket_cols = [slice(0, 3), slice(0, 3), slice(0, 1), slice(0, 3), slice(0, 4)]
    bucket = GradBucket([params[k] for k in names], cols=bucket_cols, names=names, chunks=max(1, a.ar_chunks),
                        algo="all_reduce" if a.ar_algo == "auto" else a.ar_algo)
    rast = GaussianRasterizer(rs)

    def step(exchange=True):
        means2D.grad = None
        if use_dist and exchange:
            # the exchange step: the backward writes the gradients into the bucket and starts the RCCL all-reduce of each
            # Gaussian range as soon as it is computed; finish() waits and leaves the sums in every .grad
            bucket.begin()
        else:
            for p in params.values():
                p.grad = None
        color, radii, invdepth = rast(params["means3D"], means2D, params["opacities"], colors_precomp=params["colors"],
                                      scales=params["scales"], rotations=params["rotations"])
        torch.autograd.backward([color], [dL])  # the loss gradient dL/dcolor is an input of the path
        if use_dist and exchange:
            bucket.finish()
        return color, radii, invdepth

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # Initialisation, before the contract's warmup: a fresh box starts at idle clocks and the first ~1 s of work runs
    # 20-40 % slow (measured: 1.29-1.54 ms/step in the first 25 ms of GPU time against 1.07 afterwards).
    # (The ramp is timed, so ranks run different numbers of steps: no collective inside it.)
    t_ramp = time.perf_counter()
    while time.perf_counter() - t_ramp < 1.5:
        step(exchange=False)
        torch.cuda.synchronize()
    ramp_s = time.perf_counter() - t_ramp
    exchange = None
    if use_dist:
        # who is really there: a SUM all-reduce of ones over RCCL
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)
        exchange = {"rccl_ranks": int(ones.item()), "bytes": int(bucket.flat.numel() * 4),
                    "bytes_per_gaussian": bucket.bytes_per_gaussian, "ipc_mode_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}
        if a.full:
            # the collective alone (not overlapped with anything), max over ranks
            fence()
            t0 = time.perf_counter()
            for _ in range(10):
                dist.all_reduce(bucket.flat)
            fence()
            tt = torch.tensor([(time.perf_counter() - t0) / 10], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            exchange["allreduce_ms"] = float(tt.item()) * 1e3
        # How the exchange is issued is measured, not guessed: {all-reduce, reduce-scatter + all-gather} x Gaussian ranges
        # {1, 4} of the overlapped backward (ranges only with the all-reduce). Every rank times every candidate, the
        # clocks are combined with MAX over the ranks, so every rank picks the same one.
        algos = ["all_reduce", "rs_ag"] if (a.ar_algo == "auto" and world > 1 and a.backend == "nccl") else [bucket.algo]
        cand = [(al, k) for al in algos for k in ([a.ar_chunks] if a.ar_chunks > 0 else [1, 4]) if al == "all_reduce" or k == 1]
        if not cand:
            cand = [(algos[0], 1)]
        buckets = {bucket.algo: bucket}
        tried = {}
        for al, k in cand:
            if al not in buckets:
                buckets[al] = GradBucket([params[n] for n in names], cols=bucket_cols, names=names, algo=al)
            bucket = buckets[al]
            bucket.chunks = k
            for _ in range(5):
                step()
            fence()
            t0 = time.perf_counter()
            for _ in range(30):
                step()
            fence()
            tt = torch.tensor([(time.perf_counter() - t0) / 30], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            tried[f"{al}/{k}"] = float(tt.item()) * 1e3
        # the fastest; a candidate listed earlier (plain all-reduce, one range) keeps the job unless another beats it by 2 %
        best = next(iter(tried))
        for name, ms in tried.items():
            if ms < 0.98 * tried[best]:
                best = name
        bucket = buckets[best.split("/")[0]]
        bucket.chunks = int(best.split("/")[1])
        for al, b in buckets.items():
            if b is not bucket:
                b.close()
        exchange.update(algo=bucket.algo, chunks=bucket.chunks, candidates_tried_ms_per_step=tried)
    for _ in range(a.warmup):
        step()
    fence()
    # Timed region: EXACTLY a.steps steps. With --full, HIP events (inside the library, on the launch stream) bracket the
    # dominant kernel here — every bracket costs two event records of ~3.4 us of queue time, and bracketing all six
    # kernel groups slows the step by 5 %. The per-group breakdown is taken right after, outside the timed region.
    if a.full:
        slots = abi.profile_slot_names()
        abi.profile_select(1 << slots.index("render_bwd"))
        abi.profile_reset()
        abi.profile_enable(1)
    stamps = [0.0] * (a.steps + 1)  # host clock after each step's calls returned (no synchronisation: diagnostics only)
    last = None
    t0 = stamps[0] = time.perf_counter()
    for i in range(a.steps):
        last = None  # (the previous step's outputs are released before the next step starts)
        last = step()
        stamps[i + 1] = time.perf_counter()
    fence()
    dt = time.perf_counter() - t0
    color, radii, invdepth = last
    if a.dump_outputs and rank == 0:
        grads = {k: params[k].grad for k in names}
        grads["means2D"] = means2D.grad
        dump_outputs(a.dump_outputs, color, radii, invdepth, grads)
    if a.full:
        abi.profile_enable(0)
        prof_timed = abi.profile()
        abi.profile_select(0xFFFFFFFF)
        abi.profile_reset()
        abi.profile_enable(1)
        for _ in range(a.steps):
            step()
        fence()
        abi.profile_enable(0)
        prof = abi.profile()
        if prof_timed.get("render_bwd", (0, 0))[1]:
            prof["render_bwd"] = prof_timed["render_bwd"]  # the live measurement over the timed region
    if use_dist:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())

    # num_rendered of this rank's view (the last timed step's), straight from the API's own bookkeeping
    # (num_rendered_exact: this forward's own counts; num_rendered may name a workspace sized from the previous forward)
    nr = int(getattr(color.grad_fn, "num_rendered_exact", getattr(color.grad_fn, "num_rendered", -1)))
    # the API's num_rendered packs both counts: (tile, Gaussian) record slots below, (32-px block, Gaussian) list entries
    # above (csrc/common.h nr_pack)
    R, R_entries = (nr & 0x7FFFFFFF, (nr >> 32) & 0x07FFFFFF) if nr >= 0 else (-1, -1)

    ti_dist = None
    if use_dist and a.full and not a.no_train_iter:
        # the iteration that can actually scale: three renders, ONE exchange, the optimizer step
        ti_dist = train_iteration(sc, P, H, W, dev, fused=True, dist=dist, view_seed=rank, algo=bucket.algo)
    ti_dist_graphed = None
    if use_dist and a.full and not a.no_train_iter and a.graph_train_iter:
        # opt-in (never part of the driver's line): the same iteration with its three renders, loss and backward passes
        # recorded into a HIP graph per rank; the exchange and the optimizer step stay outside
        ti_dist_graphed = train_iteration(sc, P, H, W, dev, fused=True, dist=dist, view_seed=rank, algo=bucket.algo, graphed=True)
    if rank == 0:
        ms_step = dt / a.steps * 1e3
        npx = H * W
        if a.full:
            kern = {k: ms / a.steps for k, (ms, n) in prof.items() if n}  # device ms per step of each kernel group
            dom = max(kern, key=kern.get) if kern else None
            # algorithmic bytes per launch group. Since round 3 the groups "binning" (count scan, entry expand,
            # block sort) and "depth_sort" (per-block depth order + split into tile lists) together do the job the survey
            # prices at 12 R + 2 x 24 R + 8 R (keys written, a two-pass sort of 12-byte pairs, ranges) and 64 P (the depth
            # order): the figures stay the survey's, the split between the two groups follows what each kernel moves
            # (16-byte entries: write + one sort pass; then 8-byte list items written once).
            alg = {
                "render_bwd": 52 * R + 32 * npx,
                "render_fwd": 52 * R + 32 * npx,
                "binning": 12 * R + 24 * R * 2 + 8 * R,
                "preprocess_fwd": 104 * P,
                "depth_sort": 4 * 16 * P,
                "gaussian_bwd": 300 * P,
            }
            roof = None
            live = {}
            if dom:
                ach = alg[dom] / (kern[dom] * 1e-3) / 1e9
                # observed in this run (rocprofv3 --pmc children) where the profiler is there; else the committed profile of the
                # same kernel sources; else null
                live, live_note = ({}, "disabled") if (a.no_live_traffic or use_dist) else live_traffic(a)
                traffic, tsrc = (live[dom], live_note) if dom in live else measured_traffic(dom, a)
                roof = {"kernel": dom, "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": ach / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": tsrc,
                        "algorithmic_bytes": alg[dom], "kernel_ms": kern[dom]}
                valu = measured_valu(dom, a)
                if valu:
                    # the bound this kernel really runs at: VALU issue. 1024 SIMDs x 2.4 GHz; a wave64 VALU instruction
                    # occupies its SIMD for 2.4 (all-VGPR fma/mul/add) to 4.2 cycles (SGPR operand, cmp, cndmask, DPP) and
                    # 8.5 for v_exp/v_rcp (tools/ubench.hip)
                    cyc = kern[dom] * 1e-3 * 2.4e9 * 1024 / valu
                    roof["valu_issue"] = {"valu_wave_insts": valu, "simd_cycles_per_valu_inst": cyc,
                                          "floor_simd_cycles_per_inst": [2.4, 4.2],
                                          "insts_per_pair": valu / max(R, 1)}
                    # the same kernel against the fp32 vector peak (157.3 TFLOP/s = 1024 SIMDs x 64 FLOP/clk x 2.4 GHz): every
                    # VALU wave-instruction counted as 64 lanes x 2 FLOP, i.e. an upper bound on useful work. The headline
                    # `frac` stays the HBM one, as BASELINE.md prescribes.
                    tf = valu * 64 * 2 / (kern[dom] * 1e-3) / 1e12
                    # ... and against what the kernel's own instruction mix can issue at best: its trips timed as bare instruction
                    # SEQUENCES (tools/ubench.hip, profiles/r02_ubench.txt: 105 cycles per wave for the backward trip's 32 VALU
                    # + 2 SALU at 8 waves per SIMD, LDS traffic overlapped) = 3.3 SIMD-cycles per VALU instruction
                    floor_cyc = 105.0 / 32.0
                    roof["valu"] = {"bound": "valu", "achieved": tf, "peak": 157.3, "unit": "TFLOP/s", "frac": tf / 157.3,
                                    "issue_floor_simd_cycles_per_inst": floor_cyc, "frac_of_issue_floor": floor_cyc / cyc}
                    # the second pipe this kernel keeps busy: the LDS array (one per CU, 256 B per clock). SQ_LDS_IDX_ACTIVE = its
                    # active cycles summed over the CUs; against 256 CUs x the launch's duration at the nominal 2.4 GHz (the
                    # clock under this load is lower, DESIGN.md 2.8: the true share is higher). Round 5 found the backward at
                    # 0.65 of that (0.8 of its real clock) beside a VALU that never idles: its ds_read_b96 and ds_read2_b32 forms
                    # were costing twice their bytes.
                    lds_active, lds_conf = measured_valu(dom, a, "SQ_LDS_IDX_ACTIVE"), measured_valu(dom, a, "SQ_LDS_BANK_CONFLICT")
                    if lds_active:
                        cu_cycles = 256 * kern[dom] * 1e-3 * 2.4e9
                        roof["lds"] = {"lds_array_active_cycles": lds_active, "cu_cycles_at_2.4GHz": cu_cycles,
                                       "frac_of_cu_cycles": lds_active / cu_cycles, "bank_conflict_cycles": lds_conf}
            # every kernel group against the HBM roofline (the render kernels are VALU-issue-bound: DESIGN.md §4)
            per_kernel = {}
            for k, ms in kern.items():
                if k in alg and ms > 0:
                    tr = live[k] if (dom and k in live) else measured_traffic(k, a)[0]
                    per_kernel[k] = {"algorithmic_bytes": alg[k], "achieved": alg[k] / (ms * 1e-3) / 1e9,
                                     "frac": alg[k] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": tr}
        pipe_bytes = 432 * P + 268 * R + 64 * npx
        pipe = {"algorithmic_bytes": pipe_bytes, "achieved": pipe_bytes / (ms_step * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
                "achievable_stream_GBps": HBM_ACHIEVABLE_GBS,
                "unit": "GB/s", "frac": pipe_bytes / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "ideal_sort_frac": (432 * P + 148 * R + 64 * npx) / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS}
        line = {
            "metric": "rasterizer fwd+bwd throughput @1M Gaussians/1024^2 (train iters/s with 1 render/iter)",
            "value": world * a.steps / dt, "unit": "views/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"{P} Gaussians x {H}x{W} x 5 channels, opacity={a.opacity}, 1 view per GPU, "
                                   f"fwd+bwd" + (" + RCCL grad all-reduce (56 B/Gaussian)" if use_dist else ""),
                       "gaussians": P, "height": H, "width": W, "num_rendered": R, "list_entries": R_entries,
                       "list_block_px": 32 if nr >= 0 and (nr >> 62) & 1 else 8,
                       "parallelism": f"view-dp{world}"},
            "pipeline": pipe,
            "ramp_s": ramp_s,  # untimed clock ramp before the contract's warmup (a fresh box starts at idle clocks)
        }
        # how the forwards of the run obtained their counts (eogs2_amd/rasterizer.py: "hit" = queued whole on the previous
        # forward's counts)
        from eogs2_amd import rasterizer as _rz
        # An eager forward blocks on its count readback (as the reference's does, rasterizer_impl.cu:284), so the host is never
        # more than one step ahead and a stall of the host idles the GPU: the per-step host intervals of the timed region say
        # whether `ms_per_step` is the steady state (median = mean) or carries a hiccup (max >> median).
        iv = sorted((stamps[i + 1] - stamps[i]) * 1e3 for i in range(a.steps))
        line["host"] = {"count_readback": _rz.speculation_stats(),
                        "timed_step_intervals_ms": {"median": iv[len(iv) // 2], "min": iv[0], "max": iv[-1]} if iv else None}
        if a.full:
            line.update(roofline=roof, kernels_ms=kern, kernel_rooflines=per_kernel)
            # how much of the step the host adds on top of the kernels (launch gaps, the count readback)
            ksum = float(sum(kern.values()))
            line["host"].update(kernel_sum_ms=ksum, step_over_kernel_sum=ms_step / ksum if ksum > 0 else None)
        if exchange is not None:
            exchange["backend"] = a.backend + (" (rehearsal: ranks share one GPU)" if a.share_gpu else "")
            line["exchange"] = exchange
            line["rccl_ranks"] = exchange["rccl_ranks"]
            if "allreduce_ms" in exchange:
                line["allreduce_ms"] = exchange["allreduce_ms"]
        if use_dist and a.full and not a.no_train_iter:
            line["train_iter_fused"] = ti_dist
            if ti_dist_graphed is not None:
                line["train_iter_fused_graphed"] = ti_dist_graphed
        if a.full and world == 1 and not use_dist and not a.no_train_iter:
            line["train_iter"] = train_iteration(sc, P, H, W, dev, fused=False)
            line["train_iter_fused"] = train_iteration(sc, P, H, W, dev, fused=True)
            line["train_iter_fused_sun_altitude_only"] = train_iteration(sc, P, H, W, dev, fused=True, sun_altitude_only=True)
            # the three renders queued on three streams (eogs2_amd.graph.Branches) in the EAGER loop
            line["train_iter_fused_three_streams"] = train_iteration(sc, P, H, W, dev, fused=True, parallel=True)
            # The same step and the same iteration recorded into HIP graphs and replayed (eogs2_amd/graph.py): beside the
            # headline, never the headline — `value` stays the eager call through the reference's API. Measured in a child
            # process started after everything above is done: a failed capture must not cost this line.
            line.update(graph_extras_from_child(a, line["host"]["kernel_sum_ms"]))
            # the regimes beside the headline (worst case included): opacity 0.1, trained opacities, the 2048^2 sun-camera
            # size, 2 M Gaussians — `value` / `config` stay the headline's
            line["regimes"] = regime_scan(dev)
            line["train_example"] = train_example_bench(P, H)
            line["photometric_loss"] = photometric_loss_bench(abi, dev, H, W)
            line["optimizer"] = optimizer_bench(abi, dev, P)
            line["resample"] = resample_bench(abi, dev, H, W)
            line["shade"] = shade_bench(abi, dev, H, W)
            line["tsdf"] = tsdf_bench(abi, dev)
        if a.full and world == 1 and not a.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(P, H)
        print(json.dumps(line), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
