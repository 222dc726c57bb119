"""The mesh extraction on one GPU (eogs2_amd.mesh, TSDFVolume.extract_mesh's work) on synthetic terrain volumes, beside the
first step of what the reference does instead: the copy of the whole volume to the host (tsdf.py:523,
`self._tsdf_vol.cpu().numpy()`), which is a floor under the reference's cost. The third-party `mcubes` that the reference
runs on that copy is not installed here and is NOT timed.

    python tools/mesh_probe.py [--out profiles/mesh_probe.json] [--rounds 7] [--iters 20]
    python tools/mesh_probe.py --trace 512 --iters 20          warm calls at one size and nothing else: the program to put
                                                               after `rocprofv3 --kernel-trace --stats ... --`
    python tools/mesh_probe.py --kernel-stats 512=<kernel_stats.csv> [...] --out <json>
                                                               folds the per-launch averages of such a run into the file

Times: a host clock around `iters` calls that end in a device synchronise; after a warm-up of every shape the paths
alternate, `rounds` turns each. Reported per path: the median turn in ms per call and the spread of the turns (min, max).
`count` and `emit` are the two phases through the C-ABI alone (device events around each entry's launches, the emit phase
on the sizes already known); the per-launch times come from a profiler run of its own. Before anything is timed the mesh
at the timed size is checked: closed but for the volume's boundary, the vertex count of the sign changes. No time is an
acceptance condition; the file records what was measured and what was not.
"""
import argparse
import csv
import ctypes
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd import _lib, mesh  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402

SHAPES = {256: (256, 256, 96), 512: (512, 512, 192)}


def terrain_volume(shape, dev, trunc=4.0):
    """A truncated signed distance to a rolling terrain with two box buildings, in voxels: negative below the surface."""
    nx, ny, nz = shape
    x, y = torch.meshgrid(torch.linspace(-1, 1, nx, device=dev), torch.linspace(-1, 1, ny, device=dev), indexing="ij")
    h = nz * (0.4 + 0.12 * torch.sin(5 * x) * torch.cos(4 * y) + 0.2 * ((x.abs() < 0.3) & (y.abs() < 0.2)) +
              0.15 * (((x - 0.6).abs() < 0.15) & ((y + 0.5).abs() < 0.25)))
    z = torch.arange(nz, device=dev, dtype=torch.float32)
    return ((z[None, None, :] - h[:, :, None] + 0.37) / trunc).clamp(-1.0, 1.0).contiguous()


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def check(vol, vertices, triangles):
    ins = vol < 0
    crossings = sum(int((ins.narrow(a, 0, vol.shape[a] - 1) != ins.narrow(a, 1, vol.shape[a] - 1)).sum()) for a in range(3))
    assert vertices.shape[0] == crossings, (vertices.shape[0], crossings)
    t = triangles.long()
    nv = vertices.shape[0]
    fwd = (t * nv + t.roll(-1, dims=1)).reshape(-1)
    rev = (t.roll(-1, dims=1) * nv + t).reshape(-1)
    assert fwd.unique().numel() == fwd.numel(), "a directed edge occurs twice"
    lone = int((~torch.isin(fwd, rev)).sum())
    assert lone < 8 * sum(vol.shape[:2]), f"{lone} unpaired edges: more than the volume's boundary can hold"
    return {"vertices": int(nv), "triangles": int(t.shape[0]), "unpaired_boundary_edges": lone}


def phases(vol, iters):
    """Device events around the launches of eogs_mesh_count and of eogs_mesh_emit (its 16-byte read-back included)."""
    abi, dev = _lib.get(), vol.device
    nx, ny, nz = vol.shape
    nb = ctypes.c_size_t()
    abi.check(abi.mesh_bytes(nx, ny, nz, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    count = lambda: abi.check(abi.mesh_count(nx, ny, nz, p(vol), 0.0, p(ws), ws.numel(), p(counts), stream))  # noqa: E731
    count()
    nv, nt = (int(c) for c in counts.cpu().numpy().view(np.uint32)[:2])
    vertices = torch.empty((nv, 3), dtype=torch.float64, device=dev)
    triangles = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    emit = lambda: abi.check(abi.mesh_emit(nx, ny, nz, p(vol), 0.0, None, None, None, None, p(ws), ws.numel(), p(vertices), nv,  # noqa: E731
                                           p(triangles), nt, stream))
    out = {}
    for name, fn in (("count", count), ("emit", emit)):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name + "_ms"] = a.elapsed_time(b) / iters
    return out


def fold_kernel_stats(out, specs):
    for spec in specs:
        size, path = spec.split("=", 1)
        per = {}
        for r in csv.DictReader(open(path)):
            m = re.search(r"\bmesh_[a-z_]+_kernel\b", r["Name"])  # "(anonymous namespace)::mesh_count_kernel(...)"
            if m:
                per[m.group(0)] = {"average_us": float(r["AverageNs"]) / 1e3, "calls": int(r["Calls"])}
        assert per, f"{path}: no mesh_* kernel in the statistics"
        out.setdefault(f"extract_mesh_{size}", {})["per_launch"] = per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_probe.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--trace", type=int, default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=None)
    a = ap.parse_args()
    if a.kernel_stats is not None:
        out = json.load(open(a.out))
        fold_kernel_stats(out, a.kernel_stats)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print("folded", a.kernel_stats, "into", a.out)
        return
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    if a.trace is not None:
        vol = terrain_volume(SHAPES[a.trace], dev)
        for _ in range(a.iters + 3):
            mesh.marching_cubes(vol)
        torch.cuda.synchronize()
        return
    out = {"what": f"host clock around {a.iters} calls that end in a device synchronise; the paths alternate, {a.rounds} turns each; "
                   "ms per call", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0)}
    for S in a.sizes:
        shape = SHAPES[S]
        vol = terrain_volume(shape, dev)
        agree = check(vol, *mesh.marching_cubes(vol))
        hip = lambda: mesh.marching_cubes(vol)  # noqa: E731
        copy = lambda: vol.cpu().numpy()  # noqa: E731
        ours, theirs = [], []
        for k in range(a.rounds + 1):  # one warm-up turn
            th, tc = timed(hip, a.iters), timed(copy, a.iters)
            if k:
                ours.append(th)
                theirs.append(tc)
        h, c = summary(ours), summary(theirs)
        voxels = shape[0] * shape[1] * shape[2]
        out[f"extract_mesh_{S}"] = {"shape": list(shape), "voxels": voxels, "mesh": agree, "marching_cubes": h, "volume_to_host_copy": c,
                                    "copy_over_marching_cubes": c["median_ms"] / h["median_ms"],
                                    "spread_ms": max(h["max_ms"] - h["min_ms"], c["max_ms"] - c["min_ms"]), "phases": phases(vol, a.iters),
                                    "volume_bytes": 4 * voxels,
                                    "note": "marching_cubes: both phases, the wait for the sizes, the workspace and output allocations; "
                                            "the copy is only the FIRST step of the reference's extract_mesh, mcubes itself is not timed"}
        print(f"extract_mesh_{S}", json.dumps(out[f"extract_mesh_{S}"]), flush=True)
    out["not_measured"] = ("the third-party mcubes on the host copy (not installed here): the copy alone stands for the reference, as a "
                           "floor; the OBJ write; world coordinates and the shift (two more multiplies and adds per vertex); random "
                           "volumes, whose surface is far denser than terrain; an LDS halo tile for the eight corner reads")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
