"""The DSM raster on one GPU (eogs2_amd.dsm_raster) against the same computation written as PyTorch ops, on the same card:

  view    dsm_from_view on a 1024^2 and a 2048^2 altitude image (bounds pass, one wait for the grid, scatter, stencil; no
          cloud is materialised) against: the cloud by einsum in float64 (affine_cameras.py:440-447, dsm_utils.py:11), its
          min / max read back, nine shifted index_add_ passes over float32 sums and counts, one divide;
  cloud   plyflatten on a 4 M-point float64 cloud with a given grid (no wait) against the nine passes and the divide alone.

    python tools/dsm_raster_probe.py [--out profiles/dsm_raster_probe.json] [--rounds 9] [--iters 100]

Times: a host clock around `iters` calls that end in a device synchronise; after a warm-up of every shape the two paths
alternate, `rounds` turns each. Reported per path: the median turn in ms per call and the spread of the turns (min, max).
Before anything is timed the two paths are compared at the timed size: the same counts (but for a point that a 1-ulp float64
difference moves across a cell edge), values within the float32 rounding of the yardstick's own sums. No time is an acceptance condition; the file records what was measured and
what was not.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd import dsm_raster  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402
from eogs2_amd.synthetic import ALT_SCALE, make_camera  # noqa: E402

CENTER = (512345.25, 4321987.75, 31.5)


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def torch_raster(cloud, xoff, yoff, res, xsize, ysize, radius=1):
    """Nine shifted index_add_ passes plus a divide; a pass routes the targets outside the raster to one spare cell."""
    i = torch.floor((cloud[:, 0] - xoff) / res).long()
    j = torch.floor((yoff - cloud[:, 1]) / res).long()
    z = cloud[:, 2].float()
    one = torch.ones_like(z)
    cells = xsize * ysize
    sums = torch.zeros(cells + 1, dtype=torch.float32, device=cloud.device)
    cnts = torch.zeros(cells + 1, dtype=torch.float32, device=cloud.device)
    for dj in range(-radius, radius + 1):
        for di in range(-radius, radius + 1):
            ii, jj = i + di, j + dj
            inside = (ii >= 0) & (ii < xsize) & (jj >= 0) & (jj < ysize)
            idx = torch.where(inside, jj * xsize + ii, cells)
            sums.index_add_(0, idx, z)
            cnts.index_add_(0, idx, one)
    out = torch.where(cnts > 0, sums / cnts, float("nan"))[:cells]
    return out.reshape(ysize, xsize, 1), cnts[:cells].reshape(ysize, xsize)


def torch_view(alt, cam, u, v, scale, center, res):
    """compute_dsm_from_view in PyTorch ops on the device, the reference's statements."""
    uva = torch.stack(torch.meshgrid(u, v, indexing="xy") + (alt,), dim=-1).reshape(-1, 3)
    b = cam.affine[3, :3].double()
    cloud = torch.einsum("...ij,...j->...i", cam.Ainv.double(), uva.double() - b) * scale + center
    bounds = torch.stack([cloud[:, 0].min(), cloud[:, 0].max(), cloud[:, 1].min(), cloud[:, 1].max()]).cpu().numpy()  # the wait
    xoff, yoff, xsize, ysize = dsm_raster.raster_geometry(*bounds, res)
    return torch_raster(cloud, float(xoff), float(yoff), res, xsize, ysize)


def compare(ours, ours_cnt, ref, ref_cnt, what):
    assert ours.shape == ref.shape, (what, ours.shape, ref.shape)
    moved = int((ours_cnt.clamp(min=0).float() != ref_cnt).sum())  # (a 1-ulp float64 difference in x or y may move a point)
    assert moved <= 1e-4 * ref_cnt.numel() + 1, f"{what}: {moved} cells count differently"
    same = (ours_cnt.float() == ref_cnt) & (ref_cnt > 0)
    err = float((ours[:, :, 0][same] - ref[:, :, 0][same]).abs().max())
    assert err <= 1e-3, f"{what}: the rasters differ by {err}"  # faster and different is not faster
    return {"cells": int(ref_cnt.numel()), "filled": int((ref_cnt > 0).sum()), "cells_with_other_count": moved, "max_abs_difference": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsm_raster_probe.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 2048])
    ap.add_argument("--points", type=int, default=4_000_000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    out = {"what": f"host clock around {a.iters} calls that end in a device synchronise; the two paths alternate, {a.rounds} turns each; "
                   "ms per call", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0)}
    center = torch.tensor(CENTER, dtype=torch.float64, device=dev)
    for S in a.sizes:
        vm = make_camera(S, S, seed=3, device=dev)
        cam = types.SimpleNamespace(affine=vm, Ainv=torch.inverse(vm[:3, :3].T))
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, S, device=dev), torch.linspace(-1, 1, S, device=dev), indexing="ij")
        alt = (ALT_SCALE * (0.1 * torch.sin(3 * xx) * torch.cos(2 * yy) + 0.05 * (xx > 0.1))).contiguous()
        scale, res = 0.25 * S, 0.5  # a 0.5 m raster with about one pixel per cell
        u, v = dsm_raster.view_axes(S, S, dev)
        sp = [CENTER, scale]
        hip = lambda: dsm_raster.dsm_from_view(alt, cam, sp, res, return_count=True)  # noqa: E731
        ref = lambda: torch_view(alt, cam, u, v, scale, center, res)  # noqa: E731
        (_, d0, c0), (d1, c1) = hip(), ref()
        agree = compare(d0, c0, d1, c1, f"view {S}")
        ours, theirs = [], []
        for k in range(a.rounds + 1):  # one warm-up turn
            th, tr = timed(hip, a.iters), timed(ref, a.iters)
            if k:
                ours.append(th)
                theirs.append(tr)
        h, t = summary(ours), summary(theirs)
        out[f"dsm_from_view_{S}"] = {"hip": h, "torch_ops": t, "torch_over_hip": t["median_ms"] / h["median_ms"],
                                     "spread_ms": max(h["max_ms"] - h["min_ms"], t["max_ms"] - t["min_ms"]),
                                     "raster": list(d0.shape[:2]), "agreement": agree,
                                     "note": "both sides include the one wait for the bounds"}
        print(f"dsm_from_view_{S}", json.dumps(out[f"dsm_from_view_{S}"]), flush=True)
    # ---- a cloud with a given grid ----
    N = a.points
    g = torch.Generator().manual_seed(0)
    xsize = ysize = 2048
    cloud = torch.stack([CENTER[0] + torch.rand(N, generator=g, dtype=torch.float64) * xsize * 0.5,
                         CENTER[1] - torch.rand(N, generator=g, dtype=torch.float64) * ysize * 0.5,
                         30.0 + 15.0 * torch.randn(N, generator=g, dtype=torch.float64)], dim=1).to(dev)
    geo = (CENTER[0], CENTER[1], 0.5, xsize, ysize)
    hip = lambda: dsm_raster.plyflatten(cloud, *geo, return_count=True)  # noqa: E731
    ref = lambda: torch_raster(cloud, *geo)  # noqa: E731
    (d0, c0), (d1, c1) = hip(), ref()
    agree = compare(d0, c0, d1, c1, "cloud")
    ours, theirs = [], []
    for k in range(a.rounds + 1):
        th, tr = timed(hip, a.iters), timed(ref, a.iters)
        if k:
            ours.append(th)
            theirs.append(tr)
    h, t = summary(ours), summary(theirs)
    out["plyflatten_cloud"] = {"points": N, "hip": h, "torch_ops": t, "torch_over_hip": t["median_ms"] / h["median_ms"],
                               "spread_ms": max(h["max_ms"] - h["min_ms"], t["max_ms"] - t["min_ms"]), "raster": [ysize, xsize],
                               "agreement": agree, "computed_bytes_per_call": 24 * N + 12 * (xsize + 2) * (ysize + 2) * 2 + 8 * xsize * ysize,
                               "note": "uniformly scattered points: the worst case for the atomics' locality"}
    print("plyflatten_cloud", json.dumps(out["plyflatten_cloud"]), flush=True)
    out["not_measured"] = ("the per-kernel split (bounds, clear, scatter, stencil); merging the lanes of a wave that share a cell before "
                           "the atomic; radius 0 and 2; the TSDF surface source; other point densities; the third-party plyflatten "
                           "itself, which is not installed here (the PyTorch ops stand in for it)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
