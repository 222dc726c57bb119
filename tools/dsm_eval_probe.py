"""DSM evaluation on one GPU: compute_shift + MAE (eogs2_amd.dsm_eval) at 512^2, 1024^2 and 2048^2 against the vectorised
CPU restatement of the reference (tests/dsm_eval_cases.py, torch / numpy on the CPUs the job has) on the same inputs.

    python tools/dsm_eval_probe.py [--out profiles/dsm_eval_probe.json] [--sizes 512 1024 2048] [--reps 25]

Inputs: the terrain with buildings of eogs2_amd.synthetic._height_field in altitude units (ALT_SCALE x normalised z),
float32, the second image shifted by a known (dx, dy) and mapped by 0.97 z + 2.5, 5 % NaN in each.
Times: after a warm-up of every shape, `reps` repetitions; per repetition the library's profile slots (HIP events on the
launch stream around each kernel group) give the device time of each group, and a host clock around the call, which ends
in its own read-back, gives the end-to-end time; medians are reported. The level-0 search is also timed alone
(ncc_search at full resolution around the known centre): its `dsm_moments` time over the two images' bytes is the achieved
rate of the one pass the search makes over them. The reference's own implementation (numba) cannot run here; the CPU figure
is the restatement's, once per size (it takes seconds), and no ratio is an acceptance condition.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dsm_eval_cases as C  # noqa: E402
from eogs2_amd import _lib, dsm_eval as D  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402
from eogs2_amd.synthetic import ALT_SCALE, _height_field  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s
SLOTS = ("dsm_downsample", "dsm_pivots", "dsm_moments", "dsm_finalize", "dsm_apply_shift", "dsm_mae")


def pair(S, shift, seed):
    dx, dy = shift
    m = max(abs(dx), abs(dy)) + 2
    n = S + 2 * m
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.linspace(-0.9, 0.9, n, dtype=torch.float64), torch.linspace(-0.9, 0.9, n, dtype=torch.float64),
                          indexing="ij")
    base = (_height_field(x, y, g)[0] * ALT_SCALE).numpy()
    rng = np.random.default_rng(seed)
    base = base + 0.05 * rng.normal(size=base.shape)  # sensor-like noise: flat roofs alone have no texture
    u = base[m:m + S, m:m + S].astype(np.float32)
    v = (0.97 * base[m - dy:m - dy + S, m - dx:m - dx + S] + 2.5).astype(np.float32)
    u[rng.random(u.shape) < 0.05] = np.nan
    v[rng.random(v.shape) < 0.05] = np.nan
    return u, v


def measure(abi, fn, reps):
    """Per repetition: host ms around fn() (which ends in a read-back) and the device ms of every DSM slot."""
    host, slots = [], {k: [] for k in SLOTS}
    for _ in range(reps):
        abi.profile_reset()
        torch.cuda.synchronize()
        abi.profile_enable(1)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        abi.profile_enable(0)
        prof = abi.profile()
        for k in SLOTS:
            slots[k].append(prof[k][0])
    return float(np.median(host)), {k: float(np.median(v)) for k, v in slots.items()}


def plain_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsm_eval_probe.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=(512, 1024, 2048))
    ap.add_argument("--reps", type=int, default=25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.reps >= 20
    dev = torch.device("cuda:0")
    abi = _lib.get()
    abi.profile_select(0xFFFFFFFF)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"what": "compute_shift + dsm_mae, float32 images, irange 5; median of %d after warm-up; CPU = the vectorised "
                   "restatement of the reference (tests/dsm_eval_cases.py), one run" % a.reps,
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(), "sizes": {}}
    for S in a.sizes:
        shift = (7, -9)
        u, v = pair(S, shift, seed=S)
        gu, gv = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
        for _ in range(3):  # warm-up of every shape
            tr = D.compute_shift(gu, gv)
            mae, _, _, _ = D.dsm_mae(gv, gu, clip="finite")
            D.ncc_search(gu, gv, 5, *shift)
        shift_ms, shift_slots = measure(abi, lambda: D.compute_shift(gu, gv), a.reps)
        mae_ms, mae_slots = measure(abi, lambda: D.dsm_mae(gv, gu, clip="finite"), a.reps)
        _, l0_slots = measure(abi, lambda: D.ncc_search(gu, gv, 5, *shift), a.reps)
        shift_ms_plain = plain_ms(lambda: D.compute_shift(gu, gv), a.reps)  # without the event brackets
        mae_ms_plain = plain_ms(lambda: D.dsm_mae(gv, gu, clip="finite"), a.reps)
        t0 = time.perf_counter()
        ctr = C.compute_shift(u, v)
        t1 = time.perf_counter()
        cdiff, _, _ = C.dsm_pointwise_diff(v, u, clip="finite")
        cmae = C.mae_of(cdiff)
        t2 = time.perf_counter()
        assert tr[:2] == ctr[:2] == shift, (tr, ctr)
        image_bytes = 2 * S * S * 4
        l0 = l0_slots["dsm_moments"]
        row = {
            "shift_found": list(tr[:2]), "a": tr[2], "b": tr[3], "mae": mae, "cpu_mae": cmae,
            "compute_shift_ms": shift_ms_plain, "compute_shift_ms_with_event_brackets": shift_ms,
            "compute_shift_kernels_ms": {k: shift_slots[k] for k in SLOTS[:4]},
            "dsm_mae_ms": mae_ms_plain, "dsm_mae_includes": "its own compute_shift(scaling=False), apply_shift, clip + diff + sum",
            "dsm_mae_kernels_ms": mae_slots,
            "level0_search_kernels_ms": {k: l0_slots[k] for k in SLOTS[1:4]},
            "level0_image_bytes": image_bytes,
            "level0_moments_GBps": image_bytes / (l0 * 1e-3) / 1e9 if l0 > 0 else None,
            "level0_moments_frac_of_8TBps": image_bytes / (l0 * 1e-3) / 1e9 / HBM_PEAK_GBS if l0 > 0 else None,
            "level0_pair_shift_per_s": S * S * 121 / (l0 * 1e-3) if l0 > 0 else None,
            "cpu_compute_shift_ms": (t1 - t0) * 1e3, "cpu_pointwise_diff_and_mae_ms": (t2 - t1) * 1e3,
        }
        assert abs(mae - cmae) <= 1e-6 * max(1.0, cmae), (mae, cmae)
        out["sizes"][f"{S}x{S}"] = row
        print(S, json.dumps(row), flush=True)
    out["not_measured"] = ("the reference's own numba implementation (numba is not installed); plyflatten and GeoTIFF I/O (the caller's); "
                           "a speed ratio is not an acceptance condition of this capability")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
