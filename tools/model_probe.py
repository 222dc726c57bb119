"""`eogs2_amd.model.GaussianModel` on one GPU against the reference's own lines (scene/gaussian_model.py) as torch / numpy on
the same host and card, at `--rows` Gaussians and `--sh`:

  create_from_pcd  without the kNN (`dist2` is handed to both sides): one launch against gaussian_model.py:167-215 as torch ops;
  save_ply         pack launch + one copy into page-locked memory + one write, against :313-343: seven `.cpu().numpy()`, the
                   concatenation, and `elements[:] = list(map(tuple, attributes))`. plyfile is not installed here: the
                   reference's `PlyData([el]).write(path)` is stood in for by the header and `elements.tofile`, what plyfile's
                   binary writer comes to;
  load_ply         header parse + one read into page-locked memory + one copy + unpack launch, against :374-447: the columns
                   one by one into float64 `np.zeros`, then six `torch.tensor(..., device="cuda")`. `PlyData.read` is stood in for
                   by `np.fromfile` with the structured dtype;
  pack kernel      eogs_model_rows_pack against a device-to-device copy of the block's bytes: 200 back-to-back launches between
                   one pair of device events, once on the same buffers (warm in the last-level cache) and once rotating over 8
                   independent sets; and, apart, one whole `pack_rows` call of the Python wrapper between events.

    python tools/model_probe.py [--out profiles/model_probe.json] [--rows 1000000] [--sh 0] [--rounds 5] [--dir DIR]

Times: after one warm-up turn the two paths alternate, `rounds` times; a turn is the host clock around one call that ends in
a device synchronise (the pack kernel: device events, see above). Reported per path: the median turn in ms and the spread (min, max).
The files go to `--dir` (default: the system's temporary directory), whose file system is part of what is measured. No speed
ratio is an acceptance condition of this feature; the file records what was measured and what was not.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd import _lib, model as M  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402

C0 = 0.28209479177387814
LAUNCHES = 200  # back-to-back launches between one pair of events
ROTATE = 8      # independent buffer sets of the cold-cache variant


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(paths, rounds, warmup=1):
    rows = {n: [] for n, _ in paths}
    for k in range(rounds + warmup):
        for n, fn in paths:
            ms = fn()
            if k >= warmup:
                rows[n].append(ms)
    out = {n: summary(ts) for n, ts in rows.items()}
    out["spread_ms"] = max(v["max_ms"] - v["min_ms"] for v in out.values())
    return out


# ---- the reference's steps ----
# What the other side of each comparison costs is decided by WHICH operations the reference runs and how often: they are kept
# one for one (every copy, every float64 array, every Python-level loop), written over this probe's own names and loops.
SAVE_ORDER = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def ref_create(points, colors, dist2, sh, opacity_init):
    """The op sequence of gaussian_model.py:167-215 on device tensors (distCUDA2's result handed in): a zero [P, 3, K] feature
    array with the colours written into its first column, clamp -> sqrt -> log -> repeat, a zero [P, 4] with a column of ones,
    the logit of a filled [P, 1], two transposed copies, six Parameters and a zero [P]."""
    n, dev = points.shape[0], points.device
    feats = torch.zeros((n, 3, (sh + 1) ** 2)).float().to(dev)
    feats[:, :3, 0] = (colors - 0.5) / C0
    feats[:, 3:, 1:] = 0.0
    scales = torch.log(torch.sqrt(torch.clamp_min(dist2, 0.0000001)))[..., None].repeat(1, 3)
    rots = torch.zeros((n, 4), device=dev)
    rots[:, 0] = 1
    o = opacity_init * torch.ones((n, 1), dtype=torch.float, device=dev)
    tensors = (points, feats[:, :, 0:1].transpose(1, 2).contiguous(), feats[:, :, 1:].transpose(1, 2).contiguous(), scales, rots,
               torch.log(o / (1 - o)))
    return [torch.nn.Parameter(t.requires_grad_(True)) for t in tensors], torch.zeros(n, device=dev)


def ref_save(m, path):
    """The steps of gaussian_model.py:313-345: one `.cpu().numpy()` per tensor (the two feature tensors transposed and
    flattened on the device first), a zero array of normals, one concatenation, a structured array filled from one Python tuple
    per row, and the write (stood in for: see the module docstring)."""
    host = {}
    for attr in SAVE_ORDER:
        t = getattr(m, attr).detach()
        if t.ndim == 3:
            t = t.transpose(1, 2).flatten(start_dim=1).contiguous()
        host[attr] = t.cpu().numpy()
    names = m.construct_list_of_attributes()
    table = np.concatenate([host["_xyz"], np.zeros_like(host["_xyz"])] + [host[a] for a in SAVE_ORDER[1:]], axis=1)
    elements = np.empty(table.shape[0], dtype=[(n, "f4") for n in names])
    elements[:] = list(map(tuple, table))
    with open(path, "wb") as f:
        f.write(M.ply_header(names, table.shape[0]))
        elements.tofile(f)


def ref_load(path, sh):
    """The steps of gaussian_model.py:374-447 over a structured array (PlyData.read stood in for by np.fromfile): every family
    of properties gathered column by column into a float64 array, then one `torch.tensor(..., dtype=float, device="cuda")`
    per tensor, the two feature tensors transposed and made contiguous on the device."""
    with open(path, "rb") as f:
        names, count, offset = M.parse_ply_header(f.read(1 << 16))
    el = np.fromfile(path, dtype=np.dtype([(n, "<f4") for n in names]), count=count, offset=offset)

    def columns(cols):  # a float64 [P, len(cols)] filled one column at a time
        out = np.zeros((count, len(cols)))
        for k, c in enumerate(cols):
            out[:, k] = np.asarray(el[c])
        return out

    def family(prefix):
        return sorted((n for n in names if n.startswith(prefix)), key=lambda n: int(n.rsplit("_", 1)[1]))

    rest = family("f_rest_")
    assert len(rest) == 3 * (sh + 1) ** 2 - 3
    host = [np.stack([np.asarray(el[c]) for c in "xyz"], axis=1), columns(["f_dc_0", "f_dc_1", "f_dc_2"]).reshape(count, 3, 1),
            columns(rest).reshape(count, 3, (sh + 1) ** 2 - 1), np.asarray(el["opacity"])[..., np.newaxis], columns(family("scale_")),
            columns(family("rot"))]
    dev = [torch.tensor(h, dtype=torch.float, device="cuda") for h in host]
    dev[1], dev[2] = dev[1].transpose(1, 2).contiguous(), dev[2].transpose(1, 2).contiguous()
    return [torch.nn.Parameter(t.requires_grad_(True)) for t in dev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_probe.json"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev, P, sh = torch.device("cuda:0"), a.rows, a.sh
    g = torch.Generator().manual_seed(0)
    out = {"what": f"{P} rows, sh_degree {sh}; the two paths alternate, {a.rounds} turns each after one warm-up turn; host clock around "
                   "one call that ends in a device synchronise (pack kernel: device events); ms per call",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0)}
    points, colors = (torch.rand(P, 3, generator=g) * 2 - 1).to(dev), torch.rand(P, 3, generator=g).to(dev)
    dist2 = torch.exp(torch.empty(P).uniform_(-16, -4, generator=g)).to(dev)
    pcd, cams = types.SimpleNamespace(points=points, colors=colors), [types.SimpleNamespace(image_name="v")]
    quiet = open(os.devnull, "w")

    def hip_create():
        m = M.GaussianModel(sh)
        stdout, sys.stdout = sys.stdout, quiet  # (create_from_pcd prints the number of points, as the reference does)
        try:
            m.create_from_pcd(pcd, cams, 1.0, 0.1, dist2=dist2)
        finally:
            sys.stdout = stdout
        return m

    # the two sides make the same model (f_dc and scaling up to the last bit of a division and a log)
    m = hip_create()
    ref, _ = ref_create(points.clone(), colors, dist2, sh, 0.1)
    for got, want in zip((m._xyz, m._features_dc, m._features_rest, m._scaling, m._rotation, m._opacity), ref):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    out["create_from_pcd"] = alternate([("hip", lambda: host_timed(hip_create)[0]),
                                        ("torch_lines", lambda: host_timed(lambda: ref_create(points.clone(), colors, dist2, sh, 0.1))[0])], a.rounds)
    out["create_from_pcd"]["note"] = "without the kNN; the torch side's points.clone() stands for the upload both sides would do"
    print("create_from_pcd", json.dumps(out["create_from_pcd"]), flush=True)

    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        ours, theirs = os.path.join(d, "ours.ply"), os.path.join(d, "theirs.ply")
        m.save_ply(ours)
        ref_save(m, theirs)
        assert open(ours, "rb").read() == open(theirs, "rb").read()  # the same file, byte for byte
        out["file_bytes"] = os.path.getsize(ours)
        out["save_ply"] = alternate([("hip", lambda: host_timed(lambda: m.save_ply(ours))[0]),
                                     ("reference_lines", lambda: host_timed(lambda: ref_save(m, theirs))[0])], a.rounds)
        print("save_ply", json.dumps(out["save_ply"]), flush=True)

        def hip_load():
            fresh = M.GaussianModel(sh)
            fresh.load_ply(ours)
            return fresh

        fresh, want = hip_load(), ref_load(theirs, sh)
        for got, w in zip((fresh._xyz, fresh._features_dc, fresh._features_rest, fresh._opacity, fresh._scaling, fresh._rotation), want):
            assert torch.equal(got, w)
        out["load_ply"] = alternate([("hip", lambda: host_timed(hip_load)[0]),
                                     ("reference_lines", lambda: host_timed(lambda: ref_load(theirs, sh))[0])], a.rounds)
        print("load_ply", json.dumps(out["load_ply"]), flush=True)

    # ---- the pack kernel itself: LAUNCHES back-to-back calls of the C entry between ONE pair of events, so that the host work of
    # a call (a few microseconds of ctypes each, queued ahead of the device) is no part of the figure ----
    abi, stream = _lib.get(), torch.cuda.current_stream(dev).cuda_stream
    n_rest, ptr = (sh + 1) ** 2 - 1, lambda t: t.data_ptr() if t.numel() else None  # noqa: E731

    def sets(k):  # k independent (six tensors, block, twin) sets
        out_ = []
        for _ in range(k):
            six = tuple(getattr(m, a_).detach().clone() for a_ in SAVE_ORDER)
            block = torch.empty((P, M.row_cols(n_rest)), dtype=torch.float32, device=dev)
            out_.append((six, block, torch.empty_like(block)))
        return out_

    def kernel_ms(group, what):
        def run():
            for i in range(LAUNCHES):
                six, block, twin = group[i % len(group)]
                if what == "pack":
                    abi.check(abi.model_rows_pack(P, n_rest, *(ptr(t) for t in six), ptr(block), stream))
                else:
                    twin.copy_(block)
        return event_timed(run) / LAUNCHES

    block_bytes = P * M.row_cols(n_rest) * 4
    warm, rotating = sets(1), sets(ROTATE)
    out["pack_kernel"] = {"block_bytes": block_bytes, "launches_per_turn": LAUNCHES}
    for label, group in (("same_buffers", warm), ("rotating_buffers", rotating)):
        r = alternate([("pack_rows_kernel", lambda g=group: kernel_ms(g, "pack")), ("device_copy_of_the_block", lambda g=group: kernel_ms(g, "copy"))],
                      a.rounds, warmup=1)
        r["kernel_over_copy"] = r["pack_rows_kernel"]["median_ms"] / r["device_copy_of_the_block"]["median_ms"]
        out["pack_kernel"][label] = r
    out["pack_kernel"]["note"] = (
        f"ms per launch = one event pair around {LAUNCHES} back-to-back launches / {LAUNCHES}. same_buffers: every launch reads and writes "
        f"the same tensors, {2 * block_bytes >> 20} MiB in all, which stay warm in the 256 MiB last-level cache on both sides; "
        f"rotating_buffers: {ROTATE} independent sets in turn ({ROTATE * 2 * block_bytes >> 20} MiB in all), so that a launch finds "
        "little of its data cached. Both sides move block_bytes in and block_bytes out (at sh 0 the kernel reads 14 of the 17 columns: the "
        "normals are written, not read)")
    # one whole call of the Python wrapper (argument checks, ctypes, the launch), between events: what a caller of pack_rows sees
    six, block, _ = warm[0]
    out["pack_rows_call"] = alternate([("pack_rows", lambda: event_timed(lambda: M.pack_rows(*six, out=block)))], max(a.rounds, 20), warmup=3)
    print("pack_kernel", json.dumps(out["pack_kernel"]), flush=True)
    print("pack_rows_call", json.dumps(out["pack_rows_call"]), flush=True)
    out["not_measured"] = ("the kNN of create_from_pcd (tests/test_gpu_knn.py, profiles: the same on both sides); plyfile itself (not "
                           "installed: its binary write and read are stood in for by tofile / fromfile); other row counts and SH "
                           "degrees; a cold page cache; a network file system; the first call's page-locked allocation (warm-up turn)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
