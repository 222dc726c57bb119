"""bench.py's plain run and --dump-outputs: the line of a run without --full carries the headline alone, and the dump holds
what the last timed step returned, bounded in size, the same for two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# what a plain run leaves to --full
FULL_ONLY = ("roofline", "kernels_ms", "kernel_rooflines", "train_iter", "train_iter_fused", "graphed_step", "regimes",
             "train_example", "photometric_loss", "optimizer", "resample", "shade", "tsdf", "cpu_baseline")


def _fake_outputs(P, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    color, invdepth = torch.rand(5, H, W, generator=g), torch.rand(1, H, W, generator=g)
    radii = torch.randint(0, 50, (P,), generator=g, dtype=torch.int32)
    grads = {k: torch.randn(P, c, generator=g) for k, c in
             (("means3D", 3), ("colors", 5), ("opacities", 1), ("scales", 3), ("rotations", 4), ("means2D", 3))}
    return color, radii, invdepth, grads


def test_dump_writes_small_outputs_whole(tmp_path):
    import bench

    color, radii, invdepth, grads = _fake_outputs(1000, 24, 40, 0)
    bench.dump_outputs(str(tmp_path), color, radii, invdepth, grads)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"color", "invdepth", "radii"} | {"grad_" + k for k in grads}
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["color"], color.numpy()) and np.array_equal(got["invdepth"], invdepth.numpy())
    assert np.array_equal(got["radii"], radii.numpy().astype(np.float32))
    for k, g in grads.items():
        assert np.array_equal(got["grad_" + k], g.numpy()), k


def test_dump_samples_large_outputs_within_64_mb(tmp_path):
    import bench

    P, H, W = bench.DUMP_ROWS + 7, 1030, 1025
    outs = _fake_outputs(P, H, W, 1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), *outs)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64e6
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert a["color"].shape == (5, bench.DUMP_PIXELS) and a["invdepth"].shape == (1, bench.DUMP_PIXELS)
    assert a["radii"].shape == (bench.DUMP_ROWS,) and a["grad_colors"].shape == (bench.DUMP_ROWS, 5)
    # the sample is fixed: the same positions in every run, in every channel, and the same rows in every array
    for f in files:
        assert np.array_equal(a[f[:-4]], np.load(tmp_path / "b" / f)), f
    # real elements, in index order: the same pixel positions across channels, the same rows across arrays
    color, _, _, grads = outs
    flat = color.reshape(5, -1).numpy()
    idx = [int(np.flatnonzero(flat[0] == v)[0]) for v in a["color"][0, :16]]
    assert np.array_equal(flat[:, idx], a["color"][:, :16]) and idx == sorted(idx)
    g = grads["means3D"].numpy()
    ridx = [int(np.flatnonzero(g[:, 0] == v)[0]) for v in a["grad_means3D"][:16, 0]]
    assert np.array_equal(g[ridx], a["grad_means3D"][:16]) and np.array_equal(grads["scales"].numpy()[ridx], a["grad_scales"][:16])


def _plain_run(dump_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--gaussians", "30000", "--size", "160", "--dump-outputs", str(dump_dir)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_and_its_dump(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    line = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "config", "host"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "views/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    assert not [k for k in FULL_ONLY if k in line], [k for k in FULL_ONLY if k in line]
    P, S = 30000, 160
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    shapes = {"color": (5, S, S), "invdepth": (1, S, S), "radii": (P,), "grad_means3D": (P, 3), "grad_means2D": (P, 3),
              "grad_colors": (P, 5), "grad_opacities": (P, 1), "grad_scales": (P, 3), "grad_rotations": (P, 4)}
    assert {k: v.shape for k, v in got.items()} == shapes
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert (got["radii"] > 0).sum() > 0 and np.abs(got["grad_means3D"]).max() > 0
    # a second run with the same arguments renders the same inputs: the same image and radii
    _plain_run(tmp_path / "b")
    for k in ("color", "invdepth", "radii"):
        assert np.array_equal(got[k], np.load(tmp_path / "b" / (k + ".npy"))), k
