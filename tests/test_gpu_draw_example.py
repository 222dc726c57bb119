"""GPU: the end-to-end example with the per-iteration draws inside the recorded step (examples/train_synthetic.py
--random-background --virtual-camera-extent X: eogs2_amd.draw.IterationDraws after the bank's load). Each run is a fresh child
process under its own time limit. With the flags: finite losses, one recording, and the draws the run logs for every
iteration are `draws_for(seed, iteration, 0)`. Without them: the loss lines of the same command before the flags existed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import draw_cases as DC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--gaussians", "20000", "--size", "128", "--iters", "12", "--views", "3", "--graph", "--optimizer-in-graph", "--random-camera"]
EXTENT = 0.02
# what `BASE` printed at the commit before the flags existed (an MI355X; the run is deterministic: tests/test_gpu_views_example.py
# compares it bit for bit between the eager loop and the recorded step)
PARENT_LOSS_LINES = ["iter    1  loss 0.17429  gaussians 20000", "iter   12  loss 0.13318  gaussians 20000"]


def _run(extra):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), *BASE, *extra], capture_output=True,
                         text=True, timeout=170, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    return run.stdout


def _loss_lines(out):
    return [m.group(0) for m in re.finditer(r"^iter +\d+ +loss [0-9.naninf-]+ +gaussians \d+", out, flags=re.M)]


def test_draws_inside_the_recorded_step_are_the_streams():
    from eogs2_amd.draw import draws_for

    seed = 2 ** 64 - 3
    out = _run(["--virtual-camera-extent", str(EXTENT), "--random-background", "--draw-seed", str(seed)])
    losses = [float(line.split()[3]) for line in _loss_lines(out)]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), out[-2000:]
    assert re.search(r"the step was recorded 1 time\(s\)", out), out[-2000:]
    rows = re.findall(r"^draw +(\d+)  bg (\S+) (\S+) (\S+)  shear (\S+) (\S+)$", out, flags=re.M)
    assert [int(r[0]) for r in rows] == list(range(12))
    for r in rows:
        k = int(r[0])
        uniforms, normals = draws_for(seed, k, 0)  # iteration k + 1 of the run drew at index k: the schedule's cursor
        assert [DC.f32_bits(float(x)) for x in r[1:4]] == [DC.f32_bits(u) for u in uniforms], k
        for got, z in zip(r[4:6], normals):
            got = float(np.float32(float(got)))  # (nine significant digits name one fp32 value)
            want = float(np.float32(z) * np.float32(EXTENT))
            assert abs(got - want) <= DC.ulp(want) and abs(got) <= float(np.float32(EXTENT)), (k, got, want)
    assert len({r[1:4] for r in rows}) == 12 and len({r[4:6] for r in rows}) > 6  # another background, another camera


def test_without_the_flags_the_example_prints_what_it_printed():
    out = _run([])
    assert _loss_lines(out) == PARENT_LOSS_LINES, out[-2000:]
    assert "draw" not in out  # no line of the new report
