"""GPU: the end-to-end example with the random-camera loss in full (examples/train_synthetic.py --random-camera-type
rawrender_wshadow: eogs2_amd.randomcam.RandomcamRendering_Loss). Each run is a fresh child process under its own time limit: the eager
loop, the renders side by side (--parallel-renders, with the ground truth as target), and the recorded step with a drawn virtual
camera, where the compose launch follows the draw. Losses are finite and the step is recorded once."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gaussians", "20000", "--size", "128", "--iters", "8", "--random-camera", "--random-camera-type", "rawrender_wshadow"]


@functools.lru_cache(maxsize=None)
def _run(extra):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), *SMALL, *extra], capture_output=True,
                         text=True, timeout=170, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    return run.stdout


def _check(out, shared, target, recordings):
    losses = [float(m.group(1)) for m in re.finditer(r"^iter +\d+ +loss ([0-9.naninf-]+) +gaussians \d+", out, flags=re.M)]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), out[-2000:]
    m = re.search(r"^random camera: rawrender_wshadow, target (.+?), sun render (.+?); last L_new_altitude_resample (\S+) "
                  r"L_new_rgb_resample (\S+); the step was recorded (\d+) time\(s\)$", out, flags=re.M)
    assert m, out[-2000:]
    assert (m.group(1), m.group(2), int(m.group(5))) == (target, shared, recordings)
    L_alt, L_rgb = float(m.group(3)), float(m.group(4))
    assert np.isfinite(L_alt) and np.isfinite(L_rgb) and L_alt >= 0 and L_rgb > 0, m.group(0)
    return losses, (L_alt, L_rgb)


def test_eager_with_the_sun_render_shared():
    _check(_run(()), "shared", "the view itself", 0)


def test_eager_rendered_twice_starts_from_the_same_loss():
    shared = _check(_run(()), "shared", "the view itself", 0)
    twice = _check(_run(("--no-share-sun-render",)), "rendered twice", "the view itself", 0)
    # the same image either way: the first iteration's loss is the same figure (later ones follow gradients that differ in their
    # last bits: two backward passes summed against one)
    assert shared[0][0] == twice[0][0]


def test_parallel_renders_with_the_ground_truth_as_target():
    _check(_run(("--parallel-renders", "--random-camera-gt", "--sun-altitude-only")), "shared", "ground truth", 0)


def test_recorded_step_follows_the_drawn_camera_with_one_recording():
    out = _run(("--views", "3", "--graph", "--optimizer-in-graph", "--virtual-camera-extent", "0.02", "--iters", "12"))
    _check(out, "shared", "the view itself", 1)
    rows = re.findall(r"^draw +(\d+)  bg \S+ \S+ \S+  shear (\S+) (\S+)$", out, flags=re.M)
    assert len(rows) == 12 and len({r[1:] for r in rows}) > 6  # another virtual camera on every replay
