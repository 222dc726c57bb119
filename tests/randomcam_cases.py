"""Cases of the random-camera tests (eogs2_amd.randomcam, include/eogs_randomcam.h): the matrices the composition is checked
on, the host program over csrc/randomcam_compose.h (built once per session), and the fixtures of tests/golden/randomcam."""
import atexit
import functools
import glob
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "randomcam")


def ulp32(x):
    """The spacing of fp32 at |x|, elementwise."""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def shear(a, b):
    return np.array([[1, 0, a], [0, 1, b], [0, 0, 1]], dtype=np.float32)


def compose_cases():
    """[(name, cam2virt float32[3,3], camera_to_sun float32[3,3])]: shears as sample_random_camera builds them (the draw's
    extent times the altitude scale), general well-conditioned matrices, the identity."""
    g = np.random.default_rng(7)
    cases = [("identity", np.eye(3, dtype=np.float32), shear(0.37, -1.25))]
    for i, (a, b) in enumerate(((0.0, 0.0), (0.5, -0.25), (1e-3, 3e-4), (-7.0, 3.5), (0.013671875, -0.99999994), (123.456, -0.001))):
        s = shear(*g.normal(size=2)) if i % 2 else (np.eye(3) + 0.3 * g.normal(size=(3, 3))).astype(np.float32)
        cases.append((f"shear{i}", shear(a, b), s))
    for i in range(8):
        c = (np.eye(3) + 0.3 * g.normal(size=(3, 3))).astype(np.float32)
        s = (np.eye(3) + 0.5 * g.normal(size=(3, 3))).astype(np.float32)
        assert np.linalg.cond(c.astype(np.float64)) < 50.0
        cases.append((f"general{i}", c, s))
    return cases


SINGULAR = (
    ("zero", np.zeros((3, 3), dtype=np.float32)),
    ("equal_rows", np.array([[1, 2, 3], [1, 2, 3], [0, 1, 0]], dtype=np.float32)),
    ("zero_column", np.array([[1, 0, 3], [4, 0, 6], [7, 0, 9]], dtype=np.float32)),
    ("nan", np.array([[1, 0, np.nan], [0, 1, 0], [0, 0, 1]], dtype=np.float32)),
    ("inf", np.array([[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)),
)


def compose_float64(c, s):
    """(inv(C) @ S, inv(C) @ S @ C) in numpy's float64 over the float32 inputs."""
    C, S = c.astype(np.float64), s.astype(np.float64)
    V = np.linalg.inv(C) @ S
    return V, V @ C


@functools.lru_cache(maxsize=None)
def _host_exe():
    """Builds tests/randomcam_compose_host.cpp with the host compiler under AddressSanitizer and UBSan (nothing is preloaded:
    the program has its own main) and -ffp-contract=off, as the library is built. (directory, executable, how it was built)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    tmp = tempfile.mkdtemp(prefix="randomcam_compose_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "randomcam_compose_host")
    base = [cxx, "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "eogs2_amd", "csrc"),
            os.path.join(ROOT, "tests", "randomcam_compose_host.cpp"), "-o", exe]
    built = "sanitized"
    build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if build.returncode != 0:  # a compiler without the sanitizers' runtimes: the plain program computes the same
        built = "plain"
        build = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    return tmp, exe, built


def host_build():
    """"sanitized" or "plain": how the host program of this session was built."""
    return _host_exe()[2]


def host_compose(pairs):
    """[(virt_to_sun float32[3,3], K float32[3,3])] of the host program for [(cam2virt, camera_to_sun)]."""
    tmp, exe, _ = _host_exe()
    path = os.path.join(tmp, "cases.txt")
    with open(path, "w") as f:
        for c, s in pairs:
            words = np.concatenate([np.ascontiguousarray(c, dtype=np.float32).reshape(-1), np.ascontiguousarray(s, dtype=np.float32).reshape(-1)])
            f.write(" ".join(f"{w:08x}" for w in words.view(np.uint32)) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    outs = []
    for line in run.stdout.splitlines():
        if line.startswith("OUT "):
            o = np.array([int(x, 16) for x in line.split()[1:]], dtype=np.uint32).view(np.float32)
            outs.append((o[:9].reshape(3, 3).copy(), o[9:].reshape(3, 3).copy()))
    assert f"CASES {len(pairs)}" in run.stdout and len(outs) == len(pairs)
    return outs


def fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ---- the fixtures of tests/golden/randomcam (written by tests/golden/make_golden_randomcam.py) ----
RENDER_TYPES = ("rawrender", "rawrender_wshadow")
# kind: which camera the true camera is — cc (Conv2d(3,3,1) + shadow), exposure (3 x 4 matrix + shadow), pan_identity (a PAN camera,
# colour correction first, the identity map: 3 planes), pan_base_first (weird_pan_setup: the sigmoid map first, then a 1 -> 1 colour
# correction: 1 plane). span: the extent of the true camera's (u, v) grid; shear: cam2virt's; sun_scale: camera_to_sun's footprint
# factor (the reference's 1 / f = 0.5; 1.2 puts part of the view outside the sun camera).
SETUPS = (
    dict(name="cc_shadow", H=24, W=20, kind="cc", planes=3, span=0.9, shear=(0.05, -0.03), sun_scale=0.5, empty=False),
    dict(name="exposure", H=17, W=33, kind="exposure", planes=3, span=0.9, shear=(-0.04, 0.06), sun_scale=0.5, empty=False),
    dict(name="pan_identity", H=33, W=47, kind="pan_identity", planes=3, span=0.9, shear=(0.03, 0.05), sun_scale=0.5, empty=False),
    dict(name="pan_base_first", H=33, W=47, kind="pan_base_first", planes=1, span=0.9, shear=(-0.05, -0.04), sun_scale=0.5, empty=False),
    dict(name="outside", H=40, W=56, kind="cc", planes=3, span=1.15, shear=(0.06, -0.05), sun_scale=1.2, empty=False),
    dict(name="empty", H=8, W=8, kind="cc", planes=3, span=0.9, shear=(0.05, 0.02), sun_scale=0.5, empty=True),
    dict(name="identity", H=16, W=16, kind="cc", planes=3, span=1.0, shear=(0.0, 0.0), sun_scale=0.5, empty=False),
)
RESULT_FACTOR = 16.0  # the bound of the parity test: 16 x d32 of each array (four reused kernels in a chain and the composed matrix)


def variants():
    return [(s["name"], rt, gt) for s in SETUPS for rt in RENDER_TYPES for gt in (0, 1)]


@functools.lru_cache(maxsize=None)
def load_inputs(setup):
    return load_fixture(f"{setup}_inputs")


def load_results(setup, render_type, use_gt):
    """{name: (float64 result, d32)} of one variant; the float64 result is rebuilt from the float32 one and the stored difference."""
    z = load_fixture(f"{setup}_{render_type}_gt{int(use_gt)}")
    return {k: (z[k].astype(np.float64) + z[k + "_delta"].astype(np.float64), float(z[k + "_d32"]))
            for k in z if not k.endswith(("_delta", "_d32"))}
