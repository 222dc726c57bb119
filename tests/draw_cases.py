"""Cases of the draw tests (eogs2_amd.draw, include/eogs_draw.h): the Random123 known-answer vectors, the host program over
csrc/draw_rng.h (built once per session), the affines the camera formula is checked on, its float64 statement and the
bounds of the GPU tests with where they come from."""
import functools
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "draw")

# philox4x32-10, Random123's kat_vectors: (counter, key, output)
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)
ITERATIONS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1)  # 2^32: the carry into counter word 1
SEEDS = (0, 2 ** 64 - 1)
U = 2.0 ** -24  # fp32 unit roundoff


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def f32_bits(x):
    return struct.unpack("I", struct.pack("f", x))[0]


def ulp(x):
    """The spacing of fp32 at |x| (of the normal range)."""
    return float(np.spacing(np.float32(abs(x))))


def bits(t):
    return t.detach().contiguous().cpu().reshape(-1).view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


@functools.lru_cache(maxsize=None)
def host_program():
    """Builds tests/draw_rng_host.cpp with the host compiler under AddressSanitizer and UBSan and runs it: (stdout, how it
    was built). Nothing is preloaded: the program has its own main."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    tmp = tempfile.mkdtemp(prefix="draw_rng_host_")
    try:
        exe = os.path.join(tmp, "draw_rng_host")
        base = [cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "eogs2_amd", "csrc"), os.path.join(ROOT, "tests", "draw_rng_host.cpp"),
                "-o", exe]
        built = "sanitized"
        build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
        if build.returncode != 0:  # a compiler without the sanitizers' runtimes: the plain program checks the same properties
            built = "plain"
            build = subprocess.run(base, capture_output=True, text=True, timeout=300)
        assert build.returncode == 0, build.stderr[-3000:]
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
        return run.stdout, built
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def host_samples():
    """[(seed, iteration, slot, bg words[4], uniform bits[3], shear words[2], normal bits[2])] the host program printed."""
    out = []
    for line in host_program()[0].splitlines():
        if line.startswith("SAMPLE "):
            f = line.split()
            h = [int(x, 16) for x in f[4:]]
            out.append((int(f[1]), int(f[2]), int(f[3]), h[0:4], h[4:7], h[7:9], h[9:11]))
    return out


# ---- the camera formula ----
def affine_of(A, b):
    """The reference's storage: the 4 x 4 affine transposed, float32."""
    m = np.eye(4, dtype=np.float64)
    m[:3, :3] = A
    m[:3, 3] = b
    return np.ascontiguousarray(m.T.astype(np.float32))


def camera_inputs(kind, seed=0):
    """(affine float32[4,4], center float32[3]) of a named case: `well` — entries of order one; `utm` — intercepts of 1e6, as
    UTM-based scenes have them, and a centre of 1e5; `zero_center`."""
    g = np.random.default_rng(1000 + seed)
    A = g.normal(size=(3, 3)) * 0.5 + np.eye(3)
    A[2, 2] = 0.8 + 0.1 * seed  # (the nadir shear divides by it)
    if kind == "well":
        b, c = g.normal(size=3), g.normal(size=3)
    elif kind == "utm":
        b, c = g.normal(size=3) * 1e6, g.normal(size=3) * 1e5
    elif kind == "zero_center":
        b, c = g.normal(size=3) * 10.0, np.zeros(3)
    else:
        raise KeyError(kind)
    return affine_of(A, b), np.ascontiguousarray(c.astype(np.float32))


CAMERA_KINDS = ("well", "utm", "zero_center")


def camera_exact(affine, center, d):
    """The formula of include/eogs_draw.h in float64 over the float32 inputs: (new_A[3,3], new_b[3], the bound on new_b[i]).

    |new_b[i] - exact| <= 2 u (|b_i| + 4 |d_i| sum_j |A[2][j] c_j|): the chain s has three roundings, each at most u times the
    running sum of magnitudes, the final fma one more of the result's magnitude; doubled."""
    a = affine.astype(np.float64)
    A, b = a[:3, :3].T, a[3, :3]
    c = center.astype(np.float64)
    d = np.asarray(d, dtype=np.float64)
    new_A, new_b = A.copy(), b.copy()
    s = float(A[2] @ c)
    mag = float(np.abs(A[2] * c).sum())
    bound = np.zeros(3)
    for i in (0, 1):
        new_A[i] = A[i] + d[i] * A[2]
        new_b[i] = b[i] - d[i] * s
        bound[i] = 2 * U * (abs(b[i]) + 4 * abs(d[i]) * mag)
    return new_A, new_b, bound


def restated_matrices(affine, d, scale):
    """What must hold bit for bit whatever the shear: the copied and fixed entries of virt_affine (transposed storage; NaN
    where an entry is computed) and cam2virt's fixed entries."""
    va = np.full((4, 4), np.nan, dtype=np.float32)
    va[:, 2] = affine[:, 2]  # row 2 of A and b[2]
    va[:3, 3] = 0.0
    va[3, 3] = 1.0
    m = np.eye(3, dtype=np.float32)
    m[0, 2] = np.float32(d[0]) * np.float32(scale)
    m[1, 2] = np.float32(d[1]) * np.float32(scale)
    return va, m
