"""Cases of the report tests (eogs2_amd.report, include/eogs_report.h): seeded inputs shared by
tests/golden/make_golden_report.py and the tests, the float64 formulas and bounds they are held to, the host program over
csrc/report_cc.h (built once per session), the numpy rules of the packing modes, and the fixtures of tests/golden/report."""
import atexit
import functools
import hashlib
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "report")
C0 = np.float32(0.28209479177387814)  # utils/sh_utils.py, as the fp32 scalar both torch and the kernel multiply by
U = 2.0 ** -24  # one fp32 rounding, relative
F64_NOISE = 1e-14  # float64 evaluation noise relative to the size of a result's terms (2^-53 x the condition bound MAX_COND x a few operations)


def ulp32(x):
    """The spacing of fp32 at |x|, elementwise."""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ---- colour alignment ------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, 63, 64, 65, 4099)  # a vector tail, and more than one workgroup (4 rows per lane, 256 lanes)
NOISES = (0.05, 0.3, 1.0)
MAGNITUDES = (0.5, 3.0, 30.0)
N_CAMERAS = 5
MAX_COND = 30.0  # of the reference camera's matrix: a draw beyond it is replaced by the next (the bounds below hold for any
#                  matrix; this keeps the recorded fp32 values of the reference, which inverts in double, inside theirs)


def align_cases():
    """[dict(name, noise, mag, P, seed)]: every noise with every magnitude; the full row count on the diagonal."""
    out = []
    for i, noise in enumerate(NOISES):
        for j, mag in enumerate(MAGNITUDES):
            out.append(dict(name=f"n{i}_m{j}", noise=noise, mag=mag, P=ROW_COUNTS[-1] if i == j else 65, seed=100 + 10 * i + j))
    return out


@functools.lru_cache(maxsize=None)
def _align_inputs(noise, mag, P, seed):
    g = np.random.default_rng(seed)
    while True:
        weights = (np.eye(3) + noise * g.normal(size=(N_CAMERAS, 3, 3))).astype(np.float32)
        ref = int(g.integers(N_CAMERAS))
        if np.linalg.cond(weights[ref].astype(np.float64)) < MAX_COND:
            break
    biases = (0.1 * g.normal(size=(N_CAMERAS, 3))).astype(np.float32)
    f_dc = (mag * g.normal(size=(P, 1, 3))).astype(np.float32)
    return dict(weights=weights.reshape(N_CAMERAS, 3, 3, 1, 1), biases=biases, ref=ref, f_dc=f_dc)


def align_inputs(case):
    """weights f32[V,3,3,1,1], biases f32[V,3], ref (the reference camera's index), f_dc f32[P,1,3]; copies."""
    d = _align_inputs(case["noise"], case["mag"], case["P"], case["seed"])
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def rows_float64(f_dc, A1, b1):
    """((A1 . (f C0 + 0.5) + b1) - 0.5) / C0 in float64 over the fp32 inputs, and the bound 8 . 2^-24 . M with
    M = (sum_j |A_ij| (|f_j| C0 + 0.5) + |b_i| + 0.5) / C0: eight fp32 roundings sit on the path of an element (two in
    SH2RGB, a product and two sums in the dot product, the bias, the 0.5, the division), none on a value larger than M C0."""
    f = f_dc.reshape(-1, 3).astype(np.float64)
    A, b, c0 = A1.reshape(3, 3).astype(np.float64), b1.reshape(3).astype(np.float64), np.float64(C0)
    out = ((f * c0 + 0.5) @ A.T + b - 0.5) / c0
    M = ((np.abs(f) * c0 + 0.5) @ np.abs(A).T + np.abs(b) + 0.5) / c0
    return out.reshape(f_dc.shape), (8 * U * M).reshape(f_dc.shape)


def recompose_float64(Ai, bi, A1, b1):
    """(Ai . A1^-1, bi - Ai . A1^-1 . b1) in numpy's float64 over the fp32 inputs, and the magnitudes |Ai| |A1^-1| and
    |Ai| |A1^-1| |b1| + |bi| the reference's fp32 results are bounded by."""
    A, b = Ai.reshape(3, 3).astype(np.float64), bi.reshape(3).astype(np.float64)
    C, c = A1.reshape(3, 3).astype(np.float64), b1.reshape(3).astype(np.float64)
    inv = np.linalg.inv(C)
    R = A @ inv
    magA = np.abs(A) @ np.abs(inv)
    return R, b - R @ c, magA, magA @ np.abs(c) + np.abs(b)


SINGULAR = (
    ("zero", np.zeros((3, 3), dtype=np.float32)),
    ("equal_rows", np.array([[1, 2, 3], [1, 2, 3], [0, 1, 0]], dtype=np.float32)),
    ("zero_column", np.array([[1, 0, 3], [4, 0, 6], [7, 0, 9]], dtype=np.float32)),
    ("nan", np.array([[1, 0, np.nan], [0, 1, 0], [0, 0, 1]], dtype=np.float32)),
    ("inf", np.array([[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)),
)


@functools.lru_cache(maxsize=None)
def _host_exe():
    """Builds tests/report_cc_host.cpp with the host compiler under AddressSanitizer and UBSan (nothing is preloaded: the
    program has its own main) and -ffp-contract=off, as the library is built. (directory, executable, how it was built)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    tmp = tempfile.mkdtemp(prefix="report_cc_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "report_cc_host")
    base = [cxx, "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "eogs2_amd", "csrc"),
            os.path.join(ROOT, "tests", "report_cc_host.cpp"), "-o", exe]
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


def host_recompose(cases):
    """[(Ai' f32[3,3], bi' f32[3])] of the host program for [(Ai, bi, A1, b1)]."""
    tmp, exe, _ = _host_exe()
    path = os.path.join(tmp, "cases.txt")
    with open(path, "w") as f:
        for parts in cases:
            words = np.concatenate([np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in parts])
            assert words.size == 24
            f.write(" ".join(f"{w:08x}" for w in words.view(np.uint32)) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    outs = []
    for line in run.stdout.splitlines():
        if line.startswith("OUT "):
            o = np.array([int(x, 16) for x in line.split()[1:]], dtype=np.uint32).view(np.float32)
            outs.append((o[:9].reshape(3, 3).copy(), o[9:].copy()))
    assert f"CASES {len(cases)}" in run.stdout and len(outs) == len(cases)
    return outs


# ---- train -> test colour correction ------------------------------------------------------------------------------------------
def convert_inputs():
    """Per camera list ("msi", "pan"): train weights f32[V,3,3,1,1], biases f32[V,3], the reference camera's index, and the
    test cameras' starting values."""
    g = np.random.default_rng(77)
    out = {}
    for kind, V, T in (("msi", 7, 3), ("pan", 7, 3)):
        out[kind] = dict(weights=(np.eye(3) + 0.3 * g.normal(size=(V, 3, 3))).astype(np.float32).reshape(V, 3, 3, 1, 1),
                         biases=(0.1 * g.normal(size=(V, 3))).astype(np.float32),
                         test_weights=g.normal(size=(T, 3, 3, 1, 1)).astype(np.float32), test_biases=g.normal(size=(T, 3)).astype(np.float32))
        out[kind]["biases"][2, 1] = np.float32(-0.0)  # a signed zero: "ref" keeps it, "average" adds it to +0
    out["ref"] = 4
    return out


# ---- report metrics -----------------------------------------------------------------------------------------------------------
# 1 x 257 x 256: 65 792 pixels, 257 workgroups of 256 lanes, and the last pass (256 lanes over the partials) takes a second round
METRIC_SHAPES = ((1, 1, 1), (3, 7, 5), (1, 33, 65), (4, 64, 64), (1, 257, 256))
METRIC_CONTENTS = ("random", "gt_outside", "equal", "nan")


def metric_cases():
    return [(s, c) for s in METRIC_SHAPES for c in METRIC_CONTENTS]


def metric_name(shape, content):
    return "x".join(str(v) for v in shape) + "_" + content


@functools.lru_cache(maxsize=None)
def _metric_inputs(shape, content):
    g = np.random.default_rng(1000 * METRIC_SHAPES.index(shape) + METRIC_CONTENTS.index(content))
    image = g.uniform(0.0, 1.0, size=shape).astype(np.float32)
    gt = np.clip(image + 0.1 * g.normal(size=shape), 0.0, 1.0).astype(np.float32)
    if content == "gt_outside":
        gt = (image + 0.8 * g.normal(size=shape)).astype(np.float32)  # many values below 0 and above 1
        gt.reshape(-1)[0] = np.float32(1.75)
    elif content == "equal":
        image = gt.copy()  # (gt is already inside [0, 1]: the clamp changes nothing, every plane's error is 0)
    elif content == "nan":
        image.reshape(-1)[image.size // 2] = np.nan
    return image, gt


def metric_inputs(shape, content):
    image, gt = _metric_inputs(tuple(shape), content)
    return image.copy(), gt.copy()


def metrics_float64(image, gt):
    """(L1, PSNR) of one view in float64 over the fp32 inputs: train_pan.py:917,942-943."""
    d = image.astype(np.float64) - np.clip(gt, np.float32(0), np.float32(1)).astype(np.float64)
    l1 = np.abs(d).mean()
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = (d * d).reshape(d.shape[0], -1).mean(axis=1)
        psnr = (20.0 * np.log10(1.0 / np.sqrt(mse))).mean()
    return l1, psnr


def close_or_same(a, b, tol):
    """|a - b| <= tol, or both the same infinity, or both NaN."""
    a, b = float(a), float(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= tol


# ---- product packing -----------------------------------------------------------------------------------------------------------
def decision_values():
    """fp32 values on the decisions of the 8-bit modes: k / 255 and (k +- 0.5) / 255 with one ulp either side, 0, -0, 1,
    values below 0 and above 1, +-inf and NaN."""
    k = np.arange(256, dtype=np.float64)
    base = np.concatenate([k / 255.0, (k + 0.5) / 255.0, (k - 0.5) / 255.0]).astype(np.float32)
    vals = np.concatenate([base, np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf)),
                           np.array([0.0, -0.0, 1.0, -0.25, -1e-30, -3.0, 1.0000001, 1.5, 300.0, np.inf, -np.inf, np.nan], dtype=np.float32)])
    return vals.astype(np.float32)


def pack_source(shape, seed):
    """An fp32 image of `shape`: the decision values from a seeded start, cyclically, then shuffled with random values in
    [-0.2, 1.2] for every third element."""
    g = np.random.default_rng(seed)
    vals = decision_values()
    n = int(np.prod(shape))
    start = int(g.integers(vals.size))
    x = vals[(start + np.arange(n)) % vals.size].copy()
    third = np.arange(n) % 3 == 2
    x[third] = g.uniform(-0.2, 1.2, size=int(third.sum())).astype(np.float32)
    if n > 8:
        g.shuffle(x)
    return x.reshape(shape)


def u8_round(x):
    """trunc(clamp(x 255 + 0.5, 0, 255)) in fp32; a NaN gives 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = x.astype(np.float32) * np.float32(255.0) + np.float32(0.5)
        t = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(255)))
    return np.trunc(t).astype(np.uint8)


def u8_trunc(x):
    """trunc(clip(x, 0, 1) 255) in fp32; a NaN gives 0."""
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(x), np.float32(0), np.clip(x.astype(np.float32), np.float32(0), np.float32(1)))
        t = c.astype(np.float32) * np.float32(255.0)
    return np.trunc(t).astype(np.uint8)


def premap(x, lo, hi):
    """(x - lo) / (hi - lo) as torch computes it for an fp32 tensor and Python floats: both scalars rounded to fp32."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return ((x.astype(np.float32) - np.float32(lo)) / np.float32(hi - lo)).astype(np.float32)


def expected_item(src, mode, reverse=False, replicate=False, pre=None):
    """The (H, W, channels) array an item writes, by numpy."""
    x = src[None] if src.ndim == 2 else src
    if pre is not None:
        x = premap(x, *pre)
    if replicate:
        x = np.repeat(x, 3, axis=0)
    elif reverse:
        x = x[::-1]
    hwc = np.ascontiguousarray(np.transpose(x, (1, 2, 0)))
    return {"float": lambda a: a, "u8_round": u8_round, "u8_trunc": u8_trunc}[mode](hwc)


# ---- the chain: a scene, three viewpoints with an MSI and a PAN camera each ----------------------------------------------------
def make_pipe():
    import types

    return types.SimpleNamespace(debug=False, antialiasing=False, compute_cov3D_python=False, require_radii=False)


def make_viewpoints(device, n=3, H=48, W=64):
    """Duck-typed viewpoints with what renderer.py, renderer_cc_shadow.py, render_pipeline, training_report and render_set read:
    an MSI camera (three planes, eogs2_amd.shade.render_pipeline) and a PAN camera (one plane through the "average" map,
    eogs2_amd.pan.render_pipeline) per viewpoint, each with a sun camera at twice and a nadir camera at its own size, a
    ground truth that leaves [0, 1] in places, and altitude bounds the background does not start with."""
    import types

    import torch

    from eogs2_amd.pan import PanMap, render_pipeline as pan_pipeline
    from eogs2_amd.shade import render_pipeline
    from eogs2_amd.synthetic import ALT_SCALE, make_camera

    def bare(h, w, seed):
        c = types.SimpleNamespace(FoVx=1.0, FoVy=1.0, learn_wv_only_lastparam=False, image_height=h, image_width=w,
                                  camera_center=torch.zeros(3, device=device), image_name=f"view_{seed}")
        c.affine = c.world_view_transform = c.full_proj_transform = make_camera(h, w, seed=seed, device=device)
        return c

    g = torch.Generator().manual_seed(11)
    views = []
    for v in range(n):
        cams = {}
        for k, kind in enumerate(("msi", "pan")):
            c = bare(H, W, 60 + 2 * v + k)
            c.image_type = kind
            c.altitude_bounds = torch.tensor([-9.0 - v - 0.5 * k, 40.0], device=device)
            c.UV_grid = torch.meshgrid(torch.linspace(-1, 1, W, device=device), torch.linspace(-1, 1, H, device=device), indexing="xy")
            for name, (h2, w2), seed in (("sun", (2 * H, 2 * W), 80), ("nadir", (H, W), 90)):
                other = bare(h2, w2, seed + 2 * v + k)
                m = torch.eye(3, device=device)
                m[:2, 2] = (other.affine[2, :2] - c.affine[2, :2]) / ALT_SCALE
                setattr(c, f"get_{name}_camera", lambda other=other, m=m: (other, m))
            c.use_cc, c.use_exposure, c.use_shadow = True, False, True
            c.color_correction = torch.nn.Conv2d(3, 3, 1, bias=True).to(device)
            with torch.no_grad():
                c.color_correction.weight.copy_((torch.eye(3) + 0.1 * torch.randn(3, 3, generator=g)).reshape(3, 3, 1, 1))
                c.color_correction.bias.copy_(0.02 * torch.randn(3, generator=g))
            c.inshadow_color_correction = torch.full((3, 1, 1), 0.05, device=device)
            planes = 3
            if kind == "pan":
                c.msi_to_pan, c.weird_pan_setup, planes = PanMap("average"), False, 1
                c.render_pipeline = lambda raw_render, sun_altitude_diff=None, c=c: pan_pipeline(c, raw_render, sun_altitude_diff)
            else:
                c.render_pipeline = lambda raw_render, sun_altitude_diff=None, c=c: render_pipeline(c, raw_render, sun_altitude_diff)
            c.original_image = (0.5 + 0.4 * torch.randn(planes, H, W, generator=g)).to(device)
            cams[kind] = c
        views.append(types.SimpleNamespace(image_name=f"viewpoint_{v}", is_reference_camera=(v == 1), get_msi_cameras=lambda c=cams["msi"]: c,
                                           get_pan_cameras=lambda c=cams["pan"]: c))
    return views
