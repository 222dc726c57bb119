"""GPU (MI355X): fused virtual-camera resample (include/eogs_resample.h, eogs2_amd/resample.py) against the oracle —
the reference's statements over torch.nn.functional.grid_sample in float64 (oracle/resample_oracle.py) — and against
the same statements run in fp32 by PyTorch on the GPU (what the reference executes)."""
import pytest
import torch

import resample_cases as RC
from util import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def _case(H, W, f, seed, shear=0.08, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    vr = torch.rand(5, H * f, W * f, generator=g)
    vr[3] = vr[3] * 40 - 10  # altitude-like channel
    alt = torch.rand(H, W, generator=g) * 2 - 0.5
    U, V = torch.meshgrid(torch.linspace(-1, 1, W), torch.linspace(-1, 1, H), indexing="xy")
    M = torch.eye(3)
    M[:2, 2] = torch.tensor([shear, -0.7 * shear])
    M[0, 0], M[1, 1] = 1.0 + shift, 1.0 - 0.5 * shift  # pushes part of the grid outside [-1, 1]
    w_s = torch.randn(4, H, W, generator=g)
    w_uv = torch.randn(H, W, 2, generator=g)
    return vr, alt, (U, V), M, w_s, w_uv


def _run(fn, vr, alt, UV, M, w_s, w_uv, dev):
    vr = vr.to(dev).requires_grad_(True)
    alt = alt.to(dev).requires_grad_(True)
    uva = torch.stack((UV[0].to(dev), UV[1].to(dev), alt), dim=-1)  # train_pan.py:281
    s, uv = fn(vr, M.to(dev), uva)
    ((s * w_s.to(dev)).sum() + (uv * w_uv.to(dev)).sum()).backward()
    return s.detach().cpu(), uv.detach().cpu(), vr.grad.cpu(), alt.grad.cpu()


@pytest.mark.parametrize("H,W,f,shift", [(64, 80, 2, 0.0), (33, 47, 1, 0.3), (128, 128, 2, -0.2), (17, 300, 1, 0.0)])
def test_resample_matches_oracle(dev, H, W, f, shift):
    from oracle import resample_oracle

    from eogs2_amd.resample import resample

    c = _case(H, W, f, seed=H + W, shift=shift)
    got = _run(resample, *c, dev)
    ref = _run(resample_oracle.resample, *c, torch.device("cpu"))
    if shift:
        assert int((got[0][3] == -100).sum()) > 0  # the out-of-view fill is exercised
    for name, a, b in zip(("sample", "uv", "g_virtual_render", "g_altitude"), got, ref):
        assert_close(a, b, name, rtol=1e-4, allow_flips=False)  # fp32 pixel coordinates up to 2047: weights good to ~1e-4


def test_resample_matches_reference_ops_on_gpu_full_size(dev):
    """1024^2 true camera, 2048^2 sun camera: the reference's fp32 op sequence on the same GPU."""
    from eogs2_amd.resample import resample

    ref_ops = RC.reference_resample_ops  # the reference's statements in fp32

    c = _case(1024, 1024, 2, seed=7, shift=0.05)
    got = _run(resample, *c, dev)
    ref = _run(ref_ops, *c, dev)
    for name, a, b in zip(("sample", "uv", "g_virtual_render", "g_altitude"), got, ref):
        # two fp32 evaluations (each within 1e-4 of the float64 oracle at small sizes), atomics in different orders.
        # Where a coordinate rounds onto a cell border the two pick different cells: the sample is continuous there but
        # its derivative with respect to the coordinate is not, so a few pixels in a million may differ arbitrarily.
        err = (a.double() - b.double()).abs() / b.abs().max().clamp_min(1e-30).double()
        assert float((err > 2e-4).double().mean()) <= 2e-5, f"{name}: {float(err.max()):.3e}"
    assert float(got[2][4].abs().max()) == 0.0  # the unused accumulated-opacity channel receives no gradient


def test_resample_entry_point_and_errors(dev):
    import types

    from test_fused_cpu import _Cam, _Model
    from util import raw_params_from_scene

    from eogs2_amd.resample import render_resample_virtual_camera, resample
    from eogs2_amd.synthetic import make_scene

    H, W, P = 96, 128, 3000
    scene = make_scene(P, H, W, seed=3, opacity="trained", device=dev, scale_mult=2.0)
    raw, _ = raw_params_from_scene(scene)
    cam, pc = _Cam(scene["viewmatrix"], H, W), _Model(raw)
    cam.last_row = cam.last_row.detach().to(dev)
    cam.camera_center = cam.camera_center.to(dev)
    pipe = types.SimpleNamespace(debug=False, antialiasing=False, compute_cov3D_python=False, require_radii=False)
    U, V = torch.meshgrid(torch.linspace(-1, 1, W, device=dev), torch.linspace(-1, 1, H, device=dev), indexing="xy")
    uva = torch.stack((U, V, torch.zeros(H, W, device=dev)), dim=-1)
    rgb, alt, uv = render_resample_virtual_camera(cam, torch.eye(3, device=dev), uva, pc, pipe, scene["bg"])
    assert rgb.shape == (3, H, W) and alt.shape == (H, W) and uv.shape == (H, W, 2)
    # identity reprojection onto the same grid reproduces the render itself
    from eogs2_amd.render import render

    direct = render(cam, pc, pipe, scene["bg"])["render"]
    assert_close(rgb, direct[:3], "identity resample", rtol=1e-5, allow_flips=False)
    (rgb.sum() + alt.sum()).backward()
    assert pc._xyz.grad is not None and float(pc._xyz.grad.abs().max()) > 0
    with pytest.raises(RuntimeError):
        resample(direct, torch.eye(4, device=dev), uva)
    with pytest.raises(RuntimeError):
        resample(direct, torch.eye(3, device=dev), uva[..., :2])


# ---- vectors from the REFERENCE's own render_resample_virtual_camera (tests/golden/make_golden_resample.py) ----
import glob  # noqa: E402
import os  # noqa: E402

from util import GOLDEN_DIR  # noqa: E402

RESAMPLE_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "resample_*.npz")))


@pytest.mark.parametrize("path", RESAMPLE_FIXTURES, ids=lambda p: os.path.basename(p)[9:-4])
def test_resample_matches_reference_vectors(dev, path):
    """The HIP resample (forward and backward through the C-ABI) against what the reference's function returned and what
    autograd gave for it: RGB / altitude samples with the -100 fill, coordinates, d/d virtual render, d/d altitude."""
    from test_resample_oracle import compare, load, run

    from eogs2_amd.resample import resample

    c = load(path)
    compare(run(resample, c, dev), c, rtol=1e-4)


def test_entry_point_matches_reference_vectors_with_a_stub_render(dev, monkeypatch):
    """eogs2_amd.resample.render_resample_virtual_camera (the reference's signature) with step 1 replaced by the fixture's
    virtual render, exactly as the fixture was produced."""
    from test_resample_oracle import compare, load

    import eogs2_amd.render as R
    from eogs2_amd.resample import render_resample_virtual_camera

    c = load(RESAMPLE_FIXTURES[1])
    vr = c["virtual_render"].to(dev).requires_grad_(True)
    alt = c["altitude"].to(dev).requires_grad_(True)
    monkeypatch.setattr(R, "render", lambda cam, pc, pipe, bg: {"render": vr})
    uva = torch.stack((c["U"].to(dev), c["V"].to(dev), alt), dim=-1)
    rgb, a, uv, extra = render_resample_virtual_camera(None, c["cam2virt"].to(dev), uva, None, None, None, return_extra=True)
    assert extra is vr
    ((rgb * c["w_rgb"].to(dev)).sum() + (a * c["w_alt"].to(dev)).sum() + (uv * c["w_uv"].to(dev)).sum()).backward()
    got = dict(rgb_sample=rgb.detach().cpu(), altitude_sample=a.detach().cpu(), virtual_uv=uv.detach().cpu(),
               g_virtual_render=vr.grad.cpu(), g_altitude=alt.grad.cpu())
    compare(got, c, rtol=1e-4)


def test_first_form_of_the_backward_tile_kernel_still_matches_the_oracle(dev):
    """EOGS_RESAMPLE_BWD=1 (read once per process) selects the round-2 tile kernel (LDS float atomics) instead of the bucketed
    gather: the oracle comparisons above, in a child process with it set."""
    import os
    import subprocess
    import sys

    if os.environ.get("EOGS_RESAMPLE_BWD") == "1":
        pytest.skip("already the child")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_resample.py"), "-m", "gpu", "-q", "-x",
                        "-k", "matches_oracle or matches_reference_ops"], env=dict(os.environ, EOGS_RESAMPLE_BWD="1"),
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def test_backward_is_reproducible_bit_for_bit(dev):
    """The gather sums in a fixed order (candidate tiles in tile order, a bucket's entries in pixel order): repeated backward
    passes over the same inputs give the same bits — at 1:1 and under minification, where several true-camera pixels land in one
    virtual cell and the order of the sum is visible, one plane and four."""
    from eogs2_amd.resample import resample

    for f, H, W, n_out in ((1, 300, 420, 4), (1, 300, 420, 1)):
        vr, alt, UV, M, w_s, w_uv = _case(H, W, f, seed=7, shift=0.2)
        M = M.clone()
        M[0, 0], M[1, 1] = 0.45, 0.6  # several pixels per virtual cell
        grads = []
        for _ in range(6):
            v = vr[:5 if n_out == 4 else 1].to(dev).requires_grad_(True)
            a = alt.to(dev).requires_grad_(True)
            uva = torch.stack((UV[0].to(dev), UV[1].to(dev), a), dim=-1)
            s, uv = resample(v, M.to(dev), uva, n_out=n_out, fill_channel=n_out - 1)
            ((s * w_s[:n_out].to(dev)).sum() + (uv * w_uv.to(dev)).sum()).backward()
            grads.append((v.grad.clone(), a.grad.clone()))
        assert float(grads[0][0].abs().max()) > 0
        for gv, ga in grads[1:]:
            assert torch.equal(gv, grads[0][0]) and torch.equal(ga, grads[0][1])


# ---- the edge cases of the bucketed gather (tests/resample_cases.py; the cases themselves are checked on the CPU by
# tests/test_resample_cases.py) ----
def _hip(vr, M, uva, n_out, fill_channel):
    from eogs2_amd.resample import resample

    return resample(vr, M, uva, n_out=n_out, fill_channel=fill_channel)


@pytest.mark.parametrize("name", RC.RESAMPLE)
def test_resample_case_matches_oracle(dev, name):
    """Forward and backward of every case against the float64 oracle under the rule of the case module: 1e-4 of each quantity's
    maximum, no element left out of the lattice cases, elsewhere only dL/duva of pixels on a cell border. (The name matches the
    filter of the first-form test below, whose child runs these cases through the LDS-atomic tile kernel.)"""
    c = RC.resample_case(name)
    got, ref = RC.run_resample(_hip, c, dev), RC.oracle_resample(name)
    f = c["fill_channel"]
    if f >= 0:
        assert torch.equal(got["sample"][f] == -100, ref["sample"][f] == -100), "the out-of-view fill covers different pixels"
    err = RC.compare_resample(got, ref, c, RC.TOL, name)
    print(f"{name}: " + " ".join(f"{k} {e:.2e}" for k, e in err.items()))
    assert not got["g_virtual"][c["n_out"]:].any()  # trailing channels receive zeros
    if name == "all_out":
        assert not got["g_virtual"].any() and (got["sample"][3] == -100).all() and not got["sample"][:3].any()


def _abi_backward(dev, c, g_vr, g_uva):
    """eogs_resample_backward straight through the C-ABI into the caller's buffers."""
    import ctypes

    from eogs2_amd import _lib
    from eogs2_amd._host import Ctx, ptr

    abi = _lib.get()
    (C, Hv, Wv), (H, W) = c["vr"].shape, c["alt"].shape
    vr, M = c["vr"].to(dev), c["M"].to(dev)
    uva = torch.stack((c["U"], c["V"], c["alt"]), dim=-1).to(dev)
    gs, guv = c["w_s"].to(dev), c["w_uv"].to(dev)
    with Ctx(abi, dev) as cx:
        n = ctypes.c_size_t()
        abi.check(abi.resample_bytes(H, W, ctypes.byref(n)))
        ws = torch.empty((n.value,), dtype=torch.uint8, device=dev)
        abi.check(abi.resample_backward(C, Hv, Wv, H, W, c["n_out"], ptr(vr), ptr(uva), ptr(M), c["fill_channel"], ptr(gs), ptr(guv),
                                        ptr(g_vr), ptr(g_uva), ptr(ws), ws.numel(), cx.stream))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["all_out", "big4", "one_past", RC.channel_name("minify8", 6, 5, -1), RC.channel_name("partly_out", 6, 5, -1)])
def test_backward_overwrites_every_element_of_its_outputs(dev, name):
    """dL_dvirtual and dL_duva handed over full of NaN: every element is written, channels >= n_out and every cell no tap
    reaches (from the float64 coordinates, grown by one cell) with exact zeros — also where no output tile is a candidate."""
    c = RC.resample_case(name)
    (C, Hv, Wv), (H, W) = c["vr"].shape, c["alt"].shape
    g_vr = torch.full((C, Hv, Wv), float("nan"), device=dev)
    g_uva = torch.full((H, W, 3), float("nan"), device=dev)
    _abi_backward(dev, c, g_vr, g_uva)
    g_vr, g_uva = g_vr.cpu(), g_uva.cpu()
    assert not torch.isnan(g_vr).any() and not torch.isnan(g_uva).any()
    assert not g_vr[c["n_out"]:].any()
    reached = torch.from_numpy(RC.reached_cells(*RC.tap_cells(c), Hv, Wv, dilate=1))
    assert not g_vr[:, ~reached].any()
    assert (name == "all_out") == (not reached.any())
    if name == "all_out":
        assert not g_vr.any()
    else:
        assert g_vr[:c["n_out"]].abs().amax(dim=(1, 2)).min() > 0
    ref = RC.oracle_resample(name)
    RC.compare_resample(dict(ref, g_virtual=g_vr, g_uva=g_uva), ref, c, RC.TOL, name)


@pytest.mark.parametrize("name", ["collapse_exact", "minify8", "rounds4"])
def test_case_backward_is_reproducible_bit_for_bit(dev, name):
    """Six backward passes give the same bits: a full bucket ranked by pixel id, tens of pixels per cell, two scan rounds."""
    c = RC.resample_case(name)
    runs = [RC.run_resample(_hip, c, dev) for _ in range(6)]
    assert float(runs[0]["g_virtual"].abs().max()) > 0
    for r in runs[1:]:
        assert torch.equal(r["g_virtual"], runs[0]["g_virtual"]) and torch.equal(r["g_uva"], runs[0]["g_uva"])


def test_cases_in_sequence_on_one_stream_equal_each_alone(dev):
    """The 64x32 and 32x32 tile kernels, two scan rounds and a launch without candidates queued back to back on one stream with
    no synchronisation in between (inputs uploaded beforehand): bit for bit what each case gives alone. The workspace is per
    call, the kernel form is chosen by static state."""
    names = ("big4", "one_tile", "rounds4", "all_out")

    def upload(c):
        uva = torch.stack((c["U"], c["V"], c["alt"]), dim=-1)
        return {k: t.to(dev) for k, t in dict(vr=c["vr"], uva=uva, M=c["M"], w_s=c["w_s"], w_uv=c["w_uv"]).items()}

    def go(c, d):
        vr, uva = d["vr"].clone().requires_grad_(True), d["uva"].clone().requires_grad_(True)
        s, uv = _hip(vr, d["M"], uva, c["n_out"], c["fill_channel"])
        ((s * d["w_s"]).sum() + (uv * d["w_uv"]).sum()).backward()
        return s.detach(), uv.detach(), vr.grad, uva.grad

    cases = [RC.resample_case(n) for n in names]
    on_dev = [upload(c) for c in cases]
    alone = []
    for c, d in zip(cases, on_dev):
        torch.cuda.synchronize()
        alone.append([t.cpu() for t in go(c, d)])
    torch.cuda.synchronize()
    queued = [go(c, d) for c, d in zip(cases, on_dev)]  # nothing waits for the device in here
    torch.cuda.synchronize()
    for n, a, q in zip(names, alone, queued):
        for what, x, y in zip(("sample", "uv", "g_virtual", "g_uva"), a, q):
            assert torch.equal(x, y.cpu()), f"{n}: {what} differs in sequence"
