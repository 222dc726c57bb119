"""GPU (MI355X): the TSDF stages around integrate (include/eogs_tsdf.h: eogs_tsdf_normals / _prior / _surface;
eogs2_amd/tsdf.py: RangeImage, TSDFVolume.apply_prior / surface / surface_cloud) against the vectors the reference's own
tsdf.py produced (tests/golden/tsdf_post/, pinned on the CPU by tests/test_tsdf_post_oracle.py) and against the
restatement of its statements (tests/tsdf_post_cases.py) run on the GPU at full size: 1024^2 images, 512 x 512 x 160
volumes. The prior and the surface are comparisons and constant stores: bit for bit. The normals are fp32 arithmetic in
another order: within 2e-5 of the reference's fp32 vectors, and no further from float64 than the reference's fp32 op
sequence is, except at near-ties of a branch comparison where the kernel took the other branch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tsdf_post_cases as P
from util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

POST_DIR = os.path.join(GOLDEN_DIR, "tsdf_post")
TIE_RTOL = 1e-4   # a branch comparison within this relative distance of a tie (float64) may go either way
TIE_SHARE = 1e-3  # ... in at most this share of the pixels


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def load(name):
    z = np.load(os.path.join(POST_DIR, f"{name}.npz"))
    return {k: z[k] for k in z.files}


def bits(a, b):
    """Equal bit for bit, NaN pattern included."""
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def meta(coef, intercept, scale=1.0, name="view"):
    return {"img": name, "model": {"scale": scale, "coef_": np.asarray(coef).tolist(), "intercept_": np.asarray(intercept).tolist()}}


def scene(H, W, seed, shear=0.2):
    """A near-nadir affine camera over a smooth altitude field with noise, a cliff and a NaN pixel."""
    g = torch.Generator().manual_seed(seed)
    coef = torch.tensor([[0.0, 0.9, 0.0], [0.9, 0.0, 0.0], [0.0, 0.0, 1.0]])
    coef[:2, 2] = shear * torch.randn(2, generator=g)
    intercept = torch.tensor([0.02, -0.03, 0.1]) + 0.01 * torch.randn(3, generator=g)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    alt = 0.15 * torch.sin(3 * xx + 0.3 * seed) * torch.cos(2 * yy) + 0.002 * torch.rand((H, W), generator=g)
    alt[:, W // 2:] += 0.12
    alt[H // 3, W // 5] = float("nan")
    return coef, intercept, alt


def outside_accepted(hip_n, hip_a, bad, alt64, coef64, b64, tol):
    """Pixels outside the bound (`bad`, [H, W]) are accepted only where the float64 left / right comparison of one axis is
    within TIE_RTOL of a tie and the kernel matches float64 with that axis' other branch. Returns the accepted count."""
    win = P.windows(P.world_positions(alt64, coef64, b64))
    el_x, er_x, el_y, er_y = P.branch_errors(win)
    lx, ly = el_x < er_x, el_y < er_y
    tie = lambda l, r: (l - r).abs() <= TIE_RTOL * torch.maximum(l, r)
    ok = torch.zeros_like(bad)
    for flip_x, near in ((True, tie(el_x, er_x)[0]), (False, tie(el_y, er_y)[0])):
        _, n_f, a_f, _ = P.reconstruct(alt64, coef64, b64, left_x=~lx if flip_x else lx, left_y=ly if flip_x else ~ly)
        close = ((hip_n.double() - n_f).abs().amax(dim=1)[0] <= tol) & ((hip_a.double() - a_f).abs()[0, 0] <= tol)
        ok |= near & close
    assert bool((ok | ~bad).all()), f"{int((bad & ~ok).sum())} pixels outside the bound and not at a near-tie"
    return int(bad.sum())


def test_normals_match_reference_vectors(dev):
    from eogs2_amd.tsdf import RangeImage, RangeImageEOGS

    assert RangeImageEOGS is RangeImage
    c = load("normals")
    total = accepted = 0
    for i in range(int(c["n_cases"])):
        alt = c[f"c{i}_altitude"]
        ri = RangeImage(meta(c[f"c{i}_coef"], c[f"c{i}_intercept"], name=f"n{i}"), alt, device=dev)
        H, W = alt.shape
        assert (ri.height, ri.width, ri.img_name, ri.model_scale) == (H, W, f"n{i}", 1.0)
        assert ri.altitude_img.shape == (1, 1, H, W) and ri.pixels_normals.shape == (1, 3, H, W)
        assert ri.pixels_angle.shape == (1, 1, H, W) and ri.get_weights().shape == (1, 1, H, W)
        assert float((ri.view_direction.cpu() - torch.as_tensor(c[f"c{i}_view_direction"])).abs().max()) <= 1e-6
        n, a = ri.pixels_normals.cpu(), ri.pixels_angle.cpu()
        rn, ra = torch.as_tensor(c[f"c{i}_pixels_normals"]), torch.as_tensor(c[f"c{i}_pixels_angle"])
        assert torch.equal(torch.isnan(n), torch.isnan(rn)) and torch.equal(torch.isnan(a), torch.isnan(ra)), f"case {i}: NaN"
        bad = ((n - rn).abs().amax(dim=1)[0] > 2e-5) | ((a - ra).abs()[0, 0] > 2e-5)  # NaN compares False
        t64 = lambda k: torch.as_tensor(c[f"c{i}_{k}"]).double()
        accepted += outside_accepted(n, a, bad, t64("altitude"), t64("coef"), t64("intercept"), 2e-5)
        total += H * W
        w = ri.get_weights().cpu()
        assert bits(w, a.clamp(0.0, 1.0)), f"case {i}: weights are not clamp(angle, 0, 1)"
        rw = torch.as_tensor(c[f"c{i}_weights"])
        assert torch.equal(torch.isnan(w), torch.isnan(rw))
    assert accepted <= TIE_SHARE * total, f"{accepted} near-tie pixels of {total}"


def test_normals_full_size_against_float64(dev):
    """1024^2: |hip - f64| <= 2 |torch32 - f64| + 1e-5 per normal component and on the angle, near-ties aside."""
    from eogs2_amd.tsdf import RangeImage

    coef, intercept, alt = scene(1024, 1024, 3)
    ri = RangeImage(meta(coef, intercept), alt.to(dev))
    _, n32, a32, _ = P.reconstruct(alt.to(dev), coef.to(dev), intercept.to(dev))
    a64_, c64, b64 = alt.double().to(dev), coef.double().to(dev), intercept.double().to(dev)
    _, n64, a64, _ = P.reconstruct(a64_, c64, b64)
    n, a = ri.pixels_normals, ri.pixels_angle
    assert torch.equal(torch.isnan(n), torch.isnan(n64)) and torch.equal(torch.isnan(a), torch.isnan(a64))
    assert int(torch.isnan(a).sum()) > 0  # the NaN pixel's neighbourhood
    bound = lambda h, f32, f64: (h.double() - f64).abs() > 2 * (f32.double() - f64).abs() + 1e-5
    bad = bound(n, n32, n64).any(dim=1)[0] | bound(a, a32, a64)[0, 0]
    accepted = outside_accepted(n, a, bad, a64_, c64, b64, 2e-5)
    assert accepted <= TIE_SHARE * alt.numel(), f"{accepted} near-tie pixels"
    assert bits(ri.get_weights(), a.clamp(0.0, 1.0))


def test_prior_matches_reference_vectors(dev):
    from eogs2_amd.tsdf import apply_prior

    c = load("prior_built")
    for i in range(int(c["n_cases"])):
        t, w = torch.as_tensor(c[f"c{i}_tsdf_before"]).to(dev), torch.as_tensor(c[f"c{i}_weight_before"]).to(dev)
        apply_prior(t, w)
        assert bits(t, c[f"c{i}_tsdf_after"]) and bits(w, c[f"c{i}_weight_after"]), f"case {i}"


def test_surface_matches_reference_vectors(dev):
    from eogs2_amd.tsdf import TSDFVolume, surface

    c = load("surface_built")
    for i in range(int(c["n_cases"])):
        t, az = torch.as_tensor(c[f"c{i}_tsdf"]).to(dev), torch.as_tensor(c[f"c{i}_axis2"]).to(dev)
        idx, h = surface(t, az)
        assert idx.dtype == torch.int64 and bits(idx, c[f"c{i}_indices"]), f"case {i}: indices"
        assert bits(h, az.cpu()[torch.as_tensor(c[f"c{i}_indices"])]), f"case {i}: heights"
        vol = TSDFVolume.__new__(TSDFVolume)  # the stored axes and volume in place of the constructor's
        vol.axes = [torch.as_tensor(c[f"c{i}_axis{k}"]).to(dev) for k in range(3)]
        vol._tsdf_vol = t
        cloud = vol.surface_cloud([c[f"c{i}_center"], 1.0, 17, "T"])
        assert cloud.dtype == np.float64 and np.array_equal(cloud, c[f"c{i}_cloud"]), f"case {i}: cloud"


def random_volume(dims, seed, dev):
    """A volume with every state of the prior: sparse occupancy, NaN, t == 0 and -0, t == 1 with and without weight."""
    g = torch.Generator(device=dev).manual_seed(seed)
    vals = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 0.6, -0.3, -1.0, 0.0, -0.0, float("nan")], device=dev)
    t = vals[torch.randint(0, len(vals), dims, generator=g, device=dev)]
    w = torch.where(torch.rand(dims, generator=g, device=dev) < 0.6, 0.0, 0.5)
    return t, w


def test_prior_and_surface_full_size_against_restatement(dev):
    """512 x 512 x 160 voxels: bit for bit against the restatement's torch ops on the same GPU."""
    from eogs2_amd.tsdf import apply_prior, surface

    dims = (512, 512, 160)
    t, w = random_volume(dims, 5, dev)
    tr, wr = P.apply_prior(t, w)
    assert int((tr != t).sum()) > 1000
    apply_prior(t, w)
    assert bits(t, tr) and bits(w, wr)
    az = torch.linspace(-3.0, 12.0, dims[2], device=dev)
    idx, h = surface(t, az)
    ri, rh = P.surface(t, az)
    assert bits(idx, ri) and bits(h, rh)
    t2, _ = random_volume(dims, 6, dev)
    t2[t2 < 0] = 1.0  # no voxel below zero, except in a few columns
    t2[7, 9, 0] = t2[100, 3, 159] = t2[511, 511, 63] = t2[511, 511, 64] = -2.0
    idx, h = surface(t2, az)
    ri, rh = P.surface(t2, az)
    assert bits(idx, ri) and bits(h, rh) and int(idx[511, 511]) == 64 and int(idx[100, 3]) == 159


def test_chain_matches_reference(dev):
    """The fixture views through RangeImage -> integrate -> apply_prior -> surface_cloud against the reference's chain."""
    from eogs2_amd.tsdf import RangeImage, TSDFVolume

    c = load("chain_48x64")
    scale = float(c["model_scale"])
    vol = TSDFVolume(c["vol_bounds"], float(c["vox_size"]), float(c["trunc_margin_fact"]), device=dev)
    for v in range(int(c["n_views"])):
        ri = RangeImage(meta(c[f"v{v}_coef"], c[f"v{v}_intercept"], scale, f"view{v}"), c[f"v{v}_altitude"], device=dev)
        vol.integrate(ri)
    n = vol._tsdf_vol.numel()

    def close(a, b, what):  # integrate's tolerance (tests/test_gpu_tsdf.py)
        a, b = a.double().cpu(), torch.as_tensor(b).double()
        assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN pattern differs"
        bad = (a - b).abs() > 2e-5  # NaN compares False
        assert int(bad.sum()) <= 2e-5 * n + 1, f"{what}: {int(bad.sum())} voxels"

    close(vol._tsdf_vol, c["tsdf_integrated"], "integrated tsdf")
    close(vol._weight_vol, c["weight_integrated"], "integrated weights")
    vol.apply_prior()
    close(vol._tsdf_vol, c["tsdf_prior"], "tsdf after the prior")
    close(vol._weight_vol, c["weight_prior"], "weights after the prior")
    idx, _ = vol.surface()
    ref_idx = torch.as_tensor(c["indices"])
    d = (idx.cpu() - ref_idx).abs()
    t_ref = torch.as_tensor(c["tsdf_prior"])
    moved = d > 0
    assert int(d.max()) <= 1 and int(moved.sum()) <= 1e-3 * d.numel() + 1, f"{int(moved.sum())} columns moved"
    for x, y in moved.nonzero().tolist():
        assert abs(float(t_ref[x, y, int(ref_idx[x, y])])) <= 1e-4 or abs(float(t_ref[x, y, int(idx[x, y])])) <= 1e-4
    cloud = vol.surface_cloud([c["center"], scale, 17, "T"])
    assert cloud.dtype == np.float64 and cloud.shape == c["cloud"].shape
    keep = ~moved.reshape(-1).numpy()
    assert np.array_equal(cloud[keep], c["cloud"][keep])
    assert np.array_equal(cloud[:, :2], c["cloud"][:, :2])


def test_determinism_and_workspace(dev):
    from eogs2_amd import _lib
    from eogs2_amd.tsdf import RangeImage, apply_prior, surface

    coef, intercept, alt = scene(1024, 1024, 8)
    r1, r2 = RangeImage(meta(coef, intercept), alt.to(dev)), RangeImage(meta(coef, intercept), alt.to(dev))
    assert bits(r1.pixels_normals, r2.pixels_normals) and bits(r1.pixels_angle, r2.pixels_angle)
    dims = (300, 257, 130)
    t, w = random_volume(dims, 9, dev)
    t2, w2 = t.clone(), w.clone()
    apply_prior(t, w)
    apply_prior(t2, w2)
    assert bits(t, t2) and bits(w, w2)
    az = torch.arange(dims[2], dtype=torch.float32, device=dev)
    assert all(bits(a, b) for a, b in zip(surface(t, az), surface(t, az)))
    abi = _lib.get()
    nb = ctypes.c_size_t()
    for nx, ny, nz in ((512, 512, 160), (1, 1, 1), (3, 5, 7), (300, 257, 130)):
        abi.check(abi.tsdf_prior_bytes(nx, ny, nz, ctypes.byref(nb)))
        assert nx * ny * nz + 4 * nx * ny <= nb.value <= nx * ny * nz + 4 * nx * ny + 256


def test_error_codes(dev):
    from eogs2_amd import _lib

    abi = _lib.get()
    nb = ctypes.c_size_t()
    dims = (4, 5, 6)
    t, w = torch.ones(dims, device=dev), torch.zeros(dims, device=dev)
    abi.check(abi.tsdf_prior_bytes(*dims, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert abi.tsdf_prior_bytes(-1, 5, 6, ctypes.byref(nb)) == -1
    assert abi.tsdf_prior_bytes(4, 5, 6, None) == -1
    assert abi.tsdf_prior_bytes(1 << 14, 1 << 14, 1 << 13, ctypes.byref(nb)) == -5
    assert abi.tsdf_prior(4, 5, 6, None, p(w), p(ws), nb.value, s) == -1
    assert abi.tsdf_prior(4, 5, 6, p(t), p(w), None, nb.value, s) == -1
    assert abi.tsdf_prior(4, -5, 6, p(t), p(w), p(ws), nb.value, s) == -1
    assert abi.tsdf_prior(4, 5, 6, p(t), p(w), p(ws), nb.value - 1, s) == -3
    assert b"workspace" in abi.cdll.eogs_rast_last_error()
    assert abi.tsdf_prior(1 << 14, 1 << 14, 1 << 13, p(t), p(w), p(ws), nb.value, s) == -5
    assert abi.tsdf_prior(0, 5, 6, None, None, None, 0, s) == 0  # an empty volume: nothing to do
    az = torch.zeros(6, device=dev)
    idx = torch.empty((4, 5), dtype=torch.int64, device=dev)
    assert abi.tsdf_surface(4, 5, 0, p(t), p(az), p(idx), None, s) == -1
    assert abi.tsdf_surface(4, 5, 6, None, p(az), p(idx), None, s) == -1
    assert abi.tsdf_surface(4, 5, 6, p(t), None, p(idx), None, s) == -1
    assert abi.tsdf_surface(4, 5, 6, p(t), p(az), None, None, s) == -1
    assert abi.tsdf_surface(1 << 14, 1 << 14, 1 << 13, p(t), p(az), p(idx), None, s) == -5
    img = torch.zeros((8, 9), device=dev)
    aff, vd = torch.zeros(24, device=dev), torch.zeros(3, device=dev)
    assert abi.tsdf_normals(0, 9, p(img), p(aff), p(vd), None, p(img), None, s) == -1
    assert abi.tsdf_normals(8, 9, None, p(aff), p(vd), None, p(img), None, s) == -1
    assert abi.tsdf_normals(8, 9, p(img), p(aff), None, None, p(img), None, s) == -1
    assert abi.tsdf_normals(8, 9, p(img), p(aff), p(vd), None, None, None, s) == -1
    torch.cuda.synchronize(dev)
    assert torch.equal(t, torch.ones_like(t)) and float(w.abs().max()) == 0.0
