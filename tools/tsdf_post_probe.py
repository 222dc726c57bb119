"""The TSDF stages around integrate on one GPU: the reference's op sequence (src/gaussiansplatting/tsdf.py, restated with
torch on the same device, as bench.py's tsdf_bench does for integrate) against the native stages of include/eogs_tsdf.h.

    python tools/tsdf_post_probe.py [--out profiles/tsdf_post_probe.json] [--views 20] [--size 1024] [--dims 512 512 160]

Workload: 20 altitude views of 1024^2 fused into a 512 x 512 x 160 volume, a JAX-sized area at the shipped vox_size 0.5
(an estimate of the area, not taken from data). Per stage:
  weights   per view: view_direction + reconstruct_normals + get_weights (tsdf.py:213-231, 243-323) against RangeImage
  prior     TSDFVolume.apply_prior (tsdf.py:602-638, with its np.indices on the host and its conv3d) against apply_prior()
  surface   extract_dsm up to the cloud (tsdf.py:530-556) against TSDFVolume.surface_cloud()
it reports ms per call (host clock around synchronised calls, median of windows), the peak device memory the call adds
(torch's allocator), and for the native kernels their own time (the library's profile slots) with the algorithmic bytes
over that time against the 8 TB/s peak. The volume the prior and the surface see is the 20 views integrated natively.
Results are checked: prior and surface bit for bit, normals to fp32 rounding.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_post_cases as P  # noqa: E402  (the reference's reconstruct_normals / extract_dsm statements)
from eogs2_amd import _lib  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402
from eogs2_amd.tsdf import RangeImage, TSDFVolume  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s


def ref_apply_prior(t, w, dims):
    """tsdf.py:602-638 as the reference runs it (np.indices of the whole volume as int64 on the host, conv3d)."""
    dev = t.device
    untouched = (w == 0) & (t == 1.0)
    occ = t <= 0
    t[:, :, 0] = -1.0
    w[:, :, 0] = 1.0
    kernel = torch.ones((3, 3, 3), device=dev, dtype=torch.float32)
    occ_conv = F.conv3d(occ.unsqueeze(0).unsqueeze(0).float(), kernel.unsqueeze(0).unsqueeze(0), padding=1).squeeze()
    isolated = (occ_conv == 1) & occ.squeeze()
    t[isolated] = 1.0
    w[isolated] = 0.0
    idx = torch.arange(0, t.shape[-1], device=dev)
    indices = torch.argmax(occ * idx, dim=-1, keepdim=False)
    vox_idx = torch.tensor(np.indices(dims)).to(dev, torch.int64)
    mask = (vox_idx[-1, :, :, :] < indices.unsqueeze(-1)) & untouched
    t[mask] = -1.0
    w[mask] = 1.0


def timed(fn, iters, windows=3, setup=None):
    """median over windows of the mean ms per call; `setup` (untimed) runs before every call."""
    ws = []
    for _ in range(windows):
        total = 0.0
        for _ in range(iters):
            if setup is not None:
                setup()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            total += time.perf_counter() - t0
        ws.append(total / iters * 1e3)
    return float(np.median(ws))


def peak_mb(fn, setup=None):
    if setup is not None:
        setup()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def kernel_ms(abi, slot, fn, iters, setup=None):
    abi.profile_reset()
    for _ in range(iters):
        if setup is not None:
            setup()
        abi.profile_enable(1)
        fn()
        abi.profile_enable(0)
    ms, n = abi.profile()[slot]
    return ms / max(n, 1)


def views(n, H, W, seed=0):
    """Near-nadir affine cameras (the reference's Nadir coefficients plus shear) over one smooth scene with a cliff."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    out = []
    for v in range(n):
        coef = torch.tensor([[0.0, 0.9, 0.0], [0.9, 0.0, 0.0], [0.0, 0.0, 1.0]])
        coef[:2, 2] = 0.2 * torch.randn(2, generator=g)
        intercept = torch.tensor([0.02, -0.03, 0.1]) + 0.01 * torch.randn(3, generator=g)
        alt = 0.15 * torch.sin(3 * xx + 0.1 * v) * torch.cos(2 * yy) + 0.002 * torch.rand((H, W), generator=g)
        alt[:, W // 2:] += 0.12
        out.append((coef, intercept, alt))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_post_probe.json"))
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dims", type=int, nargs=3, default=(512, 512, 160))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    abi = _lib.get()
    H = W = a.size
    nx, ny, nz = a.dims
    N = nx * ny * nz
    scale, vox = 150.0, 0.5  # world metres = model units * scale; 0.5 m voxels (gs_config tsdf vox_size)
    bounds = np.array([[-0.5 * (nx - 1) * vox, 0.5 * (nx - 1) * vox], [-0.5 * (ny - 1) * vox, 0.5 * (ny - 1) * vox],
                       [-0.3 * scale, -0.3 * scale + (nz - 1) * vox]])
    bounds[:, 1] += vox / 2  # (b1 - b0) // vox + 1 == n
    vol = TSDFVolume(bounds, vox, 3.0, device=dev)
    assert tuple(vol.num_voxels_per_dimension) == (nx, ny, nz), vol.num_voxels_per_dimension
    vs = [(c.to(dev), b.to(dev), alt.to(dev)) for c, b, alt in views(a.views, H, W)]
    metas = [{"img": f"v{i}", "model": {"scale": scale, "coef_": c.tolist(), "intercept_": b.tolist()}} for i, (c, b, _) in
             enumerate(views(a.views, H, W))]
    res = {"what": f"{a.views} views of {H}x{W}, {nx}x{ny}x{nz} voxels (vox_size {vox}); reference op sequence restated with "
                   "torch on the same GPU vs the native stages", "source_hash": source_hash(), "device": torch.cuda.get_device_name(dev)}
    print(res["what"], flush=True)

    # ---- weights: per view ----
    def ref_weights():
        for c, b, alt in vs:
            P.reconstruct(alt, c, b)

    def nat_weights():
        for m, (_, _, alt) in zip(metas, vs):
            RangeImage(m, alt).get_weights()

    ref_weights(), nat_weights()  # warm-up
    st = {"ref_ms_per_view": timed(ref_weights, 1) / a.views, "native_ms_per_view": timed(nat_weights, 1) / a.views,
          "ref_peak_MB": peak_mb(lambda: P.reconstruct(*[vs[0][k] for k in (2, 0, 1)])),
          "native_peak_MB": peak_mb(lambda: RangeImage(metas[0], vs[0][2]))}
    st["native_kernel_ms"] = kernel_ms(abi, "tsdf_normals", lambda: RangeImage(metas[0], vs[0][2]), 10)
    st["algorithmic_bytes"] = 24 * H * W  # altitude read; normals, angle and weights written
    _, n32, a32, _ = P.reconstruct(vs[0][2], vs[0][0], vs[0][1])
    ri = RangeImage(metas[0], vs[0][2])
    fin = torch.isfinite(a32) & torch.isfinite(ri.pixels_angle)
    st["max_abs_diff_angle"] = float((ri.pixels_angle - a32)[fin].abs().max())
    st["pixels_beyond_2e-5"] = int(((ri.pixels_angle - a32).abs() > 2e-5).sum())
    res["weights"] = st
    print("weights", st, flush=True)

    # ---- integrate the views natively: the volume the prior and the surface see ----
    for m, (_, _, alt) in zip(metas, vs):
        vol.integrate(RangeImage(m, alt))
    t0, w0 = vol._tsdf_vol.clone(), vol._weight_vol.clone()
    t, w = vol._tsdf_vol, vol._weight_vol

    def reset():
        t.copy_(t0)
        w.copy_(w0)

    # ---- prior ----
    reset()
    ref_apply_prior(t, w, (nx, ny, nz))  # warm-up (conv3d picks its algorithm)
    tr, wr = t.clone(), w.clone()
    reset()
    vol.apply_prior()
    st = {"bit_exact": bool(torch.equal(torch.isnan(t), torch.isnan(tr)) and torch.equal(t.nan_to_num(7.0), tr.nan_to_num(7.0))
                            and torch.equal(w, wr)),
          "ref_ms": timed(lambda: ref_apply_prior(t, w, (nx, ny, nz)), 2, setup=reset),
          "native_ms": timed(vol.apply_prior, 5, setup=reset),
          "ref_peak_MB": peak_mb(lambda: ref_apply_prior(t, w, (nx, ny, nz)), setup=reset),
          "ref_host_indices_MB": 24 * N / 2**20,
          "native_peak_MB": peak_mb(vol.apply_prior, setup=reset),
          "native_kernel_ms": kernel_ms(abi, "tsdf_prior", vol.apply_prior, 5, setup=reset)}
    occ = t0 <= 0
    iso = occ & (P.occupancy_count(occ) == 1)
    top = torch.argmax(occ * torch.arange(nz, device=dev), dim=-1)
    z = torch.arange(nz, device=dev)
    stores = int((iso | (z == 0) | ((w0 == 0) & (t0 == 1.0) & (z < top[..., None]))).sum())
    st["stored_voxels"] = stores
    st["algorithmic_bytes"] = 8 * N + 2 * N + 8 * stores + 8 * nx * ny
    res["prior"] = st
    print("prior", st, flush=True)
    del tr, wr, iso, occ

    # ---- surface ----
    reset()
    vol.apply_prior()
    center = np.array([512345.25, 4321987.75, 31.5])

    def ref_surface():
        idx, zv = P.surface(t, vol.axes[2])
        return P.surface_cloud(vol.axes[:2], zv, center)

    ref_surface()
    c_ref, c_nat = ref_surface(), vol.surface_cloud([center])
    st = {"bit_exact": bool(np.array_equal(c_ref, c_nat)),
          "ref_ms": timed(ref_surface, 5), "native_ms": timed(lambda: vol.surface_cloud([center]), 5),
          "ref_kernels_ms": timed(lambda: P.surface(t, vol.axes[2]), 5), "native_kernels_ms": timed(vol.surface, 5),
          "ref_peak_MB": peak_mb(lambda: P.surface(t, vol.axes[2])), "native_peak_MB": peak_mb(vol.surface),
          "native_kernel_ms": kernel_ms(abi, "tsdf_surface", vol.surface, 5)}
    idx, _ = vol.surface()
    neg = (t < 0).any(-1)
    chunks_top = (nz + 63) // 64
    visited = torch.where(neg, chunks_top - idx // 64, torch.full_like(idx, chunks_top))
    st["algorithmic_bytes"] = int(torch.minimum(visited * 64, torch.full_like(visited, nz)).sum()) * 4 + 12 * nx * ny
    st["columns_with_surface"] = int(neg.sum())
    res["surface"] = st
    print("surface", st, flush=True)

    for k in ("weights", "prior", "surface"):
        s = res[k]
        s["native_GBps"] = s["algorithmic_bytes"] / (s["native_kernel_ms"] * 1e-3) / 1e9
        s["frac_of_8TBps"] = s["native_GBps"] / HBM_PEAK_GBS
    res["not_measured"] = ("plyflatten rasterisation and the GeoTIFF write (the caller's); integrate (bench.py tsdf); the host "
                           "time of np.indices is inside ref prior ms, its 24 B/voxel host buffer is computed, not measured")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
