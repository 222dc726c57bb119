"""Case module of the TSDF integration tests (tsdf_integrate_kernel, include/eogs_tsdf.h): scenes, the attributed
comparison, exact lattice cases and single planted non-finite pixels. DESIGN.md §8 (f4) states the rules.

Attribution. NaN voxels must coincide exactly. A voxel whose value differs from the restatement by more than the tolerance is
accepted only where the float64 restatement of some accumulated view puts it within a margin of a decision the fp32 arithmetic may
take the other way: |sdf64 + trunc| <= delta (the truncation test) or ||u64| - 1| <= delta_v or ||v64| - 1| <= delta_v (the
view test). The margins are measured on the restatement, never on the kernel: 4 x the largest |sdf32 - sdf64|, respectively
|view32 - view64|, between oracle.tsdf_oracle.sample_sdf run in fp32 and in float64 on the CPU over that view (4: the
kernel may order its sums differently from torch's GEMM). Every other outlier fails, and the accepted ones stay under the
old share, 2e-5 n + 1.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import tsdf_oracle as O

CAP = lambda n: 2e-5 * n + 1


def scene(H, W, seed, shear=0.15):
    """A near-nadir affine camera (coef ~ the reference's Nadir model, to_affine.py:244-249, plus shear) looking at a
    smooth altitude field; the volume is larger than the footprint so part of it falls outside the view."""
    g = torch.Generator().manual_seed(seed)
    coef = torch.tensor([[0.0, 0.9, 0.0], [0.9, 0.0, 0.0], [0.0, 0.0, 1.0]])
    coef[:2, 2] = shear * torch.randn(2, generator=g)
    intercept = torch.tensor([0.02, -0.03, 0.1])
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    alt = (0.15 * torch.sin(3 * xx) * torch.cos(2 * yy) + 0.05 * torch.rand((H, W), generator=g))[None, None]
    wgt = torch.rand((1, 1, H, W), generator=g).clamp(0.0, 1.0)
    wgt[..., : H // 4, : W // 4] = 0.0  # zero-weight region: 0/0 -> NaN exactly as in the reference
    return coef, intercept, alt, wgt


def _world(axes, dt):
    return torch.stack(torch.meshgrid(*[a.to(dt).cpu() for a in axes], indexing="ij"), dim=-1).reshape(-1, 3)


def reference(axes, views, scale, trunc, t0=None, w0=None):
    """views: [(coef, intercept, alt[1,1,H,W], wgt[1,1,H,W])], fp32 CPU tensors; axes: three fp32 vectors.
    -> dict: t64 / w64 and t32 / w32 (the restatement's sequence in float64 and in fp32 on the CPU), near (voxels within the
    margins of a decision in any view), margins [(delta, delta_v)] per view."""
    dims = tuple(int(a.numel()) for a in axes)
    out = {}
    near = torch.zeros(int(np.prod(dims)), dtype=torch.bool)
    per = {}
    for dt in (torch.float64, torch.float32):
        t = (torch.ones(dims) if t0 is None else t0.cpu()).to(dt)
        w = (torch.zeros(dims) if w0 is None else w0.cpu()).to(dt)
        ax = [a.to(dt).cpu() for a in axes]
        pts = _world(axes, dt)
        per[dt] = []
        for coef, intercept, alt, wgt in views:
            c, b = coef.to(dt), intercept.to(dt)
            sdf, _, _ = O.sample_sdf(pts, c, b, scale, alt.to(dt), wgt.to(dt))
            view = F.linear(pts / scale, c, b)  # sample_sdf's own first two statements
            per[dt].append((sdf, view))
            t, w = O.integrate(t, w, ax, c, b, scale, trunc, alt.to(dt), wgt.to(dt))
        out["t64" if dt == torch.float64 else "t32"] = t
        out["w64" if dt == torch.float64 else "w32"] = w
    margins = []
    for (s64, v64), (s32, v32) in zip(per[torch.float64], per[torch.float32]):
        ds = (s32.double() - s64).abs()
        ds = ds[torch.isfinite(ds)]
        delta = 4.0 * float(ds.max()) if ds.numel() else 0.0
        dv = (v32.double() - v64)[:, :2].abs()
        dv = dv[torch.isfinite(dv)]
        delta_v = 4.0 * float(dv.max()) if dv.numel() else 0.0
        margins.append((delta, delta_v))
        near |= (s64 + trunc).abs() <= delta
        near |= ((v64[:, :2].abs() - 1.0).abs() <= delta_v).any(dim=1)
    out.update(near=near.reshape(dims), margins=margins)
    return out


def outliers(a, b, tol):
    """Voxels that hold numbers in both volumes and differ by more than tol (equal infinities agree)."""
    a, b = a.double().cpu(), b.double().cpu()
    d = (a - b).abs()
    same_inf = torch.isinf(a) & torch.isinf(b) & (a == b)
    return ~torch.isnan(a) & ~torch.isnan(b) & ~same_inf & ~(d <= tol)


def assert_attributed(a, b, tol, ref, what):
    """NaN at exactly the same voxels (the restatement's own fp32 and float64 runs agree on them in every case, so no NaN is ever
    put down to a decision); every other voxel of a within tol of b, except voxels the reference run places within its margins
    of a decision, and those stay under the cap."""
    na, nb = torch.isnan(a.cpu()), torch.isnan(b.cpu())
    assert torch.equal(na, nb), f"{what}: NaN pattern differs at {torch.nonzero(na != nb)[:5].tolist()}"
    bad = outliers(a, b, tol)
    n = bad.numel()
    stray = bad & ~ref["near"]
    if bool(stray.any()):
        i = tuple(int(x) for x in torch.nonzero(stray)[0])
        raise AssertionError(f"{what}: {int(stray.sum())} of {n} voxels differ by more than {tol} away from every decision, first at {i}: "
                             f"{float(a[i])!r} against {float(b[i])!r}; margins (delta, delta_v) per view {ref['margins']}")
    assert int(bad.sum()) <= CAP(n), (f"{what}: {int(bad.sum())} of {n} voxels differ at a decision, more than the cap {CAP(n):.2f}; "
                                      f"margins {ref['margins']}")


def linspace_axes(bounds, dims):
    return [torch.linspace(float(lo), float(hi), int(n)) for (lo, hi), n in zip(bounds, dims)]


# name: (H, W, dims); three accumulated views each (seeds 1..3), the volume wider than the footprint
BOUNDS = [[-1.3, 1.25], [-1.2, 1.3], [-0.3, 0.4]]
SHAPES = {
    "image_1x1": (1, 1, (5, 6, 7)),  # W - 1 = H - 1 = 0 under align_corners=True
    "image_1x9": (1, 9, (6, 5, 9)),
    "image_9x1": (9, 1, (5, 6, 9)),
    "one_voxel": (7, 9, (1, 1, 1)),
    "nz_1": (7, 9, (9, 11, 1)),
    "nz_65": (9, 7, (5, 3, 65)),  # a column longer than a wave
    "voxels_255": (9, 9, (5, 3, 17)),
    "voxels_256": (9, 9, (4, 4, 16)),  # exactly one workgroup
    "voxels_257": (9, 9, (1, 1, 257)),
    "largest": (65, 65, (64, 64, 65)),
}
SCALE, TRUNC = 1.7, 0.15


def shape_case(name):
    H, W, dims = SHAPES[name]
    bounds = [[0.1, 0.1], [-0.2, -0.2], [0.05, 0.05]] if name == "one_voxel" else BOUNDS
    if name == "voxels_257":
        bounds = [[0.1, 0.1], [-0.2, -0.2], [-0.3, 0.4]]
    return linspace_axes(bounds, dims), [scene(H, W, seed) for seed in (1, 2, 3)]


# ---- exact lattice: every product, sum, square root and quotient is exact in fp32 -----------------------------------------
LATTICE_TRUNC = 0.25
LATTICE_SCALES = (1.0, 2.0)


def lattice_case(scale, plant=None):
    """coef = 1/2 x a permutation, dyadic intercept, axes, altitudes and trunc; 9 x 9 image (pixel pitch 1/4 in u and v), voxel
    pitch 1/8 in u and v (pixel centres and midpoints) and 1/16 in altitude; two views with weights 1 (w_new = 1, then 2).
    u = y / (2 scale) + 1/4 runs -1.25 .. 1.75, v = x / (2 scale) - 1/8 runs -1.625 .. 1.375: both hit +-1 exactly and the
    next lattice step outside. Altitudes are multiples of 1/16, so sdf = (z / scale + 1/2 - altitude) scale lands on
    -trunc, one step below it, 0 and >= trunc. The voxels one lattice step outside the view (|u| = 1.125 or |v| = 1.125) and x
    index 0 (v = -1.625) are pre-filled with NaN / -0 in the TSDF and -0 in the weights.
    plant = (what, value): one pixel of the first view's altitude or weight image replaced (row 4, column 5)."""
    s = float(scale)
    coef = torch.tensor([[0.0, 0.5, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 1.0]])
    intercept = torch.tensor([0.25, -0.125, 0.5])
    axes = [s * (-3.0 + 0.25 * torch.arange(25.0)), s * (-3.0 + 0.25 * torch.arange(25.0)), s * (-0.5 + 0.0625 * torch.arange(17.0))]
    r, c = torch.meshgrid(torch.arange(9), torch.arange(9), indexing="ij")
    views = []
    for k in range(2):
        alt = ((4 + (3 * r + 5 * c + 2 * k) % 9) / 16.0).float()[None, None]
        views.append([coef, intercept, alt, torch.ones(1, 1, 9, 9)])
    if plant is not None:
        what, value = plant
        views[0][2 if what == "altitude" else 3] = views[0][2 if what == "altitude" else 3].clone()
        views[0][2 if what == "altitude" else 3][0, 0, 4, 5] = value
    dims = (25, 25, 17)
    t0, w0 = torch.ones(dims), torch.zeros(dims)
    t0[0, ::2, :], t0[0, 1::2, :], w0[0] = float("nan"), -0.0, -0.0
    v_of_x, u_of_y = 0.5 * (axes[0] / s) - 0.125, 0.5 * (axes[1] / s) + 0.25  # exact
    for ix in torch.nonzero(v_of_x.abs() == 1.125).flatten().tolist():
        t0[ix, ::2, :], t0[ix, 1::2, :], w0[ix] = -0.0, float("nan"), -0.0
    for iy in torch.nonzero(u_of_y.abs() == 1.125).flatten().tolist():
        t0[:, iy, ::2], t0[:, iy, 1::2], w0[:, iy] = float("nan"), -0.0, -0.0
    return axes, [tuple(v) for v in views], t0, w0


PLANTS = [("altitude", float("nan")), ("altitude", float("inf")), ("altitude", float("-inf")),
          ("weight", float("nan")), ("weight", float("inf")), ("weight", -0.5), ("weight", 0.0)]


def lattice_facts(axes, view, scale):
    """float64: u, v, sdf of the first view and the voxels it updates."""
    pts = _world(axes, torch.float64)
    coef, intercept, alt, wgt = (x.double() for x in view)
    sdf, valid, _ = O.sample_sdf(pts, coef, intercept, scale, alt, wgt)
    uv = F.linear(pts / scale, coef, intercept)[:, :2]
    return uv, sdf, valid & (sdf >= -LATTICE_TRUNC)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)
