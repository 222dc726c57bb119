"""Generates tests/golden/reg/*.npz by running the REFERENCE's own loss classes (OpacityLoss, radiiOpacityLoss,
AccumulatedOpacity of loss/opacity.py; erankLoss, Total_variation of loss/main_loss.py) on the seeded inputs of
tests/reg_cases.py, once in float32 and once in float64. Only inputs, outputs and autograd gradients are stored.

    python tests/golden/make_golden_reg.py <reference checkout>/src/gaussiansplatting

`loss/opacity.py` and `loss/main_loss.py` are loaded without executing `loss/__init__.py` (which pulls the renderer and the
dataset readers): a stub `loss` package and stub renderer modules, as make_golden_shade.py does. The classes are handed a
plain namespace with the two properties they read, `get_opacity` = sigmoid(_opacity) and `get_scaling` = exp(_scaling)
(scene/gaussian_model.py:41,50,110-111,136-137). Rows at RETIRED_LOGIT are taken out before the reference sees the model
and their gradients stored as zeros.

Keys: inputs `opacity` [P,1], `log_scales` [P,3], `radii` [P], `n_init`, `upstream` [3] (the gradient of
upstream[k] * term_k is stored); outputs `<name>@32` and `<name>@64` for the two runs.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import reg_cases as rc  # noqa: E402

OUT = os.path.join(HERE, "reg")


def load_ref(refroot):
    sys.path.insert(0, refroot)
    pkg = types.ModuleType("loss")
    pkg.__path__ = [os.path.join(refroot, "loss")]
    sys.modules["loss"] = pkg
    for name in ("gaussian_renderer", "gaussian_renderer.renderer_cc_shadow"):  # main_loss.py imports the renderer at module level
        m = types.ModuleType(name)
        m.render_resample_virtual_camera = m.render_resample_virtual_camera_wshadowmapping = None
        sys.modules.setdefault(name, m)
    return importlib.import_module("loss.opacity"), importlib.import_module("loss.main_loss")


class Model:
    def __init__(self, opacity, scaling):
        self._opacity, self._scaling = opacity, scaling

    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_scaling = property(lambda s: torch.exp(s._scaling))


def run_gauss(op_mod, ml_mod, opacity, log_scales, radii, n_init, upstream, dtype):
    alive = opacity.reshape(-1) > 0.5 * rc.RETIRED_LOGIT
    m = Model(opacity[alive].to(dtype).requires_grad_(True), log_scales[alive].to(dtype).requires_grad_(True))
    L = [op_mod.OpacityLoss(0.1, n_init)(m), op_mod.radiiOpacityLoss(0.1, n_init)(m, radii[alive]), ml_mod.erankLoss(0.1)(m)]
    g_op, = torch.autograd.grad(float(upstream[0]) * L[0], m._opacity)
    if bool((radii[alive] > 0).any()):
        g_rad, = torch.autograd.grad(float(upstream[1]) * L[1], m._opacity)
    else:
        g_rad = torch.zeros_like(g_op)  # opacity[visible] is empty: the term is 0
    g_sc, = torch.autograd.grad(float(upstream[2]) * L[2], m._scaling)

    def full(g):
        out = torch.zeros((opacity.shape[0],) + tuple(g.shape[1:]), dtype=dtype)
        out[alive] = g
        return out.numpy()

    return {"L_opacity": L[0].detach().numpy(), "L_opacity_radii": L[1].detach().numpy(), "L_erank": L[2].detach().numpy(),
            "g_opacity_op": full(g_op), "g_opacity_radii": full(g_rad), "g_scaling": full(g_sc)}


def gauss_case(mods, name, opacity, log_scales, radii, n_init, upstream):
    d = dict(opacity=opacity.numpy(), log_scales=log_scales.numpy(), radii=radii.numpy(), n_init=np.float64(n_init),
             upstream=np.asarray(upstream, np.float32))
    for tag, dtype in (("@32", torch.float32), ("@64", torch.float64)):
        for k, v in run_gauss(*mods, opacity, log_scales, radii, n_init, upstream, dtype).items():
            d[k + tag] = v
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    t = rc.gauss_bounds(opacity, log_scales, radii, n_init, upstream)["t"]
    print(name, opacity.shape[0], "rows;", float(d["L_opacity@64"]), float(d["L_opacity_radii@64"]), float(d["L_erank@64"]),
          "; clip active / inactive by more than 1e-3:", int((t > 1e-3).sum()), int((t < -1e-3).sum()), ";", os.path.getsize(path), "bytes")


def clip_equality_row():
    """A row whose fp32 run lands exactly on the clip, -log(e + 1e-5) == 0: the float32 neighbours of the crossing of a
    disk's thin axis are tried in turn (float64 bisection first)."""
    f = lambda d, dt: rc.erank_rows(torch.tensor([[0.25, -0.125, d]], dtype=dt))[1][0]  # noqa: E731
    lo, hi = -3.0, 0.0  # t(lo) > 0 (rank below 2), t(hi) < 0
    assert f(lo, torch.float64) > 0 > f(hi, torch.float64)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid, torch.float64) > 0 else (lo, mid)
    c = np.float32(lo)
    cand = [c]
    up = dn = c
    for _ in range(4096):
        up, dn = np.nextafter(up, np.float32(1)), np.nextafter(dn, np.float32(-9))
        cand += [up, dn]
    l = torch.tensor([[0.25, -0.125, float(v)] for v in cand], dtype=torch.float32)
    hit = (rc.erank_rows(l)[1] == 0).nonzero().reshape(-1)
    assert hit.numel(), "no float32 neighbour lands on the clip"
    return l[hit[0]].clone()


def image_case(mods, name, alt, acc, upstream):
    op_mod, ml_mod = mods
    d = dict(altitude=alt.numpy(), accumulated_opacity=acc.numpy(), upstream=np.asarray(upstream, np.float32))
    for tag, dtype in (("@32", torch.float32), ("@64", torch.float64)):
        a, c = alt.to(dtype).requires_grad_(True), acc.to(dtype).requires_grad_(True)
        tv = ml_mod.Total_variation(0.1)(a)
        ao = op_mod.AccumulatedOpacity(0.1)(c)
        g_a, = torch.autograd.grad(float(upstream[0]) * tv, a)
        g_c, = torch.autograd.grad(float(upstream[1]) * ao, c)
        d.update({"L_TV_altitude" + tag: tv.detach().numpy(), "L_accumulated_opacity" + tag: ao.detach().numpy(),
                  "g_altitude" + tag: g_a.numpy(), "g_accumulated_opacity" + tag: g_c.numpy()})
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print(name, tuple(alt.shape), float(d["L_TV_altitude@64"]), float(d["L_accumulated_opacity@64"]), ";", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    mods = load_ref(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    up = (0.75, -1.25, 2.5)  # (exact in float32)
    # the four populations, the row on the clip, rows parked at RETIRED_LOGIT in between
    g = torch.Generator().manual_seed(101)
    ls = torch.cat([rc.log_scales(k, 512, g) for k in ("isotropic", "two_small", "disk", "needle")] + [clip_equality_row()[None]])
    ls = ls[torch.randperm(ls.shape[0], generator=g)]
    n = ls.shape[0] + 64
    op = rc.opacity_logits(n, g)
    retired = torch.randperm(n, generator=g)[:64]
    op[retired] = rc.RETIRED_LOGIT
    full = (3.0 * torch.randn(n, 3, generator=g)).to(torch.float32)  # (whatever a retired row still holds)
    full[op.reshape(-1) > 0.5 * rc.RETIRED_LOGIT] = ls
    gauss_case(mods, "gauss_mix", op, full, rc.radii_mix(n, g), 3000, up)
    g = torch.Generator().manual_seed(102)
    gauss_case(mods, "gauss_radii_all_zero", rc.opacity_logits(300, g), rc.log_scales("loguniform", 300, g),
               torch.zeros(300, dtype=torch.int32), 250, up)
    g = torch.Generator().manual_seed(103)
    gauss_case(mods, "gauss_isotropic_init", torch.full((777, 1), float(np.log(0.3 / 0.7)), dtype=torch.float32),
               rc.log_scales("isotropic", 777, g), rc.radii_mix(777, g), 777, up)
    g = torch.Generator().manual_seed(104)
    image_case(mods, "image_24x37", rc.altitude_image(24, 37, g), rc.accumulated_image(24, 37, g), (0.875, -1.75))
    image_case(mods, "image_2x2", torch.tensor([[1.5, 1.5], [-2.0, 3.25]]), torch.tensor([[0.0, 1.0], [0.25, 0.5]]), (0.875, -1.75))
    image_case(mods, "image_flat_9x16", torch.full((9, 16), -4.75), rc.accumulated_image(9, 16, g), (1.0, 1.0))
