"""The two in-place resets on one GPU (eogs2_amd.reset) against the reference's own lines as torch ops on the same card:

  color reset    the device part of one colour reset — erode, flags and rows (shadow_reset_flags + color_reset_) for `--views`
                 shadow maps of `--size`^2 and `--rows` Gaussians — against color_reset_op.py:45-88: max_pool2d, grid_sample and
                 `|` per view, then the three masked assignments and the six masked_fill_ of the moments. The renders of
                 render_all_views are the same on both sides and are not timed;
  opacity reset  reset_opacity_ at `--rows` rows against gaussian_model.py:347-352 with replace_tensor_to_optimizer
                 (eogs2_amd.optim.reset_opacity: sigmoid, min, log, two zeros_like, a new Parameter).

    python tools/reset_probe.py [--out profiles/reset_probe.json] [--rows 1000000] [--views 20] [--size 1024] [--rounds 10]

Times: after a warm-up the two paths alternate, `rounds` times; each turn is one call between two device events (the state is
rebuilt from clones before every turn, outside the events). Reported per path: the median turn in ms and the spread of the
turns (min, max). No speed ratio is an acceptance condition of this feature; the file records what was measured and what was not.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eogs2_amd import optim, reset  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402

GROUPS = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (0, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
C0 = 0.28209479177387814


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def make_opt(par, mom):
    groups = [{"params": [torch.nn.Parameter(par[n].clone())], "lr": 1e-3, "name": n} for n in GROUPS]
    opt = optim.FusedAdam(groups, lr=0.0, eps=1e-15)
    for gr in opt.param_groups:
        m, v = mom[gr["name"]]
        opt.state[gr["params"][0]] = {"step": torch.tensor(5.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    return opt


def by_name(opt):
    return {g["name"]: g["params"][0] for g in opt.param_groups}


def torch_color_reset(opt, xyz, views):
    """color_reset_op.py:43-88 on the optimizer's groups (projxyz as ECEF_to_UVA computes it)."""
    to_reset = torch.full((xyz.size(0),), False, device=xyz.device, dtype=bool)
    for shadowmap, affine in views:
        pts = xyz @ affine[:3, :2] + affine[3, :2]
        e = 1 - torch.max_pool2d(1 - shadowmap[None, None], 5, stride=1, padding=2).squeeze()
        hit = F.grid_sample(e[None, None], pts[None, None], mode="bilinear", align_corners=True, padding_mode="zeros").squeeze() < 0.5
        to_reset = to_reset | hit
    p = by_name(opt)
    with torch.no_grad():
        x = 0.005 * torch.ones_like(p["opacity"][to_reset])
        p["opacity"][to_reset] = torch.log(x / (1 - x))
        p["f_dc"][to_reset] = (torch.full_like(p["f_dc"][to_reset], 1.1) - 0.5) / C0
        p["scaling"][to_reset] = torch.log((1.0 / 400) * torch.ones_like(p["scaling"][to_reset]))
        for name in ("opacity", "f_dc", "scaling"):
            mask = to_reset.squeeze().clone()
            while len(mask.shape) < len(p[name].shape):
                mask = mask.unsqueeze(-1)
            opt.state[p[name]]["exp_avg"].masked_fill_(mask, 0.0)
            opt.state[p[name]]["exp_avg_sq"].masked_fill_(mask, 0.0)
    return to_reset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reset_probe.json"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev, P, S = torch.device("cuda:0"), a.rows, a.size
    g = torch.Generator().manual_seed(0)
    out = {"what": f"{P} rows, {a.views} shadow maps of {S} x {S}, fp32; the two paths alternate, {a.rounds} turns each, one call per "
                   "turn between device events, the state rebuilt outside the events; ms per call",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0)}
    par = {n: torch.randn((P,) + s, generator=g).to(dev) for n, s in GROUPS.items()}
    par["xyz"] = (torch.rand(P, 3, generator=g) * 2.0 - 1.0).to(dev)
    par["opacity"] = (torch.rand(P, 1, generator=g) * 11.0 - 8.0).to(dev)
    mom = {n: (torch.randn((P,) + s, generator=g).to(dev), torch.rand((P,) + s, generator=g).to(dev)) for n, s in GROUPS.items()}
    y, x = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    views = []
    for k in range(a.views):  # mostly lit maps with dark bands, one view matrix each that keeps most rows inside
        f = (torch.rand(4, generator=g) * 0.05 + 0.01).tolist()
        s = (1.35 + torch.sin(f[0] * x + 3.0 * f[1]) * torch.cos(f[2] * y + 3.0 * f[3])).clamp(0.0, 1.0)
        A = torch.zeros(4, 4)
        A[:3, :3] = torch.eye(3) * 0.8 + 0.08 * torch.randn(3, 3, generator=g)
        A[3, :3], A[3, 3] = 0.05 * torch.randn(3, generator=g), 1.0
        views.append((s.to(dev).contiguous(), A.to(dev).contiguous()))
    xyz = par["xyz"]

    def hip_color(opt):
        reset.color_reset_(opt, reset.shadow_reset_flags(xyz, views))

    # ---- colour reset ----
    a_opt, b_opt = make_opt(par, mom), make_opt(par, mom)
    flags = reset.shadow_reset_flags(xyz, views)
    reset.color_reset_(a_opt, flags)
    want = torch_color_reset(b_opt, xyz, views)
    differ = int((flags.bool() != want).sum())
    flagged = flags.bool()
    # (the library stores the reference's CPU bits; the torch lines run log on the GPU, which may round the last bit differently)
    same = all(torch.allclose(by_name(a_opt)[n][flagged & want], by_name(b_opt)[n][flagged & want], rtol=1e-6, atol=0.0)
               for n in ("opacity", "f_dc", "scaling"))
    assert differ <= 1e-3 * P and same, (differ, same)  # faster and different is not faster
    rows = {"hip": [], "torch_lines": []}
    for k in range(a.rounds + 2):  # two warm-up turns
        for name, fn in (("hip", hip_color), ("torch_lines", lambda o: torch_color_reset(o, xyz, views))):
            opt = make_opt(par, mom)
            ms = timed(lambda: fn(opt))
            if k >= 2:
                rows[name].append(ms)
    h, t = summary(rows["hip"]), summary(rows["torch_lines"])
    out["color_reset"] = {"hip": h, "torch_lines": t, "spread_ms": max(h["max_ms"] - h["min_ms"], t["max_ms"] - t["min_ms"]),
                          "torch_over_hip": t["median_ms"] / h["median_ms"], "flagged_fraction": float(flagged.float().mean()),
                          "rows_flagged_differently": differ,
                          "note": "erode + flags + rows; the torch side's boolean-mask assignments wait for the device (nonzero), "
                                  "the library's side queues launches alone"}
    print("color_reset", json.dumps(out["color_reset"]), flush=True)
    # ---- opacity reset ----
    rows = {"hip": [], "torch_lines": []}
    for k in range(a.rounds + 2):
        for name, fn in (("hip", reset.reset_opacity_), ("torch_lines", optim.reset_opacity)):
            opt = make_opt(par, mom)
            ms = timed(lambda: fn(opt))
            if k >= 2:
                rows[name].append(ms)
    h, t = summary(rows["hip"]), summary(rows["torch_lines"])
    out["reset_opacity"] = {"hip": h, "torch_lines": t, "spread_ms": max(h["max_ms"] - h["min_ms"], t["max_ms"] - t["min_ms"]),
                            "torch_over_hip": t["median_ms"] / h["median_ms"]}
    print("reset_opacity", json.dumps(out["reset_opacity"]), flush=True)
    out["not_measured"] = ("the renders of render_all_views (the same on both sides); other row counts, view counts and map sizes; the "
                           "split between erode, flags and rows; the resets inside a recorded graph; what a new recording of the step "
                           "costs after the replacing reset_opacity (tools/step_probe.py times recordings); more than one GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
