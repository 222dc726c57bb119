"""Density control on one GPU (eogs2_amd.density) against what it replaces, on the same card:

  statistics   DensityStats.update (one launch) against the reference's PyTorch lines (train_pan.py:681-690,
               gaussian_model.py:719-723: nonzero(radii > 0), then three indexed read-modify-writes), at `--rows` rows with
               half of them visible;
  densify      densify_and_prune (one decision pass, one wait, one build pass) against the stepwise path of eogs2_amd.optim
               with the reference's mask expressions in PyTorch: densify_and_clone -> densify_and_split -> prune_optimizer.

    python tools/density_probe.py [--out profiles/density_probe.json] [--rows 1000000] [--rounds 10] [--iters 20]

Times: after a warm-up the two paths alternate, `rounds` times; each turn is `iters` calls between two device events (the
densify paths rebuild their optimizer state from clones before every call, OUTSIDE the events: a turn there is one call).
Reported per path: the median turn in ms per call and the spread of the turns (min, max). No speed ratio is an acceptance
condition of this feature; the file records what was measured and what was not.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eogs2_amd import density, optim  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402

EXTENT, PD, THR, N = 5.0, 0.01, 2.0 ** -19, 2
GROUPS = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (0, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def timed(fn, iters=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_stats(accum, denom, maxr, vg, radii):
    """train_pan.py:681-690 with renderer.py:128-130's visibility_filter."""
    vis = torch.nonzero(radii > 0)
    maxr[vis] = torch.max(maxr[vis], radii[vis])
    accum[vis] += torch.norm(vg[vis, :2], dim=-1, keepdim=True)
    denom[vis] += 1


def make_state(P, dev, g):
    par = {n: torch.randn((P,) + s, generator=g).to(dev) for n, s in GROUPS.items()}
    par["scaling"] = torch.log(torch.exp(torch.rand(P, 3, generator=g) * np.log(200.0)) * 0.005).to(dev)  # 0.005 .. 1
    par["opacity"] = (torch.rand(P, 1, generator=g) * 11.0 - 8.0).to(dev)
    mom = {n: (torch.randn((P,) + s, generator=g).to(dev), torch.rand((P,) + s, generator=g).to(dev)) for n, s in GROUPS.items()}
    denom = torch.randint(0, 9, (P, 1), generator=g).float()
    accum = (denom * THR * torch.exp2(torch.randint(-3, 4, (P, 1), generator=g).float())).to(dev)
    return par, mom, {"xyz_gradient_accum": accum, "denom": denom.to(dev), "max_radii2D": torch.zeros(P, device=dev)}


def make_opt(par, mom):
    groups = [{"params": [torch.nn.Parameter(par[n].clone())], "lr": 1e-3, "name": n} for n in GROUPS]
    opt = optim.FusedAdam(groups, lr=0.0, eps=1e-15)
    for gr in opt.param_groups:
        m, v = mom[gr["name"]]
        opt.state[gr["params"][0]] = {"step": torch.tensor(5.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    return opt


def stepwise(opt, stats):
    """Today's path: the reference's mask expressions in PyTorch, one library call per stage."""
    import optim_cases as oc

    par = lambda: {g["name"]: g["params"][0].detach() for g in opt.param_groups}  # noqa: E731
    grads = oc.mean_grads(stats["xyz_gradient_accum"], stats["denom"])
    optim.densify_and_clone(opt, oc.clone_mask(grads, par()["scaling"], THR, PD, EXTENT))
    optim.densify_and_split(opt, oc.split_mask(grads, par()["xyz"].shape[0], par()["scaling"], THR, PD, EXTENT), N=N)
    n = par()["xyz"].shape[0]
    m = oc.final_prune_mask(par()["opacity"], par()["scaling"], torch.zeros(n, device=grads.device), 20, EXTENT)
    optim.prune_optimizer(opt, ~m)
    return par()["xyz"].shape[0]


def one_pass(opt, stats):
    _, _, info = density.densify_and_prune(opt, stats, grad_threshold=THR, min_opacity=0.005, screen_size_threshold=EXTENT,
                                           max_screen_size=20, scene_extent=EXTENT, percent_dense=PD, N=N)
    return info.n_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_probe.json"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    dev, P = torch.device("cuda:0"), a.rows
    g = torch.Generator().manual_seed(0)
    out = {"what": f"{P} rows, fp32; the two paths alternate, {a.rounds} turns each between device events; ms per call "
                   f"(statistics: {a.iters} calls per turn; densify: one call per turn, the state rebuilt outside the events)",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0)}
    # ---- statistics ----
    vg = torch.randn(P, 3, generator=g).to(dev) * 1e-5
    radii = (torch.randint(1, 41, (P,), generator=g) * (torch.rand(P, generator=g) < 0.5)).to(torch.int32).to(dev)
    radii_f = radii.float()
    ours, ref = density.DensityStats(P, dev), density.DensityStats(P, dev)
    for _ in range(3):
        ours.update(vg, radii)
        torch_stats(*ref.tensors(), vg, radii_f)
    same = [bool(torch.equal(x, y)) for x, y in zip(ours.tensors(), ref.tensors())]
    err = float((ours.xyz_gradient_accum - ref.xyz_gradient_accum).abs().max() / ref.xyz_gradient_accum.abs().max())
    assert same[1] and same[2] and err <= 1e-6, (same, err)  # faster and different is not faster
    hip, tor = [], []
    for _ in range(a.rounds):
        hip.append(timed(lambda: ours.update(vg, radii), a.iters))
        tor.append(timed(lambda: torch_stats(*ref.tensors(), vg, radii_f), a.iters))
    h, t = summary(hip), summary(tor)
    out["statistics"] = {"hip": h, "torch_lines": t, "spread_ms": max(h["max_ms"] - h["min_ms"], t["max_ms"] - t["min_ms"]),
                         "torch_over_hip": t["median_ms"] / h["median_ms"], "visible_fraction": float((radii > 0).float().mean()),
                         "computed_bytes_per_row": 40, "computed_GBps_at_median": 40.0 * P / (h["median_ms"] * 1e-3) / 1e9,
                         "xyz_gradient_accum_max_relative_difference": err}
    print("statistics", json.dumps(out["statistics"]), flush=True)
    # ---- densify ----
    par, mom, stats = make_state(P, dev, g)
    rows = {"one_pass": [], "stepwise": []}
    sizes = {}
    for k in range(a.rounds + 2):  # two warm-up turns
        for name, fn in (("one_pass", one_pass), ("stepwise", stepwise)):
            opt = make_opt(par, mom)
            st = {k2: v.clone() for k2, v in stats.items()}
            torch.manual_seed(1)
            box = []
            ms = timed(lambda: box.append(fn(opt, st)))
            sizes[name] = box[0]
            if k >= 2:
                rows[name].append(ms)
    assert sizes["one_pass"] == sizes["stepwise"], sizes
    h, t = summary(rows["one_pass"]), summary(rows["stepwise"])
    out["densify_and_prune"] = {"one_pass": h, "stepwise_with_torch_masks": t,
                                "spread_ms": max(h["max_ms"] - h["min_ms"], t["max_ms"] - t["min_ms"]),
                                "stepwise_over_one_pass": t["median_ms"] / h["median_ms"], "rows_after": sizes["one_pass"],
                                "note": "wall time between device events around ONE call, host waits included (one for the one-pass "
                                        "path, three and the mask expressions' own for the stepwise path)"}
    print("densify_and_prune", json.dumps(out["densify_and_prune"]), flush=True)
    out["not_measured"] = ("other row counts and selection mixes; sh_degree > 0; the statistics update inside a recorded graph; the per-kernel "
                           "split of densify_and_prune (decide, scan, gather of the draw's scales, build); the reference's own "
                           "densify_and_prune in PyTorch (the stepwise path of eogs2_amd.optim stands in for it); more than one GPU")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
