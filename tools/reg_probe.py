"""The regularisers on one GPU: forward + backward of eogs2_amd.regularizers against the reference's PyTorch op sequences
(loss/opacity.py:14-17,44-45, loss/main_loss.py:26-34,46-50: sigmoid / exp on the raw parameters, the elementwise ops,
autograd's backward) on the same card:

  opacity alone at 1 M rows; opacity + erank at 1 M rows; TV + accumulated opacity at 1024^2 and at 2048^2;
  ms/iter of examples/train_synthetic.py at its documented size without the term, with --opacity-loss 0.1, and with the same
  term added as the reference's torch expression (eager and under --graph).

    python tools/reg_probe.py [--out profiles/reg_probe.json] [--rounds 10] [--iters 40]

Times: after a warm-up of every shape the two paths alternate, `rounds` times; each turn is `iters` forward + backward calls
between two device events (rounds x iters >= 200 calls per path). Reported per path: the median turn in ms per call and the
spread of the turns (min, max). Kernel-group times are the library's profile slots reg_fwd / reg_bwd (HIP events around each
launch group: bracket times, which include the events' own cost), taken in a separate pass. Acceptance (per case): the HIP
path is not slower than the PyTorch sequence by more than the measured spread; for the example, the HIP term does not add
more ms per iteration than the torch expression does, by more than the spread.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eogs2_amd import _lib, regularizers as R  # noqa: E402
from eogs2_amd.build import source_hash  # noqa: E402


def torch_opacity(o, n_init):
    return torch.sigmoid(o).squeeze().sum() / n_init


def torch_erank(l):
    s2 = torch.exp(l).square() + 1e-5
    S = s2.sum(dim=1, keepdim=True)
    q = s2 / S
    erankm1 = torch.expm1(-(q * torch.log(q + 1e-6)).sum(dim=1))
    return (torch.log(erankm1 + 1e-5).mul(-1).clip(min=0.0) + s2.amin(1).sqrt()).mean()


def torch_tv(a):
    d1 = a[..., 1:, :] - a[..., :-1, :]
    d2 = a[..., :, 1:] - a[..., :, :-1]
    return 0.5 * (d1.abs().mean() + d2.abs().mean())


def turn(step, leaves, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        for x in leaves:
            x.grad = None
        step().backward()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def case(abi, name, hip_step, ref_step, leaves, rounds, iters):
    grads = []
    for _ in range(10):  # warm-up of every shape, both paths
        for step in (hip_step, ref_step):
            for x in leaves:
                x.grad = None
            v = step()
            v.backward()
            grads.append((float(v.detach()), [x.grad.clone() for x in leaves]))
    (v1, g1), (v2, g2) = grads[-2], grads[-1]
    err = [abs(v1 - v2) / abs(v2)] + [float((p - q).abs().max() / q.abs().max()) for p, q in zip(g1, g2)]
    # faster and different is not faster. A guard, not the parity bar (tests/test_gpu_reg.py holds that, against float64): two
    # fp32 evaluations of erank's gradient differ by up to ~1e-3 of the largest entry on needle-shaped rows, where
    # -log(e + 1e-5) amplifies the rounding of log(q + 1e-6) at q ~ 1 (tests/reg_cases.py derives it)
    assert err[0] <= 2e-4 and max(err[1:]) <= 5e-3, (name, err)
    hip, ref = [], []
    for _ in range(rounds):
        hip.append(turn(hip_step, leaves, iters))
        ref.append(turn(ref_step, leaves, iters))
    fwd, bwd = [], []
    for _ in range(25):  # kernel-group bracket times, in a pass of their own
        abi.profile_reset()
        torch.cuda.synchronize()
        abi.profile_enable(1)
        for x in leaves:
            x.grad = None
        hip_step().backward()
        torch.cuda.synchronize()
        abi.profile_enable(0)
        prof = abi.profile()
        fwd.append(prof["reg_fwd"][0])
        bwd.append(prof["reg_bwd"][0])
    h, r = summary(hip), summary(ref)
    spread = max(h["max_ms"] - h["min_ms"], r["max_ms"] - r["min_ms"])
    row = {"hip": h, "torch_sequence": r, "spread_ms": spread, "torch_over_hip": r["median_ms"] / h["median_ms"],
           "hip_not_slower_beyond_spread": h["median_ms"] <= r["median_ms"] + spread,
           "hip_bracket_ms": {"reg_fwd": float(np.median(fwd)), "reg_bwd": float(np.median(bwd))},
           "max_relative_difference": {"value": err[0], "gradients": err[1:]}}
    print(name, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reg_probe.json"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--no-example", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe times the GPU; there is no CPU fallback"
    assert a.rounds * a.iters >= 200
    import reg_cases as rc

    dev = torch.device("cuda:0")
    abi = _lib.get()
    abi.profile_select(0xFFFFFFFF)
    out = {"what": f"forward + backward of the regularisers, fp32; HIP path and the reference's PyTorch op sequence alternating, {a.rounds} "
                   f"turns of {a.iters} calls each between device events; ms per call. hip_bracket_ms: profile slots, HIP events around "
                   "each launch group, separate pass",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "cases": {}}
    g = torch.Generator().manual_seed(0)
    P = a.rows
    o = rc.opacity_logits(P, g).to(dev).requires_grad_(True)
    l = rc.log_scales("loguniform", P, g).to(dev).requires_grad_(True)
    w1, w2 = torch.tensor([0.1, 0.0, 0.0], device=dev), torch.tensor([0.1, 0.0, 0.02], device=dev)
    out["cases"][f"opacity, {P} rows"] = case(
        abi, "opacity", lambda: R.gaussian_regularizers(o, n_init=P, weights=w1)[0], lambda: 0.1 * torch_opacity(o, P), [o], a.rounds, a.iters)
    out["cases"][f"opacity + erank, {P} rows"] = case(
        abi, "opacity+erank", lambda: R.gaussian_regularizers(o, l, n_init=P, weights=w2, want=("opacity", "erank"))[0],
        lambda: 0.1 * torch_opacity(o, P) + 0.02 * torch_erank(l), [o, l], a.rounds, a.iters)
    wi = torch.tensor([0.3, 0.7], device=dev)
    for size in (1024, 2048):
        alt = rc.altitude_image(size, size, g).to(dev).requires_grad_(True)
        acc = rc.accumulated_image(size, size, g).to(dev).requires_grad_(True)
        out["cases"][f"TV + accumulated opacity, {size} x {size}"] = case(
            abi, f"image {size}", lambda: R.render_regularizers(alt, acc, weights=wi)[0],
            lambda: 0.3 * torch_tv(alt) + 0.7 * (1.0 - acc).mean(), [alt, acc], a.rounds, a.iters)
    if not a.no_example:
        import train_synthetic

        hip_entry = train_synthetic.gaussian_regularizers

        def torch_entry(opacity, scaling=None, radii=None, *, n_init, weights, want):  # the same term as the reference's expression
            return weights[0] * torch_opacity(opacity, n_init), None

        out["example_ms_per_iter"] = {"what": "examples/train_synthetic.py --quiet --no-prune (200 000 Gaussians, 512 x 512, 200 iterations, "
                                              "steady-state half), three runs each, alternating: without the term, with --opacity-loss 0.1 "
                                              "(HIP), and with the same term as the reference's torch expression in its place"}
        for mode, extra in (("eager", []), ("graph", ["--graph"])):
            base = ["--quiet", "--no-prune"] + extra
            ms = {"plain": [], "hip_term": [], "torch_term": []}
            for _ in range(3):  # alternating
                train_synthetic.main(base)
                ms["plain"].append(train_synthetic.main.last_ms_per_iter)
                train_synthetic.main(base + ["--opacity-loss", "0.1"])
                ms["hip_term"].append(train_synthetic.main.last_ms_per_iter)
                train_synthetic.gaussian_regularizers = torch_entry
                try:
                    train_synthetic.main(base + ["--opacity-loss", "0.1"])
                finally:
                    train_synthetic.gaussian_regularizers = hip_entry
                ms["torch_term"].append(train_synthetic.main.last_ms_per_iter)
            s = {k: summary(v) for k, v in ms.items()}
            spread = max(v["max_ms"] - v["min_ms"] for v in s.values())
            s["spread_ms"] = spread
            s["added_ms"] = {"hip_term": s["hip_term"]["median_ms"] - s["plain"]["median_ms"],
                             "torch_term": s["torch_term"]["median_ms"] - s["plain"]["median_ms"]}
            s["hip_adds_no_more_than_torch_beyond_spread"] = s["hip_term"]["median_ms"] <= s["torch_term"]["median_ms"] + spread
            out["example_ms_per_iter"][mode] = s
            print(mode, json.dumps(s), flush=True)
    out["not_measured"] = "the opacity_radii term on its own; other row counts and image sizes; more than one GPU; the example with --erank-loss"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
