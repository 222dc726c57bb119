"""Generates tests/golden/optim/*.npz by running the REFERENCE's own `GaussianModel` (scene/gaussian_model.py) through the
optimizer / density-control lifecycle of train_pan.py:664-732 on the CPU. Build machine only: it imports the reference
through make_golden_render.load_reference(). Only data is stored.

    python tests/golden/make_golden_optim.py [--out DIR] [case names: default all]

A fixture whose arrays are unchanged is not rewritten.

What runs is the reference's Python, unmodified: `training_setup`, `optimizer.step()` (torch.optim.Adam as configured
there), `add_densification_stats`, `prune_points`, `densify_and_prune` (`densify_and_clone`, `densify_and_split`,
`densification_postfix`, `prune_points`) and `reset_opacity`, on a `GaussianModel` whose tensors are set directly. The cases
and their scripts, the closed-form gradients, screen radii and screen-space gradients are tests/optim_cases.py's.

Device: the reference allocates with `device="cuda"`. While a case runs, `torch.zeros`, `zeros_like`, `ones`, `tensor` and
`eye` answer such a request on the CPU, in this process only. `torch.cuda.empty_cache()` does nothing without a device.

Recorded while the reference runs, by wrappers that call through: the result of every `torch.logical_and` (the clone and the
split mask), the argument of every `prune_points` (the split's prune filter, the final prune mask), the samples
`torch.normal` returned, and a snapshot of the model after `densification_postfix` of the clone and after every
`prune_points`. `densify_and_split` prints; stdout is silenced around the call.

Every case runs twice: in fp32, as the reference trains, and in float64 (default dtype float64, parameters and gradients
cast up, the fp32 run's normal samples handed back instead of a fresh draw) as the truth beside each stored array. The
generator asserts that both runs select the same rows everywhere and that no thresholded quantity of the float64 run lies
within optim_cases.MARGIN of its threshold, and prints the distance between the two runs at every snapshot.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import make_golden_render as mgr  # noqa: E402
import optim_cases as oc  # noqa: E402

REFROOT = mgr.REFROOT
OUT = oc.GOLDEN_DIR


@contextlib.contextmanager
def cuda_means_cpu():
    names = ("zeros", "zeros_like", "ones", "tensor", "eye")
    orig = {n: getattr(torch, n) for n in names}

    def wrap(f):
        def g(*a, **k):
            if str(k.get("device", "")).startswith("cuda"):
                k["device"] = "cpu"
            return f(*a, **k)
        return g

    for n in names:
        setattr(torch, n, wrap(orig[n]))
    try:
        yield
    finally:
        for n in names:
            setattr(torch, n, orig[n])


class Recorder:
    """Wraps torch.logical_and / torch.normal and two methods of one model for the duration of a densify_and_prune."""

    def __init__(self, model, snap, replay_normal=None):
        self.model, self.snap, self.replay = model, snap, replay_normal
        self.ands, self.prunes, self.normals, self.snaps = [], [], [], []

    def __enter__(self):
        self.o_and, self.o_normal = torch.logical_and, torch.normal
        m = self.model
        o_post, o_prune = m.densification_postfix, m.prune_points

        def logical_and(*a, **k):
            r = self.o_and(*a, **k)
            self.ands.append(r.clone())
            return r

        def normal(*a, **k):
            r = self.o_normal(*a, **k)
            if self.replay is not None:
                r = self.replay.pop(0).to(r.dtype)
            self.normals.append(r.detach().clone())
            return r

        def postfix(*a, **k):
            o_post(*a, **k)
            self.snaps.append(("postfix", self.snap(m), m.tmp_radii.clone()))

        def prune_points(mask):
            self.prunes.append(mask.clone())
            o_prune(mask)
            self.snaps.append(("prune", self.snap(m), None))

        torch.logical_and, torch.normal = logical_and, normal
        m.densification_postfix, m.prune_points = postfix, prune_points
        return self

    def __exit__(self, *exc):
        torch.logical_and, torch.normal = self.o_and, self.o_normal
        del self.model.densification_postfix, self.model.prune_points


def snapshot(m):
    """{key: numpy} of the model's parameters, Adam state and statistics."""
    d, steps = {}, []
    par = dict(xyz=m._xyz, f_dc=m._features_dc, f_rest=m._features_rest, opacity=m._opacity, scaling=m._scaling, rotation=m._rotation)
    for g in m.optimizer.param_groups:
        n, p = g["name"], g["params"][0]
        assert p is par[n], n  # the model's attribute and the optimizer's parameter are one object
        d[f"{n}/p"] = p.detach().numpy().copy()
        st = m.optimizer.state.get(p)
        if st:
            d[f"{n}/m"], d[f"{n}/v"] = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
        steps.append(int(st["step"]) if st else -1)
    assert len(m.optimizer.state) == sum(s >= 0 for s in steps)
    d["step"] = np.array(steps, dtype=np.int32)
    for k in oc.STATS:
        d[k] = getattr(m, k).numpy().copy()
    return d


def run_case(GaussianModel, cfg, f64, normals=None):
    """Runs the case's script on the reference. Returns (snapshots: list of dicts, stages: list of dicts, extras: dict)."""
    dt = torch.float64 if f64 else torch.float32
    P, sh = cfg["P"], cfg["sh"]
    m = GaussianModel(sh)
    init = oc.initial_params(cfg)
    m._xyz, m._features_dc, m._features_rest, m._opacity, m._scaling, m._rotation = (
        torch.nn.Parameter(init[n].to(dt)) for n in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))
    m.spatial_lr_scale = 1
    m._exposure = torch.nn.Parameter(torch.eye(3, 4)[None])
    m.max_radii2D = torch.zeros(P)
    m.training_setup(types.SimpleNamespace(**oc.TRAIN_ARGS))
    ids = np.arange(P, dtype=np.int32)
    snaps, stages, extras = [dict(snapshot(m), ids=ids)], [], {}
    normals = list(normals) if normals is not None else None
    it = 0

    def push(stage, snap, ids):
        snaps.append(dict(snap, ids=ids.copy()))
        stages.append(dict(stage, src=f"s{len(snaps) - 2}", dst=f"s{len(snaps) - 1}"))

    for op in cfg["script"]:
        k = len(snaps)
        if op[0] == "steps":
            for _ in range(op[1]):
                it += 1
                for g in m.optimizer.param_groups:
                    g["params"][0].grad = oc.hashed_grad(it, ids, g["name"], sh).to(dt)
                m.optimizer.step()
                m.optimizer.zero_grad(set_to_none=True)
                if op[2]:
                    r = oc.radii(it, ids).to(dt)
                    vis = r > 0
                    m.max_radii2D[vis] = torch.max(m.max_radii2D[vis], r[vis])
                    m.add_densification_stats(types.SimpleNamespace(grad=oc.viewspace_grad(it, ids).to(dt)), vis)
            push(dict(op="steps", n=op[1], it0=it - op[1], stats=bool(op[2])), snapshot(m), ids)
        elif op[0] == "tprune":
            mask = m._opacity.squeeze() < oc.MIN_OPACITY
            extras[f"mask{k}"] = mask.numpy().copy()
            if mask.any():
                m.prune_points(mask)
            ids = ids[~mask.numpy()]
            push(dict(op="tprune", mask=f"mask{k}", called=bool(mask.any())), snapshot(m), ids)
        elif op[0] == "reset":
            m.reset_opacity()
            push(dict(op="reset"), snapshot(m), ids)
        elif op[0] == "densify":
            rad = oc.radii(it, ids).to(dt)
            with Recorder(m, snapshot, normals) as rec, contextlib.redirect_stdout(io.StringIO()):
                m.densify_and_prune(cfg["grad_threshold"], oc.DENSIFY_MIN_OPACITY, cfg["extent"], op[1], rad, cfg["extent"])
            (k1, s_clone, r_clone), (k2, _, r_split), (k3, s_split, _), (k4, s_prune, _) = rec.snaps
            assert (k1, k2, k3, k4) == ("postfix", "postfix", "prune", "prune") and len(rec.ands) == 2 and len(rec.prunes) == 2
            cm, sm, fm = rec.ands[0].numpy(), rec.ands[1].numpy(), rec.prunes[1].numpy()
            nsel = int(sm.sum())
            assert np.array_equal(rec.prunes[0].numpy(), np.concatenate([sm, np.zeros(oc.SPLIT_N * nsel, bool)]))
            assert len(rec.normals) == 1 and rec.normals[0].shape == (oc.SPLIT_N * nsel, 3)
            extras[f"mask{k}"], extras[f"mask{k + 1}"], extras[f"mask{k + 2}"] = cm, sm, fm
            extras[f"normal{k + 1}"] = rec.normals[0].numpy().copy()
            extras[f"radii{k}"] = rad.numpy().copy()
            extras[f"tmp_radii{k}"], extras[f"tmp_radii{k + 1}"] = r_clone.numpy().copy(), r_split.numpy().copy()
            ids = np.concatenate([ids, ids[cm]])
            push(dict(op="clone", mask=f"mask{k}", radii=f"radii{k}", tmp_radii=f"tmp_radii{k}"), s_clone, ids)
            ids = np.concatenate([ids, np.tile(ids[sm], oc.SPLIT_N)])[~rec.prunes[0].numpy()]
            push(dict(op="split", mask=f"mask{k + 1}", normal=f"normal{k + 1}", radii=f"tmp_radii{k}", tmp_radii=f"tmp_radii{k + 1}",
                      N=oc.SPLIT_N), s_split, ids)
            ids = ids[~fm]
            push(dict(op="prune", mask=f"mask{k + 2}", max_screen_size=op[1]), s_prune, ids)
        else:
            raise ValueError(op)
    return snaps, stages, extras


def check_row_bookkeeping(snaps, stages, extras):
    """The id column is kept by this generator, not by the reference. Shown right here: every tensor a structural stage only
    moves equals the source snapshot's rows picked by the same bookkeeping applied to row numbers."""
    for st in stages:
        a, b = snaps[int(st["src"][1:])], snaps[int(st["dst"][1:])]
        n = len(a["ids"])
        rows = np.arange(n)
        if st["op"] in ("tprune", "prune"):
            rows = rows[~extras[st["mask"]]]
        elif st["op"] == "clone":
            rows = np.concatenate([rows, rows[extras[st["mask"]]]])
        elif st["op"] == "split":
            sm = extras[st["mask"]]
            rows = np.concatenate([rows[~sm], np.tile(rows[sm], st["N"])])
        else:
            continue
        assert np.array_equal(b["ids"], a["ids"][rows]), st
        moved = ["f_dc", "f_rest", "opacity", "rotation"] + ([] if st["op"] == "split" else ["xyz", "scaling"])
        for g in moved:
            assert np.array_equal(b[f"{g}/p"], a[f"{g}/p"][rows]), (st, g)
        old = rows[:n - int(extras[st["mask"]].sum())] if st["op"] == "split" else rows[:n] if st["op"] == "clone" else rows
        for g in oc.GROUPS:  # moments: moved for the old rows, zero for the new ones
            for mv in ("m", "v"):
                assert np.array_equal(b[f"{g}/{mv}"][:len(old)], a[f"{g}/{mv}"][old]) and not b[f"{g}/{mv}"][len(old):].any()


def check_margins(cfg, snaps64, stages, ex32, ex64):
    """No thresholded quantity of the float64 run within MARGIN of its threshold, and the same masks in both runs."""
    pd_ext = oc.TRAIN_ARGS["percent_dense"] * cfg["extent"]
    for k in ex32:
        if k.startswith("mask"):
            assert np.array_equal(ex32[k], ex64[k]), k
    for st in stages:
        a, b = snaps64[int(st["src"][1:])], snaps64[int(st["dst"][1:])]
        if st["op"] == "tprune":
            assert not oc.near(a["opacity/p"], oc.MIN_OPACITY).any(), st
        elif st["op"] == "reset":
            assert not oc.near(1 / (1 + np.exp(-a["opacity/p"])), oc.RESET_CAP).any(), st
        elif st["op"] in ("clone", "split"):
            smax = np.exp(a["scaling/p"]).max(1)
            assert not oc.near(smax, pd_ext).any(), st
            if st["op"] == "clone":
                with np.errstate(invalid="ignore", divide="ignore"):
                    g = np.nan_to_num(a["xyz_gradient_accum"] / a["denom"], nan=0.0)
                assert not oc.near(g, cfg["grad_threshold"]).any(), st
        elif st["op"] == "prune":
            assert not oc.near(1 / (1 + np.exp(-a["opacity/p"])), oc.DENSIFY_MIN_OPACITY).any(), st
            if st["max_screen_size"]:
                assert not oc.near(np.exp(a["scaling/p"]).max(1), 0.1 * cfg["extent"]).any(), st
                assert not oc.near(a["max_radii2D"], st["max_screen_size"]).any(), st


def assemble(cfg, r32, r64):
    """The fixture's arrays. float64 twins: everything at the end of an Adam stretch, the parameters elsewhere."""
    (s32, stages, e32), (s64, stages64, e64) = r32, r64
    assert stages == stages64 and all(a["ids"].tolist() == b["ids"].tolist() for a, b in zip(s32, s64))
    d = {"stages": np.array(json.dumps(stages))}
    steps_dst = {st["dst"] for st in stages if st["op"] == "steps"}
    for i, (a, b) in enumerate(zip(s32, s64)):
        for k, v in a.items():
            d[f"s{i}/{k}"] = v.astype(np.float32) if v.dtype.kind == "f" else v
            assert v.dtype in (np.float32, np.int32), (k, v.dtype)
            if v.dtype.kind == "f" and (f"s{i}" in steps_dst or k.endswith("/p")) and i > 0:
                assert b[k].dtype == np.float64, k
                d[f"s{i}/{k}@64"] = b[k]
    d.update(e32)  # masks, the normal draw, radii: the same in both runs
    return d, stages


def distances(d, stages):
    """[(snapshot, group, array, max |fp32 - float64| / max |float64|)] over every float64 twin."""
    out = []
    for k in sorted(d):
        if k.endswith("@64") and k.startswith("s") and d[k].size:
            a, b = d[k[:-3]].astype(np.float64), d[k]
            out.append((k[:-3], float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    torch.set_num_threads(1)
    _, GaussianModel, _ = mgr.load_reference()
    os.makedirs(a.out, exist_ok=True)
    for name, cfg in oc.CASES.items():
        if a.cases and name not in a.cases:
            continue
        torch.manual_seed(cfg["seed"])
        with cuda_means_cpu():
            r32 = run_case(GaussianModel, cfg, False)
            torch.set_default_dtype(torch.float64)
            try:
                normals = [torch.from_numpy(v) for k, v in sorted(r32[2].items()) if k.startswith("normal")]
                r64 = run_case(GaussianModel, cfg, True, normals)
            finally:
                torch.set_default_dtype(torch.float32)
        check_row_bookkeeping(r32[0], r32[1], r32[2])
        check_row_bookkeeping(r64[0], r64[1], r64[2])
        check_margins(cfg, r64[0], r64[1], r32[2], r64[2])
        d, stages = assemble(cfg, r32, r64)
        path = oc.fixture_path(name, a.out)
        dist = distances(d, stages)
        worst = {}
        for k, v in dist:
            s = k.split("/")[0]
            worst[s] = max(worst.get(s, 0.0), v)
        rows = [len(s["ids"]) for s in r32[0]]
        sel = {st["dst"]: int(d[st["mask"]].sum()) for st in stages if "mask" in st}
        print(f"{name}: rows {rows} selected {sel}")
        print(f"{name}: fp32-to-float64 distance per snapshot (of the array's scale): " + ", ".join(f"{s} {v:.1e}" for s, v in worst.items()))
        if mgr.unchanged(path, d):
            print(f"{name}: unchanged")
            continue
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < oc.MAX_FIXTURE_BYTES, (name, size)
        print(f"{name}: -> {size / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
