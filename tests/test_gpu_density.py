"""GPU (MI355X): density control (include/eogs_density.h, eogs2_amd/density.py).

1. the statistics of the lifecycle fixtures (tests/golden/optim, recorded from the reference's GaussianModel) through
   `DensityStats.update`, float32 and int32 radii;
2. `densify_and_prune` from the fixtures' snapshot before `clone` against their snapshot after `prune`;
3. beyond one workgroup: sizes around the 256-row workgroup and the 256-workgroup scan round, selection patterns, against
   the stepwise `optim.densify_and_clone` -> `densify_and_split` -> `prune_optimizer` with the reference's mask expressions;
4. rows parked by `optim.retire_rows`;
5. reproducibility and graph capture;
6. examples/train_synthetic.py --densify-every.

What is moved is compared bit for bit. What is computed (a sample's position and log-scale) is held to
max(4 x the distance of the reference's / the stepwise path's own fp32 result from float64, 4 ulp): the rule of
optim_cases._computed_close; every such comparison prints its worst error / bound. An fp32 transcription of the kernel's
sample arithmetic on the CPU sits at 0.25 of that bound on the fixtures.
"""
import os
import sys

import numpy as np
import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("densify", "densify_screen", "empty_masks", "sh1")
EXTENT, PD, THR = 5.0, oc.TRAIN_ARGS["percent_dense"], oc.TIE_GRAD


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


# ---- 1. fixture statistics ----
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("int_radii", [False, True])
def test_fixture_statistics(dev, name, int_radii):
    from eogs2_amd.density import DensityStats

    fx = oc.Fixture(name)
    stages = [st for st in fx.stages if st["op"] == "steps" and st["stats"]]
    assert len(stages) == 2
    for st in stages:
        ids = fx.ids(st["src"])
        stats = DensityStats.of(oc.stats_of(fx, st["src"], dev))
        for k in range(st["n"]):
            it = st["it0"] + k + 1
            r = oc.radii(it, ids)
            stats.update(oc.viewspace_grad(it, ids).to(dev), (r.to(torch.int32) if int_radii else r).to(dev))
        dst = st["dst"]
        assert _bits(stats.denom) == fx.z[f"{dst}/denom"].tobytes(), (name, dst, "denom")
        assert _bits(stats.max_radii2D) == fx.z[f"{dst}/max_radii2D"].tobytes(), (name, dst, "max_radii2D")
        key = f"{dst}/xyz_gradient_accum"
        bound, scale, dist = oc.steps_bound(fx, key)
        err = float(np.abs(stats.xyz_gradient_accum.cpu().numpy().astype(np.float64) - fx.z[key + "@64"]).max())
        print(f"{name} {key}: error {err:.3e} bound {bound:.3e} (scale {scale:.3e}, fp32-to-float64 {dist:.3e})")
        assert stats.xyz_gradient_accum.shape == fx.z[key].shape and err <= bound, (name, key, err, bound)


# ---- 2. fixture densify ----
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_densify_and_prune(dev, name):
    from eogs2_amd.density import densify_and_prune
    from eogs2_amd.optim import FusedAdam

    fx = oc.Fixture(name)
    k = next(i for i, st in enumerate(fx.stages) if st["op"] == "clone")
    clone, split, prune = fx.stages[k:k + 3]
    assert (clone["op"], split["op"], prune["op"]) == ("clone", "split", "prune")
    src, dst = clone["src"], prune["dst"]
    opt = oc.make_optimizer(fx, src, FusedAdam, dev)
    stats, ids = oc.stats_of(fx, src, dev), fx.t(f"{src}/ids", dev)
    with oc.normal_returns(fx.t(split["normal"], dev)) as nr:
        params, new_stats, info = densify_and_prune(
            opt, stats, grad_threshold=fx.cfg["grad_threshold"], min_opacity=oc.DENSIFY_MIN_OPACITY,
            screen_size_threshold=fx.cfg["extent"], max_screen_size=prune["max_screen_size"], scene_extent=fx.cfg["extent"],
            percent_dense=PD, N=split["N"], radii=fx.t(clone["radii"], dev), extra=[ids])
    assert nr.calls == 1
    # the reference's three masks, rebuilt from the flag bytes, on every row
    for got, st in ((info.clone_mask(), clone), (info.split_mask(), split), (info.prune_mask(), prune)):
        want = fx.z[st["mask"]]
        assert got.dtype == torch.bool and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), (name, st["op"])
    m2, m3, m4 = fx.z[clone["mask"]], fx.z[split["mask"]], fx.z[prune["mask"]]
    n_mid = int((~m3).sum())  # rows before the samples in the reference's intermediate order
    assert info.n_split == int(m3.sum()) and info.n_kept + info.n_kept_clones == int((~m4[:n_mid]).sum())
    assert split["N"] * info.n_kept_split == int((~m4[n_mid:]).sum()) and info.n_kept_clones <= int(m2.sum())
    n_old = info.n_kept + info.n_kept_clones
    after = {g["name"]: g["params"][0] for g in opt.param_groups}
    assert all(params[n] is after[n] and after[n].requires_grad and isinstance(after[n], torch.nn.Parameter) for n in oc.GROUPS)
    assert len(opt.state) == len(oc.GROUPS) and all(after[n] in opt.state for n in oc.GROUPS)
    for n, want_step in zip(oc.GROUPS, fx.z[f"{dst}/step"]):
        state = opt.state[after[n]]
        assert int(state["step"]) == int(want_step) == int(fx.z[f"{src}/step"][oc.GROUPS.index(n)]), (name, n, "step")
        for kk, got in (("p", after[n].detach()), ("m", state["exp_avg"]), ("v", state["exp_avg_sq"])):
            key = f"{dst}/{n}/{kk}"
            got, want = got.cpu().numpy(), fx.z[key]
            assert got.dtype == np.float32 and got.shape == want.shape, (name, key, got.shape, want.shape)
            if kk == "p" and n in ("xyz", "scaling"):
                assert got[:n_old].tobytes() == want[:n_old].tobytes(), (name, key, "moved rows")
                r = oc._computed_close(fx, key, got, slice(n_old, None))
                print(f"{name} {key}: computed rows at {r:.3f} of their bound")
            else:
                assert got.tobytes() == want.tobytes(), (name, key)
    (ids2,) = info.extra
    assert ids2.dtype == torch.int32 and np.array_equal(ids2.cpu().numpy(), fx.z[f"{dst}/ids"]), (name, "ids")
    for kk in oc.STATS:  # zeros of the new size
        assert _bits(new_stats[kk]) == fx.z[f"{dst}/{kk}"].tobytes() and not bool(new_stats[kk].any()), (name, kk)


# ---- 3. beyond one workgroup ----
SIZES = (1, 255, 256, 257, 65_537, 131_329)
PATTERNS = ("none", "clone_all", "split_all", "prune_all", "alternating", "split_first", "split_last", "runs300", "sh1")
SCREEN = {"prune_all": 20, "alternating": 20, "runs300": 20, "sh1": 20}  # max_screen_size; the others None
LOGIT_MIN = float(np.log(oc.DENSIFY_MIN_OPACITY / (1 - oc.DENSIFY_MIN_OPACITY)))


def _pattern(pattern, P):
    """(category per row: 0 neither, 1 clone, 2 split; low-opacity rows)."""
    i = np.arange(P)
    low = (i % 7 == 3)
    if pattern == "none":
        cat = np.zeros(P, int)
    elif pattern == "clone_all":
        cat = np.ones(P, int)
    elif pattern == "split_all":
        cat = np.full(P, 2)
    elif pattern == "prune_all":
        cat, low = i % 3, np.ones(P, bool)
    elif pattern in ("alternating", "sh1"):
        cat = (i + 1) % 3
    elif pattern == "split_first":
        cat, low = np.zeros(P, int), np.zeros(P, bool)
        cat[0] = 2
    elif pattern == "split_last":
        cat, low = np.zeros(P, int), np.zeros(P, bool)
        cat[P - 1] = 2
    elif pattern == "runs300":  # runs of 300 consecutive split rows, each across a workgroup edge, 200 other rows between them
        cat = np.where((i + 400) % 500 < 300, 2, i % 2)
    else:
        raise ValueError(pattern)
    return cat, low


def make_case(pattern, P, seed=0):
    """A model state whose rows realise `pattern`, no thresholded quantity within oc.MARGIN of its threshold except the
    exact ties (rows with id % 16 == 5 that are selected: mean gradient norm == threshold). Returns a dict of CPU tensors."""
    sh = 1 if pattern == "sh1" else 0
    g = np.random.default_rng(seed + 1000 * PATTERNS.index(pattern) + P)
    cat, low = _pattern(pattern, P)
    i = np.arange(P)
    # statistics: denom 0..8 views, mean gradient norm 4 x / a quarter of the threshold, or exactly on it (powers of two: exact)
    denom = g.integers(1, 9, P).astype(np.float64)
    mean = np.where(cat > 0, 4.0 * THR, 0.25 * THR)
    mean[(cat > 0) & (i % 16 == 5)] = THR  # the ties: `>=` selects them
    never = (cat == 0) & (i % 5 == 0)  # never visible: 0 / 0 -> NaN -> 0
    denom[never] = 0.0
    accum = np.where(never, 0.0, mean * denom)
    # scales: clone rows below percent_dense * extent = 0.05; split rows above it, in three bands around 0.1 * extent = 0.5
    # (plain, the row too big, the row and its samples too big: exp(s) / 1.6 > 0.5); other rows anywhere
    band = g.integers(0, 4, P)
    band = np.where(cat == 1, 0, np.where(cat == 2, np.maximum(band, 1), band))
    lo = np.array([0.005, 0.07, 0.55, 0.9])[band]
    hi = np.array([0.04, 0.4, 0.75, 3.0])[band]
    smax = np.exp(g.uniform(np.log(lo), np.log(hi)))
    scaling = np.log(smax)[:, None] + np.log(g.uniform(0.2, 1.0, (P, 3)))
    scaling[i, g.integers(0, 3, P)] = np.log(smax)
    opacity = np.where(low, g.uniform(-9.0, LOGIT_MIN - 0.1, P), g.uniform(LOGIT_MIN + 0.1, 3.0, P))[:, None]
    shp = oc.shapes(sh)
    par = {"xyz": g.uniform(-5, 5, (P, 3)), "f_dc": g.normal(size=(P, 1, 3)), "f_rest": 0.1 * g.normal(size=(P,) + shp["f_rest"]),
           "opacity": opacity, "scaling": scaling, "rotation": g.normal(size=(P, 4)) * np.exp(g.uniform(-1, 1, (P, 1)))}
    case = {"P": P, "sh": sh, "pattern": pattern, "max_screen_size": SCREEN.get(pattern),
            "grad_threshold": 1.0 if pattern == "none" else THR,
            "p": {n: torch.from_numpy(np.ascontiguousarray(par[n], dtype=np.float32)) for n in oc.GROUPS},
            "m": {n: torch.from_numpy(g.normal(size=par[n].shape).astype(np.float32)) for n in oc.GROUPS},
            "v": {n: torch.from_numpy((g.normal(size=par[n].shape) ** 2).astype(np.float32)) for n in oc.GROUPS},
            "stats": {"xyz_gradient_accum": torch.from_numpy(accum.astype(np.float32)[:, None]),
                      "denom": torch.from_numpy(denom.astype(np.float32)[:, None]), "max_radii2D": torch.from_numpy(g.integers(0, 41, P).astype(np.float32))},
            "ids": torch.arange(P, dtype=torch.int32)}
    assert np.array_equal(case["stats"]["xyz_gradient_accum"].double().numpy()[:, 0], accum)  # exact in fp32
    return case


def decide_f64(case, alive=None):
    """The decisions in float64 on the CPU from the fp32 state, with the assertion that none of them is near its threshold
    (a condition of the comparison, not a tolerance). Returns (clone, split, prune_self, prune_samp) boolean arrays."""
    thr = case["grad_threshold"]
    a, d = case["stats"]["xyz_gradient_accum"].double().numpy()[:, 0], case["stats"]["denom"].double().numpy()[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        gm = a / d
    gm[np.isnan(gm)] = 0.0
    s = np.exp(case["p"]["scaling"].double().numpy())
    smax = s.max(axis=1)
    samp = np.exp(np.log(s / (0.8 * oc.SPLIT_N))).max(axis=1)
    sig = 1.0 / (1.0 + np.exp(-case["p"]["opacity"].double().numpy()[:, 0]))
    big = 0.1 * EXTENT
    for x, t in ((gm, thr), (smax, PD * EXTENT), (sig, oc.DENSIFY_MIN_OPACITY)) + (((smax, big), (samp, big)) if case["max_screen_size"] else ()):
        assert not oc.near(x, np.float64(np.float32(t))).any() and not oc.near(x, t).any(), (case["pattern"], case["P"], t)
    sel = gm >= np.float32(thr)
    if alive is not None:
        sel = sel & alive
    low = sig < np.float32(oc.DENSIFY_MIN_OPACITY)
    scr = bool(case["max_screen_size"])
    return (sel & (smax <= np.float32(PD * EXTENT)), sel & (smax > np.float32(PD * EXTENT)),
            low | (scr & (smax > np.float32(big))), low | (scr & (samp > np.float32(big))))


def make_opt(case, dev, cls):
    groups = [{"params": [torch.nn.Parameter(case["p"][n].clone().to(dev))], "lr": oc.lrs()[n], "name": n} for n in oc.GROUPS]
    opt = cls(groups, lr=0.0, eps=oc.EPS)
    for g in opt.param_groups:
        n = g["name"]
        opt.state[g["params"][0]] = {"step": torch.tensor(7.0), "exp_avg": case["m"][n].clone().to(dev), "exp_avg_sq": case["v"][n].clone().to(dev)}
    return opt


def snapshot(opt):
    out = {}
    for g in opt.param_groups:
        p = g["params"][0]
        st = opt.state[p]
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and int(st["step"]) == 7
        out[g["name"]] = (p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
    assert len(opt.state) == len(oc.GROUPS)
    return out


def stepwise(case, dev, samples, ids=None, stats=None, opt=None):
    """The existing path: the reference's mask expressions (optim_cases) -> densify_and_clone -> densify_and_split ->
    prune_optimizer, on `dev`, with the handed-in samples. Returns (snapshot, ids, (clone, split, prune) masks)."""
    from eogs2_amd import optim
    from eogs2_amd.optim import FusedAdam

    opt = opt or make_opt(case, dev, FusedAdam)
    stats = stats or {k: v.to(dev) for k, v in case["stats"].items()}
    ids = case["ids"].to(dev) if ids is None else ids
    par = lambda: {g["name"]: g["params"][0].detach() for g in opt.param_groups}  # noqa: E731
    thr, mss = case["grad_threshold"], case["max_screen_size"]
    grads = oc.mean_grads(stats["xyz_gradient_accum"], stats["denom"])
    m_clone = oc.clone_mask(grads, par()["scaling"], thr, PD, EXTENT)
    _, ids = optim.densify_and_clone(opt, m_clone, tmp_radii=ids)
    m_split = oc.split_mask(grads, par()["xyz"].shape[0], par()["scaling"], thr, PD, EXTENT)
    with oc.normal_returns(samples.to(dev)) as nr:
        _, ids, keep = optim.densify_and_split(opt, m_split, N=oc.SPLIT_N, tmp_radii=ids)
    assert nr.calls == 1
    ids = ids[keep]
    n = par()["xyz"].shape[0]
    m_prune = oc.final_prune_mask(par()["opacity"], par()["scaling"], torch.zeros(n, device=dev), mss, EXTENT)
    _, (ids,) = optim.prune_optimizer(opt, ~m_prune, extra=[ids])
    return snapshot(opt), ids.cpu().numpy(), (m_clone.cpu().numpy(), m_split.cpu().numpy(), m_prune.cpu().numpy())


def one_pass(case, dev, samples, **kw):
    from eogs2_amd.density import densify_and_prune
    from eogs2_amd.optim import FusedAdam

    opt = kw.pop("opt", None) or make_opt(case, dev, FusedAdam)
    stats = kw.pop("stats", None) or {k: v.to(dev) for k, v in case["stats"].items()}
    ids = kw.pop("ids", None)
    ids = case["ids"].to(dev) if ids is None else ids
    with oc.normal_returns(samples.to(dev)) as nr:
        params, new_stats, info = densify_and_prune(opt, stats, grad_threshold=case["grad_threshold"], min_opacity=oc.DENSIFY_MIN_OPACITY,
                                                    screen_size_threshold=EXTENT, max_screen_size=case["max_screen_size"],
                                                    scene_extent=EXTENT, percent_dense=PD, N=oc.SPLIT_N, extra=[ids])
    assert nr.calls == 1
    now = {g["name"]: g["params"][0] for g in opt.param_groups}
    assert all(params[n] is now[n] for n in oc.GROUPS)
    for k in oc.STATS:
        assert new_stats[k].shape[0] == info.n_out and new_stats[k].ndim == case["stats"][k].ndim and not bool(new_stats[k].any())
    return snapshot(opt), info.extra[0].cpu().numpy(), info


def samples_f64(case, samples, split, kept_split):
    """float64 positions and log-scales of the kept samples, copy-major, from the fp32 state and the fp32 draw."""
    N, nS = oc.SPLIT_N, int(split.sum())
    srank = np.cumsum(split) - 1
    rows = np.nonzero(kept_split)[0]
    q = case["p"]["rotation"].double().numpy()[rows]
    q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    r, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    sm = samples.double().numpy()
    xyz, sc = [], []
    for c in range(N):
        s = sm[c * nS + srank[rows]]
        xyz.append(np.einsum("kij,kj->ki", R, s) + case["p"]["xyz"].double().numpy()[rows])
        sc.append(np.log(np.exp(case["p"]["scaling"].double().numpy()[rows]) / (0.8 * N)))
    return np.concatenate(xyz) if rows.size else np.zeros((0, 3)), np.concatenate(sc) if rows.size else np.zeros((0, 3))


def compare(case, dev, got, got_ids, info, want, want_ids, want_masks, alive=None):
    """One-pass result against the stepwise one; returns the worst error / bound of the computed rows."""
    clone, split, pself, psamp = decide_f64(case, alive)
    counts = (int((~split & ~pself).sum()), int((clone & ~pself).sum()), int(split.sum()), int((split & ~psamp).sum()))
    assert (info.n_kept, info.n_kept_clones, info.n_split, info.n_kept_split) == counts, (case["pattern"], case["P"], counts)
    f = info.flags.cpu().numpy()
    for bit, m in ((1, clone), (2, split), (4, pself), (8, psamp)):
        assert np.array_equal((f & bit) != 0, m), (case["pattern"], case["P"], "flag bit", bit)
    for g_, w_ in zip((info.clone_mask(), info.split_mask(), info.prune_mask()), want_masks):
        assert np.array_equal(g_.cpu().numpy(), w_), (case["pattern"], case["P"], "mask")
    assert got_ids.dtype == np.int32 and np.array_equal(got_ids, want_ids), (case["pattern"], case["P"], "ids / order")
    n_old = counts[0] + counts[1]
    xyz64, sc64 = samples_f64(case, case["samples"], split, split & ~psamp)
    worst = 0.0
    for n in oc.GROUPS:
        for k, (a, b) in enumerate(zip(got[n], want[n])):
            assert a.dtype == np.float32 and a.shape == b.shape, (case["pattern"], case["P"], n, k, a.shape, b.shape)
            if k == 0 and n in ("xyz", "scaling"):
                assert a[:n_old].tobytes() == b[:n_old].tobytes(), (case["pattern"], case["P"], n, "moved rows")
                f64 = xyz64 if n == "xyz" else sc64
                assert f64.shape == a[n_old:].shape
                if f64.size:
                    dist = float(np.abs(b[n_old:].astype(np.float64) - f64).max())  # the existing path's own distance
                    bound = np.maximum(4 * dist, 4 * oc._ulp32(f64))
                    ratio = float((np.abs(a[n_old:].astype(np.float64) - f64) / bound).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (case["pattern"], case["P"], n, ratio)
            else:
                assert a.tobytes() == b.tobytes(), (case["pattern"], case["P"], n, ("p", "m", "v")[k])
    return worst


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("P", SIZES)
def test_sizes_and_patterns_equal_the_stepwise_path(dev, P, pattern):
    case = make_case(pattern, P)
    _, split, _, _ = decide_f64(case)
    g = torch.Generator().manual_seed(P)
    case["samples"] = 0.1 * torch.randn(oc.SPLIT_N * int(split.sum()), 3, generator=g)
    want, want_ids, want_masks = stepwise(case, dev, case["samples"])
    got, got_ids, info = one_pass(case, dev, case["samples"])
    worst = compare(case, dev, got, got_ids, info, want, want_ids, want_masks)
    print(f"{pattern} P={P}: {info.n_out} rows, computed rows worst ratio {worst:.3f}")


# ---- 4. retired rows ----
def test_retired_rows_are_never_selected_and_never_survive(dev):
    from eogs2_amd import optim
    from eogs2_amd.density import DensityStats
    from eogs2_amd.optim import FusedAdam

    P = 1000
    case = make_case("alternating", P, seed=4)
    keep = torch.from_numpy((np.arange(P) // 2) % 3 != 0)  # a third, in pairs: every category on both sides
    retired = ~keep.numpy()
    # (1) statistics: the rasterizer gives a retired row radius 0; its statistics keep their bits
    stats = DensityStats.of({k: v.clone().to(dev) for k, v in case["stats"].items()})
    before = [t.clone() for t in stats.tensors()]
    vg = oc.viewspace_grad(3, np.arange(P)).to(dev)
    r = torch.where(keep, oc.radii(3, np.arange(P)) + 1.0, torch.zeros(P)).to(torch.int32).to(dev)
    stats.update(vg, r)
    small = DensityStats.of({k: v[keep].clone().to(dev) for k, v in case["stats"].items()})
    small.update(vg[keep.to(dev)].contiguous(), r[keep.to(dev)].contiguous())
    for t, t0, ts in zip(stats.tensors(), before, small.tensors()):
        assert _bits(t[~keep.to(dev)]) == _bits(t0[~keep.to(dev)]) and _bits(t[keep.to(dev)]) == _bits(ts)
        assert _bits(t[keep.to(dev)]) != _bits(t0[keep.to(dev)])
    # (2) densify: the retired state in one pass == compaction first, then the same pass
    clone, split, pself, psamp = decide_f64(case, alive=~retired)
    assert (decide_f64(case)[1] & retired).any() and pself[~retired].sum() < (~retired).sum()  # the rule is exercised
    g = torch.Generator().manual_seed(5)
    case["samples"] = 0.1 * torch.randn(oc.SPLIT_N * int(split.sum()), 3, generator=g)
    optA = make_opt(case, dev, FusedAdam)
    optim.retire_rows(optA, keep.to(dev))
    case_r = dict(case, p=dict(case["p"], opacity=torch.where(keep[:, None], case["p"]["opacity"], torch.full((P, 1), optim.RETIRED_LOGIT))))
    gotA, idsA, infoA = one_pass(case_r, dev, case["samples"], opt=optA)
    fA = infoA.flags.cpu().numpy()
    assert not (fA[retired] & 3).any() and (fA[retired] & 4).all() and (fA[retired] & 8).all()  # never selected, always pruned
    assert not np.isin(idsA, np.nonzero(retired)[0]).any()
    optB = make_opt(case, dev, FusedAdam)
    optim.retire_rows(optB, keep.to(dev))
    statsB = [v.to(dev) for v in case["stats"].values()]
    _, extra = optim.prune_optimizer(optB, optim.alive_rows(optB), extra=statsB + [case["ids"].to(dev)])
    gotB, idsB, infoB = one_pass(case, dev, case["samples"], opt=optB, stats=dict(zip(oc.STATS, extra[:3])), ids=extra[3])
    assert (infoA.n_kept, infoA.n_kept_clones, infoA.n_split, infoA.n_kept_split) == (infoB.n_kept, infoB.n_kept_clones, infoB.n_split, infoB.n_kept_split)
    assert np.array_equal(idsA, idsB) and infoA.n_out == infoB.n_out > 0
    for n in oc.GROUPS:
        for a, b in zip(gotA[n], gotB[n]):
            assert a.tobytes() == b.tobytes(), n
    # and against the stepwise path on the compacted state, with the usual bound for the computed rows
    sub = {"P": int(keep.sum()), "sh": 0, "pattern": "alternating", "max_screen_size": case["max_screen_size"], "grad_threshold": THR,
           "p": {n: v[keep] for n, v in case["p"].items()}, "m": {n: v[keep] for n, v in case["m"].items()},
           "v": {n: v[keep] for n, v in case["v"].items()}, "stats": {k: v[keep] for k, v in case["stats"].items()},
           "ids": case["ids"][keep], "samples": case["samples"]}
    want, want_ids, want_masks = stepwise(sub, dev, case["samples"])
    worst = compare(sub, dev, gotB, idsB, infoB, want, want_ids, want_masks)
    print(f"retired rows: {infoA.n_out} rows, computed rows worst ratio {worst:.3f}")


# ---- 5. reproducibility and capture ----
def test_two_runs_give_the_same_bits(dev):
    case = make_case("alternating", 70_001, seed=6)
    from eogs2_amd.density import densify_and_prune
    from eogs2_amd.optim import FusedAdam

    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        opt = make_opt(case, dev, FusedAdam)
        _, _, info = densify_and_prune(opt, {k: v.to(dev) for k, v in case["stats"].items()}, grad_threshold=THR, screen_size_threshold=EXTENT,
                                       max_screen_size=20, scene_extent=EXTENT, extra=[case["ids"].to(dev)])
        runs.append((snapshot(opt), info.extra[0].cpu().numpy(), info.flags.cpu().numpy()))
    (a, ia, fa), (b, ib, fb) = runs
    assert np.array_equal(ia, ib) and np.array_equal(fa, fb) and len(ia) != case["P"]
    for n in oc.GROUPS:
        for x, y in zip(a[n], b[n]):
            assert x.tobytes() == y.tobytes(), n


def test_statistics_update_replays_in_a_graph(dev):
    from eogs2_amd.density import DensityStats

    P = 70_001
    ids = np.arange(P)
    inputs = [(oc.viewspace_grad(it, ids).to(dev), oc.radii(it, ids).to(torch.int32).to(dev)) for it in (1, 2, 3)]
    eager = DensityStats(P, dev)
    for vg, r in inputs:
        eager.update(vg, r)
    assert float(eager.denom.max()) >= 2 and float(eager.denom.min()) == 0
    graphed = DensityStats(P, dev)
    vg, r = torch.zeros(P, 3, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed.update(vg, r)  # warm-up: radius 0 everywhere, nothing changes
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.update(vg, r)
    assert not bool(graphed.denom.any())
    for vg_k, r_k in inputs:
        vg.copy_(vg_k)
        r.copy_(r_k)
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(graphed.tensors(), eager.tensors()):
        assert _bits(a) == _bits(b)


# ---- 6. the example ----
def test_example_densifies_and_reproduces(dev):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_synthetic
    finally:
        sys.path.pop(0)
    args = ["--gaussians", "20000", "--size", "128", "--iters", "60", "--densify-every", "20", "--quiet"]
    runs = []
    for extra in ([], [], ["--graph"]):
        first, last, n = train_synthetic.main(args + extra)
        runs.append((first, last, n, {k: v.numpy().tobytes() for k, v in train_synthetic.main.last_params.items()}))
        assert train_synthetic.main.last_params["xyz"].shape[0] == n
    first, last, n, _ = runs[0]
    print(f"example: {n} Gaussians from 20000, loss {first:.5f} -> {last:.5f}")
    assert n != 20000 and last < first
    assert runs[1] == runs[0]  # the same bits twice
    assert runs[2] == runs[0]  # and as a recorded graph
