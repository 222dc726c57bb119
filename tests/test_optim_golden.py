"""CPU: the optimizer / density-control fixtures (tests/golden/optim/*.npz, written by tests/golden/make_golden_optim.py from
the reference's own `GaussianModel`) against the parts of eogs2_amd/optim.py that are plain PyTorch.

* Integrity of the fixtures: size, keys, dtypes, and the margins the generator asserted, re-checked from the stored float64
  arrays: no thresholded quantity within 1e-3 relative of its threshold, so a mask recomputed anywhere is a condition on every
  row and not a tolerance.
* Replay on the CPU over a `torch.optim.Adam`: `prune_optimizer`, `densify_and_clone`, `densify_and_split`,
  `cat_tensors_to_optimizer`, `reset_opacity`, `build_rotation` with boolean indexing standing in for `compact_rows` (the
  one piece without a CPU path). Every array, `step` and the identity of the optimizer's state entries must equal the
  reference's fp32 result BIT FOR BIT; every mask recomputed with tests/optim_cases.py's restatement of the reference's
  expressions must equal the recorded one. `retire_rows` + `alive_rows` + `prune_optimizer` must give the direct prune.
* `_reference_densify`, the helper tests/test_gpu_optim.py compares the HIP path with, on the fixtures' inputs: it must
  return the reference's outputs.
* The derived one-step bound of fp32 Adam (optim_cases.adam_step_bound) asserted for `torch.optim.Adam` itself at factor 1
  over the whole grid, before tests/test_gpu_optim.py asks it of the kernel at factor 2.
* Where the reference's sources are present: the generator run again writes the committed arrays bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_cases as oc

GEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_optim.py")
NAMES = sorted(oc.CASES)


@pytest.fixture
def optim_cpu(monkeypatch):
    from eogs2_amd import optim

    monkeypatch.setattr(optim, "compact_rows", lambda mask, tensors: [t.detach()[mask.bool()] for t in tensors])
    return optim


def test_fixtures_present_and_small():
    assert sorted(f[:-4] for f in os.listdir(oc.GOLDEN_DIR) if f.endswith(".npz")) == NAMES
    for n in NAMES:
        assert os.path.getsize(oc.fixture_path(n)) < oc.MAX_FIXTURE_BYTES


@pytest.mark.parametrize("name", NAMES)
def test_fixture_layout(name):
    fx = oc.Fixture(name)
    ops = [s["op"] for s in fx.stages]
    want = []
    for op in fx.cfg["script"]:
        want += ["clone", "split", "prune"] if op[0] == "densify" else [op[0]]
    assert ops == want and fx.stages[0]["op"] == "steps"
    shp = oc.shapes(fx.cfg["sh"])
    for i in range(len(fx.stages) + 1):
        s = f"s{i}"
        rows = fx.z[f"{s}/ids"].shape[0]
        assert fx.z[f"{s}/ids"].dtype == np.int32 and fx.z[f"{s}/step"].dtype == np.int32 and fx.z[f"{s}/step"].shape == (6,)
        for n in oc.GROUPS:
            for k in "pmv":
                key = f"{s}/{n}/{k}"
                if i == 0 and k != "p":
                    assert not fx.has(key)  # no Adam state before the first step
                    continue
                assert fx.z[key].dtype == np.float32 and fx.z[key].shape == (rows,) + shp[n], key
        for k in oc.STATS:
            assert fx.z[f"{s}/{k}"].dtype == np.float32 and fx.z[f"{s}/{k}"].shape[0] == rows
    for st in fx.stages:
        if st["op"] == "steps":  # the truth beside every array an Adam stretch ends in
            for n in oc.GROUPS:
                for k in "pmv":
                    assert fx.z[f"{st['dst']}/{n}/{k}@64"].dtype == np.float64
        if "mask" in st:
            assert fx.z[st["mask"]].dtype == np.bool_ and fx.z[st["mask"]].shape == fx.z[f"{st['src']}/ids"].shape
        if st["op"] == "split":
            assert fx.z[st["normal"]].dtype == np.float32 and fx.z[st["normal"]].shape == (st["N"] * int(fx.z[st["mask"]].sum()), 3)
    assert fx.z["s0/ids"].tolist() == list(range(fx.cfg["P"]))


def test_fixtures_cover_what_they_are_for():
    sel = {n: {st["op"]: int(oc.Fixture(n).z[st["mask"]].sum()) for st in oc.Fixture(n).stages if "mask" in st} for n in NAMES}
    assert sel["prune_only"]["tprune"] > 10
    for n in ("densify", "densify_screen", "sh1"):
        assert sel[n]["clone"] > 3 and sel[n]["split"] > 10 and sel[n]["prune"] > 10, (n, sel[n])
    assert not any(sel["empty_masks"].values())
    assert oc.Fixture("sh1").z["s0/f_rest/p"].shape[1:] == (3, 3) and oc.Fixture("densify").z["s0/f_rest/p"].shape[1:] == (0, 3)
    screen = {n: [st["max_screen_size"] for st in oc.Fixture(n).stages if st["op"] == "prune"] for n in NAMES}
    assert screen["densify"] == [None] and screen["densify_screen"] == [20]
    # with a screen size set, the world-size clause removes rows the opacity clause alone would keep
    fx = oc.Fixture("densify_screen")
    st = next(s for s in fx.stages if s["op"] == "prune")
    alone = oc.final_prune_mask(fx.t(f"{st['src']}/opacity/p"), fx.t(f"{st['src']}/scaling/p"), fx.t(f"{st['src']}/max_radii2D"), None, 5.0)
    assert int(alone.sum()) < int(fx.z[st["mask"]].sum())
    # the reset caps some logits and keeps others
    fx = oc.Fixture("prune_only")
    st = next(s for s in fx.stages if s["op"] == "reset")
    capped = oc.stored_mask(fx, st)
    assert 10 < capped.sum() < capped.size - 10


@pytest.mark.parametrize("name", NAMES)
def test_margins_hold_in_float64(name):
    """From the stored float64 arrays: every thresholded quantity keeps 1e-3 relative from its threshold."""
    fx = oc.Fixture(name)
    cfg, pd_ext = fx.cfg, oc.TRAIN_ARGS["percent_dense"] * fx.cfg["extent"]
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    checked = 0
    for st in fx.stages:
        s = st["src"]
        if st["op"] == "steps":
            continue
        op64, sc64 = fx.z[f"{s}/opacity/p@64"], np.exp(fx.z[f"{s}/scaling/p@64"]).max(1)
        if st["op"] == "tprune":
            assert not oc.near(op64, oc.MIN_OPACITY).any()
        elif st["op"] == "reset":
            assert not oc.near(sig(op64), oc.RESET_CAP).any()
        elif st["op"] == "clone":
            with np.errstate(invalid="ignore", divide="ignore"):
                g = np.nan_to_num(fx.z[f"{s}/xyz_gradient_accum@64"] / fx.z[f"{s}/denom@64"], nan=0.0)
            assert not oc.near(g, cfg["grad_threshold"]).any() and not oc.near(sc64, pd_ext).any()
        elif st["op"] == "split":
            assert not oc.near(sc64, pd_ext).any()
        elif st["op"] == "prune":
            assert not oc.near(sig(op64), oc.DENSIFY_MIN_OPACITY).any()
            if st["max_screen_size"]:
                assert not oc.near(sc64, 0.1 * cfg["extent"]).any()
                assert not oc.near(fx.z[f"{s}/max_radii2D"], st["max_screen_size"]).any()
        else:
            continue
        checked += 1
    assert checked == sum(s["op"] != "steps" for s in fx.stages)


def test_hashed_gradients():
    """Exact in fp32, a function of the original id alone, half the rows zero, magnitudes over ten decades."""
    ids = np.arange(500)
    g = torch.cat([oc.hashed_grad(it, ids, "rotation") for it in range(1, 41)], 1)
    a = g.abs()[g != 0]
    assert float(a.min()) < 1e-8 and float(a.max()) > 1e2
    zero = (torch.cat([oc.hashed_grad(it, ids, "xyz") for it in range(1, 41)], 1) == 0).float().mean()
    assert 0.45 < float(zero) < 0.55
    perm = np.random.default_rng(0).permutation(500)[:77]
    for n in oc.GROUPS:
        assert torch.equal(oc.hashed_grad(7, perm, n, sh=1), oc.hashed_grad(7, ids, n, sh=1)[perm])
    rows_zero = [(oc.hashed_grad(3, ids, n, sh=1).reshape(500, -1) == 0).all(1) for n in oc.GROUPS]
    assert all(torch.equal(rows_zero[0], r) for r in rows_zero) and torch.equal(rows_zero[0], oc.radii(3, ids) == 0)


@pytest.mark.parametrize("name", NAMES)
def test_cpu_replay_is_bit_equal_to_the_reference(name, optim_cpu):
    oc.replay(oc.Fixture(name), "cpu", torch.optim.Adam, optim_cpu, exact=True)


@pytest.mark.parametrize("name", NAMES)
def test_retire_then_compact_equals_the_prune(name, optim_cpu):
    """`retire_rows` now, `prune_optimizer(alive_rows())` later: the rows and state of the reference's immediate prune."""
    fx = oc.Fixture(name)
    for st in fx.stages:
        if st["op"] != "tprune":
            continue
        opt = oc.make_optimizer(fx, st["src"], torch.optim.Adam)
        mask = fx.t(st["mask"])
        optim_cpu.retire_rows(opt, ~mask)
        assert torch.equal(optim_cpu.alive_rows(opt), ~mask)
        optim_cpu.prune_optimizer(opt, optim_cpu.alive_rows(opt))
        for g in opt.param_groups:
            p = g["params"][0]
            for k, got in (("p", p.detach()), ("m", opt.state[p]["exp_avg"]), ("v", opt.state[p]["exp_avg_sq"])):
                assert got.numpy().tobytes() == fx.z[f"{st['dst']}/{g['name']}/{k}"].tobytes(), (g["name"], k)


@pytest.mark.parametrize("name", NAMES)
def test_reference_densify_helper_gives_the_reference(name):
    """tests/test_gpu_optim.py's `_reference_densify` on the fixture's inputs returns the fixture's outputs."""
    from test_gpu_optim import _reference_densify

    fx = oc.Fixture(name)
    for st in fx.stages:
        if st["op"] not in ("clone", "split"):
            continue
        opt = oc.make_optimizer(fx, st["src"], torch.optim.Adam)
        split = st["op"] == "split"
        with oc.normal_returns(fx.t(st["normal"]) if split else torch.zeros(0, 3)):
            out, radii = _reference_densify(opt, fx.t(st["mask"]), split, oc.SPLIT_N, fx.t(st["radii"]))
        assert radii.numpy().tobytes() == fx.z[st["tmp_radii"]].tobytes()
        for n in oc.GROUPS:
            for k, got in zip("pmv", out[n]):
                assert got.detach().numpy().tobytes() == fx.z[f"{st['dst']}/{n}/{k}"].tobytes(), (name, st["op"], n, k)


@pytest.mark.parametrize("eps", oc.ADAM_GRID_EPS)
@pytest.mark.parametrize("step", oc.ADAM_GRID_STEPS)
def test_torch_adam_stays_inside_the_one_step_bound(step, eps):
    worst = [0.0, 0.0, 0.0]
    for gscale in oc.ADAM_GRID_GSCALE:
        r = oc.adam_check_one_step(torch.optim.Adam, "cpu", step, gscale, eps, oc.FACTOR_TORCH)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"step {step} eps {eps:g}: worst error / bound m {worst[0]:.3f} v {worst[1]:.3f} p {worst[2]:.3f}")


def test_one_step_bound_is_sharp_enough_to_bite():
    """The bound is no blanket: an update with 1 - beta2 swapped for 1 - beta1, with float bias corrections at step 5000, or
    with eps divided by sqrt(bc2) too leaves it by a wide margin somewhere on the grid."""
    def worst(mutate):
        w = 0.0
        for step in oc.ADAM_GRID_STEPS:
            for gscale in (1e-12, 1.0):
                for eps in oc.ADAM_GRID_EPS:
                    p, g, m, v = oc.adam_grid_state(gscale, seed=step)
                    b1, b2 = oc.BETAS
                    want = oc.adam_step_f64(p, g, m, v, 1e-2, oc.BETAS, eps, step)
                    bm, bv, bp = oc.adam_step_bound(p, g, m, v, 1e-2, oc.BETAS, eps, step)
                    P, G, M, V = (x.double() for x in (p, g, m, v))
                    m2 = M + (1 - b1) * (G - M)
                    v2 = b2 * V + (mutate.get("w2", 1 - b2)) * G * G
                    if mutate.get("float_bc"):
                        bc1 = float(1 - torch.tensor(b1, dtype=torch.float32) ** step)
                        bc2 = float(1 - torch.tensor(b2, dtype=torch.float32) ** step)
                    else:
                        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
                    d = (v2.sqrt() + eps) / bc2 ** 0.5 if mutate.get("eps_scaled") else v2.sqrt() / bc2 ** 0.5 + eps
                    p2 = P - 1e-2 / bc1 * m2 / d
                    w = max(w, float(((v2 - want[2]).abs() / bv).max()), float(((p2 - want[0]).abs() / bp).max()))
        return w

    assert worst({}) < 1e-6
    assert worst({"w2": 1 - oc.BETAS[0]}) > 100
    assert worst({"float_bc": True}) > 2 * oc.FACTOR_KERNEL
    assert worst({"eps_scaled": True}) > 2 * oc.FACTOR_KERNEL


def test_fixtures_regenerate_bit_for_bit(tmp_path):
    """The generator, run again, writes the committed arrays bit for bit (where the reference's sources are present)."""
    sys.path.insert(0, os.path.dirname(GEN))
    try:
        import make_golden_optim as gen
    finally:
        sys.path.remove(os.path.dirname(GEN))
    if not os.path.isdir(gen.REFROOT):
        pytest.skip("the reference's sources are not on this machine")
    subprocess.run([sys.executable, GEN, "--out", str(tmp_path)], check=True, timeout=900)
    for n in NAMES:
        a, b = np.load(oc.fixture_path(n)), np.load(tmp_path / (n + ".npz"))
        assert sorted(a.files) == sorted(b.files), n
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{n}:{k}"


@pytest.mark.parametrize("name", ["densify", "densify_screen", "sh1"])
def test_tie_rows_sit_on_the_gradient_threshold(name):
    """Rows whose mean gradient norm IS the threshold, in fp32 and in float64: selected by the reference (`>=`), so a
    recomputed mask with `>` differs from the stored one."""
    fx = oc.Fixture(name)
    st = next(s for s in fx.stages if s["op"] == "clone")
    s = st["src"]
    g32 = oc.mean_grads(fx.t(f"{s}/xyz_gradient_accum"), fx.t(f"{s}/denom")).numpy()[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        g64 = (fx.z[f"{s}/xyz_gradient_accum@64"] / fx.z[f"{s}/denom@64"])[:, 0]
    tie = g32 == np.float32(oc.TIE_GRAD)
    assert tie.sum() >= 4 and np.array_equal(tie, g64 == oc.TIE_GRAD)
    split = next(x for x in fx.stages if x["op"] == "split")
    picked = fx.z[st["mask"]][tie].sum() + fx.z[split["mask"]][:tie.size][tie].sum()
    assert picked == tie.sum()  # every tie row is cloned or split: the reference reads the threshold as inclusive
