"""GPU (MI355X): multi-tensor Adam and row compaction (include/eogs_optim.h, eogs2_amd/optim.py) against PyTorch's own
`torch.optim.Adam` and boolean-mask indexing — the two things the reference uses (gaussian_model.py:228-262,466-505)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (0, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def _groups(P, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"params": [torch.nn.Parameter(torch.randn((P,) + s, generator=g).to(device))], "lr": LRS[n], "name": n}
            for n, s in SHAPES.items()]


@pytest.mark.parametrize("P", [1, 1023, 50_001])
def test_fused_adam_matches_torch_adam(dev, P):
    from eogs2_amd.optim import FusedAdam

    ref = torch.optim.Adam(_groups(P, "cpu"), lr=0.0, eps=1e-15)  # the reference's constructor call
    ours = FusedAdam(_groups(P, dev), lr=0.0, eps=1e-15)
    g = torch.Generator().manual_seed(1)
    for it in range(6):
        for gr, go in zip(ref.param_groups, ours.param_groups):
            grad = torch.randn(gr["params"][0].shape, generator=g) * (10.0 ** (it - 3))
            grad[::2] = 0.0  # Gaussians no view touched this iteration
            gr["params"][0].grad = grad
            go["params"][0].grad = grad.to(dev)
        if it == 3:  # the reference changes learning rates between steps (update_learning_rate)
            ref.param_groups[0]["lr"] = ours.param_groups[0]["lr"] = 3e-5
        ref.step()
        ours.step()
    for gr, go in zip(ref.param_groups, ours.param_groups):
        pr, po = gr["params"][0], go["params"][0]
        # fp32 on both sides, identical formula; rounding differs in lerp / division: 2e-6 of the tensor's scale
        close = lambda a, b: b.numel() == 0 or bool(((a - b).abs() <= 2e-6 * b.abs().max().clamp_min(1e-30)).all())
        assert close(po.detach().cpu(), pr.detach()), gr["name"]
        if pr.numel():
            for k in ("exp_avg", "exp_avg_sq"):
                assert close(ours.state[po][k].cpu(), ref.state[pr][k]), (gr["name"], k)
            assert int(ours.state[po]["step"]) == int(ref.state[pr]["step"]) == 6


@pytest.mark.parametrize("N,frac", [(1, 1.0), (255, 0.5), (256, 0.0), (100_003, 0.9), (70_000, 0.01), (4096, 1.0)])
def test_compact_rows_equals_boolean_indexing(dev, N, frac):
    from eogs2_amd.optim import compact_rows

    g = torch.Generator().manual_seed(N)
    mask = (torch.rand(N, generator=g) < frac).to(dev)
    tensors = [torch.randn(N, 3, generator=g).to(dev), torch.randn(N, 1, 3, generator=g).to(dev),
               torch.randn(N, 0, 3).to(dev), torch.randn(N, generator=g).to(dev),
               torch.randint(0, 1000, (N, 4), generator=g, dtype=torch.int32).to(dev),
               torch.randn(N, 14, generator=g).to(dev)[:, ::2]]  # a strided view: made contiguous like tensor[mask] would
    out = compact_rows(mask, tensors)
    for o, t in zip(out, tensors):
        assert o.shape == t[mask].shape and torch.equal(o, t[mask])


def test_prune_optimizer_keeps_training_state(dev):
    """Same result as the reference's per-tensor `_prune_optimizer` / `prune_points`, then the optimizer keeps stepping."""
    from eogs2_amd.optim import FusedAdam, prune_optimizer

    P = 10_000
    opt = FusedAdam(_groups(P, dev, seed=3), lr=0.0, eps=1e-15)
    g = torch.Generator().manual_seed(4)
    for gr in opt.param_groups:
        gr["params"][0].grad = torch.randn(gr["params"][0].shape, generator=g).to(dev)
    opt.step()
    keep = (torch.rand(P, generator=g) < 0.7).to(dev)
    before = {gr["name"]: (gr["params"][0].detach().clone(), {k: v.clone() for k, v in opt.state[gr["params"][0]].items()})
              for gr in opt.param_groups}
    accum, radii = torch.rand(P, 1, generator=g).to(dev), torch.rand(P, generator=g).to(dev)
    tensors, (accum2, radii2) = prune_optimizer(opt, keep, extra=(accum, radii))
    assert torch.equal(accum2, accum[keep]) and torch.equal(radii2, radii[keep])
    for gr in opt.param_groups:
        p = gr["params"][0]
        assert tensors[gr["name"]] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad
        p0, st0 = before[gr["name"]]
        assert torch.equal(p.detach(), p0[keep])
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], st0["exp_avg"][keep]) and torch.equal(st["exp_avg_sq"], st0["exp_avg_sq"][keep])
        assert int(st["step"]) == 1 and len(opt.state) == len(opt.param_groups)
        p.grad = torch.ones_like(p)
    opt.step()
    assert all(int(opt.state[gr["params"][0]]["step"]) == 2 for gr in opt.param_groups)


def test_reset_opacity_caps_logits_and_restarts_moments(dev):
    """gaussian_model.py:347-352,451-464: opacities above 0.01 are capped, smaller ones kept, the group's Adam moments
    restart at zero under a new Parameter, every other group is untouched, and the optimizer keeps stepping."""
    from eogs2_amd.optim import FusedAdam, reset_opacity

    P = 5_000
    opt = FusedAdam(_groups(P, dev, seed=5), lr=0.0, eps=1e-15)
    for gr in opt.param_groups:
        gr["params"][0].grad = torch.ones_like(gr["params"][0])
    opt.step()
    others = {gr["name"]: gr["params"][0] for gr in opt.param_groups if gr["name"] != "opacity"}
    old = next(gr["params"][0] for gr in opt.param_groups if gr["name"] == "opacity").detach().clone()
    out = reset_opacity(opt)
    new = next(gr["params"][0] for gr in opt.param_groups if gr["name"] == "opacity")
    assert out["opacity"] is new and new.requires_grad and len(opt.state) == len(opt.param_groups)
    expect = torch.min(torch.sigmoid(old), torch.full_like(old, 0.01))
    assert torch.allclose(torch.sigmoid(new.detach()), expect, rtol=1e-5, atol=1e-8)
    assert float(torch.sigmoid(new.detach()).max()) <= 0.01 * (1 + 1e-5)
    st = opt.state[new]
    assert float(st["exp_avg"].abs().max()) == 0.0 and float(st["exp_avg_sq"].abs().max()) == 0.0 and int(st["step"]) == 1
    for gr in opt.param_groups:
        if gr["name"] != "opacity":
            assert gr["params"][0] is others[gr["name"]]
        gr["params"][0].grad = torch.ones_like(gr["params"][0])
    opt.step()
    assert int(opt.state[new]["step"]) == 2


def test_grad_bucket_pack_kernel_equals_cat(dev):
    """The data-parallel bucket's blocks against torch.cat over the same column slices (the partially bucketed colour
    block goes through eogs_pack_columns), and both directions of that C-ABI call against slicing."""
    import ctypes

    from eogs2_amd import _lib
    from eogs2_amd._abi import PackTensor
    from eogs2_amd.parallel import GradBucket

    P = 70_001
    g = torch.Generator().manual_seed(11)
    widths, cols = (3, 5, 1, 3, 4), [slice(0, 3), slice(0, 3), slice(0, 1), slice(0, 3), slice(0, 4)]
    params = [torch.zeros(P, w, device=dev, requires_grad=True) for w in widths]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    want = torch.cat([p.grad[:, c] for p, c in zip(params, cols)], dim=1)
    # the bucket: one contiguous [P, k] block per parameter (the colour block is filled by eogs_pack_columns)
    b = GradBucket(params, cols=cols)
    assert b.bytes_per_gaussian == 56
    b.pack()
    o = 0
    for i, c in enumerate(cols):
        n = c.stop - c.start
        assert torch.equal(b.block(i), want[:, o:o + n]), i
        o += n
    b.unpack()  # no process group: the sums are the gradients themselves
    for i, (p, c) in enumerate(zip(params, cols)):
        assert b._is_block(p.grad, i) == (i != 1)
    assert torch.equal(torch.cat([p.grad[:, c] for p, c in zip(params, cols)], dim=1), want)
    # a missing gradient counts as zeros
    params[2].grad = None
    b2 = GradBucket(params, cols=cols)
    b2.pack()
    assert float(b2.block(2).abs().max()) == 0.0 and torch.equal(b2.block(4), want[:, 10:14])
    # unpack direction of the C-ABI
    abi = _lib.get()
    outs = [torch.full((P, w), 7.0, device=dev) for w in widths]
    arr = (PackTensor * 5)()
    for a, o, c in zip(arr, outs, cols):
        a.data, a.width, a.col0, a.ncols = o.data_ptr(), o.shape[1], c.start, c.stop - c.start
    abi.check(abi.pack_columns(P, 5, ctypes.cast(arr, ctypes.c_void_p), ctypes.c_void_p(want.data_ptr()), 14, 1,
                               ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    o = 0
    for out, c, w in zip(outs, cols, widths):
        n = c.stop - c.start
        assert torch.equal(out[:, c], want[:, o:o + n])
        if n < w:
            assert torch.equal(out[:, n:], torch.full((P, w - n), 7.0, device=dev))  # other columns untouched
        o += n


def _reference_densify(opt, mask, split, N, tmp_radii):
    """gaussian_model.py:507-660 in plain PyTorch ops (boolean-mask indexing, torch.cat), on this optimizer."""
    from eogs2_amd.optim import build_rotation

    par = {g["name"]: g["params"][0] for g in opt.param_groups}
    if split:
        stds = torch.exp(par["scaling"])[mask].repeat(N, 1)
        samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=stds.device), std=stds)
        rots = build_rotation(par["rotation"][mask]).repeat(N, 1, 1)
        new = {"xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + par["xyz"][mask].repeat(N, 1),
               "scaling": torch.log(torch.exp(par["scaling"])[mask].repeat(N, 1) / (0.8 * N)),
               "rotation": par["rotation"][mask].repeat(N, 1), "f_dc": par["f_dc"][mask].repeat(N, 1, 1),
               "f_rest": par["f_rest"][mask].repeat(N, 1, 1), "opacity": par["opacity"][mask].repeat(N, 1)}
        radii = torch.cat((tmp_radii, tmp_radii[mask].repeat(N)))
    else:
        new = {n: par[n][mask] for n in par}
        radii = torch.cat((tmp_radii, tmp_radii[mask]))
    out = {}
    for g in opt.param_groups:  # cat_tensors_to_optimizer
        p, ext = g["params"][0], new[g["name"]]
        st = opt.state[p]
        out[g["name"]] = (torch.cat((p.data, ext)), torch.cat((st["exp_avg"], torch.zeros_like(ext))),
                          torch.cat((st["exp_avg_sq"], torch.zeros_like(ext))))
    if split:  # prune_points(cat(mask, zeros))
        keep = ~torch.cat((mask, torch.zeros(N * int(mask.sum()), dtype=torch.bool, device=mask.device)))
        out = {n: tuple(t[keep] for t in v) for n, v in out.items()}
    return out, radii


@pytest.mark.parametrize("split", [False, True])
def test_densify_clone_and_split_match_reference_ops(dev, split):
    """Clone / split densification (gaussian_model.py:573-660; off by default in the reference) through the compaction
    primitives: same tensors, same moments, same random draw as the reference's op sequence."""
    from eogs2_amd.optim import FusedAdam, densify_and_clone, densify_and_split

    P, N = 20_000, 2
    opt = FusedAdam(_groups(P, dev, seed=5), lr=0.0, eps=1e-15)
    g = torch.Generator().manual_seed(6)
    for gr in opt.param_groups:
        gr["params"][0].grad = torch.randn(gr["params"][0].shape, generator=g).to(dev)
    opt.step()
    mask = (torch.rand(P, generator=g) < 0.15).to(dev)
    radii = torch.rand(P, generator=g).to(dev)
    torch.manual_seed(123)
    want, want_radii = _reference_densify(opt, mask, split, N, radii)
    torch.manual_seed(123)
    if split:
        params, got_radii, keep = densify_and_split(opt, mask, N=N, tmp_radii=radii)
        assert int(keep.sum()) == P - int(mask.sum()) + N * int(mask.sum())
    else:
        params, got_radii = densify_and_clone(opt, mask, tmp_radii=radii)
    assert torch.equal(got_radii, want_radii)
    for gr in opt.param_groups:
        p = gr["params"][0]
        st = opt.state[p]
        w = want[gr["name"]]
        assert params[gr["name"]] is p and p.requires_grad and tuple(p.shape) == tuple(w[0].shape)
        assert torch.equal(p.detach(), w[0]) and torch.equal(st["exp_avg"], w[1]) and torch.equal(st["exp_avg_sq"], w[2])
        p.grad = torch.ones_like(p)
    opt.step()  # training goes on over the new rows
    assert all(int(opt.state[gr["params"][0]]["step"]) == 2 for gr in opt.param_groups)


def test_retired_rows_render_nothing_and_stay_retired(dev):
    """`retire_rows` (the deferred prune): a retired Gaussian is listed nowhere and gets zero gradients, the survivors' render and
    gradients are those of the compacted model bit for bit, FusedAdam steps with momentum in the retired rows leave them retired,
    and `prune_optimizer(alive_rows())` removes exactly them."""
    from eogs2_amd.fused import rasterize_raw
    from eogs2_amd.optim import RETIRED_LOGIT, FusedAdam, alive_rows, prune_optimizer, retire_rows
    from eogs2_amd.synthetic import make_scene, settings_for

    P, H, W = 20000, 160, 192
    sc = make_scene(P, H, W, seed=5, opacity="trained", device=dev)
    rs, alt = settings_for(sc, H, W), sc["viewmatrix"][:, 2].contiguous()
    dL = torch.randn(5, H, W, device=dev) / (H * W)
    names = ("xyz", "f_dc", "opacity", "scaling", "rotation")
    init = dict(xyz=sc["means3D"], f_dc=torch.logit(sc["colors"][:, :3].clamp(0.01, 0.99)).reshape(P, 1, 3),
                opacity=torch.logit(sc["opacities"].clamp(1e-4, 1 - 1e-4)), scaling=sc["scales"].log(), rotation=sc["rotations"])
    opt = FusedAdam([{"params": [torch.nn.Parameter(init[n].clone())], "lr": 1e-2, "name": n} for n in names], lr=0.0, eps=1e-15)

    def params():
        return {g["name"]: g["params"][0] for g in opt.param_groups}

    def fwd_bwd(p):
        for t in p.values():
            t.grad = None
        m2 = torch.zeros_like(p["xyz"], requires_grad=True)
        color, radii, _ = rasterize_raw(p["xyz"], m2, p["f_dc"], p["opacity"], p["scaling"], p["rotation"], alt, rs)
        torch.autograd.backward([color], [dL])
        return color.detach().clone()

    fwd_bwd(params())
    opt.step()  # every row now carries Adam momentum
    keep = torch.rand(P, generator=torch.Generator().manual_seed(3)).to(dev) > 0.3
    retire_rows(opt, keep)
    p = params()
    assert bool((p["opacity"].view(-1)[~keep] == RETIRED_LOGIT).all()) and bool(torch.equal(alive_rows(opt), keep))
    color = fwd_bwd(p)
    for n in names:
        assert float(p[n].grad[~keep].abs().max()) == 0.0, n
    # the compacted model: same image, same gradients in the surviving rows
    compact = {n: torch.nn.Parameter(p[n].detach()[keep].clone()) for n in names}
    color_c = fwd_bwd(compact)
    assert torch.equal(color, color_c)
    for n in names:
        assert torch.equal(p[n].grad[keep], compact[n].grad), n
    for _ in range(5):  # momentum from before the retirement, zero gradients since
        opt.step()
    assert bool(torch.equal(alive_rows(opt), keep))
    new, _ = prune_optimizer(opt, alive_rows(opt))
    assert new["xyz"].shape[0] == int(keep.sum())
    assert torch.isfinite(new["opacity"]).all()


def test_sum_into_equals_the_sequence_of_adds(dev):
    """eogs_sum_into (include/eogs_optim.h): dst += s0; dst += s1; ... for several tensors in one launch — the additions autograd
    makes render by render, bit for bit, odd sizes and unaligned views included; `Branches.run(shared=...)` sums its pieces with it."""
    from eogs2_amd.optim import sum_into_

    g = torch.Generator(device="cpu").manual_seed(3)
    shapes = [(1000, 3), (1000, 1, 3), (1000, 1), (777, 4), (5,), (0, 3)]
    base = [torch.randn(s, generator=g).to(dev) for s in shapes]
    srcs = [[torch.randn(s, generator=g).to(dev) * (10.0 ** j) for s in shapes] for j in range(3)]
    # an unaligned destination / source (a view one float into a larger buffer): the scalar path
    big = torch.randn(4001, generator=g).to(dev)
    base.append(big[1:])
    for j in range(3):
        srcs[j].append(torch.randn(4003, generator=g).to(dev)[3:])
    want = [b.clone() for b in base]
    for s in srcs:
        for w, x in zip(want, s):
            w.add_(x)
    got = [b.clone() for b in base[:-1]] + [big.clone()[1:]]
    sum_into_(got, srcs)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError):
        sum_into_([base[0]], [[base[3]]])  # sizes differ
    sum_into_([], [])  # nothing to do


# ---- the reference's own lifecycle (tests/golden/optim/*.npz, from its GaussianModel) ----
import numpy as np  # noqa: E402

import optim_cases as oc  # noqa: E402


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_lifecycle_matches_the_reference_fixture(dev, name):
    """Every stage of the fixture on the device with FusedAdam, prune_optimizer, densify_and_clone, densify_and_split and
    reset_opacity, fed the hashed gradients, the stored masks and the recorded normal draw (optim_cases.replay).

    Structural stages run on the fixture's pre-stage state. What they only move (kept and cloned rows, both moments, the zero
    moments of new rows, step, the id column, the statistics, the repeated rows of a split) equals the reference bit for bit;
    a split's new positions and log-scales and the reset's logits go through exp / log / sigmoid / a 3x3 product and are held to
    the fixture's float64 arrays within max(4 x the reference's own fp32-to-float64 distance for the array, 4 ulp). Adam
    stretches are held to the float64 arrays within max(2e-6 of the tensor's scale, 4 x that distance) per tensor. Every
    mask recomputed from the device-side state equals the stored one on every row."""
    from eogs2_amd import optim

    log = []
    try:
        oc.replay(oc.Fixture(name), dev, optim.FusedAdam, optim, exact=False, log=log)
    finally:
        print("\n".join(log))


# ---- one step from a given state, every element against float64 ----
def _checked_step(opt, factor=oc.FACTOR_KERNEL):
    """One `opt.step()`; every element of every parameter and moment against torch's formula in float64 from the state the
    device held before the step, within `factor` x optim_cases.adam_step_bound. A parameter without a gradient keeps its bits
    and its step."""
    pre = []
    for g in opt.param_groups:
        for p in g["params"]:
            st = opt.state.get(p) or {}
            z = torch.zeros(p.shape)
            pre.append((g, p, p.detach().cpu().clone(), None if p.grad is None else p.grad.detach().cpu().clone(),
                        st["exp_avg"].cpu().clone() if st else z, st["exp_avg_sq"].cpu().clone() if st else z.clone(),
                        int(st["step"]) if st else 0))
    opt.step()
    worst = 0.0
    for g, p, p0, g0, m0, v0, t0 in pre:
        st = opt.state.get(p) or {}
        if g0 is None:
            assert torch.equal(p.detach().cpu(), p0) and (int(st["step"]) if st else 0) == t0
            if st:
                assert torch.equal(st["exp_avg"].cpu(), m0) and torch.equal(st["exp_avg_sq"].cpu(), v0)
            continue
        assert int(st["step"]) == t0 + 1
        args = (p0, g0, m0, v0, float(g["lr"]), g["betas"], g["eps"], t0 + 1)
        want, bound = oc.adam_step_f64(*args), oc.adam_step_bound(*args)
        for what, got, w, b in (("exp_avg", st["exp_avg"], want[1], bound[0]), ("exp_avg_sq", st["exp_avg_sq"], want[2], bound[1]),
                                ("param", p.detach(), want[0], bound[2])):
            if not w.numel():
                continue
            r = (got.cpu().double() - w).abs() / b
            worst = max(worst, float(r.max()))
            assert float(r.max()) <= factor, (g.get("name"), what, int(r.argmax()), float(r.max()))
        if float(g["lr"]) == 0.0:
            assert torch.equal(p.detach().cpu(), p0)
    return worst


@pytest.mark.parametrize("eps", oc.ADAM_GRID_EPS)
@pytest.mark.parametrize("step", oc.ADAM_GRID_STEPS)
def test_fused_adam_one_step_elementwise(dev, step, eps):
    """The grid of optim_cases: step 1..30000 (bias corrections), |g| from 1e-20 (g^2 subnormal) to 1e15, a third of the
    gradients zero, moments from zero to 1e3 x the gradient scale, both eps. Bound: optim_cases.adam_step_bound, derived
    from the roundings of the formula, x FACTOR_KERNEL = 2 (the kernel's constants are rounded to fp32 before the launch)."""
    from eogs2_amd.optim import FusedAdam

    worst = [0.0, 0.0, 0.0]
    for gscale in oc.ADAM_GRID_GSCALE:
        r = oc.adam_check_one_step(FusedAdam, dev, step, gscale, eps, oc.FACTOR_KERNEL)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"step {step} eps {eps:g}: worst error / bound m {worst[0]:.3f} v {worst[1]:.3f} p {worst[2]:.3f}")


def test_fused_adam_squared_gradient_overflow(dev):
    """|g| = 1e20: g^2 overflows fp32. Like torch.optim.Adam in fp32 on the device the reference trains on (its kernels
    square the gradient before they scale it by 1 - beta2): v = +inf, the update 0, the parameter's bits unchanged, on both
    sides. (torch's CPU kernel scales first, (1 - beta2) g g = 1e37, and does not overflow here; it is not the comparison.)"""
    from eogs2_amd.optim import FusedAdam

    p, g, m, v = oc.adam_grid_state(1.0, n=1029, seed=3)
    g = torch.where(torch.arange(1029) % 2 == 0, 1e20, -1e20).float()
    out = []
    for cls in (torch.optim.Adam, FusedAdam):
        par = torch.nn.Parameter(p.clone().to(dev))
        opt = cls([{"params": [par], "lr": 1e-2}], lr=0.0, eps=1e-15)
        opt.state[par] = {"step": torch.tensor(9.0), "exp_avg": m.clone().to(dev), "exp_avg_sq": v.clone().to(dev)}
        par.grad = g.clone().to(dev)
        opt.step()
        assert int(opt.state[par]["step"]) == 10
        out.append((par.detach().cpu(), opt.state[par]["exp_avg"].cpu(), opt.state[par]["exp_avg_sq"].cpu()))
    (pr, mr, vr), (po, mo, vo) = out
    assert torch.equal(pr, p) and torch.equal(po, p)
    assert bool(torch.isposinf(vr).all()) and bool(torch.isposinf(vo).all())
    assert bool(((mo.double() - mr.double()).abs() <= 4 * oc.U * mr.double().abs()).all())


def _plain(sizes, d, seed=0, **group_kw):
    g = torch.Generator().manual_seed(seed)
    return [dict({"params": [torch.nn.Parameter(torch.randn(n, generator=g).to(d))], "lr": 1e-2 * (1 + i % 3), "name": f"t{i}"},
                 **{k: v[i % len(v)] for k, v in group_kw.items()}) for i, n in enumerate(sizes)]


def _rand_grads(opt, gen, scale=1.0, skip=()):
    for i, gr in enumerate(opt.param_groups):
        p = gr["params"][0]
        p.grad = None if i in skip else (torch.randn(p.shape, generator=gen) * scale + 0.01).to(p.device)


@pytest.mark.parametrize("numel", [1, 3, 4, 5, 1023, 1024, 1025, 4097])
def test_fused_adam_vector_path_tail_and_workgroup_edge(dev, numel):
    from eogs2_amd.optim import FusedAdam

    opt = FusedAdam(_plain([numel], dev, seed=numel), lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(numel + 1)
    for it in range(4):
        _rand_grads(opt, gen, 10.0 ** (it - 2))
        _checked_step(opt)


@pytest.mark.parametrize("off_p,off_g,off_m,off_v", [(1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (1, 2, 3, 1), (3, 3, 3, 3)])
def test_fused_adam_unaligned_views_touch_nothing_else(dev, off_p, off_g, off_m, off_v):
    """Parameter, gradient or moments that start one, two or three floats into a larger buffer (the scalar path): right
    values, and the guard values either side of every buffer stay as they were."""
    from eogs2_amd.optim import FusedAdam

    n, pad, guard = 1030, 8, 12345.0
    gen = torch.Generator().manual_seed(off_p * 64 + off_g * 16 + off_m * 4 + off_v)
    bufs = {}
    for k, off in (("p", off_p), ("g", off_g), ("m", off_m), ("v", off_v)):
        b = torch.full((n + 2 * pad,), guard)
        x = torch.randn(n, generator=gen)
        b[pad + off:pad + off + n] = x.abs() if k == "v" else x
        bufs[k] = (b.to(dev), off)
    view = lambda k: bufs[k][0][pad + bufs[k][1]:pad + bufs[k][1] + n]
    par = torch.nn.Parameter(view("p"))
    assert par.data_ptr() == view("p").data_ptr()
    opt = FusedAdam([{"params": [par], "lr": 1e-2, "name": "x"}], lr=0.0, eps=1e-15)
    opt.state[par] = {"step": torch.tensor(3.0), "exp_avg": view("m"), "exp_avg_sq": view("v")}
    for _ in range(2):
        view("g").copy_(torch.randn(n, generator=gen).to(dev) + 0.01)
        par.grad = view("g")
        _checked_step(opt)
    for k, (b, off) in bufs.items():
        outside = torch.cat((b[:pad + off], b[pad + off + n:]))
        assert bool((outside == guard).all()), k
    assert opt.state[par]["exp_avg"].data_ptr() == view("m").data_ptr()


@pytest.mark.parametrize("n_groups", [17, 33])
def test_fused_adam_more_tensors_than_one_launch(dev, n_groups):
    """More single-tensor groups than EOGS_ADAM_MAX_TENSORS = 16 in one step(), mixed sizes, empty tensors in the middle."""
    from eogs2_amd.optim import FusedAdam

    sizes = [(5, 0, 1024, 3, 4097, 0, 1, 70_001, 256, 1025, 2)[i % 11] for i in range(n_groups)]
    opt = FusedAdam(_plain(sizes, dev, seed=n_groups), lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        _rand_grads(opt, gen)
        _checked_step(opt)
    assert all(int(opt.state[g["params"][0]]["step"]) == 3 for g in opt.param_groups)


def test_fused_adam_groups_with_their_own_betas_eps_and_steps(dev):
    """Two betas and two eps in one optimizer; a parameter without a gradient stays untouched with its step not advanced,
    so groups sit at different steps; a learning rate changed between steps; a group with lr 0 (bits unchanged, moments
    advance); a non-contiguous gradient."""
    from eogs2_amd.optim import FusedAdam

    groups = _plain([1000, 1000, 777, 777, 4099, 64], dev, seed=8, betas=[(0.9, 0.999), (0.8, 0.99)], eps=[1e-15, 1e-15, 1e-8])
    groups[5]["lr"] = 0.0
    opt = FusedAdam(groups, lr=0.0)
    gen = torch.Generator().manual_seed(9)
    for it in range(5):
        _rand_grads(opt, gen, skip=(2,) if it in (1, 2) else (4,) if it == 3 else ())
        wide = torch.randn(1000, 2, generator=gen).to(dev)
        opt.param_groups[1]["params"][0].grad = wide[:, 0]
        assert not wide[:, 0].is_contiguous()
        if it == 2:
            opt.param_groups[0]["lr"] = 3e-5
        m_before = opt.state[opt.param_groups[5]["params"][0]]["exp_avg"].clone() if it else None
        _checked_step(opt)
        if it:
            assert not torch.equal(m_before, opt.state[opt.param_groups[5]["params"][0]]["exp_avg"])
    assert [int(opt.state[g["params"][0]]["step"]) for g in opt.param_groups] == [5, 5, 3, 5, 4, 5]


@pytest.mark.parametrize("kw", [{"amsgrad": True}, {"weight_decay": 0.1}, {"maximize": True}])
def test_fused_adam_refuses_what_it_does_not_implement(dev, kw):
    from eogs2_amd.optim import FusedAdam

    opt = FusedAdam(_plain([8], dev), lr=0.0)
    opt.param_groups[0].update(kw)
    opt.param_groups[0]["params"][0].grad = torch.ones(8, device=dev)
    with pytest.raises(NotImplementedError):
        opt.step()


def test_fused_adam_headline_size(dev):
    """The six groups at P = 1,048,576, three steps: thousands of workgroups per tensor through the first_block table."""
    from eogs2_amd.optim import FusedAdam

    opt = FusedAdam(_groups(1_048_576, dev, seed=2), lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        _rand_grads(opt, gen, 1e-3)
        _checked_step(opt)


# ---- compaction ----
def _keep_pattern(N, pattern):
    k = torch.zeros(N, dtype=torch.bool)
    if pattern == "all":
        k[:] = True
    elif pattern == "first":
        k[0] = True
    elif pattern == "last":
        k[-1] = True
    elif pattern == "255_256":
        k[255:257] = True
    elif pattern == "alternating":
        k[::2] = True
    elif pattern == "gap":  # one whole workgroup (rows 256..511) empty between full ones
        k[:] = True
        k[256:512] = False
    else:
        assert pattern == "none"
    return k


@pytest.mark.parametrize("pattern", ["all", "none", "first", "last", "255_256", "alternating", "gap"])
@pytest.mark.parametrize("N", [65_535, 65_536, 65_537, 2_097_153])
def test_compact_rows_scan_rounds_and_patterns(dev, N, pattern):
    """255, 256, 257 and 8193 workgroups: the single-workgroup scan's 256-entry rounds and its carry."""
    from eogs2_amd.optim import compact_rows

    mask = _keep_pattern(N, pattern).to(dev)
    tensors = [torch.arange(N, dtype=torch.int32, device=dev), torch.arange(3 * N, dtype=torch.float32, device=dev).reshape(N, 3),
               torch.arange(N, dtype=torch.float32, device=dev).reshape(N, 1, 1) * 0.5]
    for o, t in zip(compact_rows(mask, tensors), tensors):
        assert o.shape == t[mask].shape and torch.equal(o, t[mask])


def test_compact_rows_uint8_mask_wide_rows_and_many_tensors(dev):
    from eogs2_amd.optim import compact_rows

    N = 70_001
    g = torch.Generator().manual_seed(21)
    m8 = torch.randint(0, 256, (N,), generator=g, dtype=torch.uint8)
    m8[torch.rand(N, generator=g) < 0.5] = 0
    assert int((m8 > 1).sum()) > 1000
    m8, keep = m8.to(dev), (m8 != 0).to(dev)
    wide = torch.randn(N, 64, generator=g).to(dev)  # the widest legal row
    (o,) = compact_rows(m8, [wide])
    assert torch.equal(o, wide[keep])
    with pytest.raises(RuntimeError):
        compact_rows(m8, [torch.zeros(N, 65, device=dev)])
    for count in (24, 25, 49):  # EOGS_COMPACT_MAX_TENSORS = 24 per launch; empty rows inside the first batch
        tensors = []
        for i in range(count):
            if i in (3, 11, 23):
                tensors.append(torch.zeros(N, 0, 3, device=dev))
            else:
                tensors.append((torch.randn(N, 1 + i % 5, generator=g) + i).to(dev))
        outs = compact_rows(m8, tensors)
        assert len(outs) == count
        for i, (o, t) in enumerate(zip(outs, tensors)):
            assert o.shape == t[keep].shape and torch.equal(o, t[keep]), (count, i)


def test_compact_c_abi_writes_only_the_kept_rows(dev):
    """eogs_compact_plan / eogs_compact_apply straight through the C-ABI with outputs inside larger buffers: a sentinel row
    before and after each output stays untouched."""
    import ctypes

    from eogs2_amd import _lib

    abi = _lib.get()
    N, guard = 66_000, -777.0
    g = torch.Generator().manual_seed(31)
    keep = (torch.rand(N, generator=g) < 0.37).to(dev).to(torch.uint8)
    srcs = [torch.randn(N, w, generator=g).to(dev) for w in (3, 1, 9, 64)]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nbytes = ctypes.c_size_t()
    abi.check(abi.compact_bytes(N, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    n_keep = ctypes.c_int64()
    abi.check(abi.compact_plan(N, ctypes.c_void_p(keep.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.byref(n_keep), stream))
    K = n_keep.value
    assert K == int(keep.sum())
    bufs = [torch.full((K + 2, s.shape[1]), guard, device=dev) for s in srcs]
    S = (ctypes.c_void_p * 4)(*[s.data_ptr() for s in srcs])
    D = (ctypes.c_void_p * 4)(*[b[1:].data_ptr() for b in bufs])
    RB = (ctypes.c_int * 4)(*[s.shape[1] * 4 for s in srcs])
    abi.check(abi.compact_apply(N, ctypes.c_void_p(keep.data_ptr()), 4, ctypes.cast(S, ctypes.c_void_p), ctypes.cast(D, ctypes.c_void_p),
                                ctypes.cast(RB, ctypes.c_void_p), ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream))
    torch.cuda.synchronize(dev)
    for b, s in zip(bufs, srcs):
        assert torch.equal(b[1:K + 1], s[keep.bool()])
        assert bool((b[0] == guard).all()) and bool((b[K + 1] == guard).all())


def test_sum_into_more_tensors_and_sources_than_one_launch(dev):
    """11 destinations (EOGS_SUM_MAX_TENSORS = 8) and 6 sources (EOGS_SUM_MAX_SOURCES = 4) in one call: the sequence of adds."""
    from eogs2_amd.optim import sum_into_

    g = torch.Generator().manual_seed(41)
    shapes = [(1000, 3), (5,), (0, 3), (777, 4), (1025,), (1,), (300, 1, 3), (4097,), (64,), (2, 2), (1023,)]
    base = [torch.randn(s, generator=g).to(dev) for s in shapes]
    srcs = [[(torch.randn(s, generator=g) * 10.0 ** (j - 2)).to(dev) for s in shapes] for j in range(6)]
    want = [b.clone() for b in base]
    for s in srcs:
        for w, x in zip(want, s):
            w.add_(x)
    got = [b.clone() for b in base]
    sum_into_(got, srcs)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
