"""GPU (MI355X): the optimizer step inside a recorded graph (include/eogs_step.h, eogs2_amd.optim.FusedAdam(capturable=True),
eogs2_amd.rasterizer.captured_gate).

What is tested: the device-side bias corrections against float64 on the grid of optim_cases (same bound as the host path,
FACTOR_KERNEL = 2: the four constants are rounded to fp32 from the same double expressions); the prologue's scalars within one
fp32 ulp of the host's and, where equal, the whole step bit for bit against the host-stepped FusedAdam; the element kernel's
edges through the capturable path; a closed gate changes nothing at all; the in-launch retire equals retire_rows after the step;
a captured step replays like the eager one, counters included; the gate's rule equals eogs_rast_capacity_token's; a whole
training step (render, L1 loss, backward, gate, Adam) as a GraphedStep equals the eager loop bit for bit, an outgrown replay
updates nothing and is recorded again, a forward's error leaves every bit in place; the reference's lifecycle fixtures keep
working with a device step tensor."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def _capturable():
    from eogs2_amd.optim import FusedAdam

    return functools.partial(FusedAdam, capturable=True)


def _gate(dev, a, b):
    return torch.tensor([a, b], dtype=torch.int32, device=dev).view(torch.uint32)


# ---- 1. arithmetic against float64 ----
@pytest.mark.parametrize("eps", oc.ADAM_GRID_EPS)
@pytest.mark.parametrize("step", oc.ADAM_GRID_STEPS)
def test_capturable_one_step_elementwise(dev, step, eps):
    """The grid of tests/test_gpu_optim.py::test_fused_adam_one_step_elementwise through the device-side prologue: same bound,
    same factor (the prologue rounds lr, 1 / bc1, sqrt(bc2) and eps to fp32 from the double expressions of the host path)."""
    worst = [0.0, 0.0, 0.0]
    for gscale in oc.ADAM_GRID_GSCALE:
        r = oc.adam_check_one_step(_capturable(), dev, step, gscale, eps, oc.FACTOR_KERNEL)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"step {step} eps {eps:g}: worst error / bound m {worst[0]:.3f} v {worst[1]:.3f} p {worst[2]:.3f}")


# ---- 2. the prologue's scalars, and bits against the host path ----
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 30000])
def test_prologue_scalars_and_bits_against_the_host_path(dev, t):
    from eogs2_amd.optim import FusedAdam

    b1, b2 = oc.BETAS
    lr = 1e-2
    want1, want2 = np.float32(1.0 / (1.0 - b1 ** t)), np.float32(math.sqrt(1.0 - b2 ** t))
    equal = 0
    for eps in oc.ADAM_GRID_EPS:
        p, g, m, v = oc.adam_grid_state(1e-2, n=3077, seed=t)
        out = []
        for cls in (FusedAdam, _capturable()):
            par = torch.nn.Parameter(p.clone().to(dev))
            opt = cls([{"params": [par], "lr": lr, "name": "x"}], lr=0.0, betas=oc.BETAS, eps=eps)
            opt.state[par] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.clone().to(dev), "exp_avg_sq": v.clone().to(dev)}
            par.grad = g.clone().to(dev)
            opt.step()
            st = opt.state[par]
            assert int(st["step"]) == t
            out.append((opt, par, [par.detach().cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()]))
        (_, _, host), (opt, par, got) = out
        assert opt.state[par]["step"].device.type == "cuda" and opt.state[par]["step"].dtype == torch.float32
        row = opt.step_scalars(par).cpu().numpy()
        print(f"t {t} eps {eps:g}: prologue {row.tolist()} host ({float(want1)!r}, {float(want2)!r})")
        assert row.dtype == np.float32 and row[0] == np.float32(lr) and row[3] == 0.0
        assert abs(float(row[1]) - float(want1)) <= float(np.spacing(want1))
        assert abs(float(row[2]) - float(want2)) <= float(np.spacing(want2))
        if row[1] == want1 and row[2] == want2:
            equal += 1
            for what, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, host):
                assert a.numpy().tobytes() == b.numpy().tobytes(), (what, t, eps)
    assert equal >= 1, t


# ---- 3. edges of the element kernel ----
def _checked_step(opt, factor=oc.FACTOR_KERNEL, **kw):
    """One `opt.step()`; every element of every parameter and moment against torch's formula in float64 from the state the
    device held before the step, within `factor` x optim_cases.adam_step_bound (tests/test_gpu_optim.py holds the host path to
    the same). A parameter without a gradient keeps its bits and its step."""
    pre = []
    for g in opt.param_groups:
        for p in g["params"]:
            st = opt.state.get(p) or {}
            z = torch.zeros(p.shape)
            pre.append((g, p, p.detach().cpu().clone(), None if p.grad is None else p.grad.detach().cpu().clone(),
                        st["exp_avg"].cpu().clone() if st else z, st["exp_avg_sq"].cpu().clone() if st else z.clone(),
                        int(st["step"]) if st else 0))
    opt.step(**kw)
    worst = 0.0
    for g, p, p0, g0, m0, v0, t0 in pre:
        st = opt.state.get(p) or {}
        if g0 is None:
            assert torch.equal(p.detach().cpu(), p0) and (int(st["step"]) if st else 0) == t0
            if st:
                assert torch.equal(st["exp_avg"].cpu(), m0) and torch.equal(st["exp_avg_sq"].cpu(), v0)
            continue
        assert int(st["step"]) == t0 + 1 and st["step"].device == p.device and st["step"].dtype == torch.float32
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


def _plain(sizes, d, seed=0, **group_kw):
    g = torch.Generator().manual_seed(seed)
    return [dict({"params": [torch.nn.Parameter(torch.randn(n, generator=g).to(d))], "lr": 1e-2 * (1 + i % 3), "name": f"t{i}"},
                 **{k: v[i % len(v)] for k, v in group_kw.items()}) for i, n in enumerate(sizes)]


def _rand_grads(opt, gen, scale=1.0, skip=()):
    for i, gr in enumerate(opt.param_groups):
        p = gr["params"][0]
        p.grad = None if i in skip else (torch.randn(p.shape, generator=gen) * scale + 0.01).to(p.device)


@pytest.mark.parametrize("numel", [1, 3, 4, 5, 1023, 1024, 1025, 4097])
def test_capturable_vector_path_tail_and_workgroup_edge(dev, numel):
    opt = _capturable()(_plain([numel], dev, seed=numel), lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(numel + 1)
    for it in range(4):
        _rand_grads(opt, gen, 10.0 ** (it - 2))
        _checked_step(opt)


@pytest.mark.parametrize("off_p,off_g,off_m,off_v", [(1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (1, 2, 3, 1), (3, 3, 3, 3)])
def test_capturable_unaligned_views_touch_nothing_else(dev, off_p, off_g, off_m, off_v):
    n, pad, guard = 1030, 8, 12345.0
    gen = torch.Generator().manual_seed(off_p * 64 + off_g * 16 + off_m * 4 + off_v)
    bufs = {}
    for k, off in (("p", off_p), ("g", off_g), ("m", off_m), ("v", off_v)):
        b = torch.full((n + 2 * pad,), guard)
        x = torch.randn(n, generator=gen)
        b[pad + off:pad + off + n] = x.abs() if k == "v" else x
        bufs[k] = (b.to(dev), off)
    view = lambda k: bufs[k][0][pad + bufs[k][1]:pad + bufs[k][1] + n]  # noqa: E731
    par = torch.nn.Parameter(view("p"))
    assert par.data_ptr() == view("p").data_ptr()
    opt = _capturable()([{"params": [par], "lr": 1e-2, "name": "x"}], lr=0.0, eps=1e-15)
    opt.state[par] = {"step": torch.tensor(3.0), "exp_avg": view("m"), "exp_avg_sq": view("v")}
    for _ in range(2):
        view("g").copy_(torch.randn(n, generator=gen).to(dev) + 0.01)
        par.grad = view("g")
        _checked_step(opt)
    for k, (b, off) in bufs.items():
        outside = torch.cat((b[:pad + off], b[pad + off + n:]))
        assert bool((outside == guard).all()), k
    assert opt.state[par]["exp_avg"].data_ptr() == view("m").data_ptr()


@pytest.mark.parametrize("n_groups", [16, 17, 40])
def test_capturable_one_and_several_launches(dev, n_groups):
    """16 tensors: one prologue + one element launch; 17 and 40: several, each with its own table; mixed sizes, empty ones."""
    sizes = [(5, 0, 1024, 3, 4097, 0, 1, 70_001, 256, 1025, 2)[i % 11] for i in range(n_groups)]
    opt = _capturable()(_plain(sizes, dev, seed=n_groups), lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        _rand_grads(opt, gen)
        _checked_step(opt)
    assert all(int(opt.state[g["params"][0]]["step"]) == 3 for g in opt.param_groups)
    tables = {opt._ws_row[g["params"][0]][0].data_ptr() for g in opt.param_groups}
    assert len(tables) == (n_groups + 15) // 16
    for i, g in enumerate(opt.param_groups):  # every tensor's row holds ITS learning rate and t = 3
        row = opt.step_scalars(g["params"][0]).cpu().numpy()
        assert row[0] == np.float32(g["lr"]) and row[3] == 0.0
        assert abs(float(row[1]) - 1.0 / (1.0 - 0.9 ** 3)) <= 1e-6 * float(row[1])


def test_capturable_groups_with_their_own_betas_eps_and_steps(dev):
    """Two betas and two eps in one optimizer; a parameter without a gradient keeps its bits and its device step, so groups
    sit at different steps; a learning rate changed between steps; a non-contiguous gradient; lr_tensor written to zero:
    parameter bits unchanged, moments advance."""
    groups = _plain([1000, 1000, 777, 777, 4099, 64], dev, seed=8, betas=[(0.9, 0.999), (0.8, 0.99)], eps=[1e-15, 1e-15, 1e-8])
    opt = _capturable()(groups, lr=0.0)
    gen = torch.Generator().manual_seed(9)
    p5 = opt.param_groups[5]["params"][0]
    for it in range(5):
        _rand_grads(opt, gen, skip=(2,) if it in (1, 2) else (4,) if it == 3 else ())
        wide = torch.randn(1000, 2, generator=gen).to(dev)
        opt.param_groups[1]["params"][0].grad = wide[:, 0]
        assert not wide[:, 0].is_contiguous()
        if it == 2:
            opt.param_groups[0]["lr"] = 3e-5
        if it < 4:
            _checked_step(opt)
            if it == 2:
                assert float(opt.param_groups[0]["lr_tensor"]) == float(np.float32(3e-5))
        else:  # the supported way to change a rate between replays: write the device scalar (group["lr"] is not read again)
            opt.param_groups[5]["lr_tensor"].zero_()
            before = (p5.detach().clone(), opt.state[p5]["exp_avg"].clone(), opt.state[p5]["exp_avg_sq"].clone())
            opt.step()
            assert torch.equal(p5.detach(), before[0])
            assert not torch.equal(opt.state[p5]["exp_avg"], before[1]) and not torch.equal(opt.state[p5]["exp_avg_sq"], before[2])
            assert float(opt.step_scalars(p5)[0]) == 0.0
    steps = [opt.state[g["params"][0]]["step"] for g in opt.param_groups]
    assert all(s.device.type == "cuda" for s in steps) and [int(s) for s in steps] == [5, 5, 3, 5, 4, 5]


def test_capturable_empty_group_and_refusals(dev):
    """The reference's six groups with f_rest [P, 0, 3]: the empty tensor takes part (its step advances, as torch's does) and
    nothing else; what FusedAdam does not implement is refused in the capturable mode too."""
    shapes = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (0, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
    g = torch.Generator().manual_seed(0)
    groups = [{"params": [torch.nn.Parameter(torch.randn((1023,) + s, generator=g).to(dev))], "lr": 1e-3, "name": n} for n, s in shapes.items()]
    opt = _capturable()(groups, lr=0.0, eps=1e-15)
    for _ in range(2):
        for gr in opt.param_groups:
            gr["params"][0].grad = torch.randn(gr["params"][0].shape, generator=g).to(dev)
        _checked_step(opt)
    assert all(int(opt.state[gr["params"][0]]["step"]) == 2 for gr in opt.param_groups)
    for kw in ({"amsgrad": True}, {"weight_decay": 0.1}, {"maximize": True}):
        par = torch.nn.Parameter(torch.zeros(8, device=dev))
        bad = _capturable()([par], lr=1e-2)
        bad.param_groups[0].update(kw)
        par.grad = torch.ones(8, device=dev)
        with pytest.raises(NotImplementedError):
            bad.step()
    par = torch.nn.Parameter(torch.zeros(8, device=dev, dtype=torch.float64))
    par.grad = torch.ones(8, device=dev, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="fp32"):
        _capturable()([par], lr=1e-2).step()
    opt.retire_below = {"no_such_group": 0.0}
    with pytest.raises(ValueError, match="no_such_group"):
        opt.step()


# ---- 4. gate ----
class _Guarded:
    """An optimizer over views into sentinel-padded buffers: parameter, gradient and both moments of every tensor."""

    PAD, GUARD = 8, 12345.0

    def __init__(self, sizes, dev, seed, names=None, **kw):
        gen = torch.Generator().manual_seed(seed)
        self.bufs, groups = [], []
        for i, n in enumerate(sizes):
            b = {}
            for k in "pgmv":
                full = torch.full((n + 2 * self.PAD,), self.GUARD)
                x = torch.randn(n, generator=gen)
                full[self.PAD:self.PAD + n] = x.abs() if k == "v" else x
                b[k] = full.to(dev)
            self.bufs.append(b)
            groups.append({"params": [torch.nn.Parameter(self.view(i, "p", n))], "lr": 1e-2 * (1 + i), "name": (names or {}).get(i, f"t{i}")})
        self.sizes = sizes
        self.opt = _capturable()(groups, lr=0.0, eps=1e-15, **kw)
        for i, (gr, n) in enumerate(zip(self.opt.param_groups, sizes)):
            p = gr["params"][0]
            self.opt.state[p] = {"step": torch.tensor(float(3 + i), device=dev), "exp_avg": self.view(i, "m", n), "exp_avg_sq": self.view(i, "v", n)}
            p.grad = self.view(i, "g", n)

    def view(self, i, k, n):
        return self.bufs[i][k][self.PAD:self.PAD + n]

    def snapshot(self):
        out = [b[k].cpu().clone() for b in self.bufs for k in "pgmv"]
        return out + [self.opt.state[gr["params"][0]]["step"].cpu().clone() for gr in self.opt.param_groups]

    def steps(self):
        return [int(self.opt.state[gr["params"][0]]["step"]) for gr in self.opt.param_groups]


def _equal_snapshots(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.numpy().tobytes() == y.numpy().tobytes(), i


def test_closed_gate_changes_nothing_open_gate_equals_no_gate(dev):
    sizes = [5, 50_001, 1000]
    closed = _Guarded(sizes, dev, seed=11)
    closed.opt.step()  # (uploads the rates, moves nothing of interest: the comparison starts after it)
    pre = closed.snapshot()
    for x in (0, 5):
        closed.opt.step(gate=_gate(dev, 0, x))
        _equal_snapshots(closed.snapshot(), pre)
        assert all(float(closed.opt.step_scalars(gr["params"][0])[3]) == 1.0 for gr in closed.opt.param_groups)
    assert closed.steps() == [4, 5, 6]
    opened, plain = _Guarded(sizes, dev, seed=12), _Guarded(sizes, dev, seed=12)
    opened.opt.step(gate=_gate(dev, 1, 0))
    plain.opt.step()
    _equal_snapshots(opened.snapshot(), plain.snapshot())
    assert opened.steps() == [4, 5, 6]
    for b, n in zip(opened.bufs, sizes):  # the step did move the tensors, and only them
        for k in "pmv":
            assert bool((b[k][:_Guarded.PAD] == _Guarded.GUARD).all()) and bool((b[k][_Guarded.PAD + n:] == _Guarded.GUARD).all())
    fresh = _Guarded(sizes, dev, seed=12)
    assert not torch.equal(fresh.bufs[1]["p"], opened.bufs[1]["p"])
    with pytest.raises(RuntimeError, match="uint32"):
        plain.opt.step(gate=torch.zeros(2, device=dev))


# ---- 5. retire ----
def test_retire_in_the_launch_equals_retire_rows_after_the_step(dev):
    from eogs2_amd.optim import RETIRED_LOGIT, retire_rows

    P = 5003
    gen = torch.Generator().manual_seed(21)
    opacity = torch.rand(P, 1, generator=gen) * 11.0 - 9.0  # logits over -9 .. 2: both sides of the threshold
    opacity[::7] = RETIRED_LOGIT  # retired earlier
    opacity[3] = -6.0             # exactly on the threshold after a zero update: kept (>=)
    xyz = torch.randn(P, 3, generator=gen)
    grad_o = torch.randn(P, 1, generator=gen) * 5.0
    grad_o[::7] = 0.0  # a retired Gaussian is listed nowhere: zero gradient
    grad_o[3] = 0.0
    grad_x = torch.randn(P, 3, generator=gen)

    def make():
        po, px = torch.nn.Parameter(opacity.clone().to(dev)), torch.nn.Parameter(xyz.clone().to(dev))
        opt = _capturable()([{"params": [px], "lr": 1e-3, "name": "xyz"}, {"params": [po], "lr": 5e-2, "name": "opacity"}], lr=0.0, eps=1e-15)
        return opt, po, px

    a, ao, ax = make()
    b, bo, bx = make()
    a.retire_below = {"opacity": -6.0}
    for it in range(3):
        for po, px in ((ao, ax), (bo, bx)):
            po.grad, px.grad = (grad_o * (it + 1)).to(dev), grad_x.to(dev)
            po.grad[(po.detach() < -1e29)] = 0.0
        a.step()
        b.step()
        retire_rows(b, bo.detach().view(-1) >= -6.0)
        for x, y in ((ao, bo), (ax, bx)):
            assert x.detach().cpu().numpy().tobytes() == y.detach().cpu().numpy().tobytes(), it
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(a.state[x][k], b.state[y][k])
    retired = ao.detach().view(-1) == RETIRED_LOGIT
    assert bool(retired[::7].all()) and int(retired.sum()) > P // 7 + 1 and not bool(retired[3])
    assert float(ax.detach().min()) > -1e29  # only the named group retires


# ---- 6. capture ----
def test_captured_step_replays_like_the_eager_one(dev):
    sizes = [1, 7, 1024, 4097, 20_000]

    def make():
        g = torch.Generator().manual_seed(31)
        groups = [{"params": [torch.nn.Parameter(torch.randn(n, generator=g).to(dev))], "lr": 1e-2 * (1 + i), "name": f"t{i}"} for i, n in enumerate(sizes)]
        opt = _capturable()(groups, lr=0.0, eps=1e-15)
        bufs = [torch.zeros(n, device=dev) for n in sizes]
        for gr, b in zip(opt.param_groups, bufs):
            gr["params"][0].grad = b  # a fixed buffer, rewritten between replays
        start = [gr["params"][0].detach().clone() for gr in opt.param_groups]
        for b in bufs:
            b.fill_(0.5)
        opt.step()  # creates the state, uploads the rates; then back to the start, in place
        for gr, s in zip(opt.param_groups, start):
            p = gr["params"][0]
            with torch.no_grad():
                p.copy_(s)
            st = opt.state[p]
            st["step"].zero_(), st["exp_avg"].zero_(), st["exp_avg_sq"].zero_()
        return opt, bufs

    def grads(r):
        g = torch.Generator().manual_seed(100 + r)
        return [torch.randn(n, generator=g) * 10.0 ** (r - 3) for n in sizes]

    cap, cap_bufs = make()
    ref, ref_bufs = make()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.step()
    torch.cuda.synchronize()
    assert all(int(cap.state[gr["params"][0]]["step"]) == 0 for gr in cap.param_groups)  # a capture runs nothing
    for r in range(6):
        for cb, rb, x in zip(cap_bufs, ref_bufs, grads(r)):
            cb.copy_(x)
            rb.copy_(x)
        if r == 3:
            cap.param_groups[2]["lr_tensor"].fill_(3e-4)
            ref.param_groups[2]["lr"] = 3e-4
        graph.replay()
        ref.step()
    torch.cuda.synchronize()
    for gc, gr in zip(cap.param_groups, ref.param_groups):
        pc, pr = gc["params"][0], gr["params"][0]
        assert pc.detach().cpu().numpy().tobytes() == pr.detach().cpu().numpy().tobytes(), gc["name"]
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(cap.state[pc][k], ref.state[pr][k]), (gc["name"], k)
        assert int(cap.state[pc]["step"]) == 6
    assert float(cap.step_scalars(cap.param_groups[2]["params"][0])[0]) == float(np.float32(3e-4))
    # a changed group["lr"] cannot reach a recording
    cap.param_groups[0]["lr"] = 0.5
    other = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="lr"):
        with torch.cuda.graph(other):
            cap.step()
    torch.cuda.synchronize()
    assert int(cap.state[cap.param_groups[0]["params"][0]]["step"]) == 6


# ---- 7. the gate's rule ----
_SLOTS, _ENTRIES_SHIFT, _ENTRIES = 0x7FFFFFFF, 32, 0x07FFFFFF


def _pack(slots, entries):
    return (entries << _ENTRIES_SHIFT) | slots  # csrc/common.h nr_pack, every flag clear


def test_gate_rule_equals_capacity_token(dev):
    from eogs2_amd import _lib
    from eogs2_amd._abi import FLAG_DEFER_COUNTS, FLAG_NO_READBACK, StepForward
    from eogs2_amd.synthetic import make_scene, settings_for

    abi = _lib.get()
    P, H, W = 2000, 64, 64
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def forward(sc, opacities):
        """eogs_rast_forward_prepare with deferred counts, nothing read back; then its exact token"""
        rs = settings_for(sc, H, W)
        n = ctypes.c_size_t()
        abi.check(abi.geom_bytes(P, ctypes.byref(n)))
        geom = torch.empty((n.value,), dtype=torch.uint8, device=dev)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        R = ctypes.c_int64()
        ins = [sc[k].contiguous() for k in ("means3D", "scales", "rotations")] + [opacities.contiguous(), sc["colors"].contiguous()]
        vm, pm = rs.viewmatrix.contiguous(), rs.projmatrix.contiguous()
        abi.check(abi.forward_prepare(P, H, W, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), None, ptr(ins[3]), ptr(ins[4]), 1.0, ptr(vm), ptr(pm),
                                      None, FLAG_DEFER_COUNTS | FLAG_NO_READBACK, ptr(radii), ptr(geom), geom.numel(), None, 0,
                                      ctypes.byref(R), stream))
        abi.check(abi.read_counts(P, H, W, ptr(geom), geom.numel(), 0, stream, ctypes.byref(R)))
        return geom, R.value, ins

    for mult in (1.0, 3.0, 8.0):  # (the hand-made capacities below need more than eogs_rast_capacity_token's floor of 4096 / 1024)
        sc = make_scene(P, H, W, seed=31, opacity="trained", device=dev, scale_mult=mult)
        geom, exact, keep = forward(sc, sc["opacities"])
        slots, entries = exact & _SLOTS, (exact >> _ENTRIES_SHIFT) & _ENTRIES
        if slots > 4097 and entries > 1025:
            break
    print(f"exact counts: {slots} record slots, {entries} list entries (scale_mult {mult})")
    assert slots > 4097 and entries > 1025
    gate = _gate(dev, 7, 7)

    def run(forwards, accumulate=0):
        arr = (StepForward * len(forwards))()
        for a, (g, cap) in zip(arr, forwards):
            a.geom, a.geom_bytes, a.P, a.capacity = g.data_ptr(), g.numel(), P, cap
        abi.check(abi.step_gate(len(forwards), ctypes.cast(arr, ctypes.c_void_p), accumulate, ptr(gate), stream))
        return gate.view(torch.int32).cpu().tolist()

    def capacity(cap_slots, cap_entries, of=None):
        """a capacity token of exactly these counts from eogs_rast_capacity_token, and its verdict on `of`"""
        cap, fits = ctypes.c_int64(), ctypes.c_int()
        abi.check(abi.capacity_token(P, _pack(cap_slots - 4096, cap_entries - 1024), 0.0, 0, exact if of is None else of,
                                     ctypes.byref(cap), ctypes.byref(fits)))
        assert (cap.value & _SLOTS, (cap.value >> _ENTRIES_SHIFT) & _ENTRIES) == (cap_slots, cap_entries)
        return cap.value, fits.value

    for cap_slots, cap_entries, want in ((slots, entries, 1), (slots - 1, entries, 0), (slots, entries - 1, 0), (slots + 1, entries + 1, 1)):
        cap, fits = capacity(cap_slots, cap_entries)
        got = run([(geom, cap)])
        assert fits == want and got == [want, 0 if want else 1], (cap_slots, cap_entries, got, fits)
    # nothing listed: fits whatever the capacity
    geom0, exact0, keep0 = forward(sc, torch.zeros_like(sc["opacities"]))
    assert exact0 == 0
    assert run([(geom0, 0)]) == [1, 0] and capacity(4096, 1024, of=0)[1] == 1
    # two forwards, the second too small
    ok, _ = capacity(slots, entries)
    small, _ = capacity(slots - 1, entries)
    assert run([(geom, ok), (geom, small)]) == [0, 0b10]
    assert run([(geom, ok), (geom0, 0)]) == [1, 0]
    # accumulate: a closed gate stays closed, the masks are ORed; an open one stays open
    assert run([(geom, small)]) == [0, 1]
    assert run([(geom, ok), (geom, ok)], accumulate=1) == [0, 1]
    assert run([(geom, ok), (geom, small)], accumulate=1) == [0, 0b11]
    assert run([(geom, ok)]) == [1, 0]
    assert run([(geom0, 0)], accumulate=1) == [1, 0]
    assert run([], accumulate=0) == [1, 0]


# ---- 8. / 9. the whole step ----
NAMES = ("means3D", "colors", "opacities", "scales", "rotations")
LRS = {"means3D": 1e-5, "colors": 1e-3, "opacities": 1e-3, "scales": 1e-6, "rotations": 1e-4}


class _Train:
    """render -> L1 loss -> backward -> captured_gate -> FusedAdam(capturable=True), over tensors that stay where they are"""

    def __init__(self, P, H, W, dev, seed, **kw):
        from eogs2_amd import GaussianRasterizer
        from eogs2_amd.synthetic import make_scene, settings_for

        self.args = (P, H, W, dev, seed, kw)
        sc = make_scene(P, H, W, seed=seed, opacity="trained", device=dev, **kw)
        self.rast = GaussianRasterizer(settings_for(sc, H, W))
        self.params = {k: torch.nn.Parameter(sc[k].clone()) for k in NAMES}
        self.m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        self.target = torch.rand(5, H, W, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
        self.opt = _capturable()([{"params": [self.params[k]], "lr": LRS[k], "name": k} for k in NAMES], lr=0.0, eps=1e-15)

    def twin(self):
        """Another instance holding copies of every bit this one holds now."""
        P, H, W, dev, seed, kw = self.args
        t = _Train(P, H, W, dev, seed, **kw)
        with torch.no_grad():
            for k in NAMES:
                t.params[k].copy_(self.params[k])
        for k in NAMES:
            st = self.opt.state.get(self.params[k])
            if st:
                t.opt.state[t.params[k]] = {n: v.clone() for n, v in st.items()}
        return t

    def __call__(self):
        from eogs2_amd import rasterizer

        p = self.params
        for t in p.values():
            t.grad = None
        self.m2.grad = None
        color, radii, invd = self.rast(p["means3D"], self.m2, p["opacities"], colors_precomp=p["colors"], scales=p["scales"],
                                       rotations=p["rotations"])
        loss = (color - self.target).abs().mean()
        loss.backward()
        self.opt.step(gate=rasterizer.captured_gate())  # (None in an eager run)
        return loss.detach()

    def state(self):
        out = []
        for k in NAMES:
            st = self.opt.state[self.params[k]]
            out += [self.params[k].detach().cpu().clone(), st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone(), st["step"].cpu().clone()]
        return out

    def steps(self):
        return [int(self.opt.state[self.params[k]]["step"]) for k in NAMES]


def test_whole_step_as_a_graph_equals_the_eager_loop(dev):
    from eogs2_amd.graph import GraphedStep

    a = _Train(2000, 64, 64, dev, seed=41)
    b = a.twin()
    g = GraphedStep(a, warmup=1, idempotent=True)  # (the warm-up run is a real step: the eager loop takes it too)
    want = [b().clone()]
    assert len(g.forwards) == 1 and a.steps() == [1] * 5
    _equal_snapshots(a.state(), b.state())
    got = []
    for _ in range(8):
        got.append(g().clone())
        want.append(b().clone())
    torch.cuda.synchronize()
    assert g.replays == 8 and g.recaptures == 0
    assert all(torch.equal(x, y) for x, y in zip(got, want[1:]))
    _equal_snapshots(a.state(), b.state())
    assert a.steps() == [9] * 5


def test_outgrown_replay_updates_nothing_and_is_recorded_again(dev):
    from eogs2_amd import RastError
    from eogs2_amd.graph import GraphedStep

    a = _Train(20011, 200, 168, dev, seed=6, scale_mult=0.4)  # (a shape whose counts no other test has raised)
    g = GraphedStep(a, warmup=1, idempotent=True)
    assert a.steps() == [1] * 5
    with torch.no_grad():
        a.params["scales"].mul_(7.5)  # several times the listed tiles: beyond 1.25 x the recorded counts
    b = a.twin()
    loss = g().clone()  # replay: gate closed, nothing updated -> recorded again with room -> replay: one update
    assert g.recaptures == 1 and g.replays == 2
    want = b()  # ONE eager update from the enlarged state
    torch.cuda.synchronize()
    assert torch.equal(loss, want), (float(loss), float(want))
    _equal_snapshots(a.state(), b.state())
    assert a.steps() == [2] * 5
    # a forward's own error: raised as before, and every bit stays
    with torch.no_grad():
        z = a.params["means3D"][17, 2].clone()
        a.params["means3D"][17, 2] = 1.0  # altitude 350 > 200
    pre = a.state()
    with pytest.raises(RastError, match="too high"):
        g()
    torch.cuda.synchronize()
    _equal_snapshots(a.state(), pre)
    with torch.no_grad():
        a.params["means3D"][17, 2] = z
        b.params["means3D"][17, 2] = z
    loss = g().clone()  # the step goes on from where it was
    assert torch.equal(loss, b()) and a.steps() == [3] * 5 and g.recaptures == 1


# ---- 10. the reference's lifecycle with a device step tensor ----
@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_lifecycle_with_a_device_step(dev, name):
    """tests/test_gpu_optim.py::test_lifecycle_matches_the_reference_fixture with FusedAdam(capturable=True): prune, clone,
    split, opacity reset and the Adam stretches between them, same comparisons, same bounds."""
    from eogs2_amd import optim

    log = []
    try:
        oc.replay(oc.Fixture(name), dev, _capturable(), optim, exact=False, log=log)
    finally:
        print("\n".join(log))
