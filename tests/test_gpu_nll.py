"""GPU (MI355X): the transient-uncertainty term (eogs2_amd.uncertainty, include/eogs_nll.h) against torch's float64 run of
train_pan.py:434-440 (tests/golden/nll/*.npz) and, where a file would be too large, its numpy float64 restatement, inside the
derived bound of tests/nll_cases.py — every element, nothing left out; bitwise reproducibility; the autograd path; one recorded
graph whose weight is switched between replays; the per-view chain (mask in a ViewBank state slot under a capturable FusedAdam
inside a GraphedStep) against the eager loop bit for bit; and the example.

Largest multiples of E x magnitude reached on an MI355X (the bound is 8, and 4 for the statistics): loss 1.86, g_input 2.59,
g_mask 3.39, g_var 1.02, mean 0.68, std 0.60; torch-float32's own run of the two statements reaches 2.18, 4.49, 5.87, 4.35, 2.5,
0.60. The file takes about 6 s.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import nll_cases as nc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (g_loss, g_total, weight) -> k = g_total * weight + g_loss, every product and sum exact in float32; None = NULL
UPSTREAMS = {"loss": (1.0, None, None), "total": (None, 0.75, 0.5), "both": (-1.25, 0.75, 0.5), "total_unweighted": (None, 2.0, None)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).tolist() if t.numel() < 64 else t.detach().cpu().contiguous().numpy().tobytes()


def _k(up):
    g_loss, g_total, w = up
    return (0.0 if g_total is None else g_total * (1.0 if w is None else w)) + (0.0 if g_loss is None else g_loss)


def run_abi(dev, image, gt, vm, kind, full=False, sum=False, up=UPSTREAMS["loss"], floor=nc.FLOOR, eps=nc.EPS, outputs=(True, True)):  # noqa: A002
    """One forward and one backward straight through the C-ABI: (out f32[6], g_input, g_vm) as numpy."""
    from eogs2_amd import _lib
    from eogs2_amd._abi import NLL_FULL, NLL_MASK, NLL_SUM

    lib = _lib.get()
    x, t, m = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (image, gt, vm))
    planes, (H, W) = (x.shape[0] if x.ndim == 3 else 1), x.shape[-2:]
    var_planes = planes if (m.ndim == 3 and m.shape[0] == planes) else 1
    mode = (NLL_MASK if kind == "mask" else 0) | (NLL_FULL if full else 0) | (NLL_SUM if sum else 0)
    n = ctypes.c_size_t()
    lib.check(lib.nll_bytes(planes, H, W, ctypes.byref(n)))
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
    out = torch.full((6,), float("nan"), device=dev)
    scalars = [None if v is None else torch.tensor([v], dtype=torch.float32, device=dev) for v in up]
    g_loss, g_total, w = (None if s is None else ctypes.c_void_p(s.data_ptr()) for s in scalars)
    g_x = torch.full_like(x, float("nan")) if outputs[0] else None
    g_m = torch.full_like(m, float("nan")) if outputs[1] else None
    p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(lib.nll_forward(planes, H, W, mode, p(x), p(t), p(m), var_planes, floor, eps, w, p(out), p(ws), n.value, stream))
    lib.check(lib.nll_backward(planes, H, W, mode, p(x), p(t), p(m), var_planes, floor, eps, w, g_loss, g_total, p(g_x), p(g_m), stream))
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if g_x is None else g_x.cpu().numpy(), None if g_m is None else g_m.cpu().numpy()


def run_python(dev, image, gt, vm, kind, full=False, sum=False, up=UPSTREAMS["loss"]):  # noqa: A002
    """The same through eogs2_amd.uncertainty and autograd: g_loss * loss + g_total * total, backward."""
    from eogs2_amd import uncertainty as U

    g_loss, g_total, w = up
    x = torch.from_numpy(image).to(dev).requires_grad_(True)
    m = torch.from_numpy(vm).to(dev).requires_grad_(True)
    t = torch.from_numpy(gt).to(dev)
    if kind == "mask":
        total, loss, stats = U.transient_nll(x, t, m, weight=w)
    else:
        assert g_total is None
        loss, stats = U.gaussian_nll_loss(x, t, m, full=full, reduction="sum" if sum else "mean", return_out=True)
        total = loss
    assert not stats.requires_grad
    obj = (0.0 if g_loss is None else g_loss * loss) + (0.0 if g_total is None else g_total * total)
    obj.backward()
    out = np.concatenate([[float(loss.detach()), float(total.detach())], stats.cpu().numpy()])
    return out.astype(np.float32), x.grad.cpu().numpy(), m.grad.cpu().numpy()


def scaled(ref, k):
    """`restate`'s (or a fixture's) reference for the upstream factor k instead of 1: the gradients are linear in it."""
    out = dict(ref)
    for key in ("g_input", "g_vm"):
        if key in ref:
            out[key] = ref[key] * k
    out["g_mag"] = ref["g_mag"] * abs(k)
    return out


def check_run(got, ref, vm, kind, tag, k=1.0, scalars_only=False, w=None):
    out, g_x, g_m = got
    ref = scaled(ref, k)
    quantities = {"loss": out[0], "mean": out[2], "std": out[3]}
    if not scalars_only or "g_input" in ref:
        quantities.update(g_input=g_x, g_vm=g_m)
    mult = nc.check(quantities, ref, tag)
    assert out[1] == np.float32(out[0]) * np.float32(1.0 if w is None else w)  # total = weight * loss, in float32
    assert out[4] == ((vm < 0).sum() if kind == "var" else 0) and out[5] == (((vm < 0) | (vm > 1)).sum() if kind == "mask" else 0)
    if kind == "mask":
        outside = (vm < 0) | (vm > 1)
        assert not g_m[outside].any() and not np.signbit(g_m[outside]).any()  # exactly 0.0 outside [0, 1]
        edge = (vm == 0) | (vm == 1)  # (-0.0 included: it compares equal)
        if edge.any() and k:
            assert (g_m[edge] != 0).all()  # inclusive bounds, as torch's clamp backward
    return mult


# ---- 1. every case, through the C-ABI and through the Python entry points ----
@pytest.mark.parametrize("path", ["abi", "python"])
@pytest.mark.parametrize("name", nc.FIXTURES)
def test_fixture_cases_inside_the_bound(dev, name, path):
    c = nc.case(name)
    (image, gt, vm), ref = nc.fixture_reference(name)
    if c["scalars_only"]:  # the file holds the scalars; the gradients of this size come from the restatement
        full = nc.restate(image, gt, vm, c["kind"], c["full"], c["sum"])
        ref.update(g_input=full["g_input"], g_vm=full["g_vm"])
    ups = UPSTREAMS if c["kind"] == "mask" else {"loss": UPSTREAMS["loss"]}
    for label, up in ups.items():
        run = run_abi if path == "abi" else run_python
        got = run(dev, image, gt, vm, c["kind"], c["full"], c["sum"], up)
        check_run(got, ref, vm, c["kind"], f"{name} {path} {label}", _k(up), w=up[2])
    if c["constant"] is not None:
        assert got[0][3] == 0.0 and got[0][2] == np.float32(c["constant"])  # a constant mask: std exactly 0.0, no NaN


@pytest.mark.parametrize("name", sorted(nc.EXTRA))
def test_extra_cases_inside_the_bound(dev, name):
    image, gt, vm = nc.extra_inputs(name)
    kind = nc.EXTRA[name]["kind"]
    ref = nc.restate(image, gt, vm, kind)
    up = UPSTREAMS["both"] if kind == "mask" else UPSTREAMS["loss"]
    got = run_abi(dev, image, gt, vm, kind, up=up)
    check_run(got, ref, vm, kind, name + " abi", _k(up), w=up[2])
    if name.startswith("var_negative"):
        # the stated deviation: no exception and no wait; the entry is counted, its element is 0.5 (log eps + r^2 / eps),
        # finite, and its gradient is passed on as for any variance below eps
        at = nc.EXTRA[name]["negative_at"]
        assert got[0][4] == 1.0 and np.isfinite(got[0][0]) and np.isfinite(got[2]).all() and got[2].reshape(-1)[at] != 0
        r = float(image.reshape(-1)[at]) - float(gt.reshape(-1)[at])
        with_one = nc.restate(image, gt, np.where(vm < 0, np.float32(1.0), vm), kind)  # var 1 there: its element is 0.5 r^2
        assert abs((ref["loss"] - with_one["loss"]) * image.size - (0.5 * (np.log(nc.EPS) + r * r / nc.EPS) - 0.5 * r * r)) < 1e-6
        py = run_python(dev, image, gt, vm, kind)
        assert _bits(torch.from_numpy(py[0][[0, 2, 3, 4, 5]])) == _bits(torch.from_numpy(got[0][[0, 2, 3, 4, 5]]))


def test_neither_upstream_and_single_outputs(dev):
    """No upstream gradient at all: exact zeros everywhere. And either output alone (the other NULL) gives the bits of both."""
    (image, gt, vm), _ = nc.fixture_reference("mask_3x37x53")
    out, g_x, g_m = run_abi(dev, image, gt, vm, "mask", up=(None, None, 0.5))
    assert np.isfinite(out[0]) and not g_x.any() and not g_m.any()
    both = run_abi(dev, image, gt, vm, "mask", up=UPSTREAMS["both"])
    only_x = run_abi(dev, image, gt, vm, "mask", up=UPSTREAMS["both"], outputs=(True, False))
    only_m = run_abi(dev, image, gt, vm, "mask", up=UPSTREAMS["both"], outputs=(False, True))
    assert only_x[2] is None and only_m[1] is None
    assert only_x[1].tobytes() == both[1].tobytes() and only_m[2].tobytes() == both[2].tobytes()


def test_weight_zero_does_not_pass_a_nan_pixel_on(dev):
    (image, gt, vm), _ = nc.fixture_reference("mask_4x12x20")
    image, vm = image.copy(), vm.copy()
    image[1, 3, 5], vm[3, 5] = np.nan, 0.5  # (a pixel whose mask lies inside [0, 1]: its gradient is not the clamp's 0)
    out, g_x, g_m = run_abi(dev, image, gt, vm, "mask", up=(None, 1.0, 0.0))
    assert np.isnan(out[0]) and out[1] == 0.0 and not np.signbit(out[1])  # the term itself is NaN, its weighted total exactly 0
    assert not g_x.any() and not g_m.any()
    out, g_x, g_m = run_abi(dev, image, gt, vm, "mask", up=(None, 1.0, 0.5))  # switched on: the NaN shows, at its pixel only
    assert np.isnan(out[1]) and np.isnan(g_x[1, 3, 5]) and np.isnan(g_m[3, 5]) and np.isnan(g_x).sum() == 1 and np.isnan(g_m).sum() == 1


# ---- 2. same bits on every run ----
@pytest.mark.parametrize("name", ["mask_2x300x300", "mask_3x37x53", "var_planes_3x37x53_full_sum"])
def test_two_runs_give_the_same_bits(dev, name):
    c = nc.case(name)
    image, gt, vm = nc.inputs(name)
    up = UPSTREAMS["both"] if c["kind"] == "mask" else UPSTREAMS["loss"]
    a = run_abi(dev, image, gt, vm, c["kind"], c["full"], c["sum"], up)
    b = run_abi(dev, image, gt, vm, c["kind"], c["full"], c["sum"], up)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_vector_and_scalar_paths_give_the_same_bits(dev):
    """H W a multiple of four: planes that start 16-byte aligned take the 16-byte loads, the same planes 4 bytes further on the
    scalar ones; the arithmetic is ordered by units of four pixels in both."""
    from eogs2_amd import uncertainty as U

    image, gt, vm = nc.inputs("mask_4x12x20")
    res = []
    for shift in (0, 1):
        def place(a):
            buf = torch.zeros(a.size + 4, device=dev)
            buf[shift:shift + a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
            return buf[shift:shift + a.size].view(a.shape)
        x, t, m = place(image).requires_grad_(True), place(gt), place(vm).requires_grad_(True)
        assert x.data_ptr() % 16 == 4 * shift
        total, loss, stats = U.transient_nll(x, t, m, weight=0.5)
        g = torch.autograd.grad(total, (x, m))
        res.append([_bits(v) for v in (total, loss, stats, *g)])
    assert res[0] == res[1]


# ---- 3. the autograd path ----
def test_image_gradient_adds_onto_a_second_loss(dev):
    from eogs2_amd import uncertainty as U

    (image, gt, vm), ref = nc.fixture_reference("mask_3x37x53")
    x = torch.from_numpy(image).to(dev).requires_grad_(True)
    m = torch.from_numpy(vm).to(dev).requires_grad_(True)
    t = torch.from_numpy(gt).to(dev)
    term = U.TransientNLL(0.1)
    (0.1 * term(x, t, m)).backward()
    alone_x, alone_m = x.grad.clone(), m.grad.clone()
    k = float(np.float32(0.1))
    nc.check({"g_input": alone_x.cpu().numpy(), "g_vm": alone_m.cpu().numpy()}, scaled(ref, k), "TransientNLL x 0.1")
    stats = term.log_stats()
    assert stats["clipped"] == int(((vm < 0) | (vm > 1)).sum()) and abs(stats["mean"] - ref["mean"]) <= 4 * nc.E * abs(ref["mean"])
    assert abs(stats["std"] - ref["std"]) <= 4 * nc.E * ref["std"]
    x.grad = m.grad = None
    second = (x * t).sum()  # (x enters it once: its gradient, t, meets the term's in ONE float32 add, autograd's own)
    (0.1 * term(x, t, m) + second).backward()
    assert _bits(x.grad) == _bits(alone_x + t) and _bits(m.grad) == _bits(alone_m)
    # a term nobody differentiates launches no backward; a mask that needs no gradient gets none
    total, loss, _ = U.transient_nll(x.detach(), t, m.detach())
    assert not total.requires_grad and not loss.requires_grad
    x.grad = None
    U.transient_nll(x, t, m.detach())[1].backward()
    nc.check({"g_input": x.grad.cpu().numpy()}, ref, "image alone")
    p = U.transient_parameters(5, 9, 0.25, dev)
    assert isinstance(p, torch.nn.Parameter) and p.shape == (5, 9) and p.requires_grad and bool((p == 0.25).all())


# ---- 4. one recorded graph ----
def test_forward_and_backward_replay_in_a_graph_across_the_weight_switch(dev):
    from eogs2_amd import uncertainty as U

    image, gt, vm = nc.inputs("mask_3x37x53")
    x = torch.from_numpy(image).to(dev).requires_grad_(True)
    m = torch.from_numpy(vm).to(dev).requires_grad_(True)
    t = torch.from_numpy(gt).to(dev)
    weight = torch.zeros(1, device=dev)

    def fn():
        total, loss, stats = U.transient_nll(x, t, m, weight=weight)
        g_x, g_m = torch.autograd.grad(total, (x, m))
        return total, loss, stats, g_x, g_m

    def eager(w):
        weight.fill_(w)
        return [_bits(v) for v in fn()]

    want = {w: eager(w) for w in (0.0, 0.1, 0.7)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = fn()
    for w in (0.0, 0.1, 0.0, 0.7, 0.1):  # the switch is a write into the weight tensor: no new capture
        weight.fill_(w)
        graph.replay()
        torch.cuda.synchronize()
        assert [_bits(v) for v in outs] == want[w], w
    assert want[0.1] != want[0.7] and not any(np.frombuffer(b, np.float32).any() for b in want[0.0][3:])
    # weight 0 and a NaN pixel: every gradient exactly 0, in the same recording
    with torch.no_grad():
        x[2, 7, 11] = float("nan")
    weight.fill_(0.0)
    graph.replay()
    torch.cuda.synchronize()
    total, loss, _, g_x, g_m = outs
    assert float(total.detach()) == 0.0 and bool(loss.isnan()) and not bool(g_x.any()) and not bool(g_m.any())
    weight.fill_(0.1)
    graph.replay()
    torch.cuda.synchronize()
    assert bool(g_x[2, 7, 11].isnan()) and int(g_x.isnan().sum()) == 1


# ---- 5. the per-view chain ----
ORDER = [0, 1, 1, 0, 1, 0]


def _chain(dev, graphed):
    from eogs2_amd import uncertainty as U
    from eogs2_amd.graph import GraphedStep
    from eogs2_amd.optim import FusedAdam
    from eogs2_amd.rasterizer import captured_gate
    from eogs2_amd.views import ViewBank, ViewSchedule

    V, C, H, W = 2, 3, 24, 40
    rows = [nc.make_inputs("mask", C, H, W, seed=40 + v) for v in range(V)]
    image, gt = torch.zeros(C, H, W, device=dev), torch.zeros(C, H, W, device=dev)
    mask = U.transient_parameters(H, W, 0.5, dev)
    sched = ViewSchedule(ORDER, V, dev)
    bank = ViewBank(sched)
    bank.add_input("image", image, [torch.from_numpy(r[0]).to(dev) for r in rows])
    bank.add_input("gt", gt, [torch.from_numpy(r[1]).to(dev) for r in rows])
    bank.add_state("transient_mask", mask, [torch.full((H, W), 0.5, device=dev), torch.from_numpy(rows[1][2]).to(dev)])
    opt = FusedAdam([mask], lr=1e-2, capturable=True)
    mask.grad = torch.zeros_like(mask)
    opt.step()  # creates the state; a zero gradient moves nothing, and load() overwrites the working tensors
    bank.attach_optimizer(opt)
    weight = torch.full((1,), 0.1, device=dev)

    def fn():
        bank.load()
        opt.zero_grad(set_to_none=True)
        total, loss, stats = U.transient_nll(image, gt, mask, weight=weight)
        total.backward()
        gate = captured_gate()  # (None in an eager run)
        opt.step(gate=gate)
        bank.store(gate)
        sched.advance(gate)
        return loss.detach()

    names = ("transient_mask", "transient_mask.exp_avg", "transient_mask.exp_avg_sq", "transient_mask.step")
    snap = lambda: {(n, v): _bits(bank.row(n, v)) for n in names for v in range(V)}  # noqa: E731
    untouched = []
    step = None
    for it, view in enumerate(ORDER):
        before = snap()
        if graphed and it > 0:
            if step is None:
                step = GraphedStep(fn, warmup=1)  # (its eager warm-up run really runs fn: it is this iteration)
            else:
                step()
        else:
            fn()
        torch.cuda.synchronize()
        after = snap()
        untouched.append(all(after[(n, 1 - view)] == before[(n, 1 - view)] for n in names))
        assert any(after[(n, view)] != before[(n, view)] for n in names), it
    assert sched.position() == len(ORDER)
    if graphed:
        assert step.replays == len(ORDER) - 2 and step.recaptures == 0
    return snap(), untouched, [float(bank.row("transient_mask.step", v)) for v in range(V)]


def test_per_view_masks_in_a_recorded_step_match_the_eager_loop(dev):
    eager, e_untouched, e_steps = _chain(dev, graphed=False)
    graph, g_untouched, g_steps = _chain(dev, graphed=True)
    assert e_steps == g_steps == [float(ORDER.count(v)) for v in range(2)]
    assert all(e_untouched) and all(g_untouched)  # the row of the view not visited keeps its bits, in every iteration
    assert sorted(eager) == sorted(graph)
    for key in eager:
        assert eager[key] == graph[key], key  # masks, both moments and step counts of both views, bit for bit


# ---- 6. the example ----
def test_example_with_the_term_records_once_and_matches_the_eager_loop(dev):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_synthetic as ex
    finally:
        sys.path.pop(0)
    # the scene of tests/test_gpu_example.py's smallest runs; twelve iterations reach no prune point, so whatever records a second
    # time is the term's doing
    args = ["--gaussians", "30000", "--size", "192", "--iters", "12", "--quiet", "--optimizer-in-graph", "--views", "2",
            "--transient-nll", "0.1", "--transient-from", "3"]
    runs = []
    for extra in ([], ["--graph"]):
        out = ex.main(args + extra)
        runs.append((out, ex.main.last_params, ex.main.view_bank.state_dict(), ex.main.last_recordings, ex.main.last_transient))
    (eager, e_params, e_rows, _, e_tr), (graph, g_params, g_rows, recordings, g_tr) = runs
    assert recordings == 1 and ex.main.last_step.replays >= 10  # recorded exactly once; the switch at iteration 3 was a write
    assert graph == eager, (eager, graph)
    for k in e_params:
        assert _bits(e_params[k]) == _bits(g_params[k]), k
    assert sorted(e_rows) == sorted(g_rows) and "transient_mask" in e_rows and "transient_mask.exp_avg" in e_rows
    for k in e_rows:
        assert _bits(e_rows[k]) == _bits(g_rows[k]), k
    assert e_tr == g_tr and e_tr["weight"] == pytest.approx(0.1)
    assert not _bits(e_rows["transient_mask"][0]) == _bits(torch.full_like(e_rows["transient_mask"][0], e_tr["init"]))  # the masks moved
