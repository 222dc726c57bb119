"""GPU (MI355X): the device-side view bank (include/eogs_views.h, eogs2_amd.views).

The kernels move bits, so every comparison is on bits (as int32: NaN payloads count) and the bank's tolerance is zero. What
is tested: the copy at its edges (payloads around the 16-byte and the workgroup boundaries, misaligned working tensors, 1, 32
and 33 slots, an empty slot) inside sentinel-filled allocations; an out-of-range order entry written below the Python check;
the gate; `load`, `store` and `advance` recorded into a graph and replayed across the wrap of the order; Adam with one step
count per view against three separate optimizers (bit for bit) and against float64 torch.optim.Adam (the per-step bound of
tests/optim_cases.py); and a replay that outgrew its workspaces at a view change, which updates nothing and is recorded again."""
import ctypes
import functools

import pytest
import torch

import optim_cases as oc
import views_cases as VC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wg_bytes(dev):
    from eogs2_amd import _lib

    n = ctypes.c_size_t()
    assert _lib.get().views_wg_bytes(ctypes.byref(n)) == 0
    return n.value


def _gate(dev, a, b):
    return torch.tensor([a, b], dtype=torch.int32, device=dev).view(torch.uint32)


class _RawSchedule:
    """order / cursor / current on the device and the C descriptor over them, below eogs2_amd.views' checks."""

    def __init__(self, order, n_views, dev, cursor=0, current=-7):
        from eogs2_amd._abi import ViewsSchedule

        self.order = torch.tensor(order, dtype=torch.int32, device=dev)
        self.cursor = torch.tensor(cursor, dtype=torch.int64, device=dev)
        self.current = torch.tensor(current, dtype=torch.int32, device=dev)
        self.c = ViewsSchedule(self.order.data_ptr(), len(order), self.cursor.data_ptr(), self.current.data_ptr(), n_views)


def _raw(dev, fn, slots, sched, gate=None):
    """One C-ABI call on the current stream. slots: [(GuardedTable, working int32 tensor, flags)]."""
    from eogs2_amd import _lib
    from eogs2_amd._abi import ViewsSlot

    abi = _lib.get()
    arr = (ViewsSlot * max(1, len(slots)))()
    for a, (tab, work, flags) in zip(arr, slots):
        a.table, a.working = tab.base.data_ptr(), work.data_ptr()
        a.row_stride, a.row_bytes, a.flags = 4 * tab.stride_words, 4 * tab.row_words, flags
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if fn == "load":
        abi.check(abi.views_load(len(slots), ctypes.cast(arr, ctypes.c_void_p), ctypes.byref(sched.c), stream))
    elif fn == "store":
        abi.check(abi.views_store(len(slots), ctypes.cast(arr, ctypes.c_void_p), ctypes.byref(sched.c), None if gate is None else ctypes.c_void_p(gate.data_ptr()), stream))
    else:
        abi.check(abi.views_advance(ctypes.byref(sched.c), None if gate is None else ctypes.c_void_p(gate.data_ptr()), stream))


def _filled_table(V, n, dev, seed, **kw):
    tab = VC.GuardedTable(V, n, dev, **kw)
    rows = [VC.random_bits(n, seed + v) for v in range(V)]
    for v in range(V):
        tab.set_row(v, rows[v].to(dev))
    return tab, rows


# ---- 1. the copy at its edges ----
@pytest.mark.parametrize("which", range(14))
def test_load_and_store_move_exactly_the_addressed_bits(dev, wg_bytes, which):
    n = VC.payloads(wg_bytes)[which]
    for V in VC.V_CASES:
        for view in sorted({0, V - 1}):
            for lead in VC.LEADS:
                seed = 1000 * which + 100 * V + 10 * view + lead
                state_tab, state_rows = _filled_table(V, n, dev, seed)
                input_tab, input_rows = _filled_table(V, n, dev, seed + 50)
                state_w, input_w = VC.Guarded(n, dev, lead), VC.Guarded(n, dev, (lead + 1) % 4)
                sched = _RawSchedule([view], V, dev)
                slots = [(state_tab, state_w.body, 3), (input_tab, input_w.body, 1)]
                before = (state_tab.snapshot(), input_tab.snapshot())
                _raw(dev, "load", slots, sched)
                what = (n, V, view, lead)
                assert int(sched.current) == view and int(sched.cursor) == 0, what
                assert torch.equal(state_w.body.cpu(), state_rows[view]) and state_w.guards_intact(), what
                assert torch.equal(input_w.body.cpu(), input_rows[view]) and input_w.guards_intact(), what
                assert torch.equal(state_tab.snapshot(), before[0]) and torch.equal(input_tab.snapshot(), before[1]), what
                new_state, new_input = VC.random_bits(n, seed + 7), VC.random_bits(n, seed + 8)
                state_w.body.copy_(new_state.to(dev))
                input_w.body.copy_(new_input.to(dev))
                _raw(dev, "store", slots, sched)
                want = before[0].clone()
                s = state_tab.front + view * state_tab.stride_words
                want[s:s + n] = new_state
                assert torch.equal(state_tab.snapshot(), want), what  # the addressed row; every other row, padding and guard as before
                assert state_tab.outside_rows_intact(), what
                assert torch.equal(input_tab.snapshot(), before[1]), what  # a LOAD-only slot is not written by store
                assert torch.equal(state_w.body.cpu(), new_state) and state_w.guards_intact(), what
                assert torch.equal(input_w.body.cpu(), new_input) and input_w.guards_intact(), what
                assert int(sched.current) == view and int(sched.cursor) == 0, what


def test_thirty_two_slots_in_one_call_with_an_empty_one(dev, wg_bytes):
    w = wg_bytes // 4
    sizes = [1, 3, 4, 5, 0, 9, 12, w - 1, w, w + 1, 1023, 1025] + [2 + 3 * k for k in range(20)]
    assert len(sizes) == 32
    V, view = 3, 1
    tabs, works, slots, rows = [], [], [], []
    for k, n in enumerate(sizes):
        tab, r = _filled_table(V, n, dev, 5000 + 10 * k)
        wk = VC.Guarded(n, dev, k % 4)
        tabs.append(tab); works.append(wk); rows.append(r)
        slots.append((tab, wk.body, 3 if k % 3 else 1))
    sched = _RawSchedule([2, view, 0], V, dev, cursor=4)  # 4 mod 3 = 1
    _raw(dev, "load", slots, sched)
    assert int(sched.current) == view
    for k, n in enumerate(sizes):
        assert torch.equal(works[k].body.cpu(), rows[k][view]) and works[k].guards_intact(), (k, n)
    new = [VC.random_bits(n, 6000 + k) for k, n in enumerate(sizes)]
    for k in range(32):
        works[k].body.copy_(new[k].to(dev))
    before = [t.snapshot() for t in tabs]
    _raw(dev, "store", slots, sched)
    for k, n in enumerate(sizes):
        want = before[k].clone()
        if k % 3:
            s = tabs[k].front + view * tabs[k].stride_words
            want[s:s + n] = new[k]
        assert torch.equal(tabs[k].snapshot(), want) and tabs[k].outside_rows_intact(), (k, n)
        assert works[k].guards_intact()


def test_thirty_three_slots_through_the_python_loop(dev):
    from eogs2_amd.views import ViewBank, ViewSchedule

    V = 3
    sched = ViewSchedule([2, 0, 1], V, dev)
    bank = ViewBank(sched)
    works, rows = [], []
    for k in range(33):
        n = 1 + (5 * k) % 23
        g = VC.Guarded(n, dev, k % 4)
        w = g.body.view(torch.float32)
        r = [VC.random_bits(n, 9000 + 10 * k + v).view(torch.float32).to(dev) for v in range(V)]
        (bank.add_state if k % 2 else bank.add_input)(f"s{k}", w, r)
        works.append(g); rows.append(r)
    assert [d[0] for d in bank._descriptors()] == [32, 1]
    bank.load()
    assert int(sched.current) == 2
    for k in range(33):
        assert VC.same_bits(works[k].body.view(torch.float32), rows[k][2]) and works[k].guards_intact(), k
        assert VC.same_bits(bank.row(f"s{k}", 0), rows[k][0])
    for k in range(33):
        works[k].body.copy_(VC.random_bits(works[k].n, 9500 + k).to(dev))
    bank.store()
    sched.advance()
    assert sched.position() == 1
    for k in range(33):
        want = VC.random_bits(works[k].n, 9500 + k).view(torch.float32) if k % 2 else rows[k][2].cpu()
        assert VC.same_bits(bank.row(f"s{k}", 2).cpu(), want), k
        assert VC.same_bits(bank.row(f"s{k}", 1), rows[k][1])
    # state_dict round trip, and the refusals on the device
    sd = bank.state_dict()
    bank.row("s1", 0).zero_()
    bank.load_state_dict(sd)
    assert VC.same_bits(bank.row("s1", 0), rows[1][0])
    with pytest.raises(ValueError, match="contiguous"):
        bank.add_state("t", torch.zeros(4, 6, device=dev).t())
    with pytest.raises(ValueError, match="exists already"):
        bank.add_state("s0", torch.zeros(4, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bank.add_state("c", torch.zeros(4))
    other = ViewBank(type("S", (), {"n_views": 3, "device": torch.device("cuda", 1)})())
    with pytest.raises(RuntimeError, match="lives on"):
        other.add_state("x", torch.zeros(4, device=dev))
    with pytest.raises(RuntimeError, match="gate"):
        bank.store(gate=torch.zeros(2, device=dev))
    assert len(bank.names()) == 33


# ---- 2. an order entry that names no view ----
@pytest.mark.parametrize("entry", ["V", "-1"])
def test_out_of_range_order_entry_touches_nothing(dev, wg_bytes, entry):
    V, n = 3, wg_bytes // 4 + 5
    bad = {"V": V, "-1": -1}[entry]
    # the guard rows belong to the same allocation as the table: even a kernel that formed an address from the entry would
    # stay inside memory this test owns
    tab, rows = _filled_table(V, n, dev, 77, rows_front=1, rows_back=1)
    inp, _ = _filled_table(V, n, dev, 78, rows_front=1, rows_back=1)
    w1, w2 = VC.Guarded(n, dev), VC.Guarded(n, dev, 1)
    w1.body.copy_(VC.random_bits(n, 79).to(dev))
    w2.body.copy_(VC.random_bits(n, 80).to(dev))
    sched = _RawSchedule([0, bad, 1], V, dev, cursor=1, current=0)
    slots = [(tab, w1.body, 3), (inp, w2.body, 1)]
    before = [tab.snapshot(), inp.snapshot(), w1.all.cpu().clone(), w2.all.cpu().clone()]

    def unchanged():
        now = [tab.snapshot(), inp.snapshot(), w1.all.cpu(), w2.all.cpu()]
        return all(torch.equal(a, b) for a, b in zip(now, before))

    _raw(dev, "load", slots, sched)
    assert int(sched.current) == -1 and int(sched.cursor) == 1 and unchanged()
    _raw(dev, "store", slots, sched)
    _raw(dev, "advance", [], sched)
    assert int(sched.current) == -1 and int(sched.cursor) == 1 and unchanged()
    # `current` itself out of range (a caller that wrote it): store still forms no address
    sched.current.fill_(bad)
    _raw(dev, "store", slots, sched)
    assert unchanged()
    # the neighbouring entries are served as usual
    sched.cursor.fill_(2)
    _raw(dev, "load", slots, sched)
    assert int(sched.current) == 1 and torch.equal(w1.body.cpu(), rows[1])


# ---- 3. the gate ----
def test_closed_gate_writes_nothing_and_open_equals_none(dev):
    from eogs2_amd.views import ViewBank, ViewSchedule

    results = []
    for gate in (_gate(dev, 0, 1), _gate(dev, 1, 0), None):
        sched = ViewSchedule([1, 0], 2, dev)
        bank = ViewBank(sched)
        w = VC.random_bits(4099, 1).view(torch.float32).to(dev)
        small = VC.random_bits(3, 2).view(torch.float32).to(dev)
        bank.add_state("w", w, [VC.random_bits(4099, 10 + v).view(torch.float32).to(dev) for v in range(2)])
        bank.add_state("small", small)
        bank.load()
        w.copy_(VC.random_bits(4099, 3).view(torch.float32).to(dev))
        small.copy_(VC.random_bits(3, 4).view(torch.float32).to(dev))
        before = (bank.state_dict(), sched.position(), int(sched.current))
        bank.store(gate)
        sched.advance(gate)
        after = (bank.state_dict(), sched.position(), int(sched.current))
        if gate is not None and int(gate.view(torch.int32)[0]) == 0:
            assert after[1:] == before[1:] == (0, 1)
            assert all(VC.same_bits(after[0][k], before[0][k]) for k in before[0])
        else:
            assert after[1:] == (1, 1)
            assert VC.same_bits(after[0]["w"][1], w.cpu()) and VC.same_bits(after[0]["w"][0], before[0]["w"][0])
            assert VC.same_bits(after[0]["small"][1], small.cpu())
            results.append(after[0])
    assert all(VC.same_bits(results[0][k], results[1][k]) for k in results[0])


# ---- 4. capture ----
def test_recorded_load_store_advance_follow_the_order(dev):
    from eogs2_amd.views import ViewBank, ViewSchedule

    V, order = 3, [2, 0, 0, 1, 2, 2, 0]
    L = len(order)
    sched = ViewSchedule(order, V, dev)
    bank = ViewBank(sched)
    state = torch.zeros(5, device=dev)
    inp = torch.zeros(5, device=dev)
    inputs = [torch.arange(5, dtype=torch.float32) * 0.25 + v + 1 for v in range(V)]
    bank.add_input("inp", inp, [t.to(dev) for t in inputs])
    bank.add_state("state", state, [torch.full((5,), float(10 * v), device=dev) for v in range(V)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        bank.load()
        state.mul_(1.5).add_(inp)
        bank.store()
        sched.advance()
    assert sched.position() == 0 and int(sched.current) == -1  # a capture runs nothing
    want = [torch.full((5,), float(10 * v)) for v in range(V)]
    for k in range(2 * L + 1):
        graph.replay()
        v = order[k % L]
        want[v] = want[v] * 1.5 + inputs[v]
        assert int(sched.current) == v and sched.position() == k + 1, k
        for u in range(V):  # each view's row holds what its own visits wrote
            assert VC.same_bits(bank.row("state", u).cpu(), want[u]), (k, u)
    sched.seek(3)  # takes effect without a new recording
    graph.replay()
    want[1] = want[1] * 1.5 + inputs[1]
    assert int(sched.current) == order[3] == 1 and sched.position() == 4
    assert VC.same_bits(bank.row("state", 1).cpu(), want[1]) and VC.same_bits(state.cpu(), want[1])


def test_cursor_beyond_32_bits_takes_the_wide_remainder(dev):
    from eogs2_amd.views import ViewBank, ViewSchedule

    order = [2, 0, 1, 1, 0, 2, 1]
    sched = ViewSchedule(order, 3, dev)
    bank = ViewBank(sched)
    w = torch.zeros(6, device=dev)
    bank.add_state("w", w, [torch.full((6,), float(v + 1), device=dev) for v in range(3)])
    for cursor in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40 + 3, 2 ** 62 + 1):
        sched.seek(cursor)
        bank.load()
        v = order[cursor % len(order)]
        assert int(sched.current) == v and float(w[0]) == v + 1, cursor
        sched.advance()
        assert sched.position() == cursor + 1


# ---- 5. Adam per view ----
def _camera_sets(dev, V):
    names = sorted(VC.ADAM_SHAPES)
    return names, [[torch.nn.Parameter(VC.adam_initial(n, v).to(dev)) for n in names] for v in range(V)]


@functools.lru_cache(maxsize=None)
def _separate_reference():
    """Three FusedAdam(capturable=True), each stepped only on its own view's iterations: the final state per view and, per
    iteration, (view, visit, state before, state after) on the CPU."""
    from eogs2_amd.optim import FusedAdam

    dev = torch.device("cuda:0")
    names, sets = _camera_sets(dev, VC.ADAM_V)
    opts = [FusedAdam(ps, lr=VC.ADAM_LR, betas=VC.ADAM_BETAS, eps=VC.ADAM_EPS, capturable=True) for ps in sets]
    seen, trace = [0] * VC.ADAM_V, []

    def snap(v):
        out = {}
        for n, p in zip(names, sets[v]):
            st = opts[v].state.get(p) or {}
            out[n] = (p.detach().cpu().clone(), *(st[k].cpu().clone() if st else torch.zeros(p.shape) for k in ("exp_avg", "exp_avg_sq")),
                      st["step"].cpu().clone() if st else torch.zeros(()))
        return out

    for v in VC.ADAM_ORDER:
        before = snap(v)
        for n, p in zip(names, sets[v]):
            p.grad = VC.adam_grad(n, v, seen[v]).to(dev)
        opts[v].step()
        trace.append((v, seen[v], before, snap(v)))
        seen[v] += 1
    return [snap(v) for v in range(VC.ADAM_V)], trace


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_adam_counts_and_moments_are_per_view(dev, mode):
    from eogs2_amd.optim import FusedAdam
    from eogs2_amd.views import ViewBank, ViewSchedule

    V = VC.ADAM_V
    names = sorted(VC.ADAM_SHAPES)
    work = [torch.nn.Parameter(VC.adam_initial(n, 0).to(dev)) for n in names]
    opt = FusedAdam(work, lr=VC.ADAM_LR, betas=VC.ADAM_BETAS, eps=VC.ADAM_EPS, capturable=True)
    sched = ViewSchedule(VC.ADAM_ORDER, V, dev)
    bank = ViewBank(sched)
    for n, p in zip(names, work):
        bank.add_state(n, p, [VC.adam_initial(n, v).to(dev) for v in range(V)])
    with pytest.raises(RuntimeError, match="eagerly first"):
        bank.attach_optimizer(opt)
    for p in work:  # the eager step that creates the state: zero gradients move nothing, and load() overwrites the rest
        p.grad = torch.zeros_like(p)
    opt.step()
    bank.attach_optimizer(opt)
    assert len(bank.names()) == 12
    # gradients: a table per parameter over (view, visit), gathered on the device by `current` and the view's own count
    max_visits = max(VC.visits(VC.ADAM_ORDER, V))
    gtab = {n: torch.stack([torch.stack([VC.adam_grad(n, v, k) for k in range(max_visits)]) for v in range(V)]).to(dev) for n in names}
    grads = [torch.zeros_like(p) for p in work]
    step0 = opt.state[work[0]]["step"]

    def fn():
        bank.load()
        visit = step0.to(torch.int64)  # this view's updates so far = its visit number
        for n, p, g in zip(names, work, grads):
            g.copy_(gtab[n].index_select(0, sched.current.to(torch.int64).reshape(1))[0].index_select(0, visit.reshape(1))[0])
            p.grad = g
        opt.step()
        bank.store()
        sched.advance()

    if mode == "eager":
        for _ in VC.ADAM_ORDER:
            fn()
    else:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fn()
        for _ in VC.ADAM_ORDER:
            graph.replay()
    torch.cuda.synchronize()
    assert sched.position() == len(VC.ADAM_ORDER)
    want, _ = _separate_reference()
    counts = VC.visits(VC.ADAM_ORDER, V)
    for v in range(V):
        for n in names:
            p, m, s, t = want[v][n]
            assert VC.same_bits(bank.row(n, v).cpu(), p), (v, n)
            assert VC.same_bits(bank.row(n + ".exp_avg", v).cpu(), m), (v, n)
            assert VC.same_bits(bank.row(n + ".exp_avg_sq", v).cpu(), s), (v, n)
            assert VC.same_bits(bank.row(n + ".step", v).cpu(), t) and float(bank.row(n + ".step", v)) == counts[v], (v, n)
    # what the reference saves for camera_optimizer: a torch.optim.Adam with one group per view takes it
    sd = bank.adam_state_dict(names)
    params = [[torch.nn.Parameter(bank.row(n, v).cpu().clone()) for n in names] for v in range(V)]
    ref = torch.optim.Adam([{"params": ps} for ps in params], lr=VC.ADAM_LR, betas=VC.ADAM_BETAS, eps=VC.ADAM_EPS)
    ref.load_state_dict(sd)
    assert [int(ref.state[params[v][0]]["step"]) for v in range(V)] == counts


def test_adam_per_view_against_float64_torch_adam(dev):
    """float64 torch.optim.Adam, one group per view, grad None for the views an iteration does not visit: every step of
    the separate optimizers (= the bank's, bit for bit: the test above) stays inside FACTOR_KERNEL x the per-step bound
    of tests/optim_cases.py, from the fp32 state the step started with."""
    names = sorted(VC.ADAM_SHAPES)
    _, trace = _separate_reference()
    params = [[torch.nn.Parameter(VC.adam_initial(n, v).double()) for n in names] for v in range(VC.ADAM_V)]
    ref = torch.optim.Adam([{"params": ps} for ps in params], lr=VC.ADAM_LR, betas=VC.ADAM_BETAS, eps=VC.ADAM_EPS)
    worst = 0.0
    for v, visit, before, after in trace:
        ref.zero_grad(set_to_none=True)  # the other views: grad None, skipped, their counts stay
        for n, p in zip(names, params[v]):
            p0, m0, v0, t0 = before[n]
            assert int(t0) == visit
            with torch.no_grad():
                p.copy_(p0.double())
                if visit:  # the fp32 state this step starts from, in double; the step count stays torch's own
                    ref.state[p]["exp_avg"].copy_(m0.double())
                    ref.state[p]["exp_avg_sq"].copy_(v0.double())
            p.grad = VC.adam_grad(n, v, visit).double()
        ref.step()
        for n, p in zip(names, params[v]):
            p0, m0, v0, _ = before[n]
            p1, m1, v1, t1 = after[n]
            assert int(ref.state[p]["step"]) == int(t1) == visit + 1
            bm, bv, bp = oc.adam_step_bound(p0, VC.adam_grad(n, v, visit), m0, v0, VC.ADAM_LR, VC.ADAM_BETAS, VC.ADAM_EPS, visit + 1)
            for what, got, ref64, b in (("exp_avg", m1, ref.state[p]["exp_avg"], bm), ("exp_avg_sq", v1, ref.state[p]["exp_avg_sq"], bv),
                                        ("param", p1, p.detach(), bp)):
                ratio = float(((got.double() - ref64).abs() / b).max())
                worst = max(worst, ratio)
                assert ratio <= oc.FACTOR_KERNEL, (what, n, v, visit, ratio)
    print(f"worst error / bound over {len(trace)} steps: {worst:.3f}")
    assert [int(ref.state[params[v][0]]["step"]) for v in range(VC.ADAM_V)] == VC.visits(VC.ADAM_ORDER, VC.ADAM_V)


# ---- 6. a replay that outgrew its workspaces at a view change ----
NAMES = ("means3D", "colors", "opacities", "scales", "rotations")
LRS = {"means3D": 1e-5, "colors": 1e-3, "opacities": 1e-3, "scales": 1e-6, "rotations": 1e-4}
OUTGROWN_ORDER = (0, 0, 0, 1, 1, 0, 1)


class _TwoViews:
    """render -> L1 loss (with a per-view colour offset) -> backward -> gate -> both optimizers -> store -> advance, over a
    two-view bank: the view matrix and the target are inputs, the colour offset and its Adam state are per-view state."""

    P, H, W = 20021, 200, 168  # (a shape no other test renders: its counts are forgotten below)

    def __init__(self, dev, seed=23):
        from eogs2_amd import GaussianRasterizationSettings, GaussianRasterizer
        from eogs2_amd.optim import FusedAdam
        from eogs2_amd.synthetic import make_scene, settings_for
        from eogs2_amd.views import ViewBank, ViewSchedule

        P, H, W = self.P, self.H, self.W
        sc = make_scene(P, H, W, seed=seed, opacity="trained", device=dev, scale_mult=2.0)
        self.vm = sc["viewmatrix"].clone()  # the working matrix: the rasterizer reads it by address
        wide = sc["viewmatrix"].clone()
        narrow = sc["viewmatrix"].clone()
        narrow[:, :2] *= 0.3  # the same scene, smaller on the screen: far fewer (tile, Gaussian) pairs than `wide`
        rs = settings_for(sc, H, W)._replace(viewmatrix=self.vm, projmatrix=self.vm)
        assert isinstance(rs, GaussianRasterizationSettings)
        self.rast = GaussianRasterizer(rs)
        self.params = {k: torch.nn.Parameter(sc[k].clone()) for k in NAMES}
        self.m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        g = torch.Generator().manual_seed(seed + 1)
        self.target = torch.zeros(5, H, W, device=dev)
        self.offset = torch.nn.Parameter(torch.zeros(5, 1, 1, device=dev))
        self.opt = FusedAdam([{"params": [self.params[k]], "lr": LRS[k], "name": k} for k in NAMES], lr=0.0, eps=1e-15, capturable=True)
        self.cam_opt = FusedAdam([self.offset], lr=1e-3, capturable=True)
        self.sched = ViewSchedule(OUTGROWN_ORDER, 2, dev)
        self.bank = ViewBank(self.sched)
        self.bank.add_input("vm", self.vm, [narrow, wide])
        self.bank.add_input("target", self.target, [torch.rand(5, H, W, generator=g).to(dev) for _ in range(2)])
        self.bank.add_state("offset", self.offset, [torch.full((5, 1, 1), 0.01 * (v + 1), device=dev) for v in range(2)])
        self.offset.grad = torch.zeros_like(self.offset)
        self.cam_opt.step()  # creates the state; a zero gradient moves nothing
        self.bank.attach_optimizer(self.cam_opt)

    def pairs(self, view):
        """(record slots, list entries) of an eager forward through view `view`'s matrix."""
        from eogs2_amd import rasterizer

        self.vm.copy_(self.bank.row("vm", view))
        p = self.params
        with torch.no_grad():
            self.rast(p["means3D"], self.m2, p["opacities"], colors_precomp=p["colors"], scales=p["scales"], rotations=p["rotations"])
        token = rasterizer.last_exact_token(self.vm.device)
        return token & rasterizer._SLOTS, (token & rasterizer._ENTRIES) >> 32

    def __call__(self):
        from eogs2_amd import rasterizer

        self.bank.load()
        p = self.params
        for t in (*p.values(), self.m2, self.offset):
            t.grad = None
        color, _, _ = self.rast(p["means3D"], self.m2, p["opacities"], colors_precomp=p["colors"], scales=p["scales"],
                                rotations=p["rotations"])
        loss = (color + self.offset - self.target).abs().mean()
        loss.backward()
        gate = rasterizer.captured_gate()  # (None in an eager run)
        self.opt.step(gate=gate)
        self.cam_opt.step(gate=gate)
        self.bank.store(gate)
        self.sched.advance(gate)
        return loss.detach()

    def state(self):
        """(what an outgrown replay must leave alone: cursor, model, its Adam state, every row; the working per-view tensors)"""
        core = [self.sched.cursor.cpu().clone()]
        for k in NAMES:
            st = self.opt.state[self.params[k]]
            core += [self.params[k].detach().cpu().clone(), st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone(), st["step"].cpu().clone()]
        sd = self.bank.state_dict()
        core += [sd[k] for k in sorted(sd)]
        st = self.cam_opt.state[self.offset]
        return core, [self.offset.detach().cpu().clone(), st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone(), st["step"].cpu().clone()]


def _forget_counts(t):
    """The counts the eager forwards of this shape left behind: a recording is sized from them (eogs2_amd.rasterizer._peak)."""
    from eogs2_amd import rasterizer

    for store in (rasterizer._peak, rasterizer._spec):
        for key in [k for k in store if tuple(k[1:4]) == (t.P, t.H, t.W)]:
            del store[key]


def _same(a, b):
    a, b = (x if isinstance(x, list) else x[0] + x[1] for x in (a, b))
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert VC.same_bits(x, y), i


def test_outgrown_replay_at_a_view_change_updates_nothing_and_is_recorded_again(dev):
    from eogs2_amd.graph import GraphedStep

    a, b = _TwoViews(dev), _TwoViews(dev)
    small, large = a.pairs(0), a.pairs(1)
    print(f"(record slots, list entries): view 0 {small}, view 1 {large}")
    assert large[0] > 1.25 * small[0] + 4096, (small, large)  # beyond GraphedStep's capacity margin (eogs_rast_capacity_token)
    _forget_counts(a)  # the recording below must be sized by view 0 alone, as in a run that has not met view 1 yet
    g = GraphedStep(a, warmup=1, idempotent=True)  # (the warm-up run is a real iteration: view 0, cursor 0 -> 1)
    want = [b()]
    _same(a.state(), b.state())
    got = [g().clone(), g().clone()]  # view 0 twice more
    want += [b().clone(), b().clone()]
    assert g.recaptures == 0 and a.sched.position() == 3
    _same(a.state(), b.state())
    # the replay that reaches view 1: the gate is closed, so no row, no working parameter and no cursor moves ...
    g.replay()
    assert not g.fits()
    torch.cuda.synchronize()
    assert int(a.sched.current) == 1 and a.sched.position() == 3
    _same(a.state()[0], b.state()[0])  # (all but the working tensors, into which load() did bring view 1's rows, unchanged:)
    working = a.state()[1]
    assert VC.same_bits(working[0], a.bank.row("offset", 1).cpu()) and not any(bool(t.any()) for t in working[1:])
    # ... and through __call__ it is recorded again and then trains view 1
    got.append(g().clone())
    want.append(b().clone())
    assert g.recaptures == 1
    for _ in range(3):
        got.append(g().clone())
        want.append(b().clone())
    torch.cuda.synchronize()
    assert g.recaptures == 1 and a.sched.position() == len(OUTGROWN_ORDER)
    assert all(torch.equal(x, y) for x, y in zip(got, want[1:]))
    _same(a.state(), b.state())
    steps = [float(a.bank.row("offset.step", v)) for v in range(2)]
    assert steps == [float(VC.visits(OUTGROWN_ORDER, 2)[v]) for v in range(2)]
