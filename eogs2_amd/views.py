"""Several views in one recorded step: a device-side view bank over the C-ABI of include/eogs_views.h.

The reference trains over all views of a scene: train_pan.py:252-257 pops a random view from `viewpoint_stack` every
iteration, :135-138 gives `camera_optimizer` one parameter group per camera, and because `torch.optim.Adam` skips parameters
without a gradient every camera's parameters advance on that camera's own step count, in the iterations that visit it. A
recorded step (`eogs2_amd.graph.GraphedStep`) reads fixed tensors by address — the ground truth, the matrices, and with the
optimizer inside the recording also the camera's parameters, both Adam moments and the device step counts. Here all views'
copies of those tensors sit in device tables, an order table and a cursor on the device say which view is current, ONE
launch brings that view's rows into the fixed working tensors and ONE gated launch writes the updated state back:

    schedule = ViewSchedule(reference_order(V, iterations), V, device)
    bank = ViewBank(schedule)
    bank.add_input("gt", gt, all_gts)                        # row -> working at load
    bank.add_state("cc.weight", cc.weight)                   # row -> working at load, working -> row at store
    camera_optimizer.step()                                  # one eager step creates the state ...
    bank.attach_optimizer(camera_optimizer)                  # ... whose moments and step counts become state slots

    def fn():                                                # the function of a GraphedStep
        bank.load()
        ... forwards, losses, backward ...
        gate = captured_gate()                               # None in an eager run
        model_optimizer.step(gate=gate); camera_optimizer.step(gate=gate)
        bank.store(gate)
        schedule.advance(gate)

A replay that outgrew its list workspaces finds the gate closed: the tables, the cursor and the working state stay as they
were, `GraphedStep` records again and replays the same view. The eager warm-up runs of a recording (at construction and in
`record_again`) really run `fn`: with the bank inside they are real iterations that consume views — count them, or `seek`
back and restore the rows if they are not meant to.

The kernels only move bits, and there is no CPU fallback.
"""
import ctypes
import random

import torch

from . import _lib
from ._abi import VIEWS_LOAD, VIEWS_MAX_SLOTS, VIEWS_STORE, ViewsSchedule, ViewsSlot
from ._host import Ctx, ptr


def reference_order(n_views, iterations, rng=random):
    """The views of `iterations` iterations as train_pan.py:252-257 draws them: the stack is refilled with 0..V-1 when it is
    empty, then `pop(rng.randint(0, len - 1))`. The same calls on `rng`, so a `random` seeded as the reference's gives the
    reference's order."""
    if n_views < 1 or iterations < 0:
        raise ValueError("reference_order: n_views >= 1, iterations >= 0")
    order, stack = [], []
    for _ in range(iterations):
        if not stack:
            stack = list(range(n_views))
        order.append(stack.pop(rng.randint(0, len(stack) - 1)))
    return order


def _check_gate(gate, dev, who):
    if gate is None:
        return
    if not (isinstance(gate, torch.Tensor) and gate.device == dev and gate.numel() == 2 and gate.is_contiguous()
            and gate.dtype in (torch.uint32, torch.int32)):
        raise RuntimeError(f"{who}: gate must be a contiguous uint32[2] tensor on the schedule's device")


def _require_device(dev, who):
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: tensors on '{dev.type}': the view bank lives on the GPU, there is no CPU fallback")


class ViewSchedule:
    """The order of the views, a cursor and the current view, all on the device (eogs_views_schedule). The current view is
    `order[cursor mod len(order)]`. Several banks may share one schedule — the PAN and the MSI camera of a view differ in
    size and are walked in the same iteration: each bank's `load()` leaves the same `current`, `advance()` is called once."""

    def __init__(self, order, n_views, device):
        order = [int(v) for v in order]
        n_views = int(n_views)
        if n_views < 1:
            raise ValueError("ViewSchedule: n_views must be positive")
        if not order:
            raise ValueError("ViewSchedule: an empty order")
        for k, v in enumerate(order):
            if not 0 <= v < n_views:
                raise ValueError(f"ViewSchedule: order[{k}] = {v} names no view (0 .. {n_views - 1})")
        device = torch.device(device)
        _require_device(device, "ViewSchedule")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.n_views, self.device = n_views, device
        self.order = torch.tensor(order, dtype=torch.int32, device=device)
        self.cursor = torch.zeros((), dtype=torch.int64, device=device)
        self.current = torch.full((), -1, dtype=torch.int32, device=device)
        self._struct = ViewsSchedule(self.order.data_ptr(), len(order), self.cursor.data_ptr(), self.current.data_ptr(), n_views)

    def __len__(self):
        return self.order.numel()

    def seek(self, k):
        """cursor = k: a device write, no wait. Between replays it takes effect without a new recording."""
        if int(k) < 0:
            raise ValueError("ViewSchedule.seek: a cursor is not negative")
        self.cursor.fill_(int(k))

    def position(self):
        """The cursor: one wait for the device."""
        return int(self.cursor)

    def advance(self, gate=None):
        """cursor += 1 on the device, unless `gate` (eogs2_amd.rasterizer.captured_gate()) is closed."""
        _check_gate(gate, self.device, "ViewSchedule.advance")
        abi = _lib.get()
        with Ctx(abi, self.device) as cx:
            abi.check(abi.views_advance(ctypes.byref(self._struct), ptr(gate), cx.stream))

    def state_dict(self):
        return {"order": self.order.cpu(), "cursor": self.position(), "n_views": self.n_views}

    def load_state_dict(self, sd):
        if int(sd["n_views"]) != self.n_views or tuple(sd["order"].shape) != tuple(self.order.shape):
            raise ValueError("ViewSchedule.load_state_dict: another number of views or another order length")
        order = sd["order"].to(torch.int32)
        if bool(((order < 0) | (order >= self.n_views)).any()):
            raise ValueError("ViewSchedule.load_state_dict: the order names a view that does not exist")
        self.order.copy_(order)
        self.seek(sd["cursor"])


class _Slot:
    __slots__ = ("name", "working", "table", "row_stride", "row_bytes", "flags")


def check_slot(name, working, rows, n_views, device, taken=()):
    """The refusals of `ViewBank.add_input` / `add_state`, before anything touches a device. Returns the rows as a list of
    n_views tensors (None: copies of `working`)."""
    if not isinstance(working, torch.Tensor):
        raise TypeError(f"ViewBank: slot {name!r}: the working tensor must be a torch.Tensor")
    if name in taken:
        raise ValueError(f"ViewBank: a slot named {name!r} exists already")
    if not working.is_contiguous():
        raise ValueError(f"ViewBank: slot {name!r}: the working tensor must be contiguous (a recorded step reads it by address)")
    if (working.numel() * working.element_size()) % 4:
        raise ValueError(f"ViewBank: slot {name!r}: a payload of {working.numel() * working.element_size()} bytes is not a multiple of 4")
    if rows is not None:
        rows = list(rows.unbind(0)) if isinstance(rows, torch.Tensor) else list(rows)
        if len(rows) != n_views:
            raise ValueError(f"ViewBank: slot {name!r}: {len(rows)} rows for {n_views} views")
        for v, r in enumerate(rows):
            if not isinstance(r, torch.Tensor) or r.shape != working.shape or r.dtype != working.dtype:
                raise ValueError(f"ViewBank: slot {name!r}: row {v} differs from the working tensor in shape or dtype")
    for t in [working] + list(rows or ()):
        if t.device.type != "cuda":
            _require_device(t.device, f"ViewBank: slot {name!r}")
        if t.device != device:
            raise RuntimeError(f"ViewBank: slot {name!r} lives on {t.device}, the schedule on {device}")
    return rows


def adam_state_dict_from_rows(rows, param_names, group):
    """The rows of a bank (`rows[name]`, `rows[name + '.exp_avg']`, `'.exp_avg_sq'`, `'.step'`: tensors of V rows each) in the
    layout of `torch.optim.Adam.state_dict()` with one group per view and the parameters `param_names` in each — what
    train_pan.py:653-660 saves for `camera_optimizer`. `group`: the hyperparameters every group carries (a dict such as
    `optimizer.state_dict()['param_groups'][0]`; its 'params' is replaced). A view that was never visited (step 0) has no
    entry in 'state', as a torch.optim.Adam that never stepped those parameters has none."""
    param_names = list(param_names)
    if not param_names:
        raise ValueError("adam_state_dict: no parameter names")
    V = len(rows[param_names[0] + ".step"])
    hyper = {k: v for k, v in group.items() if k != "params" and not isinstance(v, torch.Tensor)}
    state, groups = {}, []
    for v in range(V):
        ids = []
        for k, name in enumerate(param_names):
            i = v * len(param_names) + k
            ids.append(i)
            step = rows[name + ".step"][v].detach().reshape(()).to(device="cpu", dtype=torch.float32).clone()
            if float(step) == 0.0:
                continue
            state[i] = {"step": step, "exp_avg": rows[name + ".exp_avg"][v].detach().cpu().clone(),
                        "exp_avg_sq": rows[name + ".exp_avg_sq"][v].detach().cpu().clone()}
        groups.append({**hyper, "params": ids})
    return {"state": state, "param_groups": groups}


class ViewBank:
    """Per-view tensors of one shape set in padded device tables, and the two launches that move the current view's rows.

    add_input(name, working, rows)       row -> working at `load()`: ground truth, matrices, anything the step only reads
    add_state(name, working, rows=None)  also working -> row at `store()`: what the step updates (rows=None: every row starts
                                         as the working tensor's current value)
    attach_optimizer(optimizer)          the Adam state of every parameter registered as state joins as state slots

    The views of one bank share shapes: views of several sizes need one bank (and one recorded step) per size, over one
    shared `ViewSchedule`."""

    def __init__(self, schedule):
        self.schedule = schedule
        self.device = schedule.device
        self._slots = {}
        self._calls = None  # [(n, ctypes array)] of at most VIEWS_MAX_SLOTS descriptors each
        self._hyper = None

    def names(self):
        return list(self._slots)

    def _add(self, name, working, rows, flags):
        V = self.schedule.n_views
        rows = check_slot(name, working, rows, V, self.device, self._slots)
        s = _Slot()
        s.name, s.working, s.flags = name, working, flags
        s.row_bytes = working.numel() * working.element_size()
        s.row_stride = max(16, -(-s.row_bytes // 16) * 16)
        s.table = torch.zeros((V, s.row_stride), dtype=torch.uint8, device=self.device)
        self._slots[name] = s
        self._calls = None
        with torch.no_grad():
            for v in range(V):
                self.row(name, v).copy_(working.detach() if rows is None else rows[v].detach())
        return s

    def add_input(self, name, working, rows):
        if rows is None:
            raise ValueError(f"ViewBank.add_input: slot {name!r} needs its rows")
        self._add(name, working, rows, VIEWS_LOAD)

    def add_state(self, name, working, rows=None):
        self._add(name, working, rows, VIEWS_LOAD | VIEWS_STORE)

    def attach_optimizer(self, optimizer):
        """`optimizer`: a FusedAdam(capturable=True) that has taken one eager step. For every parameter already registered
        with `add_state` its `exp_avg`, `exp_avg_sq` and `state['step']` become state slots `<name>.exp_avg`, `.exp_avg_sq`,
        `.step` whose rows are zeros, step 0: torch's lazy initialisation, at a camera's first visit. (The parameter's own
        rows are yours: the eager step that created the state also moved the working parameter.)"""
        if not optimizer.defaults.get("capturable"):
            raise RuntimeError("ViewBank.attach_optimizer: the optimizer must be a FusedAdam(capturable=True): its step counts "
                               "are device scalars a recorded step reads")
        by_ptr = {s.working.data_ptr(): s.name for s in self._slots.values() if s.flags & VIEWS_STORE and s.row_bytes}
        found = []
        for group in optimizer.param_groups:
            for p in group["params"]:
                name = by_ptr.get(p.data_ptr())
                if name is None:
                    continue
                st = optimizer.state.get(p)
                if not st or not isinstance(st.get("step"), torch.Tensor) or st["step"].device != p.device:
                    raise RuntimeError(f"ViewBank.attach_optimizer: parameter {name!r} has no optimizer state on the device yet: "
                                       "run one optimizer step eagerly first, then attach")
                found.append((name, st, group))
        if not found:
            raise RuntimeError("ViewBank.attach_optimizer: none of the optimizer's parameters is a state slot of this bank")
        V = self.schedule.n_views
        for name, st, group in found:
            for key in ("exp_avg", "exp_avg_sq", "step"):
                self.add_state(f"{name}.{key}", st[key], [torch.zeros_like(st[key]) for _ in range(V)])
        group = found[0][2]
        self._hyper = {k: v for k, v in group.items() if k not in ("params", "lr_tensor", "lr_uploaded") and not isinstance(v, torch.Tensor)}
        self._hyper["capturable"] = False  # (the reference's camera_optimizer keeps its step counts on the host)

    def row(self, name, v):
        """Row `v` of slot `name`: a view into the table with the working tensor's shape and dtype, no copy."""
        s = self._slots[name]
        if not 0 <= int(v) < self.schedule.n_views:
            raise IndexError(f"ViewBank.row: view {v} of {self.schedule.n_views}")
        return s.table[int(v), :s.row_bytes].view(s.working.dtype).view(s.working.shape)

    def rows(self, name):
        """All rows of slot `name` as one [V, ...] tensor: a copy."""
        return torch.stack([self.row(name, v) for v in range(self.schedule.n_views)])

    def _descriptors(self):
        if self._calls is None:
            slots = list(self._slots.values())
            self._calls = []
            for i0 in range(0, len(slots), VIEWS_MAX_SLOTS):
                chunk = slots[i0:i0 + VIEWS_MAX_SLOTS]
                arr = (ViewsSlot * len(chunk))()
                for a, s in zip(arr, chunk):
                    a.table, a.working = s.table.data_ptr(), s.working.data_ptr()
                    a.row_stride, a.row_bytes, a.flags = s.row_stride, s.row_bytes, s.flags
                self._calls.append((len(chunk), ctypes.cast(arr, ctypes.c_void_p), arr))  # (arr: kept alive beside its pointer)
        return self._calls

    def load(self):
        """The current view's rows into the working tensors (and `schedule.current`): one launch per 32 slots."""
        abi = _lib.get()
        with Ctx(abi, self.device) as cx:
            for n, arr, _ in self._descriptors():
                abi.check(abi.views_load(n, arr, ctypes.byref(self.schedule._struct), cx.stream))

    def store(self, gate=None):
        """The state slots' working tensors into the rows of the view the last `load()` brought in, unless `gate` is closed."""
        _check_gate(gate, self.device, "ViewBank.store")
        abi = _lib.get()
        with Ctx(abi, self.device) as cx:
            for n, arr, _ in self._descriptors():
                abi.check(abi.views_store(n, arr, ctypes.byref(self.schedule._struct), ptr(gate), cx.stream))

    def state_dict(self):
        """{slot name: its rows as one [V, ...] tensor on the CPU}. The working tensors are not part of it: after `store()`
        the rows hold everything."""
        return {name: self.rows(name).cpu() for name in self._slots}

    def load_state_dict(self, sd):
        if set(sd) != set(self._slots):
            raise ValueError(f"ViewBank.load_state_dict: slots {sorted(set(sd) ^ set(self._slots))} are on one side only")
        V = self.schedule.n_views
        for name, s in self._slots.items():
            t = sd[name]
            if tuple(t.shape) != (V,) + tuple(s.working.shape) or t.dtype != s.working.dtype:
                raise ValueError(f"ViewBank.load_state_dict: slot {name!r} has another shape or dtype")
        with torch.no_grad():
            for name in self._slots:
                for v in range(V):
                    self.row(name, v).copy_(sd[name][v])

    def adam_state_dict(self, param_names):
        """The rows of the attached optimizer's state in the layout of `torch.optim.Adam.state_dict()` with one group per
        view (`adam_state_dict_from_rows`): what train_pan.py:653-660 saves for `camera_optimizer`."""
        if self._hyper is None:
            raise RuntimeError("ViewBank.adam_state_dict: no optimizer attached")
        names = [f"{n}.{k}" for n in param_names for k in ("step", "exp_avg", "exp_avg_sq")]
        return adam_state_dict_from_rows({n: self.rows(n).cpu() for n in names}, param_names, self._hyper)


__all__ = ["reference_order", "ViewSchedule", "ViewBank", "adam_state_dict_from_rows", "check_slot"]
