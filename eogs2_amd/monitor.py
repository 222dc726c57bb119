"""The training monitor over the C-ABI of include/eogs_monitor.h: what the reference's loop keeps on the host to WATCH the
training — the interval means of L1, photometric loss, PSNR and SSIM per camera kind, the two moving averages of the
progress bar, mean opacity, the number of Gaussians and the early stopper (train_pan.py:423-429, 471-495, 512-597;
utils/callback_utils.py:15-44) — kept in one device buffer and advanced by kernel launches alone.

    mon = TrainingMonitor(dev, metric_name="photometric", operator="min", patience=5)
    loss, Ll1, out = photometric_loss(image, gt, lam, return_out=True)
    mon.observe(image, gt, cam.image_type, loss_out=out, lambda_dssim=lam)   # per camera
    mon.observe_model(gaussians._opacity)
    mon.end_iteration(total_loss)                                            # per iteration
    if iteration % 10 == 0:
        mon.close_interval()
        record = mon.fetch()          # the one wait of the interval; or fetch_async() ... poll()

The reference reads five or more scalars back per camera per iteration and evaluates SSIM a second time for its log; here
nothing waits until `fetch()`, and with `loss_out` the only image pass is the per-plane sum of squared differences of the
PSNR. Every call is a few launches on the current stream, allocates nothing after its first use of a shape and reads its
changing scalars from device memory: a stream capture records it (eogs2_amd.graph.GraphedStep). `gate` is the uint32[2] of
`eogs2_amd.rasterizer.captured_gate()`: a call with gate[0] == 0 leaves every byte of the state as it was.

One monitor belongs to one stream at a time (its reduction workspaces are reused from call to call). fp32 images; CPU
tensors raise: there is no CPU fallback.
"""
import collections
import ctypes
import functools

import torch

from . import _lib
from ._abi import MONITOR_KINDS, MONITOR_METRICS, MONITOR_OPERATORS, MONITOR_RING, MonitorRecord, MonitorState
from ._host import call, on_device, query_bytes

HOST_METRICS = ("mae", "mae_wtree")  # what the reference's metric_dict holds beside the six: computed on the host there
_RECORD_BYTES = ctypes.sizeof(MonitorRecord)
_LATEST_OFFSET = MonitorState.latest.offset


_on_device = functools.partial(on_device, "monitor", "the monitor runs", non_tensor="got")


def _record_dict(r):
    d = {"interval": int(r.interval), "iteration": int(r.iteration)}
    d.update(zip(MONITOR_METRICS, (float(v) for v in r.means)))
    d.update(ema_loss=float(r.ema_loss), ema_photometric=float(r.ema_photometric), mean_opacity=float(r.mean_opacity),
             rows=int(r.rows), best=float(r.best), counter=int(r.counter), early_stop=bool(r.early_stop))
    return d


def _kind(kind):
    if kind not in MONITOR_KINDS:
        raise ValueError(f"Unknown camera type {kind}, should be either 'pan' or 'msi'")  # train_pan.py:486-489
    return MONITOR_KINDS.index(kind)


def _metric(metric_name):
    if metric_name not in MONITOR_METRICS:
        host = " (the reference computes it on the host: feed its own early stopper)" if metric_name in HOST_METRICS else ""
        raise ValueError(f"monitor: metric_name {metric_name!r} is not held on the device{host}; it is one of {MONITOR_METRICS}")
    return MONITOR_METRICS.index(metric_name)


def _operator(operator):
    if operator not in MONITOR_OPERATORS:
        raise ValueError("operator should be either min or max")  # callback_utils.py:43
    return MONITOR_OPERATORS.index(operator)


class TrainingMonitor:
    """Device-resident monitor; see the module docstring. `patience=None` is `use_early_stopping: False`: the records are
    written, the stopper's state stays at its start. `metric_name` is one of MONITOR_METRICS."""

    def __init__(self, device, metric_name="photometric", operator="min", patience=5):
        self.metric, self.op = _metric(metric_name), _operator(operator)
        self.metric_name, self.operator = metric_name, operator
        if patience is not None and int(patience) < 0:
            raise ValueError(f"monitor: patience is a non-negative integer or None, got {patience}")
        self.patience = -1 if patience is None else int(patience)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"monitor: device '{device.type}'; the monitor runs on the GPU only, there is no CPU fallback")
        self._device = device
        self._state = None  # allocated and reset at the first use: constructing a monitor touches no device
        self._ws = {}  # (call, shape) -> workspace, kept: a recorded graph points into it
        self._pending = collections.deque()  # fetch_async: (event, pinned buffer)
        self._polled = None

    # ---- device side -------------------------------------------------------------------------------------------------
    @property
    def device(self):
        if self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    @property
    def state(self):
        """The device buffer (uint8, eogs_monitor_state). Use the monitor once OUTSIDE a capture before recording it."""
        if self._state is None:
            n = ctypes.c_size_t()
            abi = _lib.get()
            abi.check(abi.monitor_state_bytes(ctypes.byref(n)))
            if n.value != ctypes.sizeof(MonitorState):
                raise RuntimeError(f"monitor: the library's state holds {n.value} bytes, _abi.MonitorState {ctypes.sizeof(MonitorState)}")
            self._state = torch.empty((n.value,), dtype=torch.uint8, device=self.device)
            self.reset()
        return self._state

    def reset(self):
        """Zero sums, counts, averages and ring; best = +inf (min) or -inf (max). One launch."""
        st = self.state if self._state is None else self._state  # (the first access resets by itself)
        call("eogs_monitor_reset", self.device, st.data_ptr(), st.numel(), self.op)

    def _gate(self, gate, what):
        if gate is None:
            return None
        _on_device(gate, what)
        if gate.dtype not in (torch.int32, torch.uint32) or gate.numel() != 2 or not gate.is_contiguous() or gate.device != self.device:
            raise ValueError(f"monitor {what}: the gate is the uint32[2] device tensor of captured_gate(), on {self.device}")
        return gate.data_ptr()

    def _workspace(self, key, query, *args):
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty((query_bytes(_lib.get(), query, *args),), dtype=torch.uint8, device=self.device)
        return ws

    def observe(self, image, gt, kind, loss_out=None, lambda_dssim=0.2, photometric_on=True, gate=None):
        """One camera of one iteration (train_pan.py:423-429, 471-485). `loss_out` is the third value of
        `photometric_loss(image, gt, lambda_dssim, return_out=True)` for these images: its L1 and SSIM are read on the device
        and SSIM is not evaluated again. Without it the fused loss forward runs first."""
        what = "observe"
        k = _kind(kind)
        _on_device(image, what)
        _on_device(gt, what)
        if image.shape != gt.shape:
            raise ValueError(f"monitor {what}: shapes differ: {tuple(image.shape)} vs {tuple(gt.shape)}")
        if image.ndim < 2 or image.numel() == 0:
            raise ValueError(f"monitor {what}: expected non-empty (..., H, W) images, got {tuple(image.shape)}")
        if image.dtype != torch.float32 or gt.dtype != torch.float32:
            raise TypeError(f"monitor {what}: images are float32, got {image.dtype} and {gt.dtype}")
        if image.device != self.device or gt.device != self.device:
            raise RuntimeError(f"monitor {what}: the images live on {image.device} and {gt.device}, the monitor on {self.device}")
        H, W = int(image.shape[-2]), int(image.shape[-1])
        planes = image.numel() // (H * W)
        x, y = image.detach().contiguous(), gt.detach().contiguous()
        lo = None
        if loss_out is not None:
            _on_device(loss_out, what)
            if loss_out.dtype != torch.float32 or loss_out.numel() != 3 or loss_out.device != self.device:
                raise ValueError(f"monitor {what}: loss_out is the float32[3] of photometric_loss(..., return_out=True) on {self.device}")
            lo = loss_out.detach().contiguous()
        g = self._gate(gate, what)
        ws = self._workspace(("observe", planes, H, W, lo is None), "monitor_observe_bytes", planes, H, W, int(lo is None))
        call("eogs_monitor_observe", self.device, planes, H, W, x.data_ptr(), y.data_ptr(), None if lo is None else lo.data_ptr(),
             float(lambda_dssim), k, int(bool(photometric_on)), g, self.state.data_ptr(), ws.data_ptr(), ws.numel())

    def observe_model(self, opacity_logits, gate=None):
        """Mean opacity and number of rows over the raw `_opacity` [P,1] or [P]; rows that eogs2_amd.optim.retire_rows parked are
        left out (the reference takes both after a physical prune: train_pan.py:331,521,534)."""
        what = "observe_model"
        _on_device(opacity_logits, what)
        o = opacity_logits
        if o.ndim not in (1, 2) or o.numel() == 0 or (o.ndim == 2 and o.shape[1] != 1):
            raise ValueError(f"monitor {what}: the opacity logits are a non-empty (P, 1) or (P,) tensor, got {tuple(o.shape)}")
        if o.dtype != torch.float32:
            raise TypeError(f"monitor {what}: the opacity logits are float32, not {o.dtype}")
        if o.device != self.device:
            raise RuntimeError(f"monitor {what}: the logits live on {o.device}, the monitor on {self.device}")
        o = o.detach().contiguous()
        P = o.shape[0]
        g = self._gate(gate, what)
        ws = self._workspace(("model",), "monitor_model_bytes", 1 << 40)  # (one size from 2^20 rows on: the grid is capped)
        call("eogs_monitor_observe_model", self.device, P, o.data_ptr(), g, self.state.data_ptr(), ws.data_ptr(), ws.numel())

    def end_iteration(self, loss, gate=None):
        """`loss` is the iteration's total loss as a device scalar (train_pan.py:467,492-495)."""
        what = "end_iteration"
        _on_device(loss, what)
        if loss.numel() != 1 or loss.dtype != torch.float32 or loss.device != self.device:
            raise ValueError(f"monitor {what}: the loss is one float32 on {self.device}, got {tuple(loss.shape)} {loss.dtype} on {loss.device}")
        g = self._gate(gate, what)
        lv = loss.detach()
        call("eogs_monitor_end_iteration", self.device, lv.data_ptr(), g, self.state.data_ptr())

    def close_interval(self, gate=None):
        """train_pan.py:512-519, 572-597: means, early stopper, one record, sums cleared. One launch."""
        g = self._gate(gate, "close_interval")
        call("eogs_monitor_close_interval", self.device, self.metric, self.op, self.patience, g, self.state.data_ptr())

    # ---- reading -----------------------------------------------------------------------------------------------------
    def _latest_view(self):
        return self.state[_LATEST_OFFSET:_LATEST_OFFSET + _RECORD_BYTES]

    def fetch(self):
        """The newest record as a dict, by ONE device-to-host copy (it waits for the work queued before it on the current
        stream). None before the first close_interval."""
        host = self._latest_view().cpu()
        return self._decode(host)

    @staticmethod
    def _decode(host):
        r = MonitorRecord.from_buffer_copy(host.numpy().tobytes())
        return _record_dict(r) if r.interval > 0 else None

    def fetch_async(self):
        """Queues the copy of the newest record into pinned memory behind an event on the current stream and returns at
        once; `poll()` hands the record out when it has arrived."""
        buf = torch.empty((_RECORD_BYTES,), dtype=torch.uint8, pin_memory=True)
        buf.copy_(self._latest_view(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._pending.append((ev, buf))

    def poll(self):
        """The newest record whose copy has completed, without waiting (None when none has). A loop that polls learns of
        `early_stop` as many iterations late as the device runs behind the host."""
        while self._pending and self._pending[0][0].query():
            self._polled = self._decode(self._pending.popleft()[1])
        return self._polled

    def snapshot(self):
        """The whole state as a dict (one copy, waits): the open interval's sums and counts, `last` = the four fp32 values of
        the last observation, the stopper, and `ring`: the up to 16 newest records, oldest first. For tests and debugging."""
        raw = self.state.cpu().numpy().tobytes()
        s = MonitorState.from_buffer_copy(raw)
        n = int(s.intervals)
        ring = [_record_dict(s.ring[(k - 1) % MONITOR_RING]) for k in range(max(1, n - MONITOR_RING + 1), n + 1)]
        return {"sums": dict(zip(MONITOR_METRICS, (float(v) for v in s.sums))), "n_photo": int(s.n_photo), "n_pan": int(s.n_pan),
                "n_msi": int(s.n_msi), "ema_loss": float(s.ema_loss), "ema_photometric": float(s.ema_photometric),
                "iteration": int(s.iteration), "best": float(s.best), "counter": int(s.counter), "early_stop": bool(s.early_stop),
                "intervals": n, "last": dict(zip(("l1", "ssim", "photometric", "psnr"), (float(v) for v in s.last))),
                "mean_opacity": float(s.mean_opacity), "rows": int(s.rows), "ring": ring, "bytes": raw}


__all__ = ["TrainingMonitor", "MONITOR_METRICS", "MONITOR_KINDS", "MONITOR_OPERATORS", "HOST_METRICS"]
