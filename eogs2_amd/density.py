"""Adaptive density control over the C-ABI of include/eogs_density.h: the reference's training mode `only_prune: False`
(gs_config/train.yaml:39, classic 3DGS densification).

* `DensityStats(P, device)` / `add_densification_stats(...)` — the per-iteration statistics of train_pan.py:679-690 and
  `GaussianModel.add_densification_stats` (gaussian_model.py:719-723) in ONE launch: per row with `radii > 0`,
  `max_radii2D = max(max_radii2D, radii)`, `xyz_gradient_accum += |grad[:2]|`, `denom += 1`; every other row keeps its bits.
  No `nonzero`, no host wait, fixed addresses: the call can sit inside a `GraphedStep` function after `backward()`. Rows
  parked by `optim.retire_rows` have radius 0 and stay untouched.
* `densify_and_prune(optimizer, stats, ...)` — `GaussianModel.densify_and_prune` as a whole (gaussian_model.py:685-717:
  `densify_and_clone` :625-660, `densify_and_split` :573-623, `densification_postfix` :541-571, `prune_points` :488-505),
  decided from the P original rows in one pass, ONE host wait (four counts), the `torch.normal` draw of the reference, and
  one build pass that writes every parameter, both Adam moments and every `extra` tensor at its final size.

No CPU / eager fallback: arithmetic only in the HIP library.
"""
import ctypes
import functools

import torch

from . import _lib
from . import optim as _optim
from ._abi import (DENSITY_CLONE, DENSITY_COPY, DENSITY_MAX_N, DENSITY_PRUNE_SAMP, DENSITY_PRUNE_SELF, DENSITY_SCALING,
                   DENSITY_SPLIT, DENSITY_XYZ, DENSITY_ZERO, DensityTensor)
from ._host import Ctx, call, on_device, query_bytes

STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
# the bit layout of DensifyInfo.flags, one byte per ORIGINAL row (include/eogs_density.h EOGS_DENSITY_*)
FLAG_CLONE, FLAG_SPLIT, FLAG_PRUNE_SELF, FLAG_PRUNE_SAMPLES = DENSITY_CLONE, DENSITY_SPLIT, DENSITY_PRUNE_SELF, DENSITY_PRUNE_SAMP


_on_device = functools.partial(on_device, "density", "density control runs")


def _check_stats(accum, denom, maxr, what):
    """The three statistics in the reference's shapes ([P,1], [P,1], [P]: float32, contiguous, one device); returns P."""
    for n, t in zip(STATS, (accum, denom, maxr)):
        if not torch.is_tensor(t):
            raise TypeError(f"density {what}: {n} is a tensor, not {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"density {what}: {n} is float32, not {t.dtype}")
    P = maxr.shape[0] if maxr.ndim == 1 else -1
    if P < 0 or tuple(accum.shape) != (P, 1) or tuple(denom.shape) != (P, 1):
        raise ValueError(f"density {what}: xyz_gradient_accum [P,1], denom [P,1], max_radii2D [P]; got {tuple(accum.shape)}, "
                         f"{tuple(denom.shape)}, {tuple(maxr.shape)}")
    for t in (accum, denom, maxr):
        if not t.is_contiguous():
            raise ValueError(f"density {what}: the statistics are updated in place and must be contiguous")
    return P


def _check_devices(tensors, what):
    """Every tensor on one GPU (checked after types and shapes, so that a wrong call is named for what is wrong with it)."""
    for t in tensors:
        _on_device(t, what)
        if t.device != tensors[0].device:
            raise RuntimeError(f"density {what}: tensors on {t.device} and on {tensors[0].device}")
    return tensors[0].device


def add_densification_stats(xyz_gradient_accum, denom, max_radii2D, viewspace_grad, radii):
    """train_pan.py:683-690 on the caller's own tensors, in place, one launch and no wait: per row with `radii > 0`
    `max_radii2D = max(max_radii2D, float(radii))`, `xyz_gradient_accum += sqrt(gx^2 + gy^2)`, `denom += 1`.
    `viewspace_grad` is the float32 [P, 3] gradient of the screen-space points (its third column is not read); `radii` is
    int32 (what the rasterizer returns) or float32, [P]. About 40 bytes of traffic per row."""
    what = "add_densification_stats"
    P = _check_stats(xyz_gradient_accum, denom, max_radii2D, what)
    if viewspace_grad is None:
        raise ValueError(f"density {what}: viewspace_grad is None (the screen-space points received no gradient: call after "
                         "backward(), with settings that ask for radii)")
    if not torch.is_tensor(viewspace_grad) or not torch.is_tensor(radii):
        raise TypeError(f"density {what}: viewspace_grad and radii are tensors")
    if viewspace_grad.dtype != torch.float32:
        raise TypeError(f"density {what}: viewspace_grad is float32, not {viewspace_grad.dtype}")
    if radii.dtype not in (torch.int32, torch.float32):
        raise TypeError(f"density {what}: radii are int32 or float32, not {radii.dtype}")
    if tuple(viewspace_grad.shape) != (P, 3) or tuple(radii.shape) != (P,):
        raise ValueError(f"density {what}: viewspace_grad [{P}, 3] and radii [{P}] for {P} rows of statistics; got "
                         f"{tuple(viewspace_grad.shape)} and {tuple(radii.shape)}")
    dev = _check_devices((max_radii2D, xyz_gradient_accum, denom, viewspace_grad, radii), what)
    if P == 0:
        return
    vg = viewspace_grad.detach()
    vg = vg if vg.is_contiguous() else vg.contiguous()
    r = radii if radii.is_contiguous() else radii.contiguous()
    call("eogs_density_stats_update", dev, P, vg.data_ptr(), r.data_ptr(), int(r.dtype == torch.float32),
         xyz_gradient_accum.data_ptr(), denom.data_ptr(), max_radii2D.data_ptr())


class DensityStats:
    """The three statistics of `GaussianModel` in the reference's shapes: `xyz_gradient_accum` [P,1], `denom` [P,1],
    `max_radii2D` [P], float32 zeros. The tensors are plain attributes (and `stats[name]`), so
    `parallel.all_reduce_densification_stats(stats.xyz_gradient_accum, stats.denom, stats.max_radii2D)` takes them as is."""

    def __init__(self, P, device):
        device = torch.device(device)
        self.xyz_gradient_accum = torch.zeros((P, 1), dtype=torch.float32, device=device)
        self.denom = torch.zeros((P, 1), dtype=torch.float32, device=device)
        self.max_radii2D = torch.zeros((P,), dtype=torch.float32, device=device)

    @classmethod
    def of(cls, stats):
        """A DensityStats over the given tensors (a DensityStats, a mapping by name, or the three tensors in order)."""
        if isinstance(stats, cls):
            return stats
        self = cls.__new__(cls)
        vals = [stats[k] for k in STATS] if hasattr(stats, "keys") else list(stats)
        if len(vals) != 3:
            raise ValueError("density: statistics are (xyz_gradient_accum, denom, max_radii2D)")
        self.xyz_gradient_accum, self.denom, self.max_radii2D = vals
        return self

    def update(self, viewspace_grad, radii):
        add_densification_stats(self.xyz_gradient_accum, self.denom, self.max_radii2D, viewspace_grad, radii)

    def tensors(self):
        return self.xyz_gradient_accum, self.denom, self.max_radii2D

    def keys(self):
        return STATS

    def __getitem__(self, name):
        if name not in STATS:
            raise KeyError(name)
        return getattr(self, name)

    def __len__(self):
        return int(self.max_radii2D.shape[0])


class DensifyInfo:
    """What `densify_and_prune` decided. `flags` is a uint8 device tensor, one byte per ORIGINAL row:

        bit 0 FLAG_CLONE          the row is in the reference's clone mask
        bit 1 FLAG_SPLIT          the row is in the reference's split mask (never together with bit 0)
        bit 2 FLAG_PRUNE_SELF     the final prune removes the row and, if it was cloned, its clone
        bit 3 FLAG_PRUNE_SAMPLES  the final prune removes the N samples of the row (meaningful with bit 1)

    `n_kept` rows with neither bit 1 nor bit 2, `n_kept_clones` rows with bit 0 and not bit 2, `n_split` rows with bit 1,
    `n_kept_split` rows with bit 1 and not bit 3: the result holds n_kept + n_kept_clones + N n_kept_split rows. The three
    mask methods rebuild the reference's masks with PyTorch ops (they wait for the device; diagnostics, not the hot path)."""

    def __init__(self, flags, counts, N):
        self.flags, self.N = flags, N
        self.n_kept, self.n_kept_clones, self.n_split, self.n_kept_split = (int(c) for c in counts)
        self.n_out = self.n_kept + self.n_kept_clones + N * self.n_kept_split

    def clone_mask(self):
        """[P]: `selected_pts_mask` of densify_and_clone."""
        return (self.flags & FLAG_CLONE) != 0

    def split_mask(self):
        """[P + number of clones]: `selected_pts_mask` of densify_and_split (the appended clones are never selected)."""
        n_clone = int(self.clone_mask().sum())
        return torch.cat(((self.flags & FLAG_SPLIT) != 0, torch.zeros(n_clone, dtype=torch.bool, device=self.flags.device)))

    def prune_mask(self):
        """[P - n_split + number of clones + N n_split]: `prune_mask` of densify_and_prune over the rows after the split."""
        f = self.flags
        split, pself, psamp = (f & FLAG_SPLIT) != 0, (f & FLAG_PRUNE_SELF) != 0, (f & FLAG_PRUNE_SAMPLES) != 0
        return torch.cat((pself[~split], pself[self.clone_mask()], psamp[split].repeat(self.N)))


def _row_bytes(t, what):
    width = 1
    for d in t.shape[1:]:
        width *= int(d)
    if t.element_size() != 4 or width * 4 > 256:
        raise RuntimeError(f"density densify_and_prune: {what}: 4-byte element types and rows of at most 64 elements")
    return width * 4


def densify_and_prune(optimizer, stats, grad_threshold, min_opacity=0.005, screen_size_threshold=None, max_screen_size=None,
                      scene_extent=None, percent_dense=0.01, N=2, radii=None, extra=()):
    """`GaussianModel.densify_and_prune(grad_threshold, min_opacity, screen_size_threshold, max_screen_size, radii,
    scene_extent)` (gaussian_model.py:685-717) on the optimizer's six groups, computed from the P original rows.

    Per original row: g = xyz_gradient_accum / denom (NaN -> 0), smax = max exp(scaling);
    clone = g >= grad_threshold and smax <= percent_dense * scene_extent; split = g >= grad_threshold and smax > that (the
    clones the reference appends before the split carry a padded gradient of 0 and are never split);
    low = sigmoid(opacity) < min_opacity; with a truthy `max_screen_size`, big_self = smax > 0.1 * screen_size_threshold and,
    for the samples of a split row, big_samp = max exp(log(exp(s) / (0.8 N))) > 0.1 * screen_size_threshold. A row and its
    clone are pruned when low or big_self, its samples when low or big_samp. The thresholds are formed in double, as Python
    forms them, and rounded once to fp32.

    The reference's third term of the final prune, `max_radii2D > max_screen_size`, reads a statistic that
    `densification_postfix` has just zeroed: it can never be true. That is reproduced, not repaired: `max_screen_size` only
    switches the two world-space terms on.

    Result rows, the reference's order after its four stages: [rows neither split nor pruned], [clones of the clone rows not
    pruned], N x [samples of the split rows whose samples are not pruned] copy-major. Survivors keep parameters and both
    moments, new rows copy their origin's parameters and get zero moments, `step` is unchanged; a sample's position is
    R(q/|q|) . sample + xyz, its log-scale log(exp(s) / (0.8 N)). The samples are drawn with
    `torch.normal(mean=zeros, std=exp(scaling[split]).repeat(N, 1))` for ALL split-selected rows before the final prune —
    the call `optim.densify_and_split` makes, so the same generator state gives the stepwise path's samples. `extra`
    per-row tensors (4-byte elements) ride along, new rows copy their origin's. `radii` is accepted for signature parity and
    not used (the reference concatenates `tmp_radii` and discards it).

    The optimizer's groups and state are re-keyed as by the stepwise functions of `optim`. One host wait: the four counts.
    Rows retired by `optim.retire_rows` are never selected and the final prune removes them (min_opacity > 0): a compaction
    beforehand is not needed on this path. P = 0 and "everything pruned" return zero-row tensors. `only_densify`
    (gaussian_model.py:661-683) is not built: in the reference it cannot run.

    Returns ({group name: new nn.Parameter}, DensityStats of zeros at the new size, DensifyInfo) — and the tensors of
    `extra` at the new size as `info.extra`."""
    what = "densify_and_prune"
    if scene_extent is None:
        raise ValueError(f"density {what}: scene_extent is needed (percent_dense * scene_extent separates clone from split)")
    if max_screen_size and screen_size_threshold is None:
        raise ValueError(f"density {what}: max_screen_size needs screen_size_threshold")
    N, extra = int(N), list(extra)
    if not 1 <= N <= DENSITY_MAX_N:
        raise ValueError(f"density {what}: N in 1..{DENSITY_MAX_N}")
    st = DensityStats.of(stats)
    P = _check_stats(st.xyz_gradient_accum, st.denom, st.max_radii2D, what)
    plan = _optim._groups(optimizer)
    by_name = {g["name"]: p for g, p, _ in plan}
    for n in ("xyz", "opacity", "scaling", "rotation"):
        if n not in by_name:
            raise KeyError(f"density {what}: no parameter group named {n!r}")
    for n, width in (("xyz", 3), ("opacity", 1), ("scaling", 3), ("rotation", 4)):
        if by_name[n].shape[0] != P or by_name[n].numel() != P * width:
            raise ValueError(f"density {what}: group {n!r} is [{P}, {width}] for {P} rows of statistics, got {tuple(by_name[n].shape)}")
    dev = _check_devices(st.tensors(), what)
    # (source tensor, kind) of everything that moves; the contiguous copies live until the launches are queued
    items = []
    for group, p, state in plan:
        kind = {"xyz": DENSITY_XYZ, "scaling": DENSITY_SCALING}.get(group["name"], DENSITY_COPY)
        items.append((p.data, kind, group["name"]))
        if state is not None:
            items.append((state["exp_avg"], DENSITY_ZERO, group["name"] + " exp_avg"))
            items.append((state["exp_avg_sq"], DENSITY_ZERO, group["name"] + " exp_avg_sq"))
    items += [(e, DENSITY_COPY, f"extra[{k}]") for k, e in enumerate(extra)]
    srcs = []
    for t, kind, name in items:
        _on_device(t, what)
        if t.device != dev or t.shape[0] != P:
            raise RuntimeError(f"density {what}: {name} needs {P} rows on {dev}")
        if kind != DENSITY_COPY and t.dtype != torch.float32:
            raise TypeError(f"density {what}: {name} is float32, not {t.dtype}")
        srcs.append(t.detach().contiguous())
    rbs = [_row_bytes(t, name) for t, (_, _, name) in zip(srcs, items)]

    opacity, scaling, rot = (by_name[n].detach().contiguous() for n in ("opacity", "scaling", "rotation"))
    abi = _lib.get()
    thr_dense = percent_dense * scene_extent  # doubles, as Python forms them; ctypes rounds each once to fp32
    thr_big = 0.1 * screen_size_threshold if max_screen_size else 0.0
    split_div = 0.8 * N
    with Ctx(abi, dev) as cx, torch.no_grad():
        ws = torch.empty((query_bytes(abi, "density_bytes", P),), dtype=torch.uint8, device=dev)
        flags = torch.empty((P,), dtype=torch.uint8, device=dev)
        counts = (ctypes.c_int64 * 4)()
        ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
        abi.check(abi.density_decide(P, ptr(st.xyz_gradient_accum), ptr(st.denom), ptr(opacity), ptr(scaling),
                                     float(grad_threshold), thr_dense, float(min_opacity), int(bool(max_screen_size)), thr_big, split_div,
                                     ptr(flags), ws.data_ptr(), ws.numel(), counts, cx.stream))
        info = DensifyInfo(flags, counts, N)
        # the draw of densify_and_split, for ALL split-selected rows and also when there are none (the reference calls
        # torch.normal with empty tensors then): one call per densify_and_prune, whatever was selected
        sel = torch.empty((info.n_split, 3), dtype=torch.float32, device=dev)
        if info.n_split:
            abi.check(abi.density_split_rows(P, ptr(flags), scaling.data_ptr(), sel.data_ptr(), 12, ws.data_ptr(),
                                             ws.numel(), cx.stream))
        stds = torch.exp(sel).repeat(N, 1)
        means = torch.zeros((stds.size(0), 3), device=dev)
        samples = torch.normal(mean=means, std=stds)
        if samples.dtype != torch.float32 or tuple(samples.shape) != (N * info.n_split, 3) or samples.device != dev:
            raise RuntimeError(f"density {what}: torch.normal returned {samples.dtype} {tuple(samples.shape)} on {samples.device}")
        samples = samples.contiguous()
        outs = [torch.empty((info.n_out,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in srcs]
        if P and outs:
            arr = (DensityTensor * len(outs))()
            for a, s, o, rb, (_, kind, _) in zip(arr, srcs, outs, rbs, items):
                a.src, a.dst, a.row_bytes, a.kind = ptr(s), ptr(o), rb, kind
            abi.check(abi.density_build(P, N, ptr(flags), counts, len(outs), ctypes.cast(arr, ctypes.c_void_p),
                                        rot.data_ptr(), ptr(samples),
                                        split_div, ws.data_ptr(), ws.numel(), cx.stream))
    n_extra = len(extra)
    params = _optim._install(optimizer, plan, outs[:len(outs) - n_extra])
    info.extra = outs[len(outs) - n_extra:]
    return params, DensityStats(info.n_out, dev), info


__all__ = ["DensityStats", "add_densification_stats", "densify_and_prune", "DensifyInfo", "FLAG_CLONE", "FLAG_SPLIT", "FLAG_PRUNE_SELF",
           "FLAG_PRUNE_SAMPLES"]
