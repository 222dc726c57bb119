"""DSM evaluation on the GPU over the eogs_tsdf_dsm_* entries of include/eogs_tsdf.h: the reference's NCC registration,
shift and masked MAE (src/gaussiansplatting/eval/dsmr.py, eval/eval_dsm.py:35-69, 334-341), the last stage of the chain
render -> fuse -> DSM -> score. Names follow the reference so that a user can swap imports:

  downsample2x(u)                                   dsmr.py:15-43   (the last-writer rule, float64 out, bit-exact)
  ncc_search(ref, sec, irange, dx, dy)              dsmr.py:146-163 (compute_ncc at one level, all shifts in one pass)
  compute_shift(dsm_ref, dsm_sec, scaling)          dsmr.py:165-179, 198-225 -> (dx, dy, a, b)
  apply_shift(in_dsm, dx, dy, a, b, c, d)           dsmr.py:182-192, 258-271
  mask_dsm(dsm, water_mask, vis_mask, tree_mask)    eval_dsm.py:35-53
  dsm_pointwise_diff(pred_dsm, gt_dsm, clip)        eval_dsm.py:56-69 -> (diff, pred_rdsm)
  dsm_mae(pred_dsm, gt_dsm, clip)                   Mae_Computer.compute_mae_from_pred_dsm, eval_dsm.py:334-341, 378-387

Images are float32 or float64 [H][W] tensors on the GPU; CPU tensors raise (no CPU fallback). `dsm_ref` is the ground
truth, `dsm_sec` the DSM to register: it may be larger than the reference, not smaller in either dimension (ValueError;
the reference reads out of bounds). All arithmetic is float64, as numba types the reference's accumulators.

`compute_shift` is one stream-ordered chain (both pyramids, then one search per level whose centre is read on the device
from the result of the level below) with ONE read-back at its end; `compute_shift_device` enqueues the same chain without
the read-back and can be captured in a `torch.cuda.graph` (call it once on the capture stream first, so that the capture
allocates nothing). Workspaces are allocated per (device, stream, call shape) on first use and kept for the life of the
process — about 35 MB for a 2048 x 2048 pair —; `clear_workspaces()` drops them (not while a captured graph that uses them
is alive). A stream handle the runtime hands out again after its stream was destroyed finds the old stream's buffers.

`clip="reference"` reproduces the reference's clip bounds, numpy's `gt.min() - 10`, `gt.max() + 10`: ONE NaN in the ground
truth makes both NaN, `np.clip` then returns NaN everywhere and the MAE raises ValueError — what the reference does to a
masked ground truth. `clip="finite"` takes the bounds from the ground truth's non-NaN pixels (an explicit deviation).
"""
import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._host import Ctx, Workspaces, nbytes, on_device, ptr

MAX_IRANGE = 8  # include/eogs_tsdf.h EOGS_TSDF_DSM_MAX_IRANGE
RESULT_DTYPE = np.dtype([("dx", "<i4"), ("dy", "<i4"), ("valid", "<i4"), ("reserved", "<i4"), ("count", "<f8"), ("muu", "<f8"),
                         ("muv", "<f8"), ("sigu", "<f8"), ("sigv", "<f8"), ("xcorr", "<f8"), ("ncc", "<f8")])  # eogs_tsdf_dsm_result
_ws_cache = Workspaces()
_on_device = functools.partial(on_device, "dsm_eval", "the DSM evaluation runs")


def _image(t, what):
    if not torch.is_tensor(t) or t.ndim != 2 or t.numel() == 0:
        raise TypeError(f"dsm_eval {what}: images are non-empty [H][W] tensors")
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"dsm_eval {what}: images are float32 or float64, not {t.dtype}")
    return t.detach().contiguous()


def _pair(ref, sec, irange, what):
    ref, sec = _image(ref, what), _image(sec, what)
    if not 0 <= int(irange) <= MAX_IRANGE:
        raise ValueError(f"dsm_eval {what}: irange must be 0 .. {MAX_IRANGE}")
    if sec.shape[0] < ref.shape[0] or sec.shape[1] < ref.shape[1]:
        raise ValueError(f"dsm_eval {what}: the DSM to register {tuple(sec.shape)} is smaller than the reference DSM "
                         f"{tuple(ref.shape)}")
    _on_device(ref, what)
    _on_device(sec, what)
    if ref.device != sec.device:
        raise RuntimeError(f"dsm_eval {what}: the two images live on different devices")
    if ref.dtype != sec.dtype:  # an exact conversion: every value is read as float64 anyway
        ref, sec = ref.double(), sec.double()
    return ref, sec


def clear_workspaces():
    """Drops every cached workspace (a caller that scores DSMs of many sizes, or on short-lived streams). Buffers returned
    by compute_shift_device stay valid as long as the caller holds them; a captured graph holds none of them."""
    _ws_cache.clear()


def read_results(results):
    """The eogs_tsdf_dsm_result records of a device buffer as a numpy structured array (one read-back)."""
    return results.cpu().numpy().view(RESULT_DTYPE)


def downsample2x(u):
    """dsmr.py:15-43: float64 [ceil(H/2)][ceil(W/2)], the mean over the finite pixels of the block whose top-left corner is
    (min(2J+1, H-1), min(2I+1, W-1)) (the reference's last writer), NaN where none is finite."""
    u = _image(u, "downsample2x")
    _on_device(u, "downsample2x")
    abi = _lib.get()
    H, W = u.shape
    out = torch.empty(((H + 1) // 2, (W + 1) // 2), dtype=torch.float64, device=u.device)
    with Ctx(abi, u.device) as cx:
        abi.check(abi.tsdf_dsm_downsample(H, W, ptr(u), int(u.dtype == torch.float64), ptr(out), cx.stream))
    return out


def ncc_search(ref, sec, irange=5, dx=0, dy=0):
    """compute_ncc (dsmr.py:146-163) around the centre (dx, dy): (best dx, best dy, table) with table[y][x] the NCC of
    the shift (dx - irange + x, dy - irange + y), a float64 [2 irange + 1][2 irange + 1] tensor on the device. ValueError if
    no candidate has a finite NCC (no overlap holds a finite pair: outside the reference's domain)."""
    ref, sec = _pair(ref, sec, irange, "ncc_search")
    abi = _lib.get()
    dev = ref.device
    (Hu, Wu), (Hv, Wv), n = ref.shape, sec.shape, 2 * int(irange) + 1

    def make():
        return (Workspaces.bytes(dev, nbytes(abi, "tsdf_dsm_ncc_bytes", Hu, Wu, int(irange))),
                Workspaces.bytes(dev, RESULT_DTYPE.itemsize))

    ws, res = _ws_cache.of(("ncc", Hu, Wu, int(irange)), dev, make)
    table = torch.empty((n, n), dtype=torch.float64, device=dev)
    centre = torch.tensor([int(dx), int(dy)], dtype=torch.int32, device=dev)
    with Ctx(abi, dev) as cx:
        abi.check(abi.tsdf_dsm_ncc(Hu, Wu, ptr(ref), Hv, Wv, ptr(sec), int(ref.dtype == torch.float64), int(irange),
                                   ptr(centre), 1, ptr(table), ptr(res), ptr(ws), ws.numel(), cx.stream))
    r = read_results(res)[0]
    if not r["valid"]:
        raise ValueError("dsm_eval ncc_search: no candidate shift has a finite NCC")
    return int(r["dx"]), int(r["dy"]), table


def compute_shift_device(dsm_ref, dsm_sec, irange=5):
    """The device work of compute_shift, enqueued on the current stream without waiting for it: (results, tables) with
    `results` the eogs_tsdf_dsm_result records of every pyramid level as bytes ([0] = full resolution; read_results()
    decodes them) and `tables` float64 [levels][2 irange + 1][2 irange + 1]. Both belong to the reused workspace of this
    call shape: the next call of the same shape on the same stream overwrites them."""
    ref, sec = _pair(dsm_ref, dsm_sec, irange, "compute_shift")
    abi = _lib.get()
    dev = ref.device
    (Hu, Wu), (Hv, Wv), n = ref.shape, sec.shape, 2 * int(irange) + 1

    def make():
        nb, lv = ctypes.c_size_t(), ctypes.c_int()  # (a size and a level count: not a plain size query)
        abi.check(abi.tsdf_dsm_shift_bytes(Hu, Wu, Hv, Wv, int(irange), ctypes.byref(nb), ctypes.byref(lv)))
        return (Workspaces.bytes(dev, nb.value), Workspaces.bytes(dev, lv.value * RESULT_DTYPE.itemsize),
                torch.empty((lv.value, n, n), dtype=torch.float64, device=dev))

    ws, results, tables = _ws_cache.of(("shift", Hu, Wu, Hv, Wv, int(irange)), dev, make)
    with Ctx(abi, dev) as cx:
        abi.check(abi.tsdf_dsm_shift(Hu, Wu, ptr(ref), Hv, Wv, ptr(sec), int(ref.dtype == torch.float64), int(irange),
                                     ptr(tables), ptr(results), ptr(ws), ws.numel(), cx.stream))
    return results, tables


def compute_shift(dsm_ref, dsm_sec, scaling=True):
    """dsmr.py:198-225: (dx, dy, a, b) registering `dsm_sec` on `dsm_ref`; a = sigu / sigv, or the integer 1 without
    `scaling`; b = muu - muv a. One read-back. ValueError if some level has no candidate with a finite NCC."""
    results, _ = compute_shift_device(dsm_ref, dsm_sec)
    r = read_results(results)
    if not r["valid"].all():
        raise ValueError("dsm_eval compute_shift: no candidate shift has a finite NCC at some pyramid level")
    r = r[0]
    a = float(r["sigu"]) / float(r["sigv"]) if scaling else 1
    b = float(r["muu"]) - float(r["muv"]) * a
    return int(r["dx"]), int(r["dy"]), a, b


def apply_shift(in_dsm, dx=0, dy=0, a=1, b=0, c=0, d=0):
    """dsmr.py:258-271: out[j][i] = a valnan(in_dsm, i + dx, j + dy) + b + c i + d j in float64, stored in in_dsm's dtype."""
    v = _image(in_dsm, "apply_shift")
    _on_device(v, "apply_shift")
    abi = _lib.get()
    H, W = v.shape
    out = torch.empty_like(v)
    with Ctx(abi, v.device) as cx:
        abi.check(abi.tsdf_dsm_apply_shift(H, W, ptr(v), int(v.dtype == torch.float64), int(dx), int(dy), float(a), float(b),
                                           float(c), float(d), ptr(out), cx.stream))
    return out


def mask_dsm(dsm, water_mask, vis_mask, tree_mask):
    """eval_dsm.py:35-53, in place like the reference: water mask cropped to the DSM's shape -> NaN, visibility mask ->
    NaN, DSM cropped to the tree mask's shape if they differ and NaN where the tree mask is FALSE. Masks are bool tensors
    (or None). Returns the (possibly cropped view of the) DSM. Not a hot path: torch indexing."""
    _image(dsm, "mask_dsm")
    _on_device(dsm, "mask_dsm")
    nan = float("nan")
    if water_mask is not None:
        dsm.masked_fill_(water_mask[: dsm.shape[0], : dsm.shape[1]].to(dsm.device, torch.bool), nan)
    if vis_mask is not None:
        dsm.masked_fill_(vis_mask.to(dsm.device, torch.bool), nan)
    if tree_mask is not None:
        if dsm.shape != tree_mask.shape:
            dsm = dsm[: tree_mask.shape[0], : tree_mask.shape[1]]
        dsm.masked_fill_(~tree_mask.to(dsm.device, torch.bool), nan)
    return dsm


def _pointwise(pred_dsm, gt_dsm, clip):
    if clip not in ("reference", "finite"):
        raise ValueError('dsm_eval: clip is "reference" or "finite"')
    gt, pred = _pair(gt_dsm, pred_dsm, 5, "dsm_pointwise_diff")
    abi = _lib.get()
    dev = gt.device
    transform = compute_shift(gt, pred, scaling=False)
    pred_r = apply_shift(pred, *transform)
    (Hp, Wp), (Hg, Wg) = pred_r.shape, gt.shape
    h, w = min(Hp, Hg), min(Wp, Wg)

    (ws,) = _ws_cache.of(("mae",), dev, lambda: (Workspaces.bytes(dev, nbytes(abi, "tsdf_dsm_mae_bytes")),))
    diff = torch.empty((h, w), dtype=pred_r.dtype, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    with Ctx(abi, dev) as cx:
        abi.check(abi.tsdf_dsm_mae(Hp, Wp, ptr(pred_r), Hg, Wg, ptr(gt), int(gt.dtype == torch.float64), int(clip == "finite"),
                                   ptr(diff), ptr(out), ptr(ws), ws.numel(), cx.stream))
    return diff, pred_r, transform, out


def dsm_pointwise_diff(pred_dsm, gt_dsm, clip="reference"):
    """eval_dsm.py:56-69: compute_shift(gt, pred, scaling=False), apply_shift, clip to the ground truth's range widened by
    10, diff = pred_rdsm[:h, :w] - gt[:h, :w]. Returns (diff, pred_rdsm). Images of different types are both taken as
    float64. See the module docstring for `clip`."""
    diff, pred_r, _, _ = _pointwise(pred_dsm, gt_dsm, clip)
    return diff, pred_r


def dsm_mae(pred_dsm, gt_dsm, clip="reference"):
    """(mae, diff, pred_rdsm, (dx, dy, a, b)): mae = nanmean(|diff|) summed in float64 in a fixed order; ValueError when it
    is NaN (every pixel of diff is NaN), as eval_dsm.py:334-341 raises."""
    diff, pred_r, transform, out = _pointwise(pred_dsm, gt_dsm, clip)
    total, count = out[:2].tolist()
    mae = total / count if count > 0 else float("nan")
    if mae != mae:
        raise ValueError("The computed MAE is NaN, this means that the diff array contains only NaN values (a NaN in the ground "
                         'truth makes the reference\'s clip bounds NaN: see clip="finite")')
    return mae, diff, pred_r, transform


__all__ = ["MAX_IRANGE", "RESULT_DTYPE", "apply_shift", "clear_workspaces", "compute_shift", "compute_shift_device", "downsample2x", "dsm_mae",
           "dsm_pointwise_diff", "mask_dsm", "ncc_search", "read_results"]
