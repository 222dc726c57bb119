"""The end of a training run and the inference side over the C-ABI of include/eogs_report.h: what the reference does with a
trained model around the render chain this package already has.

* `normalize_before_saving(scene, gaussians)` / `normalize_colors_(f_dc, ref_weight, ref_bias, cc_weights, cc_biases)` —
  utils/save_utils.py:10-33, the global colour alignment before the final `save_ply` (train_pan.py:614-620): every Gaussian's
  colour through the reference camera's correction in one in-place pass, every MSI camera's correction recomposed against it
  in one launch of one wave, in double, without `torch.linalg.inv` and without a host wait. IN PLACE: `_features_dc` stays the
  same Parameter at the same address with its optimizer state (the reference rebinds the attribute to a plain tensor), and
  the cameras' `weight` / `bias` keep their storage.
* `load_convert_color_correction_train_to_test(name)` — utils/convert_color_correction.py: "ref" and "average", written into
  the test cameras' existing parameters by one launch per camera list (the reference makes new `nn.Parameter`s).
* `ReportAccumulator`, `evaluate_views(viewpoints, gaussians, pipe, opt, background)` — the L1 / PSNR loop of
  `training_report` (train_pan.py:876-951) with no host wait per camera: float64 sums per camera kind in a device table,
  one copy at the end.
* `pack_products`, `video_frame`, `view_products`, `fetch_products` — `render_set`'s products of one camera
  (render_pan.py:94-476) as device tensors under its directory names, all of them into file layout by one launch per 16
  and ONE copy into page-locked memory; render_video.py:138-164's frame `[final | normalised elevation]` in one launch.
  Writing .iio, GeoTIFF and .avi files stays the caller's.

PyTorch is plumbing; there is no CPU or eager fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._abi import (REPORT_CC_AVERAGE, REPORT_CC_REF, REPORT_FLOAT_HWC, REPORT_KINDS, REPORT_MAX_CAMERAS, REPORT_MAX_CC_ELEMS,
                   REPORT_MAX_CHANNELS, REPORT_MAX_ITEMS, REPORT_PACK_MAX_CHANNELS, REPORT_PREMAP, REPORT_REPLICATE, REPORT_REVERSE,
                   REPORT_U8_ROUND, REPORT_U8_TRUNC, ReportCamera, ReportItem, ReportTable)
from ._host import Ctx, nbytes, ptr

MODES = {"float": REPORT_FLOAT_HWC, "u8_round": REPORT_U8_ROUND, "u8_trunc": REPORT_U8_TRUNC}
KINDS = REPORT_KINDS
PRODUCT_KEYS = ("rawrender", "altitude", "accumulated_opacity", "sunpovsampled", "nadirpov", "nadirpovsampled", "nadiraltitudesampled",
                "nadir_altitude_diff", "gt")  # plus the keys of render_pipeline, and "dsm" when asked for


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _check(what, name, t, shape=None, numel=None, dtype=torch.float32):
    """A contiguous `dtype` tensor of the given shape (or element count); the device is checked by `_one_device`."""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{what}: {name} must be {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{what}: {name} must hold {numel} elements, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous (it is read or written by address)")


def _one_device(what, named):
    """All tensors on one device; which one. (The `check_*` functions stop here, so that they can be asked on any device;
    their callers go on to `_need_gpu`.)"""
    named = [(n, t) for n, t in named if t is not None]
    dev = named[0][1].device
    for n, t in named:
        if t.device != dev:
            raise RuntimeError(f"{what}: {n} on {t.device}, {named[0][0]} on {dev}")
    return dev


def _need_gpu(what, dev):
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: tensors on '{dev}': this runs on the GPU, there is no CPU fallback")
    return dev


def _span(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _no_overlap(what, outs, ins):
    """No written tensor shares bytes with a read one or with another written one."""
    outs = [(n, t) for n, t in outs if t is not None and t.numel()]
    ins = [(n, t) for n, t in ins if t is not None and t.numel()]
    for i, (no, o) in enumerate(outs):
        o0, o1 = _span(o)
        for nb, b in ins + outs[:i]:
            b0, b1 = _span(b)
            if o0 < b1 and b0 < o1:
                raise ValueError(f"{what}: {no} overlaps {nb}")


def _check_gate(gate, dev, who):
    if gate is None:
        return
    if not (torch.is_tensor(gate) and gate.numel() == 2 and gate.is_contiguous() and gate.dtype in (torch.uint32, torch.int32)):
        raise ValueError(f"{who}: gate must be a contiguous uint32[2] tensor (eogs2_amd.rasterizer.captured_gate())")
    if gate.device != dev:
        raise RuntimeError(f"{who}: gate on {gate.device}, the table on {dev}")


def _camera_table(pairs):
    arr = (ReportCamera * max(1, len(pairs)))()
    for a, (w, b) in zip(arr, pairs):
        a.weight, a.bias = w.data_ptr(), b.data_ptr()
    return arr


# ---- 1. colour alignment ---------------------------------------------------------------------------------------------------
def check_normalize(f_dc, ref_weight, ref_bias, cc_weights, cc_biases):
    """Everything `normalize_colors_` refuses before its launches; returns (device, rows)."""
    what = "normalize_colors_"
    _check(what, "f_dc", f_dc)
    if not ((f_dc.ndim == 3 and tuple(f_dc.shape[1:]) == (1, 3)) or (f_dc.ndim == 2 and f_dc.shape[1] == 3)):
        raise ValueError(f"{what}: f_dc must be (P, 1, 3) or (P, 3), got {tuple(f_dc.shape)}")
    _check(what, "ref_weight", ref_weight, numel=9)
    _check(what, "ref_bias", ref_bias, numel=3)
    cc_weights, cc_biases = list(cc_weights), list(cc_biases)
    if len(cc_weights) != len(cc_biases):
        raise ValueError(f"{what}: {len(cc_weights)} weights for {len(cc_biases)} biases")
    if len(cc_weights) > REPORT_MAX_CAMERAS:
        raise ValueError(f"{what}: {len(cc_weights)} cameras, at most {REPORT_MAX_CAMERAS} in one call")
    for i, (w, b) in enumerate(zip(cc_weights, cc_biases)):
        _check(what, f"cc_weights[{i}]", w, numel=9)
        _check(what, f"cc_biases[{i}]", b, numel=3)
    named = [("f_dc", f_dc), ("ref_weight", ref_weight), ("ref_bias", ref_bias)]
    named += [(f"cc_weights[{i}]", w) for i, w in enumerate(cc_weights)] + [(f"cc_biases[{i}]", b) for i, b in enumerate(cc_biases)]
    dev = _one_device(what, named)
    # the reference camera's own tensors are expected among the cameras'; any other sharing of bytes is refused
    same = lambda a, b: a.data_ptr() == b.data_ptr()  # noqa: E731
    outs = [("f_dc", f_dc)] + [(n, t) for n, t in named[3:]]
    ins = [(n, t) for n, t in named[1:3] if not any(same(t, o) and t.numel() == o.numel() for _, o in named[3:])]
    _no_overlap(what, outs, ins)
    return dev, f_dc.shape[0]


def normalize_colors_(f_dc, ref_weight, ref_bias, cc_weights, cc_biases):
    """In place: f_dc <- RGB2SH(A1 . SH2RGB(f_dc) + b1) per row in fp32, then for every camera i Ai <- Ai . A1^-1 and
    bi <- bi - Ai . A1^-1 . b1 in double, rounded once (A1, b1: `ref_weight`, `ref_bias`, normally one of the cameras' own
    tensors: every camera, that one included, is recomposed against their ORIGINAL values). Two launches, no wait; a singular
    A1 gives NaN corrections where the reference's torch.linalg.inv raises. Returns f_dc."""
    dev, P = check_normalize(f_dc, ref_weight, ref_bias, cc_weights, cc_biases)
    _need_gpu("normalize_colors_", dev)
    abi = _lib.get()
    pairs = [(w.detach(), b.detach()) for w, b in zip(cc_weights, cc_biases)]
    arr = _camera_table(pairs)
    with Ctx(abi, dev) as cx, torch.no_grad():
        abi.check(abi.report_normalize_rows(P, ptr(f_dc.detach()), ptr(ref_weight.detach()), ptr(ref_bias.detach()), cx.stream))
        abi.check(abi.report_recompose(len(pairs), ctypes.cast(arr, ctypes.c_void_p), ptr(ref_weight.detach()), ptr(ref_bias.detach()),
                                       cx.stream))
    return f_dc


def normalize_before_saving(scene, gaussians):
    """utils/save_utils.py:10-33 with the reference's arguments: the reference camera is the train camera with
    `is_reference_camera`; its MSI camera's colour correction becomes the identity, every Gaussian's colour and every other
    MSI camera's correction are mapped so that renders stay the same. In place (see `normalize_colors_`)."""
    view = None
    for c in scene.getTrainCameras():
        if c.is_reference_camera:
            view = c.get_msi_cameras()
            break
    assert view is not None
    cams = [c.get_msi_cameras() for c in scene.getTrainCameras()]
    normalize_colors_(gaussians._features_dc, view.color_correction.weight, view.color_correction.bias,
                      [c.color_correction.weight for c in cams], [c.color_correction.bias for c in cams])


# ---- 2. train -> test colour correction --------------------------------------------------------------------------------------
def get_list_cam(viewpoint_cam, opt):
    """utils/camera_utils.py:22-31: the MSI camera, then the PAN camera, as far as `opt` loads them."""
    list_cam = []
    if opt.load_msi:
        list_cam.append(viewpoint_cam.get_msi_cameras())
    if opt.load_pan:
        list_cam.append(viewpoint_cam.get_pan_cameras())
    return list_cam


def check_cc_to_test(train, test):
    """Everything a converter refuses before its launch, over [(weight, bias)] lists; returns (device, w_elems, b_elems)."""
    what = "cc_to_test"
    if not train:
        raise ValueError(f"{what}: no train camera")
    if len(train) > REPORT_MAX_CAMERAS or len(test) > REPORT_MAX_CAMERAS:
        raise ValueError(f"{what}: at most {REPORT_MAX_CAMERAS} cameras of a kind in one call")
    w0, b0 = train[0]
    named = []
    for side, cams in (("train", train), ("test", test)):
        for i, (w, b) in enumerate(cams):
            _check(what, f"{side}[{i}].weight", w, shape=w0.shape if torch.is_tensor(w0) else None)
            _check(what, f"{side}[{i}].bias", b, shape=b0.shape if torch.is_tensor(b0) else None)
            named += [(f"{side}[{i}].weight", w), (f"{side}[{i}].bias", b)]
    if w0.numel() < 1 or b0.numel() < 1 or w0.numel() + b0.numel() > REPORT_MAX_CC_ELEMS:
        raise ValueError(f"{what}: a correction of {w0.numel()} + {b0.numel()} elements, at most {REPORT_MAX_CC_ELEMS} together")
    dev = _one_device(what, named)
    _no_overlap(what, named[2 * len(train):], named[:2 * len(train)])
    return dev, w0.numel(), b0.numel()


def _cc_to_test(mode, train, test):
    train = [(c.color_correction.weight, c.color_correction.bias) for c in train]
    test = [(c.color_correction.weight, c.color_correction.bias) for c in test]
    dev, nw, nb = check_cc_to_test(train, test)
    _need_gpu("cc_to_test", dev)
    if not test:
        return
    abi = _lib.get()
    a = _camera_table([(w.detach(), b.detach()) for w, b in train])
    b = _camera_table([(w.detach(), b.detach()) for w, b in test])
    with Ctx(abi, dev) as cx, torch.no_grad():
        abi.check(abi.report_cc_to_test(mode, len(train), ctypes.cast(a, ctypes.c_void_p), len(test), ctypes.cast(b, ctypes.c_void_p), nw, nb,
                                        cx.stream))


class base_cc_train_to_test:
    def __init__(self):
        pass

    def get_train_test_camlist(self, train_viewpoints, test_cameras, opt):
        n = len(get_list_cam(train_viewpoints[0], opt))
        list_train_cameras, list_test_cameras = [[] for _ in range(n)], [[] for _ in range(n)]
        for vp in train_viewpoints:
            for k, cam in enumerate(get_list_cam(vp, opt)):
                list_train_cameras[k].append(cam)
        for vp in test_cameras:
            for k, cam in enumerate(get_list_cam(vp, opt)):
                list_test_cameras[k].append(cam)
        return list_train_cameras, list_test_cameras

    def perform_cc_to_test(self, train_viewpoints, test_cameras, opt):
        list_train_cameras, list_test_cameras = self.get_train_test_camlist(train_viewpoints, test_cameras, opt)
        for k in range(len(list_train_cameras)):
            self.correct_test_cameras(list_train_cameras[k], list_test_cameras[k])
        return test_cameras

    def correct_test_cameras(self, train_cameras, test_cameras):
        raise NotImplementedError


class perform_cc_by_ref_test(base_cc_train_to_test):
    """The reference camera's weight and bias into every test camera, bit for bit (the last train camera with
    `is_reference_camera`, as the reference's loop leaves it)."""

    def correct_test_cameras(self, train_cameras, test_cameras):
        view = None
        for train_cam in train_cameras:
            if train_cam.is_reference_camera:
                view = train_cam
        if view is None:
            raise ValueError("No reference camera found in train cameras")
        _cc_to_test(REPORT_CC_REF, [view], list(test_cameras))


class perform_average_cc_test(base_cc_train_to_test):
    """The train cameras' corrections summed in camera order from zero and divided by their count, in fp32 as the
    reference's `+=` and `/=`: the same bits."""

    def correct_test_cameras(self, train_cameras, test_cameras):
        _cc_to_test(REPORT_CC_AVERAGE, list(train_cameras), list(test_cameras))
        return test_cameras


def load_convert_color_correction_train_to_test(name="None"):
    if name == "ref":
        return perform_cc_by_ref_test()
    if name == "average":
        return perform_average_cc_test()
    if name == "closesttime":
        raise NotImplementedError("Because JAX doesn't have timestamp yet ")
    raise NotImplementedError(f"color correction {name} not implemented")


# ---- 3. report metrics ------------------------------------------------------------------------------------------------------
def kind_index(kind):
    if kind not in KINDS:
        raise ValueError(f"ReportAccumulator: kind must be one of {KINDS}, got {kind!r}")
    return KINDS.index(kind)


def check_accumulate(image, gt, kind):
    """Everything `ReportAccumulator.accumulate` refuses that does not involve its own table; returns (k, C, H, W)."""
    what = "ReportAccumulator.accumulate"
    k = kind_index(kind)
    _check(what, "image", image)
    _check(what, "gt", gt)
    if image.ndim != 3 or not 1 <= image.shape[0] <= REPORT_MAX_CHANNELS or image.numel() == 0:
        raise ValueError(f"{what}: image must be (C, H, W) with 1 <= C <= {REPORT_MAX_CHANNELS}, got {tuple(image.shape)}")
    if tuple(gt.shape) != tuple(image.shape):
        raise ValueError(f"{what}: gt must be {tuple(image.shape)} like image, got {tuple(gt.shape)}")
    return (k,) + tuple(image.shape)


class ReportAccumulator:
    """training_report's `l1_test` / `psnr_test` (train_pan.py:878-946) as a device table: per kind ("pan", "msi") a float64
    sum of the per-view L1, a float64 sum of the per-view mean PSNR and a count.

    accumulate(image, gt, kind, gate=None)  one launch group, no wait: `l1_loss(image, clamp(gt, 0, 1)).mean().double()` and
                                            `psnr(image, clamp(gt, 0, 1)).mean().double()` added to `kind`'s sums
    fetch(n_viewpoints)                     the one copy: {"l1": {"pan", "msi"}, "psnr": {"pan", "msi"}}, the sums divided by
                                            the number of VIEWPOINTS (not of cameras of the kind), as the reference divides
    reset()                                 a launch

    The per-view figures are formed in double over the fp32 inputs and rounded to fp32 once (the reference sums in fp32);
    every sum has a fixed order: the same bits on every run."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"ReportAccumulator: device '{device}': this runs on the GPU, there is no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        abi = _lib.get()
        assert ctypes.sizeof(ReportTable) == 64
        self.table = torch.zeros((8,), dtype=torch.float64, device=device)  # eogs_report_table
        self._ws = torch.empty((nbytes(abi, "report_metrics_bytes"),), dtype=torch.uint8, device=device)

    def reset(self):
        abi = _lib.get()
        with Ctx(abi, self.device) as cx:
            abi.check(abi.report_metrics_reset(ptr(self.table), cx.stream))

    def accumulate(self, image, gt, kind, gate=None):
        k, C, H, W = check_accumulate(image, gt, kind)
        what = "ReportAccumulator.accumulate"
        _need_gpu(what, _one_device(what, [("the table", self.table), ("image", image), ("gt", gt)]))
        _check_gate(gate, self.device, what)
        _no_overlap(what, [("the table", self.table), ("the workspace", self._ws)], [("image", image), ("gt", gt)])
        abi = _lib.get()
        with Ctx(abi, self.device) as cx:
            abi.check(abi.report_metrics_accumulate(C, H, W, ptr(image.detach()), ptr(gt.detach()), k, ptr(self.table), ptr(gate),
                                                    ptr(self._ws), self._ws.numel(), cx.stream))

    def read(self):
        """The table as it stands (one copy, one wait): {"l1": [pan, msi], "psnr": [...], "views": [...], "last": (L1, PSNR)}."""
        t = ReportTable.from_buffer_copy(self.table.cpu().numpy().tobytes())
        return {"l1": list(t.l1), "psnr": list(t.psnr), "views": list(t.views), "last": (t.last_l1, t.last_psnr)}

    def fetch(self, n_viewpoints):
        if int(n_viewpoints) < 1:
            raise ValueError("ReportAccumulator.fetch: the number of viewpoints must be positive")
        t = self.read()
        return {m: {kind: t[m][i] / int(n_viewpoints) for i, kind in enumerate(KINDS)} for m in ("l1", "psnr")}


def _render_chain(cam, gaussians, pipe, bg):
    """train_pan.py:891-914: render, sun camera resampled onto the view, the camera's render pipeline."""
    from .render import render
    from .resample import render_resample_virtual_camera

    render_pkg = render(cam, gaussians, pipe, bg)["render"]
    raw_render, altitude_render = render_pkg[:3], render_pkg[3]
    rendered_uva = torch.stack(tuple(cam.UV_grid) + (altitude_render,), dim=-1)
    sun_camera, cam2sun = cam.get_sun_camera()
    sun_rgb_sample, sun_altitude_sample, _, sunpov = render_resample_virtual_camera(
        virtual_camera=sun_camera, cam2virt=cam2sun, rendered_uva=rendered_uva, gaussians=gaussians, pipe=pipe, background=bg,
        return_extra=True)
    sun_altitude_diff = altitude_render - sun_altitude_sample
    renderings = cam.render_pipeline(raw_render=raw_render, sun_altitude_diff=sun_altitude_diff)
    return render_pkg, rendered_uva, sun_rgb_sample, sun_altitude_diff, renderings


@torch.no_grad()
def evaluate_views(viewpoints, gaussians, pipe, opt, background, accumulator=None):
    """One validation config of training_report (train_pan.py:876-951): for every camera of every viewpoint in `get_list_cam`
    order (MSI, then PAN, as `opt.load_msi` / `opt.load_pan` say) the background (`torch.rand(5)` on the device under
    `opt.random_background`, else `background`, written in place as the reference writes it; bg[3] from `altitude_bounds[0]`
    without `.item()`, bg[4] = 0), render, sun resample, `render_pipeline`, and `renderings["shaded"]` against
    `cam.original_image` into the accumulator's `cam.image_type`. No host wait in the loop; returns `fetch(len(viewpoints))`.
    `accumulator=None` makes one; a given one is NOT reset here."""
    viewpoints = list(viewpoints)
    if not viewpoints:
        raise ValueError("evaluate_views: no viewpoints")
    dev = gaussians.get_xyz.device
    acc = ReportAccumulator(dev) if accumulator is None else accumulator
    for viewpoint in viewpoints:
        for cam in get_list_cam(viewpoint, opt):
            bg = torch.rand((5,), device=dev) if opt.random_background else background
            bg[3] = cam.altitude_bounds[0]
            bg[4] = 0.0
            renderings = _render_chain(cam, gaussians, pipe, bg)[4]
            gt = cam.original_image.to(device=dev, dtype=torch.float32).contiguous()
            acc.accumulate(renderings["shaded"].contiguous(), gt, cam.image_type)
    return acc.fetch(len(viewpoints))


# ---- 4. product packing -------------------------------------------------------------------------------------------------------
class PackItem:
    """One image of `pack_products`: src f32 (C, H, W) or (H, W); mode "float" | "u8_round" | "u8_trunc"; offset / pitch in
    bytes (None: chosen by `pack_products`); reverse: channels last to first; replicate: a one-channel source three times;
    premap=(lo, hi): x <- (x - lo) / (hi - lo) first, with lo and the double difference hi - lo each rounded to fp32."""

    __slots__ = ("src", "mode", "offset", "pitch", "reverse", "replicate", "premap")

    def __init__(self, src, mode="float", offset=None, pitch=None, reverse=False, replicate=False, premap=None):
        self.src, self.mode, self.offset, self.pitch = src, mode, offset, pitch
        self.reverse, self.replicate, self.premap = bool(reverse), bool(replicate), premap

    def geometry(self):
        """(C, H, W, channels written, element size)"""
        s = self.src.shape
        C, H, W = (1, s[0], s[1]) if len(s) == 2 else s
        return C, H, W, (3 if self.replicate else C), (4 if self.mode == "float" else 1)


def check_pack(items, out=None):
    """Everything `pack_products` refuses before its launch. Fills in the offsets and pitches left None (the items one after
    another, each at a multiple of 16 bytes); returns (items, bytes needed)."""
    what = "pack_products"
    items = [it if isinstance(it, PackItem) else PackItem(**it) for it in items]
    if not items:
        raise ValueError(f"{what}: no items")
    if len(items) > REPORT_MAX_ITEMS:
        raise ValueError(f"{what}: {len(items)} items, at most {REPORT_MAX_ITEMS} in one call")
    end = 0
    for i, it in enumerate(items):
        if it.mode not in MODES:
            raise ValueError(f"{what}: item {i}: mode must be one of {tuple(MODES)}, got {it.mode!r}")
        _check(what, f"item {i}", it.src)
        if it.src.ndim not in (2, 3) or it.src.numel() == 0:
            raise ValueError(f"{what}: item {i} must be (C, H, W) or (H, W), got {tuple(it.src.shape)}")
        C, H, W, Co, eb = it.geometry()
        if not 1 <= C <= REPORT_PACK_MAX_CHANNELS:
            raise ValueError(f"{what}: item {i} has {C} channels, at most {REPORT_PACK_MAX_CHANNELS}")
        if it.replicate and C != 1:
            raise ValueError(f"{what}: item {i}: replicate takes a one-channel source, got {C} channels")
        if it.premap is not None:
            lo, hi = (float(v) for v in it.premap)
            it.premap = (lo, hi)
        row = W * Co * eb
        if it.pitch is None:
            it.pitch = row
        if it.offset is None:
            it.offset = -(-end // 16) * 16
        it.offset, it.pitch = int(it.offset), int(it.pitch)
        if it.offset < 0 or it.pitch < row:
            raise ValueError(f"{what}: item {i}: offset {it.offset} is negative or pitch {it.pitch} shorter than a row of {row} bytes")
        if eb == 4 and (it.offset % 4 or it.pitch % 4):
            raise ValueError(f"{what}: item {i}: a float item's offset and pitch must be multiples of 4")
        end = max(end, it.offset + (H - 1) * it.pitch + row)
    named = [(f"item {i}", it.src) for i, it in enumerate(items)]
    if out is not None:
        _check(what, "out", out, dtype=torch.uint8)
        if out.numel() < end:
            raise ValueError(f"{what}: out holds {out.numel()} bytes, the items reach byte {end}")
        named.append(("out", out))
    _one_device(what, named)
    if out is not None:
        _no_overlap(what, [("out", out)], named[:-1])
    return items, end


def pack_products(items, out=None):
    """Up to 16 images into one uint8 buffer in ONE launch (eogs_report_pack). `items`: `PackItem`s or dicts of their
    arguments. Returns (out, [(offset, pitch, (H, W, channels), numpy dtype)] per item). `out=None` allocates the buffer
    (bytes between the items are then left as they come); a given `out` keeps every byte outside the items' rectangles.
    In both 8-bit modes a NaN gives 0 (numpy's cast of a NaN is undefined)."""
    items, need = check_pack(items, out)
    dev = _need_gpu("pack_products", items[0].src.device)
    if out is None:
        out = torch.empty((need,), dtype=torch.uint8, device=dev)
    arr = (ReportItem * len(items))()
    layout = []
    for a, it in zip(arr, items):
        C, H, W, Co, eb = it.geometry()
        a.src, a.C, a.H, a.W, a.mode = it.src.data_ptr(), C, H, W, MODES[it.mode]
        a.dst_offset, a.dst_pitch = it.offset, it.pitch
        a.flags = (REPORT_REVERSE if it.reverse else 0) | (REPORT_REPLICATE if it.replicate else 0) | (REPORT_PREMAP if it.premap else 0)
        a.lo, a.d = (np.float32(it.premap[0]), np.float32(it.premap[1] - it.premap[0])) if it.premap else (0.0, 1.0)
        layout.append((it.offset, it.pitch, (H, W, Co), np.float32 if eb == 4 else np.uint8))
    abi = _lib.get()
    with Ctx(abi, dev) as cx:
        abi.check(abi.report_pack(len(items), ctypes.cast(arr, ctypes.c_void_p), ptr(out), out.numel(), cx.stream))
    return out, layout


def video_frame(final, altitude, altitude_min, altitude_max, out=None):
    """render_video.py:138-164's frame as a device tensor uint8 (H, 2 W, 3): `[final | (altitude - min) / (max - min)]`,
    clipped to [0, 1], x 255, truncated, BGR; a one-plane (PAN) `final` is repeated. One launch, two items side by side."""
    what = "video_frame"
    _check(what, "final", final)
    _check(what, "altitude", altitude)
    if final.ndim != 3 or final.shape[0] not in (1, 3):
        raise ValueError(f"{what}: final must be (3, H, W) or (1, H, W), got {tuple(final.shape)}")
    H, W = final.shape[1:]
    altitude = altitude.reshape(H, W) if altitude.numel() == H * W else altitude
    if tuple(altitude.shape) != (H, W):
        raise ValueError(f"{what}: altitude must be ({H}, {W}), got {tuple(altitude.shape)}")
    if out is None:
        out = torch.empty((H, 2 * W, 3), dtype=torch.uint8, device=final.device)
    elif not torch.is_tensor(out) or tuple(out.shape) != (H, 2 * W, 3):
        raise ValueError(f"{what}: out must be uint8 ({H}, {2 * W}, 3)")
    pan = final.shape[0] == 1
    pack_products([PackItem(final, "u8_trunc", offset=0, pitch=6 * W, reverse=not pan, replicate=pan),
                   PackItem(altitude, "u8_trunc", offset=3 * W, pitch=6 * W, replicate=True, premap=(altitude_min, altitude_max))],
                  out=out.view(-1) if torch.is_tensor(out) and out.is_contiguous() else out)
    return out


@torch.no_grad()
def view_products(cam, gaussians, pipe, background, gt=None, dsm=None, random_camera=False):
    """The products `render_set` writes for one camera (render_pan.py:189-411) as device tensors under its directory names:
    rawrender, altitude, accumulated_opacity, sunpovsampled, nadirpov, nadirpovsampled, nadiraltitudesampled,
    nadir_altitude_diff, the keys of `cam.render_pipeline`, gt (`gt`, or `cam.original_image[0:3]`), and with
    `dsm=dict(scene_params=..., resolution=..., [radius, geometry])` the view's DSM through `dsm_raster.dsm_from_view` under
    "dsm" (its profile under "dsm_profile"). The random camera the reference renders there and saves nothing from is left
    out; the flow-matched variants need the caller's network."""
    from .resample import render_resample_virtual_camera

    if random_camera:
        raise NotImplementedError("view_products: the reference saves nothing from its random camera; render it with "
                                  "eogs2_amd.resample.render_resample_virtual_camera if you want it")
    render_pkg, rendered_uva, sun_rgb_sample, sun_altitude_diff, renderings = _render_chain(cam, gaussians, pipe, background)
    altitude_render = render_pkg[3]
    nadir_camera, cam2nadir = cam.get_nadir_camera()
    nadir_rgb_sample, nadir_altitude_sample, _, nadirpov = render_resample_virtual_camera(
        virtual_camera=nadir_camera, cam2virt=cam2nadir, rendered_uva=rendered_uva, gaussians=gaussians, pipe=pipe,
        background=background, return_extra=True)
    out = {"rawrender": render_pkg[:3], "altitude": altitude_render, "accumulated_opacity": render_pkg[4],
           "sunpovsampled": sun_rgb_sample, "nadirpov": nadirpov[:3], "nadirpovsampled": nadir_rgb_sample,
           "nadiraltitudesampled": nadir_altitude_sample, "nadir_altitude_diff": altitude_render - nadir_altitude_sample}
    out.update({k: v for k, v in renderings.items() if v is not None})
    out["gt"] = cam.original_image[0:3] if gt is None else gt
    if dsm is not None:
        from .dsm_raster import dsm_from_view

        kw = {k: dsm[k] for k in ("radius", "geometry") if k in dsm}
        out["dsm_profile"], out["dsm"] = dsm_from_view(altitude_render, cam if hasattr(cam, "Ainv") else cam.affine, dsm["scene_params"], dsm["resolution"],
                                                       uv_axes=dsm.get("uv_axes"), **kw)
    return out


def fetch_products(products):
    """{name: numpy array in file layout} for a dict of device tensors ((C, H, W) -> (H, W, C) as
    `permute(1, 2, 0).cpu().numpy()` gives it; (H, W) and the already pixel-major (H, W, 1) "dsm" as they are): everything is
    packed into one device buffer (one launch per 16 tensors), copied ONCE into page-locked memory, and the arrays are views
    of that. Entries that are not tensors (a DSM's profile) are passed through."""
    names, items, shapes, passed = [], [], [], {}
    for name, t in products.items():
        if not torch.is_tensor(t):
            passed[name] = t
            continue
        t = t.detach()
        if t.dtype != torch.float32:
            raise ValueError(f"fetch_products: {name} must be float32, got {t.dtype}")
        t = t.contiguous()
        if t.ndim == 3 and t.shape[-1] == 1 and name == "dsm":
            src, shape = t.reshape(t.shape[0], t.shape[1]), tuple(t.shape)
        elif t.ndim == 3:
            src, shape = t, (t.shape[1], t.shape[2], t.shape[0])
        elif t.ndim == 2:
            src, shape = t, tuple(t.shape)
        else:
            raise ValueError(f"fetch_products: {name} must be (C, H, W) or (H, W), got {tuple(t.shape)}")
        names.append(name)
        items.append(PackItem(src, "float"))
        shapes.append(shape)
    if not items:
        return passed
    # one buffer for all calls: the offsets of a later chunk continue where the earlier one ended
    end = 0
    for it in items:
        C, H, W, Co, eb = it.geometry()
        it.offset, it.pitch = -(-end // 16) * 16, W * Co * eb
        end = it.offset + H * it.pitch
    dev = items[0].src.device
    buf = torch.empty((end,), dtype=torch.uint8, device=dev)
    for i0 in range(0, len(items), REPORT_MAX_ITEMS):
        pack_products(items[i0:i0 + REPORT_MAX_ITEMS], out=buf)
    host = torch.empty((end,), dtype=torch.uint8, pin_memory=True)
    host.copy_(buf, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    flat = host.numpy()
    out = dict(passed)
    for name, it, shape in zip(names, items, shapes):
        n = int(np.prod(shape)) * 4
        out[name] = flat[it.offset:it.offset + n].view(np.float32).reshape(shape)
    return out


__all__ = ["normalize_before_saving", "normalize_colors_", "check_normalize", "load_convert_color_correction_train_to_test",
           "base_cc_train_to_test", "perform_cc_by_ref_test", "perform_average_cc_test", "check_cc_to_test", "get_list_cam",
           "ReportAccumulator", "check_accumulate", "kind_index", "evaluate_views", "PackItem", "check_pack", "pack_products",
           "video_frame", "view_products", "fetch_products", "MODES", "KINDS", "PRODUCT_KEYS"]
