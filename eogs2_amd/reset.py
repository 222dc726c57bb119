"""Shadow-based colour reset and in-place opacity reset over the C-ABI of include/eogs_reset.h.

* `shadow_reset_flags(xyz, views, *, opacity=None, out=None)` — the verdict of the reference's `color_reset`
  (src/gaussiansplatting/densification_pruning/color_reset_op.py:42-64): every view's shadow map eroded
  (`1 - max_pool2d(1 - s, 5, 1, 2)`), sampled at every Gaussian's projected position (`grid_sample`, bilinear,
  align_corners, zeros padding), `< 0.5`, ORed over the views. uint8[P] on the device, no host read.
* `color_reset_(optimizer, flags)` — color_reset_op.py:66-88 in ONE launch: the flagged rows of the groups `opacity`, `f_dc`
  and `scaling` get the reference's three values, the same rows of their Adam moments get 0. In place: no Parameter, no
  moment tensor and no address changes, so a recorded `eogs2_amd.graph.GraphedStep` keeps replaying.
* `color_reset(gaussians, cameras, pipe, *, optimizer=None)` — the reference's call: `render_all_views`, then the two above.
* `render_all_views(cameras, gaussians, pipe, bg=None, override_color=None)` — gaussian_renderer/renderer_cc_shadow.py:148-193
  over this library's `render.render` and `resample.render_resample_virtual_camera` and the camera's own `render_pipeline`;
  also what the loop's Nadir evaluation calls (train_pan.py:758).
* `reset_opacity_(optimizer, name="opacity", cap=0.01)` — the in-place twin of `eogs2_amd.optim.reset_opacity`
  (scene/gaussian_model.py:347-352): logit = min(logit, logit(cap)), both moments zero, same tensors.

Deviations, on purpose: a Gaussian whose projection into a view is not finite is not flagged by that view
(torch leaves the sample undefined); rows retired by `eogs2_amd.optim.retire_rows` are never flagged and never capped (the
reference would have pruned them; a reset would revive them); below the cap `reset_opacity_` keeps the stored logit where the
reference's sigmoid -> log round trip perturbs it by rounding (and yields -inf once the sigmoid underflows).

No CPU / eager fallback: arithmetic only in the HIP library.
"""
import ctypes

import torch

from . import _lib
from ._abi import RESET_MAX_TENSORS, RESET_MAX_VIEWS, ResetTensor, ResetView
from ._host import Ctx, ptr
from .optim import RETIRED_LOGIT

C0 = 0.28209479177387814  # utils/sh_utils.py
RETIRED_BELOW = 0.5 * RETIRED_LOGIT  # what eogs2_amd.optim.alive_rows tests
RESET_GROUPS = ("opacity", "f_dc", "scaling")

_values = None
_workspaces = {}  # device -> fp32 workspace holding the eroded maps of one chunk of views
_recorded = []    # workspaces a graph capture has seen: a recording points into them, so they are never dropped


def inverse_sigmoid(x):
    """utils/general_utils.py inverse_sigmoid"""
    return torch.log(x / (1 - x))


def fill_values():
    """The three values of color_reset_op.py:67-75 as Python floats holding fp32 values: computed once, with the reference's
    own ops on a one-element CPU fp32 tensor, so the bits that are stored are the reference's."""
    global _values
    if _values is None:
        one = torch.ones(1, dtype=torch.float32)
        _values = {
            "opacity": float(inverse_sigmoid(0.005 * torch.ones_like(one))),  # inverse_opacity_activation
            "f_dc": float((torch.full_like(one, 1.1) - 0.5) / C0),  # RGB2SH
            "scaling": float(torch.log((1.0 / 400) * torch.ones_like(one))),  # scaling_inverse_activation
        }
    return dict(_values)


def cap_logit(cap=0.01):
    """inverse_sigmoid(min(sigmoid(p), cap)) where the minimum is `cap` (gaussian_model.py:347-350), on a CPU fp32 scalar."""
    return float(inverse_sigmoid(torch.ones(1, dtype=torch.float32) * cap))


def _check_f32(t, what, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be float32, not {t.dtype}")
    if shape is not None and (t.ndim != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape))):
        raise RuntimeError(f"{what} must have shape {tuple('*' if s is None else s for s in shape)}, not {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{what} must be contiguous")


def _same_device(dev, t, what):
    if t.device != dev:
        raise RuntimeError(f"{what} is on {t.device}, expected {dev}: all tensors of a call live on one device")


def _need_gpu(dev, who):
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: tensors on '{dev.type}'; the HIP library works on device memory and there is no CPU fallback")


def _workspace(dev, numel):
    ws = _workspaces.get(dev)
    if ws is None or ws.numel() < numel:
        ws = _workspaces[dev] = torch.empty((numel,), dtype=torch.float32, device=dev)
    if torch.cuda.is_current_stream_capturing() and not any(w is ws for w in _recorded):
        _recorded.append(ws)
    return ws


def shadow_reset_flags(xyz, views, *, opacity=None, out=None):
    """uint8[P]: 1 where some view's eroded shadow map, sampled at the Gaussian's projection, is below 0.5.

    xyz f32[P,3]; views: an iterable of (shadowmap f32[H,W], affine f32[4,4]) device tensors, sizes may differ per view,
    `affine` the torch-layout matrix `AffineCamera.ECEF_to_UVA` reads; opacity: the opacity logits (P elements): rows retired
    by `retire_rows` are never flagged; out: a uint8[P] tensor to write into. Kernel launches alone: it can be recorded."""
    _check_f32(xyz, "xyz", (None, 3))
    dev, P = xyz.device, xyz.shape[0]
    views = list(views)
    for k, view in enumerate(views):
        if not isinstance(view, (tuple, list)) or len(view) != 2 or view[0] is None or view[1] is None:
            raise ValueError(f"view {k}: every view is a (shadowmap, affine) pair, a map for every view")
        _check_f32(view[0], f"view {k}: shadowmap", (None, None))
        _check_f32(view[1], f"view {k}: affine", (4, 4))
        if view[0].numel() == 0 or view[0].numel() >= 1 << 31 or max(view[0].shape) > 1 << 24:
            raise RuntimeError(f"view {k}: shadowmap of {tuple(view[0].shape)}: H, W in 1 .. 2^24 and H W < 2^31")
        _same_device(dev, view[0], f"view {k}: shadowmap")
        _same_device(dev, view[1], f"view {k}: affine")
    if opacity is not None:
        _check_f32(opacity, "opacity")
        if opacity.numel() != P:
            raise RuntimeError(f"opacity has {opacity.numel()} elements for {P} Gaussians")
        _same_device(dev, opacity, "opacity")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.ndim != 1 or out.numel() != P or not out.is_contiguous():
            raise RuntimeError(f"out must be a contiguous uint8 tensor of {P} bytes")
        _same_device(dev, out, "out")
    _need_gpu(dev, "shadow_reset_flags")
    abi = _lib.get()
    with Ctx(abi, dev) as cx, torch.no_grad():
        flags = out if out is not None else torch.empty((P,), dtype=torch.uint8, device=dev)
        if not views:
            flags.zero_()
            return flags
        pad = lambda n: -(-n // 64) * 64  # noqa: E731
        for k0 in range(0, len(views), RESET_MAX_VIEWS):
            chunk = views[k0:k0 + RESET_MAX_VIEWS]
            # (one workspace per device, reused by every chunk and every call: the stream orders its readers and writers)
            ws = _workspace(dev, sum(pad(s.numel()) for s, _ in chunk))
            arr, at = (ResetView * len(chunk))(), 0
            for a, (s, affine) in zip(arr, chunk):
                H, W = s.shape
                eroded = ws[at:at + H * W]
                at += pad(H * W)
                abi.check(abi.reset_erode(H, W, ptr(s), ptr(eroded), cx.stream))
                a.eroded, a.affine, a.H, a.W = eroded.data_ptr(), affine.data_ptr(), H, W
            abi.check(abi.reset_flags(P, ptr(xyz), ptr(opacity), RETIRED_BELOW, len(chunk), ctypes.cast(arr, ctypes.c_void_p),
                                      int(k0 > 0), ptr(flags), cx.stream))
    return flags


def _check_flags(flags, P, dev):
    if not isinstance(flags, torch.Tensor) or flags.dtype not in (torch.uint8, torch.bool) or not flags.is_contiguous():
        raise RuntimeError("flags must be a contiguous uint8 (or bool) tensor")
    if flags.numel() != P:
        raise RuntimeError(f"flags of {flags.numel()} bytes for {P} Gaussians")
    _same_device(dev, flags, "flags")


def _group(optimizer, name):
    for group in optimizer.param_groups:
        if group.get("name") == name:
            if len(group["params"]) != 1:
                raise RuntimeError(f"parameter group {name!r}: one tensor per group, as the reference's model has")
            return group["params"][0]
    raise KeyError(f"the optimizer has no parameter group named {name!r}")


def _moments(optimizer, p, what):
    """(exp_avg, exp_avg_sq) of a parameter, or () while the group has no state yet."""
    st = optimizer.state.get(p, None)
    if not st or "exp_avg" not in st:
        return ()
    out = (st["exp_avg"], st["exp_avg_sq"])
    for m in out:
        _check_f32(m, f"a moment of {what}", tuple(p.shape))
        _same_device(p.device, m, f"a moment of {what}")
    return out


def color_reset_(optimizer, flags):
    """color_reset_op.py:66-88 on the optimizer's groups `opacity`, `f_dc` and `scaling`, in place and in one launch: rows with
    flags[i] != 0 get inverse_sigmoid(0.005), RGB2SH(1.1) and log(1 / 400); the same rows of `exp_avg` and `exp_avg_sq` get 0
    (a group without state yet has none to clear); `step` is untouched, as in the reference. Nothing else changes: not the
    other rows, not a Parameter, a moment tensor or an address."""
    values = fill_values()
    plan, dev, P = [], None, None
    for name in RESET_GROUPS:
        p = _group(optimizer, name)
        _check_f32(p, f"parameter {name!r}")
        if dev is None:
            dev, P = p.device, p.shape[0] if p.ndim else 1
        _same_device(dev, p, f"parameter {name!r}")
        if p.ndim == 0 or p.shape[0] != P:
            raise RuntimeError(f"parameter {name!r} has {tuple(p.shape)} for {P} Gaussians")
        plan.append((p.detach(), values[name]))
        plan += [(m, 0.0) for m in _moments(optimizer, p, name)]
    _check_flags(flags, P, dev)
    _need_gpu(dev, "color_reset_")
    assert len(plan) <= RESET_MAX_TENSORS
    if P == 0:
        return
    abi = _lib.get()
    arr = (ResetTensor * len(plan))()
    for a, (t, value) in zip(arr, plan):
        a.data, a.row_elems, a.value = t.data_ptr(), t.numel() // P, value
    with Ctx(abi, dev) as cx, torch.no_grad():
        abi.check(abi.reset_rows(P, ptr(flags), len(plan), ctypes.cast(arr, ctypes.c_void_p), cx.stream))


def reset_opacity_(optimizer, name="opacity", cap=0.01):
    """`GaussianModel.reset_opacity` (gaussian_model.py:347-352) in place: every logit above logit(cap) becomes logit(cap)
    (the reference's `inverse_sigmoid` of the fp32 `cap`), both Adam moments of the group become 0, and the Parameter, the
    moment tensors and their addresses stay: where `eogs2_amd.optim.reset_opacity` forces a new recording of a GraphedStep,
    this does not. A logit at or below the cap keeps its stored bits (the reference's sigmoid -> log round trip perturbs it
    by rounding and gives -inf once the sigmoid underflows); NaN stays NaN; rows retired by `retire_rows` stay retired."""
    p = _group(optimizer, name)
    _check_f32(p, f"parameter {name!r}")
    moments = _moments(optimizer, p, name)
    _need_gpu(p.device, "reset_opacity_")
    abi = _lib.get()
    m1, m2 = moments if moments else (None, None)
    with Ctx(abi, p.device) as cx, torch.no_grad():
        abi.check(abi.reset_opacity_cap(p.numel(), ptr(p), ptr(m1), ptr(m2), cap_logit(cap), RETIRED_BELOW, cx.stream))


@torch.no_grad()
def render_all_views(cameras, gaussians, pipe, bg=None, override_color=None):
    """gaussian_renderer/renderer_cc_shadow.py:148-193: for every camera the view render, the sun camera's altitude resampled
    onto it, and the camera's own `render_pipeline`; a list of dicts with the reference's keys (image_name, shadow, raw_render,
    cc, render, projxyz, altitude_render). bg[3] is written from `altitude_bounds[0]` without `.item()` (no wait), bg[4] = 0;
    `projxyz` is `xyz @ affine[:3, :2] + affine[3, :2]` (ECEF_to_UVA: the camera's `affine`, not a learned transform)."""
    from .render import render
    from .resample import render_resample_virtual_camera

    if bg is None:
        bg = torch.rand((5,), device=gaussians.get_xyz.device)
    out = []
    for cam in cameras:
        bg[3] = cam.altitude_bounds[0]
        bg[4] = 0.0
        render_pkg = render(cam, gaussians, pipe, bg, override_color=override_color)
        raw_render = render_pkg["render"][:3]
        altitude_render = render_pkg["render"][3]
        rendered_uva = torch.stack(tuple(cam.UV_grid) + (altitude_render,), dim=-1)
        sun_camera, camera_to_sun = cam.get_sun_camera()
        _, sun_altitude_sample, _ = render_resample_virtual_camera(virtual_camera=sun_camera, cam2virt=camera_to_sun,
                                                                   rendered_uva=rendered_uva, gaussians=gaussians, pipe=pipe,
                                                                   background=bg)
        sun_altitude_diff = altitude_render - sun_altitude_sample
        output = cam.render_pipeline(raw_render=raw_render, sun_altitude_diff=sun_altitude_diff)
        xyz = gaussians.get_xyz
        out.append({
            "image_name": getattr(cam, "image_name", None),
            "shadow": output["shadowmap"],
            "raw_render": raw_render,
            "cc": output["cc"],
            "render": output["final"],
            "projxyz": xyz @ cam.affine[:3, :2] + cam.affine[3, :2],
            "altitude_render": altitude_render,
        })
    return out


@torch.no_grad()
def color_reset(gaussians, cameras, pipe, *, optimizer=None):
    """The reference's `color_reset(gaussians, scene, pipe)` (color_reset_op.py:42-88): `cameras` is the list of training
    cameras, or a scene with `getTrainCameras()`. Returns the uint8[P] flags (a device tensor: nothing is read back)."""
    if hasattr(cameras, "getTrainCameras"):
        cameras = cameras.getTrainCameras()
    cameras = list(cameras)
    optimizer = gaussians.optimizer if optimizer is None else optimizer
    outputs = render_all_views(cameras, gaussians, pipe)
    f32 = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()  # noqa: E731  (a camera without a shadow
    views = [(f32(o["shadow"]), f32(cam.affine)) for o, cam in zip(outputs, cameras)]  # map is refused by shadow_reset_flags)
    flags = shadow_reset_flags(gaussians.get_xyz.detach().contiguous(), views, opacity=gaussians._opacity.detach())
    color_reset_(optimizer, flags)
    return flags


__all__ = ["shadow_reset_flags", "color_reset_", "color_reset", "render_all_views", "reset_opacity_", "fill_values", "cap_logit",
           "inverse_sigmoid", "RESET_GROUPS", "RETIRED_BELOW"]
