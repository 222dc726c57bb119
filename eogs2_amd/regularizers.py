"""The regularisers of the training loss that read the model or a render directly, over the C-ABI of include/eogs_reg.h:
the terms of `inter_loss` (train_pan.py:450-465) that are neither photometric nor a resample consistency pair.

Same names and call signatures as the reference (paths under src/gaussiansplatting/); each class returns the UNWEIGHTED
term, as the reference's does, and `gaussians` is duck-typed: it carries the raw parameters `_opacity` [P,1] and `_scaling`
[P,3] (the activations, sigmoid and exp, happen in the kernel, as on the raw-parameter render path):

  OpacityLoss(w, init_number_of_gaussians)(gaussians)              loss/opacity.py:7-20
  radiiOpacityLoss(w, init_number_of_gaussians)(gaussians, radii)  loss/opacity.py:23-35
  erankLoss(w)(gaussians)                                          loss/main_loss.py:21-37
  Total_variation(w)(altitude_render)                              loss/main_loss.py:40-53
  AccumulatedOpacity(w)(accumulated_opacity_render)                loss/opacity.py:38-45

The functional entry points run several terms in one launch group each way and also return their weighted sum:

  gaussian_regularizers(opacity_logits, log_scales=None, radii=None, *, n_init, weights, want=("opacity",))
  render_regularizers(altitude_render=None, accumulated_opacity_render=None, *, weights)

both -> (total, terms). `weights` are Python floats (copied once into a cached device tensor) or a device tensor that the
kernels read on every run: write into it to switch a term on at `iteration > iterstart_*`, and a recorded GraphedStep keeps
replaying across the switch (the idea of the device gate of eogs2_amd.flow). Rows that eogs2_amd.optim.retire_rows parked
contribute nothing, receive no gradient and are left out of erank's mean; the count is made on the device. fp32 only; CPU
tensors raise (no CPU fallback).
"""
import functools

import torch

from . import _lib
from ._abi import REG_ERANK, REG_OPACITY, REG_OPACITY_RADII
from ._host import call, nbytes, on_device

GAUSSIAN_TERMS = ("opacity", "opacity_radii", "erank")  # the order of terms[] and weights[]
RENDER_TERMS = ("tv_altitude", "accumulated_opacity")
_WANT = dict(zip(GAUSSIAN_TERMS, (REG_OPACITY, REG_OPACITY_RADII, REG_ERANK)))
_on_device = functools.partial(on_device, "regularizers", "the regularisers run")

# The calls sit at the launch floor (the kernels take 10-20 microseconds at a million rows), so the path through this file is
# kept short: `_host.call` (entry points resolved once, raw pointers, the current stream's handle without a Stream object)
# and ONE allocation per forward: the five output floats, then the reduction workspace (one size for every shape).
_OUT_BYTES = 32


def _buffer(dev):
    """(float32 tensor, workspace bytes): out[5] at its start, the workspace from byte _OUT_BYTES on."""
    n = nbytes(_lib.get(), "reg_gauss_bytes", 1)
    return torch.empty(((_OUT_BYTES + n + 3) // 4,), dtype=torch.float32, device=dev), n


def _grad_ptr(g, k):
    """Device pointer of an upstream gradient of k floats (None: NULL = zero)."""
    if g is None:
        return None
    if g.dtype != torch.float32:
        g = g.to(torch.float32)
    if k > 1 and not g.is_contiguous():
        g = g.contiguous()
    return g.data_ptr(), g  # (the tensor rides along so that it outlives the launch call)


_weight_cache = {}


def _weights(weights, names, dev, what):
    """`weights` as a float32 device tensor of len(names): a tensor is used as it is (the kernels read it on every run),
    Python floats — a sequence in the order of `names`, or a dict by name, missing = 0 — are copied to the device once."""
    k = len(names)
    if torch.is_tensor(weights):
        if weights.dtype != torch.float32:
            raise TypeError(f"regularizers {what}: the weight tensor is float32, not {weights.dtype}")
        if weights.numel() != k or weights.ndim != 1:
            raise ValueError(f"regularizers {what}: the weight tensor holds {k} floats {names}, got {tuple(weights.shape)}")
        _on_device(weights, what)
        if weights.device != dev:
            raise RuntimeError(f"regularizers {what}: the weight tensor lives on {weights.device}, the inputs on {dev}")
        return weights.detach() if weights.requires_grad else weights
    if isinstance(weights, dict):
        unknown = set(weights) - set(names)
        if unknown:
            raise ValueError(f"regularizers {what}: unknown weights {sorted(unknown)}; the terms are {names}")
        weights = [weights.get(n, 0.0) for n in names]
    vals = tuple(float(w) for w in weights)
    if len(vals) != k:
        raise ValueError(f"regularizers {what}: {k} weights {names}, got {len(vals)}")
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), vals)
    t = _weight_cache.get(key)
    if t is None:
        t = _weight_cache[key] = torch.tensor(vals, dtype=torch.float32, device=dev)
    return t


def _cont(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


class _GaussianReg(torch.autograd.Function):
    """(total [], terms [3]) = f(opacity [P,1], log_scales [P,3] | None); radii, weights, n_init, want ride along."""

    @staticmethod
    def forward(ctx, opacity, log_scales, radii, weights, n_init, want):
        o, s = _cont(opacity), _cont(log_scales)
        P = o.shape[0]
        buf, ws_bytes = _buffer(o.device)
        p = buf.data_ptr()
        call("eogs_reg_gauss_forward", o.device, P, want, o.data_ptr(), None if s is None else s.data_ptr(),
             None if radii is None else radii.data_ptr(), n_init, weights.data_ptr(), p, p + _OUT_BYTES, ws_bytes)
        ctx.cfg = (P, want, n_init)
        ctx.save_for_backward(o, s, radii, weights, buf)
        ctx.set_materialize_grads(False)
        return buf[3], buf[:3]

    @staticmethod
    def backward(ctx, g_total, g_terms):
        if g_total is None and g_terms is None:
            return (None,) * 6
        P, want, n_init = ctx.cfg
        o, s, radii, weights, buf = ctx.saved_tensors
        gt, gk = _grad_ptr(g_total, 1), _grad_ptr(g_terms, 3)
        g_o = torch.empty_like(o)
        g_s = torch.empty_like(s) if want & REG_ERANK else None
        call("eogs_reg_gauss_backward", o.device, P, want, o.data_ptr(), None if s is None else s.data_ptr(),
             None if radii is None else radii.data_ptr(), n_init, weights.data_ptr(), buf.data_ptr(), gt and gt[0], gk and gk[0],
             g_o.data_ptr(), None if g_s is None else g_s.data_ptr())
        return g_o, g_s, None, None, None, None


def gaussian_regularizers(opacity_logits, log_scales=None, radii=None, *, n_init, weights, want=("opacity",)):
    """(total, terms) of the Gaussian-space regularisers named in `want` (any of "opacity", "opacity_radii", "erank"):

      terms[0] = L_opacity       = sum sigmoid(opacity_logits) / n_init                       loss/opacity.py:14-17
      terms[1] = L_opacity_radii = sum over radii > 0 of sigmoid(opacity_logits) / n_init     loss/opacity.py:30-35
      terms[2] = L_erank         of exp(log_scales)                                           loss/main_loss.py:26-34
      total    = sum of weights[k] * terms[k] over the wanted terms

    `opacity_logits` is the raw `_opacity` [P,1] (or [P]), `log_scales` the raw `_scaling` [P,3], `radii` what the render
    returned (any integer dtype; [P]). `n_init` is the reference's `init_number_of_gaussians`, a constant, not P.
    `weights`: three floats in the order above (or a dict by name) or a float32 device tensor of three, read by the kernels
    on every run. Terms that are not wanted are 0 and receive no gradient. Gradients reach the raw parameters; one forward
    and one backward launch group whatever the number of terms."""
    what = "gaussian_regularizers"
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in _WANT]
    if unknown or not want:
        raise ValueError(f"regularizers {what}: `want` names at least one of {GAUSSIAN_TERMS}, got {want}")
    mask = 0
    for w in want:
        mask |= _WANT[w]
    if not torch.is_tensor(opacity_logits) or opacity_logits.ndim not in (1, 2) or opacity_logits.numel() == 0 or \
            (opacity_logits.ndim == 2 and opacity_logits.shape[1] != 1):
        raise ValueError(f"regularizers {what}: the opacity logits are a non-empty (P, 1) or (P,) tensor, got "
                         f"{tuple(getattr(opacity_logits, 'shape', ()))}")
    if opacity_logits.dtype != torch.float32:
        raise TypeError(f"regularizers {what}: the opacity logits are float32, not {opacity_logits.dtype}")
    P = opacity_logits.shape[0]
    if mask & REG_ERANK:
        if not torch.is_tensor(log_scales) or tuple(log_scales.shape) != (P, 3):
            raise ValueError(f"regularizers {what}: the erank term needs the log-scales as a ({P}, 3) tensor, got "
                             f"{tuple(getattr(log_scales, 'shape', ()))}")
        if log_scales.dtype != torch.float32:
            raise TypeError(f"regularizers {what}: the log-scales are float32, not {log_scales.dtype}")
    else:
        log_scales = None
    if mask & REG_OPACITY_RADII:
        if not torch.is_tensor(radii) or radii.numel() != P or radii.ndim != 1:
            raise ValueError(f"regularizers {what}: the visible-opacity term needs radii as a ({P},) tensor, got "
                             f"{tuple(getattr(radii, 'shape', ()))}")
        if radii.dtype.is_floating_point or radii.dtype.is_complex or radii.dtype == torch.bool:
            raise TypeError(f"regularizers {what}: radii are integers, not {radii.dtype}")
    else:
        radii = None
    if mask & (REG_OPACITY | REG_OPACITY_RADII) and not float(n_init) > 0:
        raise ValueError(f"regularizers {what}: n_init (init_number_of_gaussians) must be positive, got {n_init}")
    _on_device(opacity_logits, what)
    dev = opacity_logits.device
    for t in (log_scales, radii):
        if t is not None:
            _on_device(t, what)
            if t.device != dev:
                raise RuntimeError(f"regularizers {what}: the inputs live on different devices")
    if radii is not None:
        radii = radii.detach().to(torch.int32).contiguous()
    return _GaussianReg.apply(opacity_logits, log_scales, radii, _weights(weights, GAUSSIAN_TERMS, dev, what), float(n_init), mask)


class _RenderReg(torch.autograd.Function):
    """(total [], terms [2]) = f(altitude [H,W] | None, accumulated opacity [H,W] | None)"""

    @staticmethod
    def forward(ctx, alt, acc, weights, H, W):
        a, c = _cont(alt), _cont(acc)
        dev = weights.device
        buf, ws_bytes = _buffer(dev)
        p = buf.data_ptr()
        call("eogs_reg_image_forward", dev, H, W, None if a is None else a.data_ptr(), None if c is None else c.data_ptr(),
             weights.data_ptr(), p, p + _OUT_BYTES, ws_bytes)
        ctx.cfg = (H, W)
        ctx.save_for_backward(a, c, weights)
        ctx.set_materialize_grads(False)
        return buf[2], buf[:2]

    @staticmethod
    def backward(ctx, g_total, g_terms):
        if g_total is None and g_terms is None:
            return (None,) * 5
        H, W = ctx.cfg
        a, c, weights = ctx.saved_tensors
        gt, gk = _grad_ptr(g_total, 1), _grad_ptr(g_terms, 2)
        g_a = torch.empty_like(a) if a is not None else None
        g_c = torch.empty_like(c) if c is not None else None
        call("eogs_reg_image_backward", weights.device, H, W, None if a is None else a.data_ptr(), None if c is None else c.data_ptr(),
             weights.data_ptr(), gt and gt[0], gk and gk[0], None if g_a is None else g_a.data_ptr(),
             None if g_c is None else g_c.data_ptr())
        return g_a, g_c, None, None, None


def _plane(t, name, what):
    if not torch.is_tensor(t) or t.ndim < 2 or t.numel() != t.shape[-1] * t.shape[-2]:
        raise ValueError(f"regularizers {what}: {name} is one (H, W) plane (leading dimensions of size 1 allowed), got "
                         f"{tuple(getattr(t, 'shape', ()))}")
    if t.dtype != torch.float32:
        raise TypeError(f"regularizers {what}: {name} is float32, not {t.dtype}")
    if t.shape[-2] < 2 or t.shape[-1] < 2:
        raise ValueError(f"regularizers {what}: H and W must be at least 2 (the reference takes the mean of an empty tensor there), "
                         f"got {tuple(t.shape[-2:])}")
    return int(t.shape[-2]), int(t.shape[-1])


def render_regularizers(altitude_render=None, accumulated_opacity_render=None, *, weights):
    """(total, terms) of the render-space regularisers over one (H, W) plane each, either may be None:

      terms[0] = L_TV_altitude         = 0.5 (mean |a[1:, :] - a[:-1, :]| + mean |a[:, 1:] - a[:, :-1]|)   loss/main_loss.py:46-50
      terms[1] = L_accumulated_opacity = mean(1 - accumulated_opacity_render)                             loss/opacity.py:44-45
      total    = weights[0] terms[0] + weights[1] terms[1] over the planes given

    One forward and one backward launch group serve both terms when the two planes have the same size; planes of different
    sizes are two calls."""
    what = "render_regularizers"
    if altitude_render is None and accumulated_opacity_render is None:
        raise ValueError(f"regularizers {what}: give the altitude render, the accumulated-opacity render or both")
    sizes = [_plane(t, n, what) for t, n in ((altitude_render, "altitude_render"), (accumulated_opacity_render, "accumulated_opacity_render"))
             if t is not None]
    if len(set(sizes)) != 1:
        raise ValueError(f"regularizers {what}: the two planes have different sizes {sizes}; call once per plane")
    H, W = sizes[0]
    first = altitude_render if altitude_render is not None else accumulated_opacity_render
    for t in (altitude_render, accumulated_opacity_render):
        if t is not None:
            _on_device(t, what)
            if t.device != first.device:
                raise RuntimeError(f"regularizers {what}: the inputs live on different devices")
    return _RenderReg.apply(altitude_render, accumulated_opacity_render, _weights(weights, RENDER_TERMS, first.device, what), H, W)


class _Loss(torch.nn.Module):
    """loss/base_loss.py:5-20"""

    def __init__(self, weight=-1):
        super().__init__()
        self.weight = weight

    def get_loss_name(self):
        return self.__class__.__name__

    def log_loss(self, tb_writer, loss_value, iteration):
        tb_writer.add_scalar(f"loss/{self.get_loss_name()}", loss_value, iteration)


# Each class asks for its one term with weight 1: `total` is then that term, bit for bit, and autograd sees one node.
class OpacityLoss(_Loss):
    def __init__(self, w_L_opacity, init_number_of_gaussians):
        super().__init__()
        self.w_L_opacity = w_L_opacity
        self.init_number_of_gaussians = init_number_of_gaussians

    def forward(self, gaussians):
        return gaussian_regularizers(gaussians._opacity, n_init=self.init_number_of_gaussians, weights=(1.0, 0.0, 0.0),
                                     want=("opacity",))[0]

    def get_loss_name(self):
        return "L_opacity"


class radiiOpacityLoss(_Loss):
    def __init__(self, w_L_opacity, init_number_of_gaussians):
        super().__init__()
        self.w_L_opacity = w_L_opacity
        self.init_number_of_gaussians = init_number_of_gaussians

    def forward(self, gaussians, radii):
        return gaussian_regularizers(gaussians._opacity, radii=radii, n_init=self.init_number_of_gaussians,
                                     weights=(0.0, 1.0, 0.0), want=("opacity_radii",))[0]


class erankLoss(_Loss):
    def __init__(self, w_L_erank):
        super().__init__(weight=w_L_erank)

    def forward(self, gaussians):
        return gaussian_regularizers(gaussians._opacity, gaussians._scaling, n_init=1, weights=(0.0, 0.0, 1.0), want=("erank",))[0]

    def get_loss_name(self):
        return "L_erank"


class Total_variation(_Loss):
    def __init__(self, w_L_TV_altitude):
        super().__init__(weight=w_L_TV_altitude)

    def forward(self, altitude_render):
        return render_regularizers(altitude_render, weights=(1.0, 0.0))[0]

    def get_loss_name(self):
        return "L_TV_altitude"


class AccumulatedOpacity(_Loss):
    def __init__(self, w_L_accumulated_opacity):
        super().__init__()
        self.w_L_accumulated_opacity = w_L_accumulated_opacity

    def forward(self, accumulated_opacity_render):
        return render_regularizers(None, accumulated_opacity_render, weights=(0.0, 1.0))[0]


__all__ = ["gaussian_regularizers", "render_regularizers", "OpacityLoss", "radiiOpacityLoss", "erankLoss", "Total_variation",
           "AccumulatedOpacity", "GAUSSIAN_TERMS", "RENDER_TERMS"]
