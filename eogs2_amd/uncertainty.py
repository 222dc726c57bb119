"""The transient-uncertainty term of the training loss over the C-ABI of include/eogs_nll.h: the Gaussian negative
log-likelihood of the shaded image under a per-pixel variance formed from the camera's trainable transient mask
(train_pan.py:433-449, `transient_params.use_transient`, scene/cameras/affine_cameras.py:280-292):

    betaprime = (cam.transient_mask.clip(0, 1) + 1e-3).square()
    L_nll = torch.nn.functional.gaussian_nll_loss(input=image, target=gt_image, var=betaprime.unsqueeze(0).repeat(C, 1, 1))

  transient_nll(image, gt_image, transient_mask, *, weight=None, floor=1e-3, eps=1e-6) -> (total, loss, stats)
  gaussian_nll_loss(input, target, var, full=False, eps=1e-6, reduction="mean")            torch's signature
  TransientNLL(w_L_nll)(image, gt_image, transient_mask)                                   the unweighted term, as a loss class
  transient_parameters(H, W, init_value, device)                                           affine_cameras.py:282-289

One forward launch group and one backward launch; the variance is never stored, nothing waits for the device: the
reference's `torch.any(var < 0)` is a count the forward leaves in `out[4]`, the mask's mean and standard deviation
(train_pan.py:441-448, two `.item()` waits there) arrive in `out[2:4]` of the same launch. `weight` is a Python float (copied
once into a cached device tensor) or a device f32[1] tensor that the kernels read on every run: write into it at
`iteration > iterstart_L_nll` and a recorded GraphedStep keeps replaying across the switch; weight 0 gives exactly 0 for
`total` and for every gradient through it, also at a NaN pixel. fp32 only; CPU tensors raise (no CPU fallback).

Deviations from torch, stated: a negative variance does not raise (that needs a wait) — it is counted in `out[4]` and its
element is clamped like any other variance below `eps`, l = 0.5 (log eps + (x - t)^2 / eps); `reduction="none"`, gradients
to the target and batched (B, C, H, W) inputs are not provided.
"""
import functools

import torch

from . import _lib
from ._abi import NLL_FULL, NLL_MASK, NLL_SUM
from ._host import call, nbytes, on_device

_on_device = functools.partial(on_device, "uncertainty", "the NLL term runs")
STATS = ("mean", "std", "negative", "clipped")  # the order of `stats` = out[2:6]

# ONE allocation per forward: the six output floats, then the reduction workspace (one size for every shape)
_OUT_BYTES = 32


def _buffer(dev):
    """(float32 tensor, workspace bytes): out[6] at its start, the workspace from byte _OUT_BYTES on."""
    n = nbytes(_lib.get(), "nll_bytes", 1, 1, 1)
    return torch.empty(((_OUT_BYTES + n + 3) // 4,), dtype=torch.float32, device=dev), n


def _grad_ptr(g):
    """Device pointer of an upstream gradient of one float (None: NULL = zero); the tensor rides along to outlive the call."""
    if g is None:
        return None, None
    if g.dtype != torch.float32:
        g = g.to(torch.float32)
    return g.data_ptr(), g


_weight_cache = {}


def _weight(weight, dev, what):
    """`weight` as a float32 device tensor of one element (None: NULL, the kernels take 1). A tensor is used as it is (the
    kernels read it on every run), a Python float is copied to the device once."""
    if weight is None:
        return None
    if torch.is_tensor(weight):
        if weight.dtype != torch.float32:
            raise TypeError(f"uncertainty {what}: the weight tensor is float32, not {weight.dtype}")
        if weight.numel() != 1:
            raise ValueError(f"uncertainty {what}: the weight tensor holds one float, got {tuple(weight.shape)}")
        _on_device(weight, what)
        if weight.device != dev:
            raise RuntimeError(f"uncertainty {what}: the weight tensor lives on {weight.device}, the inputs on {dev}")
        return weight.detach() if weight.requires_grad else weight
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), float(weight))
    t = _weight_cache.get(key)
    if t is None:
        t = _weight_cache[key] = torch.tensor([float(weight)], dtype=torch.float32, device=dev)
    return t


class _NLL(torch.autograd.Function):
    """(total [], loss [], stats [4]) = f(input [C,H,W], var_or_mask [Cv,H,W]); target, weight and the sizes ride along."""

    @staticmethod
    def forward(ctx, x, vm, target, weight, cfg):
        planes, H, W, mode, var_planes, floor, eps = cfg
        x = x if x.is_contiguous() else x.contiguous()
        vm = vm if vm.is_contiguous() else vm.contiguous()
        buf, ws_bytes = _buffer(x.device)
        p = buf.data_ptr()
        call("eogs_nll_forward", x.device, planes, H, W, mode, x.data_ptr(), target.data_ptr(), vm.data_ptr(), var_planes, floor,
             eps, None if weight is None else weight.data_ptr(), p, p + _OUT_BYTES, ws_bytes)
        ctx.cfg = cfg
        ctx.save_for_backward(x, vm, target, weight)
        ctx.set_materialize_grads(False)
        stats = buf[2:6]
        ctx.mark_non_differentiable(stats)
        return buf[1], buf[0], stats

    @staticmethod
    def backward(ctx, g_total, g_loss, _g_stats):
        want_x, want_vm = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_total is None and g_loss is None) or not (want_x or want_vm):
            return (None,) * 5
        planes, H, W, mode, var_planes, floor, eps = ctx.cfg
        x, vm, target, weight = ctx.saved_tensors
        (pt, _kt), (pl, _kl) = _grad_ptr(g_total), _grad_ptr(g_loss)
        g_x = torch.empty_like(x) if want_x else None
        g_vm = torch.empty_like(vm) if want_vm else None
        call("eogs_nll_backward", x.device, planes, H, W, mode, x.data_ptr(), target.data_ptr(), vm.data_ptr(), var_planes, floor,
             eps, None if weight is None else weight.data_ptr(), pl, pt, None if g_x is None else g_x.data_ptr(),
             None if g_vm is None else g_vm.data_ptr())
        return g_x, g_vm, None, None, None


def _image(t, name, what):
    """(planes, H, W) of a (C, H, W) or (H, W) float32 image."""
    if not torch.is_tensor(t):
        raise TypeError(f"uncertainty {what}: expected a tensor for {name}, got {type(t).__name__}")
    if t.ndim not in (2, 3):
        raise ValueError(f"uncertainty {what}: {name} is a (C, H, W) or (H, W) tensor (batched inputs are not provided), got {tuple(t.shape)}")
    if t.numel() == 0:
        raise ValueError(f"uncertainty {what}: {name} is empty, {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"uncertainty {what}: {name} is float32, not {t.dtype}")
    return (1,) * (3 - t.ndim) + tuple(int(s) for s in t.shape)


def _run(what, x, target, vm, vm_name, mode, weight, floor, eps):
    planes, H, W = _image(x, "the input", what)
    if not torch.is_tensor(target) or tuple(target.shape) != tuple(x.shape):
        raise ValueError(f"uncertainty {what}: the target has the input's shape {tuple(x.shape)}, got {tuple(getattr(target, 'shape', ()))}")
    if target.dtype != torch.float32:
        raise TypeError(f"uncertainty {what}: the target is float32, not {target.dtype}")
    if target.requires_grad:
        raise RuntimeError(f"uncertainty {what}: the target requires grad; the ground truth takes no gradient here")
    if not torch.is_tensor(vm):
        raise TypeError(f"uncertainty {what}: expected a tensor for {vm_name}, got {type(vm).__name__}")
    shapes = [(H, W), (1, H, W)] if mode & NLL_MASK else [tuple(x.shape), (H, W), (1, H, W)]
    if tuple(vm.shape) not in shapes:
        raise ValueError(f"uncertainty {what}: {vm_name} has one of the shapes {shapes}, got {tuple(vm.shape)}")
    if vm.dtype != torch.float32:
        raise TypeError(f"uncertainty {what}: {vm_name} is float32, not {vm.dtype}")
    var_planes = planes if (vm.ndim == 3 and vm.shape[0] == planes) else 1
    floor, eps = float(floor), float(eps)
    if not (0.0 <= floor < float("inf")):
        raise ValueError(f"uncertainty {what}: floor must be finite and not negative, got {floor}")
    if not (0.0 < eps < float("inf")):
        raise ValueError(f"uncertainty {what}: eps must be finite and positive, got {eps}")
    for t in (x, target, vm):
        _on_device(t, what)
        if t.device != x.device:
            raise RuntimeError(f"uncertainty {what}: the inputs live on different devices")
    target = target if target.is_contiguous() else target.contiguous()
    return _NLL.apply(x, vm, target, _weight(weight, x.device, what), (planes, H, W, mode, var_planes, floor, eps))


def transient_nll(image, gt_image, transient_mask, *, weight=None, floor=1e-3, eps=1e-6):
    """(total, loss, stats) of train_pan.py:434-440 in one launch each way:

      loss  = gaussian_nll_loss(image, gt_image, var = (transient_mask.clip(0, 1) + floor)^2 shared by the planes), the mean
      total = weight * loss (weight None: 1)
      stats = the device view of out[2:6]: the mask's mean, its unbiased standard deviation (Tensor.std()), 0, and the number
              of mask pixels outside [0, 1] (`STATS` names them)

    `image`, `gt_image` (C, H, W) or (H, W), `transient_mask` (H, W). Gradients reach `image` and `transient_mask`; the mask's
    is exactly 0 where it lies outside [0, 1] (inclusive bounds, as torch's clamp backward). `weight`: a Python float, or a
    device f32[1] tensor that the kernels read on every run."""
    return _run("transient_nll", image, gt_image, transient_mask, "the transient mask", NLL_MASK, weight, floor, eps)


def gaussian_nll_loss(input, target, var, full=False, eps=1e-6, reduction="mean", *, return_out=False):  # noqa: A002
    """torch.nn.functional.gaussian_nll_loss over (C, H, W) or (H, W) float32 tensors on the GPU, `var` of the input's shape,
    (H, W) or (1, H, W). Never waits: a negative variance is not refused but counted — `return_out=True` also returns the
    device view of out[2:6] = {mean of var, its std, entries with var < 0, 0} — and its element is clamped to `eps` like any
    other, l = 0.5 (log eps + (input - target)^2 / eps). The gradient of `var` is passed on also below `eps`, as torch's."""
    what = "gaussian_nll_loss"
    if reduction == "none":
        raise NotImplementedError(f"uncertainty {what}: reduction='none' is not provided; 'mean' and 'sum' are")
    if reduction not in ("mean", "sum"):
        raise ValueError(reduction + " is not valid")
    mode = (NLL_FULL if full else 0) | (NLL_SUM if reduction == "sum" else 0)
    _, loss, stats = _run(what, input, target, var, "var", mode, None, 0.0, eps)
    return (loss, stats) if return_out else loss


class TransientNLL(torch.nn.Module):
    """The term as a loss class (loss/base_loss.py:5-20): `forward` returns the UNWEIGHTED L_nll, as the reference's classes
    do; the statistics of the last forward stay on the device until `log_stats` asks for them."""

    def __init__(self, w_L_nll, floor=1e-3, eps=1e-6):
        super().__init__()
        self.weight = self.w_L_nll = w_L_nll
        self.floor, self.eps = floor, eps
        self.stats = None

    def forward(self, image, gt_image, transient_mask):
        _, loss, self.stats = transient_nll(image, gt_image, transient_mask, floor=self.floor, eps=self.eps)
        return loss

    def get_loss_name(self):
        return "L_nll"

    def log_loss(self, tb_writer, loss_value, iteration):
        tb_writer.add_scalar(f"loss/{self.get_loss_name()}", loss_value, iteration)

    def log_stats(self):
        """train_pan.py:441-448's two numbers, and the pixels outside [0, 1], of the last forward: ONE small copy."""
        if self.stats is None:
            raise RuntimeError("uncertainty TransientNLL.log_stats: no forward has run yet")
        mean, std, _, clipped = self.stats.tolist()
        return {"mean": mean, "std": std, "clipped": int(clipped)}


def transient_parameters(H, W, init_value, device):
    """The camera's transient mask as affine_cameras.py:282-289 builds it: an (H, W) Parameter filled with `init_value`.
    (`transient_canvas`, :290, is not carried over: its only use is commented out, :339-342.)"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"uncertainty transient_parameters: tensors live on '{device.type}'; the NLL term runs on the GPU only, "
                           "there is no CPU fallback")
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"uncertainty transient_parameters: an empty mask, ({H}, {W})")
    return torch.nn.Parameter(torch.full((int(H), int(W)), float(init_value), device=device, requires_grad=True))


__all__ = ["transient_nll", "gaussian_nll_loss", "TransientNLL", "transient_parameters", "STATS"]
