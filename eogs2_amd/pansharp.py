"""Pansharpening of the PAN target and the PAN-side losses over the C-ABI of include/eogs_gtprep.h.

Same names, keyword names and accepted shapes as the reference (paths under src/gaussiansplatting/):

  brovey_pansharp(img_pan, img_msi, W=0.1)     pansharpening/algorithm/brovey.py:31-49   PAN (H,W), (1,H,W) or (H,W,1); MSI (C,h,w)
  simple_brovey(img_pan, img_msi)              pansharpening/algorithm/brovey.py:5-28    PAN (H,W); MSI (1,C,h,w)
  ihs_fusion(img_pan, img_msi)                 pansharpening/algorithm/ihs.py            PAN (1,H,W); MSI (3,h,w)
  load_pansharp(pansharp_cfg)                  pansharpening/load_pansharp.py            an object with `.method`, or the name
  Lpan(lambda_Lpan)(pan_image, gt_pan_image)                                   loss/PAN_loss.py:5-13
  Lgradient_pan(lambda_lgradient_pan)(pan_image, gt_pan_image)                 loss/PAN_loss.py:16-30
  Pansharploss(lambda_L_pansharp, pansharp_cfg)(syn_msi_image, gt_pan_image, gt_msi_image)   loss/pansharp_loss.py

and beside each class a plain function: `pan_l2`, `pan_gradient_l2`, `pansharp_l2`.

One kernel upsamples the MSI image (torch's F.interpolate rule, align_corners=False: bicubic for brovey, bilinear for the
other two) and fuses it with the PAN image; the three results are (C, H, W) float32 on the device and carry NO gradient:
the inputs are ground truth. `Pansharploss` computes that value on the fly in its forward and its backward kernel and never
stores it; the gradient of every loss reaches the rendered image only (the first argument). Sums run in a fixed order: the
same bits on every run. Every call only queues launches, so a recorded step holds it. fp32 only; CPU tensors raise (no CPU
fallback).
"""
import functools

import torch

from . import _lib
from ._abi import GTPREP_BROVEY, GTPREP_IHS, GTPREP_MAX_CHANNELS, GTPREP_SIMPLE_BROVEY
from ._host import call, nbytes, on_device

METHODS = {"brovey": GTPREP_BROVEY, "simple_brovey": GTPREP_SIMPLE_BROVEY, "ihs": GTPREP_IHS}
_OUT_BYTES = 32
_on_device = functools.partial(on_device, "pansharp", "ground-truth preparation runs")


def _buffer(dev, C=1):
    """(float32 tensor, workspace bytes): the result float at its start, the reduction workspace from byte _OUT_BYTES on."""
    n = nbytes(_lib.get(), "gtprep_bytes", C)
    return torch.empty(((_OUT_BYTES + n + 3) // 4,), dtype=torch.float32, device=dev), n


def _f32(t, name, what):
    if not torch.is_tensor(t):
        raise TypeError(f"pansharp {what}: {name} is a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"pansharp {what}: {name} is float32, not {t.dtype}")


def _pair(img_pan, img_msi, what, syn=None):
    """(pan (H,W), msi (C,h,w)) contiguous and detached, after the checks every method shares; `syn`: the image a loss
    compares with, (C,H,W) on the same device."""
    if img_pan.ndim != 2 or img_msi.ndim != 3 or 0 in img_pan.shape or 0 in img_msi.shape:
        raise ValueError(f"pansharp {what}: a non-empty PAN plane (H, W) and MSI image (C, h, w), got {tuple(img_pan.shape)} and "
                         f"{tuple(img_msi.shape)}")
    if img_msi.shape[0] > GTPREP_MAX_CHANNELS:
        raise ValueError(f"pansharp {what}: at most {GTPREP_MAX_CHANNELS} MSI channels, got {img_msi.shape[0]}")
    if syn is not None:
        _f32(syn, "syn_msi_image", what)
        want = (img_msi.shape[0],) + tuple(img_pan.shape)
        if tuple(syn.shape) != want:
            raise ValueError(f"pansharp {what}: syn_msi_image is {want}, the shape of the pansharpened image, got {tuple(syn.shape)}")
    for t in (img_pan, img_msi) + (() if syn is None else (syn,)):
        _on_device(t, what)
        if t.device != img_pan.device:
            raise RuntimeError(f"pansharp {what}: the inputs live on different devices")
    return img_pan.detach().contiguous(), img_msi.detach().contiguous()


def _fuse(method, pan, msi, weight):
    C, h, w = msi.shape
    H, W = pan.shape
    out = torch.empty((C, H, W), dtype=torch.float32, device=pan.device)
    call("eogs_gtprep_pansharp", pan.device, method, C, h, w, H, W, msi.data_ptr(), pan.data_ptr(), float(weight), out.data_ptr())
    return out


def _brovey_args(img_pan, img_msi, what, syn=None):
    _f32(img_pan, "img_pan", what)
    _f32(img_msi, "img_msi", what)
    if img_pan.ndim == 3:  # brovey.py:37-38: squeeze(); (1,H,W) or (H,W,1) -> (H,W)
        if 1 not in (img_pan.shape[0], img_pan.shape[2]):
            raise ValueError(f"pansharp {what}: img_pan is (H, W), (1, H, W) or (H, W, 1), got {tuple(img_pan.shape)}")
        img_pan = img_pan[0] if img_pan.shape[0] == 1 else img_pan[:, :, 0]
    return _pair(img_pan, img_msi, what, syn)


def _simple_brovey_args(img_pan, img_msi, what, syn=None):
    _f32(img_pan, "img_pan", what)
    _f32(img_msi, "img_msi", what)
    if img_msi.ndim != 4 or img_msi.shape[0] != 1:
        raise ValueError(f"pansharp {what}: img_msi is (1, C, h, w), got {tuple(img_msi.shape)}")
    return _pair(img_pan, img_msi[0], what, syn)


def _ihs_args(img_pan, img_msi, what, syn=None):
    _f32(img_pan, "img_pan", what)
    _f32(img_msi, "img_msi", what)
    assert img_pan.ndim == 3 and img_pan.shape[0] == 1  # ihs.py:17-18
    assert img_msi.ndim == 3 and img_msi.shape[0] == 3
    return _pair(img_pan[0], img_msi, what, syn)


def brovey_pansharp(img_pan, img_msi, W=0.1):
    """Bicubic upsample of `img_msi` (C, h, w) to the size of `img_pan`, then (pan / max(W sum_c u_c, 1e-8)) u_c: (C, H, W)."""
    pan, msi = _brovey_args(img_pan, img_msi, "brovey_pansharp")
    return _fuse(GTPREP_BROVEY, pan, msi, W)


def simple_brovey(img_pan, img_msi):
    """Bilinear upsample of `img_msi` (1, C, h, w) to the size of `img_pan` (H, W), then u_c pan / (sum_c u_c + 1e-8): (C, H, W)."""
    pan, msi = _simple_brovey_args(img_pan, img_msi, "simple_brovey")
    return _fuse(GTPREP_SIMPLE_BROVEY, pan, msi, 0.0)


def ihs_fusion(img_pan, img_msi):
    """Bilinear upsample of `img_msi` (3, h, w) to the size of `img_pan` (1, H, W), then clamp(u_c + pan - mean_c u_c, 0, 1)."""
    pan, msi = _ihs_args(img_pan, img_msi, "ihs_fusion")
    return _fuse(GTPREP_IHS, pan, msi, 0.0)


_BY_NAME = {"ihs": ihs_fusion, "simple_brovey": simple_brovey, "brovey": brovey_pansharp}
_ARGS = {"ihs": _ihs_args, "simple_brovey": _simple_brovey_args, "brovey": _brovey_args}


def _method_name(pansharp_cfg):
    return pansharp_cfg if isinstance(pansharp_cfg, str) else pansharp_cfg.method


def load_pansharp(pansharp_cfg):
    """pansharpening/load_pansharp.py: the function of `pansharp_cfg.method` (or of the name itself), None for "nopansharp"."""
    method = _method_name(pansharp_cfg)
    if method == "nopansharp":
        return None
    if method not in _BY_NAME:
        raise ValueError(f"Unsupported pansharpening method: {method}. Supported methods are 'ihs' and 'brovey'.")
    return _BY_NAME[method]


def _upstream(g):
    """(device pointer, tensor kept alive) of the upstream scalar."""
    if g.dtype != torch.float32:
        g = g.to(torch.float32)
    return g.data_ptr(), g


class _PansharpL2(torch.autograd.Function):
    """mean((syn - pansharp(pan, msi))^2); the gradient reaches syn alone"""

    @staticmethod
    def forward(ctx, syn, pan, msi, method, weight):
        s = syn.contiguous()
        C, h, w = msi.shape
        H, W = pan.shape
        buf, ws_bytes = _buffer(s.device, C)
        p = buf.data_ptr()
        call("eogs_gtprep_pansharp_l2_forward", s.device, method, C, h, w, H, W, s.data_ptr(), msi.data_ptr(), pan.data_ptr(), weight,
             p, p + _OUT_BYTES, ws_bytes)
        ctx.cfg = (method, weight)
        ctx.save_for_backward(s, pan, msi)
        return buf[0]

    @staticmethod
    def backward(ctx, g):
        method, weight = ctx.cfg
        s, pan, msi = ctx.saved_tensors
        C, h, w = msi.shape
        H, W = pan.shape
        up, keep = _upstream(g)
        g_syn = torch.empty_like(s)
        call("eogs_gtprep_pansharp_l2_backward", s.device, method, C, h, w, H, W, s.data_ptr(), msi.data_ptr(), pan.data_ptr(), weight,
             up, g_syn.data_ptr())
        return g_syn, None, None, None, None


class _L2(torch.autograd.Function):
    """mean((image - target)^2); the gradient reaches image alone"""

    @staticmethod
    def forward(ctx, image, target):
        a = image.contiguous()
        buf, ws_bytes = _buffer(a.device)
        p = buf.data_ptr()
        call("eogs_gtprep_l2_forward", a.device, a.numel(), a.data_ptr(), target.data_ptr(), p, p + _OUT_BYTES, ws_bytes)
        ctx.save_for_backward(a, target)
        return buf[0]

    @staticmethod
    def backward(ctx, g):
        a, target = ctx.saved_tensors
        up, keep = _upstream(g)
        g_a = torch.empty_like(a)
        call("eogs_gtprep_l2_backward", a.device, a.numel(), a.data_ptr(), target.data_ptr(), up, g_a.data_ptr())
        return g_a, None


class _GradL2(torch.autograd.Function):
    """mean(gy(image - target)^2) + mean(gx(image - target)^2); the gradient reaches image alone"""

    @staticmethod
    def forward(ctx, image, target):
        a = image.contiguous()
        H, W = a.shape[-2:]
        B = a.numel() // (H * W)
        buf, ws_bytes = _buffer(a.device)
        p = buf.data_ptr()
        call("eogs_gtprep_grad_l2_forward", a.device, B, H, W, a.data_ptr(), target.data_ptr(), p, p + _OUT_BYTES, ws_bytes)
        ctx.save_for_backward(a, target)
        return buf[0]

    @staticmethod
    def backward(ctx, g):
        a, target = ctx.saved_tensors
        H, W = a.shape[-2:]
        up, keep = _upstream(g)
        g_a = torch.empty_like(a)
        call("eogs_gtprep_grad_l2_backward", a.device, a.numel() // (H * W), H, W, a.data_ptr(), target.data_ptr(), up, g_a.data_ptr())
        return g_a, None


def _image_pair(image, target, what):
    _f32(image, "the image", what)
    _f32(target, "the ground truth", what)
    if image.numel() == 0:
        raise ValueError(f"pansharp {what}: empty image")
    _on_device(image, what)
    _on_device(target, what)
    if image.device != target.device:
        raise RuntimeError(f"pansharp {what}: the inputs live on different devices")
    if target.shape != image.shape:  # the reference broadcasts; the kernels read two images of one shape
        target = target.expand(torch.broadcast_shapes(image.shape, target.shape))
        if target.shape != image.shape:
            raise ValueError(f"pansharp {what}: the ground truth {tuple(target.shape)} does not broadcast to the image {tuple(image.shape)}")
    return target.detach().contiguous()


def pan_l2(pan_image, gt_pan_image):
    """Lpan: mean((pan_image - gt_pan_image)^2), one forward and one backward kernel."""
    return _L2.apply(pan_image, _image_pair(pan_image, gt_pan_image, "pan_l2"))


def pan_gradient_l2(pan_image, gt_pan_image):
    """Lgradient_pan: with d = pan_image - gt_pan_image, mean(gy(d)^2) + mean(gx(d)^2) over the last two dimensions, g =
    torch.gradient (unit spacing, edge order 1). An axis shorter than 2 raises ValueError before any launch."""
    what = "pan_gradient_l2"
    if torch.is_tensor(pan_image) and (pan_image.ndim < 2 or pan_image.shape[-1] < 2 or pan_image.shape[-2] < 2):
        raise ValueError(f"pansharp {what}: torch.gradient needs at least 2 elements along each of the last two dimensions "
                         f"(edge order 1), got {tuple(pan_image.shape)}")
    return _GradL2.apply(pan_image, _image_pair(pan_image, gt_pan_image, what))


def pansharp_l2(syn_msi_image, gt_pan_image, gt_msi_image, method="brovey", W=0.1):
    """Pansharploss: mean((syn_msi_image - method(gt_pan_image, gt_msi_image))^2) with the pansharpened image computed on
    the fly; `method` is a name of `load_pansharp`, the shapes of the ground truth are that method's."""
    what = "pansharp_l2"
    if method not in _ARGS:
        raise ValueError(f"Unsupported pansharpening method: {method}. Supported methods are 'ihs' and 'brovey'.")
    pan, msi = _ARGS[method](gt_pan_image, gt_msi_image, what, syn_msi_image)
    return _PansharpL2.apply(syn_msi_image, pan, msi, METHODS[method], float(W) if method == "brovey" else 0.0)


class _Loss(torch.nn.Module):
    """loss/base_loss.py:5-20"""

    def __init__(self, weight=-1):
        super().__init__()
        self.weight = weight

    def get_loss_name(self):
        return self.__class__.__name__

    def log_loss(self, tb_writer, loss_value, iteration):
        tb_writer.add_scalar(f"loss/{self.get_loss_name()}", loss_value, iteration)


class Lpan(_Loss):
    def __init__(self, lambda_Lpan):
        super().__init__()
        self.lambda_Lpan = lambda_Lpan

    def forward(self, pan_image, gt_pan_image):
        return pan_l2(pan_image, gt_pan_image)


class Lgradient_pan(_Loss):
    def __init__(self, lambda_lgradient_pan):
        super().__init__()
        self.lambda_lgradient_pan = lambda_lgradient_pan

    def forward(self, pan_image, gt_pan_image):
        return pan_gradient_l2(pan_image, gt_pan_image)


class Pansharploss(_Loss):
    def __init__(self, lambda_L_pansharp, pansharp_cfg):
        super().__init__()
        self.lambda_L_pansharp = lambda_L_pansharp
        self.pansharp_method = load_pansharp(pansharp_cfg)
        if self.pansharp_method is None:  # (the reference would call None on the first step)
            raise ValueError("Pansharploss: the pansharpening method is 'nopansharp': there is no target to compare with")
        self.method = _method_name(pansharp_cfg)

    def forward(self, syn_msi_image, gt_pan_image, gt_msi_image):
        return pansharp_l2(syn_msi_image, gt_pan_image, gt_msi_image, method=self.method)


__all__ = ["brovey_pansharp", "simple_brovey", "ihs_fusion", "load_pansharp", "pan_l2", "pan_gradient_l2", "pansharp_l2", "Lpan",
           "Lgradient_pan", "Pansharploss", "METHODS"]
