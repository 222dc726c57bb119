"""Flow matching on the GPU over the eogs_resample_flow_* entries of include/eogs_resample.h: everything the reference
runs around its optical-flow network (src/gaussiansplatting/flowmatching/flow_matching.py, flow_matching_toaffine.py:11-25,
loss/flowmatch.py). Names and signatures follow the reference so that a user can swap imports:

  apply_flow(img, flow, gate=None)                          flow_matching.py:225-253   the warp, one HIP kernel each way
  flow_stats(flow)                                          [mean x, mean y, mean |flow|, std x, std y] on the device
  performOpticalmatching(perform_cst_displacement, ...)     flow_matching.py:18-287
  perform_flow_matching(opt, warper, image, gt_image)       flow_matching.py:293-329
  adjust_affine(world_view_transform, img_W, img_H, flows)  flow_matching_toaffine.py:11-25
  flowmatch_l(flow)                                         loss/flowmatch.py:12-14

The flow network itself (torchvision's RAFT and its weights in the reference) is the caller's: hand any callable with
RAFT's call shape to `performOpticalmatching(model=...)`.

`apply_flow` samples `img` at (x + flow_x, y + flow_y) in pixels, clamped to the image (border padding), bilinear; the
gradient reaches `img` only (the reference detaches the grid) and is bitwise reproducible, unlike grid_sample's atomic
scatter. A flow whose two spatial strides are 0 — what `set_cst_displacement` returns — is one displacement for the whole
image: the kernels read its two floats from device memory, no host read is made. `gate` (a one-element device tensor)
switches the warp off where it is zero: output and gradient are then copies, bit for bit. With it
`perform_flow_matching(..., on_device=True)` makes the reference's `if abs(flow).mean() < max_value_flow` without waiting
for the device, so the step can be recorded into a HIP graph. fp32 only; CPU tensors raise (no CPU fallback).
"""
import functools

import torch

from . import _lib
from ._host import Ctx, call, nbytes, on_device, ptr


def pgd8(n, k=8):
    """Greatest multiple of k <= n (flow_matching.py:4-6)."""
    return (n // k) * k


def ppcm8(n, k=8):
    """Smallest multiple of k >= n (flow_matching.py:13-15)."""
    return ((n + k - 1) // k) * k


_on_device = functools.partial(on_device, "flow", "the flow warp runs")


def _check_flow(flow, what, H=None, W=None):
    if not torch.is_tensor(flow) or flow.ndim != 4 or flow.shape[0] != 1 or flow.shape[1] != 2:
        raise ValueError(f"flow {what}: the flow is a (1, 2, H, W) tensor, got {tuple(getattr(flow, 'shape', ()))}")
    if flow.dtype != torch.float32:
        raise TypeError(f"flow {what}: the flow is float32, not {flow.dtype}")
    if H is not None and tuple(flow.shape[2:]) != (H, W):
        raise ValueError(f"flow {what}: the flow is {tuple(flow.shape[2:])}, the image ({H}, {W})")
    if flow.shape[2] < 2 or flow.shape[3] < 2:
        raise ValueError(f"flow {what}: H and W must be at least 2 (the reference divides by W - 1), got {tuple(flow.shape[2:])}")
    return flow.detach()


def _strides(flow):
    return int(flow.stride(1)), int(flow.stride(2)), int(flow.stride(3))


def _check_gate(gate, dev):
    if gate is None:
        return None
    _on_device(gate, "apply_flow")
    if gate.device != dev:
        raise RuntimeError("flow apply_flow: gate lives on another device")
    return gate.detach().reshape(1).to(torch.float32)  # (of a bool: a device op, no host read)


class _ApplyFlow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, flow, gate):
        C, H, W = img.shape
        x = img if img.is_contiguous() else img.contiguous()
        out = torch.empty_like(x)
        call("eogs_resample_flow_forward", x.device, C, H, W, x.data_ptr(), flow.data_ptr(), *flow.stride()[1:],
             None if gate is None else gate.data_ptr(), out.data_ptr())
        ctx.flow, ctx.gate = flow, gate  # (not save_for_backward: a network run under inference_mode returns inference tensors)
        return out

    @staticmethod
    def backward(ctx, g_out):
        if g_out is None or not ctx.needs_input_grad[0]:
            return None, None, None
        flow, gate = ctx.flow, ctx.gate
        C, H, W = g_out.shape
        sc, sy, sx = flow.stride()[1:]
        g = g_out if g_out.dtype == torch.float32 and g_out.is_contiguous() else g_out.to(torch.float32).contiguous()
        g_img = torch.empty_like(g)
        ws, ws_ptr, ws_bytes = None, None, 0
        if sy or sx:  # a field: the boxes of the bucketed gather (a constant displacement needs no workspace)
            ws_bytes = nbytes(_lib.get(), "resample_flow_bytes", H, W)
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=g.device)
            ws_ptr = ws.data_ptr()
        call("eogs_resample_flow_backward", g.device, C, H, W, flow.data_ptr(), sc, sy, sx,
             None if gate is None else gate.data_ptr(), g.data_ptr(), g_img.data_ptr(), ws_ptr, ws_bytes)
        return g_img, None, None


def apply_flow(img, flow, gate=None):
    """flow_matching.py:225-253: `img` (C, H, W) or (H, W) warped by `flow` (1, 2, H, W) in pixels (channel 0 horizontal,
    1 vertical); returns (C, H, W), so (1, H, W) for a 2-D input. See the module docstring for `gate`.

    The backward reads `flow` and `gate` again, from the same memory, and autograd does not watch them (they are kept
    beside the graph, not in it: a flow network run under inference_mode returns tensors that cannot be saved for backward).
    Overwriting either buffer between forward and backward therefore changes the gradient without an error; a replayed
    graph, which refills the flow buffer before each replay, relies on exactly that."""
    if not torch.is_tensor(img) or img.ndim not in (2, 3) or img.numel() == 0:
        raise ValueError(f"flow apply_flow: the image is a non-empty (C, H, W) or (H, W) tensor, got {tuple(getattr(img, 'shape', ()))}")
    if img.dtype != torch.float32:
        raise TypeError(f"flow apply_flow: the image is float32, not {img.dtype}")
    if img.ndim == 2:
        img = img.unsqueeze(0)
    flow = _check_flow(flow, "apply_flow", int(img.shape[1]), int(img.shape[2]))
    if gate is not None and (not torch.is_tensor(gate) or gate.numel() != 1):
        raise ValueError("flow apply_flow: gate is a one-element tensor on the device")
    _on_device(img, "apply_flow")
    _on_device(flow, "apply_flow")
    if flow.device != img.device:
        raise RuntimeError("flow apply_flow: image and flow live on different devices")
    return _ApplyFlow.apply(img, flow, _check_gate(gate, img.device))


def flow_stats(flow):
    """Device tensor [mean x, mean y, mean |flow| over both planes, std x, std y] of a (1, 2, H, W) flow; the std is
    unbiased, as torch.std. One pass, sums in float64 in a fixed order: bitwise reproducible."""
    flow = _check_flow(flow, "flow_stats")
    _on_device(flow, "flow_stats")
    abi = _lib.get()
    H, W = int(flow.shape[2]), int(flow.shape[3])
    dev = flow.device
    with Ctx(abi, dev) as cx:
        ws = torch.empty((nbytes(abi, "resample_flow_stats_bytes", H, W),), dtype=torch.uint8, device=dev)
        stats = torch.empty((5,), dtype=torch.float32, device=dev)
        abi.check(abi.resample_flow_stats(H, W, ptr(flow), *_strides(flow), ptr(stats), ptr(ws), ws.numel(), cx.stream))
    return stats


class performOpticalmatching:
    """flow_matching.py:18-287 around a flow network the caller brings: `model(gt[1,3,h,w], target[1,3,h,w],
    num_flow_updates=...) -> list of flows`, h and w multiples of 8 (torchvision RAFT's call shape)."""

    def __init__(self, perform_cst_displacement, mode="downscale", device="cuda", model_name="large", num_flow_updates=12,
                 criteria="max_value_flow", model=None):
        self.device = device
        self.perform_cst_displacement = perform_cst_displacement
        assert mode in ["downscale", "upscale"], f"mode should be downscale or upscale, got {mode}"
        self.mode = mode
        self.model_name = model_name
        assert model_name in ["large", "small"], f"model_name should be either large or small, got {model_name}"
        assert criteria in ["max_value_flow", "psnr", "l_photom", "always"], \
            f"criteria should be either max_value_flow, psnr, l_photom or always, got {criteria}"
        self.criteria = criteria
        self.num_flow_updates = num_flow_updates
        self._model = model

    def set_cst_displacement(self, flow):
        """The mean displacement as a (1, 2, H, W) flow: the reference's filled tensor as a stride-0 view of two floats."""
        return flow_stats(flow)[:2].view(1, 2, 1, 1).expand(1, 2, flow.shape[2], flow.shape[3])

    def _get_model(self):
        if self._model is None:
            raise RuntimeError(f"performOpticalmatching: no flow network. The reference loads torchvision's raft_{self.model_name} here; "
                               "in this package the flow network is the caller's: pass model=<callable(gt, target, "
                               "num_flow_updates=...) -> list of flows>")
        return self._model

    def normalize_img_raft(self, img):
        """[0, 1] -> [-1, 1]."""
        return (img - 0.5) * 2

    def adjust_img_for_raft(self, normalized_img_msi_gt, normalized_img_msi_target, img_msi_gt, img_msi_target):
        """The network wants sizes that are multiples of 8: "downscale" crops all four images to the greatest one,
        "upscale" reflect-pads the two normalised ones on the right and at the bottom (the flow is cropped back to (n, m))."""
        if self.mode == "downscale":
            i1 = min(pgd8(normalized_img_msi_gt.shape[2]), pgd8(normalized_img_msi_target.shape[2]))
            j1 = min(pgd8(normalized_img_msi_gt.shape[3]), pgd8(normalized_img_msi_target.shape[3]))
            normalized_img_msi_gt = normalized_img_msi_gt[:, :, :i1, :j1]
            normalized_img_msi_target = normalized_img_msi_target[:, :, :i1, :j1]
            img_msi_gt = img_msi_gt[:, :i1, :j1]
            img_msi_target = img_msi_target[:, :i1, :j1]
            n = m = -1
        elif self.mode == "upscale":
            n, m = img_msi_gt.shape[1], img_msi_gt.shape[2]
            i1 = max(ppcm8(normalized_img_msi_gt.shape[2]), ppcm8(normalized_img_msi_target.shape[2]))
            j1 = max(ppcm8(normalized_img_msi_gt.shape[3]), ppcm8(normalized_img_msi_target.shape[3]))
            pad = lambda t: torch.nn.functional.pad(t, (0, j1 - t.shape[-1], 0, i1 - t.shape[-2]), mode="reflect")  # noqa: E731
            normalized_img_msi_gt, normalized_img_msi_target = pad(normalized_img_msi_gt), pad(normalized_img_msi_target)
        else:
            raise ValueError("mode should be either downscale or upscale")
        return normalized_img_msi_gt, normalized_img_msi_target, img_msi_gt, img_msi_target, n, m

    def get_flow(self, img_msi_gt, img_msi_target, device="cuda"):
        """(flow, gt, target): the network's last flow from `gt` to `target` (one-plane images are repeated three times),
        cropped back in "upscale" mode, replaced by its mean displacement with perform_cst_displacement."""
        assert img_msi_gt.shape[0] == img_msi_target.shape[0], \
            " size of both images should be the same, got {} and {}".format(img_msi_gt.shape, img_msi_target.shape)
        if img_msi_gt.shape[0] == 1:
            normalized_img_msi_gt = img_msi_gt.expand(3, -1, -1)
            normalized_img_msi_target = img_msi_target.expand(3, -1, -1)
        else:
            normalized_img_msi_gt, normalized_img_msi_target = img_msi_gt, img_msi_target
        assert normalized_img_msi_gt.shape[0] == 3, "Image should have 3 channels, got {}".format(normalized_img_msi_gt.shape[0])
        normalized_img_msi_gt = self.normalize_img_raft(normalized_img_msi_gt).unsqueeze(0)
        normalized_img_msi_target = self.normalize_img_raft(normalized_img_msi_target).unsqueeze(0)
        normalized_img_msi_gt, normalized_img_msi_target, img_msi_gt, img_msi_target, n, m = self.adjust_img_for_raft(
            normalized_img_msi_gt, normalized_img_msi_target, img_msi_gt, img_msi_target)
        model = self._get_model()
        with torch.inference_mode():
            list_of_flows = model(normalized_img_msi_gt.to(device), normalized_img_msi_target.to(device),
                                  num_flow_updates=self.num_flow_updates)
        predicted_flows = list_of_flows[-1]
        if self.mode == "upscale":
            predicted_flows = predicted_flows[:, :, :n, :m]
        if self.perform_cst_displacement:
            predicted_flows = self.set_cst_displacement(predicted_flows)
        return predicted_flows, img_msi_gt, img_msi_target

    def apply_flow(self, img_msi_target, flow, gate=None):
        return apply_flow(img_msi_target, flow, gate)

    def compute_stats(self, predicted_flows, verbose=False):
        """(horizontal mean, vertical mean, horizontal std, vertical std) as 0-d device tensors."""
        s = flow_stats(predicted_flows)
        if verbose:
            print(f"min = {predicted_flows.min()}, max = {predicted_flows.max()}")
            print(f"horizontal mean = {s[0]}, std = {s[3]}")
            print(f"vertical mean = {s[1]}, std = {s[4]}")
        return s[0], s[1], s[3], s[4]

    def get_and_apply_flow(self, img_msi_gt, img_msi_target, device="cuda", verbose=False):
        """The flow from the gt image to the target image, applied to the target image."""
        predicted_flows, img_msi_gt, img_msi_target = self.get_flow(img_msi_gt, img_msi_target, device)
        return predicted_flows, img_msi_gt, self.apply_flow(img_msi_target, predicted_flows)


def psnr(img1, img2):
    """utils/image_utils.py:19-21: one value per leading plane, shape (C, 1)."""
    mse = ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def perform_flow_matching(opt, warper, image, gt_image, on_device=False):
    """flow_matching.py:293-329: (predicted_flows, gt_image, image) with the image warped onto the ground truth when the
    warper's criterion accepts the flow, the ORIGINAL `image` and `gt_image` objects when it rejects it.

    on_device=True (mode "upscale" with criteria "max_value_flow" or "always"; anything else raises ValueError): the
    comparison stays on the device and gates the warp, no host read is made, and the returned image is always the gated
    warp — the input's values where the criterion rejects, gradient passed through unchanged."""
    if on_device:
        if warper.mode != "upscale" or warper.criteria not in ("max_value_flow", "always"):
            raise ValueError('perform_flow_matching: on_device=True needs mode "upscale" (a crop changes shapes with the decision) '
                             f'and criteria "max_value_flow" or "always", got {warper.mode!r} and {warper.criteria!r}')
        predicted_flows, gt_image2, image_t = warper.get_flow(gt_image, image)
        gate = None
        if warper.criteria == "max_value_flow":
            gate = flow_stats(predicted_flows)[2:3] < opt.flowmatching.max_value_flow
        return predicted_flows, gt_image2, warper.apply_flow(image_t, predicted_flows, gate=gate)
    predicted_flows, gt_image2, image2 = warper.get_and_apply_flow(img_msi_gt=gt_image, img_msi_target=image)
    apply_flowmatch = False
    if warper.criteria == "max_value_flow":
        if float(flow_stats(predicted_flows)[2]) < opt.flowmatching.max_value_flow:
            apply_flowmatch = True
    if warper.criteria == "always":
        apply_flowmatch = True
    if warper.criteria == "psnr":
        with torch.no_grad():
            if psnr(gt_image2, image2) > psnr(gt_image, image):  # (more than one plane: ambiguous, raises as the reference's does)
                apply_flowmatch = True
    if warper.criteria == "l_photom":
        from .losses import photometric_loss

        with torch.no_grad():
            before, _ = photometric_loss(image, gt_image, 0.2)
            after, _ = photometric_loss(image2, gt_image2, 0.2)
            if float(after) < float(before):
                apply_flowmatch = True
    if apply_flowmatch:
        gt_image, image = gt_image2, image2
    return predicted_flows, gt_image, image


def adjust_affine(world_view_transform, img_W, img_H, predicted_flows):
    """flow_matching_toaffine.py:11-25, in place on the last row: the mean displacement (gt image -> image, in pixels)
    leaves the camera's offsets, rescaled to its [-1, 1] coordinates. No host read."""
    s = flow_stats(predicted_flows)
    b = world_view_transform[-1, :]
    b[0] -= s[0] * 2 / img_W
    b[1] -= s[1] * 2 / img_H
    world_view_transform[-1, :] = b
    return world_view_transform


def flowmatch_l(flow):
    """loss/flowmatch.py:12-14: |mean(flow)| over both planes."""
    s = flow_stats(flow)
    return torch.abs((s[0] + s[1]) * 0.5)


__all__ = ["adjust_affine", "apply_flow", "flow_stats", "flowmatch_l", "perform_flow_matching", "performOpticalmatching", "pgd8", "ppcm8",
           "psnr"]
