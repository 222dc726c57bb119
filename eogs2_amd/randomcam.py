"""The random-camera loss in full over the C-ABI of include/eogs_randomcam.h and the resample, shade / pan and rasterizer
modules: the reference's `RandomcamRendering_Loss` (src/gaussiansplatting/loss/main_loss.py:56-221) with both render types,
`use_gt`, and a panchromatic camera.

Same names, arguments and return values as the reference:

* `RandomcamRendering_Loss(w_L_new_altitude_resample, w_L_new_rgb_resample, render_type, use_gt=False)` with `forward`,
  `_forward` and `log_loss`. `forward` takes two keyword-only extras, `virtual_render` and `sun_render`: renders made
  elsewhere (side by side under `eogs2_amd.graph.Branches`, or the iteration's own sun render, train_pan.py:305-316, which
  is the render the reference makes a second time inside this loss: same camera, same Gaussians, same background).
* `render_resample_virtual_camera_wshadowmapping(...)` — gaussian_renderer/renderer_cc_shadow.py:57-145: the virtual view
  goes through the true camera's whole render pipeline, with a shadow map of its own, before it is resampled.
* `virtual_to_sun(cam2virt, camera_to_sun, out=None)` — `(virt_to_sun, K)` in one launch of one wave: the reference's
  `torch.inverse(cam2virt) @ camera_to_sun` (:93-95) and `K = virt_to_sun @ cam2virt`, the matrix from the true camera's
  (u, v, altitude) to the sun camera's. No host wait, no solver library: a stream capture records it, and `cam2virt` may be
  what `eogs2_amd.draw.IterationDraws` writes anew on every replay.
* `cmloss(new_altitude_diff, rgb_render, new_rgb_sample, new_uv)` — `shade.randomcam_l` for 1 to 4 planes; a side that does
  not require grad gets no gradient tensor (the ground-truth image under `use_gt`).

The inner sun lookup is `resample(sun altitude plane, K, rendered_uva, n_out=1, fill_channel=0)`: one composed matrix
where the reference chains two fp32 products per pixel. The reference's indexing is kept: that sample,
indexed by the TRUE camera's pixel, is subtracted from the VIRTUAL camera's altitude at the same index
(renderer_cc_shadow.py:85-109). PyTorch is plumbing; there is no CPU or eager fallback.
"""
import torch

from . import _lib, pan as _pan, shade as _shade
from ._abi import CMLOSS_MAX_CHANNELS
from ._host import Ctx, f32c, nbytes, ptr
from .resample import render_resample_virtual_camera, resample

RENDER_TYPES = ("rawrender", "rawrender_wshadow")


def _on_gpu(what, name, t):
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: {name} on '{t.device}': this runs on the GPU, there is no CPU fallback")


# ---- the composed matrices ----------------------------------------------------------------------------------------------
def check_compose(cam2virt, camera_to_sun, out=None):
    """Everything `virtual_to_sun` refuses before its launch."""
    what = "virtual_to_sun"
    for name, t in (("cam2virt", cam2virt), ("camera_to_sun", camera_to_sun)):
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if tuple(t.shape) != (3, 3):
            raise ValueError(f"{what}: {name} must have shape (3, 3), got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if out is not None:
        if not torch.is_tensor(out):
            raise TypeError(f"{what}: out must be a tensor, got {type(out).__name__}")
        if out.dtype != torch.float32 or out.numel() != 18 or not out.is_contiguous():
            raise ValueError(f"{what}: out must be 18 contiguous float32 values, got {tuple(out.shape)} {out.dtype}")
        if out.requires_grad:
            raise ValueError(f"{what}: out is written in place and must not require grad")
    dev = cam2virt.device
    for name, t in (("camera_to_sun", camera_to_sun), ("out", out)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{what}: {name} on {t.device}, cam2virt on {dev}")
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: cam2virt on '{dev}': this runs on the GPU, there is no CPU fallback")
    return dev


def virtual_to_sun(cam2virt, camera_to_sun, out=None):
    """(virt_to_sun[3,3], K[3,3]) = (inv(cam2virt) @ camera_to_sun, virt_to_sun @ cam2virt), formed in double on the device and
    rounded to float32 once; views of `out` (18 floats). With `out=None` the 18 floats are allocated here: inside a stream capture
    they come from the graph's private pool like every other intermediate of the step (this is what
    `render_resample_virtual_camera_wshadowmapping` does); `out` is for a caller that keeps the matrices across replays.
    A singular `cam2virt` gives NaN where the reference's torch.inverse raises. The matrices are constants to autograd, as in
    the reference, where they come from fixed camera matrices."""
    dev = check_compose(cam2virt, camera_to_sun, out)
    abi = _lib.get()
    c = cam2virt.detach().contiguous()
    s = camera_to_sun.detach().contiguous()
    with Ctx(abi, dev) as cx:
        if out is None:
            out = torch.empty((18,), dtype=torch.float32, device=dev)
        abi.check(abi.randomcam_compose(ptr(c), ptr(s), ptr(out), cx.stream))
    flat = out.view(-1)
    return flat[:9].view(3, 3), flat[9:].view(3, 3)


# ---- the comparison -----------------------------------------------------------------------------------------------------
def check_cmloss(alt_diff, rgb_a, rgb_b, uv):
    """Everything `cmloss` refuses before its launch; returns (C, H, W)."""
    what = "cmloss"
    for name, t in (("new_altitude_diff", alt_diff), ("rgb_render", rgb_a), ("new_rgb_sample", rgb_b), ("new_uv", uv)):
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if alt_diff.ndim != 2 or alt_diff.numel() == 0:
        raise ValueError(f"{what}: new_altitude_diff must be (H, W), got {tuple(alt_diff.shape)}")
    H, W = alt_diff.shape
    if rgb_a.ndim != 3 or not 1 <= rgb_a.shape[0] <= CMLOSS_MAX_CHANNELS or tuple(rgb_a.shape[1:]) != (H, W):
        raise ValueError(f"{what}: rgb_render must be (C, {H}, {W}) with 1 <= C <= {CMLOSS_MAX_CHANNELS}, got {tuple(rgb_a.shape)}")
    if tuple(rgb_b.shape) != tuple(rgb_a.shape):
        raise ValueError(f"{what}: new_rgb_sample must be {tuple(rgb_a.shape)} like rgb_render, got {tuple(rgb_b.shape)}")
    if tuple(uv.shape) != (H, W, 2):
        raise ValueError(f"{what}: new_uv must be ({H}, {W}, 2), got {tuple(uv.shape)}")
    dev = alt_diff.device
    for name, t in (("rgb_render", rgb_a), ("new_rgb_sample", rgb_b), ("new_uv", uv)):
        if t.device != dev:
            raise RuntimeError(f"{what}: {name} on {t.device}, new_altitude_diff on {dev}")
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: new_altitude_diff on '{dev}': this runs on the GPU, there is no CPU fallback")
    return rgb_a.shape[0], H, W


class _CMLoss(torch.autograd.Function):
    """out[3] = {L_alt, L_rgb, mask count}"""

    @staticmethod
    def forward(ctx, alt_diff, rgb_a, rgb_b, uv):
        C, H, W = check_cmloss(alt_diff, rgb_a, rgb_b, uv)
        abi = _lib.get()
        dev = alt_diff.device
        d, a, b, u = (f32c(t, dev, f"cmloss: {n}") for n, t in (("new_altitude_diff", alt_diff), ("rgb_render", rgb_a),
                                                              ("new_rgb_sample", rgb_b), ("new_uv", uv)))
        with Ctx(abi, dev) as cx:
            out = torch.empty((3,), dtype=torch.float32, device=dev)
            ws = torch.empty((nbytes(abi, "cmloss_bytes", H, W),), dtype=torch.uint8, device=dev)
            abi.check(abi.cmloss_forward(H, W, C, ptr(d), ptr(a), ptr(b), ptr(u), ptr(out), ptr(ws), ws.numel(), cx.stream))
        ctx.cfg = (H, W, C)
        ctx.save_for_backward(d, a, b, u, out)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_out):
        if g_out is None:
            return (None,) * 4
        abi = _lib.get()
        H, W, C = ctx.cfg
        d, a, b, u, out = ctx.saved_tensors
        dev = d.device
        with Ctx(abi, dev) as cx:
            up = f32c(g_out, dev, "cmloss: the upstream gradient")[:2].contiguous()
            g_alt = torch.empty((H, W), dtype=torch.float32, device=dev)
            g_a = torch.empty((C, H, W), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
            g_b = torch.empty((C, H, W), dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
            abi.check(abi.cmloss_backward(H, W, C, ptr(d), ptr(a), ptr(b), ptr(u), ptr(out), ptr(up), ptr(g_alt), ptr(g_a),
                                          ptr(g_b), cx.stream))
        return g_alt, g_a, g_b, None


def cmloss(new_altitude_diff, rgb_render, new_rgb_sample, new_uv):
    """(L_new_altitude_resample, L_new_rgb_resample), loss/main_loss.py:149-164, for (C, H, W) images with 1 <= C <= 4:
    occlusion map |diff| < 0.30 inside the virtual view, masked mean absolute differences (all C planes over the pixel
    count); two device zeros for an empty map, without the reference's `.any()` wait."""
    out = _CMLoss.apply(new_altitude_diff, rgb_render, new_rgb_sample, new_uv)
    return out[0], out[1]


# ---- the shadow-mapped virtual view --------------------------------------------------------------------------------------
def _pipeline_of(true_cam):
    return _pan.render_pipeline if hasattr(true_cam, "msi_to_pan") else _shade.render_pipeline


def render_resample_virtual_camera_wshadowmapping(virtual_camera, true_cam, cam2virt, rendered_uva, gaussians, pipe, background,
                                                  return_extra=False, *, virtual_render=None, sun_render=None):
    """renderer_cc_shadow.py:57-145. Returns (virtual_rgb_sample[n,H,W], virtual_altitude_sample[H,W], virtual_uv[H,W,2]), and
    with `return_extra` the whole sample [n+1,H,W] as a fourth value; n = 3, or 1 for a panchromatic camera.

    `true_cam` is duck-typed: `get_sun_camera()` -> (sun_camera, camera_to_sun), and what `shade.render_pipeline` reads, or
    `pan.render_pipeline` when it carries `msi_to_pan`. `virtual_render` [5,H,W] hands in the virtual camera's render,
    `sun_render` the sun camera's — [5,Hs,Ws] or the altitude-only [1,Hs,Ws] — instead of rendering here; with the iteration's
    own sun render the loss costs no second one (same camera, Gaussians and background: the same image), and its gradient
    reaches that render's graph. With both None this renders as the reference does."""
    what = "render_resample_virtual_camera_wshadowmapping"
    _on_gpu(what, "rendered_uva", rendered_uva)
    if rendered_uva.ndim != 3 or rendered_uva.shape[-1] != 3:
        raise ValueError(f"{what}: rendered_uva must be (H, W, 3), got {tuple(rendered_uva.shape)}")
    H, W = rendered_uva.shape[:2]
    if virtual_render is not None:
        _on_gpu(what, "virtual_render", virtual_render)
        if virtual_render.ndim != 3 or virtual_render.shape[0] < 4 or tuple(virtual_render.shape[1:]) != (H, W):
            raise ValueError(f"{what}: virtual_render must be (5, {H}, {W}) — the virtual camera's altitude is compared index by "
                             f"index with a sample on the true camera's grid —, got {tuple(virtual_render.shape)}")
    if sun_render is not None:
        _on_gpu(what, "sun_render", sun_render)
        if sun_render.ndim != 3 or sun_render.shape[0] not in (1, 5):
            raise ValueError(f"{what}: sun_render must be (5, Hs, Ws) or the altitude-only (1, Hs, Ws), got {tuple(sun_render.shape)}")
    sun_camera, camera_to_sun = true_cam.get_sun_camera()
    check_compose(cam2virt, camera_to_sun)
    from .render import render

    if virtual_render is None:
        virtual_render = render(virtual_camera, gaussians, pipe, background)["render"]
        if tuple(virtual_render.shape[1:]) != (H, W):
            raise ValueError(f"{what}: the virtual camera renders {tuple(virtual_render.shape[1:])}, rendered_uva is ({H}, {W})")
    _, K = virtual_to_sun(cam2virt, camera_to_sun)
    if sun_render is None:
        sun_render = render(sun_camera, gaussians, pipe, background)["render"]
    sun_plane = sun_render if sun_render.shape[0] == 1 else sun_render[3:4]
    sun_sample, _ = resample(sun_plane, K, rendered_uva, n_out=1, fill_channel=0, fill_value=-100.0)
    virtual_altitude_diff = virtual_render[3] - sun_sample[0]
    true_output = _pipeline_of(true_cam)(true_cam, virtual_render[:3], virtual_altitude_diff)
    shaded = true_output["shaded"]
    n = shaded.shape[0]
    source = torch.cat([shaded, virtual_render[3:]], dim=0)
    sample, virtual_uv = resample(source, cam2virt, rendered_uva, n_out=n + 1, fill_channel=n, fill_value=-100.0)
    if return_extra:
        return sample[:n], sample[n], virtual_uv, sample
    return sample[:n], sample[n], virtual_uv


class RandomcamRendering_Loss(torch.nn.Module):
    """loss/main_loss.py:56-221: the small-deformation loss, consistent rendering under a small camera perturbation.

    render_type "rawrender": the virtual camera's raw render is resampled and compared with `raw_render`;
    "rawrender_wshadow": it goes through the true camera's render pipeline first and is compared with `shaded`.
    use_gt: the comparison target is `gt_image`, which takes no gradient.

    The reference's `_forward_from_camera` (main_loss.py:166-191) is not here: nothing calls it, and it cannot run there either
    (it hands three arguments to the eleven-argument `forward`)."""

    def __init__(self, w_L_new_altitude_resample, w_L_new_rgb_resample, render_type, use_gt: bool = False):
        super().__init__()
        self.weight = 0  # base_Loss(weight=0)
        self.w_L_randomcam_rendering = w_L_new_altitude_resample
        self.w_L_new_rgb_resample = w_L_new_rgb_resample
        self.render_type = render_type
        self.use_gt = use_gt
        if self.use_gt:
            print("You are using gt image for random camera loss, be sure this is what you want")
        assert self.render_type in RENDER_TYPES, "render type not implemented,got " + str(self.render_type)

    def get_loss_name(self):
        return self.__class__.__name__

    def _forward(self, new_occlusion_map, new_altitude_diff, new_rgb_diff_map):
        """main_loss.py:83-96 for a map that `forward`'s statement built (:151-154: it is set only where |diff| < 0.30): the
        masked means through the same kernels — the difference map against zero, the map as coordinates inside or outside the
        view —, two device zeros for an empty map. `forward` itself does not come through here: it hands the kernels the
        coordinates it has. A pixel the map sets where |diff| >= 0.30 is left out."""
        inside = new_occlusion_map.bool()[..., None].expand(*new_occlusion_map.shape, 2)
        uv = torch.where(inside, 0.0, 2.0).to(torch.float32).contiguous()
        return cmloss(new_altitude_diff, new_rgb_diff_map, torch.zeros_like(new_rgb_diff_map), uv)

    def forward(self, new_camera, true_cam, camera_to_new, rendered_uva, gaussians, pipe, bg, altitude_render, raw_render, gt_image,
                shaded, *, virtual_render=None, sun_render=None):
        if self.render_type == "rawrender":
            if sun_render is not None:
                raise ValueError("RandomcamRendering_Loss: sun_render belongs to render_type 'rawrender_wshadow'")
            new_rgb_sample, new_altitude_sample, new_uv = self._rawrender_from_camera(
                new_camera, camera_to_new, rendered_uva, gaussians, pipe, bg, virtual_render=virtual_render)
            rgb_render = raw_render
        elif self.render_type == "rawrender_wshadow":
            new_rgb_sample, new_altitude_sample, new_uv = self._rawrender_from_camera_wshadow(
                new_camera, true_cam, camera_to_new, rendered_uva, gaussians, pipe, bg, virtual_render=virtual_render,
                sun_render=sun_render)
            rgb_render = shaded
        else:
            raise NotImplementedError("render type not implemented,got ", self.render_type)
        if self.use_gt:
            rgb_render = gt_image.detach()
        new_altitude_diff = altitude_render - new_altitude_sample
        return cmloss(new_altitude_diff, rgb_render, new_rgb_sample, new_uv)

    def _rawrender_from_camera(self, new_camera, camera_to_new, rendered_uva, gaussians, pipe, bg, *, virtual_render=None):
        if virtual_render is not None:
            sample, new_uv = resample(virtual_render, camera_to_new, rendered_uva)
            return sample[:3], sample[3], new_uv
        return render_resample_virtual_camera(new_camera, camera_to_new, rendered_uva, gaussians, pipe, bg)

    def _rawrender_from_camera_wshadow(self, new_camera, true_cam, camera_to_new, rendered_uva, gaussians, pipe, bg, *,
                                       virtual_render=None, sun_render=None):
        return render_resample_virtual_camera_wshadowmapping(new_camera, true_cam, camera_to_new, rendered_uva, gaussians, pipe, bg,
                                                             return_extra=False, virtual_render=virtual_render, sun_render=sun_render)

    def log_loss(self, tb_writer, L_new_altitude_resample, L_new_rgb_resample, iteration: int) -> None:
        tb_writer.add_scalar("loss/L_new_altitude_resample", L_new_altitude_resample, iteration)
        tb_writer.add_scalar("loss/L_new_rgb_resample", L_new_rgb_resample, iteration)


__all__ = ["RandomcamRendering_Loss", "render_resample_virtual_camera_wshadowmapping", "virtual_to_sun", "cmloss", "check_compose",
           "check_cmloss", "RENDER_TYPES"]
