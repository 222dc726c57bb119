"""The optical-flow network of the flow-matching step, RAFT (the reference takes it from torchvision:
flowmatching/flow_matching.py:76-86), with its correlation looked up ON DEMAND over the eogs_raft_* entries of include/eogs_resample.h.

  corr_pyramid(fmap, levels)                        channel-last feature pyramid in one workspace      one launch per level
  corr_lookup(fmap1_cl, pyramid, coords, radius)    [N, levels (2r+1)^2, h, w] correlation features    one launch
  upsample_flow(flow, mask=None)                    convex (mask) or bilinear x 8 upsampling           one launch
  conv2d_cl(inputs, weight, bias, act, add)         channel-last convolution on the fp32 matrix cores  pack + one launch
  FusedUpdate(update_block)                         RAFT-small's update block over that convolution    eight launches per update
  conv2d_rect_cl(inputs, weight, bias, act, add)    the same over kh x kw taps (1 x 5, 5 x 1)          pack + one launch
  FusedUpdateLarge(update_block, mask_predictor)    RAFT-large's update block and mask predictor       eleven launches per update, two per mask
  conv2d_strided_cl(input, weight, ...), finish_cl  the encoders' strided convolution and block tail   pack + one to three launches
  FusedEncoder(encoder_module)                      one of RAFT-small's two encoders                   one call
  fold_batchnorm(weight, bias, gamma, beta, ...)    an eval-mode batch norm folded into its convolution one launch
  FusedEncoderLarge(encoder_module)                 one of RAFT-large's two encoders                   one call
  RAFT, raft_small(), raft_large()                  the two published configurations as nn.Modules
  RAFT.load_weights(path_or_state_dict)             a torchvision checkpoint, strict

RAFT as published materialises the all-pairs correlation volume, n x n floats for n = HW / 64 feature positions plus three
pooled levels, and reads it through grid_sample at every update. Average-pooling the correlation over the second image's
positions equals correlating with the pooled features, and all (2r+1)^2 taps of a pixel at a level share one fractional
offset: the on-demand lookup computes (2r+2)^2 dot products per pixel and level against a small feature pyramid and blends
them 2 x 2. Memory is linear in n. `corr="volume"` keeps the materialised form in plain torch (matmul, avg_pool2d,
grid_sample): it is the CPU path and works in any dtype, so a float64 run of the whole network arbitrates the tests.

The encoders (convolutions, norms) are torch modules under `encoder="torch"`, and so is the update block (motion encoder,
ConvGRU, flow head) under `update="torch"`. Under `encoder="fused"` RAFT-small's two encoders run over the eogs_flowenc_*
entries: the same convolution kernel with a stride, the instance norm's statistics summed in double precision by the
convolution that produces a map and applied by the one that reads it, the bottleneck's residual tail as an epilogue;
`encoder="auto"` follows tools/raft_encoder_probe.py (profiles/raft_encoder_probe.json; README). Under `encoder="fused_large"`
RAFT-large's two encoders run over the eogs_flowres_* entries: residual blocks of the same kernels, the context encoder's
eval-mode batch norms folded into their convolutions at every call (tools/raft_large_encoder_probe.py,
profiles/raft_large_encoder_probe.json; README). Under `update="fused"` RAFT-small's update block runs over the eogs_flownet_* entries of the same header:
one channel-last convolution kernel on the exact-fp32 matrix instruction with the bias, ReLU, gate and GRU-blend epilogues in
registers, the context's share of the three GRU convolutions computed once per forward and added as a plane, no torch.cat
and no layout round trip; the weights stay the torch modules' parameters and are repacked at every forward. `update="auto"`
follows the measurement of tools/raft_update_probe.py (profiles/raft_update_probe.json; README). Under `update="fused_large"`
RAFT-large's update block and mask predictor run the same way over the eogs_flowrect_* and eogs_flowlarge_*
entries of include/eogs_resample.h: the kernel over 1 x 5 and 5 x 1 taps for the two GRUs, the context's share of their six
convolutions as four planes formed once per forward, the mask head's 0.25 as an epilogue
(tools/raft_large_update_probe.py, profiles/raft_large_update_probe.json; README). The two sizes share one implementation
per role: in the library one table-driven update block and one table-driven encoder, each size a description of its widths,
taps and parameter order (csrc/flownet.hip, csrc/flowenc.hip); here `_FusedUpdate` and `_FusedEncoder`, of which FusedUpdate,
FusedUpdateLarge, FusedEncoder and FusedEncoderLarge are the tables and the checks of their module trees. Everything here is forward
only (the reference runs the network under inference_mode); the HIP operators are float32 and refuse CPU tensors (no CPU
fallback).

The module tree mirrors torchvision.models.optical_flow.raft name for name, so a torchvision state dict loads with
strict=True. torchvision is not a dependency and its checkpoints were not at hand when this was written: `TORCHVISION_NAMES`
is the one table of names, and a wrong name fails loudly at load_weights instead of leaving random weights in place.
Nothing is ever downloaded.
"""
import ctypes
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._abi import (FLOWENC_CONTEXT, FLOWENC_EPI_BIAS, FLOWENC_EPI_RELU, FLOWENC_EPI_RESIDUAL, FLOWENC_FEATURE, FLOWENC_IN_NCHW,
                   FLOWENC_OUT_NCHW, FLOWENC_PARAMS, FLOWENC_SHORTCUT_NONE, FLOWENC_SHORTCUT_NORM, FLOWENC_SHORTCUT_PLAIN,
                   FLOWRES_BN, FLOWRES_PARAMS,
                   FLOWNET_EPI_BIAS, FLOWNET_EPI_RELU, FLOWNET_MAX_KERNEL, FLOWNET_MAX_SEGMENTS, FLOWRECT_TAP_SHAPES,
                   FLOWLARGE_PARAMS, FLOWNET_UPDATE_PARAMS,
                   RAFT_MASK_CHANNELS, RAFT_MAX_LEVELS, RAFT_MAX_RADIUS, RAFT_NO_STAGE, RAFT_UP_BILINEAR, RAFT_UP_CONVEX)
from ._host import Workspaces, call, nbytes, on_device, query_bytes

_on_device = functools.partial(on_device, "raft", "the correlation lookup runs")


def _map(t, name, what, channels=None):
    if not torch.is_tensor(t):
        raise TypeError(f"raft {what}: expected a tensor for {name}, got {type(t).__name__}")
    if t.ndim != 4 or t.numel() == 0 or (channels is not None and t.shape[1] != channels):
        want = "(N, C, h, w)" if channels is None else f"(N, {channels}, h, w)"
        raise ValueError(f"raft {what}: {name} is a non-empty {want} tensor, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"raft {what}: {name} is float32, not {t.dtype}")
    return tuple(int(s) for s in t.shape)


def _levels(levels, h, w, what):
    levels = int(levels)
    if not 1 <= levels <= RAFT_MAX_LEVELS:
        raise ValueError(f"raft {what}: levels must be 1 to {RAFT_MAX_LEVELS}, got {levels}")
    if (h >> (levels - 1)) < 1 or (w >> (levels - 1)) < 1:
        raise ValueError(f"raft {what}: a ({h}, {w}) map is too small for {levels} levels (the last one would be empty)")
    return levels


class CorrPyramid:
    """The workspace `corr_pyramid` filled: `buffer` (uint8) holds level after level, channel-last. `level(l)` is a float32
    view [N, h_l, w_l, C] of one of them."""

    def __init__(self, buffer, N, C, h, w, levels):
        self.buffer, self.N, self.C, self.h, self.w, self.levels = buffer, N, C, h, w, levels

    def level(self, l):  # noqa: E741
        if not 0 <= l < self.levels:
            raise IndexError(f"raft CorrPyramid: level {l} of {self.levels}")
        off = nbytes(_lib.get(), "raft_level_offset", self.N, self.C, self.h, self.w, l)
        base = (-self.buffer.data_ptr()) % 256  # the library rounds the pointer up to 256 bytes
        hl, wl = self.h >> l, self.w >> l
        n = self.N * hl * wl * self.C
        return self.buffer[base + off: base + off + 4 * n].view(torch.float32).view(self.N, hl, wl, self.C)


def corr_pyramid(fmap, levels=4, out=None):
    """The feature pyramid of `fmap` [N, C, h, w] (NCHW, as a convolution leaves it): level l is avg_pool2d(., 2, 2) applied
    l times (floor sizes), every level channel-last. levels=1 is the channel-last copy `corr_lookup` wants of the first
    map. `out`: a CorrPyramid of the same shape to fill again instead of a new one."""
    what = "corr_pyramid"
    N, C, h, w = _map(fmap, "the feature map", what)
    if C % 4:
        raise ValueError(f"raft {what}: C must be a multiple of 4, got {C}")
    levels = _levels(levels, h, w, what)
    _on_device(fmap, what)
    x = fmap.detach()
    x = x if x.is_contiguous() else x.contiguous()
    size = nbytes(_lib.get(), "raft_bytes", N, C, h, w, levels)
    if out is None:
        out = CorrPyramid(Workspaces.bytes(x.device, size), N, C, h, w, levels)
    elif (out.N, out.C, out.h, out.w, out.levels) != (N, C, h, w, levels) or out.buffer.device != x.device:
        raise ValueError(f"raft {what}: `out` was made for another shape or device")
    call("eogs_raft_pyramid", x.device, N, C, h, w, levels, x.data_ptr(), out.buffer.data_ptr(), out.buffer.numel())
    return out


def corr_lookup(fmap1_cl, pyramid, coords, radius, no_stage=False):
    """Correlation features [N, levels (2r+1)^2, h, w] of `coords` [N, 2, h, w] (plane 0 x, plane 1 y, level-0 pixels):
    for each level the (2r+1)^2 bilinear samples, x offset slow, of <fmap1(p), fmap2_l(.)> / sqrt(C) around coords / 2^l,
    zero outside the level (include/eogs_resample.h has the statement). `fmap1_cl`: corr_pyramid(fmap1, 1); `pyramid`:
    corr_pyramid(fmap2, levels). A pixel whose coordinate is NaN or infinite gets zeros. `no_stage` forces the path that
    gathers straight from the pyramid: the same bits."""
    what = "corr_lookup"
    if not isinstance(fmap1_cl, CorrPyramid) or not isinstance(pyramid, CorrPyramid):
        raise TypeError(f"raft {what}: fmap1_cl and pyramid are what corr_pyramid returns")
    N, C, h, w = pyramid.N, pyramid.C, pyramid.h, pyramid.w
    if (fmap1_cl.N, fmap1_cl.C, fmap1_cl.h, fmap1_cl.w) != (N, C, h, w):
        raise ValueError(f"raft {what}: the two maps differ in shape, {(fmap1_cl.N, fmap1_cl.C, fmap1_cl.h, fmap1_cl.w)} and {(N, C, h, w)}")
    radius = int(radius)
    if not 1 <= radius <= RAFT_MAX_RADIUS:
        raise ValueError(f"raft {what}: radius must be 1 to {RAFT_MAX_RADIUS}, got {radius}")
    if _map(coords, "coords", what, 2) != (N, 2, h, w):
        raise ValueError(f"raft {what}: coords is {tuple(coords.shape)}, the maps ask for {(N, 2, h, w)}")
    _on_device(coords, what)
    dev = coords.device
    if fmap1_cl.buffer.device != dev or pyramid.buffer.device != dev:
        raise RuntimeError(f"raft {what}: the maps and coords live on different devices")
    c = coords.detach()
    c = c if c.is_contiguous() else c.contiguous()
    K = 2 * radius + 1
    out = torch.empty((N, pyramid.levels * K * K, h, w), dtype=torch.float32, device=dev)
    call("eogs_raft_lookup", dev, N, C, h, w, pyramid.levels, radius, fmap1_cl.buffer.data_ptr(), pyramid.buffer.data_ptr(),
         c.data_ptr(), out.data_ptr(), RAFT_NO_STAGE if no_stage else 0)
    return out


def upsample_flow(flow, mask=None):
    """`flow` [N, 2, h, w] at 1/8 resolution to [N, 2, 8h, 8w]. With `mask` [N, 576, h, w]: RAFT's learned convex
    upsampling (a softmax over 9 mask channels per output pixel weighs 8 flow over the zero-padded 3 x 3 neighbourhood);
    without: 8 * interpolate(flow, scale_factor=8, mode="bilinear", align_corners=True)."""
    what = "upsample_flow"
    N, _, h, w = _map(flow, "the flow", what, 2)
    if mask is not None and _map(mask, "the mask", what, RAFT_MASK_CHANNELS) != (N, RAFT_MASK_CHANNELS, h, w):
        raise ValueError(f"raft {what}: the mask is {tuple(mask.shape)}, the flow asks for {(N, RAFT_MASK_CHANNELS, h, w)}")
    if h > 8192 or w > 8192:
        raise ValueError(f"raft {what}: h and w at most 8192, got {(h, w)}")
    _on_device(flow, what)
    dev = flow.device
    f = flow.detach()
    f = f if f.is_contiguous() else f.contiguous()
    m = None
    if mask is not None:
        _on_device(mask, what)
        if mask.device != dev:
            raise RuntimeError(f"raft {what}: flow and mask live on different devices")
        m = mask.detach()
        m = m if m.is_contiguous() else m.contiguous()
    out = torch.empty((N, 2, 8 * h, 8 * w), dtype=torch.float32, device=dev)
    call("eogs_raft_upsample", dev, N, h, w, RAFT_UP_BILINEAR if m is None else RAFT_UP_CONVEX, f.data_ptr(),
         None if m is None else m.data_ptr(), out.data_ptr())
    return out


def stage_info():
    """(tile width, tile height, staged positions) of the lookup kernel: a workgroup stages its windows' bounding box into
    LDS when the box holds at most that many positions of the level."""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    abi = _lib.get()
    abi.check(abi.raft_stage_info(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


# ---- the update block's convolutions (eogs_flownet_*) ----

def _aligned(t):
    """`t` detached, contiguous and on a 16-byte boundary (a slice of a larger tensor may start anywhere)."""
    t = t.detach()
    t = t if t.is_contiguous() else t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _f32(t, name, what):
    if not torch.is_tensor(t):
        raise TypeError(f"raft {what}: expected a tensor for {name}, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"raft {what}: {name} is float32, not {t.dtype}")


def conv_info():
    """(tile width, tile height) of the convolution kernel: the positions of one image a workgroup owns."""
    a, b = ctypes.c_int(), ctypes.c_int()
    abi = _lib.get()
    abi.check(abi.flownet_conv_info(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def conv2d_cl(inputs, weight, bias=None, act="none", add=None):
    """conv2d(cat(inputs), weight, bias, stride 1, padding (k - 1) // 2) (+ add) (then ReLU) on CHANNEL-LAST maps: `inputs` is
    a list of one to three [N, h, w, C_i] tensors whose concatenation along the channels is never formed, `weight` torch's
    [Cout, sum C_i, k, k] with k in 1, 3, 5, 7, `bias` [Cout] or None, `add` [N, h, w, Cout] or None; returns [N, h, w, Cout].
    The weight is repacked at every call (include/eogs_resample.h has the kernel's statement and the order of its sums)."""
    return _conv2d_cl("conv2d_cl", inputs, weight, bias, act, add, rect=False)


def conv2d_rect_cl(inputs, weight, bias=None, act="none", add=None):
    """`conv2d_cl` for a weight of kh x kw taps, torch's [Cout, sum C_i, kh, kw] with (kh, kw) one of (1, 1), (3, 3), (5, 5), (7, 7),
    (1, 5), (5, 1) (RAFT-large's two GRUs are 1 x 5 and 5 x 1), padding ((kh - 1) // 2, (kw - 1) // 2): the same checks, the same
    errors, and for a square weight the same bits (include/eogs_resample.h)."""
    return _conv2d_cl("conv2d_rect_cl", inputs, weight, bias, act, add, rect=True)


def _conv2d_cl(what, inputs, weight, bias, act, add, rect):
    if not isinstance(inputs, (list, tuple)):
        raise TypeError(f"raft {what}: inputs is a list of channel-last tensors, got {type(inputs).__name__}")
    if not 1 <= len(inputs) <= FLOWNET_MAX_SEGMENTS:
        raise ValueError(f"raft {what}: one to {FLOWNET_MAX_SEGMENTS} inputs, got {len(inputs)}")
    for i, t in enumerate(inputs):
        _f32(t, f"input {i}", what)
        if t.ndim != 4 or t.numel() == 0 or t.shape[:3] != inputs[0].shape[:3]:
            raise ValueError(f"raft {what}: the inputs are non-empty (N, h, w, C_i) tensors of one (N, h, w), got {[tuple(x.shape) for x in inputs]}")
    _f32(weight, "the weight", what)
    N, h, w = (int(v) for v in inputs[0].shape[:3])
    chans = [int(t.shape[3]) for t in inputs]
    if rect:
        if weight.ndim != 4 or weight.shape[1] != sum(chans) or weight.shape[0] < 1:
            raise ValueError(f"raft {what}: the weight is (Cout, {sum(chans)}, kh, kw), got {tuple(weight.shape)}")
        if tuple(weight.shape[2:]) not in FLOWRECT_TAP_SHAPES:
            raise ValueError(f"raft {what}: the taps (kh, kw) are one of {FLOWRECT_TAP_SHAPES}, got {tuple(weight.shape[2:])}")
    elif weight.ndim != 4 or weight.shape[1] != sum(chans) or weight.shape[2] != weight.shape[3] or weight.shape[0] < 1:
        raise ValueError(f"raft {what}: the weight is (Cout, {sum(chans)}, k, k), got {tuple(weight.shape)}")
    cout, k, kw = int(weight.shape[0]), int(weight.shape[2]), int(weight.shape[3])
    if not rect and (k % 2 == 0 or k > FLOWNET_MAX_KERNEL):
        raise ValueError(f"raft {what}: the kernel size is odd and at most {FLOWNET_MAX_KERNEL}, got {k}")
    if act not in ("none", "relu"):
        raise ValueError(f"raft {what}: act is 'none' or 'relu', got {act!r}")
    if bias is not None:
        _f32(bias, "the bias", what)
        if tuple(bias.shape) != (cout,):
            raise ValueError(f"raft {what}: the bias is ({cout},), got {tuple(bias.shape)}")
    if add is not None:
        _f32(add, "add", what)
        if tuple(add.shape) != (N, h, w, cout):
            raise ValueError(f"raft {what}: add is {(N, h, w, cout)}, got {tuple(add.shape)}")
    every = list(inputs) + [weight] + [t for t in (bias, add) if t is not None]
    for t in every:
        _on_device(t, what)
    dev = inputs[0].device
    if any(t.device != dev for t in every):
        raise RuntimeError(f"raft {what}: the tensors live on different devices")
    xs = [_aligned(t) for t in inputs] + [None] * (FLOWNET_MAX_SEGMENTS - len(inputs))
    wt, b, a = _aligned(weight), None if bias is None else _aligned(bias), None if add is None else _aligned(add)
    seg = (ctypes.c_int * len(chans))(*chans)
    # (the eogs_flowrect_* entries take (kh, kw) where the eogs_flownet_conv* ones take k)
    taps, pack_bytes, pack, conv = ((k, kw), "flowrect_pack_bytes", "eogs_flowrect_pack", "eogs_flowrect_conv") if rect else \
        ((k,), "flownet_conv_pack_bytes", "eogs_flownet_conv_pack", "eogs_flownet_conv")
    size = query_bytes(_lib.get(), pack_bytes, *taps, len(chans), seg, cout)
    packed = Workspaces.bytes(dev, size)
    call(pack, dev, *taps, len(chans), seg, None, sum(chans), cout, 0, cout, wt.data_ptr(), packed.data_ptr(), size)
    out = torch.empty((N, h, w, cout), dtype=torch.float32, device=dev)
    call(conv, dev, N, h, w, *taps, len(chans), seg, *(None if x is None else x.data_ptr() for x in xs), cout,
         packed.data_ptr(), size, None if b is None else b.data_ptr(), None if a is None else a.data_ptr(), None, out.data_ptr(),
         FLOWNET_EPI_RELU if act == "relu" else FLOWNET_EPI_BIAS, 0)
    return out


class _FusedUpdate:
    """What FusedUpdate and FusedUpdateLarge share: the parameter table, `begin`, `step`, `hidden`, the workspaces and the
    pickling, driven by the subclass's tables. NAMES and SHAPES: the convolutions in the order of the entries' params table
    (PARAMS pointers: each one's weight, then its bias); HIDDEN, CONTEXT, CORR: the channels of the three inputs; ENTRIES: the
    library's entries are eogs_<ENTRIES>_{bytes, hidden_offset, begin, step}. A constructor checks its module tree and hands
    the convolutions to `_hold`. The messages carry the subclass's own name."""

    NAMES = SHAPES = ()
    HIDDEN = CONTEXT = CORR = PARAMS = 0
    ENTRIES = ""

    def _hold(self, names, convs):
        self._names, self._convs, self._ws, self._state = tuple(names), convs, Workspaces(), None

    def __getstate__(self):  # a copied or pickled module starts without workspaces
        return {"_names": self._names, "_convs": self._convs}

    def __setstate__(self, state):
        self._hold(state["_names"], state["_convs"])

    def _params(self, dev):
        out = []
        for name, c in zip(self._names, self._convs):
            for p in (c.weight, c.bias):
                if p.dtype != torch.float32 or p.device != dev:
                    raise RuntimeError(f"raft {type(self).__name__}: {name} is {p.dtype} on {p.device}; the fused update runs in float32 on "
                                       f"the inputs' device ({dev}), there is no CPU fallback")
                out.append(_aligned(p))
        return out

    @classmethod
    def workspace_bytes(cls, N, h, w):
        return nbytes(_lib.get(), f"{cls.ENTRIES}_bytes", int(N), int(h), int(w))

    def begin(self, hidden_state, context):
        what = f"{type(self).__name__}.begin"
        N, _, h, w = _map(hidden_state, "the hidden state", what, self.HIDDEN)
        if _map(context, "the context", what, self.CONTEXT) != (N, self.CONTEXT, h, w):
            raise ValueError(f"raft {what}: the context is {tuple(context.shape)}, the hidden state asks for {(N, self.CONTEXT, h, w)}")
        _on_device(hidden_state, what)
        _on_device(context, what)
        dev = hidden_state.device
        if context.device != dev:
            raise RuntimeError(f"raft {what}: the hidden state and the context live on different devices")
        params = self._params(dev)
        assert len(params) == self.PARAMS
        size = self.workspace_bytes(N, h, w)
        ws = self._ws.of((N, h, w), dev, lambda: Workspaces.bytes(dev, size))
        hid, ctx = _aligned(hidden_state), _aligned(context)
        table = (ctypes.c_void_p * len(params))(*(p.data_ptr() for p in params))
        call(f"eogs_{self.ENTRIES}_begin", dev, N, h, w, table, hid.data_ptr(), ctx.data_ptr(), ws.data_ptr(), ws.numel())
        self._state = (N, h, w, ws)

    def _begun(self, what):
        if self._state is None:
            raise RuntimeError(f"raft {type(self).__name__}.{what}: begin(hidden_state, context) comes first")
        return self._state

    def step(self, corr_features, flow):
        N, h, w, ws = self._begun("step")
        what = f"{type(self).__name__}.step"
        if _map(corr_features, "the correlation features", what, self.CORR) != (N, self.CORR, h, w) or _map(flow, "the flow", what, 2) != (N, 2, h, w):
            raise ValueError(f"raft {what}: begin was given {(N, h, w)}; the correlation features are {tuple(corr_features.shape)}, "
                             f"the flow is {tuple(flow.shape)}")
        _on_device(corr_features, what)
        _on_device(flow, what)
        if corr_features.device != ws.device or flow.device != ws.device:
            raise RuntimeError(f"raft {what}: the tensors and the workspace live on different devices")
        corr, fl = _aligned(corr_features), _aligned(flow)
        delta = torch.empty((N, 2, h, w), dtype=torch.float32, device=ws.device)
        call(f"eogs_{self.ENTRIES}_step", ws.device, N, h, w, corr.data_ptr(), fl.data_ptr(), ws.data_ptr(), ws.numel(), delta.data_ptr())
        return delta

    def hidden(self):
        N, h, w, ws = self._begun("hidden")
        off = nbytes(_lib.get(), f"{self.ENTRIES}_hidden_offset", N, h, w)
        base = (-ws.data_ptr()) % 256  # the library rounds the pointer up to 256 bytes
        cl = ws[base + off: base + off + 4 * N * h * w * self.HIDDEN].view(torch.float32).view(N, h, w, self.HIDDEN)
        return cl.permute(0, 3, 1, 2).contiguous()


class FusedUpdate(_FusedUpdate):
    """RAFT-small's `UpdateBlock` over the convolution kernel, with the call order of UpdateBlock.forward split in two:

        fused.begin(hidden_state, context)         once per forward: the NCHW halves of the context encoder after tanh / relu
        delta = fused.step(corr_features, flow)    once per update: [N, 2, h, w]; the hidden state advances in the workspace
        fused.hidden()                             the hidden state as [N, 96, h, w]

    It holds the block, not a copy of its weights: `begin` repacks them at every forward, so edited or reloaded weights can
    never go stale. It is no nn.Module and registers no parameter and no buffer. Float32 on the GPU, forward only."""

    NAMES = ("motion_encoder.convcorr1.0", "motion_encoder.convflow1.0", "motion_encoder.convflow2.0", "motion_encoder.conv.0",
             "recurrent_block.convgru1.convz", "recurrent_block.convgru1.convr", "recurrent_block.convgru1.convq",
             "flow_head.conv1", "flow_head.conv2")
    SHAPES = ((96, 196, 1, 1), (64, 2, 7, 7), (32, 64, 3, 3), (80, 128, 3, 3), (96, 242, 3, 3), (96, 242, 3, 3), (96, 242, 3, 3),
              (128, 96, 3, 3), (2, 128, 3, 3))
    HIDDEN, CONTEXT, CORR, PARAMS = 96, 64, 196, FLOWNET_UPDATE_PARAMS
    ENTRIES = "flownet_update"

    def __init__(self, update_block):
        if not isinstance(update_block, UpdateBlock):
            raise TypeError(f"raft FusedUpdate: expected an UpdateBlock, got {type(update_block).__name__}")
        convs = [update_block.get_submodule(n) for n in self.NAMES]
        got = tuple(tuple(c.weight.shape) for c in convs)
        if got != self.SHAPES or not isinstance(update_block.motion_encoder.convcorr2, nn.Identity) or \
                not isinstance(update_block.recurrent_block.convgru2, nn.Identity):
            raise ValueError("raft FusedUpdate: the fused update is RAFT-small's (one 1 x 1 correlation convolution, one 3 x 3 GRU); "
                             f"this block's convolutions are {got}")
        self._hold(self.NAMES, convs)


class FusedUpdateLarge(_FusedUpdate):
    """RAFT-large's `UpdateBlock` and `MaskPredictor` over the convolution kernel (the eogs_flowlarge_* entries of
    include/eogs_resample.h), with FusedUpdate's call order and one more call:

        fused.begin(hidden_state, context)         once per forward: the NCHW halves of the context encoder after tanh / relu
        delta = fused.step(corr_features, flow)    once per update: [N, 2, h, w]; the hidden state advances in the workspace
        mask = fused.mask()                        [N, 576, h, w] of the hidden state as it is now: what upsample_flow takes
        fused.hidden()                             the hidden state as [N, 128, h, w]

    It holds the two modules, not copies of their weights: `begin` repacks them at every forward. It is no nn.Module and
    registers no parameter and no buffer. Float32 on the GPU, forward only."""

    NAMES = ("motion_encoder.convcorr1.0", "motion_encoder.convcorr2.0", "motion_encoder.convflow1.0", "motion_encoder.convflow2.0",
             "motion_encoder.conv.0", "recurrent_block.convgru1.convz", "recurrent_block.convgru1.convr", "recurrent_block.convgru1.convq",
             "recurrent_block.convgru2.convz", "recurrent_block.convgru2.convr", "recurrent_block.convgru2.convq", "flow_head.conv1",
             "flow_head.conv2")
    MASK_NAMES = ("convrelu.0", "conv")
    SHAPES = ((256, 324, 1, 1), (192, 256, 3, 3), (128, 2, 7, 7), (64, 128, 3, 3), (126, 256, 3, 3), (128, 384, 1, 5), (128, 384, 1, 5),
              (128, 384, 1, 5), (128, 384, 5, 1), (128, 384, 5, 1), (128, 384, 5, 1), (256, 128, 3, 3), (2, 256, 3, 3),
              (256, 128, 3, 3), (RAFT_MASK_CHANNELS, 256, 1, 1))
    HIDDEN, CONTEXT, CORR, PARAMS = 128, 128, 324, FLOWLARGE_PARAMS
    ENTRIES = "flowlarge"

    def __init__(self, update_block, mask_predictor):
        what = "raft FusedUpdateLarge"
        if not isinstance(update_block, UpdateBlock):
            raise TypeError(f"{what}: expected an UpdateBlock, got {type(update_block).__name__}")
        if not isinstance(mask_predictor, MaskPredictor):
            raise TypeError(f"{what}: expected a MaskPredictor, got {type(mask_predictor).__name__}")
        if not isinstance(update_block.motion_encoder.convcorr2, nn.Sequential) or not isinstance(update_block.recurrent_block.convgru2, ConvGRU):
            raise ValueError(f"{what}: the fused update is RAFT-large's (two correlation convolutions, a 1 x 5 and a 5 x 1 GRU); this "
                             "block has one of them only")
        convs = [update_block.get_submodule(n) for n in self.NAMES] + [mask_predictor.get_submodule(n) for n in self.MASK_NAMES]
        got = tuple(tuple(c.weight.shape) for c in convs)
        if got != self.SHAPES or mask_predictor.multiplier != 0.25:
            raise ValueError(f"{what}: the fused update is RAFT-large's (two correlation convolutions, a 1 x 5 and a 5 x 1 GRU, a mask "
                             f"predictor with the multiplier 0.25); this block's convolutions are {got}, the multiplier {mask_predictor.multiplier}")
        self._hold(tuple(f"update_block.{n}" for n in self.NAMES) + tuple(f"mask_predictor.{n}" for n in self.MASK_NAMES), convs)

    def mask(self):
        N, h, w, ws = self._begun("mask")
        out = torch.empty((N, RAFT_MASK_CHANNELS, h, w), dtype=torch.float32, device=ws.device)
        call("eogs_flowlarge_mask", ws.device, N, h, w, ws.data_ptr(), ws.numel(), out.data_ptr())
        return out


# ---- the encoders' convolutions (eogs_flowenc_*) ----

def conv2d_strided_cl(input, weight, bias=None, stride=1, act="none", in_norm=None, res=None, stats=False, in_nchw=False,
                      out_nchw=False):
    """conv2d(x, weight, bias, stride 1 or 2, padding (k - 1) // 2) of ONE map, k in 1, 3, 7: `input` [N, h, w, Cin]
    (channel-last; [N, Cin, h, w] with in_nchw), `weight` torch's [Cout, Cin, k, k], `bias` [Cout] or None. With `in_norm`
    [N, Cin, 2] = (mean, rstd), x = max((input - mean) * rstd, 0), else x = input. act "none" or "relu"; with `res`
    [N, h', w', Cout] (act must be "relu") the result is relu(res + relu(v)). Returns [N, h', w', Cout] ([N, Cout, h', w'] with
    out_nchw, act "none" only), h' = ceil(h / stride). stats=True (act "none" only) returns (out, norm): norm [N, Cout, 2] is
    (mean, rstd) of the stored map per image and channel (include/eogs_resample.h has the statement)."""
    what = "conv2d_strided_cl"
    _f32(input, "the input", what)
    _f32(weight, "the weight", what)
    if input.ndim != 4 or input.numel() == 0:
        raise ValueError(f"raft {what}: the input is a non-empty 4-d tensor, got {tuple(input.shape)}")
    N, h, w, cin = (int(v) for v in (input.shape if not in_nchw else (input.shape[0], input.shape[2], input.shape[3], input.shape[1])))
    if weight.ndim != 4 or weight.shape[1] != cin or weight.shape[2] != weight.shape[3] or weight.shape[0] < 1:
        raise ValueError(f"raft {what}: the weight is (Cout, {cin}, k, k), got {tuple(weight.shape)}")
    cout, k = int(weight.shape[0]), int(weight.shape[2])
    if k not in (1, 3, 7):
        raise ValueError(f"raft {what}: the kernel size is 1, 3 or 7, got {k}")
    if stride not in (1, 2):
        raise ValueError(f"raft {what}: the stride is 1 or 2, got {stride!r}")
    if act not in ("none", "relu"):
        raise ValueError(f"raft {what}: act is 'none' or 'relu', got {act!r}")
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    if bias is not None:
        _f32(bias, "the bias", what)
        if tuple(bias.shape) != (cout,):
            raise ValueError(f"raft {what}: the bias is ({cout},), got {tuple(bias.shape)}")
    if in_norm is not None:
        _f32(in_norm, "in_norm", what)
        if tuple(in_norm.shape) != (N, cin, 2):
            raise ValueError(f"raft {what}: in_norm is {(N, cin, 2)}, got {tuple(in_norm.shape)}")
    if res is not None:
        _f32(res, "res", what)
        if tuple(res.shape) != (N, ho, wo, cout):
            raise ValueError(f"raft {what}: res is {(N, ho, wo, cout)}, got {tuple(res.shape)}")
        if act != "relu":
            raise ValueError(f"raft {what}: res closes a block as relu(res + relu(v)): act must be 'relu'")
    if (stats or out_nchw) and act != "none":
        raise ValueError(f"raft {what}: stats and out_nchw go with act='none' only")
    every = [input, weight] + [t for t in (bias, in_norm, res) if t is not None]
    for t in every:
        _on_device(t, what)
    dev = input.device
    if any(t.device != dev for t in every):
        raise RuntimeError(f"raft {what}: the tensors live on different devices")
    x, wt = _aligned(input), _aligned(weight)
    b, tn, r = (None if t is None else _aligned(t) for t in (bias, in_norm, res))
    seg = (ctypes.c_int * 1)(cin)
    size = query_bytes(_lib.get(), "flownet_conv_pack_bytes", k, 1, seg, cout)
    packed = Workspaces.bytes(dev, size)
    call("eogs_flownet_conv_pack", dev, k, 1, seg, None, cin, cout, 0, cout, wt.data_ptr(), packed.data_ptr(), size)
    out = torch.empty((N, cout, ho, wo) if out_nchw else (N, ho, wo, cout), dtype=torch.float32, device=dev)
    partials, pbytes = None, 0
    if stats:
        rows, nb = ctypes.c_int(), ctypes.c_size_t()
        abi = _lib.get()
        abi.check(abi.flowenc_conv_partials(N, ho, wo, cout, ctypes.byref(rows), ctypes.byref(nb)))
        pbytes = nb.value
        partials = torch.empty(pbytes // 8, dtype=torch.float64, device=dev)
    epi = FLOWENC_EPI_RESIDUAL if res is not None else FLOWENC_EPI_RELU if act == "relu" else FLOWENC_EPI_BIAS
    opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    call("eogs_flowenc_conv", dev, N, h, w, cin, cout, k, stride, x.data_ptr(), opt(tn), packed.data_ptr(), size, opt(b), opt(r),
         out.data_ptr(), opt(partials), pbytes, epi, (FLOWENC_IN_NCHW if in_nchw else 0) | (FLOWENC_OUT_NCHW if out_nchw else 0))
    if not stats:
        return out
    norm = torch.empty((N, cout, 2), dtype=torch.float32, device=dev)
    call("eogs_flowenc_norm", dev, N, ho, wo, cout, partials.data_ptr(), pbytes, norm.data_ptr())
    return out, norm


def finish_cl(v, norm_v, s=None, norm_s=None):
    """relu(S + relu((v - mean_v) * rstd_v)) on channel-last maps [N, h, w, C], C a multiple of 4, with norm_v [N, C, 2] =
    (mean, rstd): S = 0 without `s` (the stem: relu of the normalised map), S = s with `s` alone (a block's input), S =
    (s - mean_s) * rstd_s with `norm_s` too (the normalised downsample)."""
    what = "finish_cl"
    _f32(v, "v", what)
    _f32(norm_v, "norm_v", what)
    if v.ndim != 4 or v.numel() == 0 or v.shape[3] % 4:
        raise ValueError(f"raft {what}: v is a non-empty (N, h, w, C) tensor with C a multiple of 4, got {tuple(v.shape)}")
    N, h, w, C = (int(x) for x in v.shape)
    if tuple(norm_v.shape) != (N, C, 2):
        raise ValueError(f"raft {what}: norm_v is {(N, C, 2)}, got {tuple(norm_v.shape)}")
    if norm_s is not None and s is None:
        raise ValueError(f"raft {what}: norm_s normalises s, which is missing")
    if s is not None:
        _f32(s, "s", what)
        if s.shape != v.shape:
            raise ValueError(f"raft {what}: s is {tuple(v.shape)}, got {tuple(s.shape)}")
    if norm_s is not None:
        _f32(norm_s, "norm_s", what)
        if tuple(norm_s.shape) != (N, C, 2):
            raise ValueError(f"raft {what}: norm_s is {(N, C, 2)}, got {tuple(norm_s.shape)}")
    every = [v, norm_v] + [t for t in (s, norm_s) if t is not None]
    for t in every:
        _on_device(t, what)
    dev = v.device
    if any(t.device != dev for t in every):
        raise RuntimeError(f"raft {what}: the tensors live on different devices")
    a, ta = _aligned(v), _aligned(norm_v)
    b, tb = (None if t is None else _aligned(t) for t in (s, norm_s))
    out = torch.empty_like(a)
    mode = FLOWENC_SHORTCUT_NONE if s is None else FLOWENC_SHORTCUT_PLAIN if norm_s is None else FLOWENC_SHORTCUT_NORM
    call("eogs_flowenc_finish", dev, N, h, w, C, a.data_ptr(), ta.data_ptr(), None if b is None else b.data_ptr(),
         None if tb is None else tb.data_ptr(), mode, out.data_ptr())
    return out


class _FusedEncoder:
    """What FusedEncoder and FusedEncoderLarge share: the call, the parameter table, the workspaces and their eviction, the
    pickling. ENTRIES: the library's entries are eogs_<ENTRIES>_{bytes, run}. A constructor checks its module tree and sets
    `_names` and `_convs` (the convolutions in the order of the entry's params table), `kind`, `channels` (of the result) and
    `_ws`. The messages carry the subclass's own name."""

    MAX_WORKSPACES = 2
    ENTRIES = ""

    def __getstate__(self):  # a copied or pickled module starts without workspaces
        return {k: v for k, v in self.__dict__.items() if k != "_ws"}

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._ws = Workspaces()

    def _checked(self, name, p, dev):
        if p.dtype != torch.float32 or p.device != dev:
            raise RuntimeError(f"raft {type(self).__name__}: {name} is {p.dtype} on {p.device}; the fused encoder runs in float32 on "
                               f"the image's device ({dev}), there is no CPU fallback")
        return _aligned(p)

    def _tables(self, dev):
        """The tensors behind each pointer table the run entry takes after the kind (None: a NULL table)."""
        return [[self._checked(name, p, dev) for name, c in zip(self._names, self._convs) for p in (c.weight, c.bias)]]

    def workspace_bytes(self, N, H, W):
        return nbytes(_lib.get(), f"{self.ENTRIES}_bytes", int(N), int(H), int(W), self.kind)

    def __call__(self, image):
        what = type(self).__name__
        N, _, H, W = _map(image, "the image", what, 3)
        _on_device(image, what)
        dev = image.device
        tensors = self._tables(dev)
        size = self.workspace_bytes(N, H, W)
        ws = self._ws.of((N, H, W), dev, lambda: Workspaces.bytes(dev, size))
        while len(self._ws) > self.MAX_WORKSPACES:  # (the allocator frees in stream order: a launch in flight keeps its memory)
            del self._ws[next(k for k, v in self._ws.items() if v is not ws)]
        x = _aligned(image)
        h, w = H, W
        for _ in range(3):
            h, w = (h + 1) // 2, (w + 1) // 2
        out = torch.empty((N, self.channels, h, w), dtype=torch.float32, device=dev)
        tables = [None if t is None else (ctypes.c_void_p * len(t))(*(p.data_ptr() for p in t)) for t in tensors]
        call(f"eogs_{self.ENTRIES}_run", dev, N, H, W, self.kind, *tables, x.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr())
        return out


class FusedEncoder(_FusedEncoder):
    """One of RAFT-small's two encoders (a `FeatureEncoder` of bottleneck blocks, widths 32, 32, 64, 96, with InstanceNorm2d and
    a 128-channel head, or without a norm and a 160-channel head) as one call: `fused(image [N, 3, H, W]) -> [N, C, h, w]`,
    what the module's forward returns. It holds the module, not a copy of its weights: they are repacked at every call, so
    edited or reloaded weights can never go stale. It is no nn.Module and registers nothing. It keeps its workspace between
    calls, one per (device, stream, image shape) and at most MAX_WORKSPACES of them: a workspace is 144 MB (feature) or 109 MB
    (context, which has no norm tables to keep) per image at 1024^2 and 575 or 437 MB at 2048^2, so a caller whose image sizes vary must not collect one per size; the one least recently made is
    dropped. Float32 on the GPU, forward only."""

    WIDTHS = (32, 32, 64, 96)
    ENTRIES = "flowenc"

    def __init__(self, encoder_module):
        what = "raft FusedEncoder"
        if not isinstance(encoder_module, FeatureEncoder):
            raise TypeError(f"{what}: expected a FeatureEncoder, got {type(encoder_module).__name__}")
        names, shapes = ["convnormrelu.0"], [(32, 3, 7, 7)]
        for L in (1, 2, 3):
            for B in (0, 1):
                block = getattr(encoder_module, f"layer{L}")[B]
                if not isinstance(block, BottleneckBlock):
                    raise ValueError(f"{what}: the fused encoders are RAFT-small's, of bottleneck blocks; layer{L}.{B} is a {type(block).__name__}")
                cin, cout = self.WIDTHS[L - 1] if B == 0 else self.WIDTHS[L], self.WIDTHS[L]
                names += [f"layer{L}.{B}.convnormrelu{i}.0" for i in (1, 2, 3)]
                shapes += [(cout // 4, cin, 1, 1), (cout // 4, cout // 4, 3, 3), (cout, cout // 4, 1, 1)]
                if B == 0 and L > 1:
                    if isinstance(block.downsample, nn.Identity):
                        raise ValueError(f"{what}: layer{L}.0 has no downsample; RAFT-small's halves the map there")
                    names.append(f"layer{L}.{B}.downsample.0")
                    shapes.append((cout, cin, 1, 1))
                elif not isinstance(block.downsample, nn.Identity):
                    raise ValueError(f"{what}: layer{L}.{B} has a downsample; RAFT-small's has none there")
        names.append("conv")
        convs = [encoder_module.get_submodule(n) for n in names]
        norms = []
        for n in names[:-1]:
            unit = encoder_module.get_submodule(n.rsplit(".", 1)[0])
            norms += [(n, m) for m in list(unit)[1:] if not isinstance(m, nn.ReLU)]
        normed = bool(norms)
        for n, m in norms:
            if not isinstance(m, nn.InstanceNorm2d) or m.affine or m.track_running_stats or m.eps != 1e-5:
                raise ValueError(f"{what}: the norm is InstanceNorm2d without affine and running statistics, eps 1e-5, or none; "
                                 f"{n.rsplit('.', 1)[0]} has {m}")
        if normed and len(norms) != len(names) - 1:
            raise ValueError(f"{what}: a norm after every convolution but the head, or none; {len(norms)} of {len(names) - 1} have one")
        shapes.append((128 if normed else 160, 96, 1, 1))
        got = tuple(tuple(c.weight.shape) for c in convs)
        strides = tuple(c.stride[0] for c in convs)
        want_strides = tuple(2 if n in ("convnormrelu.0", "layer2.0.convnormrelu2.0", "layer3.0.convnormrelu2.0", "layer2.0.downsample.0",
                                        "layer3.0.downsample.0") else 1 for n in names)
        if got != tuple(shapes) or strides != want_strides or any(c.bias is None for c in convs):
            raise ValueError(f"{what}: the fused encoders are RAFT-small's (widths 32, 32, 64, 96, a head of 128 with the norm and of "
                             f"160 without); this encoder's convolutions are {got} with strides {strides}")
        assert 2 * len(convs) == FLOWENC_PARAMS
        self._names, self._convs, self.kind, self.channels = tuple(names), convs, FLOWENC_FEATURE if normed else FLOWENC_CONTEXT, shapes[-1][0]
        self._ws = Workspaces()


# ---- RAFT-large's encoders (eogs_flowres_*) ----

def fold_batchnorm(weight, bias, gamma, beta, mean, var, eps=1e-5):
    """A BatchNorm2d in eval mode folded into the convolution before it: `weight` [Cout, Cin, k, k], `bias`, `gamma`, `beta`,
    the running `mean` and `var` [Cout]; returns (w', b') with s = float(gamma / sqrt(double(var) + eps)), w' = weight * s in
    float32 and b' = float((double(bias) - mean) * s + beta), so that conv(x, w', b') is norm(conv(x, weight, bias))
    (include/eogs_resample.h has the statement). Nothing is read back: a NaN stays a NaN, a negative var gives NaN."""
    what = "fold_batchnorm"
    _f32(weight, "the weight", what)
    if weight.ndim != 4 or weight.numel() == 0:
        raise ValueError(f"raft {what}: the weight is a non-empty (Cout, Cin, kh, kw) tensor, got {tuple(weight.shape)}")
    cout = int(weight.shape[0])
    vectors = (("the bias", bias), ("gamma", gamma), ("beta", beta), ("mean", mean), ("var", var))
    for name, t in vectors:
        _f32(t, name, what)
        if tuple(t.shape) != (cout,):
            raise ValueError(f"raft {what}: {name} is ({cout},), got {tuple(t.shape)}")
    eps = float(eps)
    if not 0.0 <= eps < math.inf:
        raise ValueError(f"raft {what}: eps is a finite number of at least 0, got {eps!r}")
    every = [weight] + [t for _, t in vectors]
    for t in every:
        _on_device(t, what)
    dev = weight.device
    if any(t.device != dev for t in every):
        raise RuntimeError(f"raft {what}: the tensors live on different devices")
    wt, b, g, be, m, v = (_aligned(t) for t in every)
    w_out, b_out = torch.empty_like(wt), torch.empty_like(b)
    call("eogs_flowres_fold", dev, cout, wt.numel() // cout, wt.data_ptr(), b.data_ptr(), g.data_ptr(), be.data_ptr(), m.data_ptr(),
         v.data_ptr(), eps, w_out.data_ptr(), b_out.data_ptr())
    return w_out, b_out


class FusedEncoderLarge(_FusedEncoder):
    """One of RAFT-large's two encoders (a `FeatureEncoder` of residual blocks, widths 64, 64, 96, 128, a 256-channel head, with
    InstanceNorm2d or with BatchNorm2d in eval mode) as one call: `fused(image [N, 3, H, W]) -> [N, 256, h, w]`, what the
    module's forward returns. It holds the module, not copies: weights, biases and the batch norms' parameters and running
    statistics are read at every call (the batch norms are folded and the weights repacked there), so they never go stale.
    A batch norm in training mode raises: batch statistics are not what this computes. It is no nn.Module and registers
    nothing. It keeps its workspace between calls, one per (device, stream, image shape) and at most MAX_WORKSPACES of them:
    a workspace is 302 MB (feature) or 236 MB (context) per image at 1024^2 and 1189 or 916 MB at 2048^2 (eogs_flowres_bytes;
    the feature encoder of a forward takes two images); the one least recently made is dropped. Float32 on the GPU, forward
    only."""

    WIDTHS = (64, 64, 96, 128)
    HEAD = 256
    ENTRIES = "flowres"

    def __init__(self, encoder_module):
        what = "raft FusedEncoderLarge"
        if not isinstance(encoder_module, FeatureEncoder):
            raise TypeError(f"{what}: expected a FeatureEncoder, got {type(encoder_module).__name__}")
        names, shapes, strides = ["convnormrelu.0"], [(64, 3, 7, 7)], [2]
        for L in (1, 2, 3):
            for B in (0, 1):
                block = getattr(encoder_module, f"layer{L}")[B]
                if not isinstance(block, ResidualBlock):
                    raise ValueError(f"{what}: the fused encoders are RAFT-large's, of residual blocks; layer{L}.{B} is a {type(block).__name__}")
                cin, cout = self.WIDTHS[L - 1] if B == 0 else self.WIDTHS[L], self.WIDTHS[L]
                down = B == 0 and L > 1
                names += [f"layer{L}.{B}.convnormrelu1.0", f"layer{L}.{B}.convnormrelu2.0"]
                shapes += [(cout, cin, 3, 3), (cout, cout, 3, 3)]
                strides += [2 if down else 1, 1]
                if down:
                    if isinstance(block.downsample, nn.Identity):
                        raise ValueError(f"{what}: layer{L}.0 has no downsample; RAFT-large's halves the map there")
                    names.append(f"layer{L}.{B}.downsample.0")
                    shapes.append((cout, cin, 1, 1))
                    strides.append(2)
                elif not isinstance(block.downsample, nn.Identity):
                    raise ValueError(f"{what}: layer{L}.{B} has a downsample; RAFT-large's has none there")
        names.append("conv")
        shapes.append((self.HEAD, self.WIDTHS[3], 1, 1))
        strides.append(1)
        convs = [encoder_module.get_submodule(n) for n in names]
        norms = []
        for n in names[:-1]:
            unit = n.rsplit(".", 1)[0]
            found = [m for m in list(encoder_module.get_submodule(unit))[1:] if not isinstance(m, nn.ReLU)]
            if len(found) != 1:
                raise ValueError(f"{what}: one norm after every convolution but the head; {unit} has {found if found else 'none'}")
            norms.append(found[0])
        instance = isinstance(norms[0], nn.InstanceNorm2d)
        for n, m in zip(names, norms):
            if instance:
                ok = isinstance(m, nn.InstanceNorm2d) and not m.affine and not m.track_running_stats
            else:
                ok = type(m) is nn.BatchNorm2d and m.affine and m.track_running_stats
            if not ok or m.eps != 1e-5:
                raise ValueError(f"{what}: the norm is InstanceNorm2d without affine and running statistics or BatchNorm2d with both, "
                                 f"eps 1e-5, the same kind throughout; {n.rsplit('.', 1)[0]} has {m}")
        got = tuple(tuple(c.weight.shape) for c in convs)
        got_strides = tuple(c.stride[0] for c in convs)
        if got != tuple(shapes) or got_strides != tuple(strides) or any(c.bias is None for c in convs):
            raise ValueError(f"{what}: the fused encoders are RAFT-large's (widths 64, 64, 96, 128, a head of 256); this encoder's "
                             f"convolutions are {got} with strides {got_strides}")
        assert 2 * len(convs) == FLOWRES_PARAMS and 4 * len(norms) == FLOWRES_BN
        self._names, self._convs, self._norms = tuple(names), convs, None if instance else norms
        self.kind, self.channels = FLOWENC_FEATURE if instance else FLOWENC_CONTEXT, self.HEAD
        self._ws = Workspaces()

    def _tables(self, dev):  # (the batch norms first: a training-mode one is refused before anything else)
        bn = self._bn(dev)
        return super()._tables(dev) + [bn]

    def _bn(self, dev):
        if self._norms is None:
            return None
        out = []
        for name, m in zip(self._names, self._norms):
            unit = name.rsplit(".", 1)[0] + ".1"
            if m.training:
                raise RuntimeError(f"raft FusedEncoderLarge: {unit} is in training mode; the fused encoder folds the running statistics "
                                   "(eval mode), batch statistics are not what it computes")
            out += [self._checked(unit, p, dev) for p in (m.weight, m.bias, m.running_mean, m.running_var)]
        return out


# ---- the materialised form, in plain torch: any dtype, any device ----

def volume_pyramid(fmap1, fmap2, levels):
    """[N h w, 1, h_l, w_l] for l < levels: the all-pairs correlation / sqrt(C), average-pooled over the second map."""
    N, C, h, w = fmap1.shape
    corr = torch.matmul(fmap1.reshape(N, C, h * w).transpose(1, 2), fmap2.reshape(N, C, h * w)) / math.sqrt(C)
    corr = corr.reshape(N * h * w, 1, h, w)
    pyramid = [corr]
    for _ in range(levels - 1):
        corr = F.avg_pool2d(corr, kernel_size=2, stride=2)
        pyramid.append(corr)
    return pyramid


def volume_lookup(pyramid, coords, radius):
    """torchvision's CorrBlock.index_pyramid: grid_sample(bilinear, align_corners=True, zeros) of each level at
    coords / 2^l + (d_i, d_j), the offsets from meshgrid(d, d, indexing="ij") stacked onto (x, y): i offsets x."""
    N, _, h, w = coords.shape
    K = 2 * radius + 1
    d = torch.linspace(-radius, radius, K, dtype=coords.dtype, device=coords.device)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, K, K, 2)
    c = coords.permute(0, 2, 3, 1).reshape(N * h * w, 1, 1, 2)
    out = []
    for corr in pyramid:
        hl, wl = corr.shape[-2:]
        s = c + delta
        if hl < 2 or wl < 2:
            raise ValueError(f"raft volume_lookup: a level of {(hl, wl)} has no extent to normalise grid_sample's coordinates by")
        grid = torch.stack([2 * s[..., 0] / (wl - 1) - 1, 2 * s[..., 1] / (hl - 1) - 1], dim=-1)
        out.append(F.grid_sample(corr, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(N, h, w, K * K))
        c = c / 2
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()


def convex_upsample_torch(flow, mask):
    """The unfold / softmax / permute statement of the convex upsampling, any dtype."""
    N, _, h, w = flow.shape
    m = torch.softmax(mask.view(N, 1, 9, 8, 8, h, w), dim=2)
    u = F.unfold(8 * flow, kernel_size=3, padding=1).view(N, 2, 9, 1, 1, h, w)
    return torch.sum(m * u, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * h, 8 * w)


def _upsample_torch(flow, mask):
    if mask is not None:
        return convex_upsample_torch(flow, mask)
    return 8 * F.interpolate(flow, size=(8 * flow.shape[2], 8 * flow.shape[3]), mode="bilinear", align_corners=True)


# ---- the network: torchvision.models.optical_flow.raft, name for name ----

def _cna(cin, cout, norm, kernel_size, stride=1, act=True):
    """torchvision's Conv2dNormActivation: Sequential(conv [0], norm [1] if any, ReLU), padding (k - 1) // 2, bias=True."""
    layers = [nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=(kernel_size - 1) // 2, bias=True)]
    if norm is not None:
        layers.append(norm(cout))
    if act:
        layers.append(nn.ReLU(inplace=True))
    return nn.Sequential(*layers)


class ResidualBlock(nn.Module):
    def __init__(self, cin, cout, norm, stride=1):
        super().__init__()
        self.convnormrelu1 = _cna(cin, cout, norm, 3, stride)
        self.convnormrelu2 = _cna(cout, cout, norm, 3)
        self.downsample = nn.Identity() if stride == 1 else _cna(cin, cout, norm, 1, stride, act=False)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        y = self.convnormrelu2(self.convnormrelu1(x))
        return self.relu(self.downsample(x) + y)


class BottleneckBlock(nn.Module):
    def __init__(self, cin, cout, norm, stride=1):
        super().__init__()
        self.convnormrelu1 = _cna(cin, cout // 4, norm, 1)
        self.convnormrelu2 = _cna(cout // 4, cout // 4, norm, 3, stride)
        self.convnormrelu3 = _cna(cout // 4, cout, norm, 1)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = nn.Identity() if stride == 1 else _cna(cin, cout, norm, 1, stride, act=False)

    def forward(self, x):
        y = self.convnormrelu3(self.convnormrelu2(self.convnormrelu1(x)))
        return self.relu(self.downsample(x) + y)


class FeatureEncoder(nn.Module):
    def __init__(self, block, layers, norm):
        super().__init__()
        self.convnormrelu = _cna(3, layers[0], norm, 7, 2)
        self.layer1 = nn.Sequential(block(layers[0], layers[1], norm, 1), block(layers[1], layers[1], norm, 1))
        self.layer2 = nn.Sequential(block(layers[1], layers[2], norm, 2), block(layers[2], layers[2], norm, 1))
        self.layer3 = nn.Sequential(block(layers[2], layers[3], norm, 2), block(layers[3], layers[3], norm, 1))
        self.conv = nn.Conv2d(layers[3], layers[4], kernel_size=1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d)) and m.weight is not None:
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        return self.conv(self.layer3(self.layer2(self.layer1(self.convnormrelu(x)))))


class MotionEncoder(nn.Module):
    def __init__(self, in_channels_corr, corr_layers, flow_layers, out_channels):
        super().__init__()
        self.convcorr1 = _cna(in_channels_corr, corr_layers[0], None, 1)
        self.convcorr2 = _cna(corr_layers[0], corr_layers[1], None, 3) if len(corr_layers) == 2 else nn.Identity()
        self.convflow1 = _cna(2, flow_layers[0], None, 7)
        self.convflow2 = _cna(flow_layers[0], flow_layers[1], None, 3)
        self.conv = _cna(corr_layers[-1] + flow_layers[-1], out_channels - 2, None, 3)  # (the flow's 2 planes are appended)
        self.out_channels = out_channels

    def forward(self, flow, corr_features):
        corr = self.convcorr2(self.convcorr1(corr_features))
        f = self.convflow2(self.convflow1(flow))
        return torch.cat([self.conv(torch.cat([corr, f], dim=1)), flow], dim=1)


class ConvGRU(nn.Module):
    def __init__(self, input_size, hidden_size, kernel_size, padding):
        super().__init__()
        self.convz = nn.Conv2d(hidden_size + input_size, hidden_size, kernel_size=kernel_size, padding=padding)
        self.convr = nn.Conv2d(hidden_size + input_size, hidden_size, kernel_size=kernel_size, padding=padding)
        self.convq = nn.Conv2d(hidden_size + input_size, hidden_size, kernel_size=kernel_size, padding=padding)

    def forward(self, h, x):
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(self.convz(hx))
        r = torch.sigmoid(self.convr(hx))
        q = torch.tanh(self.convq(torch.cat([r * h, x], dim=1)))
        return (1 - z) * h + z * q


class RecurrentBlock(nn.Module):
    def __init__(self, input_size, hidden_size, kernel_size, padding):
        super().__init__()
        self.convgru1 = ConvGRU(input_size, hidden_size, kernel_size[0], padding[0])
        self.convgru2 = ConvGRU(input_size, hidden_size, kernel_size[1], padding[1]) if len(kernel_size) == 2 else nn.Identity()
        self.hidden_size = hidden_size

    def forward(self, h, x):
        h = self.convgru1(h, x)
        if isinstance(self.convgru2, ConvGRU):
            h = self.convgru2(h, x)
        return h


class FlowHead(nn.Module):
    def __init__(self, in_channels, hidden_size):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, hidden_size, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_size, 2, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.conv2(self.relu(self.conv1(x)))


class UpdateBlock(nn.Module):
    def __init__(self, motion_encoder, recurrent_block, flow_head):
        super().__init__()
        self.motion_encoder, self.recurrent_block, self.flow_head = motion_encoder, recurrent_block, flow_head
        self.hidden_state_size = recurrent_block.hidden_size

    def forward(self, hidden_state, context, corr_features, flow):
        x = torch.cat([context, self.motion_encoder(flow, corr_features)], dim=1)
        hidden_state = self.recurrent_block(hidden_state, x)
        return hidden_state, self.flow_head(hidden_state)


class MaskPredictor(nn.Module):
    def __init__(self, in_channels, hidden_size, multiplier=0.25):
        super().__init__()
        self.convrelu = _cna(in_channels, hidden_size, None, 3)
        self.conv = nn.Conv2d(hidden_size, RAFT_MASK_CHANNELS, 1, padding=0)
        self.multiplier = multiplier  # (RAFT's 0.25: it balances the gradients of the mask head)

    def forward(self, x):
        return self.multiplier * self.conv(self.convrelu(x))


# The two published configurations (torchvision's raft_small / raft_large builders).
CONFIGS = {
    "small": dict(block=BottleneckBlock, feature_layers=(32, 32, 64, 96, 128), feature_norm=nn.InstanceNorm2d,
                  context_layers=(32, 32, 64, 96, 160), context_norm=None, corr_levels=4, corr_radius=3,
                  motion_corr_layers=(96,), motion_flow_layers=(64, 32), motion_out=82, hidden=96, gru_kernels=(3,),
                  gru_paddings=(1,), flow_head_hidden=128, mask_hidden=None),
    "large": dict(block=ResidualBlock, feature_layers=(64, 64, 96, 128, 256), feature_norm=nn.InstanceNorm2d,
                  context_layers=(64, 64, 96, 128, 256), context_norm=nn.BatchNorm2d, corr_levels=4, corr_radius=4,
                  motion_corr_layers=(256, 192), motion_flow_layers=(128, 64), motion_out=128, hidden=128,
                  gru_kernels=((1, 5), (5, 1)), gru_paddings=((0, 2), (2, 0)), flow_head_hidden=256, mask_hidden=256),
}

# THE table of parameter names: this module's top-level blocks -> the prefixes of a torchvision RAFT state dict. Below a
# prefix the names are the module tree's (convnormrelu1.0.weight, layer2.1.downsample.0.bias, recurrent_block.convgru1.convz
# .weight, ...), which mirrors torchvision's. Not verified against a torchvision checkpoint; load_weights is strict.
TORCHVISION_NAMES = {
    "feature_encoder": "feature_encoder",
    "context_encoder": "context_encoder",
    "update_block": "update_block",
    "mask_predictor": "mask_predictor",
}


# What update="auto" runs for RAFT-small in float32 on the GPU when no gradient is recorded (inference_mode, no_grad: how the
# flow-matching step calls it; the fused path has no backward, so with gradients enabled "auto" stays the torch modules). It
# follows tools/raft_update_probe.py (profiles/raft_update_probe.json): the fused path only if, at 1024^2 and at 2048^2, its
# slowest turn of the update phase plus `begin` is faster than the torch path's fastest turn of the update phase. Measured:
# 5.85 + 0.15 ms against 6.49 ms at 1024^2, 13.79 + 0.33 ms against 17.36 ms at 2048^2.
AUTO_UPDATE_IS_FUSED = True

# RAFT-large's update="auto" runs the torch modules whatever this says: the existing tests take that run as their yardstick. It
# records the verdict of tools/raft_large_update_probe.py (profiles/raft_large_update_probe.json) by the same rule, so that a
# later change can flip "auto" on it. Measured (update phase with the mask predictor's call, fused + `begin` against torch):
# 14.12 + 0.37 ms (slowest turn 14.52) against 15.61 ms (fastest turn 15.60) at 1024^2, 43.50 + 0.96 ms (slowest 44.60) against
# 48.94 ms (fastest 48.91) at 2048^2: the fused path wins, by 1.08 x and 1.10 x, and peaks 0.18 and 0.74 GB higher in memory.
AUTO_UPDATE_LARGE_IS_FUSED = True

# What encoder="auto" runs under the same conditions. It follows tools/raft_encoder_probe.py (profiles/raft_encoder_probe.json):
# the fused encoders only if, at 1024^2 and at 2048^2, the slowest fused turn of the encoder phase (the feature encoder on the
# two images, then the context encoder) is faster than the fastest torch turn. Measured
# (fused median, min - max against torch): 1.80 ms (1.80 - 1.98) against 3.68 ms (3.67 - 3.80) at 1024^2, 5.62 ms (5.59 - 5.66) against
# 13.65 ms (13.62 - 13.77) at 2048^2; the fused encoders hold 0.43 and 1.72 GB of workspace there and peak HIGHER in memory. RAFT's default stays encoder="torch": "auto" is what an integrator asks for.
AUTO_ENCODER_IS_FUSED = True

# RAFT-large's encoder="auto" runs the torch modules whatever this says: the existing tests take that run as their yardstick. It
# records the verdict of tools/raft_large_encoder_probe.py (profiles/raft_large_encoder_probe.json) by the rule above, so that a
# later change can flip "auto" on it. Measured (encoder phase, fused median, min - max against torch): 6.73 ms (6.70 - 6.75) against
# 7.55 ms (7.53 - 7.58) at 1024^2, 25.21 ms (25.19 - 25.23) against 29.43 ms (29.40 - 29.56) at 2048^2: the fused encoders win, by
# 1.12 x and 1.17 x; the whole forward with update="fused_large" 25.32 against 26.14 ms and 84.16 against 88.48 ms. They hold 0.83
# and 3.29 GB of workspace there, and one forward peaks at 1.23 against 0.98 GB and 4.73 against 3.85 GB. Not measured:
# pretrained weights, batches above 1, the kernels under a profiler.
AUTO_ENCODER_LARGE_IS_FUSED = True


class RAFT(nn.Module):
    """RAFT with torchvision's call shape: `model(image1, image2, num_flow_updates=12) -> list of flows`, images [N, 3, H, W]
    in [-1, 1], H and W multiples of 8 and at least 128. The last entry is the final [N, 2, H, W] flow; with
    return_all=False (the default: flow_matching.py reads [-1] alone) it is the only one.

    corr: "ondemand" (the HIP lookup; float32 on the GPU), "volume" (plain torch, any dtype and device) or "auto": on-demand
    for float32 inputs on the GPU, volume otherwise.

    update: "torch" (the update block as torch modules, any dtype and device), "fused" (FusedUpdate: RAFT-small only, float32
    on the GPU, forward only, no CPU fallback), "fused_large" (FusedUpdateLarge: RAFT-large only, its update block and mask
    predictor, under the same conditions) or "auto": the fused path for RAFT-small in float32 on the GPU when no gradient
    is recorded, as the measurement decided (AUTO_UPDATE_IS_FUSED), the torch modules otherwise, and for RAFT-large always.

    encoder: "torch" (the two encoders as torch modules, any dtype and device; the default), "fused" (FusedEncoder: RAFT-small
    only, float32 on the GPU, forward only, no CPU fallback), "fused_large" (FusedEncoderLarge: RAFT-large only, under the same
    conditions; its context encoder's batch norms must be in eval mode) or "auto": the fused encoders for RAFT-small in float32
    on the GPU when no gradient is recorded and the measurement decided for them (AUTO_ENCODER_IS_FUSED), the torch modules
    otherwise, and for RAFT-large always (AUTO_ENCODER_LARGE_IS_FUSED records the measurement)."""

    def __init__(self, name="small", corr="auto", update="auto", encoder="torch"):
        super().__init__()
        if name not in CONFIGS:
            raise ValueError(f"raft RAFT: name is 'small' or 'large', got {name!r}")
        if corr not in ("auto", "ondemand", "volume"):
            raise ValueError(f"raft RAFT: corr is 'auto', 'ondemand' or 'volume', got {corr!r}")
        if update not in ("auto", "torch", "fused", "fused_large"):
            raise ValueError(f"raft RAFT: update is 'auto', 'torch', 'fused' or 'fused_large', got {update!r}")
        if update == "fused" and name != "small":
            raise ValueError(f"raft RAFT: update='fused' is RAFT-small's update block; '{name}' runs update='torch' or 'fused_large'")
        if update == "fused_large" and name != "large":
            raise ValueError(f"raft RAFT: update='fused_large' is RAFT-large's update block; '{name}' runs update='torch' or 'fused'")
        if encoder not in ("auto", "torch", "fused", "fused_large"):
            raise ValueError(f"raft RAFT: encoder is 'auto', 'torch', 'fused' or 'fused_large', got {encoder!r}")
        if encoder == "fused" and name != "small":
            raise ValueError(f"raft RAFT: encoder='fused' is RAFT-small's encoders; '{name}' runs encoder='torch' or 'fused_large'")
        if encoder == "fused_large" and name != "large":
            raise ValueError(f"raft RAFT: encoder='fused_large' is RAFT-large's encoders; '{name}' runs encoder='torch' or 'fused'")
        cfg = CONFIGS[name]
        self.name, self.corr, self.update, self.encoder = name, corr, update, encoder
        self.corr_levels, self.corr_radius = cfg["corr_levels"], cfg["corr_radius"]
        self.feature_encoder = FeatureEncoder(cfg["block"], cfg["feature_layers"], cfg["feature_norm"])
        self.context_encoder = FeatureEncoder(cfg["block"], cfg["context_layers"], cfg["context_norm"])
        hidden = cfg["hidden"]
        self.context_size = cfg["context_layers"][-1] - hidden
        motion = MotionEncoder(self.corr_levels * (2 * self.corr_radius + 1) ** 2, cfg["motion_corr_layers"],
                               cfg["motion_flow_layers"], cfg["motion_out"])
        recurrent = RecurrentBlock(motion.out_channels + self.context_size, hidden, cfg["gru_kernels"], cfg["gru_paddings"])
        self.update_block = UpdateBlock(motion, recurrent, FlowHead(hidden, cfg["flow_head_hidden"]))
        self.mask_predictor = None if cfg["mask_hidden"] is None else MaskPredictor(hidden, cfg["mask_hidden"])
        # this configuration's fused update and pair of fused encoders, under its size's names; the other size's stay None
        # (no Modules: nothing is registered)
        self._fused = self._fused_enc = self._fused_large = self._fused_enc_large = None
        if name == "small":
            self._fused = FusedUpdate(self.update_block)
            self._fused_enc = (FusedEncoder(self.feature_encoder), FusedEncoder(self.context_encoder))
        else:
            self._fused_large = FusedUpdateLarge(self.update_block, self.mask_predictor)
            self._fused_enc_large = (FusedEncoderLarge(self.feature_encoder), FusedEncoderLarge(self.context_encoder))

    def _ondemand(self, x):
        if self.corr == "volume":
            return False
        ok = x.device.type == "cuda" and x.dtype == torch.float32
        if self.corr == "ondemand" and not ok:
            raise RuntimeError(f"raft RAFT: corr='ondemand' runs in float32 on the GPU only (got {x.dtype} on '{x.device.type}'); "
                               "there is no CPU fallback, corr='volume' is the plain torch form")
        return ok

    def _runs_fused(self, option, noun, auto_is_fused, x):
        """Whether `option` ("update" or "encoder", RAFT-large's `noun`) runs its fused form on `x`. "fused_large" is never chosen
        under "auto" (AUTO_UPDATE_LARGE_IS_FUSED, AUTO_ENCODER_LARGE_IS_FUSED); the constructor refuses the other size's value,
        the option reassigned afterwards gets here."""
        value = getattr(self, option)
        if value == "fused_large" and self.name != "large":
            raise ValueError(f"raft RAFT: {option}='fused_large' is RAFT-large's {noun}; '{self.name}' runs {option}='torch' or 'fused'")
        if value == "torch" or (value != "fused_large" and self.name != "small"):
            return False
        ok, asked = x.device.type == "cuda" and x.dtype == torch.float32, value in ("fused", "fused_large")
        if asked and not ok:
            raise RuntimeError(f"raft RAFT: {option}='{value}' runs in float32 on the GPU only (got {x.dtype} on '{x.device.type}'); "
                               f"there is no CPU fallback, {option}='torch' is the plain torch form")
        return ok and (asked or (auto_is_fused and not torch.is_grad_enabled()))

    def _fused_update(self, x):
        return self._runs_fused("update", "update block", AUTO_UPDATE_IS_FUSED, x)

    def _fused_encoder(self, x):
        return self._runs_fused("encoder", "encoders", AUTO_ENCODER_IS_FUSED, x)

    def forward(self, image1, image2, num_flow_updates=12, return_all=False):
        N, _, H, W = image1.shape
        if image1.shape != image2.shape:
            raise ValueError("input images should have the same shape, instead got "
                             f"({H}, {W}) != ({image2.shape[-2]}, {image2.shape[-1]})")
        if H % 8 or W % 8:
            raise ValueError(f"input image H and W should be divisible by 8, instead got {H} (h) and {W} (w)")
        h, w = H // 8, W // 8
        if h < 16 or w < 16:
            raise ValueError(f"input image H and W should be at least 128, instead got {H} (h) and {W} (w): the feature "
                             "encoder downsamples by 8 and the correlation pyramid by another 8")
        ondemand, fused, fused_enc = self._ondemand(image1), self._fused_update(image1), self._fused_encoder(image1)
        if fused_enc:
            feature_encoder, context_encoder = self._fused_enc or self._fused_enc_large
        else:
            feature_encoder, context_encoder = self.feature_encoder, self.context_encoder
        fmaps = feature_encoder(torch.cat([image1, image2], dim=0))
        fmap1, fmap2 = torch.chunk(fmaps, chunks=2, dim=0)
        if ondemand:
            f1cl = corr_pyramid(fmap1, 1)
            pyramid = corr_pyramid(fmap2, self.corr_levels)
        else:
            pyramid = volume_pyramid(fmap1, fmap2, self.corr_levels)
        context_out = context_encoder(image1)
        hidden_state, context = torch.split(context_out, [self.update_block.hidden_state_size, self.context_size], dim=1)
        hidden_state, context = torch.tanh(hidden_state), F.relu(context)
        ys, xs = torch.meshgrid(torch.arange(h, dtype=image1.dtype, device=image1.device),
                                torch.arange(w, dtype=image1.dtype, device=image1.device), indexing="ij")
        coords0 = torch.stack([xs, ys], dim=0)[None].repeat(N, 1, 1, 1)
        coords1 = coords0.clone()
        fused_update = self._fused or self._fused_large
        if fused:
            fused_update.begin(hidden_state, context)
        flows = []
        for it in range(num_flow_updates):
            coords1 = coords1.detach()
            if ondemand:
                corr_features = corr_lookup(f1cl, pyramid, coords1, self.corr_radius)
            else:
                corr_features = volume_lookup(pyramid, coords1, self.corr_radius)
            if fused:  # (the hidden state stays in the workspace: RAFT-small has no mask predictor, RAFT-large's reads it there)
                delta = fused_update.step(corr_features, coords1 - coords0)
            else:
                hidden_state, delta = self.update_block(hidden_state, context, corr_features, coords1 - coords0)
            coords1 = coords1 + delta
            if return_all or it == num_flow_updates - 1:
                if self.mask_predictor is None:
                    mask = None
                else:
                    mask = fused_update.mask() if fused else self.mask_predictor(hidden_state)
                flow = coords1 - coords0
                flows.append(upsample_flow(flow, mask) if ondemand else _upsample_torch(flow, mask))
        return flows

    def torchvision_state_dict(self):
        """This module's state dict under torchvision's names (TORCHVISION_NAMES)."""
        return {_rename(k, TORCHVISION_NAMES): v for k, v in self.state_dict().items()}

    def load_weights(self, path_or_state_dict):
        """Loads a torchvision RAFT checkpoint (raft_small / raft_large weights: a path for torch.load, or the state dict),
        strict: a missing or an unexpected name raises. Returns self, in eval mode. Nothing is downloaded."""
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu", weights_only=True)
        back = {v: k for k, v in TORCHVISION_NAMES.items()}
        self.load_state_dict({_rename(k, back): v for k, v in sd.items()}, strict=True)
        return self.eval()


def _rename(key, table):
    head, _, tail = key.partition(".")
    return f"{table.get(head, head)}.{tail}" if tail else table.get(head, head)


def raft_small(corr="auto", update="auto", encoder="torch"):
    """RAFT-small: bottleneck encoders (128 feature channels), 4 levels at radius 3, one 3 x 3 GRU, bilinear upsampling."""
    return RAFT("small", corr, update, encoder)


def raft_large(corr="auto", encoder="torch", update="auto"):
    """RAFT-large: residual encoders (256 feature channels), 4 levels at radius 4, 1 x 5 + 5 x 1 GRUs, convex upsampling.
    encoder: "torch" and "auto" run the two encoders as torch modules, "fused_large" over the HIP convolutions
    (FusedEncoderLarge: the model in eval mode); encoder="fused" is RAFT-small's and refused. update: "auto" and "torch" run the
    update block and the mask predictor as torch modules, "fused_large" over the HIP convolutions (FusedUpdateLarge)."""
    return RAFT("large", corr, update, encoder)


__all__ = ["AUTO_ENCODER_IS_FUSED", "AUTO_ENCODER_LARGE_IS_FUSED", "AUTO_UPDATE_IS_FUSED", "AUTO_UPDATE_LARGE_IS_FUSED", "CONFIGS",
           "CorrPyramid", "FusedEncoder", "FusedEncoderLarge", "FusedUpdate", "FusedUpdateLarge", "RAFT", "TORCHVISION_NAMES", "conv2d_cl",
           "conv2d_rect_cl", "conv2d_strided_cl", "conv_info", "convex_upsample_torch", "corr_lookup", "corr_pyramid", "finish_cl",
           "fold_batchnorm", "raft_large", "raft_small", "stage_info", "upsample_flow",
           "volume_lookup", "volume_pyramid"]
