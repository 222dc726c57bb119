"""The flow-matching step stated in float64, in PIXEL coordinates (no normalisation round trip), and the fixtures of the
reference's own code (tests/golden/flow/*.npz, tests/golden/make_golden_flow.py). What eogs2_amd.flow and
eogs2_amd/csrc/flow.hip must compute:

  warp          out[c, y, x] = bilinear sample of img[c] at (clip(x + fx, 0, W - 1), clip(y + fy, 0, H - 1)): first tap the
                floor, second tap the next pixel (or the same one at the far border, where it weighs 0)
  warp_adjoint  the transpose of that linear map applied to an upstream gradient (the flow receives none)
  stats         mean x, mean y, mean |flow| over both planes, std x, std y (unbiased)
  criteria      the decisions of perform_flow_matching (flow_matching.py:299-329)
"""
import glob
import os

import numpy as np

FLOW_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(FLOW_DIR, "*.npz")))
APPLY = [n for n in FIXTURES if n.startswith("apply_")]
GETFLOW = [n for n in FIXTURES if n.startswith("getflow_")]
PERFORM = [n for n in FIXTURES if n.startswith("perform_")]


def load(name):
    z = np.load(os.path.join(FLOW_DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


def taps(flow, H, W):
    """(x0, x1, wx, y0, y1, wy) of a (2, H, W) flow: integer tap indices and the weight of the second tap, float64."""
    flow = np.asarray(flow, dtype=np.float64)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx, sy = np.clip(x + flow[0], 0, W - 1), np.clip(y + flow[1], 0, H - 1)
    x0, y0 = np.floor(sx), np.floor(sy)
    wx, wy = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    return x0, np.minimum(x0 + 1, W - 1), wx, y0, np.minimum(y0 + 1, H - 1), wy


def warp(img, flow):
    """img (C, H, W) or (H, W), flow (1, 2, H, W) or (2, H, W) -> (C, H, W) float64."""
    img = np.asarray(img, dtype=np.float64)
    img = img[None] if img.ndim == 2 else img
    flow = np.asarray(flow).reshape(2, *img.shape[1:])
    x0, x1, wx, y0, y1, wy = taps(flow, *img.shape[1:])
    return (img[:, y0, x0] * ((1 - wx) * (1 - wy)) + img[:, y0, x1] * (wx * (1 - wy)) + img[:, y1, x0] * ((1 - wx) * wy)
            + img[:, y1, x1] * (wx * wy))


def warp_adjoint(upstream, flow):
    """d sum(warp(img, flow) * upstream) / d img: (C, H, W) float64."""
    g = np.asarray(upstream, dtype=np.float64)
    C, H, W = g.shape
    flow = np.asarray(flow).reshape(2, H, W)
    x0, x1, wx, y0, y1, wy = taps(flow, H, W)
    out = np.zeros((C, H * W))
    for c in range(C):
        for yy, xx, w in ((y0, x0, (1 - wx) * (1 - wy)), (y0, x1, wx * (1 - wy)), (y1, x0, (1 - wx) * wy), (y1, x1, wx * wy)):
            np.add.at(out[c], (yy * W + xx).ravel(), (g[c] * w).ravel())
    return out.reshape(C, H, W)


def stats(flow):
    """[mean x, mean y, mean |flow|, std x, std y] of a (1, 2, H, W) flow, float64."""
    f = np.asarray(flow, dtype=np.float64).reshape(2, -1)
    return np.array([f[0].mean(), f[1].mean(), np.abs(f).mean(), f[0].std(ddof=1), f[1].std(ddof=1)])


def cst_displacement(flow):
    f = np.asarray(flow, dtype=np.float64)
    return np.broadcast_to(f.mean(axis=(2, 3), keepdims=True), f.shape)


def pad_shape(H, W, mode):
    """The size the flow network is called with (flow_matching.py:102-149)."""
    return ((H // 8) * 8, (W // 8) * 8) if mode == "downscale" else (-(-H // 8) * 8, -(-W // 8) * 8)


def adjust_affine(wvt, img_W, img_H, flow):
    s = stats(flow)
    out = np.array(wvt, dtype=np.float64)
    out[-1, 0] -= s[0] * 2 / img_W
    out[-1, 1] -= s[1] * 2 / img_H
    return out


def psnr(a, b):
    mse = ((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).reshape(a.shape[0], -1).mean(1)
    return 20 * np.log10(1.0 / np.sqrt(mse))


def _ssim(a, b):
    """utils/loss_utils.py:45-85 in float64: 11 x 11 Gaussian window (sigma 1.5), zero padding, mean of the map."""
    k = np.exp(-((np.arange(11) - 5) ** 2) / (2 * 1.5 ** 2))
    k /= k.sum()

    def blur(x):
        x = np.pad(x, ((0, 0), (5, 5), (5, 5)))
        x = sum(k[i] * x[:, i:i + x.shape[1] - 10, :] for i in range(11))
        return sum(k[i] * x[:, :, i:i + x.shape[2] - 10] for i in range(11))

    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    mu1, mu2 = blur(a), blur(b)
    s1, s2, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).mean()


def lphotom(image, gt, lambda_dssim=0.2):
    return (1 - lambda_dssim) * np.abs(np.asarray(gt, np.float64) - image).mean() + lambda_dssim * (1 - _ssim(image, gt))


def perform(criteria, mode, cst, image, gt, model_flow, max_value_flow):
    """perform_flow_matching in float64: (flows, accepted, gt_out, image_out)."""
    C, H, W = image.shape
    flow = np.asarray(model_flow, dtype=np.float64)
    if mode == "downscale":
        h, w = pad_shape(H, W, mode)
        image2, gt2 = image[:, :h, :w], gt[:, :h, :w]
    else:
        flow, image2, gt2 = flow[:, :, :H, :W], image, gt
    if cst:
        flow = cst_displacement(flow)
    warped = warp(image2, flow)
    if criteria == "max_value_flow":
        accepted = np.abs(flow).mean() < max_value_flow
    elif criteria == "always":
        accepted = True
    elif criteria == "psnr":
        (after,), (before,) = psnr(gt2, warped), psnr(gt, image)  # one plane only
        accepted = after > before
    else:
        accepted = lphotom(warped, gt2) < lphotom(np.asarray(image, np.float64), gt)
    return flow, bool(accepted), (gt2 if accepted else gt), (warped if accepted else image)
