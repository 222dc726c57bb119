"""CPU: the float64 statement of the flow-matching step (tests/flow_cases.py) reproduces every fixture of the reference's own
code (tests/golden/flow, tests/golden/make_golden_flow.py) within RTOL of the quantity's maximum; the decisions of the
criteria and which object comes back are compared exactly."""
import numpy as np
import pytest

import flow_cases as F
from util import assert_close


def test_fixture_set():
    assert len(F.APPLY) == 6 and len(F.GETFLOW) == 3 and len(F.PERFORM) == 6
    assert {"stats", "adjust_affine"} <= set(F.FIXTURES)


@pytest.mark.parametrize("name", F.APPLY)
def test_warp_and_adjoint(name):
    fx = F.load(name)
    assert_close(F.warp(fx["img"], fx["flow"]), fx["out"], name + " out", allow_flips=False)
    g = F.warp_adjoint(fx["upstream"], fx["flow"])
    assert_close(g if fx["img"].ndim == 3 else g[0], fx["g_img"], name + " g_img", allow_flips=False)


def test_stats_and_constant_displacement():
    fx = F.load("stats")
    for k in range(3):
        flow = fx[f"flow{k}"]
        s = F.stats(flow)
        bound = 1e-6 * np.abs(flow).max()
        assert np.abs(s[[0, 1, 3, 4]] - fx[f"stats{k}"]).max() <= bound, k
        assert abs(s[2] - fx[f"meanabs{k}"]) <= bound, k
        assert np.abs(F.cst_displacement(flow) - fx[f"cst{k}"]).max() <= bound, k


@pytest.mark.parametrize("name", F.GETFLOW)
def test_get_flow(name):
    fx = F.load(name)
    mode = "downscale" if "downscale" in name else "upscale"
    H, W = fx["gt"].shape[1:]
    assert fx["model_gt"].shape[2:] == F.pad_shape(H, W, mode) == fx["model_flow"].shape[2:]
    flow = fx["model_flow"] if mode == "downscale" else fx["model_flow"][:, :, :H, :W]
    if fx["cst"]:
        flow = F.cst_displacement(flow)
    assert fx["flows"].shape == flow.shape
    assert np.abs(flow - fx["flows"]).max() <= 1e-6 * np.abs(fx["model_flow"]).max()
    h, w = F.pad_shape(H, W, mode) if mode == "downscale" else (H, W)
    assert np.array_equal(fx["gt_out"], fx["gt"][:, :h, :w]) and np.array_equal(fx["target_out"], fx["target"][:, :h, :w])
    # the network sees the images stretched to [-1, 1], three planes, cropped or reflect-padded on the right and at the bottom
    gt3 = np.broadcast_to((fx["gt"] - 0.5) * 2, (3, H, W))
    hh, ww = min(h, H), min(w, W)
    assert np.allclose(fx["model_gt"][0, :, :hh, :ww], gt3[:, :hh, :ww], atol=1e-6)
    if mode == "upscale" and fx["model_gt"].shape[3] > W:
        assert np.allclose(fx["model_gt"][0, :, :H, W], gt3[:, :, W - 2], atol=1e-6)  # reflect: the pixel before the last


@pytest.mark.parametrize("name", F.PERFORM)
def test_perform_flow_matching(name):
    fx = F.load(name)
    criteria = {"maxflow": "max_value_flow", "always": "always", "lphotom": "l_photom", "psnr": "psnr"}[name.split("_")[1]]
    mode = "downscale" if "downscale" in name else "upscale"
    flow, accepted, gt_out, image_out = F.perform(criteria, mode, bool(fx["cst"]), fx["image"], fx["gt"], fx["model_flow"],
                                                  float(fx["max_value_flow"]))
    assert accepted == bool(fx["accepted"])
    assert np.abs(flow - fx["flows"]).max() <= 1e-6 * np.abs(fx["model_flow"]).max()
    assert_close(image_out, fx["image_out"], name + " image", allow_flips=False)
    assert np.array_equal(np.asarray(gt_out, np.float32), fx["gt_out"])
    if accepted:
        g = F.warp_adjoint(fx["upstream"], flow)
        g = np.pad(g, ((0, 0), (0, fx["image"].shape[1] - g.shape[1]), (0, fx["image"].shape[2] - g.shape[2])))  # (a crop's gradient)
    else:
        g = fx["upstream"]  # the original image object came back
        assert np.array_equal(fx["image_out"], fx["image"])
    assert_close(g, fx["g_image"], name + " g_image", allow_flips=False)


def test_adjust_affine():
    fx = F.load("adjust_affine")
    out = F.adjust_affine(fx["world_view_transform"], int(fx["img_W"]), int(fx["img_H"]), fx["flow"])
    assert np.abs(out - fx["out"]).max() <= 1e-6 * np.abs(fx["out"]).max()
    assert np.array_equal(out[:3].astype(np.float32), fx["world_view_transform"][:3])
