"""GPU (MI355X): the fused panchromatic camera pipeline (include/eogs_pan.h, eogs2_amd/pan.py) against (1) the vectors
recorded from the reference's own PANAffineCamera pipelines (tests/golden/pan/*.npz), (2) the float64 restatement
(tests/pan_cases.py, itself pinned to those vectors by tests/test_pan_reference.py) at the sizes where the kernels take
another path, (3) properties: reproducible bits, the identity map is the affine camera's pipeline, the reference's
dict, shared colour corrections, and the example."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import pan_cases

pytestmark = pytest.mark.gpu
TOL = 2e-5  # images and image gradients: of max|ref| per array
CASES = pan_cases.load_cases()
PARAM_GRADS = ("grad_M", "grad_ins", "grad_map_params", "grad_map_weight", "grad_map_bias")


def param_tol(H, W):
    """Sums of H*W signed fp32 terms: the bound tests/test_gpu_shade.py derives."""
    return 2e-5 * max(1.0, (H * W) ** 0.5 / 30)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def run_gpu(c, dev, raw=None):
    """The case through pan_shade and autograd: the out_* and grad_* entries of tests/pan_cases.py, as numpy."""
    from eogs2_amd.pan import PanMap, pan_shade

    def t(a, rg):
        return torch.tensor(np.asarray(a), device=dev).requires_grad_(bool(rg))

    raw = t(c["raw"], True) if raw is None else raw
    shadow_on = "alt_diff" in c
    d = t(c["alt_diff"], True) if shadow_on else None
    M = t(c["M"], c["order"] == "B" or c["cc_mode"] != "none")
    ins = t(c["ins"], True) if shadow_on else None
    m, leaves = c["map"], {}
    if m in ("fixed", "learnable_fixed"):
        p = t(c["map_params"], m == "learnable_fixed" and int(c["unfrozen"]))
        pm = PanMap(m, params=p)
        if p.requires_grad:
            leaves["map_params"] = p
    elif m == "base":
        leaves = {"map_weight": t(c["map_weight"], True), "map_bias": t(c["map_bias"], True)}
        pm = PanMap(m, weight=leaves["map_weight"], bias=leaves["map_bias"], remove_sigm=bool(int(c["remove_sigm"])))
    elif m == "fixedandtranslate":
        learn = bool(int(c["learn_conv2d"]))
        w, b = t(c["map_weight"], learn), t(c["map_bias"], learn)
        pm = PanMap(m, weight=w, bias=b, fixed_weights=t(c["map_fixed_weights"], False), fixed_bias=t(c["map_fixed_bias"], False),
                    learn_conv2d=learn)
        if learn:
            leaves = {"map_weight": w, "map_bias": b}
    else:
        pm = PanMap(m)
    cc, shaded, shadow = pan_shade(raw, d, M, ins, pm, c["order"])
    res = {"out_cc": cc, "out_shaded": shaded, "shaded_requires_grad": bool(shaded.requires_grad)}
    L = (cc * t(c["g_cc"], False)).sum()
    if shaded.requires_grad:
        L = L + (shaded * t(c["g_shaded"], False)).sum()
    if shadow_on:
        res["out_shadow"] = shadow
        L = L + (shadow * t(c["g_shadow"], False)).sum()
    else:
        assert shadow is None
    L.backward()
    for name, leaf in {"raw": raw, "alt_diff": d, "M": M, "ins": ins, **leaves}.items():
        if leaf is not None and leaf.requires_grad:
            res["grad_" + name] = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def compare(got, ref, keys, H, W, what):
    bad = []
    for k in keys:
        a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        tol = param_tol(H, W) if k in PARAM_GRADS else TOL
        err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
        print(f"{what} {k}: max |diff| / max |ref| = {err:.3e} (bound {tol:.3e})")
        if not err <= tol:
            bad.append((k, err, tol))
    assert not bad, (what, bad)


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_golden(dev, name, case):
    got = run_gpu(case, dev)
    _, H, W = case["raw"].shape
    keys = [k for k in case if k.startswith(("out_", "grad_"))]
    compare(got, case, keys, H, W, name)
    assert got["shaded_requires_grad"] == bool(int(case["shaded_requires_grad"]))
    for k, v in got.items():  # a gradient the reference's graph does not have
        if k.startswith("grad_") and k not in case:
            assert not np.any(v), k


# 1x1; 7x129: odd width, less than one workgroup's stride, not a multiple of 4; 64x68: H*W a multiple of 4 (the 16-byte
# path) over several workgroups with a tail; 255x257: several workgroups, odd (the 4-byte path), with a tail
@pytest.mark.parametrize("order", ["A", "B"])
@pytest.mark.parametrize("map_name", pan_cases.MAPS)
@pytest.mark.parametrize("H,W,shadow", [(1, 1, True), (7, 129, True), (33, 65, False), (64, 68, True), (64, 68, False), (255, 257, True)])
def test_vs_restatement(dev, H, W, shadow, map_name, order):
    c = pan_cases.make_case(order, map_name, H, W, shadow=shadow, seed=H * 1000 + W)
    ref = pan_cases.restate(c)
    got = run_gpu(c, dev)
    compare(got, ref, [k for k in ref if k.startswith(("out_", "grad_"))], H, W, f"{order} {map_name} {H}x{W}")
    assert got["shaded_requires_grad"] == ref["shaded_requires_grad"]


# 300x1000: more workgroups than the reduction reads in one pass per thread, on the maps with the most reduced sums
@pytest.mark.parametrize("order", ["A", "B"])
@pytest.mark.parametrize("map_name", ["learnable_fixed", "base"])
def test_vs_restatement_many_workgroups(dev, map_name, order):
    H, W = 300, 1000
    c = pan_cases.make_case(order, map_name, H, W, seed=5)
    ref = pan_cases.restate(c)
    got = run_gpu(c, dev)
    compare(got, ref, [k for k in ref if k.startswith(("out_", "grad_"))], H, W, f"{order} {map_name} {H}x{W}")
    # the same pixels behind a base pointer that is not 16-byte aligned: the 4-byte path, the same image bits
    flat = torch.zeros(3 * H * W + 1, device=dev)
    flat[1:] = torch.tensor(c["raw"], device=dev).reshape(-1)
    off = run_gpu(c, dev, raw=flat[1:].view(3, H, W).requires_grad_(True))
    for k in ("out_cc", "out_shaded", "out_shadow"):
        assert np.array_equal(off[k], got[k]), k
    compare(off, ref, [k for k in ref if k.startswith("grad_")], H, W, f"{order} {map_name} unaligned")


@pytest.mark.parametrize("order,map_name,H,W", [("A", "learnable_fixed", 255, 257), ("B", "base", 300, 1000), ("A", "fixedandtranslate", 64, 68)])
def test_same_call_twice_same_bits(dev, order, map_name, H, W):
    c = pan_cases.make_case(order, map_name, H, W, seed=11)
    a, b = run_gpu(c, dev), run_gpu(c, dev)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_identity_is_the_affine_camera_pipeline(dev):
    from eogs2_amd import pan, shade

    c = pan_cases.make_case("A", "identity", 33, 65, seed=3)
    outs = []
    for mod in (pan, shade):
        cam = types.SimpleNamespace(use_cc=True, use_exposure=False, use_shadow=True, weird_pan_setup=False,
                                    msi_to_pan=_ns("msi_to_pan_identity"))
        cam.color_correction = torch.nn.Conv2d(3, 3, 1).to(dev)
        with torch.no_grad():
            cam.color_correction.weight.copy_(torch.tensor(c["M"][:, :3]).reshape(3, 3, 1, 1))
            cam.color_correction.bias.copy_(torch.tensor(c["M"][:, 3]))
        cam.inshadow_color_correction = torch.nn.Parameter(torch.tensor(c["ins"], device=dev).reshape(3, 1, 1))
        raw = torch.tensor(c["raw"], device=dev, requires_grad=True)
        d = torch.tensor(c["alt_diff"], device=dev, requires_grad=True)
        out = mod.render_pipeline(cam, raw, d)
        ((out["final"] * torch.tensor(c["g_shaded"], device=dev)).sum() + (out["cc"] * torch.tensor(c["g_cc"], device=dev)).sum()).backward()
        outs.append([out["shadowmap"], out["shaded"], out["cc"], out["final"], raw.grad, d.grad, cam.color_correction.weight.grad,
                     cam.color_correction.bias.grad, cam.inshadow_color_correction.grad])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][1].shape == (3, 33, 65)


def _ns(name, **attrs):
    """A duck-typed module: the class name and attributes of the reference's."""
    return type(name, (), attrs)()


def _fixed_module(dev):
    return _ns("base_msi_to_pan", pan_params=torch.tensor(pan_cases.FIXED, device=dev))


def _camera(dev, order_b, module, shadow=True):
    n = 1 if order_b else 3
    cam = types.SimpleNamespace(use_cc=True, use_exposure=False, use_shadow=shadow, weird_pan_setup=order_b, msi_to_pan=module)
    cam.color_correction = torch.nn.Conv2d(n, n, 1).to(dev)
    cam.inshadow_color_correction = torch.nn.Parameter(torch.full((n, 1, 1), 0.05, device=dev))
    return cam


def test_render_pipeline_returns_the_references_dict(dev):
    from eogs2_amd.pan import render_pipeline

    H, W = 33, 65
    g = torch.Generator().manual_seed(4)
    raw = torch.rand((3, H, W), generator=g).to(dev).requires_grad_(True)
    d = torch.randn((H, W), generator=g).to(dev)
    for order_b, planes in ((False, 3), (True, 1)):
        out = render_pipeline(_camera(dev, order_b, _fixed_module(dev)), raw, d)
        assert sorted(out) == ["cc", "final", "shaded", "shadowmap"]
        assert out["cc"].shape == (planes, H, W) and out["shaded"].shape == (1, H, W) and out["final"].shape == (1, H, W)
        assert out["shadowmap"].shape == (H, W) and out["final"] is out["shaded"]
        # use_shadow off, or no altitude difference: no shadow map
        assert render_pipeline(_camera(dev, order_b, _fixed_module(dev), shadow=False), raw, d)["shadowmap"] is None
        assert render_pipeline(_camera(dev, order_b, _fixed_module(dev)), raw)["shadowmap"] is None
    # the map-first order without shadow: final is the map of raw, not cc; cc still reaches the colour correction
    cam = _camera(dev, True, _fixed_module(dev))
    with torch.no_grad():
        cam.color_correction.weight.fill_(0.7)
        cam.color_correction.bias.fill_(0.2)
    out = render_pipeline(cam, raw)
    p, x = pan_cases.FIXED, raw.detach().cpu().double().numpy()
    p0 = p[3] * (p[0] * x[0] + p[1] * x[1] + p[2] * x[2] + p[4])
    assert np.abs(out["final"][0].detach().cpu().numpy() - p0).max() <= TOL * np.abs(p0).max()
    assert np.abs(out["cc"][0].detach().cpu().numpy() - (0.7 * p0 + 0.2)).max() <= TOL * np.abs(0.7 * p0 + 0.2).max()
    assert out["shadowmap"] is None and out["final"].requires_grad
    out["cc"].sum().backward()
    gw, gb = cam.color_correction.weight.grad, cam.color_correction.bias.grad
    assert gw is not None and abs(float(gw) - p0.sum()) <= param_tol(H, W) * abs(p0.sum())
    assert abs(float(gb) - H * W) <= param_tol(H, W) * H * W
    assert np.abs(raw.grad.cpu().numpy() - 0.7 * p[3] * np.array(p[:3])[:, None, None]).max() <= TOL * 0.7 * p[3] * max(np.abs(p[:3]))


def test_shared_colour_correction_receives_both_gradients(dev):
    """MS_affine_cameras.py:48-67: the MSI and the PAN camera hold one Conv2d object."""
    from eogs2_amd import pan, shade

    H, W = 33, 65
    g = torch.Generator().manual_seed(6)
    raw_m, raw_p = (torch.rand((3, H, W), generator=g).to(dev) for _ in range(2))
    d = torch.randn((H, W), generator=g).to(dev)
    up_m, up_p = torch.randn((3, H, W), generator=g).to(dev), torch.randn((1, H, W), generator=g).to(dev)
    msi, pn = _camera(dev, False, None), _camera(dev, False, _fixed_module(dev))

    def grads(share):
        conv = torch.nn.Conv2d(3, 3, 1).to(dev)
        with torch.no_grad():
            conv.weight.copy_(torch.eye(3).reshape(3, 3, 1, 1) * 0.9 - 0.05)
            conv.bias.fill_(0.01)
        convs = (conv, conv) if share else (conv, None)
        res = []
        for i, (cam, mod, raw, up) in enumerate(((msi, shade, raw_m, up_m), (pn, pan, raw_p, up_p))):
            if convs[i] is None:
                conv.weight.grad = conv.bias.grad = None
            cam.color_correction = conv
            (mod.render_pipeline(cam, raw, d)["final"] * up).sum().backward()
            res.append((conv.weight.grad.clone(), conv.bias.grad.clone()))
        return res

    (w_m, b_m), (w_p, b_p) = grads(False)  # each camera on its own
    _, (w_both, b_both) = grads(True)  # one object: autograd accumulates
    assert w_p.abs().max() > 0 and w_m.abs().max() > 0
    assert torch.equal(w_both, w_m + w_p) and torch.equal(b_both, b_m + b_p)


def test_example_with_a_pan_camera():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    args = ["--gaussians", "30000", "--size", "192", "--iters", "120", "--quiet", "--pan-map", "fixed"]
    eager = train_synthetic.main(args)
    print("fixed, eager:", eager)
    assert eager[1] < 0.6 * eager[0], eager
    graph = train_synthetic.main(args + ["--graph"])
    assert graph == eager, (eager, graph)  # bit for bit: every sum of the chain runs in a fixed order
    first, last, _ = train_synthetic.main(args[:-1] + ["learnable_fixed", "--pan-first"])
    print("learnable_fixed, map first:", first, last)
    assert last < first, (first, last)


@pytest.mark.parametrize("order,map_name,H,W", [("A", "fixed", 7, 129), ("B", "base", 7, 129), ("A", "identity", 64, 68)])
def test_nan_altitude_difference_is_kept(dev, order, map_name, H, W):
    """`alt_diff.clip(max=0)` keeps a NaN (affine_cameras.py:38), as in shade.hip: the shadow, the shaded pixel, that pixel's raw
    gradient and every parameter sum holding s are NaN, the NaN's own gradient is 0, every other pixel keeps its bits."""
    c = pan_cases.make_case(order, map_name, H, W, seed=17)
    base = run_gpu(c, dev)
    c = dict(c, alt_diff=c["alt_diff"].copy())
    p = (H // 2, W // 3)
    c["alt_diff"][p] = np.nan
    got = run_gpu(c, dev)
    assert np.isnan(got["out_shadow"][p]) and np.isnan(got["out_shaded"][..., p[0], p[1]]).all()
    assert got["grad_alt_diff"][p] == 0.0 and np.isnan(got["grad_raw"][:, p[0], p[1]]).all() and np.isnan(got["grad_ins"]).all()
    assert not np.isnan(got["out_cc"]).any() or order == "B"
    for k in ("out_shadow", "out_shaded", "out_cc", "grad_alt_diff", "grad_raw"):
        a, b = got[k].copy(), base[k].copy()
        a[..., p[0], p[1]] = b[..., p[0], p[1]] = 0
        assert np.array_equal(a, b), k
