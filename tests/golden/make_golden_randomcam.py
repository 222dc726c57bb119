"""Generates tests/golden/randomcam/*.npz by running the REFERENCE's own `RandomcamRendering_Loss.forward`
(loss/main_loss.py:97-164) and, under it, `render_resample_virtual_camera_wshadowmapping`
(gaussian_renderer/renderer_cc_shadow.py:57-145), imported at run time from the reference's checkout (build container only),
on the CPU. Only arrays and strings are stored.

    python tests/golden/make_golden_randomcam.py

`gaussian_renderer.renderer.render` is replaced by a table lookup that returns seeded leaf tensors — the virtual camera's
render [5,H,W] and the sun camera's [5,2H,2W] —, so that the gradients with respect to both renders are autograd's own.
`render_pipeline` is called unbound on a plain namespace carrying the attributes it reads, as make_golden_shade.py and
make_golden_pan.py do; `loss`, `gaussian_renderer`, `scene`, ... are stub packages whose `__path__` points into the
reference, so that their `__init__.py` (which pull the rasterizer and the dataset readers) never run.

Every set-up of tests/randomcam_cases.SETUPS is run for both render types with `use_gt` off and on, in float32 and, by the
same statements on the inputs cast to double, in float64.

    <setup>_inputs.npz                 the inputs, shared by the four variants
    <setup>_<render_type>_gt<0|1>.npz  per result X: `X` the float32 result, `X_delta` = float64 result - X (stored as
                                       float32: X + X_delta gives the float64 result to 1e-15 of its size),
                                       `X_d32` = max |float32 - float64|

Results: both losses; gradients of 0.7 L_alt + 1.3 L_rgb with respect to both renders, `altitude_render` (through
`rendered_uva` and directly), `raw_render` / `shaded`, and the camera's colour-correction, in-shadow and MSI->PAN
parameters. An empty occlusion map makes the reference return constants without a graph: zeros are stored.

Before anything is written the float64 values are checked: every pixel is further than 1e-4 from every decision — |Δalt|
against 0.30, |u| and |v| against 1 in both resamples, the shadow clip at 0 — and further than 1e-5 from the kink of every
absolute value; a seed that fails is replaced by the next. The `identity` set-up is the exception: its border pixels sit
at exactly +-1, which float32 and float64 decide alike.
"""
import copy
import functools
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_golden_shade import REFROOT  # noqa: E402  (where the reference's sources are read from)
import randomcam_cases as RC  # noqa: E402

OUT = RC.GOLDEN
TABLE = {}  # what the stubbed render returns: camera key -> leaf tensor


def load_ref():
    for name, sub in (("scene", "scene"), ("scene.cameras", "scene/cameras"), ("scene.msi_to_pan", "scene/msi_to_pan"),
                      ("loss", "loss"), ("gaussian_renderer", "gaussian_renderer")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REFROOT, sub)]
        sys.modules[name] = pkg
    stub = types.ModuleType("gaussian_renderer.renderer")
    stub.render = lambda camera, gaussians, pipe, background, **kw: {"render": TABLE[camera]}
    sys.modules["gaussian_renderer.renderer"] = stub
    rcs = importlib.import_module("gaussian_renderer.renderer_cc_shadow")
    main_loss = importlib.import_module("loss.main_loss")
    assert main_loss.render_resample_virtual_camera_wshadowmapping is rcs.render_resample_virtual_camera_wshadowmapping
    pan = importlib.import_module("scene.cameras.PAN_affine_cameras")
    aff = importlib.import_module("scene.cameras.affine_cameras")
    maps = importlib.import_module("scene.msi_to_pan.transf_msi_to_pan")
    return types.SimpleNamespace(rcs=rcs, main_loss=main_loss, pan=pan, aff=aff, maps=maps)


def field(x, y):
    """The terrain both cameras see, over normalised image coordinates."""
    return 0.5 + 0.25 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y - 0.2)


def make_inputs(setup, seed):
    """The seeded inputs of a set-up (tests/randomcam_cases.SETUPS) as float32 arrays."""
    g = np.random.default_rng(seed)
    H, W, kind = setup["H"], setup["W"], setup["kind"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    U, V = np.meshgrid(np.linspace(-1, 1, W) * setup["span"], np.linspace(-1, 1, H) * setup["span"], indexing="xy")
    d = dict(kind=np.array(kind), U=f32(U), V=f32(V), upstream=f32([0.7, 1.3]))
    d["altitude_render"] = f32(field(U, V) + 0.02 * g.normal(size=(H, W)))
    a, b = setup["shear"]
    d["cam2virt"] = RC.shear(a, b)
    sa, sb = g.uniform(0.05, 0.12, size=2) * np.array([1, -1])
    d["camera_to_sun"] = f32(np.diag([setup["sun_scale"], setup["sun_scale"], 1.0]) @ RC.shear(sa, sb).astype(np.float64))
    # the virtual camera's render: colours, the terrain on its own grid with noise and one raised disc (an occluder: |Δalt|
    # beyond 0.30 there), accumulated opacity
    xv, yv = np.meshgrid(np.linspace(-1, 1, W), np.linspace(-1, 1, H), indexing="xy")
    alt = field(xv, yv) + 0.03 * g.normal(size=(H, W)) + 0.6 * ((xv - 0.3) ** 2 + (yv + 0.2) ** 2 < 0.12)
    if setup["empty"]:
        alt = alt + 1.0
    d["virtual_render"] = f32(np.concatenate([g.uniform(size=(3, H, W)), alt[None], g.uniform(size=(1, H, W))]))
    # the sun camera's render at twice the size: the same terrain as its footprint sees it, noise of both signs around it
    xs, ys = np.meshgrid(np.linspace(-1, 1, 2 * W), np.linspace(-1, 1, 2 * H), indexing="xy")
    salt = field(xs / setup["sun_scale"], ys / setup["sun_scale"]) + 0.1 * g.normal(size=(2 * H, 2 * W))
    d["sun_render"] = f32(np.concatenate([g.uniform(size=(3, 2 * H, 2 * W)), salt[None], g.uniform(size=(1, 2 * H, 2 * W))]))
    n = setup["planes"]
    d["raw_render"], d["shaded"] = f32(g.uniform(size=(3, H, W))), f32(g.uniform(size=(n, H, W)))
    d["gt_raw"], d["gt_shaded"] = f32(g.uniform(size=(3, H, W))), f32(g.uniform(size=(n, H, W)))
    if kind in ("cc", "pan_identity"):
        d["cc_weight"] = f32((np.eye(3) + 0.2 * g.normal(size=(3, 3))).reshape(3, 3, 1, 1))
        d["cc_bias"] = f32(0.1 * g.normal(size=3))
        d["inshadow"] = f32(0.05 + 0.3 * g.uniform(size=(3, 1, 1)))
    elif kind == "exposure":
        d["exposure"] = f32((np.eye(3, 4) + 0.2 * g.normal(size=(3, 4)))[None])
        d["inshadow"] = f32(0.05 + 0.3 * g.uniform(size=(3, 1, 1)))
    elif kind == "pan_base_first":
        d["cc_weight"] = f32(np.array(1.0 + 0.2 * g.normal()).reshape(1, 1, 1, 1))
        d["cc_bias"] = f32(0.1 * g.normal(size=1))
        d["inshadow"] = f32(0.05 + 0.3 * g.uniform(size=(1, 1, 1)))
        d["map_weight"] = f32((np.array([0.438469, 1.1331377, -0.6794343]) + 0.2 * g.normal(size=3)).reshape(1, 3, 1, 1))
        d["map_bias"] = f32(0.1 * g.normal(size=1))
    else:
        raise KeyError(kind)
    return d


def build_camera(ref, d, dtype):
    """The namespace the reference's render_pipeline and get_sun_camera are run on; {fixture name: Parameter}."""
    kind = str(d["kind"])
    t = lambda k: torch.from_numpy(d[k]).to(dtype)  # noqa: E731
    cam = types.SimpleNamespace(use_cc=False, use_exposure=False, use_shadow=True, shadow_map=ref.aff.ShadowMap(), mode="pan",
                                weird_pan_setup=False)
    leaves = {}
    if kind in ("cc", "pan_identity", "pan_base_first"):
        n = 1 if kind == "pan_base_first" else 3
        cam.use_cc = True
        cam.color_correction = torch.nn.Conv2d(n, n, 1, bias=True).to(dtype)
        with torch.no_grad():
            cam.color_correction.weight.copy_(t("cc_weight"))
            cam.color_correction.bias.copy_(t("cc_bias"))
        leaves.update(cc_weight=cam.color_correction.weight, cc_bias=cam.color_correction.bias)
    else:
        cam.use_exposure = True
        cam.exposure = torch.nn.Parameter(t("exposure").clone())
        leaves.update(exposure=cam.exposure)
    cam.inshadow_color_correction = torch.nn.Parameter(t("inshadow").clone())
    leaves.update(inshadow=cam.inshadow_color_correction)
    if kind == "pan_identity":
        cam.msi_to_pan = ref.maps.load_msi_to_pan(types.SimpleNamespace(name="identity"))
        cam._render_pipeline = functools.partial(ref.pan.PANAffineCamera._render_pipeline, cam)
        cam.render_pipeline = functools.partial(ref.pan.PANAffineCamera.render_pipeline, cam)
    elif kind == "pan_base_first":
        cam.weird_pan_setup = True
        cam.msi_to_pan = ref.maps.load_msi_to_pan(types.SimpleNamespace(name="base", msi_channels=3, pan_channels=1, kernel_size=1,
                                                                       remove_sigm=False, init_value=False, use_avgpool=False)).to(dtype)
        with torch.no_grad():
            cam.msi_to_pan.linear.weight.copy_(t("map_weight"))
            cam.msi_to_pan.linear.bias.copy_(t("map_bias"))
        leaves.update(map_weight=cam.msi_to_pan.linear.weight, map_bias=cam.msi_to_pan.linear.bias)
        cam._render_pipeline_weird = functools.partial(ref.pan.PANAffineCamera._render_pipeline_weird, cam)
        cam.render_pipeline = functools.partial(ref.pan.PANAffineCamera.render_pipeline, cam)
    else:
        cam.render_pipeline = functools.partial(ref.aff.AffineCamera.render_pipeline, cam)
    camera_to_sun = t("camera_to_sun")
    cam.get_sun_camera = lambda: ("sun", camera_to_sun)
    return cam, leaves


def run(ref, d, render_type, use_gt, dtype, empty):
    """The reference's forward and autograd on the inputs in `dtype`: {result name: numpy array}."""
    t = lambda k: torch.from_numpy(d[k]).to(dtype)  # noqa: E731
    cam, leaves = build_camera(ref, d, dtype)
    V, S = t("virtual_render").requires_grad_(True), t("sun_render").requires_grad_(True)
    A, raw, shaded = t("altitude_render").requires_grad_(True), t("raw_render").requires_grad_(True), t("shaded").requires_grad_(True)
    TABLE.clear()
    TABLE.update(virtual=V, sun=S)
    uva = torch.stack((t("U"), t("V"), A), dim=-1)  # train_pan.py:281
    gt = t("gt_raw") if render_type == "rawrender" else t("gt_shaded")
    fn = ref.main_loss.RandomcamRendering_Loss(1.0, 1.0, render_type, use_gt=use_gt)
    L_alt, L_rgb = fn.forward(new_camera="virtual", true_cam=cam, camera_to_new=t("cam2virt"), rendered_uva=uva, gaussians=None, pipe=None,
                              bg=None, altitude_render=A, raw_render=raw, gt_image=gt, shaded=shaded)
    wanted = {"g_virtual_render": V, "g_altitude_render": A}
    if render_type == "rawrender_wshadow":
        wanted["g_sun_render"] = S
        wanted.update({"g_" + k: v for k, v in leaves.items()})
    if not use_gt:
        wanted["g_raw_render" if render_type == "rawrender" else "g_shaded"] = raw if render_type == "rawrender" else shaded
    res = dict(L_alt=L_alt.detach().to(dtype).numpy().copy(), L_rgb=L_rgb.detach().to(dtype).numpy().copy())  # (an empty map: float32 constants)
    if empty:
        assert not L_alt.requires_grad and float(L_alt) == 0.0 and float(L_rgb) == 0.0
        res.update({k: np.zeros(tuple(v.shape), dtype=res["L_alt"].dtype) for k, v in wanted.items()})
        return res
    up = t("upstream")
    (up[0] * L_alt + up[1] * L_rgb).backward()
    for k, v in wanted.items():
        assert v.grad is not None, k
        res[k] = v.grad.detach().numpy().copy()
    for k, v in {"g_sun_render": S, "g_raw_render": raw, "g_shaded": shaded}.items():
        assert k in wanted or v.grad is None, k  # what the variant does not read gets no gradient
    return res


def margins_hold(ref, d, setup):
    """The float64 decisions of the set-up (the same for its four variants), each further than 1e-4 from its threshold."""
    t = lambda k: torch.from_numpy(d[k]).double()  # noqa: E731
    TABLE.clear()
    TABLE.update(virtual=t("virtual_render"), sun=t("sun_render"))
    A = t("altitude_render")
    uva = torch.stack((t("U"), t("V"), A), dim=-1)
    rgb, alt, uv = ref.rcs.render_resample_virtual_camera("virtual", t("cam2virt"), uva, None, None, None)
    virtual_uva = torch.einsum("...ij,...j->...i", t("cam2virt"), uva)
    virt_to_sun = torch.inverse(t("cam2virt")) @ t("camera_to_sun")
    _, sun_alt, sun_uv = ref.rcs.render_resample_virtual_camera("sun", virt_to_sun, virtual_uva, None, None, None)
    shadow_diff = TABLE["virtual"][3] - sun_alt
    delta = A - alt
    away = lambda x, thr, m: bool(((x.abs() - thr).abs() > m).all())  # noqa: E731
    ok = away(delta, 0.30, 1e-4) and away(sun_uv, 1.0, 1e-4) and away(shadow_diff, 0.0, 1e-4) and away(delta, 0.0, 1e-5)
    if setup["name"] != "identity":
        ok = ok and away(uv, 1.0, 1e-4)
    else:
        assert torch.equal(uv, uva[..., :2])
    cam, _ = build_camera(ref, d, torch.float64)
    out = ref.rcs.render_resample_virtual_camera_wshadowmapping("virtual", cam, t("cam2virt"), uva, None, None, None)
    ok = ok and away(t("raw_render") - rgb, 0.0, 1e-5) and away(t("gt_raw") - rgb, 0.0, 1e-5)
    ok = ok and away(t("shaded") - out[0], 0.0, 1e-5) and away(t("gt_shaded") - out[0], 0.0, 1e-5)
    occ = (delta.abs() < 0.30) & (uv.abs() < 1).all(-1)
    stats = dict(inside=int(occ.sum()), outside_virtual=int((uv.abs() >= 1).any(-1).sum()), outside_sun=int((sun_uv.abs() > 1).any(-1).sum()),
                 lit=int((shadow_diff > 0).sum()), shadowed=int((shadow_diff < 0).sum()))
    return ok, stats


def main():
    ref = load_ref()
    os.makedirs(OUT, exist_ok=True)
    for i, setup in enumerate(RC.SETUPS):
        for attempt in range(2000):
            d = make_inputs(setup, 1000 * (i + 1) + attempt)
            ok, stats = margins_hold(ref, d, setup)
            if ok:
                break
        else:
            raise RuntimeError(f"{setup['name']}: no seed keeps every pixel away from every decision")
        H, W = setup["H"], setup["W"]
        if setup["empty"]:
            assert stats["inside"] == 0
        else:
            assert 0 < stats["inside"] < H * W and stats["lit"] > 0 and stats["shadowed"] > 0, stats
        if setup["name"] == "outside":
            assert stats["outside_virtual"] > 0 and stats["outside_sun"] > 0, stats
        np.savez_compressed(os.path.join(OUT, f"{setup['name']}_inputs.npz"), **d)
        print(setup["name"], "seed offset", attempt, stats)
        for render_type in RC.RENDER_TYPES:
            for use_gt in (False, True):
                r32 = run(ref, copy.deepcopy(d), render_type, use_gt, torch.float32, setup["empty"])
                r64 = run(ref, copy.deepcopy(d), render_type, use_gt, torch.float64, setup["empty"])
                assert r32.keys() == r64.keys()
                res = {}
                for k in r32:
                    assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64, k
                    delta = r64[k] - r32[k].astype(np.float64)
                    res[k], res[k + "_delta"], res[k + "_d32"] = r32[k], delta.astype(np.float32), np.array(np.abs(delta).max())
                np.savez_compressed(os.path.join(OUT, f"{setup['name']}_{render_type}_gt{int(use_gt)}.npz"), **res)
                print("   ", render_type, "gt" if use_gt else "  ", float(r64["L_alt"]), float(r64["L_rgb"]),
                      {k: float(res[k + "_d32"]) for k in r32})


if __name__ == "__main__":
    main()
