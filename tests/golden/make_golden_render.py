"""Generates tests/golden/render/*.npz by running the REFERENCE's own `render()` (gaussian_renderer/renderer.py) on a
`GaussianModel` (scene/gaussian_model.py) whose raw parameters are set directly. Build container only: it imports the
reference from REFROOT. Only inputs, outputs and autograd gradients are stored.

    python tests/golden/make_golden_render.py [--out DIR] [case names: default all]

A fixture whose arrays are unchanged is not rewritten (a zip archive carries its write time).

What runs is the reference's Python: the activations (`get_opacity`, `get_scaling`, `get_rotation`: sigmoid, exp,
F.normalize), `SH2RGB`, `AffineCamera.ECEF_to_UVA` (called unbound on a namespace that carries the camera's attributes,
as make_golden_shade.py calls `render_pipeline`), the `learn_wv_only_lastparam` offset of the view matrix, the
reference's rasterizer wrapper (`diff_gaussian_rasterization/__init__.py`) and autograd through all of it. Below the
wrapper's `_C` the CPU oracle rasterizes activated inputs (make_golden.py's `stub_forward` / `stub_backward`), so these
vectors pin every raw-parameter front end of this project (the oracle's RAW mode, the HIP RAW path, tests/util.py's
unfused helpers) to the reference's own formulation of it.

Stubs: `plyfile`, `simple_knn._C` (neither is installed here, and `GaussianModel` imports them at module level) and
`arguments` (`GroupParams` is all gaussian_model.py needs; the real module pulls in hydra and omegaconf). The packages
`scene` and `gaussian_renderer` are bound to their directories without executing their `__init__.py` (those import the
dataset readers).

Device: the reference creates the screen-space leaf with `device="cuda"` (renderer.py:32-36). While a case runs,
`torch.zeros_like` is wrapped so that a `device="cuda"` argument means the CPU, in this process only; nothing else is
redirected and no reference file is changed.

The world-to-view matrix is made a leaf that requires a gradient (the reference's `learn_wv_transform` branch holds it
as a Parameter, affine_cameras.py:205-211), so the whole camera gradient `g_viewmatrix` is recorded beside `last_row`'s.

Not covered: `use_trained_exp`. renderer.py:112-120 multiplies the [H, W, 5] permuted render by a 3x3 exposure matrix,
which fails for the five-channel features this model renders.
"""
import argparse
import contextlib
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFROOT = "/root/reference/src/gaussiansplatting"
OUT = os.path.join(HERE, "render")
sys.path[:0] = [ROOT, os.path.dirname(HERE), HERE]  # the package, tests/util.py, make_golden.py

# case: P, H, W, seed, scale_mult, antialiasing, learn_wv_only_lastparam, scaling_modifier, extra
CASES = {
    "aa_learn_61x83": dict(P=1000, H=61, W=83, seed=41, scale_mult=2.0, aa=True, learn=True),
    "noaa_fixed_47x70": dict(P=900, H=47, W=70, seed=42, scale_mult=2.5, aa=False, learn=False),
    "modifier0p7_55x38": dict(P=700, H=55, W=38, seed=43, scale_mult=3.0, aa=True, learn=True, modifier=0.7),
    # the altitude axis of `affine` differs from the view matrix's third column, not only its offset
    "affine_tilted_50x66": dict(P=800, H=50, W=66, seed=44, scale_mult=2.0, aa=False, learn=True, tilt=True),
    # Gaussians spread 1.6x beyond the view: culled (radius 0) and partly off-screen ones
    "offscreen_45x77": dict(P=900, H=45, W=77, seed=45, scale_mult=2.0, aa=False, learn=False, xyz_mult=1.6),
    # saturated opacity logits, extreme log-scales, raw quaternions of norm 1e-3 and 1e3, negative scalar parts
    "edges_41x53": dict(P=300, H=41, W=53, seed=46, scale_mult=3.0, aa=True, learn=True, edges=True),
    # raw quaternions below F.normalize's eps. Their own fixture: dL/dq / eps is ~1e5 x every other row's rotation gradient, and
    # in one case with the edge rows it would set the scale that all of g_raw_rotation is measured against
    "subeps_29x23": dict(P=80, H=29, W=23, seed=47, scale_mult=3.0, aa=False, learn=True, subeps=True),
}

# rows of the edges case (the rest of its Gaussians are an ordinary scene)
EDGE_LOGITS = {0: 20.0, 1: 25.0, 2: -90.0, 3: -100.0, 4: 16.0}
EDGE_LOG_SCALE_SHIFT = {5: 3.0, 6: -9.0, 7: 2.5, 8: -6.0}
EDGE_QUAT_NORM = {9: 1e-3, 10: 1e3, 11: 3e-4, 12: 3e3, 13: 1e-3, 14: 1e3}
EDGE_QUAT_NEG = (15, 16, 11, 13)  # negative scalar part (q and -q are the same rotation; the raw gradient differs in sign)
SUBEPS_QUAT_NORM = {0: 1e-13, 1: 5e-14, 2: 9e-13, 3: 1e-13}
SUBEPS_QUAT_NEG = (1, 3)


def _stub_modules():
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = object
    sys.modules["plyfile"] = ply
    knn = types.ModuleType("simple_knn")
    knn.__path__ = []
    knn_c = types.ModuleType("simple_knn._C")
    knn_c.distCUDA2 = None
    sys.modules["simple_knn"], sys.modules["simple_knn._C"] = knn, knn_c
    args = types.ModuleType("arguments")

    class GroupParams:
        pass

    args.GroupParams = GroupParams
    sys.modules["arguments"] = args
    for name in ("scene", "gaussian_renderer", "scene.cameras"):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REFROOT, *name.split("."))]
        sys.modules[name] = pkg


def load_reference():
    """(renderer module, GaussianModel class, AffineCamera class) of the reference, over the oracle-backed wrapper."""
    import make_golden  # the reference wrapper with `_C` stubbed over the CPU oracle

    dgr = make_golden.load_reference_wrapper()
    sys.path.insert(0, REFROOT)
    _stub_modules()
    sys.modules["diff_gaussian_rasterization"] = dgr
    for m in ("utils.general_utils", "utils.sh_utils", "utils.graphics_utils", "utils.system_utils"):
        importlib.import_module(m)
    gm = importlib.import_module("scene.gaussian_model")
    renderer = importlib.import_module("gaussian_renderer.renderer")
    spec = importlib.util.spec_from_file_location("ref_affine_cameras", os.path.join(REFROOT, "scene/cameras/affine_cameras.py"))
    cams = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cams)
    return renderer, gm.GaussianModel, cams.AffineCamera


@contextlib.contextmanager
def cuda_means_cpu():
    orig = torch.zeros_like

    def zeros_like(t, *a, **k):
        if str(k.get("device", "")).startswith("cuda"):
            k["device"] = "cpu"
        return orig(t, *a, **k)

    torch.zeros_like = zeros_like
    try:
        yield
    finally:
        torch.zeros_like = orig


def case_inputs(cfg):
    """The raw parameters, camera matrices and upstream gradient of one case (float32 numpy)."""
    from eogs2_amd.synthetic import make_scene
    from util import raw_params_from_scene

    P, H, W, seed = cfg["P"], cfg["H"], cfg["W"], cfg["seed"]
    sc = make_scene(P, H, W, seed=seed, opacity="trained", scale_mult=cfg["scale_mult"])
    if cfg.get("xyz_mult"):
        sc["means3D"] = (sc["means3D"] * torch.tensor([cfg["xyz_mult"], cfg["xyz_mult"], 1.0])).contiguous()
    raw, _ = raw_params_from_scene(sc, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    vm = sc["viewmatrix"].clone()
    affine = vm.clone()
    affine[3, 2] += 0.125
    if cfg.get("tilt"):
        affine[:3, 2] += torch.tensor([0.04, -0.03, 0.15])
    logit, log_s, rot = raw["opacity_logit"].clone(), raw["log_scaling"].clone(), raw["raw_rotation"].clone()
    if cfg.get("subeps"):
        for i, n in SUBEPS_QUAT_NORM.items():
            rot[i] = rot[i] / rot[i].norm() * n
        for i in SUBEPS_QUAT_NEG:
            if rot[i, 0] > 0:
                rot[i] = -rot[i]
    if cfg.get("edges"):
        for i, v in EDGE_LOGITS.items():
            logit[i] = v
        for i, v in EDGE_LOG_SCALE_SHIFT.items():
            log_s[i] += v
        for i, n in EDGE_QUAT_NORM.items():
            rot[i] = rot[i] / rot[i].norm() * n
        for i in EDGE_QUAT_NEG:
            if rot[i, 0] > 0:
                rot[i] = -rot[i]
    last_row = (0.02 * torch.randn(4, generator=g)) if cfg["learn"] else torch.zeros(4)
    d = dict(H=np.int32(H), W=np.int32(W), antialiasing=np.bool_(cfg["aa"]), learn_wv_only_lastparam=np.bool_(cfg["learn"]),
             scaling_modifier=np.float32(cfg.get("modifier", 1.0)), FoVx=np.float32(1.0), FoVy=np.float32(1.0),
             xyz=raw["xyz"], f_dc=raw["f_dc"], opacity_logit=logit, log_scaling=log_s, raw_rotation=rot,
             viewmatrix=vm, affine=affine, last_row=last_row.float(), bg=sc["bg"],
             dL_drender=torch.randn(5, H, W, generator=g) / (H * W))
    return {k: (v.detach().float().contiguous().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def run_reference(ref, d):
    """The reference's render() + backward on the inputs `d`: {output name: numpy}."""
    renderer, GaussianModel, AffineCamera = ref
    t = lambda k: torch.from_numpy(np.array(d[k], copy=True))
    leaf = lambda k: torch.nn.Parameter(t(k))
    pc = GaussianModel(0)
    pc._xyz, pc._features_dc, pc._opacity = leaf("xyz"), leaf("f_dc"), leaf("opacity_logit")
    pc._scaling, pc._rotation = leaf("log_scaling"), leaf("raw_rotation")
    pc._features_rest = torch.nn.Parameter(torch.zeros(pc._xyz.shape[0], 0, 3))
    learn = bool(d["learn_wv_only_lastparam"])
    wvt = t("viewmatrix").requires_grad_(True)
    cam = types.SimpleNamespace(FoVx=float(d["FoVx"]), FoVy=float(d["FoVy"]), world_view_transform=wvt, full_proj_transform=wvt.detach(),
                                learn_wv_only_lastparam=learn, last_row=t("last_row").requires_grad_(learn),
                                image_height=int(d["H"]), image_width=int(d["W"]), camera_center=torch.zeros(3), affine=t("affine"))
    cam.ECEF_to_UVA = types.MethodType(AffineCamera.ECEF_to_UVA, cam)
    pipe = types.SimpleNamespace(debug=False, antialiasing=bool(d["antialiasing"]), compute_cov3D_python=False, require_radii=True)
    with cuda_means_cpu():
        out = renderer.render(cam, pc, pipe, t("bg"), scaling_modifier=float(d["scaling_modifier"]))
    (out["render"] * t("dL_drender")).sum().backward()
    res = dict(render=out["render"], radii=out["radii"], visibility_filter=out["visibility_filter"],
               g_viewspace_points=out["viewspace_points"].grad, g_xyz=pc._xyz.grad, g_f_dc=pc._features_dc.grad,
               g_opacity_logit=pc._opacity.grad, g_log_scaling=pc._scaling.grad, g_raw_rotation=pc._rotation.grad,
               g_viewmatrix=wvt.grad)
    if learn:
        res["g_last_row"] = cam.last_row.grad
    return {k: v.detach().contiguous().numpy() for k, v in res.items()}


def unchanged(path, d):
    if not os.path.exists(path):
        return False
    z = np.load(path)
    return sorted(z.files) == sorted(d) and all(
        z[k].dtype == np.asarray(d[k]).dtype and np.array_equal(z[k], d[k], equal_nan=z[k].dtype.kind == "f") for k in d)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    torch.set_num_threads(1)  # (CPU reductions the same on every run)
    ref = load_reference()
    os.makedirs(a.out, exist_ok=True)
    for name, cfg in CASES.items():
        if a.cases and name not in a.cases:
            continue
        d = case_inputs(cfg)
        d.update(run_reference(ref, d))
        path = os.path.join(a.out, name + ".npz")
        if unchanged(path, d):
            print(f"{name}: unchanged")
            continue
        np.savez_compressed(path, **d)
        vis = int((d["radii"] > 0).sum())
        print(f"{name}: P={cfg['P']} {cfg['H']}x{cfg['W']} visible={vis} -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
