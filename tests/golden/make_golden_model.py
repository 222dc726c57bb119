"""Generates tests/golden/model/*.npz by running the REFERENCE's own `GaussianModel.create_from_pcd`
(scene/gaussian_model.py:159-221) on the CPU. Build machine only: it imports the reference through
make_golden_render.load_reference(). Only data is stored.

    python tests/golden/make_golden_model.py [--out DIR] [case names: default all]

A fixture whose arrays are unchanged is not rewritten.

What runs is the reference's Python, unmodified. Device: the reference allocates with `device="cuda"` and calls `.cuda()`.
While a case runs, `torch.zeros`, `zeros_like`, `ones`, `tensor` and `eye` answer such a request on the CPU (the
`cuda_means_cpu` of make_golden_optim.py) and `Tensor.cuda()` returns the tensor, in this process only. `distCUDA2` (a CUDA
extension) is replaced by a brute-force 3-NN in float64 that returns fp32: the mean of the three smallest squared distances
to the OTHER points, coincident points counting as neighbours at distance 0, as simple-knn counts them.

Stored per case: the points, the colours, `dist2` (what the stand-in returned: before the clamp) and every tensor the reference
made, and beside `f_dc` and `scaling` the same formula in float64 from the fp32 inputs (`@64`). The generator prints the
largest distance between the reference's fp32 result and float64: the yardstick of tests/test_gpu_model.py.

`api.npz` holds the public names of the reference's class with their parameters (name, default), read with
`inspect.signature`: what tests/test_model_api.py holds `eogs2_amd.model.GaussianModel` to.
"""
import argparse
import contextlib
import inspect
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import make_golden_optim as mgo  # noqa: E402
import make_golden_render as mgr  # noqa: E402

OUT = os.path.join(HERE, "model")
C0 = 0.28209479177387814
MAX_FIXTURE_BYTES = 200 * 1024

# case: sh, P, seed, kind
CASES = {
    "sh0_1000": dict(sh=0, P=1000, seed=51, kind="box"),
    "sh1_257": dict(sh=1, P=257, seed=52, kind="box"),
    # coincident and nearly coincident points: dist2 == 0 and 0 < dist2 < 1e-7 both hit the clamp of gaussian_model.py:179-182
    "duplicates_300": dict(sh=0, P=300, seed=53, kind="duplicates"),
}
OPACITY_INIT = {"sh0_1000": 0.01, "sh1_257": 0.1, "duplicates_300": 0.01}  # (train.yaml's init_opacity varies per scene)
N_CAMERAS = 3


def case_inputs(cfg):
    g = np.random.default_rng(cfg["seed"])
    P = cfg["P"]
    pts = g.uniform(-1.0, 1.0, (P, 3))
    if cfg["kind"] == "duplicates":
        pts[40:80] = pts[0:40]          # pairs: one neighbour at distance 0
        pts[80:120] = pts[0:40]         # ... triples
        pts[120:160] = pts[0:40]        # ... quadruples: all three neighbours at distance 0, dist2 == 0
        pts[160:200] = pts[200:240] + g.uniform(-1e-4, 1e-4, (40, 3))  # near-coincident clusters below ...
        pts[240:260] = pts[200:220] + g.uniform(-1e-4, 1e-4, (20, 3))
        pts[260:280] = pts[200:220] + g.uniform(-1e-4, 1e-4, (20, 3))  # ... 0 < dist2 < 1e-7
    cols = g.uniform(0.0, 1.0, (P, 3))
    cols[:4] = [[0.0, 1.0, 0.5], [1.0, 0.0, 0.5], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]]
    return pts.astype(np.float32), cols.astype(np.float32)


def brute_dist2(points):
    """float32 [P]: mean squared distance to the three nearest other points, in float64 from the fp32 coordinates."""
    p = points.detach().cpu().numpy().astype(np.float64)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    d[np.arange(len(p)), np.arange(len(p))] = np.inf
    return torch.from_numpy(np.sort(d, axis=1)[:, :3].mean(axis=1).astype(np.float32))


@contextlib.contextmanager
def no_device(gm):
    """cuda_means_cpu + Tensor.cuda() + the stand-in for distCUDA2, for the duration of one create_from_pcd."""
    cuda, dist = torch.Tensor.cuda, gm.distCUDA2
    recorded = []

    def dist_fn(points):
        recorded.append(brute_dist2(points))
        return recorded[-1].clone()

    torch.Tensor.cuda = lambda self, *a, **k: self
    gm.distCUDA2 = dist_fn
    try:
        with mgo.cuda_means_cpu():
            yield recorded
    finally:
        torch.Tensor.cuda, gm.distCUDA2 = cuda, dist


def run_case(GaussianModel, gm, name, cfg):
    pts, cols = case_inputs(cfg)
    m = GaussianModel(cfg["sh"])
    cams = [types.SimpleNamespace(image_name=f"view_{k}") for k in range(N_CAMERAS)]
    with no_device(gm) as recorded, contextlib.redirect_stdout(io.StringIO()):
        m.create_from_pcd(types.SimpleNamespace(points=pts, colors=cols), cams, 2.5, OPACITY_INIT[name])
    assert len(recorded) == 1
    dist2 = recorded[0].numpy()
    d = {"points": pts, "colors": cols, "dist2": dist2, "sh": np.int32(cfg["sh"]), "opacity_init": np.float64(OPACITY_INIT[name]),
         "xyz": m._xyz, "f_dc": m._features_dc, "f_rest": m._features_rest, "scaling": m._scaling, "rotation": m._rotation,
         "opacity": m._opacity, "max_radii2D": m.max_radii2D, "exposure": m._exposure}
    d = {k: (v.detach().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    for k in ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity", "max_radii2D", "exposure"):
        assert d[k].dtype == np.float32, (k, d[k].dtype)
    assert m.spatial_lr_scale == 2.5 and m.exposure_mapping == {f"view_{k}": k for k in range(N_CAMERAS)}
    # the float64 formulas from the fp32 inputs
    d["f_dc@64"] = ((cols.astype(np.float64) - 0.5) / C0).reshape(-1, 1, 3)
    clamped = np.maximum(dist2.astype(np.float64), np.float64(np.float32(0.0000001)))
    d["scaling@64"] = np.repeat(np.log(np.sqrt(clamped))[:, None], 3, axis=1)
    return d


def own_error(d, key):
    """Largest |fp32 - float64| of the reference's own result."""
    return float(np.abs(d[key].astype(np.float64) - d[key + "@64"]).max())


def public_api(GaussianModel):
    """{name: "property" | [[parameter, default repr or None], ...]} of every public name of the class."""
    api = {}
    for name, obj in sorted(vars(GaussianModel).items()):
        if name.startswith("_") and name != "__init__":
            continue
        if isinstance(obj, property):
            api[name] = "property"
        elif callable(obj):
            api[name] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                         for p in inspect.signature(obj).parameters.values()]
    return api


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    torch.set_num_threads(1)
    _, GaussianModel, _ = mgr.load_reference()
    gm = sys.modules["scene.gaussian_model"]
    os.makedirs(a.out, exist_ok=True)
    for name, cfg in CASES.items():
        if a.cases and name not in a.cases:
            continue
        d = run_case(GaussianModel, gm, name, cfg)
        below = int((d["dist2"] < np.float32(0.0000001)).sum())
        print(f"{name}: P {cfg['P']} sh {cfg['sh']}; dist2 below the clamp on {below} rows ({int((d['dist2'] == 0).sum())} exactly 0); "
              f"reference fp32 against float64: f_dc {own_error(d, 'f_dc'):.3e}, scaling {own_error(d, 'scaling'):.3e}")
        path = os.path.join(a.out, name + ".npz")
        if mgr.unchanged(path, d):
            print(f"{name}: unchanged")
            continue
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < MAX_FIXTURE_BYTES, (name, size)
        print(f"{name}: -> {size / 1024:.0f} KiB")
    if not a.cases or "api" in a.cases:
        d = {"api": np.array(json.dumps(public_api(GaussianModel), sort_keys=True))}
        path = os.path.join(a.out, "api.npz")
        if mgr.unchanged(path, d):
            print("api: unchanged")
        else:
            np.savez_compressed(path, **d)
            print(f"api: {len(json.loads(str(d['api'])))} public names -> {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
