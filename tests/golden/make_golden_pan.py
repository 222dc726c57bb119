"""Generates tests/golden/pan/*.npz by running the REFERENCE's own `PANAffineCamera._render_pipeline` and
`_render_pipeline_weird` with the maps of its own `load_msi_to_pan`, imported at run time from the reference's checkout
(build container only). Only arrays and strings are stored: inputs, parameters, upstream gradients, outputs and the
autograd gradients of every input and Parameter. The layout is described in tests/pan_cases.py, whose `make_case` seeds
the inputs.

    python tests/golden/make_golden_pan.py

The two methods are called unbound on a plain namespace carrying the attributes they read (the class's constructor
needs the dataset stack). `scene`, `scene.cameras` and `scene.msi_to_pan` are stub packages in sys.modules whose
`__path__` points into the reference, so that `scene/__init__.py` (which pulls the dataset readers) never runs.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_golden_shade import REFROOT  # noqa: E402  (where the reference's sources are read from)
import pan_cases  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pan")


def load_ref():
    for name, sub in (("scene", "scene"), ("scene.cameras", "scene/cameras"), ("scene.msi_to_pan", "scene/msi_to_pan")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REFROOT, sub)]
        sys.modules[name] = pkg
    pan = importlib.import_module("scene.cameras.PAN_affine_cameras")
    aff = importlib.import_module("scene.cameras.affine_cameras")
    maps = importlib.import_module("scene.msi_to_pan.transf_msi_to_pan")
    return pan, aff, maps


def build_map(maps, c):
    """The reference's module for the case, its tensors set to the case's values; {fixture name: Parameter}."""
    cfg = types.SimpleNamespace(name=c["map"], msi_channels=3, pan_channels=1, kernel_size=1, remove_sigm=bool(c["remove_sigm"]),
                                init_value=False, use_avgpool=False)
    mod = maps.load_msi_to_pan(cfg)
    leaves = {}
    with torch.no_grad():
        if c["map"] in ("fixed", "learnable_fixed"):
            mod.pan_params.copy_(torch.from_numpy(c["map_params"]))
        elif c["map"] in ("base", "fixedandtranslate"):
            mod.linear.weight.copy_(torch.from_numpy(c["map_weight"]).reshape(1, 3, 1, 1))
            mod.linear.bias.copy_(torch.from_numpy(c["map_bias"]))
        if c["map"] == "fixedandtranslate":
            mod.fixed_weights.copy_(torch.from_numpy(c["map_fixed_weights"]).reshape(1, 3, 1, 1))
            mod.fixed_bias.copy_(torch.from_numpy(c["map_fixed_bias"]))
    if c["map"] == "learnable_fixed" and c["unfrozen"]:
        leaves["map_params"] = mod.pan_params
    if c["map"] == "base":
        leaves.update(map_weight=mod.linear.weight, map_bias=mod.linear.bias)
    if c["map"] == "fixedandtranslate" and c["learn_conv2d"]:
        leaves.update(map_weight=mod.linear.weight, map_bias=mod.linear.bias)
    return mod, leaves


def run_case(ref, c):
    pan, aff, maps = ref
    cam = types.SimpleNamespace(use_cc=False, use_exposure=False, use_shadow="alt_diff" in c, shadow_map=aff.ShadowMap(), mode="pan")
    cam.msi_to_pan, leaves = build_map(maps, c)
    if c["map"] in ("learnable_fixed", "fixedandtranslate") and (c["unfrozen"] if c["map"] == "learnable_fixed" else c["learn_conv2d"]):
        pan.PANAffineCamera.unfreeze_msi_to_pan(cam)  # train_pan.py:259-265
    M = torch.from_numpy(c["M"])
    assemble_M = None
    if c["order"] == "A":
        if c["cc_mode"] == "cc":
            cam.use_cc = True
            cam.color_correction = torch.nn.Conv2d(3, 3, 1, bias=True)
            with torch.no_grad():
                cam.color_correction.weight.copy_(M[:, :3].reshape(3, 3, 1, 1))
                cam.color_correction.bias.copy_(M[:, 3])
            assemble_M = lambda: torch.cat([cam.color_correction.weight.grad.reshape(3, 3),  # noqa: E731
                                            cam.color_correction.bias.grad.reshape(3, 1)], dim=1)
        elif c["cc_mode"] == "exposure":
            cam.use_exposure = True
            cam.exposure = torch.nn.Parameter(M[None].clone())
            assemble_M = lambda: cam.exposure.grad[0]  # noqa: E731
        cam.inshadow_color_correction = torch.nn.Parameter(torch.from_numpy(c["ins"]).reshape(3, 1, 1).clone())
        fn = pan.PANAffineCamera._render_pipeline
    else:
        cam.color_correction = torch.nn.Conv2d(1, 1, 1, bias=True)
        with torch.no_grad():
            cam.color_correction.weight.copy_(M[0].reshape(1, 1, 1, 1))
            cam.color_correction.bias.copy_(M[1].reshape(1))
        assemble_M = lambda: torch.cat([cam.color_correction.weight.grad.reshape(1), cam.color_correction.bias.grad.reshape(1)])  # noqa: E731
        cam.inshadow_color_correction = torch.nn.Parameter(torch.from_numpy(c["ins"]).reshape(1, 1, 1).clone())
        fn = pan.PANAffineCamera._render_pipeline_weird
    raw = torch.from_numpy(c["raw"]).clone().requires_grad_(True)
    alt = torch.from_numpy(c["alt_diff"]).clone().requires_grad_(True) if "alt_diff" in c else None
    out = fn(cam, raw_render=raw, sun_altitude_diff=alt)
    assert out["final"] is out["shaded"] or torch.equal(out["final"], out["shaded"])
    res = dict(c)
    res["out_cc"], res["out_shaded"] = out["cc"].detach().numpy(), out["shaded"].detach().numpy()
    L = (out["cc"] * torch.from_numpy(c["g_cc"])).sum()
    res["shaded_requires_grad"] = np.array(int(out["shaded"].requires_grad))
    if out["shaded"].requires_grad:
        L = L + (out["shaded"] * torch.from_numpy(c["g_shaded"])).sum()
    if alt is not None:
        res["out_shadow"] = out["shadowmap"].detach().numpy()
        L = L + (out["shadowmap"] * torch.from_numpy(c["g_shadow"])).sum()
    else:
        assert out["shadowmap"] is None
    L.backward()
    if raw.grad is not None:
        res["grad_raw"] = raw.grad.numpy()
    if alt is not None:
        res["grad_alt_diff"] = alt.grad.numpy()
        if cam.inshadow_color_correction.grad is not None:
            res["grad_ins"] = cam.inshadow_color_correction.grad.reshape(-1).numpy()
    if assemble_M is not None:
        res["grad_M"] = assemble_M().numpy()
    for name, leaf in leaves.items():
        if leaf.grad is not None:
            res["grad_" + name] = leaf.grad.reshape(-1).numpy()
    return res


# (fixture name, order, map of pan_cases.MAPS or identity, H, W, shadow, cc_mode, unfrozen)
# 33 x 65 (several workgroups' worth of lanes, an odd pixel count) where the most sums are reduced, 5 x 7 elsewhere
BIG = ("A_learnable_fixed", "B_base")
CASES = [(f"A_{m}", "A", m, *((33, 65) if f"A_{m}" in BIG else (5, 7)), True, "cc", True) for m in pan_cases.MAPS + ("identity",)]
CASES += [(f"B_{m}", "B", m, *((33, 65) if f"B_{m}" in BIG else (5, 7)), True, "cc", True) for m in pan_cases.MAPS]
CASES += [
    ("A_learnable_fixed_frozen", "A", "learnable_fixed", 5, 7, True, "cc", False),
    ("B_learnable_fixed_frozen", "B", "learnable_fixed", 5, 7, True, "cc", False),
    ("A_fixed_exposure", "A", "fixed", 5, 7, True, "exposure", True),
    ("A_base_exposure_noshadow", "A", "base", 5, 7, False, "exposure", True),
    ("A_fixed_nocc", "A", "fixed", 5, 7, True, "none", True),
    ("A_average_noshadow", "A", "average", 33, 65, False, "cc", True),
    ("B_fixed_noshadow", "B", "fixed", 33, 65, False, "cc", True),  # shaded is the map's result, not cc
    ("B_base_noshadow", "B", "base", 5, 7, False, "cc", True),
    ("B_fixedandtranslate_frozen_noshadow", "B", "fixedandtranslate_frozen", 5, 7, False, "cc", True),
]


def main():
    ref = load_ref()
    os.makedirs(OUT, exist_ok=True)
    for i, (name, order, m, H, W, shadow, cc_mode, unfrozen) in enumerate(CASES):
        c = pan_cases.make_case(order, m, H, W, shadow=shadow, cc_mode=cc_mode, unfrozen=unfrozen, seed=100 + i)
        res = run_case(ref, c)
        if m == "base":  # the sigmoid must see both signs
            x = res["raw"].astype(np.float64)
            w, b = res["map_weight"].astype(np.float64), float(res["map_bias"][0])
            z = np.tensordot(w, x, 1) + b
            assert (z > 0.2).any() and (z < -0.2).any(), name
        if shadow:
            assert (res["alt_diff"] == 0).sum() >= 3 and res["grad_alt_diff"][res["alt_diff"] == 0].any(), name
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **{k: np.asarray(v) for k, v in res.items()})
        print(name, {k: tuple(np.shape(v)) for k, v in res.items() if k.startswith(("out_", "grad_"))})


if __name__ == "__main__":
    main()
