"""Generates tests/golden/report/*.npz by running the REFERENCE's own functions, imported at run time from the reference's
checkout (build container only), on the CPU, over duck-typed scene and camera stand-ins:

    utils/save_utils.py                normalize_before_saving
    utils/convert_color_correction.py  load_convert_color_correction_train_to_test("ref" | "average").perform_cc_to_test
    utils/image_utils.py               psnr
    utils/loss_utils.py                l1_loss

    python tests/golden/make_golden_report.py

`utils` is a stub package whose `__path__` points into the reference, so that nothing but the four modules above (and
sh_utils.py under save_utils) is read; `utils.camera_utils`, which pulls the dataset readers, is replaced by a module that
holds `get_list_cam` alone (this package's own: MSI camera, then PAN camera). The inputs are the seeded ones of
tests/report_cases.py, which the tests build again; each fixture stores their sha256 beside the recorded results, and the small
ones themselves. Only arrays and strings are stored.

    align_<case>.npz   weights, biases, ref; f_dc_out, weights_out, biases_out as normalize_before_saving leaves them
    convert.npz        per camera list and converter the test cameras' weights and biases
    metrics.npz        per case `l1_loss(image, clamp(gt)).mean()` and `psnr(image, clamp(gt)).mean()` as fp32
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
import report_cases as RC  # noqa: E402


def get_list_cam(viewpoint_cam, opt):
    out = []
    if opt.load_msi:
        out.append(viewpoint_cam.get_msi_cameras())
    if opt.load_pan:
        out.append(viewpoint_cam.get_pan_cameras())
    return out


def load_ref():
    pkg = types.ModuleType("utils")
    pkg.__path__ = [os.path.join(REFROOT, "utils")]
    sys.modules["utils"] = pkg
    stub = types.ModuleType("utils.camera_utils")
    stub.get_list_cam = get_list_cam
    sys.modules["utils.camera_utils"] = stub
    return types.SimpleNamespace(save=importlib.import_module("utils.save_utils"), convert=importlib.import_module("utils.convert_color_correction"),
                                 image=importlib.import_module("utils.image_utils"), loss=importlib.import_module("utils.loss_utils"))


def camera(weight, bias, kind="msi", is_ref=False):
    conv = torch.nn.Conv2d(3, 3, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(weight))
        conv.bias.copy_(torch.from_numpy(bias))
    return types.SimpleNamespace(color_correction=conv, image_type=kind, is_reference_camera=is_ref)


def viewpoint(msi, pan=None, is_ref=False):
    return types.SimpleNamespace(is_reference_camera=is_ref, get_msi_cameras=lambda: msi, get_pan_cameras=lambda: pan)


def make_align(ref):
    for case in RC.align_cases():
        d = RC.align_inputs(case)
        V = d["weights"].shape[0]
        views = [viewpoint(camera(d["weights"][v], d["biases"][v]), is_ref=(v == d["ref"])) for v in range(V)]
        scene = types.SimpleNamespace(getTrainCameras=lambda: views)
        gaussians = types.SimpleNamespace(_features_dc=torch.nn.Parameter(torch.from_numpy(d["f_dc"].copy())))
        with torch.no_grad():
            ref.save.normalize_before_saving(scene, gaussians)
        out = gaussians._features_dc.detach().numpy()
        w_out = np.stack([v.get_msi_cameras().color_correction.weight.detach().numpy() for v in views])
        b_out = np.stack([v.get_msi_cameras().color_correction.bias.detach().numpy() for v in views])
        assert out.dtype == np.float32 and w_out.dtype == np.float32 and w_out.shape == d["weights"].shape
        f64, bound = RC.rows_float64(d["f_dc"], d["weights"][d["ref"]], d["biases"][d["ref"]])
        worst = float((np.abs(out - f64) / bound).max() * 8)
        worst_cc = 0.0
        for v in range(V):
            R, rb, magA, magb = RC.recompose_float64(d["weights"][v], d["biases"][v], d["weights"][d["ref"]], d["biases"][d["ref"]])
            worst_cc = max(worst_cc, float((np.abs(w_out[v].reshape(3, 3) - R) / (RC.U * magA)).max()),
                           float((np.abs(b_out[v] - rb) / (RC.U * magb)).max()))
        print(f"align {case['name']}: rows reach {worst:.2f} of 8 roundings, corrections {worst_cc:.2f} of 8")
        np.savez_compressed(os.path.join(RC.GOLDEN, f"align_{case['name']}.npz"), weights=d["weights"], biases=d["biases"], ref=np.array(d["ref"]),
                            f_dc_sha=np.array(RC.sha(d["f_dc"])), f_dc_out=out, weights_out=w_out, biases_out=b_out)


def make_convert(ref):
    d = RC.convert_inputs()
    res = {}
    opt = types.SimpleNamespace(load_msi=True, load_pan=True)
    for name in ("ref", "average"):
        def cams(kind, prefix, is_ref_at=None):
            w, b = d[kind][prefix + "weights"], d[kind][prefix + "biases"]
            return [camera(w[v], b[v], kind, is_ref=(v == is_ref_at)) for v in range(w.shape[0])]
        train = [viewpoint(m, p) for m, p in zip(cams("msi", "", d["ref"]), cams("pan", "", d["ref"]))]
        test = [viewpoint(m, p) for m, p in zip(cams("msi", "test_"), cams("pan", "test_"))]
        ref.convert.load_convert_color_correction_train_to_test(name).perform_cc_to_test(train, test, opt)
        for kind, get in (("msi", "get_msi_cameras"), ("pan", "get_pan_cameras")):
            res[f"{name}_{kind}_weights"] = np.stack([getattr(v, get)().color_correction.weight.detach().numpy() for v in test])
            res[f"{name}_{kind}_biases"] = np.stack([getattr(v, get)().color_correction.bias.detach().numpy() for v in test])
    for kind in ("msi", "pan"):
        for k, v in d[kind].items():
            res[f"in_{kind}_{k}"] = v
    np.savez_compressed(os.path.join(RC.GOLDEN, "convert.npz"), ref=np.array(d["ref"]), **res)
    print("convert: ref and average over", {k: d[k]["weights"].shape[0] for k in ("msi", "pan")}, "train cameras")


def make_metrics(ref):
    res = {}
    for shape, content in RC.metric_cases():
        image, gt = RC.metric_inputs(shape, content)
        name = RC.metric_name(shape, content)
        ti, tg = torch.from_numpy(image), torch.clamp(torch.from_numpy(gt), 0.0, 1.0)  # train_pan.py:917
        l1 = ref.loss.l1_loss(ti, tg).mean()
        ps = ref.image.psnr(ti, tg).mean()
        assert l1.dtype == torch.float32 and ps.dtype == torch.float32
        res[name + "_l1"], res[name + "_psnr"] = l1.numpy().copy(), ps.numpy().copy()
        res[name + "_sha"] = np.array(RC.sha(image, gt))
        if image.size <= 4096:
            res[name + "_image"], res[name + "_gt"] = image, gt
        print(f"metrics {name}: L1 {float(l1):.9g} PSNR {float(ps):.9g}; float64", *RC.metrics_float64(image, gt))
    np.savez_compressed(os.path.join(RC.GOLDEN, "metrics.npz"), **res)


def main():
    ref = load_ref()
    os.makedirs(RC.GOLDEN, exist_ok=True)
    make_align(ref)
    make_convert(ref)
    make_metrics(ref)


if __name__ == "__main__":
    main()
