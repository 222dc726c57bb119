"""Generates tests/golden/flow/*.npz by running the REFERENCE's own flow-matching code
(src/gaussiansplatting/flowmatching/flow_matching.py, flow_matching_toaffine.py:11-25, imported from /root/reference) on
seeded CPU inputs. Only inputs, outputs and autograd gradients are stored.

    python tests/golden/make_golden_flow.py

The flow network is not part of the fixtures: `torchvision.models.optical_flow` is a stub and the warper's model is a
stand-in that returns a seeded flow and records the shape it was called with. `flow_matching_toaffine.py` imports the
rasterizer-backed renderer and the dataset stack at module level; both are stubs (only `adjust_affine` is executed).
`perform_flow_matching` reaches `get_flow` with device="cuda": the warper used here forwards device="cpu".
Archives are written with a fixed time stamp, so a second run reproduces them bit for bit.
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

REFROOT = "/root/reference/src/gaussiansplatting"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flow")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_ref():
    tv, tvm, tvo = (types.ModuleType(n) for n in ("torchvision", "torchvision.models", "torchvision.models.optical_flow"))
    tvo.raft_large = tvo.raft_small = None
    tv.models, tvm.optical_flow = tvm, tvo
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.models.optical_flow": tvo})
    sys.path.insert(0, REFROOT)
    pkg = types.ModuleType("flowmatching")
    pkg.__path__ = [os.path.join(REFROOT, "flowmatching")]
    sys.modules["flowmatching"] = pkg
    fm = _load("flowmatching.flow_matching", os.path.join(REFROOT, "flowmatching", "flow_matching.py"))
    gr = types.ModuleType("gaussian_renderer")
    gr.render = None
    cu = types.ModuleType("utils.camera_utils")
    cu.get_list_cam = None
    sys.modules.update({"gaussian_renderer": gr, "utils.camera_utils": cu})
    ta = _load("flowmatching.flow_matching_toaffine", os.path.join(REFROOT, "flowmatching", "flow_matching_toaffine.py"))
    return fm, ta


def save(name, **arrays):
    """np.savez_compressed with a fixed time stamp on every member."""
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB")


def n(t):
    return t.detach().numpy().copy()


def smooth_image(C, H, W, g):
    """A low-frequency image in [0, 1] (so that a sub-pixel shift changes the photometric terms) plus a little noise."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    img = torch.stack([0.5 + 0.25 * torch.sin(0.21 * x + 0.5 * c) * torch.cos(0.17 * y - 0.3 * c) + 0.15 * torch.sin(0.05 * (x + y))
                       for c in range(C)])
    return (img + 0.01 * torch.randn(C, H, W, generator=g)).clamp(0, 1)


def apply_case(fm, name, shape, flow, seed):
    """apply_flow forward and d/d img; `shape` is (C, H, W) or (H, W), `flow` (1, 2, H, W)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(*shape, generator=g)
    if len(shape) == 2:
        img = img * 40 - 10  # an altitude render
    img.requires_grad_(True)
    w = fm.performOpticalmatching(False, device="cpu")
    out = w.apply_flow(img, flow)
    up = torch.randn(*out.shape, generator=g)
    (out * up).sum().backward()
    save("apply_" + name, img=n(img), flow=n(flow), upstream=n(up), out=n(out), g_img=n(img.grad))


def field(H, W, sigma, seed, integer=False):
    f = sigma * torch.randn(1, 2, H, W, generator=torch.Generator().manual_seed(seed))
    return f.round() if integer else f


def constant(H, W, dx, dy):
    f = torch.empty(1, 2, H, W)
    f[0, 0], f[0, 1] = dx, dy
    return f


class StubModel:
    """torchvision RAFT's call shape; returns [zeros, flow] and records what it was given."""

    def __init__(self, flow_fn):
        self.flow_fn, self.calls = flow_fn, []

    def __call__(self, gt, target, num_flow_updates=12):
        self.calls.append((gt.clone(), target.clone(), num_flow_updates))
        f = self.flow_fn(gt.shape[-2], gt.shape[-1])
        return [torch.zeros_like(f), f]


def make_warper(fm, cst, mode, criteria, model):
    class CpuWarper(fm.performOpticalmatching):
        def get_and_apply_flow(self, img_msi_gt, img_msi_target, device="cpu", verbose=False):
            return super().get_and_apply_flow(img_msi_gt, img_msi_target, device="cpu", verbose=verbose)

    w = CpuWarper(cst, mode=mode, device="cpu", model_name="small", num_flow_updates=7, criteria=criteria)
    w._model = model  # on the instance: as a class attribute the callable would bind as a method
    return w


def stats_case(fm):
    w = fm.performOpticalmatching(True, device="cpu")
    arrays = {}
    for k, (H, W, sigma, off, seed) in enumerate([(33, 47, 3.0, (0.4, -1.3), 31), (64, 80, 0.2, (150.0, -90.0), 32), (17, 90, 20.0, (0.0, 0.0), 33)]):
        f = field(H, W, sigma, seed)
        f[0, 0] += off[0]
        f[0, 1] += off[1]
        arrays[f"flow{k}"] = n(f)
        arrays[f"cst{k}"] = n(w.set_cst_displacement(f))
        arrays[f"stats{k}"] = np.array([float(v) for v in w.compute_stats(f)], dtype=np.float32)  # mean x, mean y, std x, std y
        arrays[f"meanabs{k}"] = np.float32(abs(f).mean())  # flow_matching.py:302
    save("stats", **arrays)


def get_flow_case(fm, name, mode, cst, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt, target = torch.rand(C, H, W, generator=g), torch.rand(C, H, W, generator=g)
    model = StubModel(lambda h, w: 2.0 * torch.randn(1, 2, h, w, generator=torch.Generator().manual_seed(seed + 100)))
    w = make_warper(fm, cst, mode, "always", model)
    flows, gt2, target2 = w.get_flow(gt, target, device="cpu")
    (mgt, mtarget, nfu), = model.calls
    save("getflow_" + name, gt=n(gt), target=n(target), model_flow=n(model.flow_fn(*mgt.shape[-2:])), model_gt=n(mgt), model_target=n(mtarget),
         num_flow_updates=np.int32(nfu), flows=n(flows), gt_out=n(gt2), target_out=n(target2), cst=np.bool_(cst))


def perform_case(fm, name, criteria, mode, cst, C, H, W, shift, flow_shift, max_value_flow, seed):
    """The rendered image is the ground truth displaced by `shift` px; the stand-in network answers `flow_shift` (+ noise)."""
    g = torch.Generator().manual_seed(seed)
    gt = smooth_image(C, H, W, g)
    plain = fm.performOpticalmatching(False, device="cpu")
    image = plain.apply_flow(gt, constant(H, W, -shift[0], -shift[1])).detach().clone().requires_grad_(True)

    def flow_fn(h, w):
        f = constant(h, w, *flow_shift)
        return f + 0.05 * torch.randn(1, 2, h, w, generator=torch.Generator().manual_seed(seed + 100))

    warper = make_warper(fm, cst, mode, criteria, StubModel(flow_fn))
    opt = types.SimpleNamespace(flowmatching=types.SimpleNamespace(max_value_flow=max_value_flow))
    flows, gt_out, image_out = fm.perform_flow_matching(opt, warper, image, gt)
    accepted = image_out is not image
    assert accepted or gt_out is gt
    up = torch.randn(*image_out.shape, generator=g)
    (image_out * up).sum().backward()
    hp, wp = warper._model.calls[0][0].shape[-2:]
    save("perform_" + name, gt=n(gt), image=n(image), model_flow=n(flow_fn(hp, wp)), max_value_flow=np.float32(max_value_flow),
         flows=n(flows), gt_out=n(gt_out), image_out=n(image_out), accepted=np.bool_(accepted), upstream=n(up), g_image=n(image.grad),
         cst=np.bool_(cst))
    print(f"  {name}: accepted = {accepted}")


def affine_case(ta):
    g = torch.Generator().manual_seed(71)
    wvt = torch.randn(4, 4, generator=g)
    f = field(33, 47, 2.0, 72)
    f[0, 0] += 1.7
    f[0, 1] -= 0.6
    save("adjust_affine", world_view_transform=n(wvt), flow=n(f), img_W=np.int32(47), img_H=np.int32(33),
         out=n(ta.adjust_affine(wvt.clone(), 47, 33, f)))


def main():
    fm, ta = load_ref()
    apply_case(fm, "field_s3_48x64", (3, 48, 64), field(48, 64, 3.0, 1), 11)
    apply_case(fm, "field_s20_33x47", (3, 33, 47), field(33, 47, 20.0, 2), 12)
    apply_case(fm, "integer_17x90", (2, 17, 90), field(17, 90, 3.0, 3, integer=True), 13)
    apply_case(fm, "cst_subpixel_33x47", (3, 33, 47), constant(33, 47, 0.37, -1.62), 14)
    apply_case(fm, "cst_outside_40x56", (3, 40, 56), constant(40, 56, -70.25, 9.5), 15)
    apply_case(fm, "altitude2d_40x56", (40, 56), field(40, 56, 3.0, 4), 16)
    stats_case(fm)
    get_flow_case(fm, "downscale_37x45", "downscale", False, 3, 37, 45, 41)
    get_flow_case(fm, "upscale_37x45_cst", "upscale", True, 3, 37, 45, 42)
    get_flow_case(fm, "upscale_1plane_40x41", "upscale", False, 1, 40, 41, 43)
    perform_case(fm, "maxflow_accept", "max_value_flow", "upscale", True, 3, 37, 45, (1.4, -0.8), (1.4, -0.8), 3.0, 51)
    perform_case(fm, "maxflow_reject", "max_value_flow", "upscale", True, 3, 37, 45, (1.4, -0.8), (6.0, -5.0), 3.0, 52)
    perform_case(fm, "always_downscale", "always", "downscale", False, 3, 37, 45, (1.4, -0.8), (1.4, -0.8), 3.0, 53)
    perform_case(fm, "lphotom_accept", "l_photom", "upscale", True, 3, 37, 45, (1.4, -0.8), (1.4, -0.8), 3.0, 54)
    perform_case(fm, "lphotom_reject", "l_photom", "upscale", True, 3, 37, 45, (1.4, -0.8), (-1.4, 0.8), 3.0, 55)
    perform_case(fm, "psnr_1plane", "psnr", "upscale", False, 1, 40, 41, (1.4, -0.8), (1.4, -0.8), 3.0, 56)
    affine_case(ta)


if __name__ == "__main__":
    main()
