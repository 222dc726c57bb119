"""Generates tests/golden/nll/*.npz on the CPU: the reference's two statements (train_pan.py:434-440)

    betaprime = (cam.transient_mask.clip(0, 1) + 1e-3).square()
    L_nll = torch.nn.functional.gaussian_nll_loss(input=image, target=gt_image, var=betaprime.unsqueeze(0).repeat(C, 1, 1))

with torch's own gaussian_nll_loss and autograd on the seeded inputs of tests/nll_cases.py, once in float32 and once in
float64 on the same float32-rounded inputs; for the direct-variance cases the second statement alone (a variance shared by the
planes is repeated over them, as above, and takes the summed gradient).

    python tests/golden/make_golden_nll.py [output directory]

Keys: the inputs `image`, `gt`, `vm` (the mask, or the variance) and, for the two runs, `loss@32`, `g_input@32`, `g_vm@32`,
`mean@32`, `std@32` (Tensor.mean() and Tensor.std() of `vm`) and their `@64` twins; the gradients are those of the loss itself
(upstream 1). A `scalars_only` case (2 x 300 x 300, kept for the sums over several workgroups) holds the five scalars alone:
its inputs are regenerated from the seed. tests/test_nll_api.py regenerates every file and compares it bit for bit.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nll_cases as nc  # noqa: E402


def run(image, gt, vm, c, dtype):
    x = torch.from_numpy(image).to(dtype).requires_grad_(True)
    t = torch.from_numpy(gt).to(dtype)
    m = torch.from_numpy(vm).to(dtype).requires_grad_(True)
    if c["kind"] == "mask":
        betaprime = (m.clip(0, 1) + 1e-3).square()
        var = betaprime.unsqueeze(0).repeat(x.shape[0], 1, 1)
    else:
        var = m if m.ndim == 3 else m.unsqueeze(0).repeat(x.shape[0], 1, 1)
    loss = torch.nn.functional.gaussian_nll_loss(input=x, target=t, var=var, full=c["full"], reduction="sum" if c["sum"] else "mean")
    g_x, g_m = torch.autograd.grad(loss, (x, m))
    with torch.no_grad():
        std = m.std() if m.numel() > 1 else torch.tensor(float("nan"), dtype=dtype)  # (Tensor.std() of one entry, without its warning)
        out = dict(loss=loss.detach().numpy(), mean=m.mean().numpy(), std=std.numpy())
    if not c["scalars_only"]:
        out.update(g_input=g_x.numpy(), g_vm=g_m.numpy())
    return out


def fixture(name):
    c = nc.case(name)
    image, gt, vm = nc.inputs(name)
    d = {} if c["scalars_only"] else dict(image=image, gt=gt, vm=vm)
    for tag, dtype in (("@32", torch.float32), ("@64", torch.float64)):
        for k, v in run(image, gt, vm, c, dtype).items():
            d[k + tag] = v
    return d


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else nc.GOLDEN
    os.makedirs(out, exist_ok=True)
    torch.set_num_threads(1)  # (a sum's order must not follow the machine's core count)
    for name in nc.FIXTURES:
        d = fixture(name)
        path = os.path.join(out, name + ".npz")
        np.savez_compressed(path, **d)
        (_, _, vm), ref = nc.fixture_reference(name, d)
        c = nc.case(name)
        keys = ("loss", "mean", "std") + (() if c["scalars_only"] else ("g_input", "g_vm"))
        mult = nc.multiples({k: d[k + "@32"] for k in keys}, ref)
        print(name, f"loss {float(d['loss@64']):.9g}", "torch-fp32 multiples of E:", {k: round(v, 3) for k, v in mult.items()},
              os.path.getsize(path), "bytes")
