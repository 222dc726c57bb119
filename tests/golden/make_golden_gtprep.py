"""Generates tests/golden/gtprep/*.npz by running the REFERENCE's own Python on the seeded inputs of tests/gtprep_cases.py:
`pansharpening` (brovey_pansharp, simple_brovey, ihs_fusion through load_pansharp), `utils.rescaler.rescaler` (clamper,
standard_rescaler, rescale_wrt_firstimage), `loss.PAN_loss` (Lpan, Lgradient_pan) and `loss.pansharp_loss` (Pansharploss), in
float32 on the CPU. Only outputs and autograd gradients are stored; the inputs are regenerated from their seeds by
gtprep_cases.py and pinned here by a float64 checksum.

    python tests/golden/make_golden_gtprep.py <reference checkout>/src/gaussiansplatting

`loss/PAN_loss.py` and `loss/pansharp_loss.py` are loaded without executing `loss/__init__.py` (which pulls the renderer and the
dataset readers): a stub `loss` package, as make_golden_reg.py does. There is no fixture for histogram_equalizer (torchvision
is not installed where these were made). Images of 129 x 257 pixels keep every 4th row and column (gtprep_cases.stride_of).

Files: pansharp_<method>_<family>_<h>x<w>_<H>x<W>.npz with `out_c<C>` and `checksum_c<C>`; loss_<method>_<h>x<w>_<H>x<W>.npz with
`loss`, `grad` (of UPSTREAM * loss); pan_losses_<shape>.npz with `lpan`, `lpan_grad`, `lgradient`, `lgradient_grad`;
rescale_<kind>_<shape>.npz with `clamper`, `standard`, `wrt_first` (the reference camera is the second of three) and `minmax`.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gtprep_cases as gc  # noqa: E402

OUT = os.path.join(HERE, "gtprep")


def load_ref(refroot):
    sys.path.insert(0, refroot)
    pkg = types.ModuleType("loss")
    pkg.__path__ = [os.path.join(refroot, "loss")]
    sys.modules["loss"] = pkg
    names = ("pansharpening.load_pansharp", "utils.rescaler.rescaler", "loss.PAN_loss", "loss.pansharp_loss")
    return tuple(importlib.import_module(n) for n in names)


def name_of(shape):
    return "x".join(str(s) for s in shape)


def sub(a, shape):
    s = gc.stride_of(shape)
    return np.ascontiguousarray(a[..., ::s, ::s])


def save(name, **d):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print(name, os.path.getsize(path), "bytes")


def checksum(*arrays):
    return np.float64(sum(float(np.where(np.isfinite(a), a, 0).astype(np.float64).sum()) for a in arrays))  # (finite values)


if __name__ == "__main__":
    lp, rs, pl, psl = load_ref(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    cfg = lambda m: types.SimpleNamespace(method=m)  # noqa: E731
    t = torch.from_numpy
    for method in gc.METHODS:
        fn = lp.load_pansharp(cfg(method))
        for family in gc.FAMILIES:
            for pair in gc.PAIRS:
                d = {}
                for C in gc.fixture_channels(method, pair):
                    msi, pan = gc.pansharp_inputs(family, C, pair)
                    rp, rm = gc.reference_shapes(method, msi, pan)
                    out = fn(img_pan=t(rp), img_msi=t(rm)).numpy()
                    assert out.shape == (C,) + pair[1] and out.dtype == np.float32
                    d[f"out_c{C}"] = sub(out, pair[1])
                    d[f"checksum_c{C}"] = checksum(msi, pan)
                save(f"pansharp_{method}_{family}_{name_of(pair[0])}_{name_of(pair[1])}", **d)
        for pair in gc.LOSS_PAIRS:
            syn, msi, pan = gc.loss_inputs(method, pair)
            rp, rm = gc.reference_shapes(method, msi, pan)
            s = t(syn).requires_grad_(True)
            L = psl.Pansharploss(0.1, cfg(method))(s, t(rp), t(rm))
            g, = torch.autograd.grad(gc.UPSTREAM * L, s)
            save(f"loss_{method}_{name_of(pair[0])}_{name_of(pair[1])}", loss=L.detach().numpy(), grad=sub(g.numpy(), pair[1]),
                 checksum=checksum(syn, msi, pan))
    for shape in gc.GRADIENT_SHAPES:
        a, b = gc.gradient_inputs(shape)
        d = {"checksum": checksum(a, b)}
        for key, cls in (("lpan", pl.Lpan), ("lgradient", pl.Lgradient_pan)):
            x = t(a).requires_grad_(True)
            L = cls(0.1)(x, t(b))
            g, = torch.autograd.grad(gc.UPSTREAM * L, x)
            d[key], d[key + "_grad"] = L.detach().numpy(), g.numpy()
        save(f"pan_losses_{name_of(shape)}", **d)
    for shape in gc.RESCALE_SHAPES:
        for kind in gc.RESCALE_KINDS:
            x = gc.rescale_input(shape, kind)
            first = gc.rescale_input(shape, "plain")
            cams = [types.SimpleNamespace(is_reference_camera=k == 1, original_image=t(im.copy())) for k, im in
                    enumerate((x, first, x))]
            r = rs.load_rescaler("rescale_wrt_firstimage")
            with open(os.devnull, "w") as null:  # (its setup prints the extrema)
                stdout, sys.stdout = sys.stdout, null
                try:
                    rs.perform_rescaling_listcam(cams, r)
                finally:
                    sys.stdout = stdout
            save(f"rescale_{kind}_{name_of(shape)}", clamper=sub(rs.load_rescaler("clamper").forward(t(x)).numpy(), shape),
                 standard=sub(rs.load_rescaler("standard_rescaler").forward(t(x)).numpy(), shape),
                 wrt_first=sub(cams[0].original_image.numpy(), shape),
                 minmax=np.stack([rs.compute_min_vals(t(x)).numpy(), rs.compute_max_vals(t(x)).numpy()], axis=1), checksum=checksum(x))
