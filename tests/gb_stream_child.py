"""Helper process of tests/test_gpu_gaussian_bwd_stream.py: with the EOGS_GB_WIDE of its environment (read once per process)
runs every case file of a directory forward + backward through the HIP library and writes each case's gradients to
<out_dir>/<case>.npz. A case file holds the inputs of tests/util.py run_case and `kind`:
plain (GaussianRasterizer), raw / alt (eogs2_amd.fused.rasterize_raw, the full and the altitude-only render), range (the
per-Gaussian pass over three ascending ranges, eogs_rast_backward_range) or nofit (the backward of a forward queued on a
capacity token that does not hold it)."""
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from util import raw_params_from_scene, run_case, run_raw  # noqa: E402

from eogs2_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib, rasterizer  # noqa: E402

DEV = torch.device("cuda:0")
SCENE_KEYS = ("means3D", "scales", "rotations", "opacities", "colors", "bg", "viewmatrix", "dL_dcolor")


def _plain(case):
    return run_case(case, DEV, GaussianRasterizer, GaussianRasterizationSettings)


def _range(case):
    plan = rasterizer.BackwardPlan()
    plan.chunks = 3
    bounds = rasterizer.chunk_ranges(case["means3D"].shape[0], 3)
    assert len(bounds) == 3 and all(p0 % 256 == 0 for p0, _ in bounds), bounds
    rasterizer.set_backward_plan(plan)
    try:
        return _plain(case)
    finally:
        rasterizer.set_backward_plan(None)


def _raw(case, altitude_only):
    from eogs2_amd.fused import rasterize_raw
    from eogs2_amd.synthetic import settings_for

    H, W = int(case["H"]), int(case["W"])
    scene = {k: torch.from_numpy(case[k]).to(DEV) for k in SCENE_KEYS}
    raw, alt = raw_params_from_scene(scene)
    if not altitude_only:
        out = run_raw(raw, alt, scene, H, W, False, True)
        out["_num_rendered"] = 0
        return out
    leaves = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    vm = scene["viewmatrix"].clone().requires_grad_(True)
    rs = settings_for(dict(scene, viewmatrix=vm), H, W)._replace(projmatrix=vm.detach())
    m2 = torch.zeros(raw["xyz"].shape[0], 3, device=DEV, requires_grad=True)
    color, radii, _ = rasterize_raw(leaves["xyz"], m2, leaves["f_dc"], leaves["opacity_logit"], leaves["log_scaling"],
                                    leaves["raw_rotation"], alt, rs, altitude_only=True)
    assert tuple(color.shape) == (1, H, W)
    (color[0] * scene["dL_dcolor"][3]).sum().backward()
    out = dict(out_color=color.detach(), out_radii=radii, g_means2D=m2.grad, g_viewmatrix=vm.grad)
    out.update({"g_" + k: v.grad for k, v in leaves.items()})
    out["_num_rendered"] = int(color.grad_fn.num_rendered)
    return out


def _nofit(case, small):
    """The forward of `case` queued on the capacity of the much smaller `small`, and NOT repeated: the wrapper is told that it
    fitted. Its backward finds the device's own comparison (the counts against the token) false and returns zeros."""
    abi = _lib.get()
    rasterizer.set_speculation(True, forget=True)
    try:
        _plain(small)
        real = abi.capacity_token

        def told_to_fit(P, last, slack, have_scratch, exact, cap, fits):
            rc = real(P, last, slack, have_scratch, exact, cap, fits)
            if fits is not None:
                fits._obj.value = 1
            return rc

        abi.capacity_token = told_to_fit
        try:
            got = _plain(case)
        finally:
            del abi.capacity_token
    finally:
        rasterizer.set_speculation(False, forget=True)
    assert (got["_num_rendered"] & 0x7FFFFFFF) < (got["_num_rendered_exact"] & 0x7FFFFFFF), "the guess held the forward"
    return got


def main(case_dir, out_dir):
    abi = _lib.get()
    assert abi.backend == "hip-gfx950"
    forced = int(os.environ["EOGS_GB_WIDE"])
    for f in sorted(glob.glob(os.path.join(case_dir, "*.npz"))):
        name = os.path.basename(f)[:-4]
        z = np.load(f)
        kind = str(z["kind"])
        case = {k: z[k] for k in z.files if k != "kind" and not k.startswith("small_")}
        case["antialiasing"] = False
        if kind == "plain":
            got = _plain(case)
        elif kind == "range":
            got = _range(case)
        elif kind in ("raw", "alt"):
            got = _raw(case, kind == "alt")
        elif kind == "nofit":
            small = dict(case, **{k[6:]: z[k] for k in z.files if k.startswith("small_")})
            got = _nofit(case, small)
        else:
            raise ValueError(kind)
        torch.cuda.synchronize()
        token = int(got.pop("_num_rendered", 0))
        exact = int(got.pop("_num_rendered_exact", token))
        P = case["means3D"].shape[0]
        build = abi.backward_info(P, token) if token > 0 else -1
        assert build in (-1, forced), f"{name}: the backward would launch build {build}, not the forced {forced}"
        np.savez(os.path.join(out_dir, name + ".npz"), _slots=np.int64(exact & 0x7FFFFFFF), _build=np.int64(build),
                 **{k: v.detach().cpu().numpy() for k, v in got.items()})


if __name__ == "__main__":
    main(*sys.argv[1:])
