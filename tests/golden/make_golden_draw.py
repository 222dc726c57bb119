"""Generates tests/golden/draw/*.npz by running the REFERENCE's own `AffineCamera.sample_random_camera` and
`AffineCamera.get_nadir_camera` (scene/cameras/affine_cameras.py:372-430), imported at run time from the reference's checkout
(build container only). Only arrays are stored: the inputs, the planted normals, `new_affine` and `myM` of both methods.

    python tests/golden/make_golden_draw.py

The two methods are called unbound on a plain namespace carrying the attributes they read. `torch.randn` is patched for the
call to return planted values: the two clipped normals of `eogs2_amd.draw.draws_for(seed, iteration, slot)`, so that the
device's draw at that (seed, iteration, slot) is the reference's draw and tests/test_gpu_draw.py compares the matrices
directly. `get_nadir_camera` names the device "cuda" literally; `torch.zeros` is patched for the call to stay on the CPU.
The inputs come from tests/draw_cases.py (`camera_inputs`), so the tests rebuild them and find the same arrays here.
"""
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from make_golden_shade import load_ref  # noqa: E402  (the reference's affine_cameras module, read from its checkout)
import draw_cases  # noqa: E402
from eogs2_amd.draw import draws_for  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "draw")

# (file, kind of draw_cases.camera_inputs, its seed, the stream's seed, iteration, slot, virtual_camera_extent)
CASES = [
    ("well_first", "well", 0, 0, 0, 0, 0.02),
    ("well_extent1", "well", 1, 7, 2 ** 63 - 1, 2, 1.0),
    ("utm_carry", "utm", 0, 2 ** 64 - 1, 2 ** 32, 3, 0.02),
    ("utm_extent1", "utm", 1, 12345, 2 ** 32 - 1, 7, 1.0),
    ("zero_center", "zero_center", 0, 12345, 7, 1, 0.02),
    ("zero_center_extent1", "zero_center", 1, 1, 1, 0, 1.0),
]


def stand_in(affine, center):
    return types.SimpleNamespace(affine=torch.from_numpy(affine.copy()), centerofscene_ECEF=torch.from_numpy(center.copy()),
                                 data_device="cpu", camera_center=torch.zeros(3), image_width=8, image_height=8, FoVx=1.0, FoVy=1.0)


def run_case(cams, kind, case_seed, seed, iteration, slot, extent):
    affine, center = draw_cases.camera_inputs(kind, case_seed)
    normals = np.asarray(draws_for(seed, iteration, slot)[1], dtype=np.float32)
    planted = lambda *a, **k: torch.from_numpy(normals.copy())  # noqa: E731
    with mock.patch.object(torch, "randn", planted):
        cam, myM = cams.AffineCamera.sample_random_camera(stand_in(affine, center), extent)
    real_zeros = torch.zeros
    on_cpu = lambda *a, **k: real_zeros(*a, **{**k, "device": "cpu"})  # noqa: E731
    with mock.patch.object(torch, "zeros", on_cpu):
        ncam, nM = cams.AffineCamera.get_nadir_camera(stand_in(affine, center))
    assert cam.world_view_transform is cam.full_proj_transform
    return dict(affine=affine, center=center, seed=np.array(seed, dtype=np.uint64), iteration=np.array(iteration, dtype=np.uint64),
                slot=np.array(slot), extent=np.array(extent, dtype=np.float32), normals=normals,
                new_affine=np.ascontiguousarray(cam.world_view_transform.numpy()), myM=np.ascontiguousarray(myM.numpy()),
                nadir_affine=np.ascontiguousarray(ncam.world_view_transform.numpy()), nadir_myM=np.ascontiguousarray(nM.numpy()))


def main():
    cams = load_ref()[0]
    os.makedirs(OUT, exist_ok=True)
    for name, *case in CASES:
        res = run_case(cams, *case)
        assert res["new_affine"].dtype == np.float32 and res["myM"].dtype == np.float32
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **res)
        print(name, res["normals"], res["myM"][:2, 2], res["nadir_myM"][:2, 2])


if __name__ == "__main__":
    main()
