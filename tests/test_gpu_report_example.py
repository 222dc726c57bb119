"""GPU: the end-to-end example with the report module inside (examples/train_synthetic.py --test-views, --report-every, --cc-to-test,
--normalize-colors, --render-set): two reports with finite numbers, render_set's products and the video frames of every view on
disk with their shapes and dtypes, and a PLY that holds the aligned colours."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import report_cases as RC

pytestmark = pytest.mark.gpu
SIZE, VIEWS, TEST_VIEWS = 64, 3, 2


def test_train_report_align_save_render(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(RC.ROOT, "examples"))
    import train_synthetic as ex

    ply, out_dir = str(tmp_path / "point_cloud.ply"), str(tmp_path / "render_set")
    ex.main(["--gaussians", "2000", "--size", str(SIZE), "--iters", "12", "--views", str(VIEWS), "--test-views", str(TEST_VIEWS),
             "--report-every", "6", "--cc-to-test", "average", "--normalize-colors", "--save-ply", ply, "--render-set", out_dir])
    out = capsys.readouterr().out
    # two reports (iterations 6 and 12), each over the test and the train views, finite numbers; the unused kind stays 0
    lines = re.findall(r"^\[ITER (\d+)\] Evaluating (test|train): L1 (\{.*?\}) PSNR (\{.*?\})$", out, flags=re.M)
    assert [(int(i), n) for i, n, _, _ in lines] == [(6, "test"), (6, "train"), (12, "test"), (12, "train")], out[-3000:]
    assert [(i, n) for i, n, _ in ex.main.last_reports] == [(6, "test"), (6, "train"), (12, "test"), (12, "train")]
    for _, _, res in ex.main.last_reports:
        assert set(res) == {"l1", "psnr"}
        assert np.isfinite(res["l1"]["msi"]) and res["l1"]["msi"] > 0 and np.isfinite(res["psnr"]["msi"]) and res["psnr"]["msi"] > 0
        assert res["l1"]["pan"] == 0.0 and res["psnr"]["pan"] == 0.0
    for _, _, l1, psnr in lines:
        assert all(np.isfinite(float(x)) for x in re.findall(r": ([0-9.e+-]+)", l1 + psnr))
    # the products of every view, in file layout
    names = [f"train_{v}" for v in range(VIEWS)] + [f"test_{k}" for k in range(TEST_VIEWS)]
    hwc3, hw = (SIZE, SIZE, 3), (SIZE, SIZE)
    shapes = {"rawrender": hwc3, "altitude": hw, "accumulated_opacity": hw, "sunpovsampled": hwc3, "nadirpov": hwc3, "nadirpovsampled": hwc3,
              "nadiraltitudesampled": hw, "nadir_altitude_diff": hw, "shadowmap": hw, "shaded": hwc3, "cc": hwc3, "final": hwc3, "gt": hwc3}
    for name in names:
        for key, shape in shapes.items():
            arr = np.load(os.path.join(out_dir, key, name + ".npy"))
            assert arr.shape == shape and arr.dtype == np.float32 and np.isfinite(arr).all(), (key, name)
        frame = np.load(os.path.join(out_dir, "frames", name + ".npy"))
        assert frame.shape == (SIZE, 2 * SIZE, 3) and frame.dtype == np.uint8
        final = np.load(os.path.join(out_dir, "final", name + ".npy"))
        assert np.array_equal(frame[:, :SIZE], RC.u8_trunc(final)[:, :, ::-1])  # the left half: the final image, 8-bit, BGR
        assert frame[:, SIZE:].min() < frame[:, SIZE:].max() and np.array_equal(frame[:, SIZE:, 0], frame[:, SIZE:, 2])  # the elevation
    assert len(ex.main.last_render_set) == len(names) * (len(shapes) + 1)
    # the aligned colours: in place, the float64 formula within its bound, and what the PLY holds
    al = ex.main.last_alignment
    before, after = al["f_dc_before"].numpy(), al["f_dc_after"].numpy()
    f64, bound = RC.rows_float64(before, al["A1"].numpy(), al["b1"].numpy())
    assert np.all(np.abs(after.astype(np.float64) - f64) <= bound) and not np.array_equal(before, after)
    assert "colours aligned to view 0" in out
    from eogs2_amd.model import GaussianModel

    loaded = GaussianModel(0)
    loaded.load_ply(ply)
    assert loaded._features_dc.detach().cpu().numpy().reshape(-1, 3).tobytes() == after.reshape(-1, 3).tobytes()
    # view 0's correction is the identity now; the others were recomposed in the bank's rows
    bank = ex.main.view_bank
    assert np.allclose(bank.row("camera.0", 0).cpu().numpy().reshape(3, 3), np.eye(3), atol=2e-7)
    assert np.allclose(bank.row("camera.1", 0).cpu().numpy(), 0.0, atol=2e-7)
    assert not np.allclose(bank.row("camera.0", 1).cpu().numpy().reshape(3, 3), np.eye(3), atol=1e-3)
