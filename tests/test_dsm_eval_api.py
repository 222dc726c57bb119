"""CPU: the public interface of the DSM evaluation (eogs2_amd.dsm_eval, include/eogs_tsdf.h eogs_tsdf_dsm_*): the built
library exports the entry points, their size queries and argument checks answer without a device, and the Python
wrappers refuse what they cannot run (CPU tensors: there is no CPU fallback)."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


NAMES = ("downsample", "ncc_bytes", "ncc", "shift_bytes", "shift", "apply_shift", "mae_bytes", "mae")


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HIP_ONLY, SIGNATURES

    for n in NAMES:
        assert hasattr(hip_lib.cdll, "eogs_tsdf_dsm_" + n), n
        assert "eogs_tsdf_dsm_" + n in SIGNATURES and "eogs_tsdf_dsm_" + n in HIP_ONLY
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only
    assert {"dsm_downsample", "dsm_pivots", "dsm_moments", "dsm_finalize", "dsm_apply_shift", "dsm_mae"} <= set(hip_lib.profile_slot_names())


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import dsm_eval

    assert eogs2_amd.dsm_eval is dsm_eval
    for n in ("downsample2x", "ncc_search", "compute_shift", "apply_shift", "mask_dsm", "dsm_pointwise_diff", "dsm_mae", "compute_shift_device",
              "clear_workspaces"):
        assert callable(getattr(dsm_eval, n)), n
    assert dsm_eval.RESULT_DTYPE.itemsize == 72  # sizeof(eogs_tsdf_dsm_result)


def test_size_queries_and_argument_checks_need_no_device(hip_lib):
    n, lv = ctypes.c_size_t(), ctypes.c_int()
    hip_lib.check(hip_lib.tsdf_dsm_ncc_bytes(2048, 2048, 5, ctypes.byref(n)))
    # 121 shifts x 6 moments x 2 partials per workgroup x at most 1024 workgroups x 8 bytes, plus the summed moments
    assert 121 * 6 * 2048 * 8 <= n.value <= 121 * 6 * 2048 * 8 + (1 << 16)
    hip_lib.check(hip_lib.tsdf_dsm_ncc_bytes(40, 37, 5, ctypes.byref(n)))
    assert n.value < (1 << 16)
    hip_lib.check(hip_lib.tsdf_dsm_shift_bytes(2048, 2048, 2051, 2050, 5, ctypes.byref(n), ctypes.byref(lv)))
    assert lv.value == 6  # 2048, 1024, 512, 256, 128, 64
    assert n.value >= 2 * 8 * (1024 * 1024 + 512 * 512)
    hip_lib.check(hip_lib.tsdf_dsm_shift_bytes(100, 5000, 100, 5000, 5, ctypes.byref(n), ctypes.byref(lv)))
    assert lv.value == 1  # min(H, W) > 100 fails at once
    hip_lib.check(hip_lib.tsdf_dsm_shift_bytes(202, 206, 202, 206, 5, ctypes.byref(n), ctypes.byref(lv)))
    assert lv.value == 3
    assert hip_lib.tsdf_dsm_ncc_bytes(64, 64, 9, ctypes.byref(n)) == -1
    assert b"irange" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.tsdf_dsm_ncc_bytes(64, 64, -1, ctypes.byref(n)) == -1
    assert hip_lib.tsdf_dsm_ncc_bytes(0, 64, 5, ctypes.byref(n)) == -1
    assert hip_lib.tsdf_dsm_shift_bytes(64, 64, 63, 64, 5, ctypes.byref(n), None) == -1
    hip_lib.check(hip_lib.tsdf_dsm_mae_bytes(ctypes.byref(n)))
    assert 0 < n.value < (1 << 20)
    assert hip_lib.tsdf_dsm_mae_bytes(None) == -1
    # NULL images and a too-small image are rejected before anything touches a device
    assert hip_lib.tsdf_dsm_ncc(8, 8, None, 8, 8, None, 0, 5, None, 1, None, None, None, 0, None) == -1
    assert hip_lib.tsdf_dsm_apply_shift(8, 8, None, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, None, None) == -1


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import dsm_eval as D

    u, v = torch.zeros(40, 50), torch.zeros(42, 50)
    for call in (lambda: D.downsample2x(u), lambda: D.ncc_search(u, v), lambda: D.compute_shift(u, v), lambda: D.apply_shift(u),
                 lambda: D.dsm_pointwise_diff(v, u), lambda: D.dsm_mae(v, u), lambda: D.mask_dsm(u, None, None, None)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (u.half(), u.long(), u[None], torch.zeros(0, 4)):
        with pytest.raises(TypeError):
            D.downsample2x(bad)
        with pytest.raises(TypeError):
            D.compute_shift(bad, bad)
    with pytest.raises(TypeError):
        D.apply_shift(u.numpy())
    with pytest.raises(ValueError, match="smaller"):
        D.compute_shift(v, u)  # the DSM to register is smaller than the reference
    with pytest.raises(ValueError, match="smaller"):
        D.ncc_search(torch.zeros(40, 51), torch.zeros(40, 50))
    with pytest.raises(ValueError, match="smaller"):
        D.dsm_mae(u, v)  # (pred, gt): the prediction is the one that is registered
    with pytest.raises(ValueError, match="irange"):
        D.ncc_search(u, v, irange=D.MAX_IRANGE + 1)
    with pytest.raises(ValueError, match="clip"):
        D.dsm_mae(v, u, clip="none")
