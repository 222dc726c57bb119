"""CPU: the public interface of the flow-matching step (eogs2_amd.flow, include/eogs_resample.h eogs_resample_flow_*): the
built library exports the entry points, their size queries and argument checks answer without a device, and the Python
wrappers refuse what they cannot run (CPU tensors: there is no CPU fallback)."""
import ctypes
import types

import pytest
import torch


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


NAMES = ("stats_bytes", "stats", "forward", "bytes", "backward")


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HIP_ONLY, SIGNATURES

    for n in NAMES:
        assert hasattr(hip_lib.cdll, "eogs_resample_flow_" + n), n
        assert "eogs_resample_flow_" + n in SIGNATURES and "eogs_resample_flow_" + n in HIP_ONLY
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only
    assert {"flow_fwd", "flow_bwd", "flow_stats"} <= set(hip_lib.profile_slot_names())


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import flow

    assert eogs2_amd.flow is flow
    for n in ("apply_flow", "flow_stats", "performOpticalmatching", "perform_flow_matching", "adjust_affine", "flowmatch_l"):
        assert callable(getattr(flow, n)), n
    for n in ("set_cst_displacement", "normalize_img_raft", "adjust_img_for_raft", "get_flow", "apply_flow", "compute_stats",
              "get_and_apply_flow"):
        assert callable(getattr(flow.performOpticalmatching, n)), n


def test_size_queries_and_argument_checks_need_no_device(hip_lib):
    n = ctypes.c_size_t()
    hip_lib.check(hip_lib.resample_flow_bytes(1024, 1024, ctypes.byref(n)))
    assert 64 * 64 * 16 <= n.value <= 64 * 64 * 16 + 1024  # one box per 16 x 16 tile
    hip_lib.check(hip_lib.resample_flow_stats_bytes(1024, 1024, ctypes.byref(n)))
    assert 0 < n.value < (1 << 16)
    need = n.value
    for H, W in ((1, 64), (64, 1), (0, 0), (-3, 8)):
        assert hip_lib.resample_flow_bytes(H, W, ctypes.byref(n)) == -1
        assert hip_lib.resample_flow_stats_bytes(H, W, ctypes.byref(n)) == -1
    assert hip_lib.resample_flow_bytes(8, 8, None) == -1
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is answered before anything touches a device
    # NULL pointers
    assert hip_lib.resample_flow_forward(3, 8, 8, None, one, 64, 8, 1, None, one, None) == -1
    assert hip_lib.resample_flow_forward(3, 8, 8, one, None, 64, 8, 1, None, one, None) == -1
    assert hip_lib.resample_flow_forward(3, 8, 8, one, one, 64, 8, 1, None, None, None) == -1
    assert b"NULL" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.resample_flow_backward(3, 8, 8, None, 64, 8, 1, None, one, one, one, 1 << 20, None) == -1
    assert hip_lib.resample_flow_stats(8, 8, None, 64, 8, 1, one, one, 1 << 20, None) == -1
    # sizes
    assert hip_lib.resample_flow_forward(0, 8, 8, one, one, 64, 8, 1, None, one, None) == -1
    assert hip_lib.resample_flow_forward(3, 1, 8, one, one, 8, 8, 1, None, one, None) == -1
    assert hip_lib.resample_flow_backward(3, 8, 1, one, 8, 1, 1, None, one, one, one, 1 << 20, None) == -1
    assert b"bad sizes" in hip_lib.cdll.eogs_rast_last_error()
    # a field needs its workspace, whole
    assert hip_lib.resample_flow_backward(3, 8, 8, one, 64, 8, 1, None, one, one, None, 0, None) == -3
    assert hip_lib.resample_flow_backward(3, 8, 8, one, 64, 8, 1, None, one, one, one, 8, None) == -3
    assert b"workspace" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.resample_flow_stats(1024, 1024, one, 1 << 20, 1024, 1, one, one, need - 1, None) == -3


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import flow as F

    img, fl = torch.zeros(3, 8, 9), torch.zeros(1, 2, 8, 9)
    w = F.performOpticalmatching(True, mode="upscale", model=lambda a, b, num_flow_updates=12: [fl])
    for call in (lambda: F.apply_flow(img, fl), lambda: F.apply_flow(img[0], fl), lambda: F.flow_stats(fl), lambda: F.flowmatch_l(fl),
                 lambda: w.apply_flow(img, fl), lambda: w.compute_stats(fl), lambda: w.set_cst_displacement(fl),
                 lambda: F.adjust_affine(torch.eye(4), 9, 8, fl), lambda: F.apply_flow(img, fl.mean((2, 3), keepdim=True).expand(1, 2, 8, 9))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (img.double(), img.half(), img.long()):
        with pytest.raises(TypeError):
            F.apply_flow(bad, fl)
    with pytest.raises(TypeError):
        F.apply_flow(img, fl.double())
    with pytest.raises(TypeError):
        F.flow_stats(fl.half())
    for bad_img, bad_flow in ((img[None], fl), (img, fl[0]), (img, torch.zeros(1, 2, 9, 8)), (img, torch.zeros(2, 2, 8, 9)),
                              (img, torch.zeros(1, 3, 8, 9)), (torch.zeros(3, 1, 9), torch.zeros(1, 2, 1, 9)),
                              (torch.zeros(8, 1), torch.zeros(1, 2, 8, 1)), (torch.zeros(0, 8, 9), fl)):
        with pytest.raises(ValueError):
            F.apply_flow(bad_img, bad_flow)
    with pytest.raises(ValueError):
        F.flow_stats(torch.zeros(1, 2, 1, 9))
    with pytest.raises(ValueError, match="gate"):
        F.apply_flow(img, fl, gate=torch.zeros(2))


def test_constructor_asserts_match_the_reference():
    from eogs2_amd.flow import performOpticalmatching as P

    with pytest.raises(AssertionError, match="mode should be downscale or upscale, got crop"):
        P(True, mode="crop")
    with pytest.raises(AssertionError, match="model_name should be either large or small, got tiny"):
        P(True, model_name="tiny")
    with pytest.raises(AssertionError, match="criteria should be either max_value_flow, psnr, l_photom or always, got never"):
        P(True, criteria="never")
    w = P(False)
    assert (w.mode, w.device, w.model_name, w.num_flow_updates, w.criteria) == ("downscale", "cuda", "large", 12, "max_value_flow")
    with pytest.raises(RuntimeError, match="the flow network is the caller's"):
        w._get_model()
    with pytest.raises(AssertionError, match="size of both images should be the same"):
        w.get_flow(torch.zeros(3, 8, 8), torch.zeros(1, 8, 8))
    with pytest.raises(AssertionError, match="Image should have 3 channels, got 2"):
        w.get_flow(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8))


def test_plumbing_around_the_network_is_the_reference_s():
    """normalize / adjust_img_for_raft are plain torch: the shapes and values the network sees, on the CPU."""
    from eogs2_amd.flow import performOpticalmatching as P, pgd8, ppcm8

    assert (pgd8(37), pgd8(40), ppcm8(37), ppcm8(40)) == (32, 40, 40, 40)
    g = torch.Generator().manual_seed(0)
    gt, tg = torch.rand(3, 37, 45, generator=g), torch.rand(3, 37, 45, generator=g)
    w = P(False, mode="downscale")
    a, b, c, d, n, m = w.adjust_img_for_raft(w.normalize_img_raft(gt)[None], w.normalize_img_raft(tg)[None], gt, tg)
    assert a.shape == b.shape == (1, 3, 32, 40) and c.shape == d.shape == (3, 32, 40) and (n, m) == (-1, -1)
    assert torch.equal(a[0], (gt[:, :32, :40] - 0.5) * 2)
    w = P(False, mode="upscale")
    a, b, c, d, n, m = w.adjust_img_for_raft(w.normalize_img_raft(gt)[None], w.normalize_img_raft(tg)[None], gt, tg)
    assert a.shape == b.shape == (1, 3, 40, 48) and c is gt and d is tg and (n, m) == (37, 45)
    assert torch.equal(a[0, :, :37, 45], (gt[:, :, 43] - 0.5) * 2) and torch.equal(b[0, :, 37, :45], (tg[:, 35, :] - 0.5) * 2)


def test_on_device_refuses_what_it_cannot_gate():
    from eogs2_amd import flow as F

    opt = types.SimpleNamespace(flowmatching=types.SimpleNamespace(max_value_flow=3.0))
    img = torch.zeros(3, 8, 8)
    model = lambda a, b, num_flow_updates=12: [torch.zeros(1, 2, 8, 8)]  # noqa: E731
    for mode, criteria in (("downscale", "max_value_flow"), ("downscale", "always"), ("upscale", "psnr"), ("upscale", "l_photom")):
        w = F.performOpticalmatching(True, mode=mode, criteria=criteria, model=model)
        with pytest.raises(ValueError, match="on_device"):
            F.perform_flow_matching(opt, w, img, img, on_device=True)
