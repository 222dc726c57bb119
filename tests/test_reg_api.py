"""CPU: the public interface of the regularisers (eogs2_amd.regularizers, include/eogs_reg.h): the built library exports
the entry points, their size queries and every argument refusal answer without a device, and the Python wrappers refuse
what they cannot run (CPU tensors: there is no CPU fallback)."""
import ctypes
import os
import re
import types

import pytest
import torch

import abi_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gauss_bytes", "gauss_forward", "gauss_backward", "image_bytes", "image_forward", "image_backward")


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS, HIP_ONLY

    src = AC.header_text("eogs_reg.h")
    assert sorted(set(re.findall(r"\b(eogs_reg_[a-z_0-9]+)\s*\(", src))) == sorted(HEADERS["eogs_reg.h"]) == sorted("eogs_reg_" + n for n in NAMES)
    for n in NAMES:
        assert hasattr(hip_lib.cdll, "eogs_reg_" + n), n
        assert "eogs_reg_" + n in HIP_ONLY
        assert getattr(hip_lib.cdll, "eogs_reg_" + n).argtypes == HEADERS["eogs_reg.h"]["eogs_reg_" + n][1]  # bound on load
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only
    slots = hip_lib.profile_slot_names()
    assert {"reg_fwd", "reg_bwd"} <= set(slots) and len(slots) <= 32  # (the mask of eogs_rast_profile_select has 32 bits)


def test_constants_agree_with_the_header_and_the_optimizer():
    from eogs2_amd import _abi
    from eogs2_amd.optim import RETIRED_LOGIT

    import reg_cases as rc

    src = open(os.path.join(ROOT, "include", "eogs_reg.h")).read()
    for name, value in (("OPACITY", _abi.REG_OPACITY), ("OPACITY_RADII", _abi.REG_OPACITY_RADII), ("ERANK", _abi.REG_ERANK)):
        assert int(re.search(rf"#define EOGS_REG_{name} (\d+)u", src).group(1)) == value
    below = float(re.search(r"#define EOGS_REG_RETIRED_BELOW \((-[0-9.e+]+)f\)", src).group(1))
    assert below == _abi.REG_RETIRED_BELOW == 0.5 * RETIRED_LOGIT and rc.RETIRED_LOGIT == RETIRED_LOGIT


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import regularizers as R

    assert eogs2_amd.regularizers is R
    for n in ("gaussian_regularizers", "render_regularizers", "OpacityLoss", "radiiOpacityLoss", "erankLoss", "Total_variation",
              "AccumulatedOpacity"):
        assert callable(getattr(R, n)) and n in R.__all__, n
    # the reference's constructors and names
    assert (R.OpacityLoss(0.1, 5000).w_L_opacity, R.OpacityLoss(0.1, 5000).init_number_of_gaussians) == (0.1, 5000)
    assert R.OpacityLoss(0.1, 1).get_loss_name() == "L_opacity" and R.radiiOpacityLoss(0.1, 1).get_loss_name() == "radiiOpacityLoss"
    assert R.erankLoss(0.2).weight == 0.2 and R.erankLoss(0.2).get_loss_name() == "L_erank"
    assert R.Total_variation(0.3).weight == 0.3 and R.Total_variation(0.3).get_loss_name() == "L_TV_altitude"
    assert R.AccumulatedOpacity(0.4).w_L_accumulated_opacity == 0.4


def test_size_queries_and_argument_checks_need_no_device(hip_lib):
    n = ctypes.c_size_t()
    hip_lib.check(hip_lib.reg_gauss_bytes(1 << 20, ctypes.byref(n)))
    assert 0 < n.value < (1 << 16)
    need = n.value
    hip_lib.check(hip_lib.reg_image_bytes(2048, 2048, ctypes.byref(n)))
    assert 0 < n.value < (1 << 16)
    assert hip_lib.reg_gauss_bytes(0, ctypes.byref(n)) == -1 and hip_lib.reg_gauss_bytes(-5, ctypes.byref(n)) == -1
    assert hip_lib.reg_gauss_bytes(8, None) == -1 and hip_lib.reg_image_bytes(8, 8, None) == -1
    for H, W in ((1, 64), (64, 1), (0, 0), (-3, 8)):
        assert hip_lib.reg_image_bytes(H, W, ctypes.byref(n)) == -1
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is answered before anything touches a device
    OP, RAD, ER = 1, 2, 4
    fwd, bwd = hip_lib.reg_gauss_forward, hip_lib.reg_gauss_backward
    # sizes, the selection, n_init
    assert fwd(0, OP, one, None, None, 10.0, one, one, one, need, None) == -1
    assert b"bad size" in hip_lib.cdll.eogs_rast_last_error()
    assert fwd(8, 0, one, None, None, 10.0, one, one, one, need, None) == -1
    assert fwd(8, 8, one, one, one, 10.0, one, one, one, need, None) == -1
    assert b"want" in hip_lib.cdll.eogs_rast_last_error()
    assert fwd(8, OP, one, None, None, 0.0, one, one, one, need, None) == -1
    assert fwd(8, OP, one, None, None, float("nan"), one, one, one, need, None) == -1
    assert b"n_init" in hip_lib.cdll.eogs_rast_last_error()
    # NULL pointers: each term brings its input
    assert fwd(8, OP, None, None, None, 10.0, one, one, one, need, None) == -1
    assert fwd(8, OP, one, None, None, 10.0, None, one, one, need, None) == -1
    assert fwd(8, OP, one, None, None, 10.0, one, None, one, need, None) == -1
    assert fwd(8, OP, one, None, None, 10.0, one, one, None, need, None) == -1
    assert fwd(8, OP | ER, one, None, None, 10.0, one, one, one, need, None) == -1
    assert fwd(8, OP | RAD, one, None, None, 10.0, one, one, one, need, None) == -1
    assert b"NULL" in hip_lib.cdll.eogs_rast_last_error()
    assert fwd(8, OP, one, None, None, 10.0, one, one, one, need - 1, None) == -3
    assert b"workspace" in hip_lib.cdll.eogs_rast_last_error()
    assert bwd(0, OP, one, None, None, 10.0, one, one, one, None, one, None, None) == -1
    assert bwd(8, OP, one, None, None, 10.0, one, None, one, None, one, None, None) == -1
    assert bwd(8, OP, one, None, None, 10.0, one, one, one, None, None, None, None) == -1
    assert bwd(8, ER, one, None, None, 10.0, one, one, one, None, one, one, None) == -1
    assert bwd(8, ER, one, one, None, 10.0, one, one, one, None, one, None, None) == -1  # erank without g_scaling
    assert bwd(8, OP, one, None, None, 10.0, one, one, one, None, one, one, None) == -1  # g_scaling without erank
    assert b"g_scaling" in hip_lib.cdll.eogs_rast_last_error()
    ifwd, ibwd = hip_lib.reg_image_forward, hip_lib.reg_image_backward
    for H, W in ((1, 8), (8, 1), (0, 0)):  # the reference's empty mean is NaN there
        assert ifwd(H, W, one, one, one, one, one, need, None) == -1
        assert ibwd(H, W, one, one, one, one, None, one, one, None) == -1
    assert b"bad sizes" in hip_lib.cdll.eogs_rast_last_error()
    assert ifwd(8, 8, None, None, one, one, one, need, None) == -1
    assert ifwd(8, 8, one, None, None, one, one, need, None) == -1
    assert ifwd(8, 8, one, None, one, None, one, need, None) == -1
    assert ifwd(8, 8, one, None, one, one, None, need, None) == -1
    assert ifwd(8, 8, one, one, one, one, one, 8, None) == -3
    assert ibwd(8, 8, None, None, one, one, None, None, None, None) == -1
    assert ibwd(8, 8, one, None, one, one, None, None, None, None) == -1  # the altitude without its gradient plane
    assert ibwd(8, 8, one, None, one, one, None, one, one, None) == -1  # a gradient plane without its input
    assert b"NULL with NULL" in hip_lib.cdll.eogs_rast_last_error()


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import regularizers as R

    o, s, r = torch.zeros(6, 1), torch.zeros(6, 3), torch.ones(6, dtype=torch.int32)
    img = torch.zeros(8, 9)
    m = types.SimpleNamespace(_opacity=o, _scaling=s)
    for call in (lambda: R.gaussian_regularizers(o, n_init=10, weights=(0.1, 0, 0)),
                 lambda: R.gaussian_regularizers(o.view(-1), s, r, n_init=10, weights=torch.zeros(3), want=("opacity", "opacity_radii", "erank")),
                 lambda: R.gaussian_regularizers(o, s, n_init=10, weights={"erank": 0.5}, want="erank"),
                 lambda: R.render_regularizers(img, img, weights=(1.0, 1.0)), lambda: R.render_regularizers(None, img[None], weights=(0, 1)),
                 lambda: R.OpacityLoss(0.1, 10)(m), lambda: R.radiiOpacityLoss(0.1, 10)(m, r), lambda: R.erankLoss(0.1)(m),
                 lambda: R.Total_variation(0.1)(img[None]), lambda: R.AccumulatedOpacity(0.1)(img)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (o.double(), o.half(), o.long()):
        with pytest.raises(TypeError):
            R.gaussian_regularizers(bad, n_init=10, weights=(1, 0, 0))
    with pytest.raises(TypeError):
        R.gaussian_regularizers(o, s.double(), n_init=10, weights=(1, 0, 1), want=("erank",))
    with pytest.raises(TypeError):
        R.gaussian_regularizers(o, radii=r.float(), n_init=10, weights=(1, 1, 0), want=("opacity_radii",))
    with pytest.raises(TypeError):
        R.render_regularizers(img.double(), weights=(1, 0))
    with pytest.raises(TypeError):
        R.render_regularizers(None, img.half(), weights=(1, 0))
    for kw in (dict(opacity_logits=torch.zeros(6, 2)), dict(opacity_logits=torch.zeros(0, 1)), dict(opacity_logits=torch.zeros(2, 3, 1)),
               dict(want=("erank",)), dict(want=("erank",), log_scales=torch.zeros(5, 3)), dict(want=("erank",), log_scales=torch.zeros(6, 4)),
               dict(want=("opacity_radii",)), dict(want=("opacity_radii",), radii=torch.ones(5, dtype=torch.int32)),
               dict(want=()), dict(want=("tv",)), dict(n_init=0), dict(n_init=-3)):
        args = dict(opacity_logits=o, n_init=10, weights=(1, 1, 1))
        args.update(kw)
        with pytest.raises(ValueError):
            R.gaussian_regularizers(**args)
    for a, c in ((None, None), (torch.zeros(1, 9), None), (torch.zeros(8, 1), None), (None, torch.zeros(1, 1)), (torch.zeros(3, 8, 9), None),
                 (img, torch.zeros(9, 8)), (torch.zeros(9), None)):
        with pytest.raises(ValueError):
            R.render_regularizers(a, c, weights=(1, 1))
