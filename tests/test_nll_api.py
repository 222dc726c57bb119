"""CPU: the surface of the transient-uncertainty term (include/eogs_nll.h, eogs2_amd.uncertainty) without a device — header
and binding table, every refusal before a launch, the fixtures of tests/golden/nll regenerated bit for bit, and the numpy
statement of the bound (tests/nll_cases.py): it accepts torch-float32's own results and rejects two wrong gradient rules."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import abi_cases as AC
import nll_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def test_header_table_and_constants_agree():
    from eogs2_amd import _abi

    assert _abi.ABI_VERSION == 8  # entry points were added, nothing changed
    decl = AC.declared("eogs_nll.h")
    assert sorted(decl) == sorted(_abi.HEADERS["eogs_nll.h"]) == ["eogs_nll_backward", "eogs_nll_bytes", "eogs_nll_forward"]
    for name, (res, args) in _abi.HEADERS["eogs_nll.h"].items():
        assert decl[name] == len(args) and res is ctypes.c_int, name
    defines = dict(re.findall(r"#define (EOGS_NLL_[A-Z]+) (\d+)u", AC.header_text("eogs_nll.h")))
    assert {k: int(v) for k, v in defines.items()} == {"EOGS_NLL_MASK": _abi.NLL_MASK, "EOGS_NLL_FULL": _abi.NLL_FULL, "EOGS_NLL_SUM": _abi.NLL_SUM}
    assert len(os.listdir(AC.INCLUDE)) == 22


def test_library_refuses_before_a_launch(lib):
    """Every refusal of the C-ABI comes back as a status with a message and before anything touches a device (there is none
    here): the pointers are made up and never read."""
    assert lib.cdll.eogs_rast_abi_version() == 8
    n = ctypes.c_size_t()
    lib.check(lib.nll_bytes(3, 37, 53, ctypes.byref(n)))
    ws = n.value
    assert 0 < ws <= 1 << 16
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert lib.nll_bytes(*bad, ctypes.byref(n)) == -1 and b"nll_bytes" in lib.cdll.eogs_rast_last_error()
    assert lib.nll_bytes(1, 1, 1, None) == -1
    p = ctypes.c_void_p(0x1000)  # (never dereferenced: every call below is refused)

    def fwd(planes=3, H=4, W=5, mode=1, x=p, t=p, vm=p, vp=1, floor=1e-3, eps=1e-6, w=None, out=p, ws_=p, nbytes=ws):
        return lib.nll_forward(planes, H, W, mode, x, t, vm, vp, floor, eps, w, out, ws_, nbytes, None)

    def bwd(planes=3, H=4, W=5, mode=1, x=p, t=p, vm=p, vp=1, floor=1e-3, eps=1e-6, g_in=p, g_vm=p):
        return lib.nll_backward(planes, H, W, mode, x, t, vm, vp, floor, eps, None, None, None, g_in, g_vm, None)

    refusals = [dict(planes=0), dict(H=0), dict(W=-1), dict(mode=1, vp=3), dict(mode=0, vp=2), dict(mode=0, vp=0), dict(mode=8),
                dict(floor=-1e-3), dict(floor=float("nan")), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")),
                dict(x=None), dict(t=None), dict(vm=None)]
    for kw in refusals:
        for f in (fwd, bwd):
            assert f(**kw) < 0, kw
            msg = lib.cdll.eogs_rast_last_error()
            assert msg.startswith(b"nll_forward" if f is fwd else b"nll_backward"), (kw, msg)
    assert fwd(out=None) < 0 and fwd(ws_=None) < 0
    assert fwd(nbytes=ws - 1) < 0 and b"workspace too small" in lib.cdll.eogs_rast_last_error()
    assert bwd(g_in=None, g_vm=None) < 0 and b"both outputs NULL" in lib.cdll.eogs_rast_last_error()


def test_python_refuses_before_a_launch(monkeypatch):
    from eogs2_amd import uncertainty as U

    def no_launch(*a, **k):
        raise AssertionError("a refusal came after a launch")

    monkeypatch.setattr(U, "call", no_launch)
    x, t, m = torch.rand(3, 5, 7), torch.rand(3, 5, 7), torch.rand(5, 7)
    for f in (lambda: U.transient_nll(x, t, m), lambda: U.gaussian_nll_loss(x, t, m), lambda: U.TransientNLL(0.1)(x, t, m),
              lambda: U.transient_nll(x, t, m, weight=torch.ones(1))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.transient_parameters(4, 4, 0.1, "cpu")
    with pytest.raises(TypeError, match="float32"):
        U.transient_nll(x.double(), t.double(), m)
    with pytest.raises(TypeError, match="float32"):
        U.transient_nll(x, t, m.half())
    with pytest.raises(TypeError, match="float32"):
        U.gaussian_nll_loss(x, t.double(), m)
    with pytest.raises(ValueError, match="the target has the input's shape"):
        U.transient_nll(x, t[:2], m)
    with pytest.raises(ValueError, match="the transient mask has one of the shapes"):
        U.transient_nll(x, t, torch.rand(3, 5, 7))  # a mask is one plane
    with pytest.raises(ValueError, match="var has one of the shapes"):
        U.gaussian_nll_loss(x, t, torch.rand(2, 5, 7))
    with pytest.raises(ValueError, match="empty"):
        U.transient_nll(torch.rand(3, 0, 7), torch.rand(3, 0, 7), torch.rand(0, 7))
    with pytest.raises(ValueError, match="batched inputs are not provided"):
        U.gaussian_nll_loss(x[None], t[None], m)
    with pytest.raises(NotImplementedError, match="reduction='none'"):
        U.gaussian_nll_loss(x, t, m, reduction="none")
    with pytest.raises(ValueError, match="total is not valid"):  # torch's own words
        U.gaussian_nll_loss(x, t, m, reduction="total")
    with pytest.raises(RuntimeError, match="the ground truth takes no gradient"):
        U.transient_nll(x, t.clone().requires_grad_(True), m)
    with pytest.raises(ValueError, match="floor"):
        U.transient_nll(x, t, m, floor=-1.0)
    with pytest.raises(ValueError, match="eps"):
        U.gaussian_nll_loss(x, t, m, eps=0.0)
    with pytest.raises(RuntimeError, match="no forward has run"):
        U.TransientNLL(0.1).log_stats()


def test_fixtures_regenerate_bit_for_bit():
    spec = importlib.util.spec_from_file_location("make_golden_nll", os.path.join(ROOT, "tests", "golden", "make_golden_nll.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for name in nc.FIXTURES:
            fx, again = nc.load(name), gen.fixture(name)
            assert sorted(fx) == sorted(again), name
            for k in fx:
                assert fx[k].dtype == again[k].dtype and fx[k].shape == again[k].shape, (name, k)
                assert fx[k].tobytes() == np.ascontiguousarray(again[k]).tobytes(), (name, k)
            assert os.path.getsize(os.path.join(nc.GOLDEN, name + ".npz")) < 1 << 18
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("name", nc.FIXTURES)
def test_the_restatement_is_torch_float64(name):
    """tests/nll_cases.py's numpy float64 (the reference of the GPU cases that are too large for a file) against torch's own
    float64 run: the two differ by float64 roundings, a 2^-29 th of the bound."""
    c = nc.case(name)
    (image, gt, vm), ref = nc.fixture_reference(name)
    mine = nc.restate(image, gt, vm, c["kind"], c["full"], c["sum"])
    mult = nc.multiples({k: mine[k] for k in ("loss", "g_input", "g_vm", "mean", "std") if not c["scalars_only"] or k in ("loss", "mean", "std")}, ref)
    assert max(mult.values()) <= 1e-6, mult
    specials = nc.MASK_SPECIALS if c["kind"] == "mask" else nc.VAR_SPECIALS
    if vm.size > 100 and c.get("constant") is None:  # the case holds every special value it is there for
        assert all((vm == np.float32(s)).any() for s in specials), name
        r = np.abs(image.astype(np.float64) - gt)
        assert (r == 0).any() and r.max() >= 0.999


@pytest.mark.parametrize("name", nc.FIXTURES)
def test_the_bound_accepts_torch_float32(name):
    """The bound is not tighter than the reference's own arithmetic: torch's float32 run of the two statements lies inside it.
    One exception, and the reason the kernel forms the standard deviation from (n, mean, M2): Tensor.std() of the constant
    float32 mask 0.1 is 1.5e-8 in float32, not 0 (its mean rounds away from 0.1), so that one number is left out here."""
    c = nc.case(name)
    fx = nc.load(name)
    _, ref = nc.fixture_reference(name, fx)
    keys = ("loss", "mean", "std") + (() if c["scalars_only"] else ("g_input", "g_vm"))
    got = {k: fx[k + "@32"] for k in keys}
    if c["constant"] is not None:
        assert ref["std"] == 0.0 and 0.0 < float(got.pop("std")) < 1e-7
    nc.check(got, ref, name + " torch-fp32")


def test_the_bound_rejects_wrong_gradient_rules():
    # the clamp's gradient mask with exclusive bounds: m = 0 and m = 1 (and -0) lose their gradient
    (image, gt, vm), ref = nc.fixture_reference("mask_3x37x53")
    wrong = nc.restate(image, gt, vm, "mask", exclusive_clamp=True)
    at_edge = (vm == 0) | (vm == 1)
    assert at_edge.sum() >= 3 and (ref["g_vm"][at_edge] != 0).all() and (wrong["g_vm"][at_edge] == 0).all()
    assert (ref["g_vm"][(vm < 0) | (vm > 1)] == 0).all() and (vm == -0.5).any() and (vm == 1.5).any()
    with pytest.raises(AssertionError, match="g_vm"):
        nc.check({"g_vm": wrong["g_vm"].astype(np.float32)}, ref, "exclusive clamp")
    nc.check({"g_vm": ref["g_vm"].astype(np.float32)}, ref, "inclusive clamp, rounded to float32")
    # d/dv zeroed below eps (what a clamp inside autograd would give): var 0 and 1e-8 lose their gradient
    for name in ("var_shared_3x37x53", "var_planes_3x37x53_full_sum"):
        c = nc.case(name)
        (image, gt, vm), ref = nc.fixture_reference(name)
        wrong = nc.restate(image, gt, vm, "var", c["full"], c["sum"], zero_below_eps=True)
        below = vm < np.float32(nc.EPS)
        assert below.sum() >= 10 and (ref["g_vm"][below] != 0).all()
        with pytest.raises(AssertionError, match="g_vm"):
            nc.check({"g_vm": wrong["g_vm"].astype(np.float32)}, ref, name + " zero below eps")
