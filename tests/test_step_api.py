"""CPU: the C-ABI of include/eogs_step.h (the optimizer step inside a recorded graph) is declared, bound and checked the way
the other headers are: header and binding agree, the symbols are exported, argument errors come back with their message
before anything touches a device. No compute call is made (there is no GPU here)."""
import ctypes
import os
import re

import pytest
import torch

import abi_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declarations():
    """{symbol: number of parameters} of the functions include/eogs_step.h declares."""
    src = AC.header_text("eogs_step.h")
    return {name: len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
            for name, args in re.findall(r"\bint\s+(eogs_step_[a-z_0-9]+)\s*\(([^)]*)\)", src)}


def test_header_and_binding_agree():
    from eogs2_amd import _abi

    decl = _declarations()
    assert sorted(decl) == sorted(_abi.HEADERS["eogs_step.h"]) and len(decl) == 3
    for name, (res, args) in _abi.HEADERS["eogs_step.h"].items():
        assert res is ctypes.c_int and len(args) == decl[name], name
        assert name in _abi.HIP_ONLY, name
    assert not set(_abi.HEADERS["eogs_step.h"]) & AC.elsewhere("eogs_step.h")
    # the structs are those of the header, field for field
    assert [f[0] for f in _abi.StepForward._fields_] == ["geom", "geom_bytes", "P", "capacity"]
    assert [f[0] for f in _abi.StepAdamTensor._fields_] == ["param", "grad", "exp_avg", "exp_avg_sq", "numel", "lr", "step", "retire_below"]
    assert [f[0] for f in _abi.StepAdamScalars._fields_] == ["lr", "inv_bc1", "sqrt_bc2", "skip"]
    assert ctypes.sizeof(_abi.StepAdamScalars) == 16 and ctypes.sizeof(_abi.StepAdamTensor) == 64


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def test_library_exports_and_binds_the_symbols(hip_lib):
    from eogs2_amd._abi import HEADERS

    assert hip_lib.backend == "hip-gfx950"
    assert hip_lib.cdll.eogs_rast_abi_version() == 8
    for name, (res, args) in HEADERS["eogs_step.h"].items():
        fn = getattr(hip_lib.cdll, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert hip_lib.step_adam is hip_lib.cdll.eogs_step_adam or hip_lib.step_adam.argtypes == hip_lib.cdll.eogs_step_adam.argtypes


def _err(lib):
    return lib.cdll.eogs_rast_last_error().decode()


def test_argument_errors_touch_no_device(hip_lib):
    from eogs2_amd._abi import StepAdamTensor, StepForward

    n = ctypes.c_size_t()
    assert hip_lib.step_adam_bytes(16, ctypes.byref(n)) == 0 and n.value == 16 * 16
    assert hip_lib.step_adam_bytes(17, ctypes.byref(n)) == -1 and "step_adam_bytes" in _err(hip_lib)
    assert hip_lib.step_adam_bytes(3, ctypes.byref(n)) == 0 and n.value == 48
    fake = 0x1000  # never dereferenced: every check below fails on the host
    arr = (StepAdamTensor * 17)()
    for a in arr:
        a.param = a.grad = a.exp_avg = a.exp_avg_sq = a.lr = a.step = fake
        a.numel, a.retire_below = 8, float("-inf")
    tensors = ctypes.cast(arr, ctypes.c_void_p)
    ws = ctypes.c_void_p(fake)
    assert hip_lib.step_adam(17, tensors, 0.9, 0.999, 1e-8, None, ws, 17 * 16, None) == -1
    assert "at most 16 tensors" in _err(hip_lib)
    assert hip_lib.step_adam(-1, tensors, 0.9, 0.999, 1e-8, None, ws, 256, None) == -1
    assert hip_lib.step_adam(3, None, 0.9, 0.999, 1e-8, None, ws, 48, None) == -1
    assert "NULL tensors" in _err(hip_lib)
    assert hip_lib.step_adam(3, tensors, 0.9, 0.999, 1e-8, None, ws, n.value - 1, None) == -3
    assert "workspace too small" in _err(hip_lib)
    assert hip_lib.step_adam(3, tensors, 0.9, 0.999, 1e-8, None, None, n.value, None) == -3
    arr[1].step = None
    assert hip_lib.step_adam(3, tensors, 0.9, 0.999, 1e-8, None, ws, n.value, None) == -1
    assert "NULL tensor member" in _err(hip_lib)
    arr[1].step, arr[2].numel, arr[2].grad = fake, 0, None  # an empty tensor may have NULL arrays ...
    arr[0].grad = None  # ... a non-empty one may not
    assert hip_lib.step_adam(3, tensors, 0.9, 0.999, 1e-8, None, ws, n.value, None) == -1
    assert hip_lib.step_adam(0, None, 0.9, 0.999, 1e-8, None, None, 0, None) == 0
    # gate: the same discipline
    fw = (StepForward * 17)()
    gate = ctypes.c_void_p(fake)
    assert hip_lib.step_gate(17, ctypes.cast(fw, ctypes.c_void_p), 0, gate, None) == -1 and "step_gate" in _err(hip_lib)
    assert hip_lib.step_gate(1, None, 0, gate, None) == -1
    assert hip_lib.step_gate(0, None, 0, None, None) == -1  # (n == 0 still writes the gate: it needs one)
    fw[0].geom, fw[0].geom_bytes, fw[0].P, fw[0].capacity = fake, 64, 1000, 5
    assert hip_lib.step_gate(1, ctypes.cast(fw, ctypes.c_void_p), 0, gate, None) == -3 and "geom workspace too small" in _err(hip_lib)


def test_capacity_token_keeps_its_rule(hip_lib):
    """eogs_rast_capacity_token's *fits now goes through the shared rule of csrc/common.h: what it returns is unchanged."""
    cap, fits = ctypes.c_int64(), ctypes.c_int()
    pack = lambda slots, entries: (entries << 32) | slots  # csrc/common.h nr_pack with every flag clear
    hip_lib.check(hip_lib.capacity_token(1000, pack(10_000, 2_000), 0.0, 0, pack(10_000, 2_000), ctypes.byref(cap), ctypes.byref(fits)))
    slots, entries = cap.value & 0x7FFFFFFF, (cap.value >> 32) & 0x07FFFFFF
    assert (slots, entries) == (10_000 + 4096, 2_000 + 1024) and fits.value == 1
    for exact, want in ((pack(slots, entries), 1), (pack(slots + 1, entries), 0), (pack(slots, entries + 1), 0), (0, 1), (-1, 0)):
        hip_lib.check(hip_lib.capacity_token(1000, pack(10_000, 2_000), 0.0, 0, exact, ctypes.byref(cap), ctypes.byref(fits)))
        assert fits.value == want, (exact, want)


def test_fused_adam_capturable_keyword():
    from eogs2_amd.optim import FusedAdam

    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdam([{"params": [p], "lr": 1e-2, "name": "opacity"}], lr=0.0, eps=1e-15)
    assert opt.defaults["capturable"] is False and opt.param_groups[0]["capturable"] is False
    p.grad = torch.ones(4)
    opt.retire_below = {"opacity": -6.0}
    with pytest.raises(RuntimeError, match="capturable=True"):
        opt.step()
    opt.retire_below = {}
    with pytest.raises(RuntimeError, match="capturable=True"):
        opt.step(gate=torch.zeros(2, dtype=torch.int32))
    assert "step" not in opt.state[p] and float(p.detach().abs().sum()) == 0.0  # refused before anything was counted
    cap = FusedAdam([{"params": [p], "lr": 1e-2, "name": "opacity"}], lr=0.0, eps=1e-15, capturable=True)
    assert cap.defaults["capturable"] is True and cap.param_groups[0]["capturable"] is True
