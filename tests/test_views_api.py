"""CPU: the public interface of the view bank (eogs2_amd.views, include/eogs_views.h): the header, the binding table and the
built library agree; the entries refuse bad arguments before a device is touched; `reference_order` is the reference's draw;
`adam_state_dict` gives a torch.optim.Adam its state back bit for bit; every refusal of the Python layer raises before a
launch; and the slot plan (eogs2_amd/csrc/views_plan.h) partitions every slot on the host (tests/views_plan_host.cpp)."""
import ctypes
import os
import random
import re
import shutil
import subprocess
import types

import pytest
import torch

import abi_cases as AC
import views_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def header():
    return AC.header_text("eogs_views.h")


def test_header_and_binding_agree():
    from eogs2_amd import _abi

    names = sorted(set(re.findall(r"\b(eogs_views_[a-z_0-9]+)\s*\(", header())))
    assert names == sorted(_abi.HEADERS["eogs_views.h"]) and len(names) == 4
    assert set(names) <= set(_abi.HIP_ONLY)
    assert not set(names) & AC.elsewhere("eogs_views.h")  # under this header alone
    for name, (res, args) in _abi.HEADERS["eogs_views.h"].items():
        assert res is ctypes.c_int, name  # every entry returns a status
        decl = re.search(name + r"\s*\(([^)]*)\)", header()).group(1)
        assert len(decl.split(",")) == len(args), name
        if name != "eogs_views_wg_bytes":
            assert args[-1] is ctypes.c_void_p and "void* stream" in decl  # the stream is passed in
    defines = dict(re.findall(r"#define\s+(EOGS_VIEWS_[A-Z_]+)\s+(\d+)", header()))
    assert int(defines["EOGS_VIEWS_MAX_SLOTS"]) == _abi.VIEWS_MAX_SLOTS == 32
    assert (int(defines["EOGS_VIEWS_LOAD"]), int(defines["EOGS_VIEWS_STORE"])) == (_abi.VIEWS_LOAD, _abi.VIEWS_STORE) == (1, 2)
    # the descriptors have the header's layout
    assert [f[0] for f in _abi.ViewsSlot._fields_] == ["table", "working", "row_stride", "row_bytes", "flags"]
    assert ctypes.sizeof(_abi.ViewsSlot) == 40
    assert [f[0] for f in _abi.ViewsSchedule._fields_] == ["order", "order_len", "cursor", "current", "n_views"]
    assert ctypes.sizeof(_abi.ViewsSchedule) == 40
    assert _abi.ABI_VERSION == 8


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS

    for n in HEADERS["eogs_views.h"]:
        assert hasattr(hip_lib.cdll, n), n
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only
    assert hip_lib.views_load is not None and hip_lib.views_advance is not None  # the short names resolve
    n = ctypes.c_size_t()
    assert hip_lib.views_wg_bytes(ctypes.byref(n)) == 0
    assert n.value >= 4096 and n.value % 4096 == 0  # whole 16-byte passes of a 256-thread workgroup
    assert hip_lib.views_wg_bytes(None) == -1


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import views as V

    assert eogs2_amd.views is V
    for name in ("reference_order", "ViewSchedule", "ViewBank", "adam_state_dict_from_rows"):
        assert callable(getattr(V, name)) and name in V.__all__


def _schedule(order=256, order_len=4, cursor=512, current=768, n_views=3):
    from eogs2_amd._abi import ViewsSchedule

    return ViewsSchedule(order, order_len, cursor, current, n_views)


def _slots(n, **over):
    from eogs2_amd._abi import ViewsSlot

    arr = (ViewsSlot * max(n, 1))()
    for a in arr:
        a.table, a.working, a.row_stride, a.row_bytes, a.flags = 4096, 8192, 16, 12, 3
        for k, v in over.items():
            setattr(a, k, v)
    return arr


def test_entries_check_their_arguments_without_a_device(hip_lib):
    err = lambda: hip_lib.cdll.eogs_rast_last_error()  # noqa: E731
    ok = _schedule()
    ptr = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    gate = ctypes.c_void_p(1024)
    for call in (lambda n, s, sch: hip_lib.views_load(n, s, sch, None), lambda n, s, sch: hip_lib.views_store(n, s, sch, gate, None)):
        assert call(-1, ptr(_slots(1)), ctypes.byref(ok)) == -1 and b"views_" in err()
        assert call(33, ptr(_slots(33)), ctypes.byref(ok)) == -1 and b"32" in err()
        assert call(1, None, ctypes.byref(ok)) == -1
        assert call(1, ptr(_slots(1)), None) == -1 and b"schedule" in err()
        for bad in (_schedule(order=None), _schedule(cursor=None), _schedule(current=None), _schedule(order_len=0),
                    _schedule(order_len=-3), _schedule(n_views=0), _schedule(n_views=-1), _schedule(order=258), _schedule(cursor=516)):
            assert call(1, ptr(_slots(1)), ctypes.byref(bad)) == -1
            assert call(0, None, ctypes.byref(bad)) == -1  # an empty call still names a schedule
        assert call(1, ptr(_slots(1, row_bytes=10)), ctypes.byref(ok)) == -1 and b"multiple of 4" in err()
        assert call(1, ptr(_slots(1, row_stride=24)), ctypes.byref(ok)) == -1 and b"multiple of 16" in err()
        assert call(1, ptr(_slots(1, row_stride=16, row_bytes=20)), ctypes.byref(ok)) == -1
        assert call(1, ptr(_slots(1, table=None)), ctypes.byref(ok)) == -1
        assert call(1, ptr(_slots(1, working=None)), ctypes.byref(ok)) == -1
        assert call(1, ptr(_slots(1, working=8194)), ctypes.byref(ok)) == -1 and b"aligned" in err()
        assert call(1, ptr(_slots(1, table=4098)), ctypes.byref(ok)) == -1
        assert call(1, ptr(_slots(1, flags=0)), ctypes.byref(ok)) == -1 and b"flags" in err()
        assert call(1, ptr(_slots(1, flags=4)), ctypes.byref(ok)) == -1
        assert call(2, ptr(_slots(2, row_bytes=(1 << 46) - 16, row_stride=1 << 46)), ctypes.byref(ok)) == -5  # EOGS_ERR_OVERFLOW
        assert call(0, None, ctypes.byref(ok)) == 0  # nothing to do, nothing queued
    assert hip_lib.views_store(1, ptr(_slots(1)), ctypes.byref(ok), ctypes.c_void_p(1026), None) == -1 and b"gate" in err()
    assert hip_lib.views_advance(None, None, None) == -1
    assert hip_lib.views_advance(ctypes.byref(_schedule(order_len=0)), None, None) == -1
    assert hip_lib.views_advance(ctypes.byref(_schedule(cursor=None)), None, None) == -1
    assert hip_lib.views_advance(ctypes.byref(ok), ctypes.c_void_p(1026), None) == -1


@pytest.mark.parametrize("V", VC.ORDER_V)
def test_reference_order_is_the_references_draw(V):
    from eogs2_amd.views import reference_order

    for seed, length in ((0, 3 * V), (1, 3 * V + 1), (7, 4 * V + V // 2 + 1), (11, 1), (12, 0)):
        got = reference_order(V, length, VC.seeded(seed))
        assert got == VC.literal_order(V, length, seed) and len(got) == length
        for k in range(0, length - V + 1, V):  # every aligned run of V entries is a permutation
            assert sorted(got[k:k + V]) == list(range(V))
        assert len(set(got[length - length % V:])) == length % V  # the unfinished run repeats no view
    random.seed(5)  # the default rng is the module `random`, as in the reference
    assert reference_order(V, 2 * V + 1) == VC.literal_order(V, 2 * V + 1, 5)
    with pytest.raises(ValueError):
        reference_order(0, 3)


def _separate_adam_runs(steps_per_view, dtype=torch.float32):
    """One torch.optim.Adam with one group per view, views stepped unequally (grad None elsewhere): (optimizer, params)."""
    names = sorted(VC.ADAM_SHAPES)
    params = [[torch.nn.Parameter(VC.adam_initial(n, v).to(dtype)) for n in names] for v in range(VC.ADAM_V)]
    opt = torch.optim.Adam([{"params": ps} for ps in params], lr=VC.ADAM_LR, betas=VC.ADAM_BETAS, eps=VC.ADAM_EPS)
    for v, count in enumerate(steps_per_view):
        for visit in range(count):
            opt.zero_grad(set_to_none=True)
            for n, p in zip(names, params[v]):
                p.grad = VC.adam_grad(n, v, visit).to(dtype)
            opt.step()
    return opt, params


def test_adam_state_dict_restores_a_torch_adam_bit_for_bit():
    from eogs2_amd.views import adam_state_dict_from_rows

    names = sorted(VC.ADAM_SHAPES)
    counts = (3, 0, 5)  # view 1 was never visited: no state, as in torch
    src, src_params = _separate_adam_runs(counts)
    rows = {}
    for k, n in enumerate(names):
        rows[n] = torch.stack([src_params[v][k].detach() for v in range(VC.ADAM_V)])
        for key in ("exp_avg", "exp_avg_sq"):
            rows[f"{n}.{key}"] = torch.stack([src.state[src_params[v][k]][key] if counts[v] else torch.zeros(VC.ADAM_SHAPES[n])
                                              for v in range(VC.ADAM_V)])
        rows[f"{n}.step"] = torch.tensor([float(c) for c in counts])
    group = {k: v for k, v in src.state_dict()["param_groups"][0].items() if k != "params"}
    sd = adam_state_dict_from_rows(rows, names, group)
    want = src.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in want["param_groups"]]
    assert sorted(sd["state"]) == sorted(want["state"])  # the unvisited view has no entry on either side
    for i in want["state"]:
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert VC.same_bits(sd["state"][i][key].float(), want["state"][i][key].float()), (i, key)
    # a fresh optimizer accepts it, and its next step is the source's next step
    params = [[torch.nn.Parameter(rows[n][v].clone()) for n in names] for v in range(VC.ADAM_V)]
    dst = torch.optim.Adam([{"params": ps} for ps in params], lr=VC.ADAM_LR, betas=VC.ADAM_BETAS, eps=VC.ADAM_EPS)
    dst.load_state_dict(sd)
    for v in (0, 1, 2):
        for opt, ps in ((src, src_params), (dst, params)):
            opt.zero_grad(set_to_none=True)
            for n, p in zip(names, ps[v]):
                p.grad = VC.adam_grad(n, v, counts[v])
            opt.step()
    for v in range(VC.ADAM_V):
        for k in range(len(names)):
            a, b = src_params[v][k], params[v][k]
            assert VC.same_bits(a, b)
            for key in ("exp_avg", "exp_avg_sq", "step"):
                assert VC.same_bits(src.state[a][key].float(), dst.state[b][key].float()), (v, k, key)
    with pytest.raises(ValueError):
        adam_state_dict_from_rows(rows, [], group)


def test_schedule_refuses_before_any_device_call():
    from eogs2_amd.views import ViewSchedule

    with pytest.raises(ValueError, match=r"order\[2\] = 3"):
        ViewSchedule([0, 1, 3, 0], 3, "cuda")
    with pytest.raises(ValueError, match=r"order\[0\] = -1"):
        ViewSchedule([-1], 3, "cuda")
    with pytest.raises(ValueError, match="empty"):
        ViewSchedule([], 3, "cuda")
    with pytest.raises(ValueError, match="n_views"):
        ViewSchedule([0], 0, "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ViewSchedule([0, 1], 2, "cpu")


def test_bank_refuses_before_any_launch():
    from eogs2_amd.views import ViewBank

    sched = types.SimpleNamespace(n_views=3, device=torch.device("cuda", 0))  # (what a bank reads of its schedule before a launch)
    bank = ViewBank(sched)
    w = torch.zeros(4, 5)
    rows = [torch.zeros(4, 5) for _ in range(3)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # CPU tensors
        bank.add_input("gt", w, rows)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bank.add_state("p", w)
    with pytest.raises(ValueError, match="contiguous"):
        bank.add_input("gt", torch.zeros(5, 4).t(), rows)
    with pytest.raises(ValueError, match="multiple of 4"):
        bank.add_state("h", torch.zeros(3, dtype=torch.float16))
    with pytest.raises(ValueError, match="multiple of 4"):
        bank.add_state("b", torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="row 1 differs"):
        bank.add_input("gt", w, [rows[0], torch.zeros(5, 4), rows[2]])
    with pytest.raises(ValueError, match="row 2 differs"):
        bank.add_input("gt", w, [rows[0], rows[1], rows[2].double()])
    with pytest.raises(ValueError, match="row 0 differs"):
        bank.add_input("gt", w, torch.zeros(3, 4, 6))
    with pytest.raises(ValueError, match="2 rows for 3 views"):
        bank.add_input("gt", w, rows[:2])
    with pytest.raises(ValueError, match="needs its rows"):
        bank.add_input("gt", w, None)
    with pytest.raises(TypeError):
        bank.add_input("gt", w.numpy(), rows)
    bank._slots["gt"] = object()  # (a slot of that name exists)
    with pytest.raises(ValueError, match="exists already"):
        bank.add_input("gt", w, rows)
    with pytest.raises(ValueError, match="exists already"):
        bank.add_state("gt", w)
    del bank._slots["gt"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bank.add_input("m", w.to("meta"), [r.to("meta") for r in rows])
    assert bank.names() == []  # nothing was registered by the refused calls
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    with pytest.raises(RuntimeError, match="capturable"):
        bank.attach_optimizer(opt)
    with pytest.raises(RuntimeError, match="no optimizer attached"):
        bank.adam_state_dict(["weight"])


def test_slot_plan_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "views_plan_host")
    base = [cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "eogs2_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tests", "views_plan_host.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    build = subprocess.run(base + san, capture_output=True, text=True, timeout=300)
    if build.returncode != 0:  # a compiler without the sanitizers' runtimes: the plain program checks the same properties
        build = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ALL CHECKS PASSED" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert "FAILED" not in run.stdout
