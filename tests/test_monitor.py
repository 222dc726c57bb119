"""CPU: the training monitor (eogs2_amd.monitor, include/eogs_monitor.h). The plain restatement of its semantics
(tests/monitor_cases.py) replays every fixture of tests/golden/monitor/ — made by the reference's own psnr, ssim, l1_loss,
lphotom and early_stopping — bit for bit from the fixture's per-observation fp32 values; header, ctypes tables and library
declare the same entry points and the same state layout; the Python layer refuses what it cannot run."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import abi_cases as AC
import monitor_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "eogs_monitor.h")
NAMES = ("state_bytes", "reset", "observe_bytes", "observe", "model_bytes", "observe_model", "end_iteration", "close_interval")


def test_fixtures_cover_the_sequences():
    assert mc.FIXTURES == ["alternating", "inf_and_nan", "max_patience", "no_pan_interval", "photometric_off"]
    for name in mc.FIXTURES:
        c = mc.load(name)
        assert int(c["iterations"]) <= 40 and c["gt_pan"].shape[0] == 1 and c["gt_msi"].shape[0] == 3
        assert max(c["gt_pan"].shape[1:]) <= 70 and max(c["gt_msi"].shape[1:]) <= 70
        assert os.path.getsize(os.path.join(mc.GOLDEN_DIR, name + ".npz")) < 128 * 1024
        assert len(c["kinds"]) == int(c["cams_per_iter"].sum()) == len(c["l1"]) == len(c["img_pan"]) + len(c["img_msi"])
        finite = np.isfinite(c["psnr"])
        assert (c["psnr"][finite] > 0).all()  # the generator's second guarantee
    a = mc.load("alternating")
    assert int(a["iterations"]) == 37 and int(a["interval"]) == 10 and len(a["rec_iteration"]) == 3  # the last interval stays open
    b = mc.load("max_patience")
    assert str(b["operator"]) == "max" and int(b["stop_interval"]) == 5 and len(b["rec_iteration"]) == 8
    c = mc.load("no_pan_interval")
    assert c["rec_pan_psnr"][1] == 0 and c["rec_counter"][1] == c["rec_counter"][0]
    d = mc.load("photometric_off")
    assert not bool(d["photometric_on"]) and (d["rec_photometric"] == 0).all() and (d["rec_L1"] > 0).all()
    e = mc.load("inf_and_nan")
    assert np.isposinf(e["psnr"]).sum() == 1 and np.isnan(e["psnr"]).sum() == 1 and np.isposinf(e["rec_pan_psnr"][0])


@pytest.mark.parametrize("name", mc.FIXTURES)
def test_restatement_replays_the_reference_bit_for_bit(name):
    c = mc.load(name)
    m = mc.replay(c)
    want = mc.fixture_records(c)
    assert len(m.records) == len(want)
    for got, ref in zip(m.records, want):
        assert mc.same_record(got, ref), mc.record_diff(got, ref)
    assert mc.bits(m.ema_loss) == mc.bits(float(c["final_ema_loss"]))
    assert mc.bits(m.ema_photometric) == mc.bits(float(c["final_ema_photometric"]))
    fired = next((r["interval"] for r in m.records if r["early_stop"]), 0)
    assert fired == int(c["stop_interval"])
    # the photometric value is the fp32 expression of image_utils.py:28 on the stored l1 and ssim
    if bool(c["photometric_on"]):
        p = np.array([mc.photometric_f32(a, b, float(c["lambda_dssim"])) for a, b in zip(c["l1"], c["ssim"])])
        ok = np.isfinite(c["photometric"])
        assert np.allclose(p[ok], c["photometric"][ok], rtol=3e-7, atol=0)  # (torch may fuse nothing here: within an ulp or two)


def test_restatement_edges():
    m = mc.Monitor("pan_psnr", "max", 2)
    m.observe(0.1, 0.9, 0.12, 20.0, "msi")
    m.end_iteration(0.12)
    r = m.close_interval()
    assert r["pan_psnr"] == 0 and r["counter"] == 0 and r["best"] == -math.inf  # metric 0: skipped
    for k in range(3):
        m.observe(0.1, 0.9, 0.12, float("nan"), "pan")
        r = m.close_interval()
        assert math.isnan(r["pan_psnr"]) and r["counter"] == k + 1 and r["early_stop"] == (k + 1 >= 2)  # NaN: no improvement
    m.observe(0.1, 0.9, 0.12, 30.0, "pan")
    r = m.close_interval()
    assert r["best"] == 30.0 and r["counter"] == 0 and r["early_stop"]  # the flag stays, as the reference's
    off = mc.Monitor("L1", "min", None)
    off.observe(0.1, 0.9, 0.12, 20.0, "pan", photometric_on=False)
    r = off.close_interval()
    assert r["L1"] == float(np.float32(0.1)) and r["photometric"] == 0 and r["best"] == math.inf
    with pytest.raises(ValueError):
        off.observe(0.1, 0.9, 0.12, 20.0, "rgb")


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def test_header_abi_and_library_declare_the_same_entry_points(hip_lib):
    from eogs2_amd import _abi

    src = AC.header_text("eogs_monitor.h")
    declared = sorted(set(re.findall(r"\b(eogs_monitor_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(_abi.HEADERS["eogs_monitor.h"]) == sorted("eogs_monitor_" + n for n in NAMES)
    for n in NAMES:
        fn = getattr(hip_lib.cdll, "eogs_monitor_" + n)
        assert "eogs_monitor_" + n in _abi.HIP_ONLY
        assert fn.argtypes == _abi.HEADERS["eogs_monitor.h"]["eogs_monitor_" + n][1]  # bound on load
    # argument counts of the prototypes
    for name, (_, args) in _abi.HEADERS["eogs_monitor.h"].items():
        proto = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", src, flags=re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(args), name
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only


def test_constants_and_layout_agree_with_the_header(hip_lib):
    from eogs2_amd import _abi

    full = open(HEADER).read()
    for i, name in enumerate(_abi.MONITOR_METRICS):
        assert int(re.search(rf"#define EOGS_MONITOR_{name.upper()} (\d+)", full).group(1)) == i
    assert _abi.MONITOR_METRICS == mc.METRICS
    assert int(re.search(r"#define EOGS_MONITOR_METRICS (\d+)", full).group(1)) == len(_abi.MONITOR_METRICS)
    for i, name in enumerate(_abi.MONITOR_KINDS):
        assert int(re.search(rf"#define EOGS_MONITOR_KIND_{name.upper()} (\d+)", full).group(1)) == i
    for i, name in enumerate(_abi.MONITOR_OPERATORS):
        assert int(re.search(rf"#define EOGS_MONITOR_{name.upper()} (\d+)", full).group(1)) == i
    assert int(re.search(r"#define EOGS_MONITOR_RING (\d+)", full).group(1)) == _abi.MONITOR_RING == mc.RING
    n = ctypes.c_size_t()
    hip_lib.check(hip_lib.monitor_state_bytes(ctypes.byref(n)))
    assert n.value == ctypes.sizeof(_abi.MonitorState) and ctypes.sizeof(_abi.MonitorRecord) == 128
    # the struct members, in the header's order
    for struct, cls in (("eogs_monitor_record", _abi.MonitorRecord), ("eogs_monitor_state", _abi.MonitorState)):
        body = re.search(r"typedef struct \{([^{}]*)\}\s*" + struct + ";", re.sub(r"/\*.*?\*/", "", full, flags=re.S), flags=re.S).group(1)
        names = [re.sub(r"\[.*?\]", "", w.strip()) for decl in body.split(";") if decl.strip()
                 for w in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], struct
    # the retired-row rule is eogs_reg.h's constant, used and not copied
    hip = open(os.path.join(ROOT, "eogs2_amd", "csrc", "monitor.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert "EOGS_REG_RETIRED_BELOW" in code and "5.0e29" not in hip and "atomic" not in code.lower()  # no atomics, of any type


def test_size_queries_and_argument_checks_need_no_device(hip_lib):
    n, m = ctypes.c_size_t(), ctypes.c_size_t()
    hip_lib.check(hip_lib.monitor_observe_bytes(3, 1024, 1024, 0, ctypes.byref(n)))
    hip_lib.check(hip_lib.monitor_observe_bytes(3, 1024, 1024, 1, ctypes.byref(m)))
    assert 0 < n.value < (1 << 16) and m.value > n.value + 3 * 3 * 1024 * 1024 * 4  # stand-alone: the loss's three maps as well
    hip_lib.check(hip_lib.monitor_model_bytes(1 << 20, ctypes.byref(n)))
    assert 0 < n.value < (1 << 16)
    assert hip_lib.monitor_state_bytes(None) == -1 and hip_lib.monitor_model_bytes(0, ctypes.byref(n)) == -1
    for planes, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (70000, 8, 8)):
        assert hip_lib.monitor_observe_bytes(planes, H, W, 0, ctypes.byref(n)) == -1
    one, big = ctypes.c_void_p(256), 1 << 30  # never dereferenced: every call below is answered before anything touches a device
    obs = hip_lib.monitor_observe
    assert obs(1, 8, 8, one, one, one, 0.2, 2, 1, None, one, one, big, None) == -1
    assert b"pan or msi" in hip_lib.cdll.eogs_rast_last_error()
    assert obs(0, 8, 8, one, one, one, 0.2, 0, 1, None, one, one, big, None) == -1
    assert obs(1, 8, 8, None, one, one, 0.2, 0, 1, None, one, one, big, None) == -1
    assert obs(1, 8, 8, one, None, one, 0.2, 0, 1, None, one, one, big, None) == -1
    assert obs(1, 8, 8, one, one, one, 0.2, 0, 1, None, one, None, big, None) == -1
    assert obs(1, 8, 8, one, one, one, 0.2, 0, 1, None, None, one, big, None) == -1
    assert b"NULL state" in hip_lib.cdll.eogs_rast_last_error()
    assert obs(1, 8, 8, one, one, one, 0.2, 0, 1, None, ctypes.c_void_p(264), one, big, None) == -1
    assert obs(1, 8, 8, one, one, one, float("nan"), 0, 1, None, one, one, big, None) == -1
    assert obs(1, 8, 8, one, one, one, 0.2, 0, 1, None, one, one, 8, None) == -3
    assert obs(1, 64, 64, one, one, None, 0.2, 0, 1, None, one, one, 4096, None) == -3  # stand-alone needs the loss's workspace
    assert b"workspace" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.monitor_observe_model(0, one, None, one, one, big, None) == -1
    assert hip_lib.monitor_observe_model(8, None, None, one, one, big, None) == -1
    assert hip_lib.monitor_observe_model(8, one, None, one, one, 8, None) == -3
    assert hip_lib.monitor_end_iteration(None, None, one, None) == -1 and hip_lib.monitor_end_iteration(one, None, None, None) == -1
    assert hip_lib.monitor_close_interval(6, 0, 5, None, one, None) == -1
    assert b"metric" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.monitor_close_interval(0, 2, 5, None, one, None) == -1
    assert b"min or max" in hip_lib.cdll.eogs_rast_last_error()
    assert hip_lib.monitor_close_interval(0, 0, 5, None, None, None) == -1
    assert hip_lib.monitor_reset(one, 8, 0, None) == -3 and hip_lib.monitor_reset(one, big, 3, None) == -1
    assert hip_lib.monitor_reset(None, big, 0, None) == -1


def test_python_layer_refuses_what_it_cannot_run():
    import eogs2_amd
    from eogs2_amd import monitor as M

    assert eogs2_amd.monitor is M and "TrainingMonitor" in M.__all__
    mon = M.TrainingMonitor("cuda:0", metric_name="pan_psnr", operator="max", patience=3)  # touches no device
    img = torch.zeros(3, 8, 9)
    for call in (lambda: mon.observe(img, img, "msi"), lambda: mon.observe(img[:1], img[:1], "pan", loss_out=torch.zeros(3)),
                 lambda: mon.observe_model(torch.zeros(6, 1)), lambda: mon.end_iteration(torch.zeros(())),
                 lambda: mon.close_interval(gate=torch.ones(2, dtype=torch.int32)), lambda: M.TrainingMonitor("cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for kind in ("rgb", "PAN", None, 0):
        with pytest.raises(ValueError, match="Unknown camera type .* should be either 'pan' or 'msi'"):
            mon.observe(img, img, kind)
    for name in ("mae", "mae_wtree", "psnr", "ssim", ""):
        with pytest.raises(ValueError) as e:
            M.TrainingMonitor("cuda:0", metric_name=name)
        assert all(k in str(e.value) for k in mc.METRICS), name  # the message names the six
    for op in ("minimum", "MAX", None):
        with pytest.raises(ValueError, match="operator should be either min or max"):
            M.TrainingMonitor("cuda:0", operator=op)
    with pytest.raises(ValueError):
        M.TrainingMonitor("cuda:0", patience=-2)
    assert M.TrainingMonitor("cuda:0", patience=None).patience == -1  # use_early_stopping: False


def test_photometric_loss_keeps_its_return_value():
    import inspect

    from eogs2_amd import losses

    sig = inspect.signature(losses.photometric_loss)
    assert list(sig.parameters) == ["image", "gt_image", "lambda_dssim", "return_out"] and sig.parameters["return_out"].default is False
