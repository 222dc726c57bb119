"""CPU: the public interface of the report module (eogs2_amd.report, include/eogs_report.h): the header, the binding table and
the built library agree; the C entries refuse bad arguments before a device is touched; the Python layer refuses CPU tensors,
wrong dtypes and shapes, non-contiguous tensors, overlapping outputs and more descriptors than a call takes before any
launch; the converters keep the reference's names and errors."""
import ctypes
import os
import re
import types

import pytest
import torch

import abi_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def header():
    return AC.header_text("eogs_report.h")


def test_header_and_binding_agree():
    from eogs2_amd import _abi

    names = sorted(set(re.findall(r"\b(eogs_report_[a-z_0-9]+)\s*\(", header())))
    assert names == sorted(_abi.HEADERS["eogs_report.h"]) == ["eogs_report_cc_to_test", "eogs_report_metrics_accumulate", "eogs_report_metrics_bytes",
                                                      "eogs_report_metrics_reset", "eogs_report_normalize_rows", "eogs_report_pack",
                                                      "eogs_report_recompose"]
    assert set(names) <= set(_abi.HIP_ONLY)
    assert not set(names) & AC.elsewhere("eogs_report.h")  # under this header alone
    for name, (res, args) in _abi.HEADERS["eogs_report.h"].items():
        assert res is ctypes.c_int, name
        decl = re.search(name + r"\s*\(([^)]*)\)", header()).group(1)
        assert len(decl.split(",")) == len(args), name
        if name != "eogs_report_metrics_bytes":
            assert args[-1] is ctypes.c_void_p and "void* stream" in decl
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(EOGS_REPORT_[A-Z_0-9]+)\s+(\d+)u?\b", header())}
    assert defines["EOGS_REPORT_MAX_CAMERAS"] == _abi.REPORT_MAX_CAMERAS == 64
    assert defines["EOGS_REPORT_MAX_ITEMS"] == _abi.REPORT_MAX_ITEMS == 16
    assert defines["EOGS_REPORT_MAX_CHANNELS"] == _abi.REPORT_MAX_CHANNELS == 4
    assert defines["EOGS_REPORT_PACK_MAX_CHANNELS"] == _abi.REPORT_PACK_MAX_CHANNELS == 5
    assert defines["EOGS_REPORT_MAX_CC_ELEMS"] == _abi.REPORT_MAX_CC_ELEMS
    assert (defines["EOGS_REPORT_CC_REF"], defines["EOGS_REPORT_CC_AVERAGE"]) == (_abi.REPORT_CC_REF, _abi.REPORT_CC_AVERAGE)
    assert _abi.REPORT_KINDS[defines["EOGS_REPORT_KIND_PAN"]] == "pan" and _abi.REPORT_KINDS[defines["EOGS_REPORT_KIND_MSI"]] == "msi"
    assert (defines["EOGS_REPORT_FLOAT_HWC"], defines["EOGS_REPORT_U8_ROUND"], defines["EOGS_REPORT_U8_TRUNC"]) == \
        (_abi.REPORT_FLOAT_HWC, _abi.REPORT_U8_ROUND, _abi.REPORT_U8_TRUNC)
    assert (defines["EOGS_REPORT_REVERSE"], defines["EOGS_REPORT_REPLICATE"], defines["EOGS_REPORT_PREMAP"]) == \
        (_abi.REPORT_REVERSE, _abi.REPORT_REPLICATE, _abi.REPORT_PREMAP)
    assert ctypes.sizeof(_abi.ReportTable) == 64 and ctypes.sizeof(_abi.ReportCamera) == 16 and ctypes.sizeof(_abi.ReportItem) == 56
    assert _abi.ABI_VERSION == 8  # additions only


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS

    for n in HEADERS["eogs_report.h"]:
        assert hasattr(hip_lib.cdll, n), n
    assert hip_lib.cdll.eogs_rast_abi_version() == 8
    assert hip_lib.report_pack is not None and hip_lib.report_metrics_accumulate is not None  # the short names resolve


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import report as R

    assert eogs2_amd.report is R
    for name in ("normalize_before_saving", "normalize_colors_", "load_convert_color_correction_train_to_test", "ReportAccumulator",
                 "evaluate_views", "pack_products", "video_frame", "view_products", "fetch_products"):
        assert callable(getattr(R, name)) and name in R.__all__
    assert R.KINDS == ("pan", "msi") and set(R.MODES) == {"float", "u8_round", "u8_trunc"}


def test_entries_check_their_arguments_without_a_device(hip_lib):
    from eogs2_amd._abi import ReportCamera, ReportItem

    err = lambda: hip_lib.cdll.eogs_rast_last_error()  # noqa: E731
    p = ctypes.c_void_p
    # rows
    assert hip_lib.report_normalize_rows(-1, p(4096), p(8192), p(8256), None) == -1
    assert hip_lib.report_normalize_rows(8, p(4096), None, p(8256), None) == -1 and b"NULL" in err()
    assert hip_lib.report_normalize_rows(8, p(4098), p(8192), p(8256), None) == -1 and b"aligned" in err()
    assert hip_lib.report_normalize_rows(8, p(4096), p(4100), p(8256), None) == -1 and b"overlaps" in err()
    assert hip_lib.report_normalize_rows(0, None, p(8192), p(8256), None) == 0  # nothing to do, nothing queued
    # cameras
    def table(pairs):
        arr = (ReportCamera * len(pairs))()
        for a, (w, b) in zip(arr, pairs):
            a.weight, a.bias = w, b
        return ctypes.cast(arr, p), arr

    many, keep = table([(4096 + 64 * i, 4096 + 64 * i + 36) for i in range(65)])
    assert hip_lib.report_recompose(65, many, p(4096), p(4132), None) == -1 and b"64" in err()
    two, keep2 = table([(4096, 4132), (4100, 8192)])
    assert hip_lib.report_recompose(2, two, p(4096), p(4132), None) == -1 and b"overlap" in err()
    one, keep3 = table([(4096, 4132)])
    assert hip_lib.report_recompose(1, one, p(4100), p(8192), None) == -1 and b"partly overlaps" in err()
    assert hip_lib.report_recompose(1, one, None, p(8192), None) == -1
    assert hip_lib.report_recompose(0, None, p(4096), p(4132), None) == 0
    tr, keep4 = table([(4096, 4132), (4160, 4196)])
    te, keep5 = table([(8192, 8228)])
    assert hip_lib.report_cc_to_test(7, 2, tr, 1, te, 9, 3, None) == -1 and b"mode" in err()
    assert hip_lib.report_cc_to_test(1, 0, tr, 1, te, 9, 3, None) == -1
    assert hip_lib.report_cc_to_test(1, 2, tr, 1, te, 14, 3, None) == -1 and b"element counts" in err()
    assert hip_lib.report_cc_to_test(1, 2, tr, 1, tr, 9, 3, None) == -1 and b"overlaps a train" in err()
    assert hip_lib.report_cc_to_test(1, 2, tr, 0, None, 9, 3, None) == 0
    # metrics
    n = ctypes.c_size_t()
    assert hip_lib.report_metrics_bytes(ctypes.byref(n)) == 0 and n.value >= 1024 * 8 * 8
    assert hip_lib.report_metrics_bytes(None) == -1
    assert hip_lib.report_metrics_reset(None, None) == -1
    args = lambda C=3, H=4, W=4, img=4096, gt=8192, kind=1, tab=16384, gate=None, ws=32768, nb=None: (  # noqa: E731
        C, H, W, p(img), p(gt), kind, p(tab), gate, p(ws), n.value if nb is None else nb, None)
    assert hip_lib.report_metrics_accumulate(*args(C=5)) == -1 and b"1 to 4 channels" in err()
    assert hip_lib.report_metrics_accumulate(*args(C=0)) == -1
    assert hip_lib.report_metrics_accumulate(*args(H=0)) == -1
    assert hip_lib.report_metrics_accumulate(*args(kind=2)) == -1 and b"kind" in err()
    assert hip_lib.report_metrics_accumulate(*args(nb=64)) == -3
    assert hip_lib.report_metrics_accumulate(*args(tab=4100)) == -1
    assert hip_lib.report_metrics_accumulate(*args(tab=4128)) == -1 and b"overlaps" in err()
    assert hip_lib.report_metrics_accumulate(*args(gate=p(4097))) == -1
    # pack
    def items(**kw):
        arr = (ReportItem * 1)()
        d = dict(src=4096, C=3, H=4, W=4, mode=0, dst_offset=0, dst_pitch=48, flags=0, lo=0.0, d=1.0)
        d.update(kw)
        for k, v in d.items():
            setattr(arr[0], k, v)
        return ctypes.cast(arr, p), arr

    dst, nbytes = p(1 << 20), 4 * 4 * 3 * 4
    assert hip_lib.report_pack(17, items()[0], dst, nbytes, None) == -1 and b"16" in err()
    assert hip_lib.report_pack(0, None, None, 0, None) == 0
    for kw, word in ((dict(C=6), b"1 to 5"), (dict(mode=3), b"mode"), (dict(flags=8), b"flag"), (dict(flags=2), b"REPLICATE"),
                     (dict(dst_pitch=44), b"pitch"), (dict(dst_offset=2), b"multiples of 4"), (dict(dst_offset=16), b"leaves dst"),
                     (dict(src=(1 << 20) + 8), b"overlaps dst"), (dict(src=0), b"NULL")):
        it, keep6 = items(**kw)
        assert hip_lib.report_pack(1, it, dst, nbytes, None) == -1 and word in err(), kw


def cam(w, b, is_ref=False):
    conv = types.SimpleNamespace(weight=w, bias=b)
    return types.SimpleNamespace(color_correction=conv, is_reference_camera=is_ref)


def test_converters_keep_the_references_names_and_errors():
    from eogs2_amd import report as R

    assert isinstance(R.load_convert_color_correction_train_to_test("ref"), R.perform_cc_by_ref_test)
    assert isinstance(R.load_convert_color_correction_train_to_test("average"), R.perform_average_cc_test)
    for c in (R.perform_cc_by_ref_test, R.perform_average_cc_test):
        assert issubclass(c, R.base_cc_train_to_test) and callable(c.perform_cc_to_test) and callable(c.correct_test_cameras)
    with pytest.raises(NotImplementedError):
        R.load_convert_color_correction_train_to_test("closesttime")
    with pytest.raises(NotImplementedError, match="nearest"):
        R.load_convert_color_correction_train_to_test("nearest")
    with pytest.raises(NotImplementedError):
        R.load_convert_color_correction_train_to_test()
    w, b = torch.zeros(3, 3, 1, 1), torch.zeros(3)
    with pytest.raises(ValueError, match="No reference camera"):
        R.perform_cc_by_ref_test().correct_test_cameras([cam(w, b), cam(w.clone(), b.clone())], [cam(w.clone(), b.clone())])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.perform_average_cc_test().correct_test_cameras([cam(w, b)], [cam(w.clone(), b.clone())])
    with pytest.raises(ValueError, match="shape"):
        R.check_cc_to_test([(w, b)], [(torch.zeros(1, 1, 1, 1), b.clone())])
    with pytest.raises(ValueError, match="at most 64"):
        R.check_cc_to_test([(w, b)] * 65, [])
    # get_list_cam: MSI first, then PAN, as opt says
    vp = types.SimpleNamespace(get_msi_cameras=lambda: "m", get_pan_cameras=lambda: "p")
    opt = lambda m, p: types.SimpleNamespace(load_msi=m, load_pan=p)  # noqa: E731
    assert R.get_list_cam(vp, opt(True, True)) == ["m", "p"] and R.get_list_cam(vp, opt(False, True)) == ["p"]
    assert R.get_list_cam(vp, opt(True, False)) == ["m"] and R.get_list_cam(vp, opt(False, False)) == []


def test_normalize_refuses_before_any_launch():
    from eogs2_amd import report as R

    f, w, b = torch.zeros(8, 1, 3), torch.eye(3).reshape(3, 3, 1, 1).contiguous(), torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.normalize_colors_(f, w, b, [w], [b])
    with pytest.raises(TypeError):
        R.check_normalize(None, w, b, [w], [b])
    with pytest.raises(ValueError, match="float32"):
        R.check_normalize(f.double(), w, b, [w], [b])
    with pytest.raises(ValueError, match=r"\(P, 1, 3\)"):
        R.check_normalize(torch.zeros(8, 3, 1), w, b, [w], [b])
    with pytest.raises(ValueError, match="contiguous"):
        R.check_normalize(torch.zeros(8, 1, 6)[:, :, ::2], w, b, [w], [b])
    with pytest.raises(ValueError, match="9 elements"):
        R.check_normalize(f, torch.zeros(3, 4), b, [w], [b])
    with pytest.raises(ValueError, match="weights for"):
        R.check_normalize(f, w, b, [w], [])
    with pytest.raises(ValueError, match="at most 64"):
        R.check_normalize(f, w, b, [w.clone() for _ in range(65)], [b.clone() for _ in range(65)])
    big = torch.zeros(64)
    with pytest.raises(ValueError, match="overlaps"):  # two cameras over the same bytes
        R.check_normalize(f, w, b, [w, w], [b, b.clone()])
    with pytest.raises(ValueError, match="overlaps"):  # the reference correction inside the colours
        R.check_normalize(big[:24].view(8, 1, 3), big[12:21], b, [w], [b])
    with pytest.raises(AssertionError):  # save_utils.py:16
        scene = types.SimpleNamespace(getTrainCameras=lambda: [types.SimpleNamespace(is_reference_camera=False)])
        R.normalize_before_saving(scene, types.SimpleNamespace(_features_dc=f))


def test_accumulator_refuses_before_any_launch():
    from eogs2_amd import report as R

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.ReportAccumulator("cpu")
    img = torch.zeros(3, 4, 5)
    with pytest.raises(ValueError, match="kind"):
        R.check_accumulate(img, img.clone(), "rgb")
    assert R.kind_index("pan") == 0 and R.kind_index("msi") == 1
    with pytest.raises(ValueError, match="1 <= C <= 4"):
        R.check_accumulate(torch.zeros(5, 4, 4), torch.zeros(5, 4, 4), "msi")
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):
        R.check_accumulate(torch.zeros(4, 4), torch.zeros(4, 4), "msi")
    with pytest.raises(ValueError, match="like image"):
        R.check_accumulate(img, torch.zeros(3, 5, 4), "msi")
    with pytest.raises(ValueError, match="float32"):
        R.check_accumulate(img.half(), img.clone(), "msi")
    with pytest.raises(ValueError, match="contiguous"):
        R.check_accumulate(img.permute(0, 2, 1), img.permute(0, 2, 1), "pan")
    assert R.check_accumulate(img, img.clone(), "pan") == (0, 3, 4, 5)


def test_pack_refuses_before_any_launch():
    from eogs2_amd import report as R

    img = torch.zeros(3, 4, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.pack_products([R.PackItem(img)])
    with pytest.raises(ValueError, match="no items"):
        R.check_pack([])
    with pytest.raises(ValueError, match="at most 16"):
        R.check_pack([R.PackItem(img.clone()) for _ in range(17)])
    with pytest.raises(ValueError, match="mode"):
        R.check_pack([dict(src=img, mode="u16")])
    with pytest.raises(ValueError, match="at most 5"):
        R.check_pack([R.PackItem(torch.zeros(6, 2, 2))])
    with pytest.raises(ValueError, match="replicate"):
        R.check_pack([R.PackItem(img, replicate=True)])
    with pytest.raises(ValueError, match="pitch"):
        R.check_pack([R.PackItem(img, pitch=59)])
    with pytest.raises(ValueError, match="multiples of 4"):
        R.check_pack([R.PackItem(img, offset=2)])
    with pytest.raises(ValueError, match="float32"):
        R.check_pack([R.PackItem(img.double())])
    with pytest.raises(ValueError, match="contiguous"):
        R.check_pack([R.PackItem(img.permute(0, 2, 1))])
    with pytest.raises(ValueError, match="reach byte"):
        R.check_pack([R.PackItem(img, "u8_round")], out=torch.zeros(59, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        R.check_pack([R.PackItem(img, "u8_round")], out=torch.zeros(60))
    # the layout `pack_products` chooses: one after another, each at a multiple of 16 bytes; a side-by-side pair as given
    items, need = R.check_pack([R.PackItem(img, "u8_round"), R.PackItem(img[0], "float"), dict(src=img[:1], mode="u8_trunc", replicate=True)])
    assert [(it.offset, it.pitch) for it in items] == [(0, 15), (64, 20), (144, 15)] and need == 144 + 60
    items, need = R.check_pack([R.PackItem(img, "u8_trunc", offset=0, pitch=30, reverse=True), R.PackItem(img[0], "u8_trunc", offset=15, pitch=30, replicate=True, premap=(1, 3))])
    assert need == 4 * 30 and items[1].premap == (1.0, 3.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.video_frame(img, img[0], 0.0, 1.0)
    with pytest.raises(ValueError, match=r"\(3, H, W\) or \(1, H, W\)"):
        R.video_frame(torch.zeros(2, 4, 5), img[0], 0.0, 1.0)
