"""CPU: the public interface of the resets (eogs2_amd.reset, include/eogs_reset.h): the header, the binding table and the
built library agree; the entries and the Python wrappers refuse bad arguments before any device call (CPU tensors: there is
no CPU fallback); and the cases' two references (tests/reset_cases.py: fp32 and float64) agree with each other inside the
stated margin, with the borderline share of every committed seed under its cap."""
import ctypes
import os
import re

import pytest
import torch

import abi_cases as AC
import reset_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def header():
    return AC.header_text("eogs_reset.h")


def test_header_and_binding_agree():
    from eogs2_amd import _abi

    names = sorted(set(re.findall(r"\b(eogs_reset_[a-z_0-9]+)\s*\(", header())))
    assert names == sorted(_abi.HEADERS["eogs_reset.h"]) and len(names) == 4
    assert set(names) <= set(_abi.HIP_ONLY)
    assert not set(names) & AC.elsewhere("eogs_reset.h")  # under this header alone
    for name, (res, args) in _abi.HEADERS["eogs_reset.h"].items():
        assert res is ctypes.c_int, name  # every entry returns a status
        decl = re.search(name + r"\s*\(([^)]*)\)", header()).group(1)
        assert len(decl.split(",")) == len(args), name
        assert args[-1] is ctypes.c_void_p and "void* stream" in decl  # the stream is passed in
    defines = dict(re.findall(r"#define\s+(EOGS_RESET_[A-Z_]+)\s+(\d+)", header()))
    assert int(defines["EOGS_RESET_MAX_VIEWS"]) == _abi.RESET_MAX_VIEWS == 16
    assert int(defines["EOGS_RESET_MAX_TENSORS"]) == _abi.RESET_MAX_TENSORS == 16
    assert int(defines["EOGS_RESET_MAX_ROW_ELEMS"]) == _abi.RESET_MAX_ROW_ELEMS
    assert (int(defines["EOGS_RESET_TILE_H"]), int(defines["EOGS_RESET_TILE_W"])) == (_abi.RESET_TILE_H, _abi.RESET_TILE_W)
    # the descriptors have the header's layout
    assert [f[0] for f in _abi.ResetView._fields_] == ["eroded", "affine", "H", "W"] and ctypes.sizeof(_abi.ResetView) == 24
    assert [f[0] for f in _abi.ResetTensor._fields_] == ["data", "row_elems", "value"] and ctypes.sizeof(_abi.ResetTensor) == 16
    assert _abi.ABI_VERSION == 8


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS

    for n in HEADERS["eogs_reset.h"]:
        assert hasattr(hip_lib.cdll, n), n
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only
    assert hip_lib.reset_erode is not None and hip_lib.reset_opacity_cap is not None  # the short names resolve


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import reset as R

    assert eogs2_amd.reset is R
    for name in ("shadow_reset_flags", "color_reset_", "color_reset", "render_all_views", "reset_opacity_"):
        assert callable(getattr(R, name)) and name in R.__all__


def test_entries_check_their_arguments_without_a_device(hip_lib):
    from eogs2_amd._abi import ResetTensor, ResetView

    one = ctypes.c_void_p(256)
    two = ctypes.c_void_p(512)
    err = lambda: hip_lib.cdll.eogs_rast_last_error()  # noqa: E731
    assert hip_lib.reset_erode(0, 5, one, two, None) == -1 and b"reset_erode" in err()
    assert hip_lib.reset_erode(5, -1, one, two, None) == -1
    assert hip_lib.reset_erode(65536, 32768, one, two, None) == -1 and b"2^31" in err()
    assert hip_lib.reset_erode(5, 5, None, two, None) == -1
    assert hip_lib.reset_erode(5, 5, one, None, None) == -1
    assert hip_lib.reset_erode(5, 5, one, one, None) == -1 and b"of its own" in err()
    views = (ResetView * 17)()
    for v in views:
        v.eroded, v.affine, v.H, v.W = 256, 512, 4, 4
    arr = ctypes.cast(views, ctypes.c_void_p)
    assert hip_lib.reset_flags(-1, one, None, -5e29, 1, arr, 0, one, None) == -1
    assert hip_lib.reset_flags(10, one, None, -5e29, 17, arr, 0, one, None) == -1 and b"16 views" in err()
    assert hip_lib.reset_flags(10, one, None, -5e29, 1, None, 0, one, None) == -1
    assert hip_lib.reset_flags(10, None, None, -5e29, 1, arr, 0, one, None) == -1
    assert hip_lib.reset_flags(10, one, None, -5e29, 1, arr, 0, None, None) == -1
    assert hip_lib.reset_flags(10, one, None, float("nan"), 1, arr, 0, one, None) == -1
    views[0].W = 0
    assert hip_lib.reset_flags(10, one, None, -5e29, 1, arr, 0, one, None) == -1
    views[0].W, views[0].eroded = 4, None
    assert hip_lib.reset_flags(10, one, None, -5e29, 1, arr, 0, one, None) == -1 and b"map" in err()
    assert hip_lib.reset_flags(0, None, None, -5e29, 0, None, 0, None, None) == 0  # no rows, no views: nothing to do
    tensors = (ResetTensor * 17)()
    for t in tensors:
        t.data, t.row_elems, t.value = 256, 3, 0.0
    tarr = ctypes.cast(tensors, ctypes.c_void_p)
    assert hip_lib.reset_rows(10, one, 17, tarr, None) == -1 and b"16 tensors" in err()
    assert hip_lib.reset_rows(10, None, 2, tarr, None) == -1
    assert hip_lib.reset_rows(-1, one, 2, tarr, None) == -1
    tensors[1].row_elems = 65
    assert hip_lib.reset_rows(10, one, 2, tarr, None) == -1 and b"64" in err()
    tensors[1].row_elems, tensors[1].data = 3, None
    assert hip_lib.reset_rows(10, one, 2, tarr, None) == -1
    assert hip_lib.reset_rows(0, None, 0, None, None) == 0
    assert hip_lib.reset_opacity_cap(-1, one, None, None, -4.6, -5e29, None) == -1
    assert hip_lib.reset_opacity_cap(10, None, None, None, -4.6, -5e29, None) == -1
    assert hip_lib.reset_opacity_cap(10, one, None, None, float("nan"), -5e29, None) == -1
    assert hip_lib.reset_opacity_cap(10, ctypes.c_void_p(258), None, None, -4.6, -5e29, None) == -1 and b"aligned" in err()
    assert hip_lib.reset_opacity_cap(0, None, None, None, -4.6, -5e29, None) == 0


def test_shadow_reset_flags_refuses_bad_arguments():
    from eogs2_amd.reset import shadow_reset_flags

    xyz, s, A = torch.zeros(10, 3), torch.ones(6, 7), torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shadow_reset_flags(xyz, [(s, A)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shadow_reset_flags(xyz, [], opacity=torch.zeros(10, 1), out=torch.zeros(10, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="float32"):
        shadow_reset_flags(xyz.double(), [(s, A)])
    with pytest.raises(RuntimeError, match="shape"):
        shadow_reset_flags(torch.zeros(10, 4), [(s, A)])
    with pytest.raises(RuntimeError, match="contiguous"):
        shadow_reset_flags(torch.zeros(3, 10).t(), [(s, A)])
    with pytest.raises(TypeError):
        shadow_reset_flags(xyz.numpy(), [(s, A)])
    with pytest.raises(ValueError, match="a map for every view"):
        shadow_reset_flags(xyz, [(s, A), (None, A)])
    with pytest.raises(ValueError, match="a map for every view"):
        shadow_reset_flags(xyz, [s])
    with pytest.raises(RuntimeError, match="float32"):
        shadow_reset_flags(xyz, [(s.half(), A)])
    with pytest.raises(RuntimeError, match="shape"):
        shadow_reset_flags(xyz, [(s[None], A)])
    with pytest.raises(RuntimeError, match="contiguous"):
        shadow_reset_flags(xyz, [(torch.ones(7, 6).t(), A)])
    with pytest.raises(RuntimeError, match="shape"):
        shadow_reset_flags(xyz, [(s, torch.eye(3))])
    with pytest.raises(RuntimeError, match="contiguous"):
        shadow_reset_flags(xyz, [(s, torch.eye(4).t())])
    with pytest.raises(RuntimeError, match="H, W"):
        shadow_reset_flags(xyz, [(torch.ones(0, 5), A)])
    with pytest.raises(RuntimeError, match="one device"):
        shadow_reset_flags(xyz, [(s.to("meta"), A)])
    with pytest.raises(RuntimeError, match="one device"):
        shadow_reset_flags(xyz, [(s, A.to("meta"))])
    with pytest.raises(RuntimeError, match="11 elements"):
        shadow_reset_flags(xyz, [(s, A)], opacity=torch.zeros(11))
    with pytest.raises(RuntimeError, match="one device"):
        shadow_reset_flags(xyz, [(s, A)], opacity=torch.zeros(10, device="meta"))
    with pytest.raises(RuntimeError, match="10 bytes"):
        shadow_reset_flags(xyz, [(s, A)], out=torch.zeros(9, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="10 bytes"):
        shadow_reset_flags(xyz, [(s, A)], out=torch.zeros(10, dtype=torch.int32))


def test_color_reset_and_reset_opacity_refuse_bad_arguments():
    from eogs2_amd.reset import color_reset_, reset_opacity_

    opt = RC.make_optimizer(10, "cpu")
    flags = torch.zeros(10, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        color_reset_(opt, flags)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        color_reset_(RC.make_optimizer(10, "cpu", with_state=False), flags.bool())
    with pytest.raises(RuntimeError, match="flags of 9 bytes"):
        color_reset_(opt, flags[:9])
    with pytest.raises(RuntimeError, match="uint8"):
        color_reset_(opt, flags.float())
    with pytest.raises(RuntimeError, match="one device"):
        color_reset_(opt, flags.to("meta"))
    with pytest.raises(KeyError, match="scaling"):
        color_reset_(torch.optim.Adam([dict(params=[torch.nn.Parameter(torch.zeros(10, 1))], name="opacity"),
                                       dict(params=[torch.nn.Parameter(torch.zeros(10, 1, 3))], name="f_dc")], lr=0.0), flags)
    bad = RC.make_optimizer(10, "cpu")
    bad.param_groups[4]["params"][0].data = torch.zeros(10, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="float32"):
        color_reset_(bad, flags)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reset_opacity_(opt)
    with pytest.raises(KeyError, match="alpha"):
        reset_opacity_(opt, name="alpha")
    before = RC.snapshot(opt)
    RC.assert_snapshots_equal(RC.snapshot(opt), before)  # (nothing was touched by the refused calls)


def test_fill_values_are_the_references_bits():
    from eogs2_amd.reset import cap_logit, fill_values

    one = torch.ones(3, 1)
    v = fill_values()
    assert torch.tensor([v["opacity"]]).float().item() == v["opacity"]  # the floats hold fp32 values
    assert RC.same_bits(torch.full((3, 1), v["opacity"]), torch.log(0.005 * one / (1 - 0.005 * one)))
    assert RC.same_bits(torch.full((3, 1), v["f_dc"]), (torch.full_like(one, 1.1) - 0.5) / RC.C0)
    assert RC.same_bits(torch.full((3, 1), v["scaling"]), torch.log((1.0 / 400) * one))
    assert RC.same_bits(torch.full((1,), cap_logit(0.01)), RC.reset_opacity_constant())
    # the restatement of the fills: flagged rows get those values and lose their moments, nothing else moves
    opt = RC.make_optimizer(7, "cpu")
    snap = RC.snapshot(opt)
    flags = torch.tensor([1, 0, 0, 1, 0, 1, 0], dtype=torch.uint8)
    want = RC.color_reset_ref(snap, flags)
    on = flags.bool()
    assert RC.same_bits(want["f_dc"][0][on], torch.full((3, 1, 3), v["f_dc"])) and RC.same_bits(want["f_dc"][0][~on], snap["f_dc"][0][~on])
    assert not want["scaling"][1][on].any() and RC.same_bits(want["scaling"][2][~on], snap["scaling"][2][~on])
    assert RC.same_bits(want["xyz"][1], snap["xyz"][1]) and RC.same_bits(want["rotation"][0], snap["rotation"][0])


def test_erode_reference_on_its_cases():
    """What the GPU test holds the kernel to: NaN spreads over its window, both subtractions are kept, -inf padding."""
    for H, W in RC.ERODE_SHAPES:
        s = RC.erode_input(H, W)
        e = RC.erode_ref(s)
        assert e.shape == s.shape
        if H * W >= 9:
            i, j = H // 2, (2 * W) // 3
            win = e[max(i - 2, 0):i + 3, max(j - 2, 0):j + 3]
            assert torch.isnan(win).all() and int(torch.isnan(e).sum()) == win.numel()
        ok = ~torch.isnan(e)
        assert bool((e[ok] <= (1 - (1 - s))[ok]).all())  # an erosion: never above the (twice rounded) pixel itself
    s = torch.tensor([[0.1]])
    assert RC.erode_ref(s).item() == 1 - (1 - s).item() and RC.erode_ref(s).item() != s.item()


@pytest.mark.parametrize("n_views", sorted(RC.FLAG_VIEWS))
@pytest.mark.parametrize("P", RC.FLAG_P)
def test_flag_references_agree_inside_the_margin(P, n_views):
    xyz, opacity, views = RC.flags_case(P, n_views)
    f32, _ = RC.flags_ref(xyz, views, opacity, torch.float32)
    f64, borderline = RC.flags_ref(xyz, views, opacity, torch.float64)
    assert int(borderline.sum()) <= RC.BORDERLINE_SHARE * P  # none below 1000 rows
    assert not bool(((f32 != f64) & ~borderline).any())
    RC.check_flags(f32.to(torch.uint8), xyz, views, opacity)  # the checker accepts the reference
    assert not f32[0] and RC.flags_ref(xyz, views, None, torch.float32)[0][0]  # row 0: flagged by every view, but retired
    if P > 1:
        assert not f32[1]  # the NaN row
        assert 0 < int(f32.sum()) < P
    if P > 40:
        wrong = f32.clone()
        wrong[40] = ~wrong[40]
        with pytest.raises(AssertionError):
            RC.check_flags(wrong.to(torch.uint8), xyz, views, opacity)


def test_reset_opacity_reference():
    l = RC.opacity_logits(257)
    want = RC.reset_opacity_ref64(l)
    cap = RC.reset_opacity_constant().item()
    above = (l >= cap).squeeze()
    assert int(above.sum()) > 50 and torch.isnan(want[11]) and want[13].item() == float("-inf")
    assert float(RC.ulp_distance(torch.full_like(l, cap)[above], want[above]).max()) <= 1.0
    keep = ~above & ~torch.isnan(l.squeeze()) & (l.squeeze() > -1e29)
    assert float(RC.ulp_distance(l[keep], want[keep]).max()) <= 1.0  # below the cap the formula is the identity up to rounding
