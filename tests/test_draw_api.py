"""CPU: the public interface of the per-iteration draws (eogs2_amd.draw, include/eogs_draw.h): the header, the binding table
and the built library agree; the entries refuse bad arguments before a device is touched; the Python-integer restatement
(`draws_for`) reproduces the Random123 known-answer vectors and agrees with the host program over csrc/draw_rng.h on its
printed sample; every pre-device refusal of the Python layer raises with a message that names the argument."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

import abi_cases as AC
import draw_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def header():
    return AC.header_text("eogs_draw.h")


def test_header_and_binding_agree():
    from eogs2_amd import _abi

    names = sorted(set(re.findall(r"\b(eogs_draw_[a-z_0-9]+)\s*\(", header())))
    assert names == sorted(_abi.HEADERS["eogs_draw.h"]) == ["eogs_draw_advance", "eogs_draw_iteration"]
    assert set(names) <= set(_abi.HIP_ONLY)
    assert not set(names) & AC.elsewhere("eogs_draw.h")  # under this header alone
    for name, (res, args) in _abi.HEADERS["eogs_draw.h"].items():
        assert res is ctypes.c_int, name
        decl = re.search(name + r"\s*\(([^)]*)\)", header()).group(1)
        assert len(decl.split(",")) == len(args), name
        assert args[-1] is ctypes.c_void_p and "void* stream" in decl
    defines = dict(re.findall(r"#define\s+(EOGS_DRAW_[A-Z_]+)\s+(\d+)", header()))
    assert int(defines["EOGS_DRAW_MAX_CAMERAS"]) == _abi.DRAW_MAX_CAMERAS == 8
    assert tuple(int(defines["EOGS_DRAW_" + k]) for k in ("BG", "BG_COPY_FIRST", "CAMERA", "NADIR")) == \
        (_abi.DRAW_BG, _abi.DRAW_BG_COPY_FIRST, _abi.DRAW_CAMERA, _abi.DRAW_NADIR) == (1, 2, 4, 8)
    assert [f[0] for f in _abi.DrawCamera._fields_] == ["affine", "center", "alt_floor", "bg", "virt_affine", "cam2virt", "shear", "extent",
                                                        "cam2virt_scale", "flags"]
    assert ctypes.sizeof(_abi.DrawCamera) == 72
    assert [f[0] for f in _abi.DrawStreamDesc._fields_] == ["seed", "counter"] and ctypes.sizeof(_abi.DrawStreamDesc) == 16
    assert _abi.ABI_VERSION == 8


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS

    for n in HEADERS["eogs_draw.h"]:
        assert hasattr(hip_lib.cdll, n), n
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only
    assert hip_lib.draw_iteration is not None and hip_lib.draw_advance is not None  # the short names resolve


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import draw as D

    assert eogs2_amd.draw is D
    for name in ("DrawStream", "IterationDraws", "draws_for", "check_camera", "check_stream"):
        assert callable(getattr(D, name)) and name in D.__all__


def _camera(**over):
    from eogs2_amd._abi import DrawCamera

    c = DrawCamera(affine=4096, center=4224, alt_floor=4352, bg=8192, virt_affine=8320, cam2virt=8448, shear=8576, extent=0.5,
                   cam2virt_scale=1.0, flags=1 | 4)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_entries_check_their_arguments_without_a_device(hip_lib):
    from eogs2_amd._abi import DrawCamera, DrawStreamDesc

    err = lambda: hip_lib.cdll.eogs_rast_last_error()  # noqa: E731
    ok = DrawStreamDesc(7, 1024)

    def call(n, cams, desc=ok):
        arr = (DrawCamera * max(1, len(cams)))(*cams)
        return hip_lib.draw_iteration(n, ctypes.cast(arr, ctypes.c_void_p), ctypes.byref(desc) if desc is not None else None, None)

    assert call(-1, [_camera()]) == -1 and b"draw_iteration" in err()
    assert call(9, [_camera()] * 9) == -1 and b"8" in err()
    assert hip_lib.draw_iteration(1, None, ctypes.byref(ok), None) == -1 and b"cams" in err()
    assert call(1, [_camera()], None) == -1 and b"stream_desc" in err()
    assert call(1, [_camera()], DrawStreamDesc(7, None)) == -1 and b"counter" in err()
    assert call(1, [_camera()], DrawStreamDesc(7, 1028)) == -1 and b"8-byte" in err()
    assert call(0, [], DrawStreamDesc(7, None)) == -1  # an empty call still names a counter
    assert hip_lib.draw_iteration(0, None, ctypes.byref(ok), None) == 0  # nothing to do, nothing queued
    # a requested output, or an input it needs, is NULL
    assert call(1, [_camera(bg=None)]) == -1 and b"bg" in err()
    assert call(1, [_camera(affine=None)]) == -1 and b"affine" in err()
    assert call(1, [_camera(center=None)]) == -1 and b"center" in err()
    assert call(1, [_camera(virt_affine=None, cam2virt=None, shear=None)]) == -1 and b"virt_affine" in err()
    # misaligned pointers
    for name in ("affine", "center", "alt_floor", "bg", "virt_affine", "cam2virt", "shear"):
        assert call(1, [_camera(**{name: 4098})]) == -1 and b"aligned" in err(), name
    # parameters
    for bad in (-1.0, math.inf, math.nan, -0.5):
        assert call(1, [_camera(extent=bad)]) == -1 and b"extent" in err(), bad
        assert call(1, [_camera(cam2virt_scale=bad)]) == -1 and b"cam2virt_scale" in err(), bad
    # flags
    assert call(1, [_camera(flags=4 | 8)]) == -1 and b"CAMERA and NADIR" in err()
    assert call(1, [_camera(flags=0)]) == -1 and b"flags" in err()
    assert call(1, [_camera(flags=2 | 4)]) == -1 and b"BG_COPY_FIRST" in err()
    assert call(1, [_camera(flags=16)]) == -1 and b"flags" in err()
    assert call(2, [_camera(), _camera(flags=4 | 8)]) == -1  # the second camera is checked too
    # the advance
    assert hip_lib.draw_advance(None, None, None) == -1 and b"counter" in err()
    assert hip_lib.draw_advance(ctypes.c_void_p(1028), None, None) == -1 and b"8-byte" in err()
    assert hip_lib.draw_advance(ctypes.c_void_p(1024), ctypes.c_void_p(1026), None) == -1 and b"gate" in err()


def test_restatement_reproduces_the_known_answers():
    from eogs2_amd.draw import block_for, draws_for, philox4x32_10, uniform_of

    for counter, key, want in DC.KAT:
        assert philox4x32_10(counter, key) == want
        # the same vectors through the stream's layout: key = the seed's words, counter = (iteration low, high, slot, purpose)
        assert block_for(key[0] | key[1] << 32, counter[0] | counter[1] << 32, counter[2], counter[3]) == want
    uniforms, normals = draws_for(0, 0, 0)
    assert uniforms == tuple((w >> 8) * 2.0 ** -24 for w in DC.KAT[0][2][:3])
    assert all(0.0 <= u < 1.0 and DC.f32(u) == u for u in uniforms)
    assert all(abs(z) <= 1.0 and DC.f32(z) == z for z in normals)
    assert uniform_of(0) == 0.0 and uniform_of(0xFFFFFFFF) == 1.0 - 2.0 ** -24
    for bad in ((-1, 0, 0), (1 << 64, 0, 0), (0, -1, 0), (0, 1 << 64, 0), (0, 0, -1), (0, 0, 1 << 32)):
        with pytest.raises(ValueError):
            draws_for(*bad)
    # slots, purposes, iterations and seeds are different blocks
    blocks = {block_for(s, i, c, p) for s in (0, 1, 2 ** 64 - 1) for i in DC.ITERATIONS for c in range(8) for p in (0, 1)}
    assert len(blocks) == 3 * len(DC.ITERATIONS) * 8 * 2


def test_restatement_agrees_with_the_host_program():
    from eogs2_amd.draw import block_for, draws_for

    rows = DC.host_samples()
    assert len(rows) >= 64
    for seed, iteration, slot, bg_words, uniform_bits, shear_words, normal_bits in rows:
        assert list(block_for(seed, iteration, slot, 0)) == bg_words
        assert list(block_for(seed, iteration, slot, 1)[:2]) == shear_words
        uniforms, normals = draws_for(seed, iteration, slot)
        assert [DC.f32_bits(u) for u in uniforms] == uniform_bits  # bit for bit
        for z, zb in zip(normals, normal_bits):  # the same formula over one libm: equal, or one ulp where the build folded a call
            host = torch.tensor([zb], dtype=torch.int64).to(torch.int32).view(torch.float32).item() if zb < 2 ** 31 else \
                torch.tensor([zb - 2 ** 32], dtype=torch.int64).to(torch.int32).view(torch.float32).item()
            assert abs(host - z) <= DC.ulp(z), (seed, iteration, slot)


def test_stream_refuses_before_any_device_call():
    from eogs2_amd.draw import DrawStream, check_stream

    with pytest.raises(TypeError, match="seed"):
        DrawStream(1.5, device="cuda")
    with pytest.raises(TypeError, match="seed"):
        DrawStream(True, device="cuda")
    with pytest.raises(ValueError, match="seed"):
        DrawStream(-1, device="cuda")
    with pytest.raises(ValueError, match="seed"):
        DrawStream(1 << 64, device="cuda")
    with pytest.raises(TypeError, match="counter"):
        DrawStream(0, counter=3)
    with pytest.raises(ValueError, match="counter"):
        DrawStream(0, counter=torch.zeros((), dtype=torch.int32))
    with pytest.raises(ValueError, match="counter"):
        DrawStream(0, counter=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DrawStream(0, counter=torch.zeros((), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DrawStream(0, device="cpu")
    with pytest.raises(ValueError, match="device"):
        DrawStream(0)
    with pytest.raises(RuntimeError, match="counter lives on"):
        check_stream(0, torch.zeros((), dtype=torch.int64), "cuda")
    assert check_stream(2 ** 64 - 1, None, "cuda:0") == (2 ** 64 - 1, torch.device("cuda:0"))


def _shared_stream():
    """A DrawStream on somebody else's counter, as far as the host side goes (no device is touched)."""
    from eogs2_amd.draw import DrawStream

    s = DrawStream.__new__(DrawStream)
    s.seed, s.device, s.shared, s.counter = 5, torch.device("cuda", 0), True, torch.zeros((), dtype=torch.int64)
    return s


def test_shared_stream_refuses_to_move_the_counter():
    s = _shared_stream()
    with pytest.raises(RuntimeError, match="owner advances"):
        s.advance()
    with pytest.raises(RuntimeError, match="seek its owner"):
        s.seek(3)
    assert int(s.counter) == 0


def test_state_dict_round_trips():
    from eogs2_amd.draw import DrawStream

    def owned(seed, counter):
        s = DrawStream.__new__(DrawStream)  # (the host side of a stream: its counter stands in on the CPU)
        s.seed, s.device, s.shared, s.counter = seed, torch.device("cuda", 0), False, torch.tensor(counter, dtype=torch.int64)
        return s

    a = owned(2 ** 64 - 1, 2 ** 63 - 1)
    sd = a.state_dict()
    assert sd == {"seed": 2 ** 64 - 1, "counter": 2 ** 63 - 1, "shared": False}
    b = owned(2 ** 64 - 1, 0)
    b.load_state_dict(sd)
    assert b.position() == 2 ** 63 - 1 and b.state_dict() == sd
    with pytest.raises(ValueError, match="seed"):
        owned(3, 0).load_state_dict(sd)
    with pytest.raises(ValueError, match="owns its counter"):
        _shared_stream().load_state_dict({"seed": 5, "counter": 1, "shared": False})
    with pytest.raises(ValueError, match="iteration index"):
        b.seek(-1)
    with pytest.raises(ValueError, match="iteration index"):
        b.seek(2 ** 63)
    shared = _shared_stream()
    shared.load_state_dict({"seed": 5, "counter": 9, "shared": True})  # the counter comes back with its owner
    assert shared.position() == 0


def _tensors():
    return dict(affine=torch.eye(4), center=torch.zeros(3), alt_floor=torch.zeros(1), bg=torch.zeros(5), virt_affine=torch.zeros(4, 4),
                cam2virt=torch.zeros(3, 3), shear=torch.zeros(2))


def _check(dev="cuda:0", others=(), **over):
    from eogs2_amd.draw import check_camera

    kw = dict(_tensors(), extent=0.02)
    kw.update(over)
    affine, center, alt_floor = kw.pop("affine"), kw.pop("center"), kw.pop("alt_floor")
    return check_camera(torch.device(dev), affine, center, alt_floor, others=others, **kw)


@pytest.mark.parametrize("name", ["affine", "center", "alt_floor", "bg", "virt_affine", "cam2virt", "shear"])
def test_camera_refuses_each_tensor_by_name(name):
    good = _tensors()[name]
    with pytest.raises(TypeError, match=name):
        _check(**{name: good.numpy()})
    with pytest.raises(ValueError, match=rf"{name} must be float32"):
        _check(**{name: good.double()})
    with pytest.raises(ValueError, match=rf"{name} must have shape"):
        _check(**{name: torch.zeros(7)})
    if name != "alt_floor":  # (one element is contiguous whatever its stride)
        bad = torch.zeros(tuple(good.shape)).t() if good.dim() == 2 else torch.zeros(2 * good.numel())[::2]
        with pytest.raises(ValueError, match=rf"{name} must be contiguous"):
            _check(**{name: bad})
    # everything else is in order and where the stream is (meta tensors stand in for the device's): the one CPU tensor is named
    with pytest.raises(RuntimeError, match=rf"{name}: tensors on 'cpu'.*no CPU fallback"):
        _check("meta", **{k: (v if k == name else v.to("meta")) for k, v in _tensors().items()})


def test_camera_refuses_parameters_flags_and_aliasing():
    from eogs2_amd._abi import DRAW_BG, DRAW_BG_COPY_FIRST, DRAW_CAMERA, DRAW_NADIR

    for bad in (-0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="extent"):
            _check(extent=bad)
        with pytest.raises(ValueError, match="cam2virt_scale"):
            _check(cam2virt_scale=bad)
    with pytest.raises(TypeError, match="extent"):
        _check(extent=torch.tensor(0.1))
    with pytest.raises(TypeError, match="cam2virt_scale"):
        _check(cam2virt_scale="1")
    with pytest.raises(ValueError, match="nadir and extent"):
        _check(nadir=True)
    with pytest.raises(ValueError, match="copy_first without bg"):
        _check(bg=None, alt_floor=None, copy_first=True)
    with pytest.raises(ValueError, match="alt_floor without bg"):
        _check(bg=None)
    with pytest.raises(ValueError, match="needs affine"):
        _check(affine=None)
    with pytest.raises(ValueError, match="virt_affine needs center"):
        _check(center=None)
    with pytest.raises(ValueError, match="one of virt_affine, cam2virt, shear"):
        _check(virt_affine=None, cam2virt=None, shear=None)
    with pytest.raises(ValueError, match="need extent or nadir"):
        _check(extent=None)
    with pytest.raises(ValueError, match="asks for nothing"):
        _check(extent=None, bg=None, alt_floor=None, virt_affine=None, cam2virt=None, shear=None)
    # aliasing: an output over an input, over another output, over another camera's tensors
    t = _tensors()
    with pytest.raises(ValueError, match="output virt_affine overlaps affine"):
        _check(virt_affine=t["affine"], affine=t["affine"])
    buf = torch.zeros(8)
    with pytest.raises(ValueError, match="output bg overlaps center"):
        _check(bg=buf[:5], center=buf[4:7])
    with pytest.raises(ValueError, match="overlaps"):
        _check(bg=buf[:5], shear=buf[4:6])
    first = _tensors()
    with pytest.raises(ValueError, match="output bg overlaps bg of another camera"):
        _check(others=[first], bg=first["bg"])
    with pytest.raises(ValueError, match="input affine overlaps output virt_affine of another camera"):
        _check(others=[first], affine=first["virt_affine"])
    with pytest.raises(ValueError, match="output cam2virt overlaps affine of another camera"):
        _check(others=[first], cam2virt=first["affine"].reshape(-1)[:9].view(3, 3))
    # shared inputs are fine; with everything in order the device is what is left to refuse
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _check(others=[first], affine=first["affine"], center=first["center"])
    with pytest.raises(RuntimeError, match="affine: tensors on 'meta'"):
        _check(**{k: v.to("meta") for k, v in _tensors().items()})
    # the flags of the legal combinations (meta tensors stand in for the device's: nothing is launched)
    ok = lambda **kw: _check("meta", **{**{k: v.to("meta") for k, v in _tensors().items()}, **kw})  # noqa: E731
    assert ok() == DRAW_BG | DRAW_CAMERA
    assert ok(copy_first=True) == DRAW_BG | DRAW_BG_COPY_FIRST | DRAW_CAMERA
    assert ok(extent=None, nadir=True) == DRAW_BG | DRAW_NADIR
    assert ok(bg=None, alt_floor=None) == DRAW_CAMERA
    assert ok(extent=None, virt_affine=None, cam2virt=None, shear=None, affine=None, center=None) == DRAW_BG


def test_iteration_draws_counts_its_cameras_before_any_launch():
    from eogs2_amd.draw import IterationDraws

    draws = IterationDraws(types.SimpleNamespace(device=torch.device("cuda", 0)))  # (what it reads of its stream before a launch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        draws.add_camera(torch.eye(4), torch.zeros(3), bg=torch.zeros(5))
    with pytest.raises(ValueError, match="bg must have shape"):
        draws.add_camera(None, None, bg=torch.zeros(4))
    assert len(draws) == 0  # nothing was registered by the refused calls
    draws._cameras = [({}, None)] * 8
    with pytest.raises(ValueError, match="at most 8 cameras"):
        draws.add_camera(None, None, bg=torch.zeros(5))
