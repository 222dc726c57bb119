"""CPU: the public interface of `eogs2_amd.model` (include/eogs_model.h): the class carries every public name of the
reference's `GaussianModel` with its parameters (tests/golden/model/api.npz, read from the reference with inspect.signature by
tests/golden/make_golden_model.py); the header, the binding table and the built library agree; the entries and the wrappers
refuse bad arguments before any device call (CPU tensors: there is no CPU fallback); the PLY header writer and parser."""
import ctypes
import inspect
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import abi_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "model")
TRAIN_ARGS = types.SimpleNamespace(position_lr_init=1.6e-4, feature_lr=2.5e-3, opacity_lr=5e-2, scaling_lr=5e-3, rotation_lr=1e-3,
                                   percent_dense=0.01)


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def header():
    return AC.header_text("eogs_model.h")


# ---- the class against the reference's ----
def test_every_public_name_and_parameter_of_the_reference_is_there():
    from eogs2_amd.model import GaussianModel

    api = json.loads(str(np.load(os.path.join(GOLDEN, "api.npz"))["api"]))
    assert len(api) == 31 and "create_from_pcd" in api and "get_xyz" in api
    for name, want in api.items():
        got = inspect.getattr_static(GaussianModel, name)  # AttributeError: the name is missing
        if want == "property":
            assert isinstance(got, property), name
            continue
        params = list(inspect.signature(got).parameters.values())
        assert len(params) >= len(want), name
        for p, (pname, default) in zip(params, want):  # the reference's parameters first, in its order, with its defaults
            assert p.name == pname, (name, p.name, pname)
            assert (None if p.default is inspect.Parameter.empty else repr(p.default)) == default, (name, pname)
        for p in params[len(want):]:  # what this class adds is optional
            assert p.default is not inspect.Parameter.empty, (name, p.name)


def test_a_fresh_model_has_the_reference_attributes():
    from eogs2_amd.model import GaussianModel

    m = GaussianModel(3)
    assert (m.active_sh_degree, m.max_sh_degree, m.optimizer_type, m.optimizer, m.percent_dense, m.spatial_lr_scale) == (0, 3, "default", None, 0, 0)
    for n in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "max_radii2D", "xyz_gradient_accum", "denom"):
        assert getattr(m, n).numel() == 0, n
    assert m.scaling_activation is torch.exp and m.scaling_inverse_activation is torch.log and m.opacity_activation is torch.sigmoid
    assert m.rotation_activation is torch.nn.functional.normalize
    x = torch.tensor([0.3])
    assert torch.equal(m.inverse_opacity_activation(x), torch.log(x / (1 - x)))
    m.oneupSHdegree(), m.oneupSHdegree(), m.oneupSHdegree(), m.oneupSHdegree()
    assert m.active_sh_degree == 3 and m.update_learning_rate(7) is None
    # the activations and get_covariance are the reference's torch expressions: they run wherever the tensors are
    m._scaling, m._rotation, m._opacity = torch.zeros(2, 3), torch.tensor([[2.0, 0, 0, 0], [0, 0, 3.0, 0]]), torch.zeros(2, 1)
    m._features_dc, m._features_rest = torch.zeros(2, 1, 3), torch.zeros(2, 15, 3)
    assert torch.equal(m.get_scaling, torch.ones(2, 3)) and torch.equal(m.get_opacity, torch.full((2, 1), 0.5))
    assert torch.equal(m.get_rotation, torch.tensor([[1.0, 0, 0, 0], [0, 0, 1.0, 0]])) and m.get_features.shape == (2, 16, 3)
    assert torch.allclose(m.get_covariance(2.0), torch.tensor([[4.0, 0, 0, 4.0, 0, 4.0]] * 2))
    names = m.construct_list_of_attributes()
    from eogs2_amd.model import attribute_names, row_cols

    assert names == attribute_names(15) and len(names) == row_cols(15) == 62
    assert attribute_names(0) == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
                                  "rot_0", "rot_1", "rot_2", "rot_3"]


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import model as M

    assert eogs2_amd.model is M
    for name in ("GaussianModel", "init_tensors", "pack_rows", "unpack_rows", "ply_header", "parse_ply_header"):
        assert callable(getattr(M, name)) and name in M.__all__


# ---- header, binding, library ----
def test_header_and_binding_agree():
    from eogs2_amd import _abi

    names = sorted(set(re.findall(r"\b(eogs_model_[a-z_0-9]+)\s*\(", header())))
    assert names == sorted(_abi.HEADERS["eogs_model.h"]) and len(names) == 3
    assert set(names) <= set(_abi.HIP_ONLY) and not set(names) & AC.elsewhere("eogs_model.h")
    for name, (res, args) in _abi.HEADERS["eogs_model.h"].items():
        assert res is ctypes.c_int, name
        decl = re.search(name + r"\s*\(([^)]*)\)", header()).group(1)
        assert len(decl.split(",")) == len(args), name
        assert args[-1] is ctypes.c_void_p and "void* stream" in decl
    defines = dict(re.findall(r"#define\s+(EOGS_MODEL_[A-Z_]+)\s+(\d+)", header()))
    assert int(defines["EOGS_MODEL_TILE_ROWS"]) == _abi.MODEL_TILE_ROWS == 64
    assert int(defines["EOGS_MODEL_MAX_REST"]) == _abi.MODEL_MAX_REST == 15
    assert _abi.ABI_VERSION == 8


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd._abi import HEADERS

    for n in HEADERS["eogs_model.h"]:
        assert hasattr(hip_lib.cdll, n), n
    assert hip_lib.cdll.eogs_rast_abi_version() == 8  # additions only
    assert hip_lib.model_init is not None and hip_lib.model_rows_unpack is not None  # the short names resolve


def test_entries_check_their_arguments_without_a_device(hip_lib):
    a, b = ctypes.c_void_p(256), ctypes.c_void_p(4096)
    outs = [ctypes.c_void_p(8192 + 256 * k) for k in range(7)]
    err = lambda: hip_lib.cdll.eogs_rast_last_error()  # noqa: E731
    assert hip_lib.model_init(-1, 0, a, a, a, 0.0, *outs, None) == -1 and b"model_init" in err()
    assert hip_lib.model_init(1 << 31, 0, a, a, a, 0.0, *outs, None) == -1
    assert hip_lib.model_init(10, 2, a, b, a, 0.0, *outs, None) == -1 and b"n_rest" in err()
    assert hip_lib.model_init(10, 0, None, b, a, 0.0, *outs, None) == -1 and b"NULL" in err()
    assert hip_lib.model_init(10, 3, a, b, a, 0.0, outs[0], outs[1], None, *outs[3:], None) == -1  # sh 1 needs f_rest
    assert hip_lib.model_init(10, 0, a, b, ctypes.c_void_p(258), 0.0, *outs, None) == -1 and b"aligned" in err()
    assert hip_lib.model_init(10, 0, a, b, outs[4], 0.0, *outs, None) == -1 and b"of its own" in err()
    assert hip_lib.model_init(0, 0, None, None, None, 0.0, *[None] * 7, None) == 0  # no rows: nothing to do
    six = outs[:6]
    for fn, args in ((hip_lib.model_rows_pack, lambda P, n, t=six, r=b: (P, n, *t, r, None)),
                     (hip_lib.model_rows_unpack, lambda P, n, t=six, r=b: (P, n, r, *t, None))):
        assert fn(*args(-1, 0)) == -1 and b"model_rows_" in err()
        assert fn(*args(10, 1)) == -1 and b"n_rest" in err()
        assert fn(*args(10, 24)) == -1
        assert fn(*args(10, 0, r=None)) == -1 and b"NULL" in err()
        assert fn(*args(10, 0, t=[None] + six[1:])) == -1
        assert fn(*args(10, 8, t=six[:2] + [None] + six[3:])) == -1  # sh 2 needs f_rest ...
        assert fn(*args(10, 0, r=ctypes.c_void_p(4098))) == -1 and b"aligned" in err()
        assert fn(*args(10, 0, r=six[3])) == -1 and b"of its own" in err()
        assert fn(*args(0, 15, t=[None] * 6, r=None)) == 0


# ---- no CPU fallback ----
def _cpu_six(P=5, n_rest=3):
    return (torch.zeros(P, 3), torch.zeros(P, 1, 3), torch.zeros(P, n_rest, 3), torch.zeros(P, 1), torch.zeros(P, 3), torch.zeros(P, 4))


def test_cpu_tensors_raise():
    from eogs2_amd.model import GaussianModel, init_tensors, pack_rows, unpack_rows

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        init_tensors(torch.zeros(5, 3), torch.zeros(5, 3), torch.ones(5), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pack_rows(*_cpu_six())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unpack_rows(torch.zeros(5, 26), 3)
    m = GaussianModel(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.create_from_pcd(types.SimpleNamespace(points=torch.zeros(5, 3), colors=torch.zeros(5, 3)), [], 1.0)
    m._xyz, m._features_dc, m._features_rest, m._opacity, m._scaling, m._rotation = (torch.nn.Parameter(t) for t in _cpu_six())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.training_setup(TRAIN_ARGS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.save_ply(os.path.join(os.sep, "nonexistent", "never_written.ply"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.reset_opacity()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.prune_points(torch.zeros(5, dtype=torch.bool))
    assert m.optimizer is None


def test_wrappers_refuse_bad_arguments():
    from eogs2_amd.model import GaussianModel, init_tensors, pack_rows, unpack_rows

    with pytest.raises(RuntimeError, match="float32"):
        init_tensors(torch.zeros(5, 3, dtype=torch.float64), torch.zeros(5, 3), torch.ones(5), 0)
    with pytest.raises(RuntimeError, match="shape"):
        init_tensors(torch.zeros(5, 3), torch.zeros(4, 3), torch.ones(5), 0)
    with pytest.raises(RuntimeError, match="shape"):
        init_tensors(torch.zeros(5, 3), torch.zeros(5, 3), torch.ones(5, 1), 0)
    with pytest.raises(ValueError, match="sh_degree"):
        init_tensors(torch.zeros(5, 3), torch.zeros(5, 3), torch.ones(5), 4)
    with pytest.raises(TypeError):
        init_tensors(np.zeros((5, 3), np.float32), torch.zeros(5, 3), torch.ones(5), 0)
    with pytest.raises(RuntimeError, match="one device"):
        init_tensors(torch.zeros(5, 3), torch.zeros(5, 3, device="meta"), torch.ones(5), 0)
    six = list(_cpu_six())
    with pytest.raises(RuntimeError, match="0, 3, 8 or 15"):
        pack_rows(six[0], six[1], torch.zeros(5, 2, 3), *six[3:])
    with pytest.raises(RuntimeError, match="shape"):
        pack_rows(six[0], torch.zeros(5, 3, 1), *six[2:])
    with pytest.raises(RuntimeError, match="shape"):
        pack_rows(*six[:5], torch.zeros(6, 4))
    with pytest.raises(RuntimeError, match="shape"):
        pack_rows(*six, out=torch.zeros(5, 17))
    with pytest.raises(RuntimeError, match="shape"):
        unpack_rows(torch.zeros(5, 17), 3)
    with pytest.raises(RuntimeError, match="0, 3, 8 or 15"):
        unpack_rows(torch.zeros(5, 23), 2)
    with pytest.raises(ValueError, match="Unknown optimizer, got:lion"):  # the reference's message, gaussian_model.py:270
        m = GaussianModel(0, "lion")
        m.training_setup(TRAIN_ARGS)
    with pytest.raises(TypeError, match="scene_extent"):
        GaussianModel(0).only_densify(1e-4, 0.005, 1.0, None, None)


# ---- the PLY header ----
def test_header_writer_and_parser_round_trip():
    from eogs2_amd.model import attribute_names, parse_ply_header, ply_columns, ply_header

    for sh, n_rest in ((0, 0), (1, 3), (2, 8), (3, 15)):
        names = attribute_names(n_rest)
        h = ply_header(names, 12345)
        assert h.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 12345\nproperty float x\n") and h.endswith(b"property float rot_3\nend_header\n")
        got, count, offset = parse_ply_header(h + b"\x00" * 40)
        assert (got, count, offset) == (names, 12345, len(h))
        assert ply_columns(got, sh) == list(range(len(names)))
    assert parse_ply_header(ply_header(["x"], 0)) == (["x"], 0, len(ply_header(["x"], 0)))


def _hand_written(props, count=2, fmt="binary_little_endian 1.0", extra=()):
    lines = ["ply", f"format {fmt}", "comment made by hand", f"element vertex {count}"] + [f"property {t} {n}" for t, n in props]
    lines += list(extra) + ["end_header"]
    return ("\n".join(lines) + "\n").encode()


def test_parser_maps_shuffled_properties_by_name():
    from eogs2_amd.model import attribute_names, parse_ply_header, ply_columns

    canon = attribute_names(3)
    order = np.random.default_rng(3).permutation(len(canon))
    shuffled = [canon[i] for i in order]
    # an extra property, `float32` spelled out, normals missing, a second element after the vertices
    shuffled = [n for n in shuffled if n not in ("nx", "ny", "nz")]
    shuffled.insert(5, "confidence")
    data = _hand_written([("float32" if k % 2 else "float", n) for k, n in enumerate(shuffled)],
                         extra=["element face 1", "property list uchar int vertex_indices"])
    names, count, offset = parse_ply_header(data)
    assert names == shuffled and count == 2 and offset == len(data)
    cols = ply_columns(names, 1)
    assert len(cols) == len(canon)
    for j, n in enumerate(canon):
        assert cols[j] == (-1 if n in ("nx", "ny", "nz") else shuffled.index(n)), n
    # f_rest_10 sorts after f_rest_9: by the numeric suffix, not as text (gaussian_model.py:394)
    n15 = attribute_names(15)
    assert ply_columns(sorted(n15), 3) == [sorted(n15).index(n) for n in n15]


def test_parser_rejects_what_it_cannot_read():
    from eogs2_amd.model import attribute_names, parse_ply_header, ply_columns

    canon = attribute_names(0)
    props = [("float", n) for n in canon]
    with pytest.raises(ValueError, match="float32 scalar"):
        parse_ply_header(_hand_written([("double", "x")] + props[1:]))
    with pytest.raises(ValueError, match="float32 scalar"):
        parse_ply_header(_hand_written(props[:-1] + [("list uchar float", "rot_3")]))
    with pytest.raises(ValueError, match="float32 scalar"):
        parse_ply_header(_hand_written([("uchar", "red")] + props))
    with pytest.raises(ValueError, match="binary_little_endian"):
        parse_ply_header(_hand_written(props, fmt="ascii 1.0"))
    with pytest.raises(ValueError, match="binary_little_endian"):
        parse_ply_header(_hand_written(props, fmt="binary_big_endian 1.0"))
    with pytest.raises(ValueError, match="not a PLY"):
        parse_ply_header(b"solid stl\n")
    with pytest.raises(ValueError, match="not a PLY"):
        parse_ply_header(_hand_written(props)[:-11])  # no end_header
    with pytest.raises(ValueError, match="twice"):
        parse_ply_header(_hand_written(props + [("float", "x")]))
    # the reference's assertion on the number of f_rest_* columns (gaussian_model.py:395)
    names, _, _ = parse_ply_header(_hand_written([("float", n) for n in attribute_names(3)]))
    with pytest.raises(AssertionError):
        ply_columns(names, 0)
    with pytest.raises(AssertionError):
        ply_columns(names[:10] + names[11:], 1)
    assert ply_columns(names, 1) == list(range(26))
    with pytest.raises(KeyError, match="opacity"):
        ply_columns([n for n in canon if n != "opacity"], 0)
    with pytest.raises(ValueError, match="3 and 4"):
        ply_columns(canon[:-1], 0)


def test_opacity_logit_is_the_references_bits():
    from eogs2_amd.model import opacity_logit

    for x in (0.01, 0.1, 0.5, 0.005):
        want = torch.log((x * torch.ones((3, 1), dtype=torch.float)) / (1 - x * torch.ones((3, 1), dtype=torch.float)))
        v = opacity_logit(x)
        assert torch.tensor([v]).float().item() == v and torch.equal(torch.full((3, 1), v), want)
    for name in ("sh0_1000", "sh1_257", "duplicates_300"):  # and what the reference's create_from_pcd stored
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert np.array_equal(z["opacity"], np.full_like(z["opacity"], opacity_logit(float(z["opacity_init"]))))


def test_entries_refuse_overlapping_ranges(hip_lib):
    """An output that shares an address with an input or with another output, base pointers apart: refused before any launch."""
    err = lambda: hip_lib.cdll.eogs_rast_last_error()  # noqa: E731
    P, v = 100, ctypes.c_void_p
    base = 1 << 20
    ins = [v(base), v(base + 4096), v(base + 8192)]
    outs = [base + 16384 + 4096 * k for k in range(7)]  # xyz f_dc f_rest scaling rotation opacity max_radii2D, 4 KiB apart
    shifted = list(outs)
    shifted[0] = base + 8  # xyz starts inside points
    assert hip_lib.model_init(P, 0, *ins, 0.0, *(v(o) for o in shifted), None) == -1 and b"of its own" in err()
    shifted = list(outs)
    shifted[4] = outs[3] + 400  # rotation starts inside scaling (1200 bytes)
    assert hip_lib.model_init(P, 0, *ins, 0.0, *(v(o) for o in shifted), None) == -1 and b"two outputs overlap" in err()
    # (every call here is refused: a call that passed would launch on these made-up addresses)
    assert hip_lib.model_init(P, 15, *ins, 0.0, *(v(o) for o in outs), None) == -1 and b"two outputs overlap" in err()  # sh 3: f_rest is 18000 bytes
    six = [base + 65536 + 32768 * k for k in range(6)]
    rows = base + (1 << 19)
    assert hip_lib.model_rows_pack(P, 0, *(v(t) for t in six[:5]), v(rows + 6796), v(rows), None) == -1 and b"of its own" in err()  # the last 4 bytes
    assert hip_lib.model_rows_unpack(P, 0, v(rows), *(v(t) for t in six[:5]), v(rows - 1596), None) == -1 and b"of its own" in err()
    assert hip_lib.model_rows_unpack(P, 15, v(rows), v(six[0]), v(six[1]), v(six[2]), v(six[2] + 17996), v(six[4]), v(six[5]), None) == -1
    assert b"two output tensors overlap" in err()
    # what pack only reads may alias
    assert b"overlap" not in (hip_lib.model_rows_pack(0, 0, *[None] * 6, None, None), err())[1]


def test_parser_wants_a_first_element_called_vertex():
    from eogs2_amd.model import attribute_names, parse_ply_header

    props = "".join(f"property float {n}\n" for n in attribute_names(0))
    with pytest.raises(ValueError, match="first element is 'face'"):
        parse_ply_header(("ply\nformat binary_little_endian 1.0\nelement face 2\n" + props + "end_header\n").encode())
    with pytest.raises(ValueError, match="first element is 'points'"):
        parse_ply_header(("ply\nformat binary_little_endian 1.0\nelement points 2\n" + props + "element vertex 2\n" + props + "end_header\n").encode())
