"""CPU: the public interface of density control (eogs2_amd.density, include/eogs_density.h): the cross-compiled library
exports every entry point of the header, the ctypes table agrees with it, the size queries and every argument refusal answer
without a device, and the Python wrappers refuse what they cannot run (CPU tensors: there is no CPU fallback)."""
import ctypes
import os
import re

import pytest
import torch

import abi_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stats_update", "bytes", "decide", "split_rows", "build")


@pytest.fixture(scope="module")
def hip_lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


def _header():
    return open(os.path.join(ROOT, "include", "eogs_density.h")).read()


def test_library_exports_the_entry_points(hip_lib):
    from eogs2_amd import _abi

    src = AC.header_text("eogs_density.h")
    declared = sorted(set(re.findall(r"\b(eogs_density_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(_abi.HEADERS["eogs_density.h"]) == sorted("eogs_density_" + n for n in NAMES)
    for n in declared:
        assert hasattr(hip_lib.cdll, n), n
        assert n in _abi.HIP_ONLY and n not in AC.elsewhere("eogs_density.h")
        assert getattr(hip_lib.cdll, n).argtypes == _abi.HEADERS["eogs_density.h"][n][1]  # bound on load
        # one ctypes argument per parameter of the declaration
        params = re.search(rf"\b{n}\s*\(([^)]*)\)", src).group(1)
        assert len([p for p in params.split(",") if p.strip()]) == len(_abi.HEADERS["eogs_density.h"][n][1]), n
    assert hip_lib.cdll.eogs_rast_abi_version() == _abi.ABI_VERSION == 8  # additions only
    assert hip_lib.density_bytes.argtypes == _abi.HEADERS["eogs_density.h"]["eogs_density_bytes"][1]  # the short prefix resolves


def test_constants_agree_with_the_header_and_the_optimizer():
    from eogs2_amd import _abi, density
    from eogs2_amd.optim import RETIRED_LOGIT

    src = _header()
    for name, value in (("CLONE", _abi.DENSITY_CLONE), ("SPLIT", _abi.DENSITY_SPLIT), ("PRUNE_SELF", _abi.DENSITY_PRUNE_SELF),
                        ("PRUNE_SAMP", _abi.DENSITY_PRUNE_SAMP)):
        assert int(re.search(rf"#define EOGS_DENSITY_{name} (\d+)u", src).group(1)) == value
    for name, value in (("COPY", _abi.DENSITY_COPY), ("ZERO", _abi.DENSITY_ZERO), ("XYZ", _abi.DENSITY_XYZ), ("SCALING", _abi.DENSITY_SCALING),
                        ("MAX_N", _abi.DENSITY_MAX_N)):
        assert int(re.search(rf"#define EOGS_DENSITY_{name} (\d+)\b", src).group(1)) == value
    below = float(re.search(r"#define EOGS_DENSITY_RETIRED_BELOW \((-[0-9.e+]+)f\)", src).group(1))
    assert below == 0.5 * RETIRED_LOGIT
    assert (density.FLAG_CLONE, density.FLAG_SPLIT, density.FLAG_PRUNE_SELF, density.FLAG_PRUNE_SAMPLES) == (1, 2, 4, 8)
    assert ctypes.sizeof(_abi.DensityTensor) == 24


def test_package_exports_the_module():
    import eogs2_amd
    from eogs2_amd import density as D

    assert eogs2_amd.density is D
    for n in ("DensityStats", "add_densification_stats", "densify_and_prune", "DensifyInfo"):
        assert callable(getattr(D, n)) and n in D.__all__, n
    s = D.DensityStats(5, "cpu")  # the reference's shapes; the tensors are exposed as they are
    assert (tuple(s.xyz_gradient_accum.shape), tuple(s.denom.shape), tuple(s.max_radii2D.shape)) == ((5, 1), (5, 1), (5,))
    assert all(t.dtype == torch.float32 and not t.any() for t in s.tensors()) and len(s) == 5
    assert s["denom"] is s.denom and tuple(s.keys()) == D.STATS


def test_size_queries_and_argument_checks_need_no_device(hip_lib):
    n = ctypes.c_size_t()
    sizes = {}
    for P in (0, 1, 256, 257, 1 << 20):
        hip_lib.check(hip_lib.density_bytes(P, ctypes.byref(n)))
        sizes[P] = n.value
        assert n.value >= ((P + 255) // 256 + 1) * 16  # four counts per 256-row workgroup and the totals
    assert 0 < sizes[0] <= sizes[1] == sizes[256] <= sizes[257] < sizes[1 << 20] < (1 << 20) // 256 * 16 + 4096
    assert hip_lib.density_bytes(-1, ctypes.byref(n)) == -1 and hip_lib.density_bytes(8, None) == -1
    assert hip_lib.density_bytes((1 << 28) + 1, ctypes.byref(n)) == -1
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is answered before anything touches a device
    need = sizes[257]
    upd = hip_lib.density_stats_update
    assert upd(-1, one, one, 0, one, one, one, None) == -1
    assert b"row count" in hip_lib.cdll.eogs_rast_last_error()
    for k in (1, 2, 4, 5, 6):
        a = [8, one, one, 0, one, one, one, None]
        a[k] = None
        assert upd(*a) == -1
    assert b"NULL" in hip_lib.cdll.eogs_rast_last_error()
    counts = (ctypes.c_int64 * 4)()
    dec = hip_lib.density_decide
    good = [257, one, one, one, one, 1e-4, 0.05, 0.005, 1, 0.5, 1.6, one, one, need, counts, None]
    for k in (1, 2, 3, 4, 11, 12, 14):
        a = list(good)
        a[k] = None
        assert dec(*a) == -1, k
    assert b"NULL" in hip_lib.cdll.eogs_rast_last_error()
    a = list(good); a[0] = -2
    assert dec(*a) == -1
    a = list(good); a[10] = 0.0
    assert dec(*a) == -1 and b"split_div" in hip_lib.cdll.eogs_rast_last_error()
    a = list(good); a[13] = need - 300
    assert dec(*a) == -3 and b"workspace" in hip_lib.cdll.eogs_rast_last_error()
    rows = hip_lib.density_split_rows
    assert rows(257, None, one, one, 12, one, need, None) == -1
    assert rows(257, one, None, one, 12, one, need, None) == -1
    assert rows(257, one, one, one, 10, one, need, None) == -1
    assert rows(257, one, one, one, 260, one, need, None) == -1
    assert rows(257, one, one, one, 12, one, 16, None) == -3
    from eogs2_amd._abi import DensityTensor

    def tensors(*spec):
        arr = (DensityTensor * len(spec))()
        for t, (src, dst, rb, kind) in zip(arr, spec):
            t.src, t.dst, t.row_bytes, t.kind = src, dst, rb, kind
        return ctypes.cast(arr, ctypes.c_void_p)

    bld = hip_lib.density_build
    counts[:] = [100, 20, 50, 40]
    ok = tensors((256, 256, 12, 2), (256, 256, 4, 0))
    assert bld(257, 0, one, counts, 2, ok, one, one, 1.6, one, need, None) == -1 and b"N out" in hip_lib.cdll.eogs_rast_last_error()
    assert bld(257, 9, one, counts, 2, ok, one, one, 1.6, one, need, None) == -1
    assert bld(257, 2, one, None, 2, ok, one, one, 1.6, one, need, None) == -1
    assert bld(257, 2, one, counts, 2, None, one, one, 1.6, one, need, None) == -1
    assert bld(257, 2, one, counts, 2, ok, None, one, 1.6, one, need, None) == -1
    assert bld(257, 2, one, counts, 2, ok, one, None, 1.6, one, need, None) == -1
    assert b"rotation and samples" in hip_lib.cdll.eogs_rast_last_error()
    assert bld(257, 2, one, counts, 2, ok, one, one, 1.6, one, 16, None) == -3
    for bad in ((256, 256, 16, 2), (256, 256, 8, 3), (256, 256, 6, 0), (256, 256, 260, 0), (256, 256, 4, 7), (None, 256, 4, 0), (256, None, 4, 0)):
        assert bld(257, 2, one, counts, 1, tensors(bad), one, one, 1.6, one, need, None) == -1, bad
    for bad in ([100, 20, 50, 60], [300, 0, 0, 0], [-1, 0, 0, 0], [200, 0, 100, 0]):
        counts[:] = bad
        assert bld(257, 2, one, counts, 2, ok, one, one, 1.6, one, need, None) == -1, bad
    assert b"counts" in hip_lib.cdll.eogs_rast_last_error()


class _Opt:
    def __init__(self, P):
        shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 0, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
        self.param_groups = [{"name": n, "params": [torch.nn.Parameter(torch.zeros(s))]} for n, s in shapes.items()]
        self.state = {}


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import density as D

    P = 6
    s = D.DensityStats(P, "cpu")
    g, r = torch.zeros(P, 3), torch.ones(P, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.update(g, r)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.add_densification_stats(s.xyz_gradient_accum, s.denom, s.max_radii2D, g, r.float())
    with pytest.raises(ValueError, match="None"):
        s.update(None, r)
    for bad_g, bad_r in ((g.double(), r), (g.half(), r), (g, r.long()), (g, r.double()), (g, r.bool())):
        with pytest.raises(TypeError):
            s.update(bad_g, bad_r)
    for bad_g, bad_r in ((torch.zeros(P + 1, 3), r), (torch.zeros(P, 2), r), (g, torch.ones(P - 1, dtype=torch.int32)), (g.view(-1), r),
                         (g, r.view(P, 1))):
        with pytest.raises(ValueError):
            s.update(bad_g, bad_r)
    with pytest.raises(TypeError):
        D.add_densification_stats(s.xyz_gradient_accum.double(), s.denom, s.max_radii2D, g, r)
    with pytest.raises(ValueError):
        D.add_densification_stats(s.xyz_gradient_accum.view(-1), s.denom, s.max_radii2D, g, r)
    with pytest.raises(ValueError):
        D.add_densification_stats(s.xyz_gradient_accum, s.denom[:-1], s.max_radii2D, g, r)
    opt = _Opt(P)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.densify_and_prune(opt, s, grad_threshold=1e-4, scene_extent=5.0)
    with pytest.raises(ValueError, match="scene_extent"):
        D.densify_and_prune(opt, s, grad_threshold=1e-4)
    with pytest.raises(ValueError, match="screen_size_threshold"):
        D.densify_and_prune(opt, s, grad_threshold=1e-4, scene_extent=5.0, max_screen_size=20)
    for N in (0, 9):
        with pytest.raises(ValueError):
            D.densify_and_prune(opt, s, grad_threshold=1e-4, scene_extent=5.0, N=N)
    with pytest.raises(ValueError):
        D.densify_and_prune(opt, D.DensityStats(P + 1, "cpu"), grad_threshold=1e-4, scene_extent=5.0)
    with pytest.raises(TypeError):
        D.densify_and_prune(opt, {"xyz_gradient_accum": s.xyz_gradient_accum.double(), "denom": s.denom, "max_radii2D": s.max_radii2D},
                            grad_threshold=1e-4, scene_extent=5.0)
