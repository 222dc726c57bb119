"""GPU (MI355X): `eogs2_amd.model` (include/eogs_model.h) in four groups.

1. Init. `GaussianModel.create_from_pcd` against tests/golden/model/*.npz, what the reference's own create_from_pcd made of the
   same points, colours and `dist2` on the CPU. xyz, rotation, f_rest, max_radii2D and opacity are bit-equal. f_dc and scaling are
   held to the float64 formula within 2 x the error the reference's own fp32 result (in the fixture) shows against float64 on
   that input, plus one fp32 ulp of the value: the margin covers a device `log` that rounds differently from the host's.
   Without an injected `dist2` the statistic comes from `knn.distCUDA2`, first held to the fixture's within the bound of
   tests/test_gpu_knn.py (rtol 2e-5, atol 1e-12); scaling is then held to the float64 formula of THAT statistic.
2. Pack / unpack against the torch expression of save_ply (gaussian_model.py:313-342), bit for bit, both directions.
3. File: save_ply read back with numpy through the parsed header, load_ply into a fresh model, a file with permuted columns.
4. Lifecycle: tests/golden/optim/*.npz (the reference's GaussianModel through train_pan.py's optimizer / density-control
   lifecycle) replayed through this class's own methods with the acceptance of tests/test_gpu_optim.py and test_gpu_density.py
   (optim_cases.check_steps / check_structural / _computed_close); capture -> restore -> one more step against the
   uninterrupted run, bit for bit, eager and capturable.
"""
import io
import os
import types

import numpy as np
import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "model")
INIT_FIXTURES = ("sh0_1000", "sh1_257", "duplicates_300")
EXACT = ("xyz", "rotation", "f_rest", "max_radii2D", "opacity")
C0 = 0.28209479177387814
ARGS = types.SimpleNamespace(**oc.TRAIN_ARGS)
PARAMS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
          "rotation": "_rotation"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype and _bits(a) == _bits(b)


def _ulp32(x64):
    return np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)


def _cams(n=3):
    return [types.SimpleNamespace(image_name=f"view_{k}") for k in range(n)]


def _model_tensors(m):
    return {"xyz": m._xyz, "f_dc": m._features_dc, "f_rest": m._features_rest, "scaling": m._scaling, "rotation": m._rotation,
            "opacity": m._opacity, "max_radii2D": m.max_radii2D}


# ---- 1. init ----
def _f64_formulas(colors, dist2):
    f_dc = ((colors.astype(np.float64) - 0.5) / C0).reshape(-1, 1, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        clamped = np.where(dist2 < np.float32(0.0000001), np.float64(np.float32(0.0000001)), dist2.astype(np.float64))  # a NaN stays
        scaling = np.repeat(np.log(np.sqrt(clamped))[:, None], 3, axis=1)
    return f_dc, scaling


def _held_to_f64(name, key, got, want64, ref_err):
    """|got - float64| <= 2 x the reference's own error + 1 ulp of the value, elementwise; prints both maxima."""
    err = np.abs(got.astype(np.float64) - want64)
    bound = 2.0 * ref_err + _ulp32(want64)
    worst = float(err.max()) if err.size else 0.0
    print(f"{name} {key}: kernel |fp32 - float64| max {worst:.3e}; reference's own {ref_err:.3e}; worst error / bound "
          f"{float((err / bound).max()) if err.size else 0.0:.3f}")
    assert (err <= bound).all(), (name, key, worst, ref_err)


@pytest.fixture(scope="module")
def init_fixtures():
    return {n: dict(np.load(os.path.join(GOLDEN, n + ".npz"))) for n in INIT_FIXTURES}


def _check_against_fixture(name, z, m, dist2):
    t = _model_tensors(m)
    for k in EXACT:
        got = t[k].detach().cpu().numpy()
        assert got.dtype == np.float32 and got.shape == z[k].shape and got.tobytes() == z[k].tobytes(), (name, k)
    f_dc64, scaling64 = _f64_formulas(z["colors"], dist2)
    ref_dc = float(np.abs(z["f_dc"].astype(np.float64) - z["f_dc@64"]).max())
    ref_sc = float(np.abs(z["scaling"].astype(np.float64) - z["scaling@64"]).max())
    assert t["f_dc"].shape == z["f_dc"].shape and t["scaling"].shape == z["scaling"].shape
    _held_to_f64(name, "f_dc", t["f_dc"].detach().cpu().numpy(), f_dc64, ref_dc)
    _held_to_f64(name, "scaling", t["scaling"].detach().cpu().numpy(), scaling64, ref_sc)
    for k in oc.GROUPS:
        p = getattr(m, PARAMS[k])
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.is_contiguous(), (name, k)
    assert not m.max_radii2D.requires_grad
    assert _same_bits(m._exposure, torch.from_numpy(z["exposure"])) and isinstance(m._exposure, torch.nn.Parameter)
    assert m.exposure_mapping == {f"view_{k}": k for k in range(3)} and m.pretrained_exposures is None and m.spatial_lr_scale == 2.5
    assert m.active_sh_degree == 0 and m.get_exposure_from_name("view_1").shape == (3, 4)


@pytest.mark.parametrize("name", INIT_FIXTURES)
@pytest.mark.parametrize("as_tensors", [False, True])
def test_create_from_pcd_matches_the_reference_fixture(dev, init_fixtures, name, as_tensors):
    from eogs2_amd.model import GaussianModel

    z = init_fixtures[name]
    assert np.array_equal(z["f_dc@64"], _f64_formulas(z["colors"], z["dist2"])[0]) and np.array_equal(z["scaling@64"], _f64_formulas(z["colors"], z["dist2"])[1])
    pts, cols = (torch.from_numpy(z[k]).to(dev) for k in ("points", "colors")) if as_tensors else (z["points"], z["colors"])
    m = GaussianModel(int(z["sh"]))
    m.create_from_pcd(types.SimpleNamespace(points=pts, colors=cols), _cams(), 2.5, float(z["opacity_init"]),
                      dist2=torch.from_numpy(z["dist2"]).to(dev))
    _check_against_fixture(name, z, m, z["dist2"])


@pytest.mark.parametrize("name", INIT_FIXTURES)
def test_create_from_pcd_with_its_own_knn(dev, init_fixtures, name):
    from eogs2_amd.knn import distCUDA2
    from eogs2_amd.model import GaussianModel

    z = init_fixtures[name]
    dist2 = distCUDA2(torch.from_numpy(z["points"]).to(dev)).cpu().numpy()
    assert np.allclose(dist2, z["dist2"], rtol=2e-5, atol=1e-12), float(np.abs(dist2 - z["dist2"]).max())
    m = GaussianModel(int(z["sh"]))
    m.create_from_pcd(types.SimpleNamespace(points=z["points"], colors=z["colors"]), _cams(), 2.5, float(z["opacity_init"]))
    _check_against_fixture(name, z, m, dist2)


def _reference_lines(points, colors, dist2, sh, opacity_init):
    """gaussian_model.py:167-215 in torch on the CPU, fp32."""
    P = points.shape[0]
    features = torch.zeros((P, 3, (sh + 1) ** 2)).float()
    features[:, :3, 0] = (colors - 0.5) / C0
    scales = torch.log(torch.sqrt(torch.clamp_min(dist2, 0.0000001)))[..., None].repeat(1, 3)
    rots = torch.zeros((P, 4))
    rots[:, 0] = 1
    o = opacity_init * torch.ones((P, 1), dtype=torch.float)
    return {"xyz": points.clone(), "f_dc": features[:, :, 0:1].transpose(1, 2).contiguous(), "f_rest": features[:, :, 1:].transpose(1, 2).contiguous(),
            "scaling": scales, "rotation": rots, "opacity": torch.log(o / (1 - o)), "max_radii2D": torch.zeros(P)}


@pytest.mark.parametrize("sh", [0, 3])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257])
def test_init_tensors_at_the_workgroup_edges(dev, P, sh):
    """One row, one row short of a workgroup, exactly one, one more; dist2 NaN / +inf / 0 / negative planted where rows exist."""
    from eogs2_amd.model import init_tensors

    g = torch.Generator().manual_seed(100 * P + sh)
    points, colors = torch.randn(P, 3, generator=g) * 50, torch.rand(P, 3, generator=g)
    dist2 = torch.exp(torch.empty(P).uniform_(-20, 5, generator=g))
    special = {3: float("nan"), 4: float("inf"), 5: 0.0, 6: -1.0, P - 1: 3e-8}
    if P >= 255:
        for i, v in special.items():
            dist2[i] = v
    want = _reference_lines(points, colors, dist2, sh, 0.1)
    got = init_tensors(points.to(dev), colors.to(dev), dist2.to(dev), sh, 0.1)
    assert set(got) == set(want)
    for k in EXACT:
        assert _same_bits(got[k], want[k]), (P, sh, k)
    f_dc64, scaling64 = _f64_formulas(colors.numpy(), dist2.numpy())
    sc_got, sc_ref = got["scaling"].cpu().numpy(), want["scaling"].numpy()
    finite = np.isfinite(scaling64)
    assert np.array_equal(np.isnan(sc_got), np.isnan(scaling64)) and np.array_equal(sc_got[~finite & ~np.isnan(scaling64)], sc_ref[~finite & ~np.isnan(scaling64)])
    if P >= 255:
        assert np.isnan(sc_got[3]).all() and np.isposinf(sc_got[4]).all() and _bits(got["scaling"][5]) == _bits(got["scaling"][6]) == _bits(got["scaling"][P - 1])
    for key, g_, w64, ref in (("f_dc", got["f_dc"].cpu().numpy(), f_dc64, want["f_dc"].numpy()), ("scaling", sc_got[finite], scaling64[finite], sc_ref[finite])):
        ref_err = float(np.abs(ref.astype(np.float64) - w64).max()) if w64.size else 0.0
        _held_to_f64(f"P {P} sh {sh}", key, g_, w64, ref_err)


# ---- 2. pack / unpack ----
def _random_six(P, n_rest, seed):
    g = torch.Generator().manual_seed(seed)
    six = [torch.randn(s, generator=g) * 10.0 ** float(torch.randint(-3, 4, (1,), generator=g)) for s in
           ((P, 3), (P, 1, 3), (P, n_rest, 3), (P, 1), (P, 3), (P, 4))]
    if P:  # values that only survive a move of bits
        six[0][0, 1], six[1][P - 1, 0, 2], six[3][P // 2, 0], six[5][0, 3] = float("nan"), -0.0, float("-inf"), -0.0
        six[4][P - 1] = torch.tensor([0x7FC12345, 0xFFC00001 - (1 << 32), 1], dtype=torch.int32).view(torch.float32)  # NaN payloads, a subnormal
        if n_rest:
            six[2][P - 1, n_rest - 1, 2], six[2][0, 0, 0] = float("nan"), -0.0
    return six


def _save_ply_expression(xyz, f_dc, f_rest, opacity, scaling, rotation):
    """gaussian_model.py:313-342: the `attributes` array."""
    return torch.cat((xyz, torch.zeros_like(xyz), f_dc.transpose(1, 2).flatten(start_dim=1).contiguous(),
                      f_rest.transpose(1, 2).flatten(start_dim=1).contiguous(), opacity, scaling, rotation), dim=1)


@pytest.mark.parametrize("sh", [0, 1, 2, 3])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 1000])
def test_pack_and_unpack_move_bits(dev, P, sh):
    from eogs2_amd.model import pack_rows, row_cols, unpack_rows

    n_rest = (sh + 1) ** 2 - 1
    six = _random_six(P, n_rest, 1000 * sh + P)
    want = _save_ply_expression(*six)
    assert want.shape == (P, row_cols(n_rest))
    rows = pack_rows(*(t.to(dev) for t in six))
    assert rows.is_contiguous() and _same_bits(rows, want), (P, sh)
    if P:
        assert _bits(rows[:, 3:6]) == bytes(12 * P)  # +0 normals
    back = unpack_rows(rows, n_rest)
    for got, t in zip(back, six):
        assert _same_bits(got, t), (P, sh, tuple(t.shape))
    noisy = want.clone()
    noisy[:, 3:6] = float("nan")  # the normals are not read
    for got, t in zip(unpack_rows(noisy.to(dev), n_rest), six):
        assert _same_bits(got, t), (P, sh, "normals ignored")


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_pack_into_a_block_off_the_16_byte_grid(dev, offset):
    """A block that starts 4, 8 or 12 bytes into a larger buffer takes the dword path; the floats either side stay."""
    from eogs2_amd.model import pack_rows, unpack_rows

    P, n_rest = 131, 3
    six = _random_six(P, n_rest, 7 + offset)
    want = _save_ply_expression(*six)
    buf = torch.full((P * 26 + 8,), 12345.0, device=dev)
    out = buf[offset:offset + P * 26].view(P, 26)
    assert out.data_ptr() % 16 == 4 * offset
    assert pack_rows(*(t.to(dev) for t in six), out=out) is out
    assert _same_bits(out, want) and bool((buf[:offset] == 12345.0).all()) and bool((buf[offset + P * 26:] == 12345.0).all())
    for got, t in zip(unpack_rows(out, n_rest), six):
        assert _same_bits(got, t)


# ---- 3. file ----
def _model_of(six, sh):
    from eogs2_amd.model import GaussianModel

    m = GaussianModel(sh)
    for n, t in zip(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), six):
        setattr(m, PARAMS[n], torch.nn.Parameter(t))
    return m


@pytest.mark.parametrize("sh,P", [(0, 1000), (1, 257), (3, 65), (0, 0)])
def test_save_ply_and_load_ply(dev, tmp_path, sh, P):
    from eogs2_amd.model import GaussianModel, attribute_names, parse_ply_header

    n_rest = (sh + 1) ** 2 - 1
    six = _random_six(P, n_rest, 50 + sh)
    m = _model_of([t.to(dev) for t in six], sh)
    path = str(tmp_path / "point_cloud" / "iteration_7" / "point_cloud.ply")  # the directory does not exist yet
    m.save_ply(path)
    data = open(path, "rb").read()
    names, count, offset = parse_ply_header(data)
    assert names == attribute_names(n_rest) == m.construct_list_of_attributes() and count == P and len(data) == offset + 4 * P * len(names)
    elements = np.fromfile(path, dtype=np.dtype([(n, "<f4") for n in names]), offset=offset)
    want = _save_ply_expression(*six).numpy()
    assert elements.shape == (P,)
    for j, n in enumerate(names):
        assert elements[n].tobytes() == np.ascontiguousarray(want[:, j]).tobytes(), n
    fresh = GaussianModel(sh)
    fresh.load_ply(path)
    assert fresh.active_sh_degree == sh
    for n, t in zip(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), six):
        p = getattr(fresh, PARAMS[n])
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.device == dev and _same_bits(p, t), n
    if sh:
        with pytest.raises(AssertionError):  # the reference's assertion on the f_rest columns
            GaussianModel(0).load_ply(path)
    m.save_ply(path)  # writing over a file that exists
    assert open(path, "rb").read() == data


def test_load_ply_with_permuted_columns(dev, tmp_path):
    """Properties in another order, an extra one among them, no normals: mapped by name, permuted on the host."""
    from eogs2_amd.model import GaussianModel, attribute_names, ply_header

    sh, P, n_rest = 2, 301, 8
    six = _random_six(P, n_rest, 77)
    canon = attribute_names(n_rest)
    block = _save_ply_expression(*six).numpy()
    order = [j for j in np.random.default_rng(5).permutation(len(canon)) if canon[j] not in ("nx", "ny", "nz")]
    names = [canon[j] for j in order]
    cols = [block[:, j] for j in order]
    names.insert(4, "confidence")
    cols.insert(4, np.full(P, 9.0, np.float32))
    path = str(tmp_path / "shuffled.ply")
    with open(path, "wb") as f:
        f.write(ply_header(names, P).replace(b"element vertex", b"comment shuffled by hand\nelement vertex"))
        f.write(np.ascontiguousarray(np.stack(cols, axis=1), dtype="<f4").tobytes())
    m = GaussianModel(sh)
    m.load_ply(path)
    for n, t in zip(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), six):
        assert _same_bits(getattr(m, PARAMS[n]), t), n
    with open(path, "r+b") as f:  # a truncated payload is refused
        f.truncate(os.path.getsize(path) - 4)
    with pytest.raises(ValueError, match="bytes after the header"):
        GaussianModel(sh).load_ply(path)
    double = str(tmp_path / "double.ply")
    with open(double, "wb") as f:
        f.write(ply_header(canon, 1).replace(b"property float opacity", b"property double opacity"))
        f.write(bytes(4 * len(canon) + 4))
    with pytest.raises(ValueError, match="float32 scalar"):
        GaussianModel(sh).load_ply(double)


# ---- 4. lifecycle ----
def _model_from_snapshot(fx, snap, dev, capturable=False):
    """A GaussianModel holding the fp32 state of the fixture's snapshot, set up by its own training_setup."""
    from eogs2_amd.model import GaussianModel
    from eogs2_amd.optim import FusedAdam

    m = GaussianModel(fx.cfg["sh"])
    for n in oc.GROUPS:
        setattr(m, PARAMS[n], torch.nn.Parameter(fx.t(f"{snap}/{n}/p", dev)))
    m.spatial_lr_scale = 1
    m.training_setup(ARGS, capturable=capturable)
    assert type(m.optimizer) is FusedAdam and [g["name"] for g in m.optimizer.param_groups] == list(oc.GROUPS)
    assert [g["lr"] for g in m.optimizer.param_groups] == [oc.lrs()[n] for n in oc.GROUPS] and m.percent_dense == oc.TRAIN_ARGS["percent_dense"]
    assert all(g["eps"] == oc.EPS and g["betas"] == oc.BETAS for g in m.optimizer.param_groups) and m.exposure_optimizer is None
    assert m.xyz_gradient_accum.shape == m.denom.shape == (m._xyz.shape[0], 1) and not m.xyz_gradient_accum.any()
    for g, n, s in zip(m.optimizer.param_groups, oc.GROUPS, fx.z[f"{snap}/step"]):
        assert g["params"][0] is getattr(m, PARAMS[n])
        if s >= 0:
            step = torch.tensor(float(s), device=dev) if capturable else torch.tensor(float(s))
            m.optimizer.state[g["params"][0]] = {"step": step, "exp_avg": fx.t(f"{snap}/{n}/m", dev), "exp_avg_sq": fx.t(f"{snap}/{n}/v", dev)}
    m.xyz_gradient_accum, m.denom, m.max_radii2D = (fx.t(f"{snap}/{k}", dev) for k in oc.STATS)
    return m


def _stats(m):
    return dict(zip(oc.STATS, (m.xyz_gradient_accum, m.denom, m.max_radii2D)))


def _attributes_are_the_optimizer_s(m):
    for g in m.optimizer.param_groups:
        assert g["params"][0] is getattr(m, PARAMS[g["name"]]), g["name"]
    P = m._xyz.shape[0]
    assert m.xyz_gradient_accum.shape == (P, 1) and m.denom.shape == (P, 1) and m.max_radii2D.shape == (P,)


def _run_steps(m, st, ids, sh, dev):
    """optim_cases.run_steps over the model: the statistics through add_densification_stats, in both of its forms."""
    for k in range(st["n"]):
        it = st["it0"] + k + 1
        for g in m.optimizer.param_groups:
            g["params"][0].grad = oc.hashed_grad(it, ids, g["name"], sh).to(dev)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        if st["stats"]:
            r, vs = oc.radii(it, ids).to(dev), types.SimpleNamespace(grad=oc.viewspace_grad(it, ids).to(dev))
            vis = r > 0
            if it % 3 == 0:  # train_pan.py:683-690 as written there: the mask ...
                m.max_radii2D[vis] = torch.max(m.max_radii2D[vis], r[vis])
                m.add_densification_stats(vs, vis)
            elif it % 3 == 1:  # ... the index list of the renderer's visibility_filter ...
                m.max_radii2D[vis] = torch.max(m.max_radii2D[vis], r[vis])
                m.add_densification_stats(vs, vis.nonzero().squeeze(-1))
            else:  # ... and both lines in one launch
                m.add_densification_stats(vs, None, radii=r.to(torch.int32))


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_lifecycle_through_the_model_matches_the_reference_fixture(dev, name):
    """Every stage of the fixture from the fixture's fp32 pre-stage state, through GaussianModel's methods. The id column of the
    fixtures is not a tensor of the model: row identity is held by the bit-equality of every moved row."""
    fx, log = oc.Fixture(name), []
    sh, cfg = fx.cfg["sh"], fx.cfg
    try:
        for i, st in enumerate(fx.stages):
            src, dst, op = st["src"], st["dst"], st["op"]
            m = _model_from_snapshot(fx, src, dev)
            ids_dst = fx.t(f"{dst}/ids", dev)
            if op == "steps":
                _run_steps(m, st, fx.ids(src), sh, dev)
                oc.check_steps(fx, st, m.optimizer, _stats(m), False, log)
            elif op in ("tprune", "prune"):
                mask = fx.t(st["mask"], dev)
                valid = m.prune_points(mask)
                assert torch.equal(valid, ~mask)
                oc.check_structural(fx, st, m.optimizer, _stats(m), ids_dst, None, False, log)
            elif op == "clone":
                # the three stages as the reference's one call, in the one pass ...
                clone, split, prune = fx.stages[i:i + 3]
                with oc.normal_returns(fx.t(split["normal"], dev)) as nr:
                    info = m.densify_and_prune(cfg["grad_threshold"], oc.DENSIFY_MIN_OPACITY, cfg["extent"], prune["max_screen_size"],
                                               fx.t(clone["radii"], dev), cfg["extent"])
                assert nr.calls == 1 and m.tmp_radii is None
                for got, s in ((info.clone_mask(), clone), (info.split_mask(), split), (info.prune_mask(), prune)):
                    assert np.array_equal(got.cpu().numpy(), fx.z[s["mask"]]), (name, s["op"])
                _check_one_pass(fx, clone["src"], prune["dst"], m, info, log)
                # ... and stage by stage: densify_and_clone here, densify_and_split and the final prune at their own stages
                m = _model_from_snapshot(fx, src, dev)
                m.tmp_radii = fx.t(st["radii"], dev)
                grads = oc.mean_grads(m.xyz_gradient_accum.clone(), m.denom)
                m.densify_and_clone(grads, cfg["grad_threshold"], cfg["extent"], cfg["extent"])
                oc.check_structural(fx, st, m.optimizer, _stats(m), ids_dst, m.tmp_radii, False, log)
            elif op == "split":
                before = fx.stages[i - 1]["src"]  # the statistics the reference's densify_and_prune took its `grads` from
                grads = oc.mean_grads(fx.t(f"{before}/xyz_gradient_accum", dev), fx.t(f"{before}/denom", dev))
                m.tmp_radii = fx.t(st["radii"], dev)
                with oc.normal_returns(fx.t(st["normal"], dev)) as nr:
                    m.densify_and_split(grads, cfg["grad_threshold"], cfg["extent"], cfg["extent"], N=st["N"])
                assert nr.calls == 1
                oc.check_structural(fx, st, m.optimizer, _stats(m), ids_dst, m.tmp_radii, False, log)
            elif op == "reset":
                ptrs = [(t.data_ptr(), id(t)) for t in _state_tensors(m)]
                m.reset_opacity()  # in place: the same Parameter, the same moment tensors, the same addresses
                assert ptrs == [(t.data_ptr(), id(t)) for t in _state_tensors(m)]
                oc.check_structural(fx, st, m.optimizer, _stats(m), ids_dst, None, False, log)
                m = _model_from_snapshot(fx, src, dev)
                old = m._opacity
                m.reset_opacity(in_place=False)  # the reference's replacement
                assert m._opacity is not old and isinstance(m._opacity, torch.nn.Parameter) and old not in m.optimizer.state
                oc.check_structural(fx, st, m.optimizer, _stats(m), ids_dst, None, False, log)
            else:
                raise ValueError(op)
            _attributes_are_the_optimizer_s(m)
    finally:
        print("\n".join(log))


def _state_tensors(m):
    out = []
    for g in m.optimizer.param_groups:
        p = g["params"][0]
        out += [p, m.optimizer.state[p]["exp_avg"], m.optimizer.state[p]["exp_avg_sq"]]
    return out


def _check_one_pass(fx, src, dst, m, info, log):
    """The acceptance of tests/test_gpu_density.py::test_fixture_densify_and_prune on the model's tensors."""
    n_old = info.n_kept + info.n_kept_clones
    for n, want_step in zip(oc.GROUPS, fx.z[f"{dst}/step"]):
        p = getattr(m, PARAMS[n])
        state = m.optimizer.state[p]
        assert int(state["step"]) == int(want_step) == int(fx.z[f"{src}/step"][oc.GROUPS.index(n)]), (fx.name, n, "step")
        for kk, got in (("p", p.detach()), ("m", state["exp_avg"]), ("v", state["exp_avg_sq"])):
            key = f"{dst}/{n}/{kk}"
            got, want = got.cpu().numpy(), fx.z[key]
            assert got.dtype == np.float32 and got.shape == want.shape, (fx.name, key, got.shape, want.shape)
            if kk == "p" and n in ("xyz", "scaling"):
                assert got[:n_old].tobytes() == want[:n_old].tobytes(), (fx.name, key, "moved rows")
                r = oc._computed_close(fx, key, got, slice(n_old, None))
                log.append(f"{fx.name} {key}: one pass, computed rows at {r:.3f} of their bound")
            else:
                assert got.tobytes() == want.tobytes(), (fx.name, key)
    for kk, t in _stats(m).items():  # zeros of the new size
        assert _bits(t) == fx.z[f"{dst}/{kk}"].tobytes() and not bool(t.any()), (fx.name, kk)
    assert len(m.optimizer.state) == len(oc.GROUPS)


def _checkpoint(obj):
    """Through torch.save / torch.load, as train_pan.py writes and reads `(gaussians.capture(), iteration)`."""
    f = io.BytesIO()
    torch.save(obj, f)
    f.seek(0)
    return torch.load(f, weights_only=False)


def _train(m, its, ids, sh, dev):
    for it in its:
        for g in m.optimizer.param_groups:
            g["params"][0].grad = oc.hashed_grad(it, ids, g["name"], sh).to(dev)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        m.add_densification_stats(types.SimpleNamespace(grad=oc.viewspace_grad(it, ids).to(dev)), None, radii=oc.radii(it, ids).to(dev))


def _assert_same_state(a, b, step):
    assert a.active_sh_degree == b.active_sh_degree and a.spatial_lr_scale == b.spatial_lr_scale and a.percent_dense == b.percent_dense
    for ga, gb in zip(a.optimizer.param_groups, b.optimizer.param_groups):
        pa, pb = ga["params"][0], gb["params"][0]
        assert ga["name"] == gb["name"] and ga["lr"] == gb["lr"] and _same_bits(pa, pb), ga["name"]
        sa, sb = a.optimizer.state[pa], b.optimizer.state[pb]
        assert _same_bits(sa["exp_avg"], sb["exp_avg"]) and _same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"]), ga["name"]
        assert float(sa["step"]) == float(sb["step"]) == step and sa["step"].device == sb["step"].device, ga["name"]
    for k in oc.STATS:
        assert _same_bits(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("capturable", [False, True])
def test_capture_restore_then_one_more_step_is_the_uninterrupted_run(dev, init_fixtures, capturable):
    from eogs2_amd.model import GaussianModel
    from eogs2_amd.optim import FusedAdam

    z = init_fixtures["sh1_257"]
    P, sh, ids = 257, 1, np.arange(257)
    a = GaussianModel(sh)
    a.create_from_pcd(types.SimpleNamespace(points=z["points"], colors=z["colors"]), _cams(), 1, 0.1, dist2=torch.from_numpy(z["dist2"]).to(dev))
    a.training_setup(ARGS, capturable=capturable)
    a.oneupSHdegree()
    _train(a, (1, 2, 3), ids, sh, dev)
    a.optimizer.param_groups[0]["lr"] = 3e-5  # a learning rate changed along the way is part of the checkpoint
    ckpt = _checkpoint(a.capture())
    assert len(ckpt) == 12 and ckpt[0] == 1 and ckpt[11] == 1 and set(ckpt[10]) == {"state", "param_groups"}
    b = GaussianModel(sh)
    b.restore(ckpt, ARGS)
    assert type(b.optimizer) is FusedAdam and bool(b.optimizer.defaults.get("capturable")) == capturable
    for g in b.optimizer.param_groups:
        step = b.optimizer.state[g["params"][0]]["step"]
        assert (step.is_cuda and step.dtype == torch.float32 and step.ndim == 0) if capturable else not step.is_cuda, g["name"]
        assert g["params"][0] is getattr(b, PARAMS[g["name"]]) and g["params"][0].data_ptr() != getattr(a, PARAMS[g["name"]]).data_ptr()
    _assert_same_state(a, b, 3)
    _train(a, (4,), ids, sh, dev)
    _train(b, (4,), ids, sh, dev)
    _assert_same_state(a, b, 4)
    if capturable:
        for g in b.optimizer.param_groups:
            lr = g["lr_tensor"]
            assert lr.is_cuda and float(lr) == np.float32(g["lr"]), g["name"]


def test_restore_takes_a_tuple_captured_from_torch_adam(dev, init_fixtures):
    """The reference's own checkpoint: torch.optim.Adam over the same six groups."""
    from eogs2_amd.model import GaussianModel, init_tensors
    from eogs2_amd.optim import FusedAdam

    z = init_fixtures["sh0_1000"]
    P, sh, ids = 1000, 0, np.arange(1000)
    t = init_tensors(*(torch.from_numpy(z[k]).to(dev) for k in ("points", "colors", "dist2")), sh)
    par = {n: torch.nn.Parameter(t[n].clone()) for n in oc.GROUPS}
    ref = torch.optim.Adam([{"params": [par[n]], "lr": oc.lrs()[n], "name": n} for n in oc.GROUPS], lr=0.0, eps=1e-15)
    for it in (1, 2):
        for n in oc.GROUPS:
            par[n].grad = oc.hashed_grad(it, ids, n, sh).to(dev)
        ref.step()
    accum, denom = torch.rand(P, 1, device=dev), torch.ones(P, 1, device=dev)
    ckpt = _checkpoint((0, par["xyz"], par["f_dc"], par["f_rest"], par["scaling"], par["rotation"], par["opacity"], t["max_radii2D"],
                        accum, denom, ref.state_dict(), 1))
    m = GaussianModel(sh)
    m.restore(ckpt, ARGS)
    assert type(m.optimizer) is FusedAdam and not m.optimizer.defaults.get("capturable")
    assert _same_bits(m.xyz_gradient_accum, accum) and _same_bits(m.denom, denom)
    for g in m.optimizer.param_groups:
        p, n = g["params"][0], g["name"]
        st, want = m.optimizer.state[p], ref.state[par[n]]
        assert _same_bits(p, par[n]) and int(st["step"]) == 2 and not st["step"].is_cuda, n
        assert _same_bits(st["exp_avg"], want["exp_avg"]) and _same_bits(st["exp_avg_sq"], want["exp_avg_sq"]), n
    # training goes on: one step of each from the same state, every element against float64 within optim_cases.adam_step_bound
    for n in oc.GROUPS:
        par[n].grad = oc.hashed_grad(3, ids, n, sh).to(dev)
    for g in m.optimizer.param_groups:
        p, n = g["params"][0], g["name"]
        if not p.numel():
            continue
        st = m.optimizer.state[p]
        args = (p.detach().cpu().clone(), par[n].grad.cpu(), st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone(), float(g["lr"]), g["betas"], g["eps"], 3)
        p.grad = par[n].grad.clone()
        g["want"] = (oc.adam_step_f64(*args)[0], oc.adam_step_bound(*args)[2])
    m.optimizer.step()
    for g in m.optimizer.param_groups:
        if "want" in g:
            want, bound = g.pop("want")
            assert int(m.optimizer.state[g["params"][0]]["step"]) == 3
            assert bool(((g["params"][0].detach().cpu().double() - want).abs() <= oc.FACTOR_KERNEL * bound).all()), g["name"]
    # and a capturable optimizer on request: the counts move to the device
    m2 = GaussianModel(sh)
    m2.restore(ckpt, ARGS, capturable=True)
    assert all(m2.optimizer.state[g["params"][0]]["step"].is_cuda and g["capturable"] for g in m2.optimizer.param_groups if g["params"][0].numel())


def test_example_saves_a_ply_and_starts_from_it(dev, tmp_path):
    """examples/train_synthetic.py --save-ply / --load-ply: the file holds the trainee of the last iteration, a run started from
    it begins where that run ended, and neither flag changes what the run computes."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    from eogs2_amd.model import GaussianModel

    args = ["--gaussians", "3000", "--size", "64", "--iters", "20", "--no-prune", "--quiet"]
    path = str(tmp_path / "point_cloud.ply")
    plain = train_synthetic.main(args)
    saved = train_synthetic.main(args + ["--save-ply", path])
    assert saved == plain
    m = GaussianModel(0)
    m.load_ply(path)
    assert m._xyz.shape == (3000, 3) and m._features_rest.shape == (3000, 0, 3) and bool(torch.isfinite(m._opacity).all())
    with pytest.raises(SystemExit):  # a file with another row count than --gaussians is refused before anything runs
        train_synthetic.main(["--gaussians", "2000"] + args[2:] + ["--load-ply", path])
    first, _, n = train_synthetic.main(args + ["--load-ply", path])
    assert n == 3000 and first < plain[0]  # the first loss of the resumed run is below the first loss of the fresh one


# ---- the optimizer methods an integrator's own code may call ----
def _snapshot_model(dev, name="sh1", snap="s1"):
    fx = oc.Fixture(name)
    return fx, _model_from_snapshot(fx, snap, dev)


def test_replace_tensor_to_optimizer(dev):
    """gaussian_model.py:451-464: a new Parameter under the group, zero moments of its shape, `step` kept, the other groups
    untouched; a group that has not stepped yet is replaced too; an unknown name changes nothing."""
    fx, m = _snapshot_model(dev)
    others = {g["name"]: (g["params"][0], m.optimizer.state[g["params"][0]]) for g in m.optimizer.param_groups if g["name"] != "opacity"}
    old, step = m._opacity, int(m.optimizer.state[m._opacity]["step"])
    new = torch.full_like(old.detach(), -3.0)
    out = m.replace_tensor_to_optimizer(new, "opacity")
    p = out["opacity"]
    assert set(out) == {"opacity"} and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.data_ptr() == new.data_ptr()
    group = next(g for g in m.optimizer.param_groups if g["name"] == "opacity")
    st = m.optimizer.state[p]
    assert group["params"][0] is p and old not in m.optimizer.state and len(m.optimizer.state) == len(oc.GROUPS)
    assert int(st["step"]) == step and st["exp_avg"].shape == p.shape and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    for g in m.optimizer.param_groups:
        if g["name"] != "opacity":
            q, state = others[g["name"]]
            assert g["params"][0] is q and m.optimizer.state[q] is state
    assert m.replace_tensor_to_optimizer(new.clone(), "no_such_group") == {}
    m._opacity = p
    for g in m.optimizer.param_groups:  # training goes on over the replaced tensor
        g["params"][0].grad = torch.ones_like(g["params"][0])
    m.optimizer.step()
    assert int(m.optimizer.state[p]["step"]) == step + 1
    # before the first step there is no state to clear
    fresh = _model_from_snapshot(oc.Fixture("prune_only"), "s0", dev)
    assert len(fresh.optimizer.state) == 0
    out = fresh.replace_tensor_to_optimizer(torch.zeros_like(fresh._scaling.detach()), "scaling")
    assert len(fresh.optimizer.state) == 0 and next(g for g in fresh.optimizer.param_groups if g["name"] == "scaling")["params"][0] is out["scaling"]


def test_cat_prune_and_postfix_equal_their_torch_expressions(dev):
    """`cat_tensors_to_optimizer`, `densification_postfix` and `_prune_optimizer` against torch.cat / boolean indexing on clones."""
    fx, m = _snapshot_model(dev)
    P, sh = m._xyz.shape[0], fx.cfg["sh"]
    g = torch.Generator().manual_seed(9)
    before = {n: (getattr(m, PARAMS[n]).detach().clone(), m.optimizer.state[getattr(m, PARAMS[n])]["exp_avg"].clone(),
                  m.optimizer.state[getattr(m, PARAMS[n])]["exp_avg_sq"].clone()) for n in oc.GROUPS}
    ext = {n: torch.randn((7,) + oc.shapes(sh)[n], generator=g).to(dev) for n in oc.GROUPS}

    def check(rows_of):
        for n in oc.GROUPS:
            p = next(gr for gr in m.optimizer.param_groups if gr["name"] == n)["params"][0]
            st = m.optimizer.state[p]
            want_p, want_m, want_v = rows_of(n)
            assert _same_bits(p, want_p) and _same_bits(st["exp_avg"], want_m) and _same_bits(st["exp_avg_sq"], want_v), n
            assert isinstance(p, torch.nn.Parameter) and p.requires_grad and int(st["step"]) == int(fx.z["s1/step"][oc.GROUPS.index(n)])
        assert len(m.optimizer.state) == len(oc.GROUPS)

    grown = lambda n: (torch.cat((before[n][0], ext[n])), torch.cat((before[n][1], torch.zeros_like(ext[n]))),  # noqa: E731
                       torch.cat((before[n][2], torch.zeros_like(ext[n]))))
    out = m.cat_tensors_to_optimizer(ext)
    assert set(out) == set(oc.GROUPS)
    check(grown)
    # densification_postfix: the same append, the attributes adopted, tmp_radii extended, the three statistics zero at the new size
    m = _model_from_snapshot(fx, "s1", dev)
    m.tmp_radii = torch.arange(P, dtype=torch.float32, device=dev)
    m.densification_postfix(ext["xyz"], ext["f_dc"], ext["f_rest"], ext["opacity"], ext["scaling"], ext["rotation"], torch.full((7,), 5.0, device=dev))
    check(grown)
    _attributes_are_the_optimizer_s(m)
    assert m.tmp_radii.shape == (P + 7,) and bool((m.tmp_radii[P:] == 5.0).all())
    assert not m.xyz_gradient_accum.any() and not m.denom.any() and not m.max_radii2D.any()
    # _prune_optimizer: a KEEP mask over the grown model
    keep = (torch.rand(P + 7, generator=g) < 0.6).to(dev)
    out = m._prune_optimizer(keep)
    assert set(out) == set(oc.GROUPS) and out["xyz"].shape[0] == int(keep.sum())
    check(lambda n: tuple(t[keep] for t in grown(n)))
