"""GPU (MI355X): the image chain of include/eogs_shade.h at its edges, every element against the float64 oracle inside its
own bound, non-finite patterns and signed zeros exactly (tests/shade_cases.py; DESIGN.md §8, f2 image chain)."""
import numpy as np
import pytest
import torch

import shade_cases as sc
from oracle import shade_oracle as O
from test_shade_oracle import run_mloss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


# ---- shadow pipeline ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,H,W,shadow", sc.PIPE_CASES, ids=lambda v: str(v))
def test_pipeline_edges(dev, kind, H, W, shadow):
    from eogs2_amd.shade import shade

    if H * W == 1:
        variants = [dict(plant=i) for i in range(sc.NPLANT)]
    else:
        variants = [dict(nan=False), dict(nan=True)]  # finite first: with a NaN every parameter sum is NaN
    for v in variants:
        fx = sc.pipeline_case(kind, H, W, shadow, **v)
        got = sc.run_shade(shade, fx, torch.float32, dev)
        ref = sc.run_shade(O.render_pipeline, fx, torch.float64, "cpu")
        sc.check_shade(got, ref, fx, f"{kind} {H}x{W} shadow={shadow} {v}")
        if shadow and v.get("nan"):
            p = H * W // 2  # the NaN altitude difference: kept in everything that holds s, 0 in its own gradient
            assert np.isnan(got["shadow"].flat[p]) and np.isnan(got["shaded"].reshape(3, -1)[:, p]).all()
            assert np.isnan(got["g_raw"].reshape(3, -1)[:, p]).all() and np.isnan(got["g_M"]).all() and np.isnan(got["g_inshadow"]).all()
            assert got["g_alt_diff"].flat[p] == 0.0 and not np.isnan(got["cc"].reshape(3, -1)[:, p]).any()


def test_golden_edge_vectors(dev):
    """The small edge cases the reference's own modules ran (tests/golden/shade_edgepipe_*.npz) hold the same inputs as the case
    functions; the kernels are held to the oracle on them, the oracle to the vectors in tests/test_shade_oracle.py."""
    from eogs2_amd.shade import shade

    paths = sc.fixtures("edgepipe_")
    assert len(paths) == len(sc.GOLDEN_PIPE)
    for path in paths:
        fx = sc.load(path)
        got = sc.run_shade(shade, fx, torch.float32, dev)
        ref = sc.run_shade(O.render_pipeline, fx, torch.float64, "cpu")
        sc.check_shade(got, ref, fx, path)


# ---- masked losses --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", sc.mloss_case_list(), ids=lambda v: str(v))
def test_masked_loss_edges(dev, name, mode):
    """Outside the mask nothing is read into the sums: the losses are the reference's on the inputs with the
    masked-out non-finite values replaced by 0. Inside the mask a non-finite value reaches the loss in both. The gradients
    are the reference's on the inputs as they are (finite there too), zeros with their signs."""
    from eogs2_amd.shade import randomcam_l, suncamera_l

    fx = sc.mloss_case(name, mode)
    got = run_mloss(suncamera_l, randomcam_l, fx, torch.float32, dev)
    ref = run_mloss(O.suncamera_l, O.randomcam_l, sc.masked_out_zeroed(fx), torch.float64, "cpu")
    proper = run_mloss(O.suncamera_l, O.randomcam_l, fx, torch.float64, "cpu")
    ref.update({k: proper[k] for k in ("g_alt_diff", "g_rgb_a", "g_rgb_b")})
    sc.check_mloss_elementwise(got, ref, fx, f"{name} {mode}")
    m = sc.mloss_mask(fx)
    if name == "one_pixel":
        assert int(m.sum()) == 1
    if name == "image_1x1_in":
        assert m.all() and got["L_alt"] == float(np.float32(0.004))
    if name in ("empty", "image_1x1_out"):
        assert not m.any() and got["L_alt"] == 0.0 and got["L_rgb"] == 0.0
    if name == "full513":
        assert m.all()
    if name in ("nonfinite_out", "uv_nan"):
        assert np.isfinite(got["L_alt"]) and np.isfinite(got["L_rgb"])
    if name == "alt_inf_in":
        assert got["L_alt"] == np.inf and np.isfinite(got["L_rgb"])
    if name == "rgb_nan_in":
        assert np.isnan(got["L_rgb"]) and np.isfinite(got["L_alt"])
    if name == "rgb_inf_in":
        assert got["L_rgb"] == np.inf
    for k in ("g_alt_diff", "g_rgb_a", "g_rgb_b"):
        assert np.isfinite(got[k]).all(), k


# ---- translucent shadow ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.TSHADOW_CASES)
def test_translucent_shadow_edges(dev, name):
    from eogs2_amd.shade import translucentshadows_l

    fx = sc.tshadow_case(name)
    got = sc.run_tshadow(translucentshadows_l, fx, torch.float32, dev)
    ref = sc.run_tshadow(O.translucentshadows_l, fx, torch.float64, "cpu")
    sc.check_tshadow(got, ref, fx, name)
    if name == "nan":
        bad = np.isnan(fx["a"])
        assert np.isnan(got["L"]) and np.isnan(got["g_a"][bad]).all() and np.isfinite(got["g_a"][~bad]).all()


# ---- API ------------------------------------------------------------------------------------------------------------
def _leaves(fx, dtype, dev):
    t = lambda a: torch.tensor(a, device=dev).to(dtype)
    return (t(fx["raw"]).requires_grad_(True), t(fx["alt_diff"]).requires_grad_(True),
            sc.matrix_of(fx, torch.float32, dev).to(dtype).requires_grad_(True), t(fx["inshadow"]).requires_grad_(True))


def _weighted(outs, fx, dev, use=("cc", "shaded", "shadow")):
    w = dict(cc=fx["g_cc"], shaded=fx["g_shaded"], shadow=fx["g_shadow"])
    return sum((o.float() * torch.tensor(w[k], device=dev)).sum() for k, o in zip(("cc", "shaded", "shadow"), outs) if k in use)


API_FX = lambda: sc.pipeline_case("exposure", 1, 257, True)


@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16])
def test_other_input_dtypes(dev, dtype):
    """Inputs are converted to fp32 for the kernel; outputs are fp32, gradients come back in each input's dtype and shape and
    are the fp32 gradients of the converted values, rounded."""
    from eogs2_amd.shade import randomcam_l, shade, translucentshadows_l

    fx = API_FX()
    fx["alt_diff"] = np.where(np.isfinite(fx["alt_diff"]), fx["alt_diff"], -1.0).astype(np.float32)
    leaves = _leaves(fx, dtype, dev)
    outs = shade(*leaves)
    assert all(o.dtype == torch.float32 for o in outs)
    _weighted(outs, fx, dev).backward()
    l32 = [x.detach().float().requires_grad_(True) for x in leaves]
    o32 = shade(*l32)
    _weighted(o32, fx, dev).backward()
    for a, b in zip(outs, o32):
        assert torch.equal(a, b)
    for x, y in zip(leaves, l32):
        assert x.grad.dtype == dtype and x.grad.shape == x.shape and torch.equal(x.grad, y.grad.to(dtype))
    # the two losses
    mf = sc.mloss_case("thresholds", "random")
    t = lambda k: torch.tensor(mf[k], device=dev).to(dtype)
    a, b, alt = t("rgb_a").requires_grad_(True), t("rgb_b").requires_grad_(True), t("alt_diff").requires_grad_(True)
    L = randomcam_l(alt, a, b, t("uv"))
    (L[0] - 2 * L[1]).backward()
    a2, b2, alt2 = (x.detach().float().requires_grad_(True) for x in (a, b, alt))
    L2 = randomcam_l(alt2, a2, b2, t("uv").float())
    (L2[0] - 2 * L2[1]).backward()
    assert torch.equal(L[0], L2[0]) and torch.equal(L[1], L2[1])
    for x, y in ((a, a2), (b, b2), (alt, alt2)):
        assert x.grad.dtype == dtype and x.grad.shape == x.shape and torch.equal(x.grad, y.grad.to(dtype))
    x = torch.tensor(sc.tshadow_case("edges")["a"], device=dev).to(dtype).reshape(5, 7).requires_grad_(True)
    translucentshadows_l(x).backward()
    x2 = x.detach().float().requires_grad_(True)
    translucentshadows_l(x2).backward()
    assert x.grad.dtype == dtype and x.grad.shape == (5, 7) and torch.equal(x.grad, x2.grad.to(dtype))


def test_non_contiguous_inputs(dev):
    from eogs2_amd.shade import shade, translucentshadows_l

    fx = API_FX()
    raw, alt, M, ins = _leaves(fx, torch.float32, dev)
    wide = torch.full((3, 1, 514), 7.0, device=dev)  # what a kernel reading the slice's storage as contiguous would pick up
    wide[:, :, ::2] = raw.detach()
    raw_nc = wide[:, :, ::2].requires_grad_(True)
    alt_nc = torch.stack([alt.detach(), torch.full_like(alt, -3.0)], dim=-1)[..., 0].requires_grad_(True)
    M_nc = M.detach().t().contiguous().t().requires_grad_(True)
    assert not raw_nc.is_contiguous() and not alt_nc.is_contiguous() and not M_nc.is_contiguous()
    res = []
    for args in ((raw, alt, M, ins), (raw_nc, alt_nc, M_nc, ins.detach().clone().requires_grad_(True))):
        outs = shade(*args)
        _weighted(outs, fx, dev).backward()
        res.append([*outs, *(x.grad for x in args)])
    for a, b in zip(*res):
        assert a.shape == b.shape and np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy(), equal_nan=True)
    x = torch.tensor(sc.tshadow_case("edges")["a"], device=dev)
    x_nc = torch.stack([x, x + 1], dim=-1)[..., 0].requires_grad_(True)
    xc = x.clone().requires_grad_(True)
    translucentshadows_l(x_nc).backward()
    translucentshadows_l(xc).backward()
    assert not x_nc.is_contiguous() and torch.equal(x_nc.grad, xc.grad)


@pytest.mark.parametrize("mode", sc.MLOSS_MODES)
def test_non_contiguous_masked_loss_inputs(dev, mode):
    """The kernel reads uv as float2 pairs and the planes as dense rows: a strided uv (two of three channels), altitude difference
    and rgb plane give the bits of their contiguous copies."""
    from eogs2_amd.shade import randomcam_l, suncamera_l

    mf = sc.mloss_case("thresholds", mode)
    t = lambda k: torch.tensor(mf[k], device=dev)
    uv3 = torch.cat([t("uv"), torch.full((7, 9, 1), 0.5, device=dev)], dim=-1)
    uv_nc = uv3[..., :2]
    alt_nc = torch.stack([t("alt_diff"), torch.full((7, 9), 0.001, device=dev)], dim=-1)[..., 0]
    a_nc = torch.stack([t("rgb_a"), t("rgb_b")], dim=-1)[..., 0]
    assert not uv_nc.is_contiguous() and not alt_nc.is_contiguous() and not a_nc.is_contiguous()
    res = []
    for a, alt, uv in ((t("rgb_a"), t("alt_diff"), t("uv")), (a_nc, alt_nc, uv_nc)):
        a, b, alt = a.requires_grad_(True), t("rgb_b").requires_grad_(True), alt.requires_grad_(True)
        L = suncamera_l(a, b, alt, uv) if mode == "sun" else randomcam_l(alt, a, b, uv)
        (0.7 * L[0] - 1.3 * L[1]).backward()
        res.append([L[0].detach(), L[1].detach(), a.grad, b.grad, alt.grad])
    for x, y in zip(*res):
        assert x.shape == y.shape and torch.equal(tc_bits(x), tc_bits(y))
    assert float(res[0][2].abs().max()) > 0


def tc_bits(t):
    return t.contiguous().view(torch.int32)


def test_second_backward_with_retain_graph(dev):
    from eogs2_amd.shade import shade, suncamera_l, translucentshadows_l

    fx = API_FX()
    leaves = _leaves(fx, torch.float32, dev)
    loss = _weighted(shade(*leaves), fx, dev)
    loss.backward(retain_graph=True)
    g1 = [x.grad.clone() for x in leaves]
    for x in leaves:
        x.grad = None
    loss.backward()
    for a, x in zip(g1, leaves):
        assert np.array_equal(a.cpu().numpy(), x.grad.cpu().numpy(), equal_nan=True)
    mf = sc.mloss_case("thresholds", "sun")
    t = lambda k: torch.tensor(mf[k], device=dev)
    a = t("rgb_a").requires_grad_(True)
    L = suncamera_l(a, t("rgb_b"), t("alt_diff"), t("uv"))[1]
    L.backward(retain_graph=True)
    g = a.grad.clone()
    a.grad = None
    L.backward()
    assert torch.equal(g, a.grad) and float(g.abs().max()) > 0
    x = torch.tensor(sc.tshadow_case("edges")["a"], device=dev).requires_grad_(True)
    L = translucentshadows_l(x)
    L.backward(retain_graph=True)
    g = x.grad.clone()
    x.grad = None
    L.backward()
    assert torch.equal(g, x.grad)


@pytest.mark.parametrize("use", ["cc", "shaded", "shadow"])
def test_one_output_used_downstream(dev, use):
    """The upstream gradients of the unused outputs are None (the g_cc / g_shadow NULL paths; a missing g_shaded is zeros):
    the same result as with explicit zero weights, held to the oracle's."""
    from eogs2_amd.shade import shade

    fx = sc.pipeline_case("cc", 255, 1, True)
    leaves = _leaves(fx, torch.float32, dev)
    _weighted(shade(*leaves), fx, dev, use=(use,)).backward()
    fz = dict(fx)
    for k in ("cc", "shaded", "shadow"):
        if k != use:
            fz["g_" + k] = np.zeros_like(fx["g_" + k])
    ref = sc.run_shade(O.render_pipeline, fz, torch.float64, "cpu")
    got = dict(g_raw=leaves[0].grad, g_alt_diff=leaves[1].grad, g_M=leaves[2].grad, g_inshadow=leaves[3].grad)
    if use == "cc":  # no path to the shadow inputs at all
        assert got["g_alt_diff"] is None or not got["g_alt_diff"].any()
        assert got["g_inshadow"] is None or not got["g_inshadow"].any()
        got = {k: got[k] for k in ("g_raw", "g_M")}
    got = {k: v.double().cpu().numpy() for k, v in got.items()}
    B = sc.shade_bounds(fz, ref)
    for k in got:
        sc.check(got[k], ref[k], B[k], f"only {use}: {k}", signed_zero=(k == "g_alt_diff"))


def test_non_default_stream(dev):
    from eogs2_amd.shade import randomcam_l, shade, translucentshadows_l

    fx = API_FX()
    mf = sc.mloss_case("thresholds", "random")
    tf = sc.tshadow_case("edges")

    def run():
        leaves = _leaves(fx, torch.float32, dev)
        outs = shade(*leaves)
        _weighted(outs, fx, dev).backward()
        t = lambda k: torch.tensor(mf[k], device=dev)
        a = t("rgb_a").requires_grad_(True)
        L = randomcam_l(t("alt_diff"), a, t("rgb_b"), t("uv"))
        (L[0] + L[1]).backward()
        x = torch.tensor(tf["a"], device=dev).requires_grad_(True)
        T = translucentshadows_l(x)
        T.backward()
        return [o.detach() for o in outs] + [v.grad for v in leaves] + [L[0].detach(), L[1].detach(), a.grad, T.detach(), x.grad]

    base = run()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        other = run()
    s.synchronize()
    for a, b in zip(base, other):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
