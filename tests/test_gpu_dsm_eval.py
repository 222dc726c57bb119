"""GPU (MI355X): DSM evaluation (include/eogs_tsdf.h eogs_tsdf_dsm_*, eogs2_amd/dsm_eval.py) against the vectors the
reference's own eval/dsmr.py and eval/eval_dsm.py produced (tests/golden/dsm_eval/, pinned on the CPU by
tests/test_dsm_eval_oracle.py) and, beyond a fixture's size, against the restatement in tests/dsm_eval_cases.py.
downsample2x and apply_shift are bit-exact; (dx, dy) is equal at every pyramid level (the fixtures' NCC gap of >= 1e-6
makes it independent of the summation order); tables, moments, a, b, diff and MAE are within the bound derived from the
level's pixel count N (dsm_eval_cases.eps: 8 N 2^-53, the centred two-pass form's own reordering error)."""
import ctypes

import numpy as np
import pytest
import torch

import dsm_eval_cases as C
from dsm_eval_cases import REGISTRATION, check_ab, check_mae, check_moments, load, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_ncc(dev, u, v, irange, cx, cy, scale=1):
    """eogs_tsdf_dsm_ncc through the C-ABI: (result record, table)."""
    from eogs2_amd import _lib
    from eogs2_amd.dsm_eval import RESULT_DTYPE, read_results

    abi = _lib.get()
    n = 2 * irange + 1
    nb = ctypes.c_size_t()
    abi.check(abi.tsdf_dsm_ncc_bytes(u.shape[0], u.shape[1], irange, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    res = torch.zeros(RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    table = torch.empty((n, n), dtype=torch.float64, device=dev)
    centre = torch.tensor([cx, cy], dtype=torch.int32, device=dev)
    abi.check(abi.tsdf_dsm_ncc(u.shape[0], u.shape[1], p(u), v.shape[0], v.shape[1], p(v), int(u.dtype == torch.float64), irange,
                               p(centre), scale, p(table), p(res), p(ws), ws.numel(), stream()))
    return read_results(res)[0], table.cpu().numpy()


def check_table(got, ref, n, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    err = float(np.nanmax(np.abs(got - ref)))
    print(f"{what}: max NCC error {err:.3e} (eps {C.eps(n):.3e})")
    assert err <= C.eps(n), what


def test_downsample_fixtures(dev):
    from eogs2_amd import _lib
    from eogs2_amd.dsm_eval import downsample2x

    abi = _lib.get()
    z = load("downsample")
    for k in z:
        if not k.startswith("in_"):
            continue
        u = torch.from_numpy(z[k]).to(dev)
        assert same_bits(downsample2x(u).cpu().numpy(), z["out_" + k[3:]]), k
        out = torch.empty(z["out_" + k[3:]].shape, dtype=torch.float64, device=dev)
        abi.check(abi.tsdf_dsm_downsample(u.shape[0], u.shape[1], p(u), int(u.dtype == torch.float64), p(out), stream()))
        assert same_bits(out.cpu().numpy(), z["out_" + k[3:]]), k


def test_downsample_large_matches_the_restatement(dev):
    from eogs2_amd.dsm_eval import downsample2x

    for shape, dt in (((301, 517), np.float32), ((1000, 999), np.float64)):
        u, _ = C.shifted_pair(*shape, (0, 0), seed=31, dtype=dt)
        assert same_bits(downsample2x(torch.from_numpy(u).to(dev)).cpu().numpy(), C.downsample2x(u))


def test_apply_shift_fixtures(dev):
    from eogs2_amd import _lib
    from eogs2_amd.dsm_eval import apply_shift

    abi = _lib.get()
    z = load("apply_shift")
    for tag in ("float32", "float64"):
        v = torch.from_numpy(z[f"in_{tag}"]).to(dev)
        for k, (dx, dy, a, b, c, d) in enumerate(z["coefs"]):
            assert same_bits(apply_shift(v, int(dx), int(dy), a, b, c, d).cpu().numpy(), z[f"out_{tag}_{k}"]), (tag, k)
            out = torch.empty_like(v)
            abi.check(abi.tsdf_dsm_apply_shift(v.shape[0], v.shape[1], p(v), int(tag == "float64"), int(dx), int(dy), a, b, c, d,
                                               p(out), stream()))
            assert same_bits(out.cpu().numpy(), z[f"out_{tag}_{k}"]), (tag, k)
    assert same_bits(apply_shift(v).cpu().numpy(), z["in_float64"])  # the defaults are the identity


@pytest.mark.parametrize("name", REGISTRATION)
def test_registration_fixture(dev, name):
    from eogs2_amd.dsm_eval import compute_shift, compute_shift_device, ncc_search, read_results

    z = load(name)
    irange = int(z["irange"])
    u, v = C.rebuild(z)
    pyr = [(u, v)]
    while min(pyr[-1][0].shape) > 100:
        pyr.append((C.downsample2x(pyr[-1][0]), C.downsample2x(pyr[-1][1])))
    pyr = pyr[::-1]  # coarsest first, as recorded
    assert len(pyr) == len(z["levels_table"])
    for (lu, lv), t, c, w in zip(pyr, z["levels_table"], z["levels_centre"], z["levels_winner"]):
        gu, gv = torch.from_numpy(lu).to(dev), torch.from_numpy(lv).to(dev)
        dx, dy, table = ncc_search(gu, gv, irange, int(c[0]), int(c[1]))
        assert (dx, dy) == (int(w[0]), int(w[1])), (name, lu.shape)
        check_table(table.cpu().numpy(), t, lu.size, f"{name} {lu.shape} ncc_search")
        res, table = c_ncc(dev, gu, gv, irange, int(c[0]), int(c[1]))
        assert (int(res["dx"]), int(res["dy"]), int(res["valid"])) == (int(w[0]), int(w[1]), 1)
        check_table(table, t, lu.size, f"{name} {lu.shape} C-ABI")
        assert abs(res["ncc"] - np.nanmax(t)) <= C.eps(lu.size)
    # the last level is the full resolution: its winner's moments are compute_shift's mean_std_base
    check_moments([float(res[k]) for k in ("muu", "muv", "sigu", "sigv", "xcorr")], z, u.size, f"{name} C-ABI")
    gu, gv = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    dx, dy, a, b = compute_shift(gu, gv, scaling=True)
    assert (dx, dy) == tuple(int(t) for t in z["shift"]), name
    check_ab(a, b, z, "ab_scaling", u.size, name)
    dx, dy, a0, b0 = compute_shift(gu, gv, scaling=False)
    assert (dx, dy) == tuple(int(t) for t in z["shift"]) and a0 == 1 and isinstance(a0, int)
    muu, muv = float(z["moments"][0]), float(z["moments"][1])
    assert abs(b0 - float(z["ab_noscale"][1])) <= C.eps(u.size) * (abs(muu) + abs(muv))
    results, tables = compute_shift_device(gu, gv)
    r = read_results(results)[::-1]
    for k in range(len(pyr)):
        assert (int(r[k]["dx"]), int(r[k]["dy"])) == tuple(int(t) for t in z["levels_winner"][k])
        check_table(tables.cpu().numpy()[::-1][k], z["levels_table"][k], pyr[k][0].size, f"{name} chain level {k}")
    # float64 images give the same answer (the float32 values are read as float64 either way)
    assert compute_shift(gu.double(), gv.double(), scaling=True)[:2] == (dx, dy)


@pytest.mark.parametrize("irange", [0, 3, 8])
def test_other_search_radii(dev, irange):
    """irange is a run-time argument: 0 (one shift), 3, and 8 (289 shifts: three rounds of 128 lanes)."""
    from eogs2_amd.dsm_eval import ncc_search

    u, v = C.shifted_pair(70, 93, (-2, 3), seed=41, extra=(1, 4))
    ref = C.ncc_table(u, v, irange, 1, -1)
    dx, dy, table = ncc_search(torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev), irange, 1, -1)
    check_table(table.cpu().numpy(), ref, u.size, f"irange {irange}")
    assert (dx, dy) == C.argmax_scan(ref, irange, 1, -1)


def test_no_finite_pair_raises(dev):
    from eogs2_amd.dsm_eval import compute_shift, ncc_search

    u = torch.full((30, 40), float("nan"), device=dev)
    v = torch.ones((30, 40), device=dev)
    with pytest.raises(ValueError, match="finite NCC"):
        ncc_search(u, v)
    with pytest.raises(ValueError, match="finite NCC"):
        compute_shift(u, v)
    # a centre that moves the overlap out of the image: every candidate is NaN
    with pytest.raises(ValueError, match="finite NCC"):
        ncc_search(v, v, 5, 100, 0)
    res, table = c_ncc(dev, v, v, 5, 100, 0)
    assert int(res["valid"]) == 0 and (int(res["dx"]), int(res["dy"])) == (100, 0) and np.isnan(table).all()


def mae_tol(z, gt_key="gt", pred_r_key="pred_r"):
    return C.diff_tol(z[gt_key], z["pred"], z[pred_r_key])


def test_mae_plain(dev):
    from eogs2_amd.dsm_eval import dsm_mae, dsm_pointwise_diff

    z = load("mae_plain")
    pred, gt = torch.from_numpy(z["pred"]).to(dev), torch.from_numpy(z["gt"]).to(dev)
    mae, diff, pred_r, tr = dsm_mae(pred, gt)
    assert tr[:3] == (int(z["transform"][0]), int(z["transform"][1]), 1)
    assert abs(tr[3] - z["transform"][3]) <= C.b_bound(z["gt"], z["pred"])
    diff, pred_r = diff.cpu().numpy(), pred_r.cpu().numpy()
    assert diff.dtype == z["diff"].dtype and diff.shape == z["diff"].shape and pred_r.shape == z["pred_r"].shape
    assert np.array_equal(np.isnan(diff), np.isnan(z["diff"])) and np.array_equal(np.isnan(pred_r), np.isnan(z["pred_r"]))
    tol = mae_tol(z)
    print("mae_plain: max |pred_r - ref|", np.nanmax(np.abs(pred_r.astype(np.float64) - z["pred_r"])), "max |diff - ref|",
          np.nanmax(np.abs(diff.astype(np.float64) - z["diff"])), "tol", tol)
    assert np.nanmax(np.abs(pred_r.astype(np.float64) - z["pred_r"])) <= tol
    assert np.nanmax(np.abs(diff.astype(np.float64) - z["diff"])) <= tol
    lo, hi = np.nanmin(z["gt"]) - np.float32(10), np.nanmax(z["gt"]) + np.float32(10)
    assert (pred_r == lo).any() and (pred_r == hi).any()  # the clip is active, at the reference's float32 bounds
    check_mae(mae, z["mae"], z["diff"], z["gt"].size, "mae_plain")
    d2, p2 = dsm_pointwise_diff(pred, gt)
    assert same_bits(d2.cpu().numpy(), diff) and same_bits(p2.cpu().numpy(), pred_r)
    # the fused clip + crop + diff + sum through its C-ABI entry, on the workspace its size query names
    from eogs2_amd import _lib
    from eogs2_amd.dsm_eval import apply_shift

    abi = _lib.get()
    nb = ctypes.c_size_t()
    abi.check(abi.tsdf_dsm_mae_bytes(ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    shifted = apply_shift(pred, *tr)
    cdiff = torch.empty_like(d2)
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    abi.check(abi.tsdf_dsm_mae(pred.shape[0], pred.shape[1], p(shifted), gt.shape[0], gt.shape[1], p(gt), 0, 0, p(cdiff), p(out),
                               p(ws), ws.numel(), stream()))
    total, count, clo, chi = out.tolist()
    assert same_bits(cdiff.cpu().numpy(), diff) and same_bits(shifted.cpu().numpy(), pred_r)
    assert total / count == mae and count == np.count_nonzero(~np.isnan(diff)) and (clo, chi) == (float(lo), float(hi))
    # float64 images: the same registration, a float64 diff
    mae64, diff64, _, _ = dsm_mae(pred.double(), gt.double())
    assert diff64.dtype == torch.float64 and abs(mae64 - mae) <= 1e-4


def test_mae_gt_nan(dev):
    from eogs2_amd.dsm_eval import dsm_mae, dsm_pointwise_diff

    z = load("mae_gt_nan")
    pred, gt = torch.from_numpy(z["pred"]).to(dev), torch.from_numpy(z["gt"]).to(dev)
    diff, pred_r = dsm_pointwise_diff(pred, gt)
    assert torch.isnan(diff).all() and torch.isnan(pred_r).all() and np.isnan(z["diff"]).all() and np.isnan(z["pred_r"]).all()
    with pytest.raises(ValueError, match="NaN"):
        dsm_mae(pred, gt)
    mae, diff, pred_r, _ = dsm_mae(pred, gt, clip="finite")
    diff, pred_r = diff.cpu().numpy(), pred_r.cpu().numpy()
    assert np.array_equal(np.isnan(diff), np.isnan(z["ours_finite_diff"]))
    assert np.array_equal(np.isnan(pred_r), np.isnan(z["ours_finite_pred_r"]))
    assert np.nanmax(np.abs(diff.astype(np.float64) - z["ours_finite_diff"])) <= mae_tol(z, "gt", "ours_finite_pred_r")
    check_mae(mae, z["ours_finite_mae"], z["ours_finite_diff"], z["gt"].size, "mae_gt_nan finite")


def test_mae_masks(dev):
    from eogs2_amd.dsm_eval import dsm_mae, mask_dsm

    z = load("mae_masks")
    t = lambda k: torch.from_numpy(z[k]).to(dev)  # noqa: E731
    masked = mask_dsm(t("gt"), t("water"), t("vis"), t("tree"))
    assert same_bits(masked.cpu().numpy(), z["masked"])
    assert same_bits(mask_dsm(t("gt"), t("water"), None, None).cpu().numpy(), z["only_water"])
    with pytest.raises(ValueError, match="NaN"):  # the reference's bounds on a masked ground truth
        dsm_mae(t("pred"), masked)
    mae, diff, _, _ = dsm_mae(t("pred"), masked, clip="finite")
    diff = diff.cpu().numpy()
    assert np.array_equal(np.isnan(diff), np.isnan(z["ours_finite_diff"]))
    assert np.nanmax(np.abs(diff.astype(np.float64) - z["ours_finite_diff"])) <= mae_tol(z, "masked", "ours_finite_pred_r")
    check_mae(mae, z["ours_finite_mae"], z["ours_finite_diff"], z["masked"].size, "mae_masks finite")


def test_deterministic_across_runs_and_streams(dev):
    from eogs2_amd.dsm_eval import compute_shift_device

    u, v = C.shifted_pair(333, 410, (6, -4), seed=51, extra=(2, 1))
    gu, gv = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    runs = []
    for _ in range(2):
        results, tables = compute_shift_device(gu, gv)
        runs.append((results.cpu().numpy().tobytes(), tables.cpu().numpy().tobytes()))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        results, tables = compute_shift_device(gu, gv)
    side.synchronize()
    runs.append((results.cpu().numpy().tobytes(), tables.cpu().numpy().tobytes()))
    assert runs[0] == runs[1] == runs[2]
    assert not np.isnan(np.frombuffer(runs[0][1])).all()


@pytest.mark.parametrize("shape,extra,shift", [((1024, 1024), (0, 0), (9, -13)), ((2048, 1536), (5, 3), (-21, 30))])
def test_large_against_the_restatement(dev, shape, extra, shift):
    """Five pyramid levels (the coarsest 64 x 64 resp. 128 x 96); shifts beyond irange at full resolution; v larger than u."""
    from eogs2_amd.dsm_eval import compute_shift, compute_shift_device, dsm_mae, read_results

    u, v = C.shifted_pair(*shape, shift, seed=61, extra=extra)
    gu, gv = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    rec = []
    rdx, rdy, ra, rb = C.compute_shift(u, v, scaling=True, record=rec)
    assert (rdx, rdy) == shift and len(rec) == len(C.level_shapes(*u.shape, *v.shape)) == 5
    results, tables = compute_shift_device(gu, gv)
    r, tables = read_results(results)[::-1], tables.cpu().numpy()[::-1]
    for k, lv in enumerate(rec):
        n = lv["shape_u"][0] * lv["shape_u"][1]
        gap = np.sort(lv["table"][np.isfinite(lv["table"])])[-2:]
        assert gap[1] - gap[0] >= 1e-6  # the condition under which (dx, dy) is demanded exactly
        check_table(tables[k], lv["table"], n, f"{shape} level {lv['shape_u']}")
        assert (int(r[k]["dx"]), int(r[k]["dy"])) == lv["winner"]
    dx, dy, a, b = compute_shift(gu, gv, scaling=True)
    e = C.eps(u.size)
    _, muu, muv, sigu, sigv, xcorr = C.mean_std(u, v, rdx, rdy)
    top = r[-1]
    print(f"{shape}: eps {e:.3e} da/a {abs(a - ra) / ra:.3e} db {abs(b - rb):.3e} dsigu/sigu {abs(top['sigu'] - sigu) / sigu:.3e} "
          f"dxcorr {abs(top['xcorr'] - xcorr):.3e}")
    assert (dx, dy) == shift and abs(a - ra) <= e * ra and abs(b - rb) <= e * (abs(muu) + abs(muv))
    assert abs(top["muu"] - muu) <= e * abs(muu) and abs(top["muv"] - muv) <= e * abs(muv)
    assert abs(top["sigu"] - sigu) <= e * sigu and abs(top["sigv"] - sigv) <= e * sigv
    assert abs(top["xcorr"] - xcorr) <= e * sigu * sigv
    if shape[0] == 1024:  # the score of the same pair, with the finite bounds (5 % of the ground truth is NaN)
        rdiff, _, _ = C.dsm_pointwise_diff(v, u, clip="finite")
        mae, diff, _, tr = dsm_mae(gv, gu, clip="finite")
        assert tr[:2] == shift and np.array_equal(np.isnan(diff.cpu().numpy()), np.isnan(rdiff))
        rmae = C.mae_of(rdiff)
        print(f"{shape}: mae {mae!r} restatement {rmae!r} |d| {abs(mae - rmae):.3e} bound {e * rmae:.3e}")
        assert abs(mae - rmae) <= e * rmae


def test_chain_is_capturable_in_a_graph(dev):
    """compute_shift's device work has no host wait between pyramid levels: it records into a HIP graph on the library's
    documented workspace (eogs_tsdf_dsm_shift_bytes) and the replay on new image contents gives eager's answer."""
    from eogs2_amd import _lib
    from eogs2_amd.dsm_eval import RESULT_DTYPE, compute_shift_device, read_results

    abi = _lib.get()
    H, W, irange, n = 260, 300, 5, 11
    pairs = [C.shifted_pair(H, W, s, seed=70 + k) for k, s in enumerate([(8, -6), (-7, 11)])]
    gu, gv = torch.empty((H, W), device=dev), torch.empty((H, W), device=dev)
    nb, lv = ctypes.c_size_t(), ctypes.c_int()
    abi.check(abi.tsdf_dsm_shift_bytes(H, W, H, W, irange, ctypes.byref(nb), ctypes.byref(lv)))
    assert lv.value == 3
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    results = torch.zeros(lv.value * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    tables = torch.zeros((lv.value, n, n), dtype=torch.float64, device=dev)

    def enqueue():
        abi.check(abi.tsdf_dsm_shift(H, W, p(gu), H, W, p(gv), 0, irange, p(tables), p(results), p(ws), ws.numel(), stream()))

    gu.copy_(torch.from_numpy(pairs[0][0]))
    gv.copy_(torch.from_numpy(pairs[0][1]))
    enqueue()  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    for (u, v), shift in zip(pairs[::-1], [(-7, 11), (8, -6)]):
        gu.copy_(torch.from_numpy(u))
        gv.copy_(torch.from_numpy(v))
        results.zero_()
        tables.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = (results.cpu().numpy().tobytes(), tables.cpu().numpy().tobytes())
        assert (int(read_results(results)[0]["dx"]), int(read_results(results)[0]["dy"])) == shift
        er, et = compute_shift_device(gu, gv)
        assert got == (er.cpu().numpy().tobytes(), et.cpu().numpy().tobytes())


def test_compute_shift_device_is_capturable(dev):
    """The Python entry itself under torch.cuda.graph: one call on the capture stream first (it allocates the workspace of
    this shape and stream), then the capture allocates nothing and the replay refills the buffers the call returned."""
    from eogs2_amd.dsm_eval import clear_workspaces, compute_shift, compute_shift_device, read_results

    H, W = 230, 270
    pairs = [C.shifted_pair(H, W, s, seed=80 + k) for k, s in enumerate([(5, 9), (-10, -4)])]
    gu, gv = torch.from_numpy(pairs[0][0]).to(dev), torch.from_numpy(pairs[0][1]).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    from eogs2_amd import dsm_eval

    with torch.cuda.stream(side):
        warm, _ = compute_shift_device(gu, gv)
    side.synchronize()
    cached = len(dsm_eval._ws_cache)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        results, tables = compute_shift_device(gu, gv)
    assert len(dsm_eval._ws_cache) == cached and results.data_ptr() == warm.data_ptr()  # the cached workspace was found
    for (u, v), shift in zip(pairs[::-1], [(-10, -4), (5, 9)]):
        gu.copy_(torch.from_numpy(u))
        gv.copy_(torch.from_numpy(v))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        r = read_results(results)[0]
        assert (int(r["dx"]), int(r["dy"])) == shift
        got = (results.cpu().numpy().tobytes(), tables.cpu().numpy().tobytes())
        er, et = compute_shift_device(gu, gv)  # eager, on the default stream: other buffers
        assert er.data_ptr() != results.data_ptr()
        assert got == (er.cpu().numpy().tobytes(), et.cpu().numpy().tobytes())
        assert compute_shift(gu, gv)[:2] == shift
    del graph
    clear_workspaces()
    assert compute_shift(gu, gv)[:2] == (5, 9)  # allocated again


def test_capi_argument_checks(dev):
    from eogs2_amd import _lib

    abi = _lib.get()
    u = torch.ones((20, 30), device=dev)
    small = torch.ones((19, 30), device=dev)
    res = torch.zeros(72, dtype=torch.uint8, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    s = stream()
    assert abi.tsdf_dsm_ncc(20, 30, p(u), 19, 30, p(small), 0, 5, None, 1, None, p(res), p(ws), ws.numel(), s) == -1
    assert b"smaller" in abi.cdll.eogs_rast_last_error()
    assert abi.tsdf_dsm_ncc(20, 30, p(u), 20, 30, p(u), 0, 9, None, 1, None, p(res), p(ws), ws.numel(), s) == -1
    assert abi.tsdf_dsm_ncc(20, 30, p(u), 20, 30, p(u), 0, 5, None, 1, None, p(res), p(ws), 16, s) == -3
    assert abi.tsdf_dsm_ncc(20, 30, None, 20, 30, p(u), 0, 5, None, 1, None, p(res), p(ws), ws.numel(), s) == -1
    assert abi.tsdf_dsm_shift(20, 30, p(u), 20, 30, p(u), 0, 5, None, None, p(ws), ws.numel(), s) == -1
    assert abi.tsdf_dsm_apply_shift(20, 30, p(u), 0, 0, 0, 1.0, 0.0, 0.0, 0.0, p(u), s) == -1  # aliased
    assert abi.tsdf_dsm_mae(20, 30, p(u), 20, 30, p(u), 0, 0, None, p(res), p(ws), ws.numel(), s) == -1
    assert abi.tsdf_dsm_downsample(0, 30, p(u), 0, p(res), s) == -1
    abi.check(abi.tsdf_dsm_ncc(20, 30, p(u), 20, 30, p(u), 0, 5, None, 1, None, p(res), p(ws), ws.numel(), s))  # NULL centre, NULL table
    torch.cuda.synchronize()
