"""GPU: the kernels of the report module (eogs2_amd.report, csrc/report.hip) against float64 formulas, numpy's rules and the
reference's recorded results (tests/golden/report, written by tests/golden/make_golden_report.py): the colour alignment's
row and camera kernels, the train -> test converters, the report metrics and the product packing."""
import numpy as np
import pytest
import torch

import report_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- colour alignment ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aligned(dev):
    """Every fixture case through normalize_colors_ at its own row count: {name: (inputs, fixture, f_dc', weights', biases')}."""
    from eogs2_amd.report import normalize_colors_

    out = {}
    for case in RC.align_cases():
        d, z = RC.align_inputs(case), RC.load_fixture(f"align_{case['name']}")
        assert RC.sha(d["f_dc"]) == str(z["f_dc_sha"]) and np.array_equal(d["weights"], z["weights"]) and int(z["ref"]) == d["ref"]
        f = t(d["f_dc"], dev)
        ws, bs = [t(w, dev) for w in d["weights"]], [t(b, dev) for b in d["biases"]]
        normalize_colors_(f, ws[d["ref"]], bs[d["ref"]], ws, bs)
        out[case["name"]] = (d, z, f.cpu().numpy(), np.stack([w.cpu().numpy() for w in ws]), np.stack([b.cpu().numpy() for b in bs]))
    return out


def test_rows_within_eight_roundings_of_float64(aligned):
    for name, (d, z, f_out, _, _) in aligned.items():
        f64, bound = RC.rows_float64(d["f_dc"], d["weights"][d["ref"]], d["biases"][d["ref"]])
        err = np.abs(f_out.astype(np.float64) - f64) / bound * 8
        print(f"{name}: rows reach {err.max():.2f} of 8 roundings; the reference's fixture {(np.abs(z['f_dc_out'] - f64) / bound * 8).max():.2f}")
        assert f_out.shape == d["f_dc"].shape and np.all(np.abs(f_out.astype(np.float64) - f64) <= bound), name
        assert np.all(np.abs(z["f_dc_out"].astype(np.float64) - f64) <= bound), name  # the reference's own fp32 result, same bound


@pytest.mark.parametrize("P", RC.ROW_COUNTS)
def test_rows_at_every_count_and_alignment(dev, aligned, P):
    """The first P rows of the 4099-row cases: the vector body, its tail, one lane, more than one workgroup; and the same rows
    from a base that is only 4-byte aligned (the float-by-float path). A row's result does not depend on its place: the same
    bits as in the full run. The rows after the P-th keep theirs."""
    from eogs2_amd.report import normalize_colors_

    for case in RC.align_cases():
        if case["P"] != RC.ROW_COUNTS[-1]:
            continue
        d, _, full, _, _ = aligned[case["name"]]
        A1, b1 = t(d["weights"][d["ref"]], dev), t(d["biases"][d["ref"]], dev)
        for shift in (0, 1):
            buf = torch.full((shift + 3 * (P + 2),), 7.25, device=dev)
            view = buf[shift:shift + 3 * P].view(P, 1, 3)
            view.copy_(t(d["f_dc"][:P], dev))
            normalize_colors_(view, A1, b1, [], [])
            got = buf.cpu().numpy()
            assert got[shift:shift + 3 * P].tobytes() == full[:P].tobytes(), (case["name"], P, shift)
            assert np.all(got[:shift] == 7.25) and np.all(got[shift + 3 * P:] == 7.25)


def test_recomposed_corrections(aligned):
    for name, (d, z, _, w_out, b_out) in aligned.items():
        ref = d["ref"]
        A1, b1 = d["weights"][ref], d["biases"][ref]
        colours = d["f_dc"].reshape(-1, 3).astype(np.float64) * np.float64(RC.C0) + 0.5
        for v in range(RC.N_CAMERAS):
            R, rb, magA, magb = RC.recompose_float64(d["weights"][v], d["biases"][v], A1, b1)
            # ours: float64 rounded once
            assert np.all(np.abs(w_out[v].reshape(3, 3).astype(np.float64) - R) <= RC.ulp32(R) + RC.F64_NOISE * magA), (name, v)
            assert np.all(np.abs(b_out[v].astype(np.float64) - rb) <= RC.ulp32(rb) + RC.F64_NOISE * magb), (name, v)
            # the reference's recorded fp32 values: eight roundings of the terms' size
            assert np.all(np.abs(z["weights_out"][v].reshape(3, 3).astype(np.float64) - R) <= 8 * RC.U * magA), (name, v)
            assert np.all(np.abs(z["biases_out"][v].astype(np.float64) - rb) <= 8 * RC.U * magb), (name, v)
            # what matters: Ai' (A1 c + b1) + bi' = Ai c + bi at every fixture colour. With dA = Ai' - Ai inv(A1) and db alike the
            # two sides differ by dA (A1 c + b1) + db: |dA| <= eps magA, |db| <= eps magb, eps = 2^-23 for one ulp, 8 x 2^-24 for
            # the reference's eight roundings
            A64, b64 = d["weights"][v].reshape(3, 3).astype(np.float64), d["biases"][v].astype(np.float64)
            mapped = colours @ A1.reshape(3, 3).astype(np.float64).T + b1.astype(np.float64)
            want = colours @ A64.T + b64
            for eps, Wn, bn in ((2.0 ** -23, w_out[v], b_out[v]), (8 * RC.U, z["weights_out"][v], z["biases_out"][v])):
                got = mapped @ Wn.reshape(3, 3).astype(np.float64).T + bn.astype(np.float64)
                bound = (eps + RC.F64_NOISE) * (np.abs(mapped) @ magA.T + magb)
                assert np.all(np.abs(got - want) <= bound), (name, v, eps)


def test_alignment_keeps_the_parameter_and_its_adam_state(dev):
    from eogs2_amd.report import normalize_before_saving
    import types

    case = RC.align_cases()[4]
    d = RC.align_inputs(case)
    convs = []
    for v in range(RC.N_CAMERAS):
        conv = torch.nn.Conv2d(3, 3, 1, bias=True).to(dev)
        with torch.no_grad():
            conv.weight.copy_(t(d["weights"][v], dev))
            conv.bias.copy_(t(d["biases"][v], dev))
        convs.append(conv)
    views = [types.SimpleNamespace(is_reference_camera=(v == d["ref"]), get_msi_cameras=lambda c=c: types.SimpleNamespace(color_correction=c))
             for v, c in enumerate(convs)]
    scene = types.SimpleNamespace(getTrainCameras=lambda: views)
    g = types.SimpleNamespace(_features_dc=torch.nn.Parameter(t(d["f_dc"], dev)))
    opt = torch.optim.Adam([g._features_dc] + [p for c in convs for p in c.parameters()], lr=1e-3)
    g._features_dc.grad = torch.ones_like(g._features_dc)
    for c in convs:
        c.weight.grad, c.bias.grad = torch.ones_like(c.weight), torch.ones_like(c.bias)
    opt.step()
    before = g._features_dc.detach().cpu().numpy().copy()
    w_before = [c.weight.detach().cpu().numpy().copy() for c in convs]
    b_before = [c.bias.detach().cpu().numpy().copy() for c in convs]
    param, ptr = g._features_dc, g._features_dc.data_ptr()
    state = opt.state[param]
    m1, m2 = state["exp_avg"].clone(), state["exp_avg_sq"].clone()
    cam_ids = [(id(c.weight), c.weight.data_ptr(), id(c.bias), c.bias.data_ptr()) for c in convs]
    normalize_before_saving(scene, g)
    assert g._features_dc is param and isinstance(param, torch.nn.Parameter) and param.data_ptr() == ptr and param.requires_grad
    assert opt.state[param] is state and torch.equal(state["exp_avg"], m1) and torch.equal(state["exp_avg_sq"], m2)
    assert cam_ids == [(id(c.weight), c.weight.data_ptr(), id(c.bias), c.bias.data_ptr()) for c in convs]
    f64, bound = RC.rows_float64(before, w_before[d["ref"]], b_before[d["ref"]])
    assert np.all(np.abs(param.detach().cpu().numpy().astype(np.float64) - f64) <= bound)
    for v, c in enumerate(convs):  # every camera against the ORIGINAL A1 and b1, the reference camera included
        R, rb, magA, magb = RC.recompose_float64(w_before[v], b_before[v], w_before[d["ref"]], b_before[d["ref"]])
        assert np.all(np.abs(c.weight.detach().cpu().numpy().reshape(3, 3) - R) <= RC.ulp32(R) + RC.F64_NOISE * magA), v
        assert np.all(np.abs(c.bias.detach().cpu().numpy() - rb) <= RC.ulp32(rb) + RC.F64_NOISE * magb), v


def test_singular_reference_gives_nan_corrections(dev):
    from eogs2_amd.report import normalize_colors_

    for name, A1 in RC.SINGULAR:
        f = torch.zeros(4, 1, 3, device=dev)
        w, b = torch.eye(3, device=dev).reshape(3, 3, 1, 1).contiguous(), torch.ones(3, device=dev)
        normalize_colors_(f, t(A1, dev), torch.zeros(3, device=dev), [w], [b])
        assert bool(torch.isnan(w).all()) and bool(torch.isnan(b).all()), name


# ---- converters -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ref", "average"])
def test_converters_reproduce_the_reference_bit_for_bit(dev, name):
    import types

    from eogs2_amd.report import load_convert_color_correction_train_to_test

    d, z = RC.convert_inputs(), RC.load_fixture("convert")
    assert int(z["ref"]) == d["ref"]

    def cams(kind, prefix, is_ref_at=None):
        w, b = d[kind][prefix + "weights"], d[kind][prefix + "biases"]
        assert np.array_equal(w, z[f"in_{kind}_{prefix}weights"]) and w.tobytes() == z[f"in_{kind}_{prefix}weights"].tobytes()
        out = []
        for v in range(w.shape[0]):
            conv = types.SimpleNamespace(weight=torch.nn.Parameter(t(w[v], dev)), bias=torch.nn.Parameter(t(b[v], dev)))
            out.append(types.SimpleNamespace(color_correction=conv, is_reference_camera=(v == is_ref_at)))
        return out

    lists = {k: (cams(k, "", d["ref"]), cams(k, "test_")) for k in ("msi", "pan")}
    train = [types.SimpleNamespace(get_msi_cameras=lambda m=m: m, get_pan_cameras=lambda p=p: p) for m, p in zip(lists["msi"][0], lists["pan"][0])]
    test = [types.SimpleNamespace(get_msi_cameras=lambda m=m: m, get_pan_cameras=lambda p=p: p) for m, p in zip(lists["msi"][1], lists["pan"][1])]
    kept = [(c.color_correction.weight, c.color_correction.weight.data_ptr(), c.color_correction.bias) for k in lists for c in lists[k][1]]
    train_before = [c.color_correction.weight.detach().clone() for k in lists for c in lists[k][0]]
    got = load_convert_color_correction_train_to_test(name).perform_cc_to_test(train, test, types.SimpleNamespace(load_msi=True, load_pan=True))
    assert got is test
    for kind in ("msi", "pan"):
        for v, c in enumerate(lists[kind][1]):
            assert c.color_correction.weight.detach().cpu().numpy().tobytes() == z[f"{name}_{kind}_weights"][v].tobytes(), (kind, v)
            assert c.color_correction.bias.detach().cpu().numpy().tobytes() == z[f"{name}_{kind}_biases"][v].tobytes(), (kind, v)
    # the test cameras keep their parameter objects and storage; the train cameras are only read
    assert kept == [(c.color_correction.weight, c.color_correction.weight.data_ptr(), c.color_correction.bias) for k in lists for c in lists[k][1]]
    assert all(torch.equal(a, c.color_correction.weight) for a, c in zip(train_before, [c for k in lists for c in lists[k][0]]))


# ---- report metrics ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def metrics(dev):
    """Every case through one accumulator, in order: {(shape, content): (L1, PSNR) of the view as fp32}, the table after every
    view, and the kinds they went to."""
    from eogs2_amd.report import ReportAccumulator

    acc = ReportAccumulator(dev)
    acc.reset()
    z = RC.load_fixture("metrics")
    per_view, tables, kinds = {}, [], []
    for i, (shape, content) in enumerate(RC.metric_cases()):
        image, gt = RC.metric_inputs(shape, content)
        assert RC.sha(image, gt) == str(z[RC.metric_name(shape, content) + "_sha"])
        kind = ("msi", "pan")[i % 2]
        acc.accumulate(t(image, dev), t(gt, dev), kind)
        r = acc.read()
        per_view[(shape, content)] = tuple(np.float32(v) for v in r["last"])
        tables.append(r)
        kinds.append(kind)
    return z, per_view, tables, kinds


@pytest.mark.parametrize("shape,content", RC.metric_cases(), ids=[RC.metric_name(*c) for c in RC.metric_cases()])
def test_per_view_metrics(metrics, shape, content):
    z, per_view, _, _ = metrics
    image, gt = RC.metric_inputs(shape, content)
    l1_64, psnr_64 = RC.metrics_float64(image, gt)
    l1, psnr = per_view[(shape, content)]
    name = RC.metric_name(shape, content)
    r_l1, r_psnr = float(z[name + "_l1"]), float(z[name + "_psnr"])
    print(f"{name}: L1 {l1!r} PSNR {psnr!r}; float64 {l1_64!r} {psnr_64!r}; the reference's fp32 {r_l1!r} {r_psnr!r}")
    if content == "equal":
        assert l1 == 0.0 and psnr == np.inf and r_psnr == np.inf
    if content == "nan":
        assert np.isnan(l1) and np.isnan(psnr) and np.isnan(r_l1) and np.isnan(r_psnr)
    # within one fp32 ulp of the float64 formulas over the fp32 inputs
    for ours, f64 in ((l1, l1_64), (psnr, psnr_64)):
        assert RC.close_or_same(ours, f64, 0.0 if not np.isfinite(f64) else float(RC.ulp32(f64)))
    # the reference's recorded fp32 values r: |r - ours| <= |r - f64| + ulp(f64)
    for ours, f64, r in ((l1, l1_64, r_l1), (psnr, psnr_64, r_psnr)):
        tol = 0.0 if not np.isfinite(f64) else abs(r - f64) + float(RC.ulp32(f64))
        assert RC.close_or_same(r, ours, tol), (ours, f64, r)


def test_table_is_the_double_sum_of_the_per_view_values(metrics):
    _, per_view, tables, kinds = metrics
    sums = {"l1": [0.0, 0.0], "psnr": [0.0, 0.0], "views": [0, 0]}
    bits = lambda v: np.float64(v).tobytes()  # noqa: E731  (NaN and inf included)
    for (key, r, kind) in zip(RC.metric_cases(), tables, kinds):
        k = ("pan", "msi").index(kind)
        with np.errstate(invalid="ignore"):
            sums["l1"][k] = float(np.float64(sums["l1"][k]) + np.float64(per_view[key][0]))
            sums["psnr"][k] = float(np.float64(sums["psnr"][k]) + np.float64(per_view[key][1]))
        sums["views"][k] += 1
        for m in ("l1", "psnr"):
            for j in range(2):
                a, b = r[m][j], sums[m][j]
                assert bits(a) == bits(b) or (np.isnan(a) and np.isnan(b)), (key, m, j, a, b)
        assert r["views"] == sums["views"]


def test_metrics_repeat_gate_graph_and_fetch(dev):
    from eogs2_amd.report import ReportAccumulator

    shapes = [((3, 7, 5), "random"), ((1, 257, 256), "gt_outside"), ((4, 64, 64), "random")]
    inputs = [tuple(t(a, dev) for a in RC.metric_inputs(s, c)) for s, c in shapes]

    def run(acc):
        acc.reset()
        for (img, gt), kind in zip(inputs, ("msi", "pan", "msi")):
            acc.accumulate(img, gt, kind)
        return acc.table.cpu().numpy().tobytes()

    a, b = ReportAccumulator(dev), ReportAccumulator(dev)
    first = run(a)
    assert first == run(b) == run(a)  # two runs, two accumulators: the same bits
    # a closed gate changes no word; an open one adds the view
    closed, opened = torch.tensor([0, 3], dtype=torch.int32, device=dev), torch.tensor([1, 0], dtype=torch.int32, device=dev)
    a.accumulate(*inputs[0], "pan", gate=closed)
    assert a.table.cpu().numpy().tobytes() == first
    a.accumulate(*inputs[0], "pan", gate=opened.view(torch.uint32))
    r = a.read()
    assert r["views"] == [2, 2] and a.table.cpu().numpy().tobytes() != first
    # fetch divides by the number of viewpoints, not by the cameras of the kind
    out = a.fetch(5)
    assert set(out) == {"l1", "psnr"} and set(out["l1"]) == set(out["psnr"]) == {"pan", "msi"}
    assert out["l1"]["pan"] == r["l1"][0] / 5 and out["l1"]["msi"] == r["l1"][1] / 5
    assert out["psnr"]["pan"] == r["psnr"][0] / 5 and out["psnr"]["msi"] == r["psnr"][1] / 5
    with pytest.raises(ValueError):
        a.fetch(0)
    # accumulate replays inside a single-stream graph: three replays after a reset equal three eager calls
    b.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        b.accumulate(*inputs[2], "msi")  # (warm-up on the side stream)
        b.reset()
        with torch.cuda.graph(graph, stream=side):
            b.accumulate(*inputs[2], "msi")
    torch.cuda.current_stream(dev).wait_stream(side)
    b.reset()
    for _ in range(3):
        graph.replay()
    a.reset()
    for _ in range(3):
        a.accumulate(*inputs[2], "msi")
    torch.cuda.synchronize()
    assert b.read()["views"] == [0, 3] and a.table.cpu().numpy().tobytes() == b.table.cpu().numpy().tobytes()


# ---- product packing ---------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (3, 5), (17, 33), (64, 65))
SENTINEL = 0xA5


def run_pack(dev, specs, total=None):
    """specs: [dict(src numpy, mode, offset, pitch, reverse, replicate, premap)] -> the buffer's bytes after one call over a
    sentinel-filled buffer, and the layout."""
    from eogs2_amd.report import PackItem, check_pack, pack_products

    items = [PackItem(t(s["src"], dev), s["mode"], s.get("offset"), s.get("pitch"), s.get("reverse", False), s.get("replicate", False),
                      s.get("premap")) for s in specs]
    _, need = check_pack(items)
    buf = torch.full((max(need, total or 0) + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    out, layout = pack_products(items, out=buf)
    assert out is buf
    return buf.cpu().numpy(), layout


def check_buffer(buf, layout, specs):
    """Every item's rectangle holds numpy's bytes; every other byte the sentinel."""
    touched = np.zeros(buf.size, dtype=bool)
    for (offset, pitch, (H, W, Co), dtype), s in zip(layout, specs):
        want = RC.expected_item(s["src"], s["mode"], s.get("reverse", False), s.get("replicate", False), s.get("premap"))
        assert want.shape == (H, W, Co) and want.dtype == dtype
        row = W * Co * want.itemsize
        for r in range(H):
            got = buf[offset + r * pitch: offset + r * pitch + row]
            if dtype == np.float32 and s.get("premap"):  # arithmetic on a NaN: which NaN comes out is nobody's rule
                g32, w32 = got.view(np.float32), want[r].reshape(-1)
                nan = np.isnan(w32)
                assert np.array_equal(np.isnan(g32), nan) and g32[~nan].tobytes() == w32[~nan].tobytes(), (s["mode"], s["src"].shape, r)
                touched[offset + r * pitch: offset + r * pitch + row] = True
                continue
            assert got.tobytes() == want[r].tobytes(), (s["mode"], s["src"].shape, r)
            touched[offset + r * pitch: offset + r * pitch + row] = True
    assert np.all(buf[~touched] == SENTINEL)


@pytest.mark.parametrize("mode", ["float", "u8_round", "u8_trunc"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_pack_one_item_every_channel_count(dev, mode, size):
    H, W = size
    for C in (1, 3, 4, 5):
        for reverse in (False, True):
            specs = [dict(src=RC.pack_source((C, H, W), 10 * C + H), mode=mode, reverse=reverse)]
            check_buffer(*run_pack(dev, specs), specs)
    for src in (RC.pack_source((1, H, W), 7), RC.pack_source((H, W), 8)):  # replicate, and a plane given as (H, W)
        specs = [dict(src=src, mode=mode, replicate=True)]
        check_buffer(*run_pack(dev, specs), specs)
    specs = [dict(src=RC.pack_source((H, W), 9), mode=mode)]
    check_buffer(*run_pack(dev, specs), specs)


def test_pack_sixteen_items_in_one_call(dev):
    specs = []
    for i in range(16):
        H, W = SIZES[i % 4]
        C = (1, 3, 4, 5)[(i // 4) % 4]
        specs.append(dict(src=RC.pack_source((C, H, W), 100 + i), mode=("float", "u8_round", "u8_trunc")[i % 3], reverse=bool(i & 1),
                          replicate=(C == 1 and i % 8 == 0)))
    check_buffer(*run_pack(dev, specs), specs)


def test_pack_two_items_side_by_side_with_the_premap(dev):
    """The video frame's layout, and bounds whose double difference is no fp32 number: 0.1 and 0.7 (0.7 - 0.1 in double is
    0.6 - 1.1e-16, which rounds to another fp32 than fp32(0.7) - fp32(0.1))."""
    lo, hi = 0.1, 0.7
    assert np.float32(hi - lo) != np.float32(hi) - np.float32(lo) and float(np.float32(hi - lo)) != hi - lo
    for H, W in SIZES:
        with np.errstate(invalid="ignore", over="ignore"):
            final, alt = RC.pack_source((3, H, W), 40 + H), (lo + (hi - lo) * RC.pack_source((H, W), 50 + H)).astype(np.float32)
        specs = [dict(src=final, mode="u8_trunc", offset=0, pitch=6 * W, reverse=True),
                 dict(src=alt, mode="u8_trunc", offset=3 * W, pitch=6 * W, replicate=True, premap=(lo, hi))]
        buf, layout = run_pack(dev, specs, total=6 * W * H)
        check_buffer(buf, layout, specs)
        specs = [dict(src=alt, mode="float", premap=(lo, hi)), dict(src=alt, mode="u8_round", premap=(lo, hi), replicate=True)]
        check_buffer(*run_pack(dev, specs), specs)


def test_video_frame(dev):
    from eogs2_amd.report import video_frame

    H, W, lo, hi = 17, 33, -3.3, 41.9
    with np.errstate(invalid="ignore", over="ignore"):
        alt = (lo + (hi - lo) * RC.pack_source((H, W), 3)).astype(np.float32)
    for C in (3, 1):
        final = RC.pack_source((C, H, W), 60 + C)
        frame = video_frame(t(final, dev), t(alt, dev), lo, hi)
        assert frame.dtype == torch.uint8 and tuple(frame.shape) == (H, 2 * W, 3)
        # render_video.py:138-164 in numpy: repeat a PAN plane, normalise the elevation, concatenate, clip, x 255, cast, RGB -> BGR
        rgb = np.repeat(final, 3, axis=0) if C == 1 else final
        image = np.concatenate([rgb, np.repeat(RC.premap(alt, lo, hi)[None], 3, axis=0)], axis=-1)
        want = RC.u8_trunc(np.transpose(image, (1, 2, 0)))[:, :, ::-1]
        assert np.array_equal(frame.cpu().numpy(), want)
