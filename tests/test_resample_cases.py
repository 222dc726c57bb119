"""CPU: the cases of tests/resample_cases.py themselves, so that a GPU test cannot pass for the wrong reason. For every case
the condition it guards is computed from its inputs (more output tiles than a scan round holds, a bucket that is full, every
box empty, ...), and the reference's own fp32 op sequence must lie within REF_TOL = 3e-5 of the float64 oracle under the
comparison rule of the case module, with at most 1 % of the pixels left out of dL/duva.

`python tests/test_resample_cases.py` writes the measured figures to profiles/resample_cases_cpu.json."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import resample_cases as RC


def _has_tap(case, x0, y0):
    Hv, Wv = case["vr"].shape[1:]
    return ((x0 >= -1) & (x0 < Wv)) & ((y0 >= -1) & (y0 < Hv))  # one of x0, x0 + 1 and one of y0, y0 + 1 is a cell


def test_the_constants_are_the_kernels():
    """OT, CHT, RB and the tile threshold as bucket_gather.h, resample.hip and flow.hip spell them."""
    import re

    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eogs2_amd", "csrc")
    h = open(os.path.join(src, "bucket_gather.h")).read()
    assert re.search(r"constexpr int OT = (\d+);", h).group(1) == str(RC.OT)
    assert re.search(r"constexpr int CHT = NACC == 1 \? (\d+) : (\d+);", h).groups() == (str(RC.CHT[1]), str(RC.CHT[4]))
    assert re.search(r"constexpr int RB = NACC == 1 \? (\d+) : (\d+);", h).groups() == (str(RC.RB[1]), str(RC.RB[4]))
    assert "constexpr int CAP = CHT * OT * OT;" in h
    for f in ("resample.hip", "flow.hip"):
        assert f"> {RC.BIG_CELLS};" in open(os.path.join(src, f)).read()


def test_every_case_is_named_with_its_guards():
    want = {"collapse_exact", "collapse_alt", "minify8", "rounds4", "rounds1", "big4", "big1", "partly_out", "all_out", "far", "edge_pm1",
            "half_cell", "thin_w", "thin_h", "one_tile", "one_past"}
    assert want <= set(RC.BASE_RESAMPLE)
    assert len(RC.CHANNEL_RESAMPLE) == 2 * len(RC.CHANNEL_MATRIX) == 16
    assert set(RC.FLOW) == {"flow_converge", "flow_converge_corner", "flow_big1", "flow_big3", "flow_big5", "flow_rounds1", "flow_strided"}
    for name in RC.RESAMPLE:
        c = RC.resample_case(name)
        assert c["guards"] and c["vr"].dtype == c["U"].dtype == c["alt"].dtype == torch.float32
        assert c["w_s"].shape == (c["n_out"],) + c["alt"].shape and -1 <= c["fill_channel"] < c["n_out"] <= c["vr"].shape[0]
    for name in RC.FLOW:
        c = RC.flow_case(name)
        assert c["guards"] and c["flow"].shape == (1, 2) + c["img"].shape[1:]
        assert float(c["flow"].abs().max()) <= 6 or name.startswith("flow_converge")
        assert torch.equal(c["flow"] * 8, (c["flow"] * 8).round())  # multiples of 1/8


@pytest.mark.parametrize("name", RC.BASE_RESAMPLE)
def test_resample_case_guards_what_it_says(name):
    c = RC.resample_case(name)
    (H, W), (C, Hv, Wv), n_out = c["alt"].shape, c["vr"].shape, c["n_out"]
    u, v, ix, iy = RC.pixel_coords(c)
    x0, y0 = RC.tap_cells(c)
    has = _has_tap(c, x0, y0)
    k = RC.nacc(n_out)
    shapes = {"collapse_exact": (64, 64, 40, 40), "collapse_alt": (64, 64, 40, 40), "minify8": (128, 160, 17, 33), "rounds4": (528, 512, 40, 40),
              "rounds1": (1040, 1024, 40, 40), "big4": (96, 112, 1025, 2049), "big1": (96, 112, 1025, 2049), "partly_out": (48, 48, 33, 65),
              "all_out": (40, 56, 40, 40), "far": (40, 40, 40, 40), "far_e12": (40, 40, 40, 40), "edge_pm1": (33, 65, 33, 65),
              "half_cell": (33, 65, 33, 65), "thin_w": (48, 48, 40, 1), "thin_h": (48, 48, 1, 40), "one_tile": (48, 48, 32, 32),
              "one_past": (48, 48, 33, 33)}
    assert (H, W, Hv, Wv) == shapes[name]
    if name in ("collapse_exact", "collapse_alt"):
        assert not c["M"][:2].any() or name == "collapse_alt"
        fill = RC.max_bucket_fill(x0, y0, has, Hv, Wv, n_out)
        if name == "collapse_exact":
            assert (ix == 19.5).all() and (iy == 19.5).all()
            assert fill == RC.CAP[k] == RC.CHT[k] * 256 and RC.output_tiles(H, W) % RC.CHT[k] == 0  # full in every chunk
        else:
            cells, counts = np.unique(y0 * Wv + x0, return_counts=True)
            assert 2 <= len(cells) <= 6 and counts.sum() == 4096 and fill >= 256
            assert float(RC.oracle_resample(name)["g_uva"][..., 2].abs().max()) > 0
    if name == "minify8":
        assert H * W / (Hv * Wv) > 30 and Wv % 32 and Hv % 32
        assert RC.max_bucket_fill(x0, y0, has, Hv, Wv, n_out) >= 10
    if name in ("rounds4", "rounds1"):
        assert RC.RB[k] < RC.output_tiles(H, W) <= 2 * RC.RB[k] and (k == 1) == (name == "rounds1")
        assert has.all()  # every output tile is a candidate of the one virtual tile
        if name == "rounds1":
            assert RC.output_tiles(H, W) >= 4096 + 1 and (C, n_out, c["fill_channel"]) == (1, 1, 0)
    if name in ("big4", "big1"):
        assert Hv * Wv > 1_500_000 and RC.virtual_tile(Hv, Wv) == (64, 32) and n_out == (4 if name == "big4" else 1)
        assert RC.reached_cells(x0, y0, Hv, Wv, dilate=1).mean() < 0.1  # most cells receive nothing
    if name == "partly_out":
        assert ((ix > -1) & (ix < 0)).any() and ((iy > -1) & (iy < 0)).any()  # x0 = -1, y0 = -1
        assert (x0 == -1).any() and (y0 == -1).any() and (np.abs(u) > 1).any() and c["fill_channel"] == 3
    if name == "all_out":
        assert not has.any()  # every box is empty
    if name == "all_out":
        assert u.min() > 1.5 and u.max() < 3 and v.min() > 1.5 and v.max() < 3
        ref = RC.oracle_resample(name)
        assert not ref["g_virtual"].any() and (ref["sample"][3] == -100).all() and not ref["sample"][:3].any()
    if name in ("far", "far_e12"):
        big = np.abs(ix).max()
        assert big > (2.0 ** 31 if name == "far_e12" else 1e7)
        reached = RC.reached_cells(x0, y0, Hv, Wv, dilate=0)
        centre = np.zeros_like(reached)
        centre[19:21, :] = centre[:, 19:21] = True
        assert not (reached & ~centre).any()
        assert has.sum() == 1 and reached.sum() == 4  # the one pixel where both coordinates are 0
    if name == "edge_pm1":
        uva = torch.stack((c["U"], c["V"], c["alt"]), -1)
        uv32 = torch.einsum("ij,hwj->hwi", c["M"], uva)[..., :2]  # fp32, as the kernel
        at_one = (uv32 == 1.0).any(-1)
        assert at_one.any() and not (uv32.abs() > 1)[at_one].any() and (uv32 == -1.0).any()
        assert (ix == np.round(ix)).all() and (iy == np.round(iy)).all() and (x0 == Wv - 1).any() and (y0 == Hv - 1).any()
    if name == "half_cell":
        assert (ix * 128 == np.round(ix * 128)).all() and (iy * 128 == np.round(iy * 128)).all()
        assert (ix != np.round(ix)).mean() > 0.9
    if name in ("thin_w", "thin_h"):
        assert (Wv if name == "thin_w" else Hv) == 1 and ((ix if name == "thin_w" else iy) == 0).all()
    if c["lattice"]:  # fp32 and float64 agree exactly on the coordinates
        uva = torch.stack((c["U"], c["V"], c["alt"]), -1)
        uv32 = torch.einsum("ij,hwj->hwi", c["M"], uva)[..., :2]
        assert np.array_equal(uv32[..., 0].double().numpy(), u) and np.array_equal(uv32[..., 1].double().numpy(), v)
        ix32 = (uv32[..., 0] + 1) * 0.5 * (Wv - 1)
        assert np.array_equal(ix32.double().numpy(), ix)
        for n in (Wv - 1, Hv - 1):
            assert (n & (n - 1)) == 0 or name == "collapse_exact"


@pytest.mark.parametrize("name", RC.FLOW)
def test_flow_case_guards_what_it_says(name):
    c = RC.flow_case(name)
    C, H, W = c["img"].shape
    x0, y0 = RC.flow_tap_cells(c["flow"])
    if name.startswith("flow_converge"):
        assert len(np.unique(y0 * W + x0)) == 1 and (x0[0, 0], y0[0, 0]) == ((40, 31) if name == "flow_converge" else (0, 0))
        k = RC.nacc(min(C, 4))
        assert RC.max_bucket_fill(x0, y0, np.ones_like(x0, dtype=bool), H, W, min(C, 4)) == RC.CHT[k] * 256 == RC.CAP[k]
    if name.startswith("flow_big"):
        assert H * W > 1_500_000 and RC.virtual_tile(H, W) == (64, 32) and C == int(name[-1])
    if name == "flow_rounds1":
        assert C == 1 and RC.RB[1] < RC.output_tiles(H, W) <= 2 * RC.RB[1] and H * W <= RC.BIG_CELLS
    if name in ("flow_rounds1", "flow_big1", "flow_big3", "flow_big5"):
        assert ((H - 1) & (H - 2)) == 0 and ((W - 1) & (W - 2)) == 0  # the reference's normalisation round trip is exact
    if name == "flow_strided":
        views = RC.strided_views(c["flow"])
        assert all(torch.equal(v, c["flow"]) and not v.is_contiguous() for v in views.values())


def _resample_reference_errors(name):
    c = RC.resample_case(name)
    got = RC.run_resample(RC.reference_resample_ops, c, torch.device("cpu"))
    return RC.resample_errors(got, RC.oracle_resample(name), c)


def _flow_reference_errors(name):
    c = RC.flow_case(name)
    return RC.flow_errors(RC.reference_flow_ops(c["img"], c["flow"], c["up"]), RC.oracle_flow(name))


@pytest.mark.parametrize("name", RC.RESAMPLE)
def test_reference_fp32_ops_hold_the_bar_alone_resample(name):
    err, frac = _resample_reference_errors(name)
    print(f"{name}: {err} left out {frac:.3%}")
    c = RC.resample_case(name)
    assert frac <= RC.MAX_LEFT_OUT and (frac == 0 or not c["lattice"])
    assert not c["vr"].requires_grad and c["vr"].grad is None  # the shared case is left as it was
    for k, e in err.items():
        assert e <= RC.REF_TOL, f"{name}: the reference's fp32 {k} is {e:.3e} of its maximum from float64 (bound {RC.REF_TOL:g})"


@pytest.mark.parametrize("name", RC.FLOW)
def test_reference_fp32_ops_hold_the_bar_alone_flow(name):
    err = _flow_reference_errors(name)
    print(f"{name}: {err}")
    for k, e in err.items():
        assert e <= RC.REF_TOL, f"{name}: the reference's fp32 {k} is {e:.3e} of its maximum from float64 (bound {RC.REF_TOL:g})"


def test_oracle_defaults_are_the_reference_statements():
    """n_keep / fill_channel of the oracle: the defaults still are `rgb, alt = s[:3], s[3]; alt[mask] = -100`."""
    from oracle import resample_oracle

    c = RC.resample_case("partly_out")
    uva = torch.stack((c["U"], c["V"], c["alt"]), -1)
    s, uv = resample_oracle.resample(c["vr"], c["M"], uva)
    raw = torch.nn.functional.grid_sample(c["vr"].double()[None], uv[None], align_corners=True)[0]
    out = (uv.abs() > 1).any(-1)
    assert 0 < int(out.sum()) < out.numel() and s.shape[0] == 4
    assert torch.equal(s[:3], raw[:3]) and (s[3][out] == -100).all() and torch.equal(s[3][~out], raw[3][~out])
    s5, _ = resample_oracle.resample(c["vr"], c["M"], uva, n_keep=5, fill_channel=-1)
    assert torch.equal(s5, raw)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (pytest gets the root from tests/conftest.py)
    out = {"bound": RC.REF_TOL, "max_left_out": RC.MAX_LEFT_OUT, "resample": {}, "flow": {}}
    for n in RC.RESAMPLE:
        err, frac = _resample_reference_errors(n)
        out["resample"][n] = dict({k: float(f"{e:.3e}") for k, e in err.items()}, left_out=round(frac, 5))
    for n in RC.FLOW:
        out["flow"][n] = {k: float(f"{e:.3e}") for k, e in _flow_reference_errors(n).items()}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample_cases_cpu.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1), file=sys.stderr)
