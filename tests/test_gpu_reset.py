"""GPU: the shadow-based colour reset and the in-place opacity reset (eogs2_amd.reset, include/eogs_reset.h) against the
reference's lines restated with torch ops on the CPU (tests/reset_cases.py): the erosion bit for bit, the flags equal to the
fp32 ones outside the float64 margin, the fills bit for bit with every tensor and address kept, the capped logits within one
ulp of the float64 formula, all of it recordable in one graph, render_all_views against its pieces called by hand, the
reference's color_reset end to end, and the example replaying one recording across both resets."""
import os
import sys

import pytest
import torch

import reset_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def erode_on_device(s, dev):
    """eogs_reset_erode alone (shadow_reset_flags keeps its eroded maps in a workspace of its own)."""
    from eogs2_amd import _lib
    from eogs2_amd._host import Ctx, ptr

    abi = _lib.get()
    src = s.to(dev)
    out = torch.full_like(src, -7.0)
    with Ctx(abi, dev) as cx:
        abi.check(abi.reset_erode(src.shape[0], src.shape[1], ptr(src), ptr(out), cx.stream))
    return out.cpu()


@pytest.mark.parametrize("H,W", RC.ERODE_SHAPES)
def test_erode_is_torchs_bits(dev, H, W):
    s = RC.erode_input(H, W)
    want = RC.erode_ref(s)
    got = erode_on_device(s, dev)
    assert RC.same_bits(got, want), f"{int((got != want).sum() - torch.isnan(want).sum())} pixels differ"
    plain = torch.rand(H, W, generator=torch.Generator().manual_seed(H + W))  # (a map without a NaN: every pixel is compared as bits)
    assert torch.equal(erode_on_device(plain, dev).view(torch.int32), RC.erode_ref(plain).view(torch.int32))


def device_views(views, dev):
    return [(s.to(dev), A.to(dev)) for s, A in views]


@pytest.mark.parametrize("n_views", sorted(RC.FLAG_VIEWS))
@pytest.mark.parametrize("P", RC.FLAG_P)
def test_flags_match_the_fp32_reference(dev, P, n_views):
    from eogs2_amd.reset import shadow_reset_flags

    xyz, opacity, views = RC.flags_case(P, n_views)
    got = shadow_reset_flags(xyz.to(dev), device_views(views, dev), opacity=opacity.to(dev))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (P,) and int(got.max()) <= 1
    RC.check_flags(got, xyz, views, opacity)
    # without the logits the retired rows are flagged like any other, and `out` is written in place, stale bytes overwritten
    out = torch.full((P,), 255, dtype=torch.uint8, device=dev)
    again = shadow_reset_flags(xyz.to(dev), device_views(views, dev), out=out)
    assert again is out and int(out.max()) <= 1
    RC.check_flags(out, xyz, views, None)
    assert int(out[0]) == 1 and int(got[0]) == 0  # row 0: far outside every view, retired


def test_flags_of_no_view_are_zero(dev):
    from eogs2_amd.reset import shadow_reset_flags

    out = torch.full((65,), 3, dtype=torch.uint8, device=dev)
    assert not shadow_reset_flags(torch.rand(65, 3, device=dev), [], out=out).any()
    assert shadow_reset_flags(torch.zeros(0, 3, device=dev), device_views(RC.flags_case(1, 1)[2], dev)).numel() == 0


def flag_patterns(P):
    alt = torch.zeros(P, dtype=torch.uint8)
    alt[::2] = 1
    return {"none": torch.zeros(P, dtype=torch.uint8), "all": torch.ones(P, dtype=torch.uint8), "alternate": alt}


@pytest.mark.parametrize("with_state", [True, False])
@pytest.mark.parametrize("pattern", ["none", "all", "alternate"])
@pytest.mark.parametrize("P", [1, 67, 259])
def test_color_reset_fills_in_place(dev, P, pattern, with_state):
    """Rows of width 1 (opacity) and 3 (f_dc [P,1,3], scaling); P no multiple of 64."""
    from eogs2_amd.reset import color_reset_

    opt = RC.make_optimizer(P, dev, seed=P, with_state=with_state)
    before, ids = RC.snapshot(opt), RC.identities(opt)
    flags = flag_patterns(P)[pattern]
    color_reset_(opt, flags.to(dev))
    RC.assert_snapshots_equal(RC.snapshot(opt), RC.color_reset_ref(before, flags))
    assert RC.identities(opt) == ids
    color_reset_(opt, flags.bool().to(dev))  # a bool mask is the same bytes; the reset is idempotent
    RC.assert_snapshots_equal(RC.snapshot(opt), RC.color_reset_ref(before, flags))


@pytest.mark.parametrize("with_state", [True, False])
@pytest.mark.parametrize("P", [1, 67, 1030])
def test_reset_opacity_in_place(dev, P, with_state):
    from eogs2_amd.reset import reset_opacity_

    opt = RC.make_optimizer(P, dev, seed=P, with_state=with_state)
    logits = RC.opacity_logits(P)
    by = {g["name"]: g["params"][0] for g in opt.param_groups}
    with torch.no_grad():
        by["opacity"].copy_(logits)
    before, ids = RC.snapshot(opt), RC.identities(opt)
    reset_opacity_(opt)
    after = RC.snapshot(opt)
    assert RC.identities(opt) == ids
    got = after["opacity"][0]
    want64 = RC.reset_opacity_ref64(logits)
    l = logits.squeeze(1)
    nan, retired = torch.isnan(l), l < -1e29
    assert torch.isnan(got.squeeze(1)[nan]).all()
    assert RC.same_bits(got.squeeze(1)[retired], l[retired])  # a retired row stays retired (the formula would give -inf)
    rest = ~nan & ~retired
    d = RC.ulp_distance(got.squeeze(1)[rest], want64.squeeze(1)[rest])
    print(f"P {P}: largest distance from the float64 formula {float(d.max()):.3f} ulp")
    assert float(d.max()) <= 1.0
    const = RC.reset_opacity_constant()
    above = rest & (l >= const.item())
    assert RC.same_bits(got.squeeze(1)[above], const.expand(int(above.sum())))
    if with_state:
        assert not after["opacity"][1].any() and not after["opacity"][2].any()
    want = {k: v for k, v in before.items()}
    want["opacity"] = after["opacity"][:3] + (before["opacity"][3],)
    RC.assert_snapshots_equal(after, want)  # every other group, its moments and every step: untouched


def test_the_resets_are_recordable(dev):
    """One linear graph of all three: nothing in them waits for the device, and a replay gives the eager results."""
    from eogs2_amd.reset import color_reset_, reset_opacity_, shadow_reset_flags

    P = 257
    xyz, opacity, views = RC.flags_case(P, 17)
    dxyz, dviews = xyz.to(dev), device_views(views, dev)

    def run(opt, flags):
        shadow_reset_flags(dxyz, dviews, opacity=opt.param_groups[3]["params"][0].detach().view(-1), out=flags)
        color_reset_(opt, flags)
        reset_opacity_(opt)

    def fresh():
        opt = RC.make_optimizer(P, dev, seed=5)
        with torch.no_grad():
            opt.param_groups[3]["params"][0].copy_(opacity.view(P, 1))
        return opt, torch.zeros(P, dtype=torch.uint8, device=dev)

    eager_opt, eager_flags = fresh()
    run(eager_opt, eager_flags)
    opt, flags = fresh()
    start = RC.snapshot(opt)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (warm-up on a side stream, torch.cuda.graph's own recipe: the workspace exists before the capture)
        shadow_reset_flags(dxyz, dviews, out=torch.zeros(P, dtype=torch.uint8, device=dev))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(opt, flags)
    RC.assert_snapshots_equal(RC.snapshot(opt), start)  # a capture runs nothing
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(flags, eager_flags) and 0 < int(flags.sum()) < P
    RC.assert_snapshots_equal(RC.snapshot(opt), RC.snapshot(eager_opt))


def pipe():
    import types

    return types.SimpleNamespace(debug=False, antialiasing=False, compute_cov3D_python=False, require_radii=False)


def test_render_all_views_is_its_pieces(dev):
    from eogs2_amd.render import render
    from eogs2_amd.resample import render_resample_virtual_camera
    from eogs2_amd.reset import render_all_views

    cams = RC.make_cameras(dev)
    model = RC.make_model(300, dev)
    bg = torch.tensor([0.2, 0.4, 0.6, 123.0, 0.7], device=dev)
    outs = render_all_views(cams, model, pipe(), bg=bg.clone())
    assert len(outs) == 2
    for cam, o in zip(cams, outs):
        assert sorted(o) == sorted(["image_name", "shadow", "raw_render", "cc", "render", "projxyz", "altitude_render"])
        H, W = cam.image_height, cam.image_width
        with torch.no_grad():
            b = bg.clone()
            b[3], b[4] = cam.altitude_bounds[0], 0.0
            pkg = render(cam, model, pipe(), b)["render"]
            uva = torch.stack(cam.UV_grid + (pkg[3],), dim=-1)
            sun, cam2sun = cam.get_sun_camera()
            _, sun_alt, _ = render_resample_virtual_camera(sun, cam2sun, uva, model, pipe(), b)
            piped = cam.render_pipeline(raw_render=pkg[:3], sun_altitude_diff=pkg[3] - sun_alt)
            proj = model.get_xyz @ cam.affine[:3, :2] + cam.affine[3, :2]
        assert o["image_name"] == cam.image_name and tuple(o["shadow"].shape) == (H, W)
        assert torch.equal(o["altitude_render"], pkg[3]) and torch.equal(o["raw_render"], pkg[:3])
        assert torch.equal(o["shadow"], piped["shadowmap"]) and torch.equal(o["cc"], piped["cc"]) and torch.equal(o["render"], piped["final"])
        assert torch.equal(o["projxyz"], proj)
        # the pieces would differ had the background kept its altitude or its constant channel, the difference the other sign,
        # or the projection come from the (shifted) world-to-view matrix
        assert 0.0 < float(o["shadow"].min()) < 0.999 and float(o["shadow"].max()) <= 1.0
        assert not torch.equal(proj, model.get_xyz @ cam.world_view_transform[:3, :2] + cam.world_view_transform[3, :2])
        assert not o["shadow"].requires_grad
    assert not torch.equal(outs[0]["altitude_render"][:8, :8], outs[1]["altitude_render"][:8, :8])


def test_color_reset_end_to_end(dev):
    from eogs2_amd.reset import color_reset, render_all_views

    cams = RC.make_cameras(dev)
    model = RC.make_model(300, dev)
    with torch.no_grad():
        model._opacity[7] = RC.RETIRED_LOGIT
    before, ids = RC.snapshot(model.optimizer), RC.identities(model.optimizer)
    torch.manual_seed(11)
    shadows = [o["shadow"].cpu() for o in render_all_views(cams, model, pipe())]  # (the background's RGB is random: same seed below)
    torch.manual_seed(11)
    flags = color_reset(model, cams, pipe())
    views = [(s, cam.affine.cpu()) for s, cam in zip(shadows, cams)]
    xyz, opacity = before["xyz"][0], before["opacity"][0].view(-1)
    borderline = RC.check_flags(flags, xyz, views, opacity)
    assert 0 < int(flags.sum()) < 300 and int(flags[7]) == 0
    want = RC.color_reset_ref(before, flags.cpu())
    RC.assert_snapshots_equal(RC.snapshot(model.optimizer), want, skip_rows=borderline)
    assert RC.identities(model.optimizer) == ids


def test_example_replays_across_both_resets(dev):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    args = ["--gaussians", "20000", "--size", "128", "--iters", "24", "--quiet", "--optimizer-in-graph", "--graph",
            "--opacity-reset-every", "8", "--color-reset-at", "12"]
    first, last, n = train_synthetic.main(args)
    step = train_synthetic.main.last_step
    assert train_synthetic.main.last_resets == [(8, "opacity", 1), (12, "color", 1), (16, "opacity", 1), (24, "opacity", 1)]
    assert train_synthetic.main.last_recordings == 1 and step.recaptures == 0  # the one recording of iteration 2 served them all
    assert step.replays == 23 and n == 20000
    assert first == first and last == last  # finite losses
