"""GPU (MI355X): the flow-matching step (eogs2_amd.flow over eogs2_amd/csrc/flow.hip) against the float64 statement of
tests/flow_cases.py, against every fixture of the reference's own code (tests/golden/flow), at full size against the
reference's fp32 op sequence on the same card; bitwise reproducible gradients; the device gate, eager and as a replayed graph;
the example's --flow-matching."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import flow_cases as FC
import resample_cases as RC
from util import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def run(F, img, flow, upstream, gate=None):
    x = img.clone().requires_grad_(True)
    out = F.apply_flow(x, flow, gate=gate)
    out.backward(upstream)
    return out.detach(), x.grad


reference_ops = RC.reference_flow_ops  # flow_matching.py:225-253 as the reference runs it (fp32 torch ops and autograd)


def flows_for(H, W, g, dev):
    cst = lambda dx, dy: torch.tensor([dx, dy], device=dev).view(1, 2, 1, 1).expand(1, 2, H, W)  # noqa: E731
    return {"field": (3.0 * torch.randn(1, 2, H, W, generator=g)).to(dev), "large": (20.0 * torch.randn(1, 2, H, W, generator=g)).to(dev),
            "integer": (3.0 * torch.randn(1, 2, H, W, generator=g)).round().to(dev), "constant": cst(0.37, -1.62),
            "constant_outside": cst(-(W + 10.25), 9.5)}


@pytest.mark.parametrize("C,H,W", [(3, 33, 47), (2, 17, 300), (3, 128, 128), (5, 64, 80), (None, 64, 80)])
def test_apply_flow_against_the_float64_statement(dev, C, H, W):
    from eogs2_amd import flow as F

    g = torch.Generator().manual_seed(H * 1000 + W)
    img = torch.rand(*((H, W) if C is None else (C, H, W)), generator=g).to(dev)
    up = torch.randn(C or 1, H, W, generator=g).to(dev)
    for name, flow in flows_for(H, W, g, dev).items():
        out, grad = run(F, img, flow, up)
        assert out.shape == (C or 1, H, W) and grad.shape == img.shape
        what = f"{name} {C}x{H}x{W}"
        e_out = assert_close(out, FC.warp(img.cpu().numpy(), flow.cpu().numpy()), what + " out", rtol=1e-4, allow_flips=False)
        want = FC.warp_adjoint(up.cpu().numpy(), flow.cpu().numpy())
        e_g = assert_close(grad if C else grad[None], want, what + " g_img", rtol=1e-4, allow_flips=False)
        print(f"{what}: out {e_out:.2e} g_img {e_g:.2e}")
    zero = torch.zeros(1, 2, H, W, device=dev)
    out, grad = run(F, img, zero, up)
    assert torch.equal(out, img.reshape(out.shape)) and torch.equal(grad, up.reshape(grad.shape))  # bit for bit
    out, grad = run(F, img, zero[:, :, :1, :1].expand(1, 2, H, W), up)
    assert torch.equal(out, img.reshape(out.shape)) and torch.equal(grad, up.reshape(grad.shape))


@pytest.mark.parametrize("name", FC.APPLY)
def test_apply_flow_against_the_reference_fixtures(dev, name):
    from eogs2_amd import flow as F

    fx = FC.load(name)
    t = lambda k: torch.from_numpy(fx[k]).to(dev)  # noqa: E731
    flow = t("flow")
    if name.startswith("apply_cst"):  # the constant-displacement path: two floats and zero strides
        flow = flow[:, :, :1, :1].contiguous().expand_as(flow)
    out, grad = run(F, t("img"), flow, t("upstream"))
    assert_close(out, fx["out"], name + " out", rtol=1e-4, allow_flips=False)
    assert_close(grad if grad.ndim == 3 else grad[None], fx["g_img"] if fx["g_img"].ndim == 3 else fx["g_img"][None], name + " g_img",
                 rtol=1e-4, allow_flips=False)
    if name.startswith("apply_cst"):  # and the same displacement as a field: the bucketed gather
        out, grad = run(F, t("img"), t("flow"), t("upstream"))
        assert_close(out, fx["out"], name + " out (field)", rtol=1e-4, allow_flips=False)
        assert_close(grad, fx["g_img"], name + " g_img (field)", rtol=1e-4, allow_flips=False)


def test_stats_against_the_fixtures(dev):
    from eogs2_amd import flow as F

    fx = FC.load("stats")
    w = F.performOpticalmatching(True, model=None)
    for k in range(3):
        flow = fx[f"flow{k}"]
        want, bound = FC.stats(flow), 1e-6 * np.abs(flow).max()
        # the fixture's own fp32 values sit within the bound of the statement
        assert np.abs(want[[0, 1, 3, 4]] - fx[f"stats{k}"]).max() <= bound and abs(want[2] - fx[f"meanabs{k}"]) <= bound
        f = torch.from_numpy(flow).to(dev)
        got = F.flow_stats(f).cpu().numpy().astype(np.float64)
        print(f"stats{k}: max error {np.abs(got - want).max():.3e}, bound {bound:.3e}")
        assert np.abs(got - want).max() <= bound, (k, got, want)
        mx, my, sx, sy = (float(v) for v in w.compute_stats(f))
        assert np.abs(np.array([mx, my, sx, sy]) - want[[0, 1, 3, 4]]).max() <= bound
        cst = w.set_cst_displacement(f)
        assert cst.shape == f.shape and cst.stride()[2:] == (0, 0)
        assert np.abs(cst.cpu().numpy() - fx[f"cst{k}"]).max() <= bound
        assert abs(float(F.flowmatch_l(f)) - abs(flow.astype(np.float64).mean())) <= bound
        # a non-contiguous flow (the crop of "upscale" mode) and a constant one
        crop = f[:, :, :-3, :-5]
        assert np.abs(F.flow_stats(crop).cpu().numpy() - FC.stats(flow[:, :, :-3, :-5])).max() <= bound
        assert np.abs(F.flow_stats(cst).cpu().numpy() - FC.stats(cst.cpu().numpy())).max() <= bound
    fx = FC.load("adjust_affine")
    wvt = torch.from_numpy(fx["world_view_transform"]).to(dev)
    out = F.adjust_affine(wvt, int(fx["img_W"]), int(fx["img_H"]), torch.from_numpy(fx["flow"]).to(dev))
    assert out is wvt and np.abs(wvt.cpu().numpy() - fx["out"]).max() <= 1e-6 * np.abs(fx["out"]).max()


class RecordingModel:
    def __init__(self, flow):
        self.flow, self.calls = flow, []

    def __call__(self, gt, target, num_flow_updates=12):
        self.calls.append((gt, target, num_flow_updates))
        return [torch.zeros_like(self.flow), self.flow]


@pytest.mark.parametrize("name", FC.GETFLOW)
def test_get_flow_against_the_reference_fixtures(dev, name):
    from eogs2_amd import flow as F

    fx = FC.load(name)
    t = lambda k: torch.from_numpy(fx[k]).to(dev)  # noqa: E731
    model = RecordingModel(t("model_flow"))
    w = F.performOpticalmatching(bool(fx["cst"]), mode="downscale" if "downscale" in name else "upscale", device=dev, model_name="small",
                                 num_flow_updates=7, criteria="always", model=model)
    flows, gt, target = w.get_flow(t("gt"), t("target"), device=dev)
    (mgt, mtarget, nfu), = model.calls
    assert nfu == int(fx["num_flow_updates"]) and mgt.shape == fx["model_gt"].shape
    assert torch.equal(mgt.cpu(), torch.from_numpy(fx["model_gt"])) and torch.equal(mtarget.cpu(), torch.from_numpy(fx["model_target"]))
    assert flows.shape == fx["flows"].shape
    assert np.abs(flows.cpu().numpy() - fx["flows"]).max() <= 1e-6 * np.abs(fx["model_flow"]).max()
    assert torch.equal(gt.cpu(), torch.from_numpy(fx["gt_out"])) and torch.equal(target.cpu(), torch.from_numpy(fx["target_out"]))


@pytest.mark.parametrize("name", FC.PERFORM)
def test_perform_flow_matching_against_the_reference_fixtures(dev, name):
    from eogs2_amd import flow as F

    fx = FC.load(name)
    t = lambda k: torch.from_numpy(fx[k]).to(dev)  # noqa: E731
    criteria = {"maxflow": "max_value_flow", "always": "always", "lphotom": "l_photom", "psnr": "psnr"}[name.split("_")[1]]
    mode = "downscale" if "downscale" in name else "upscale"
    w = F.performOpticalmatching(bool(fx["cst"]), mode=mode, device=dev, model_name="small", num_flow_updates=7, criteria=criteria,
                                 model=RecordingModel(t("model_flow")))
    opt = types.SimpleNamespace(flowmatching=types.SimpleNamespace(max_value_flow=float(fx["max_value_flow"])))
    image, gt = t("image").requires_grad_(True), t("gt")
    flows, gt_out, image_out = F.perform_flow_matching(opt, w, image, gt)
    accepted = bool(fx["accepted"])
    assert (image_out is not image) == accepted  # the decision, exactly
    if not accepted:
        assert gt_out is gt and image_out is image  # the original objects come back
    assert np.abs(flows.cpu().numpy() - fx["flows"]).max() <= 1e-6 * np.abs(fx["model_flow"]).max()
    assert torch.equal(gt_out.cpu(), torch.from_numpy(fx["gt_out"]))
    assert_close(image_out.detach(), fx["image_out"], name + " image", rtol=1e-4, allow_flips=False)
    image_out.backward(t("upstream"))
    assert_close(image.grad, fx["g_image"], name + " g_image", rtol=1e-4, allow_flips=False)
    if mode == "upscale" and criteria in ("max_value_flow", "always"):  # the same decision made on the device
        image2 = t("image").requires_grad_(True)
        _, gt2, out2 = F.perform_flow_matching(opt, w, image2, gt, on_device=True)
        out2.backward(t("upstream"))
        assert gt2 is gt and torch.equal(out2.detach(), image_out.detach()) and torch.equal(image2.grad, image.grad)
    if criteria == "psnr":  # specified for one plane; more raise as the reference's comparison does
        with pytest.raises(RuntimeError, match="ambiguous"):
            F.perform_flow_matching(opt, w, t("image").expand(3, -1, -1), gt.expand(3, -1, -1))


@pytest.mark.parametrize("kind", ["field", "constant"])
def test_full_size_against_the_reference_ops(dev, kind):
    """3 x 1024^2 against the reference's fp32 op sequence on the same GPU: every element within 2e-4 of its channel's maximum.
    (On the CPU the reference's fp32 sits 5.1e-5 from the float64 statement at 1024^2; two fp32 evaluations may differ by the sum
    of their distances from it.)"""
    from eogs2_amd import flow as F

    H = W = 1024
    g = torch.Generator().manual_seed(7)
    img, up = torch.rand(3, H, W, generator=g).to(dev), torch.randn(3, H, W, generator=g).to(dev)
    if kind == "field":
        flow = (3.0 * torch.randn(1, 2, H, W, generator=g)).to(dev)
    else:
        flow = torch.tensor([1.37, -0.62], device=dev).view(1, 2, 1, 1).expand(1, 2, H, W)
    out, grad = run(F, img, flow, up)
    ref_out, ref_grad = reference_ops(img, flow, up)
    e_out = assert_close(out, ref_out, f"{kind} 1024 out", rtol=2e-4, allow_flips=False)
    e_g = assert_close(grad, ref_grad, f"{kind} 1024 g_img", rtol=2e-4, allow_flips=False)
    print(f"{kind} 3x1024x1024: out {e_out:.2e} g_img {e_g:.2e} of the channel maximum")


def test_backward_and_stats_reproducible_bit_for_bit(dev):
    from eogs2_amd import flow as F

    H, W = 192, 256
    g = torch.Generator().manual_seed(3)
    img, up = torch.rand(3, H, W, generator=g).to(dev), torch.randn(3, H, W, generator=g).to(dev)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    # contracting: every output samples near the centre, hundreds of outputs per input cell
    contracting = torch.stack((0.9 * (W / 2 - xx), 0.9 * (H / 2 - yy)))[None].to(dev) + torch.rand(1, 2, H, W, generator=g).to(dev)
    beyond = torch.tensor([W + 40.5, -(H + 3.25)], device=dev).view(1, 2, 1, 1).expand(1, 2, H, W)
    for name, flow in (("contracting", contracting), ("beyond the border", beyond)):
        first = run(F, img, flow, up)
        assert_close(first[1], FC.warp_adjoint(up.cpu().numpy(), flow.cpu().numpy()), name + " g_img", rtol=1e-4, allow_flips=False)
        for _ in range(5):
            again = run(F, img, flow, up)
            assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), name
    s = F.flow_stats(contracting)
    for _ in range(5):
        assert torch.equal(F.flow_stats(contracting), s)


def test_gate(dev):
    from eogs2_amd import flow as F

    H, W = 96, 120
    g = torch.Generator().manual_seed(5)
    img, up = torch.rand(3, H, W, generator=g).to(dev), torch.randn(3, H, W, generator=g).to(dev)
    for name, flow in flows_for(H, W, g, dev).items():
        plain = run(F, img, flow, up)
        shut = run(F, img, flow, up, gate=torch.zeros(1, device=dev))
        assert torch.equal(shut[0], img) and torch.equal(shut[1], up), name  # copies, bit for bit
        for one in (torch.ones(1, device=dev), torch.ones(1, device=dev, dtype=torch.bool)):
            opened = run(F, img, flow, up, gate=one)
            assert torch.equal(opened[0], plain[0]) and torch.equal(opened[1], plain[1]), name


def test_on_device_decision_replayed_from_a_graph(dev):
    """perform_flow_matching(on_device=True) recorded once; the flow buffer is then overwritten with a flow below and above
    max_value_flow: both replays give what the eager host branch gives."""
    from eogs2_amd import flow as F

    H, W = 96, 120  # multiples of 8: the network's flow is the buffer itself
    g = torch.Generator().manual_seed(9)
    image, gt, up = (torch.rand(3, H, W, generator=g).to(dev) for _ in range(3))
    buf = torch.zeros(1, 2, H, W, device=dev)
    w = F.performOpticalmatching(True, mode="upscale", device=dev, criteria="max_value_flow",
                                 model=lambda a, b, num_flow_updates=12: [buf])
    opt = types.SimpleNamespace(flowmatching=types.SimpleNamespace(max_value_flow=3.0))
    x = image.clone().requires_grad_(True)

    def step():
        x.grad = None
        _, _, out = F.perform_flow_matching(opt, w, x, gt, on_device=True)
        out.backward(up)
        return out.detach(), x.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g_out, g_grad = step()
    small = (torch.tensor([1.2, -0.7]).view(1, 2, 1, 1) + 0.1 * torch.randn(1, 2, H, W, generator=g)).to(dev)
    large = (torch.tensor([6.0, -5.0]).view(1, 2, 1, 1) + 0.1 * torch.randn(1, 2, H, W, generator=g)).to(dev)
    for name, flow, accepted in (("below", small, True), ("above", large, False), ("below again", small, True)):
        buf.copy_(flow)
        graph.replay()
        torch.cuda.synchronize()
        x2 = image.clone().requires_grad_(True)
        _, gt_out, out = F.perform_flow_matching(opt, w, x2, gt)  # eager, host branch
        assert (out is not x2) == accepted, name
        out.backward(up)
        assert torch.equal(g_out, out.detach()) and torch.equal(g_grad, x2.grad), name


def test_example_flow_matching(dev):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    args = ["--gaussians", "20000", "--size", "160", "--iters", "60", "--quiet", "--flow-matching"]
    eager = train_synthetic.main(args)
    assert eager[1] < eager[0], eager  # trains
    graph = train_synthetic.main(args + ["--graph"])
    assert graph == eager, (eager, graph)  # bit for bit


# ---- the edge cases of the bucketed gather with FlowSrc (tests/resample_cases.py; checked on the CPU by
# tests/test_resample_cases.py) ----
@pytest.mark.parametrize("name", RC.FLOW)
def test_flow_case_against_the_float64_statement(dev, name):
    """Full buckets, the 64x32-tile instantiations (one, three and five planes), two scan rounds, strided fields: flows are
    multiples of 1/8, so cell and weight are exact in fp32 and no element is left out."""
    from eogs2_amd import flow as F

    c = RC.flow_case(name)
    img, up, flow = c["img"].to(dev), c["up"].to(dev), c["flow"].to(dev)
    first = run(F, img, flow, up)
    err = RC.compare_flow(first, RC.oracle_flow(name), RC.TOL, name)
    print(f"{name}: out {err['out']:.2e} g_img {err['g_img']:.2e}")
    if name == "flow_strided":
        for layout, view in RC.strided_views(flow).items():
            again = run(F, img, view, up)
            assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), layout


def test_field_backward_overwrites_every_element_of_its_output(dev):
    """eogs_resample_flow_backward straight through the C-ABI into a buffer full of NaN, five planes at 64x32 tiles (a four-plane
    and a one-plane pass): every element written, cells no tap reaches with exact zeros, the bits of the autograd path."""
    from eogs2_amd import _host, _lib
    from eogs2_amd import flow as F

    c = RC.flow_case("flow_big5")
    C, H, W = c["img"].shape
    up, flow = c["up"].to(dev), c["flow"].to(dev)
    g_img = torch.full((C, H, W), float("nan"), device=dev)
    nbytes = _host.nbytes(_lib.get(), "resample_flow_bytes", H, W)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _host.call("eogs_resample_flow_backward", up.device, C, H, W, flow.data_ptr(), *flow.stride()[1:], None, up.data_ptr(), g_img.data_ptr(),
               ws.data_ptr(), nbytes)
    torch.cuda.synchronize()
    assert not torch.isnan(g_img).any()
    reached = torch.from_numpy(RC.reached_cells(*RC.flow_tap_cells(c["flow"]), H, W, dilate=1))
    assert not g_img.cpu()[:, ~reached].any()
    assert g_img.abs().amax(dim=(1, 2)).min() > 0
    RC.compare_flow((RC.oracle_flow("flow_big5")[0], g_img), RC.oracle_flow("flow_big5"), RC.TOL, "flow_big5 through the C-ABI")
    assert torch.equal(run(F, c["img"].to(dev), flow, up)[1], g_img)


def test_full_bucket_backward_is_reproducible_bit_for_bit(dev):
    from eogs2_amd import flow as F

    c = RC.flow_case("flow_converge")
    img, up, flow = c["img"].to(dev), c["up"].to(dev), c["flow"].to(dev)
    first = run(F, img, flow, up)
    assert float(first[1].abs().max()) > 0
    for _ in range(5):
        again = run(F, img, flow, up)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
