"""GPU: ground-truth preparation (eogs2_amd.pansharp, eogs2_amd.rescaler, include/eogs_gtprep.h) against the float64
restatement of tests/gtprep_cases.py and the fixtures the reference's own Python produced (tests/golden/gtprep/):
pansharpening and the losses at 2e-5 of max |ref|, brovey's dark family per element against 4 K 2^-24 B_i, the rescalers and
the histogram bit for bit. Sizes are the smallest at which a kernel can still go wrong (gtprep_cases.PAIRS and friends)."""
import os
import types

import numpy as np
import pytest
import torch

import gtprep_cases as gc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtprep")
CFG = lambda m: types.SimpleNamespace(method=m)  # noqa: E731


def name_of(shape):
    return "x".join(str(s) for s in shape)


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def sub(a, shape):
    s = gc.stride_of(shape)
    return a[..., ::s, ::s]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    bar = gc.REL_BAR * float(np.abs(ref).max())
    print(what, "max |err|", err, "bar", bar)
    assert np.isfinite(got).all() and err <= bar, (what, err, bar)


def run_method(method, msi, pan):
    from eogs2_amd import pansharp as P

    rp, rm = gc.reference_shapes(method, msi, pan)
    out = P.load_pansharp(CFG(method))(img_pan=dev(rp), img_msi=dev(rm))
    assert out.dtype == torch.float32 and out.is_cuda and not out.requires_grad and tuple(out.shape) == (msi.shape[0],) + pan.shape
    return out.cpu().numpy()


@pytest.fixture(autouse=True)
def needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("pair", gc.PAIRS, ids=lambda p: name_of(p[0]) + "_" + name_of(p[1]))
@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("method", gc.METHODS)
def test_pansharp(method, family, pair):
    f = load(f"pansharp_{method}_{family}_{name_of(pair[0])}_{name_of(pair[1])}")
    for C in gc.channels_of(method):
        msi, pan = gc.pansharp_inputs(family, C, pair)
        got = run_method(method, msi, pan)
        fixture = f[f"out_c{C}"] if f"out_c{C}" in f.files else None
        if method == "brovey" and family == "dark":  # per element, none left out
            ref, B = gc.pansharp(method, msi, pan, with_bound=True)
            err = np.abs(got.astype(np.float64) - ref)
            bound = 4 * gc.DARK_K * gc.EPS32 * B
            print(method, family, pair, C, "largest err / (2^-24 B_i):", float((err[B > 0] / (gc.EPS32 * B[B > 0])).max()) if (B > 0).any() else 0.0)
            assert np.isfinite(got).all() and bool((err <= bound).all()), float((err - bound).max())
            if fixture is not None:  # both lie inside their own bound of the restatement
                assert bool((np.abs(sub(got, pair[1]).astype(np.float64) - fixture) <= sub(bound, pair[1]) * 1.25).all())
        else:
            close(got, gc.pansharp(method, msi, pan), (method, family, pair, C))
            if fixture is not None:
                close(sub(got, pair[1]), fixture, (method, family, pair, C, "fixture"))
            if method == "brovey":  # lit images undershoot too (one channel at (17,9)->(70,33) reaches 1e6): the bound holds here as well
                ref, B = gc.pansharp(method, msi, pan, with_bound=True)
                assert bool((np.abs(got.astype(np.float64) - ref) <= 4 * gc.DARK_K * gc.EPS32 * B).all())


def test_brovey_accepts_the_references_pan_shapes_and_weight():
    from eogs2_amd.pansharp import brovey_pansharp

    msi, pan = gc.pansharp_inputs("lit", 3, gc.PAIRS[3])
    base = brovey_pansharp(dev(pan), dev(msi))
    assert torch.equal(brovey_pansharp(dev(pan)[None], dev(msi)), base) and torch.equal(brovey_pansharp(dev(pan)[:, :, None], dev(msi)), base)
    close(brovey_pansharp(dev(pan), dev(msi), W=0.5).cpu().numpy(), gc.pansharp("brovey", msi, pan, W=0.5), "W = 0.5")
    view = dev(np.concatenate([msi, msi], axis=2))[:, :, :msi.shape[2]]  # a non-contiguous MSI image
    assert torch.equal(brovey_pansharp(dev(pan), view), base)


def loss_of(method, syn, msi, pan):
    from eogs2_amd.pansharp import Pansharploss

    rp, rm = gc.reference_shapes(method, msi, pan)
    return Pansharploss(0.1, CFG(method))(syn, dev(rp), dev(rm))


@pytest.mark.parametrize("pair", gc.LOSS_PAIRS, ids=lambda p: name_of(p[0]) + "_" + name_of(p[1]))
@pytest.mark.parametrize("method", gc.METHODS)
def test_pansharp_loss(method, pair):
    f = load(f"loss_{method}_{name_of(pair[0])}_{name_of(pair[1])}")
    syn_h, msi, pan = gc.loss_inputs(method, pair)
    ref_loss, ref_grad = gc.l2(syn_h, gc.pansharp(method, msi, pan), gc.UPSTREAM)
    runs = []
    for _ in range(2):
        syn = dev(syn_h).requires_grad_(True)
        loss = loss_of(method, syn, msi, pan)
        (gc.UPSTREAM * loss).backward()  # upstream != 1
        runs.append((loss.detach().cpu().numpy(), syn.grad.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()  # the same bits
    loss, grad = runs[0]
    close(loss, ref_loss, (method, pair, "loss"))
    close(grad, ref_grad, (method, pair, "grad"))
    close(loss, f["loss"], (method, pair, "loss, fixture"))
    close(sub(grad, pair[1]), f["grad"], (method, pair, "grad, fixture"))
    # upstream = 1 (NULL is not reachable from autograd: a tensor of one)
    syn = dev(syn_h).requires_grad_(True)
    loss_of(method, syn, msi, pan).backward()
    close(syn.grad.cpu().numpy(), ref_grad / gc.UPSTREAM, (method, pair, "grad, upstream 1"))


@pytest.mark.parametrize("method", gc.METHODS)
def test_pansharp_loss_of_the_target_itself_is_zero(method):
    from eogs2_amd import pansharp as P

    for family in gc.FAMILIES:  # dark brovey: targets up to 1e7, still no NaN
        msi, pan = gc.pansharp_inputs(family, 3, gc.LOSS_PAIRS[0])
        rp, rm = gc.reference_shapes(method, msi, pan)
        syn = P.load_pansharp(method)(dev(rp), dev(rm)).clone().requires_grad_(True)
        loss = P.Pansharploss(1.0, method)(syn, dev(rp), dev(rm))
        loss.backward()
        assert float(loss.detach()) == 0.0 and not syn.grad.any() and not torch.isnan(syn.grad).any()


def test_pansharp_loss_under_graph_capture_replays_to_the_eager_bits():
    """Forward plus backward recorded on one stream. The recipe of tests/test_gpu_reg.py: the warm-up runs on the stream that
    is captured afterwards, so the leaf's gradient accumulator belongs to that stream and the capture stays on it."""
    from eogs2_amd.pansharp import Pansharploss

    method, pair = "brovey", gc.LOSS_PAIRS[1]
    syn_h, msi_h, pan_h = gc.loss_inputs(method, pair)
    syn, msi, pan = dev(syn_h).requires_grad_(True), dev(msi_h), dev(pan_h)  # (no copies from the host inside the capture)
    term = Pansharploss(0.1, CFG(method))

    def step():
        syn.grad = None
        loss = term(syn, pan, msi)
        (gc.UPSTREAM * loss).backward()
        return loss.detach(), syn.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rec = step()
    for _ in range(2):
        rec[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rec[0], eager[0]) and torch.equal(rec[1], eager[1])
    with torch.no_grad():  # a replay reads the tensors in place
        syn.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rec[0], term(syn.detach(), pan, msi)) and not torch.equal(rec[0], eager[0])


@pytest.mark.parametrize("shape", gc.GRADIENT_SHAPES, ids=name_of)
def test_pan_losses(shape):
    from eogs2_amd.pansharp import Lgradient_pan, Lpan

    f = load(f"pan_losses_{name_of(shape)}")
    a, b = gc.gradient_inputs(shape)
    for key, cls, ref_fn in (("lpan", Lpan, gc.l2), ("lgradient", Lgradient_pan, gc.gradient_l2)):
        ref_loss, ref_grad = ref_fn(a, b, gc.UPSTREAM)
        runs = []
        for _ in range(2):
            x = dev(a).requires_grad_(True)
            loss = cls(0.1)(x, dev(b))
            (gc.UPSTREAM * loss).backward()
            runs.append((loss.detach().cpu().numpy(), x.grad.cpu().numpy()))
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
        close(runs[0][0], ref_loss, (shape, key))
        close(runs[0][1], ref_grad, (shape, key, "grad"))
        close(runs[0][0], f[key], (shape, key, "fixture"))
        close(runs[0][1], f[key + "_grad"], (shape, key, "grad, fixture"))
        x = dev(a).requires_grad_(True)  # image == ground truth: zero loss, zero gradient, no NaN
        loss = cls(0.1)(x, dev(a))
        loss.backward()
        assert float(loss.detach()) == 0.0 and not x.grad.any() and not torch.isnan(x.grad).any()


def test_pan_losses_take_views_and_broadcast_ground_truth():
    from eogs2_amd.pansharp import pan_gradient_l2, pan_l2

    a, b = gc.gradient_inputs((3, 5, 7))
    x = dev(np.concatenate([a, a], axis=2))[:, :, :7].requires_grad_(True)  # non-contiguous
    close(pan_l2(x, dev(b)).detach().cpu().numpy(), gc.l2(a, b)[0], "view")
    close(pan_gradient_l2(x, dev(b[:1])).detach().cpu().numpy(), gc.gradient_l2(a, np.broadcast_to(b[:1], a.shape))[0], "broadcast")


@pytest.mark.parametrize("kind", gc.RESCALE_KINDS)
@pytest.mark.parametrize("shape", gc.RESCALE_SHAPES, ids=name_of)
def test_rescalers_bit_for_bit(shape, kind):
    from eogs2_amd import rescaler as R

    f = load(f"rescale_{kind}_{name_of(shape)}")
    x = gc.rescale_input(shape, kind)
    mm = R.channel_minmax(dev(x)).cpu().numpy()
    assert gc.same_bits(mm, f["minmax"]) and gc.same_bits(mm, gc.minmax(x))
    assert gc.same_bits(R.compute_min_vals(dev(x)).cpu().numpy(), f["minmax"][:, 0])
    assert gc.same_bits(R.compute_max_vals(dev(x)).cpu().numpy(), f["minmax"][:, 1])
    clamped = R.load_rescaler("clamper").forward(dev(x)).cpu().numpy()
    assert gc.same_bits(clamped, gc.clamp(x)) and gc.same_bits(sub(clamped, shape), f["clamper"])
    std = R.load_rescaler("standard_rescaler").forward(dev(x)).cpu().numpy()
    assert gc.same_bits(std, gc.rescale(x, gc.minmax(x))) and gc.same_bits(sub(std, shape), f["standard"])
    # a reference camera that is not the first in the list
    first = gc.rescale_input(shape, "plain")
    cams = [types.SimpleNamespace(is_reference_camera=k == 1, original_image=dev(im)) for k, im in enumerate((x, first, x))]
    r = R.load_rescaler("rescale_wrt_firstimage")
    assert R.perform_rescaling_listcam(cams, r) is cams
    assert r.min_vals.is_cuda and gc.same_bits(torch.stack([r.min_vals, r.max_vals], 1).cpu().numpy(), gc.minmax(first))
    wrt = cams[0].original_image.cpu().numpy()
    assert gc.same_bits(wrt, gc.rescale(x, gc.minmax(first))) and gc.same_bits(sub(wrt, shape), f["wrt_first"])
    assert gc.same_bits(cams[2].original_image.cpu().numpy(), wrt)
    assert gc.same_bits(cams[1].original_image.cpu().numpy(), gc.rescale(first, gc.minmax(first)))
    if kind == "nan":  # that channel is all NaN, the others are untouched
        assert np.isnan(std[-1]).all() and not np.isnan(std[:-1]).any() and int(np.isnan(clamped).sum()) == 1
    if kind == "constant":
        assert not std[0].any()


def test_perform_rescaling_walks_the_pan_and_msi_cameras():
    from eogs2_amd import rescaler as R

    x = gc.rescale_input((3, 5, 7), "plain")
    pans = [types.SimpleNamespace(original_image=dev(x[:1])) for _ in range(2)]
    msis = [types.SimpleNamespace(original_image=dev(x)) for _ in range(2)]
    cams = [types.SimpleNamespace(get_pan_cameras=lambda k=k: pans[k], get_msi_cameras=lambda k=k: msis[k]) for k in range(2)]
    R.perform_rescaling(cams, R.load_rescaler("clamper"), types.SimpleNamespace(load_pan=True, load_msi=False))
    assert gc.same_bits(pans[1].original_image.cpu().numpy(), gc.clamp(x[:1])) and gc.same_bits(msis[1].original_image.cpu().numpy(), x)
    R.perform_rescaling(cams, R.load_rescaler("standard_rescaler"), types.SimpleNamespace(load_pan=False, load_msi=True))
    assert gc.same_bits(msis[0].original_image.cpu().numpy(), gc.rescale(x, gc.minmax(x)))


@pytest.mark.parametrize("kind", ("plain", "single", "all", "edges"))
@pytest.mark.parametrize("shape", gc.HIST_SHAPES, ids=name_of)
def test_histogram_equalizer_bit_for_bit(shape, kind):
    from eogs2_amd.rescaler import load_rescaler

    x = gc.hist_input(shape, kind)
    eq = load_rescaler("histogram_equalizer")
    got = eq.forward(dev(x)).cpu().numpy()
    assert gc.same_bits(got, gc.equalize(x))
    assert gc.same_bits(eq.forward(dev(x)).cpu().numpy(), got)  # a second run counts the same
    if shape == (3, 5, 7):  # 35 pixels: step == 0, the channel is unchanged (decided on the device)
        assert gc.same_bits(got, gc.to_levels(x).astype(np.float32) / np.float32(255))
