"""CPU: the float64 restatement of ground-truth preparation (tests/gtprep_cases.py) is pinned to the fixtures that the
reference's own Python produced (tests/golden/gtprep/, made by tests/golden/make_golden_gtprep.py): pansharpening and the
losses at 2e-5 of max |ref| (the bar of tests/test_shade_oracle.py), brovey's dark family per element against K * 2^-24 * B_i,
the rescalers bit for bit. The GPU tests hold the kernels to the same restatement and the same fixtures."""
import os

import numpy as np
import pytest

import gtprep_cases as gc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtprep")


def name_of(shape):
    return "x".join(str(s) for s in shape)


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def checksum(*arrays):
    return sum(float(np.where(np.isfinite(a), a, 0).astype(np.float64).sum()) for a in arrays)


def sub(a, shape):
    s = gc.stride_of(shape)
    return a[..., ::s, ::s]


def close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    bar = gc.REL_BAR * float(np.abs(ref).max())
    print(what, "max |err|", err, "bar", bar)
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("pair", gc.PAIRS, ids=lambda p: name_of(p[0]) + "_" + name_of(p[1]))
@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("method", gc.METHODS)
def test_pansharp_restatement_equals_the_reference(method, family, pair):
    f = load(f"pansharp_{method}_{family}_{name_of(pair[0])}_{name_of(pair[1])}")
    for C in gc.fixture_channels(method, pair):
        msi, pan = gc.pansharp_inputs(family, C, pair)
        assert checksum(msi, pan) == float(f[f"checksum_c{C}"])  # the inputs are the ones the fixture was made from
        ref = f[f"out_c{C}"]
        if method == "brovey" and family == "dark":
            out, B = gc.pansharp(method, msi, pan, with_bound=True)
            err = np.abs(ref.astype(np.float64) - sub(out, pair[1]))
            assert bool((err <= gc.DARK_K * gc.EPS32 * sub(B, pair[1])).all()), float((err - gc.DARK_K * gc.EPS32 * sub(B, pair[1])).max())
        else:
            close(sub(gc.pansharp(method, msi, pan), pair[1]), ref, (method, family, pair, C))
            if method == "brovey":  # the per-element bound holds on the lit fixtures too (largest ratio 0.125)
                out, B = gc.pansharp(method, msi, pan, with_bound=True)
                assert bool((np.abs(ref.astype(np.float64) - sub(out, pair[1])) <= gc.DARK_K * gc.EPS32 * sub(B, pair[1])).all())


def test_dark_k_is_the_smallest_integer_that_holds_every_dark_fixture():
    """The measurement behind gtprep_cases.DARK_K, made again: the dark inputs do undershoot and blow up, and K is tight."""
    worst, big, negative = 0.0, 0, 0
    for pair in gc.PAIRS:
        f = load(f"pansharp_brovey_dark_{name_of(pair[0])}_{name_of(pair[1])}")
        for C in gc.fixture_channels("brovey", pair):
            msi, pan = gc.pansharp_inputs("dark", C, pair)
            out, B = gc.pansharp("brovey", msi, pan, with_bound=True)
            err = np.abs(f[f"out_c{C}"].astype(np.float64) - sub(out, pair[1]))
            bound = gc.EPS32 * sub(B, pair[1])
            assert not err[bound == 0].any()
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            big += int((np.abs(f[f"out_c{C}"]) > 1e5).sum())
            negative += int((gc.upsample(msi, *pair[1], True).sum(axis=0) < 0).sum())
    print("largest |fixture - restatement| / (2^-24 B_i):", worst, "; elements above 1e5:", big, "; pixels with a negative sum:", negative)
    assert big > 100 and negative > 100  # the family does what it is for
    assert gc.DARK_K - 1 < worst <= gc.DARK_K
    assert gc.DARK_K < 10  # single digits, as expected of a bound with absolute weight error


@pytest.mark.parametrize("pair", gc.LOSS_PAIRS, ids=lambda p: name_of(p[0]) + "_" + name_of(p[1]))
@pytest.mark.parametrize("method", gc.METHODS)
def test_pansharp_loss_restatement_equals_the_reference(method, pair):
    f = load(f"loss_{method}_{name_of(pair[0])}_{name_of(pair[1])}")
    syn, msi, pan = gc.loss_inputs(method, pair)
    assert checksum(syn, msi, pan) == float(f["checksum"])
    loss, grad = gc.l2(syn, gc.pansharp(method, msi, pan), gc.UPSTREAM)
    close(loss, f["loss"], (method, pair, "loss"))
    close(sub(grad, pair[1]), f["grad"], (method, pair, "grad"))


@pytest.mark.parametrize("shape", gc.GRADIENT_SHAPES, ids=name_of)
def test_pan_losses_restatement_equals_the_reference(shape):
    f = load(f"pan_losses_{name_of(shape)}")
    a, b = gc.gradient_inputs(shape)
    assert checksum(a, b) == float(f["checksum"])
    loss, grad = gc.l2(a, b, gc.UPSTREAM)
    close(loss, f["lpan"], (shape, "Lpan"))
    close(grad, f["lpan_grad"], (shape, "Lpan grad"))
    loss, grad = gc.gradient_l2(a, b, gc.UPSTREAM)
    close(loss, f["lgradient"], (shape, "Lgradient_pan"))
    close(grad, f["lgradient_grad"], (shape, "Lgradient_pan grad"))


def test_gradient_restatement_is_torch_gradient():
    import torch

    for shape in gc.GRADIENT_SHAPES:
        a, _ = gc.gradient_inputs(shape)
        gy, gx = torch.gradient(torch.from_numpy(a).double(), dim=(-2, -1))
        d = a.astype(np.float64)
        assert np.allclose(np.einsum("ij,...jx->...ix", gc._grad_matrix(shape[-2]), d), gy.numpy(), rtol=0, atol=1e-15)
        assert np.allclose(np.einsum("ij,...yj->...yi", gc._grad_matrix(shape[-1]), d), gx.numpy(), rtol=0, atol=1e-15)


@pytest.mark.parametrize("kind", gc.RESCALE_KINDS)
@pytest.mark.parametrize("shape", gc.RESCALE_SHAPES, ids=name_of)
def test_rescaler_restatement_equals_the_reference_bit_for_bit(shape, kind):
    f = load(f"rescale_{kind}_{name_of(shape)}")
    x = gc.rescale_input(shape, kind)
    assert checksum(x) == float(f["checksum"])
    mm = gc.minmax(x)
    assert gc.same_bits(mm, f["minmax"])
    assert gc.same_bits(sub(gc.clamp(x), shape), f["clamper"])
    assert gc.same_bits(sub(gc.rescale(x, mm), shape), f["standard"])
    assert gc.same_bits(sub(gc.rescale(x, gc.minmax(gc.rescale_input(shape, "plain"))), shape), f["wrt_first"])
    if kind == "nan":  # the channel that holds the NaN is all NaN, the others are untouched by it
        out = gc.rescale(x, mm)
        assert np.isnan(out[-1]).all() and np.isnan(mm[-1]).all()
        assert not np.isnan(out[:-1]).any() and not np.isnan(gc.clamp(x)).sum() > 1
    if kind == "constant":
        assert not gc.rescale(x, mm)[0].any()  # 0 / 1e-8


def test_equalize_restatement_on_its_cases():
    """No fixture exists for the histogram (torchvision is not compared against): the rule's own properties."""
    x = gc.hist_input((3, 5, 7), "plain")
    assert gc.same_bits(gc.equalize(x), (gc.to_levels(x).astype(np.float32) / np.float32(255)))  # 35 pixels: step == 0, unchanged
    x = gc.hist_input((3, 64, 48), "single")
    assert gc.same_bits(gc.equalize(x)[0], np.full((64, 48), np.float32(102) / np.float32(255)))  # one level: unchanged
    x = gc.hist_input((3, 64, 48), "all")
    assert len(np.unique(gc.to_levels(x)[0])) == 256
    out = gc.equalize(x)
    assert out.min() >= 0 and out.max() <= 1 and out.dtype == np.float32
    lv = gc.to_levels(x)[1].reshape(-1)
    order = np.argsort(lv, kind="stable")
    assert bool((np.diff(out[1].reshape(-1)[order]) >= 0).all())  # monotone in the level
    special = np.array([[0.0, 1.0, -1e-7, 1.0000001, -3.0, 7.0, np.nan, np.inf, -np.inf, 1 / 255.0, 0.0039215]], np.float32)
    assert gc.to_levels(special).tolist() == [[0, 255, 0, 255, 0, 255, 0, 255, 0, 1, 0]]
