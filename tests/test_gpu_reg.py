"""GPU (MI355X): the regularisers of eogs2_amd.regularizers (include/eogs_reg.h) against the reference's float64 run
(tests/golden/reg/*.npz) and, at full size, against the float64 restatement of tests/reg_cases.py, inside KERNEL_FACTOR x the
derived bounds; bitwise reproducibility, the device weights under a replayed graph, retired rows, and the example.

Measured on an MI355X: see DESIGN.md §8 (regularisers) for the seconds this file adds to the suite.
"""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import reg_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("opacity", "opacity_radii", "erank")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def run_gauss(o, l, r, n0, up, dev):
    """The fixture's outputs through the HIP path: the gradient of upstream[k] * terms[k], term by term."""
    from eogs2_amd import regularizers as R

    od, ld = o.to(dev).requires_grad_(True), l.to(dev).requires_grad_(True)
    total, terms = R.gaussian_regularizers(od, ld, r.to(dev), n_init=n0, weights=(0.0, 0.0, 0.0), want=ALL)
    assert float(total.detach()) == 0.0
    g = [torch.autograd.grad(float(up[k]) * terms[k], (od, ld), retain_graph=True) for k in range(3)]
    assert not bool(g[0][1].any()) and not bool(g[1][1].any()) and not bool(g[2][0].any())  # no cross-talk, exact zeros
    t = terms.detach().cpu().numpy()
    return {"L_opacity": t[0], "L_opacity_radii": t[1], "L_erank": t[2], "g_opacity_op": g[0][0].cpu().numpy(),
            "g_opacity_radii": g[1][0].cpu().numpy(), "g_scaling": g[2][1].cpu().numpy()}


def run_image(a, c, up, dev):
    from eogs2_amd import regularizers as R

    ad, cd = a.to(dev).requires_grad_(True), c.to(dev).requires_grad_(True)
    total, terms = R.render_regularizers(ad, cd, weights=(0.0, 0.0))
    g_a, = torch.autograd.grad(float(up[0]) * terms[0], ad, retain_graph=True)
    g_c, = torch.autograd.grad(float(up[1]) * terms[1], cd)
    t = terms.detach().cpu().numpy()
    return {"L_TV_altitude": t[0], "L_accumulated_opacity": t[1], "g_altitude": g_a.cpu().numpy(), "g_accumulated_opacity": g_c.cpu().numpy()}


@pytest.mark.parametrize("name", rc.GAUSS_FIXTURES)
def test_gaussian_terms_against_the_reference_fixtures(dev, name):
    fx = rc.load(name)
    o, l, r, n0, up = rc.gauss_inputs(fx)
    got = run_gauss(o, l, r, n0, up, dev)
    b = rc.gauss_bounds(o, l, r, n0, up)
    rc.compare(got, {k: fx[k + "@64"] for k in rc.GAUSS_KEYS}, b, rc.GAUSS_KEYS, rc.KERNEL_FACTOR, name + " HIP", excuse_rows=True)
    retired = (o.reshape(-1) <= 0.5 * rc.RETIRED_LOGIT).numpy()
    for k in ("g_opacity_op", "g_opacity_radii", "g_scaling"):
        assert not got[k][retired].any(), k  # exactly zero, no NaN from sigmoid'
    if not fx["radii"].any():
        assert got["L_opacity_radii"] == 0.0 and not got["g_opacity_radii"].any()


@pytest.mark.parametrize("name", rc.IMAGE_FIXTURES)
def test_render_terms_against_the_reference_fixtures(dev, name):
    fx = rc.load(name)
    a, c, up = rc.image_inputs(fx)
    got = run_image(a, c, up, dev)
    rc.compare(got, {k: fx[k + "@64"] for k in rc.IMAGE_KEYS}, rc.image_bounds(a, c, up), rc.IMAGE_KEYS, rc.KERNEL_FACTOR, name + " HIP")
    if name == "image_flat_9x16":
        assert got["L_TV_altitude"] == 0.0 and not got["g_altitude"].any()  # sign(0) = 0


@pytest.mark.parametrize("kind", ("isotropic", "disk", "loguniform"))
@pytest.mark.parametrize("P", (1_000_000, 2_000_000))
def test_gaussian_terms_at_full_size(dev, kind, P):
    g = torch.Generator().manual_seed(P // 1000 + len(kind))
    o, l, r = rc.opacity_logits(P, g), rc.log_scales(kind, P, g), rc.radii_mix(P, g)
    n0, up = 1_500_000, (0.75, -1.25, 2.5)
    got = run_gauss(o, l, r, n0, up, dev)
    want = rc.restate_gauss(o, l, r, n0, up, torch.float64)
    b = rc.gauss_bounds(o, l, r, n0, up)
    print(f"{kind} {P}: {int(b['excusable'].sum())} rows inside the fp32 error of a decision")
    rc.compare(got, want, b, rc.GAUSS_KEYS, rc.KERNEL_FACTOR, f"{kind} {P} HIP", excuse_rows=True)


@pytest.mark.parametrize("H,W", ((1024, 1024), (2048, 2048)))
def test_render_terms_at_full_size(dev, H, W):
    g = torch.Generator().manual_seed(H)
    a, c, up = rc.altitude_image(H, W, g), rc.accumulated_image(H, W, g), (0.875, -1.75)
    got = run_image(a, c, up, dev)
    rc.compare(got, rc.restate_image(a, c, up, torch.float64), rc.image_bounds(a, c, up), rc.IMAGE_KEYS, rc.KERNEL_FACTOR, f"{H}x{W} HIP")


def test_weighted_total_and_single_planes(dev):
    """`total` is the weighted sum of the wanted terms, its gradient the weighted sum of theirs; a term that is not wanted
    is 0 and gets no gradient; the classes return the unweighted term."""
    from eogs2_amd import regularizers as R

    fx = rc.load("gauss_mix")
    o, l, r, n0, up = rc.gauss_inputs(fx)
    w = (0.1, 0.05, 0.02)
    od, ld, rd = o.to(dev).requires_grad_(True), l.to(dev).requires_grad_(True), r.to(dev)
    total, terms = R.gaussian_regularizers(od, ld, rd, n_init=n0, weights=w, want=ALL)
    t = terms.detach().cpu().numpy().astype(np.float64)
    assert abs(float(total.detach()) - float(np.dot(w, t))) <= 6 * rc.U * float(np.dot(w, np.abs(t)))  # the weights' rounding, 3 products, 2 sums
    g_o, g_l = torch.autograd.grad(total, (od, ld))
    b = rc.gauss_bounds(o, l, r, n0, (1.0, 1.0, 1.0))
    want_o = w[0] * fx["g_opacity_op@64"] / float(up[0]) + w[1] * fx["g_opacity_radii@64"] / float(up[1])
    bound_o = w[0] * b["g_opacity_op"] + w[1] * b["g_opacity_radii"] + 2 * rc.U * np.abs(want_o)
    assert (np.abs(g_o.cpu().numpy() - want_o) <= rc.KERNEL_FACTOR * bound_o).all()
    ok = ~b["excusable"]
    want_l = w[2] * fx["g_scaling@64"] / float(up[2])
    assert (np.abs(g_l.cpu().numpy() - want_l)[ok] <= rc.KERNEL_FACTOR * (w[2] * b["g_scaling"] + 2 * rc.U * np.abs(want_l))[ok]).all()
    # erank alone: the opacity terms are 0, the logits get exact zeros; as a dict, as a device tensor
    for weights in ({"erank": 0.02}, torch.tensor([7.0, 7.0, 0.02], device=dev)):
        od.grad = ld.grad = None
        tot2, terms2 = R.gaussian_regularizers(od, ld, n_init=n0, weights=weights, want=("erank",))
        assert terms2[:2].tolist() == [0.0, 0.0] and float(terms2[2].detach()) == float(terms[2].detach())
        assert float(tot2.detach()) == float(torch.tensor(0.02) * terms[2].detach())
        tot2.backward()
        assert not bool(od.grad.any()) and torch.equal(ld.grad, g_l)
    # the classes: the reference's call signatures, the unweighted term
    m = types.SimpleNamespace(_opacity=od, _scaling=ld)
    assert float(R.OpacityLoss(0.1, n0)(m)) == float(terms[0]) and float(R.radiiOpacityLoss(0.1, n0)(m, rd)) == float(terms[1])
    assert float(R.erankLoss(0.1)(m)) == float(terms[2])
    assert float(R.radiiOpacityLoss(0.1, n0)(m, rd.long())) == float(terms[1])  # (radii of any integer dtype)
    fi = rc.load("image_24x37")
    a, c, _ = rc.image_inputs(fi)
    ad, cd = a.to(dev).requires_grad_(True), c.to(dev).requires_grad_(True)
    both, bt = R.render_regularizers(ad, cd, weights=(0.3, 0.7))
    g_a, g_c = torch.autograd.grad(both, (ad, cd))
    tv, ao = R.Total_variation(0.3)(ad[None]), R.AccumulatedOpacity(0.7)(cd)
    assert float(tv) == float(bt[0]) and float(ao) == float(bt[1])
    g_a1, = torch.autograd.grad(0.3 * tv, ad)
    g_c1, = torch.autograd.grad(0.7 * ao, cd)
    assert torch.allclose(g_a, g_a1, rtol=1e-6, atol=0) and torch.allclose(g_c, g_c1, rtol=1e-6, atol=0)


def _step(R, od, ld, rd, n0, weights, ad, cd, iw):
    od.grad = ld.grad = ad.grad = cd.grad = None
    total, terms = R.gaussian_regularizers(od, ld, rd, n_init=n0, weights=weights, want=ALL)
    itot, iterms = R.render_regularizers(ad, cd, weights=iw)
    (total + itot).backward()
    return total.detach(), terms.detach(), itot.detach(), iterms.detach(), od.grad, ld.grad, ad.grad, cd.grad


def test_reproducible_bit_for_bit_and_on_a_side_stream(dev):
    from eogs2_amd import regularizers as R

    g = torch.Generator().manual_seed(7)
    P = 300_000
    od = rc.opacity_logits(P, g).to(dev).requires_grad_(True)
    ld = rc.log_scales("loguniform", P, g).to(dev).requires_grad_(True)
    rd = rc.radii_mix(P, g).to(dev)
    ad = rc.altitude_image(500, 700, g).to(dev).requires_grad_(True)
    cd = rc.accumulated_image(500, 700, g).to(dev).requires_grad_(True)
    w, iw = torch.tensor([0.1, 0.05, 0.02], device=dev), torch.tensor([0.3, 0.7], device=dev)
    first = [t.clone() for t in _step(R, od, ld, rd, P, w, ad, cd, iw)]
    for _ in range(3):
        again = _step(R, od, ld, rd, P, w, ad, cd, iw)
        assert all(torch.equal(x, y) for x, y in zip(first, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = [t.clone() for t in _step(R, od, ld, rd, P, w, ad, cd, iw)]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_weights_flipped_between_replays_of_one_graph(dev):
    """The step is recorded once; the weights are rewritten in the device tensor between replays (a term switched on at
    iteration > iterstart_*): every replay gives, bit for bit, what an eager run with those weights gives."""
    from eogs2_amd import regularizers as R

    g = torch.Generator().manual_seed(11)
    P = 50_000
    od = rc.opacity_logits(P, g).to(dev).requires_grad_(True)
    ld = rc.log_scales("disk", P, g).to(dev).requires_grad_(True)
    rd = rc.radii_mix(P, g).to(dev)
    ad = rc.altitude_image(96, 120, g).to(dev).requires_grad_(True)
    cd = rc.accumulated_image(96, 120, g).to(dev).requires_grad_(True)
    w, iw = torch.tensor([0.1, 0.0, 0.0], device=dev), torch.tensor([0.0, 0.0], device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(R, od, ld, rd, P, w, ad, cd, iw)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rec = _step(R, od, ld, rd, P, w, ad, cd, iw)
    seen = []
    for gw, gi in (((0.1, 0.0, 0.0), (0.0, 0.0)), ((0.1, 0.0, 0.02), (0.3, 0.0)), ((0.0, 0.05, 0.0), (0.0, 0.7)), ((0.1, 0.0, 0.0), (0.0, 0.0))):
        w.copy_(torch.tensor(gw))
        iw.copy_(torch.tensor(gi))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in rec]
        od2, ld2, ad2, cd2 = (t.detach().clone().requires_grad_(True) for t in (od, ld, ad, cd))
        eager = _step(R, od2, ld2, rd, P, gw, ad2, cd2, gi)  # Python floats: the cached device tensor of these values
        assert all(torch.equal(x, y) for x, y in zip(replayed, eager)), (gw, gi)
        seen.append((float(replayed[0]), float(replayed[2]), bool(replayed[5].any()), bool(replayed[6].any())))
    assert seen[0] == seen[3] and seen[0][2:] == (False, False) and seen[1][2:] == (True, True) and seen[2][2:] == (False, False)
    assert len({s[0] for s in seen[:3]}) == 3  # the switch changed the result


def test_retired_rows_equal_the_compacted_model(dev):
    from eogs2_amd import regularizers as R
    from eogs2_amd.optim import RETIRED_LOGIT

    g = torch.Generator().manual_seed(13)
    P = 200_000
    o, l, r = rc.opacity_logits(P, g), rc.log_scales("loguniform", P, g), rc.radii_mix(P, g)
    l[::5] = rc.log_scales("isotropic", (P + 4) // 5, g)
    retired = torch.rand(P, generator=g) < 0.3
    o[retired] = RETIRED_LOGIT
    l[retired.nonzero().reshape(-1)[::2]] = float("nan")  # whatever a parked row holds must not matter
    w = torch.tensor([0.1, 0.05, 0.02], device=dev)

    def grads(o_, l_, r_):
        od, ld = o_.to(dev).requires_grad_(True), l_.to(dev).requires_grad_(True)
        total, terms = R.gaussian_regularizers(od, ld, r_.to(dev), n_init=150_000, weights=w, want=ALL)
        total.backward()
        return total.detach(), terms.detach(), od.grad, ld.grad

    tot_f, terms_f, go_f, gl_f = grads(o, l, r)
    keep = ~retired
    tot_c, terms_c, go_c, gl_c = grads(o[keep], l[keep], r[keep])
    kd = keep.to(dev)
    assert bool(torch.isfinite(terms_f).all()) and bool(torch.isfinite(go_f).all()) and bool(torch.isfinite(gl_f).all())
    assert not bool(go_f[~kd].any()) and not bool(gl_f[~kd].any())  # zero gradient, exactly
    assert torch.equal(go_f[kd], go_c) and torch.equal(gl_f[kd], gl_c)  # the survivors': bit for bit those of the compacted model
    # zero contribution: the same addends in another partition of the grid, so the float64 sums agree to the last float32 bit or so
    assert torch.allclose(terms_f, terms_c, rtol=4 * rc.U, atol=0) and abs(float(tot_f) - float(tot_c)) <= 8 * rc.U * abs(float(tot_c))
    # every row retired: the terms are 0 and nothing is NaN
    tot0, terms0, go0, gl0 = grads(torch.full((1000, 1), RETIRED_LOGIT), l[:1000], r[:1000])
    assert terms0.tolist() == [0.0, 0.0, 0.0] and float(tot0) == 0.0 and not bool(go0.any()) and not bool(gl0.any())


def _example(args):
    """One run of the example in a process of its own, under its own time limit; (losses, Gaussians at the end)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), *args], capture_output=True, text=True,
                       timeout=420, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = re.findall(r"iter\s+(\d+)\s+loss\s+(\S+)\s+gaussians\s+(\d+)", p.stdout)
    assert rows, p.stdout[-2000:]
    return [float(x[1]) for x in rows], int(rows[-1][2])


def test_example_with_the_shipped_opacity_weight(dev):
    base = ["--gaussians", "20000", "--size", "160", "--iters", "100", "--prune-every", "25", "--graph", "--defer-prune", "4"]
    plain_losses, plain_kept = _example(base)
    losses, kept = _example(base + ["--opacity-loss", "0.1"])
    assert all(np.isfinite(losses)) and all(np.isfinite(plain_losses))
    assert losses[0] > plain_losses[0]  # the term is there
    assert kept <= plain_kept, (kept, plain_kept)  # it pushes opacities down: no more Gaussians survive the prune than without it
    both_losses, _ = _example(base + ["--opacity-loss", "0.1", "--erank-loss", "0.01", "--parallel-renders"])
    assert all(np.isfinite(both_losses))
