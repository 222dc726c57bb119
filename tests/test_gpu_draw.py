"""GPU (MI355X): the per-iteration draws (include/eogs_draw.h, eogs2_amd.draw).

What is tested, and against what:

* the known answer: seed 0, iteration 0, slot 0 gives `(w >> 8) * 2^-24` of the first Random123 vector, bit for bit;
* bit equality with the Python-integer restatement (`draws_for`) for every legal flag combination, one and eight cameras,
  iterations 0, 1, 2^32 - 1, 2^32 (the carry into counter word 1) and 2^63 - 1, seeds 0 and 2^64 - 1: the uniforms, the
  copied and fixed entries of `virt_affine` and `cam2virt`, and what the flags say is left alone (outputs start as a
  sentinel NaN);
* the normals: each `shear` within one fp32 ulp of `float32(host normal) * extent` (the device's double log / sin / cos may
  differ from libm's in the last place, which moves the float rounding by one ulp at most) and never beyond the extent;
* the matrices against float64 over the device's own shear: an fma is one rounding, so |new_A - exact| <= 1 ulp, and
  |new_b[i] - exact| <= 2 u (|b_i| + 4 |d_i| sum_j |A[2][j] c_j|) (tests/draw_cases.py: camera_exact);
* against the reference's own `sample_random_camera` and `get_nadir_camera` (tests/golden/draw/*.npz, whose planted normals
  are the draws of a stored (seed, iteration, slot): the device is run at that very position, so it draws what was planted):
  `cam2virt` bit for bit at scale 1, `new_b` within twice the bound above (both are valid fp32 evaluations), and new_A
  within 2 u (|d A[2][j]| + 2 |exact|) — the reference's matmul rounds the product and the sum, the fma the sum alone, doubled;
* NADIR at its edges, the gate, a stream on a schedule's cursor, and a GraphedStep that is recorded once and replayed.
"""
import os

import numpy as np
import pytest
import torch

import draw_cases as DC

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5EA75  # a quiet NaN with a payload: an output element no launch wrote


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def _gate(dev, a, b):
    return torch.tensor([a, b], dtype=torch.int32, device=dev).view(torch.uint32)


def _sentinel(shape, dev):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _u32(t):
    return [int(x) & 0xFFFFFFFF for x in DC.bits(t).tolist()]


# (bg, copy_first, camera): every legal combination of the four flags
COMBOS = [(bg, first, cam) for bg, first in ((False, False), (True, False), (True, True)) for cam in (None, "camera", "nadir")
          if bg or cam]
assert len(COMBOS) == 8
EXTENTS = (0.02, 1.0, 350.0, 1e-3, 0.5, 0.02, 3.0, 0.25)  # per slot
SCALES = (1.0, 350.0, 1.0, 2.5, 1.0, 350.0, 0.0, 1.0)
KINDS = ("well", "utm", "zero_center", "utm", "well", "zero_center", "utm", "well")


class Cam:
    """One camera's tensors on the device, outputs filled with the sentinel, and its keyword arguments."""

    def __init__(self, dev, combo, slot, alt_floor=True, affine=None, center=None):
        self.bg_on, self.first, self.cam = combo
        self.slot = slot
        a, c = DC.camera_inputs(KINDS[slot], slot)
        self.affine_np = a if affine is None else affine
        self.center_np = c if center is None else center
        self.affine, self.center = torch.from_numpy(self.affine_np).to(dev), torch.from_numpy(self.center_np).to(dev)
        self.alt = torch.tensor([-17.25 - slot], device=dev) if (alt_floor and self.bg_on) else None
        self.bg, self.virt, self.c2v, self.shear = (_sentinel(s, dev) for s in ((5,), (4, 4), (3, 3), (2,)))
        self.extent, self.scale = EXTENTS[slot], SCALES[slot]

    def add_to(self, draws):
        kw = {}
        if self.bg_on:
            kw.update(bg=self.bg, copy_first=self.first)
        if self.cam:
            kw.update(virt_affine=self.virt, cam2virt=self.c2v, shear=self.shear, cam2virt_scale=self.scale)
            kw.update(nadir=True) if self.cam == "nadir" else kw.update(extent=self.extent)
        return draws.add_camera(self.affine, self.center, self.alt, **kw)

    def check(self, seed, iteration, slot):
        """Everything that must hold bit for bit, plus the normals' and the matrices' bounds."""
        from eogs2_amd.draw import draws_for

        uniforms, normals = draws_for(seed, iteration, slot)
        where = (seed, iteration, slot, self.bg_on, self.first, self.cam)
        bg = _u32(self.bg)
        if self.bg_on:
            want = [uniforms[0]] * 3 if self.first else list(uniforms)
            assert bg[:3] == [DC.f32_bits(u) for u in want], where
            assert bg[3] == (DC.f32_bits(float(self.alt.cpu())) if self.alt is not None else SENTINEL), where  # given, or left alone
            assert bg[4] == 0, where
        else:
            assert bg == [SENTINEL] * 5, where
        if not self.cam:
            assert _u32(self.virt) == [SENTINEL] * 16 and _u32(self.c2v) == [SENTINEL] * 9 and _u32(self.shear) == [SENTINEL] * 2, where
            return
        d = self.shear.cpu().numpy()
        a = self.affine_np
        if self.cam == "camera":
            for i in (0, 1):
                want = float(np.float32(normals[i]) * np.float32(self.extent))
                assert abs(float(d[i]) - want) <= DC.ulp(want), (where, i, float(d[i]), want)
                assert abs(float(d[i])) <= float(np.float32(self.extent)), (where, i)
        else:
            with np.errstate(all="ignore"):
                want = -(a[2, :2] / a[2, 2])  # fp32, correctly rounded on both sides
            assert _u32(self.shear) == [DC.f32_bits(float(x)) for x in want], where
        va_fixed, c2v_want = DC.restated_matrices(a, d, self.scale)
        va = self.virt.cpu().numpy()
        fixed = ~np.isnan(va_fixed)
        assert (va.view(np.int32)[fixed] == va_fixed.view(np.int32)[fixed]).all(), where
        assert (self.c2v.cpu().numpy().view(np.int32) == c2v_want.view(np.int32)).all(), where  # (the shear entries: d * scale in fp32)
        new_A, new_b, bound = DC.camera_exact(a, self.center_np, d)
        got_A, got_b = va[:3, :3].T.astype(np.float64), va[3, :3].astype(np.float64)
        for i in (0, 1):
            for j in range(3):
                assert abs(got_A[i, j] - new_A[i, j]) <= DC.ulp(new_A[i, j]), (where, i, j, got_A[i, j], new_A[i, j])
            assert abs(got_b[i] - new_b[i]) <= bound[i], (where, i, got_b[i], new_b[i], bound[i])
        if self.cam == "nadir":  # the shear cancels column 2 of rows 0 and 1
            for i in (0, 1):
                assert abs(got_A[i, 2]) <= DC.ulp(float(a[2, i])), (where, i, got_A[i, 2])


def _launch(dev, seed, iteration, cams):
    from eogs2_amd.draw import DrawStream, IterationDraws

    stream = DrawStream(seed, device=dev)
    stream.seek(iteration)
    draws = IterationDraws(stream)
    for c in cams:
        c.add_to(draws)
    draws.draw()
    torch.cuda.synchronize()
    assert stream.position() == iteration  # a draw moves nothing
    return stream, draws


def test_known_answer(dev):
    cam = Cam(dev, (True, False, None), 0)
    _launch(dev, 0, 0, [cam])
    assert _u32(cam.bg)[:3] == [DC.f32_bits((w >> 8) * 2.0 ** -24) for w in DC.KAT[0][2][:3]]
    assert _u32(cam.bg)[:3] == [0x3ECC4FD0, 0x3F6169C5, 0x3F3C57AC]  # 0x6627e8 / 2^24, 0xe169c5 / 2^24, 0xbc57ac / 2^24 as fp32


@pytest.mark.parametrize("seed", DC.SEEDS)
@pytest.mark.parametrize("iteration", DC.ITERATIONS)
def test_bit_equality_with_the_restatement(dev, seed, iteration):
    cams = [Cam(dev, combo, slot, alt_floor=slot % 2 == 0) for slot, combo in enumerate(COMBOS)]  # eight cameras, one launch
    _launch(dev, seed, iteration, cams)
    for slot, c in enumerate(cams):
        c.check(seed, iteration, slot)
    for k, combo in enumerate(COMBOS):  # one camera: slot 0 whatever the combination
        c = Cam(dev, combo, 0, alt_floor=k % 2 == 1)
        _launch(dev, seed, iteration, [c])
        c.check(seed, iteration, 0)


def test_normals_over_512_launches(dev):
    from eogs2_amd.draw import DrawStream, IterationDraws, draws_for

    seed, n = 0x0123456789ABCDEF, 512
    stream = DrawStream(seed, device=dev)
    draws = IterationDraws(stream)
    shear = torch.zeros(8, 2, device=dev)
    affine = torch.from_numpy(DC.camera_inputs("well")[0]).to(dev)
    for slot in range(8):
        draws.add_camera(affine, None, shear=shear[slot], extent=EXTENTS[slot])
    start = 2 ** 32 - 256  # across the carry
    out = torch.zeros(n, 8, 2, device=dev)
    for k in range(n):
        stream.seek(start + k)
        draws.draw()
        out[k].copy_(shear)
    out = out.cpu().numpy()
    clipped = 0
    for k in range(n):
        for slot in range(8):
            normals = draws_for(seed, start + k, slot)[1]
            for i in (0, 1):
                want = float(np.float32(normals[i]) * np.float32(EXTENTS[slot]))
                got = float(out[k, slot, i])
                assert abs(got - want) <= DC.ulp(want), (k, slot, i, got, want)
                assert abs(got) <= float(np.float32(EXTENTS[slot])), (k, slot, i)
                clipped += abs(normals[i]) == 1.0
    share = clipped / (n * 16)
    assert abs(share - 0.3173) <= 5 * (0.3173 * 0.6827 / (n * 16)) ** 0.5, share  # the clip is exercised, at its rate


def test_distinct_streams(dev):
    from eogs2_amd.draw import DrawStream, IterationDraws, block_for, uniform_of

    seeds = (0, 1, 2 ** 63, 2 ** 64 - 1, 0xDEADBEEF)
    iterations = [0, 1, 2, 3, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 33, 2 ** 40 + 5] + [1000 + 17 * k for k in range(16)]
    assert len(seeds) * len(iterations) * 8 == 1000
    affine = torch.from_numpy(DC.camera_inputs("well")[0]).to(dev)
    rows = []
    for seed in seeds:
        stream = DrawStream(seed, device=dev)
        draws = IterationDraws(stream)
        bg, shear = torch.zeros(8, 5, device=dev), torch.zeros(8, 2, device=dev)
        for slot in range(8):
            draws.add_camera(affine, None, bg=bg[slot], shear=shear[slot], extent=1.0)
        for it in iterations:
            stream.seek(it)
            draws.draw()
            b, s = bg.cpu(), shear.cpu()
            for slot in range(8):
                rows.append((seed, it, slot, tuple(_u32(b[slot, :3])), tuple(s[slot].tolist())))
    assert len({r[3] for r in rows}) == 1000  # seeds, iterations and slots: no two background blocks collide
    free = [r[4] for r in rows if abs(r[4][0]) < 1.0 and abs(r[4][1]) < 1.0]
    assert len(free) > 300 and len(set(free)) == len(free)  # nor two shear blocks (where the clip left both normals alone)
    for seed, it, slot, got_bg, _ in rows:  # the purposes: the background is block 0 of its position, not block 1
        assert got_bg == tuple(DC.f32_bits(uniform_of(w)) for w in block_for(seed, it, slot, 0)[:3])
        assert got_bg != tuple(DC.f32_bits(uniform_of(w)) for w in block_for(seed, it, slot, 1)[:3])


@pytest.mark.parametrize("name", ["well_first", "well_extent1", "utm_carry", "utm_extent1", "zero_center", "zero_center_extent1"])
def test_against_the_references_fixtures(dev, name):
    from eogs2_amd.draw import DrawStream, IterationDraws, draws_for

    f = np.load(os.path.join(DC.GOLDEN, name + ".npz"))
    seed, iteration, slot, extent = int(f["seed"]), int(f["iteration"]), int(f["slot"]), float(f["extent"])
    assert tuple(np.float32(z) for z in draws_for(seed, iteration, slot)[1]) == tuple(f["normals"])  # what was planted is that draw
    a, c = f["affine"], f["center"]
    affine, center = torch.from_numpy(a).to(dev), torch.from_numpy(c).to(dev)
    stream = DrawStream(seed, device=dev)
    stream.seek(iteration)
    draws = IterationDraws(stream)
    for k in range(slot):  # the slots before it
        draws.add_camera(None, None, bg=torch.zeros(5, device=dev))
    virt, c2v, shear = (_sentinel(s, dev) for s in ((4, 4), (3, 3), (2,)))
    assert draws.add_camera(affine, center, virt_affine=virt, cam2virt=c2v, shear=shear, extent=extent, cam2virt_scale=1.0) == slot
    draws.draw()
    nstream = DrawStream(seed, device=dev)
    ndraws = IterationDraws(nstream)
    nvirt, nc2v = _sentinel((4, 4), dev), _sentinel((3, 3), dev)
    ndraws.add_camera(affine, center, virt_affine=nvirt, cam2virt=nc2v, nadir=True)
    ndraws.draw()
    for nadir, got_va, got_m, ref_va, ref_m in ((False, virt, c2v, f["new_affine"], f["myM"]), (True, nvirt, nc2v, f["nadir_affine"], f["nadir_myM"])):
        got_va, got_m = got_va.cpu().numpy(), got_m.cpu().numpy()
        assert (got_m.view(np.int32) == ref_m.view(np.int32)).all(), (name, got_m, ref_m)  # cam2virt: bit for bit at scale 1
        d = ref_m[:2, 2]
        new_A, new_b, bound = DC.camera_exact(a, c, d)
        fixed = ~np.isnan(DC.restated_matrices(a, d, 1.0)[0])
        assert (got_va.view(np.int32)[fixed] == ref_va.view(np.int32)[fixed]).all(), name  # copied and fixed entries
        A = a.astype(np.float64)[:3, :3].T
        for i in (0, 1):
            assert abs(float(got_va[3, i]) - float(ref_va[3, i])) <= 2 * bound[i], (name, i, got_va[3, i], ref_va[3, i], bound[i])
            for j in range(3):
                tol = 2 * DC.U * (abs(float(d[i]) * A[2, j]) + 2 * abs(new_A[i, j]))
                if nadir and j == 2:  # a cancellation: the reference keeps two roundings of A[i][2] (product, quotient), the fma one
                    tol = 3 * DC.ulp(A[i, 2])
                assert abs(float(got_va[j, i]) - float(ref_va[j, i])) <= tol, (name, i, j, got_va[j, i], ref_va[j, i], tol)


def test_nadir_at_its_edges(dev):
    base, center = DC.camera_inputs("well", 0)
    # A[2][2] == 0: the float division's infinities (and 0 / 0 = NaN) go through the formula as they are
    for a02, a12 in ((0.75, -0.5), (0.0, 0.25)):
        a = base.copy()
        a[2, 0], a[2, 1], a[2, 2] = a02, a12, 0.0
        cam = Cam(dev, (False, False, "nadir"), 0, affine=a, center=center)
        _launch(dev, 3, 5, [cam])
        d = cam.shear.cpu().numpy()
        with np.errstate(all="ignore"):
            want = -(a[2, :2] / a[2, 2])
        assert not np.isfinite(want).any()
        assert (np.isnan(d) == np.isnan(want)).all() and (d[~np.isnan(want)] == want[~np.isnan(want)]).all(), (d, want)
        va = cam.virt.cpu().numpy().astype(np.float64)
        A, b, c = a.astype(np.float64)[:3, :3].T, a.astype(np.float64)[3, :3], center.astype(np.float64)
        with np.errstate(all="ignore"):
            for i in (0, 1):
                di = float(want[i])
                for j in range(3):
                    ref = di * A[2, j] + A[i, j]  # inf * 0 = NaN, inf * x = +-inf: classes no rounding changes
                    assert (np.isnan(ref) and np.isnan(va[j, i])) or ref == va[j, i], (i, j, ref, va[j, i])
                ref = -di * float(A[2] @ c) + b[i]
                assert (np.isnan(ref) and np.isnan(va[3, i])) or ref == va[3, i], (i, ref, va[3, i])
        assert (cam.virt.cpu().numpy()[:, 2] == a[:, 2]).all()  # row 2 of A and b[2]: copied
    # a NaN in A stays a NaN where it enters, and nowhere else
    for cam_kind in ("nadir", "camera"):
        a = base.copy()
        a[1, 0] = np.nan  # A[0][1]
        cam = Cam(dev, (False, False, cam_kind), 0, affine=a, center=center)
        _launch(dev, 3, 5, [cam])
        va = cam.virt.cpu().numpy()
        assert np.isnan(va[1, 0]) and np.isnan(va).sum() == 1, va
        a = base.copy()
        a[0, 2] = np.nan  # A[2][0]: into both sheared rows' column 0 and, through s, into both intercepts
        cam = Cam(dev, (False, False, cam_kind), 0, affine=a, center=center)
        _launch(dev, 3, 5, [cam])
        va = cam.virt.cpu().numpy()
        nan_at = {(int(r), int(c)) for r, c in zip(*np.nonzero(np.isnan(va)))}
        assert nan_at == {(0, 0), (0, 1), (0, 2), (3, 0), (3, 1)}, nan_at


def test_gate_and_advance(dev):
    from eogs2_amd.draw import DrawStream, IterationDraws, draws_for
    from eogs2_amd.views import ViewSchedule

    stream = DrawStream(11, device=dev)
    draws = IterationDraws(stream)
    bg = torch.zeros(5, device=dev)
    draws.add_camera(None, None, bg=bg)

    def drawn():
        draws.draw()
        return _u32(bg)[:3]

    want = lambda it: [DC.f32_bits(u) for u in draws_for(11, it, 0)[0]]  # noqa: E731
    stream.seek(41)
    assert drawn() == want(41)
    stream.advance(_gate(dev, 0, 1))  # closed: the counter and the next draws stay
    assert stream.position() == 41 and drawn() == want(41)
    stream.advance(_gate(dev, 1, 0))  # open: one on
    assert stream.position() == 42 and drawn() == want(42)
    stream.advance()
    assert stream.position() == 43 and drawn() == want(43)
    stream.seek(2 ** 32 - 1)
    stream.advance()
    assert stream.position() == 2 ** 32 and drawn() == want(2 ** 32)
    sd = stream.state_dict()
    other = DrawStream(11, device=dev)
    other.load_state_dict(sd)
    assert other.position() == 2 ** 32 and other.state_dict() == sd
    # a stream on a schedule's cursor follows the schedule, gate included
    sched = ViewSchedule([0, 1, 0], 2, dev)
    shared = DrawStream(11, counter=sched.cursor)
    sdraws = IterationDraws(shared)
    sdraws.add_camera(None, None, bg=bg)
    with pytest.raises(RuntimeError, match="owner advances"):
        shared.advance()
    for k in range(5):
        sdraws.draw()
        assert _u32(bg)[:3] == want(k) and shared.position() == sched.position() == k
        sched.advance(_gate(dev, 0, 1))
        sdraws.draw()
        assert _u32(bg)[:3] == want(k) and sched.position() == k
        sched.advance(_gate(dev, 1, 0) if k % 2 else None)


def test_recorded_step_draws_anew_on_every_replay(dev):
    from eogs2_amd.draw import DrawStream, IterationDraws, draws_for
    from eogs2_amd.graph import GraphedStep
    from eogs2_amd.views import ViewBank, ViewSchedule

    V, order, seed, extent = 3, [2, 0, 1, 1, 2, 0], 77, 0.02
    inputs = [DC.camera_inputs(("well", "utm", "zero_center")[v], v) for v in range(V)]
    floors = [torch.tensor([0.5, 0.5, 0.5, -30.0 - v, 9.0]) for v in range(V)]

    def make():
        sched = ViewSchedule(order, V, dev)
        bank = ViewBank(sched)
        affine, center, bg = torch.zeros(4, 4, device=dev), torch.zeros(3, device=dev), torch.zeros(5, device=dev)
        bank.add_input("affine", affine, [torch.from_numpy(a).to(dev) for a, _ in inputs])
        bank.add_input("center", center, [torch.from_numpy(c).to(dev) for _, c in inputs])
        bank.add_input("bg", bg, [t.to(dev) for t in floors])  # bg[3]: the view's own floor, which the draw leaves alone
        virt, c2v = torch.zeros(4, 4, device=dev), torch.zeros(3, 3, device=dev)
        draws = IterationDraws(DrawStream(seed, counter=sched.cursor))
        draws.add_camera(affine, center, bg=bg, virt_affine=virt, cam2virt=c2v, extent=extent, cam2virt_scale=350.0)

        def fn():
            bank.load()
            draws.draw()
            out = torch.cat((bg, virt.reshape(-1), c2v.reshape(-1))) * 1.0  # a trivial use of the outputs
            sched.advance()
            return out

        return sched, fn

    sched, fn = make()
    eager = [fn().cpu() for _ in range(6)]
    assert sched.position() == 6
    sched, fn = make()
    step = GraphedStep(fn, warmup=1)  # (the warm-up run is a real iteration: cursor 0 -> 1)
    assert sched.position() == 1
    sched.seek(0)
    replayed = [step().cpu().clone() for _ in range(6)]
    assert step.recaptures == 0 and step.replays == 6 and sched.position() == 6  # recorded once
    for k in range(6):
        assert DC.same_bits(eager[k], replayed[k]), k
        uniforms, normals = draws_for(seed, k, 0)
        v = order[k]
        got = replayed[k]
        assert _u32(got[:3]) == [DC.f32_bits(u) for u in uniforms], k
        assert float(got[3]) == -30.0 - v and float(got[4]) == 0.0, k
        va, m = got[5:21].reshape(4, 4).numpy(), got[21:30].reshape(3, 3).numpy()
        d = [float(np.float32(z) * np.float32(extent)) for z in normals]
        fixed, _ = DC.restated_matrices(inputs[v][0], d, 350.0)
        keep = ~np.isnan(fixed)
        assert (va.view(np.int32)[keep] == fixed.view(np.int32)[keep]).all(), k
        new_A, new_b, bound = DC.camera_exact(inputs[v][0], inputs[v][1], d)
        for i in (0, 1):
            assert abs(float(m[i, 2]) - d[i] * 350.0) <= 350.0 * DC.ulp(d[i]) + DC.ulp(d[i] * 350.0), (k, i)
            assert abs(float(va[3, i]) - new_b[i]) <= bound[i] + DC.ulp(d[i]) * abs(float(inputs[v][0].astype(np.float64)[:3, 2] @ inputs[v][1])), (k, i)
    assert len({tuple(_u32(r[:3])) for r in replayed}) == 6  # another background on every replay
