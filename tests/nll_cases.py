"""The cases of the transient-uncertainty term (eogs2_amd.uncertainty, include/eogs_nll.h): seeded inputs, the float64
restatement of train_pan.py:434-440 in numpy, and the DERIVED bound of its results, shared by tests/golden/make_golden_nll.py,
tests/test_nll_api.py (CPU) and tests/test_gpu_nll.py.

The bound (E = 2^-24; the reference is the float64 evaluation on the float32 inputs, s and v formed in float64; every element
is compared):

  loss              |d| <= 8 E R(0.5 (1 + |log vc| + r^2 / vc)) + E |ref|          R: the loss's own mean or sum
  g_input           |d| <= 8 E |ref|
  g_var, g_mask     |d| <= 8 E sum_planes |k| / N 0.5 (1 / vc + r^2 / vc^2)  (x 2 s in mask mode): relative to the sum of
                    magnitudes, the two terms cancel where r^2 ~ v; exactly 0 outside [0, 1]
  mean, std         within 4 E relative; the std of a constant mask exactly 0

`multiples` returns, per quantity, the largest error in units of E x its magnitude: the bound is 8 (4 for the statistics).
"""
import os

import numpy as np

E = 2.0 ** -24
FLOOR, EPS = 1e-3, 1e-6
LIMIT = {"loss": 8.0, "g_input": 8.0, "g_vm": 8.0, "mean": 4.0, "std": 4.0}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nll")

# name -> kind ("mask": the transient mask; "var": the variance, `var_planes` of them), planes, H, W, seed, full, sum;
# scalars_only: a case kept for its multi-workgroup sums, whose file holds neither inputs nor gradients
CASES = {
    "mask_1x1x1": dict(kind="mask", planes=1, H=1, W=1, seed=11),
    "mask_3x37x53": dict(kind="mask", planes=3, H=37, W=53, seed=12),  # a tail, no whole vector, no whole wave
    "mask_1x64x64_constant": dict(kind="mask", planes=1, H=64, W=64, seed=13, constant=0.1),
    "mask_4x12x20": dict(kind="mask", planes=4, H=12, W=20, seed=14),
    "mask_2x300x300": dict(kind="mask", planes=2, H=300, W=300, seed=15, scalars_only=True),  # 88 workgroups of partials
    "var_shared_3x37x53": dict(kind="var", planes=3, H=37, W=53, seed=21, var_planes=1),
    "var_planes_3x37x53_full_sum": dict(kind="var", planes=3, H=37, W=53, seed=22, var_planes=3, full=True, sum=True),
    "var_planes_4x8x8_full": dict(kind="var", planes=4, H=8, W=8, seed=23, var_planes=4, full=True),
}
FIXTURES = tuple(CASES)
# GPU-only cases, checked against `restate` (tests/test_nll_api.py holds it against torch's float64 on the fixtures): no file
EXTRA = {
    # one negative variance: torch raises there, this package counts it and clamps it to eps (the stated deviation)
    "var_negative_2x5x7": dict(kind="var", planes=2, H=5, W=7, seed=31, var_planes=2, negative_at=17),
    # 257 workgroups of partials: the smallest H W at which the last workgroup's lanes take a second partial each
    "mask_1x481x545": dict(kind="mask", planes=1, H=481, W=545, seed=32),
    # more units than the forward's grid has lanes: the grid-stride loop takes a second trip
    "mask_1x1024x1028": dict(kind="mask", planes=1, H=1024, W=1028, seed=33),
}


def extra_inputs(name):
    c = dict(EXTRA[name])
    at = c.pop("negative_at", None)
    image, gt, vm = make_inputs(**c)
    if at is not None:
        vm.reshape(-1)[at] = np.float32(-0.25)
    return image, gt, vm
MASK_SPECIALS = (-0.5, -0.0, 0.0, 1.0, 1.5, 0.25, -1e-7, 1.0000001, 0.999)
VAR_SPECIALS = (0.0, 1e-8, EPS, 1.0)


def case(name):
    c = dict(full=False, sum=False, var_planes=1, constant=None, scalars_only=False)
    c.update(CASES[name])
    return c


def make_inputs(kind, planes, H, W, seed, var_planes=1, constant=None, **_):
    """image, gt [planes,H,W] and vm (mask [H,W] or var [H,W] / [planes,H,W]) as float32: residuals from 0 (exactly, at every
    seventh element) to 1 (exactly, at every eleventh), masks below, at, inside and above [0, 1]."""
    rs = np.random.RandomState(seed)
    gt = rs.uniform(0.0, 1.0, (planes, H, W)).astype(np.float32)
    r = (rs.uniform(0.0, 1.0, (planes, H, W)) * rs.choice([-1.0, 1.0], (planes, H, W))).reshape(-1)
    r[5::7] = 0.0
    r[3::11] = 1.0
    image = (gt.astype(np.float64) + r.reshape(planes, H, W)).astype(np.float32)
    image.reshape(-1)[5::7] = gt.reshape(-1)[5::7]  # residual exactly 0
    if kind == "mask":
        if constant is not None:
            vm = np.full((H, W), constant, np.float32)
        else:
            vm = rs.uniform(-0.3, 1.3, (H, W)).astype(np.float32)
            flat = vm.reshape(-1)
            if flat.size == 1:
                flat[0] = 0.3
            for i, s in enumerate(MASK_SPECIALS):
                flat[2 + i * 5::61] = np.float32(s)
    else:
        shape = (H, W) if var_planes == 1 else (var_planes, H, W)
        vm = rs.uniform(0.01, 2.0, shape).astype(np.float32)
        flat = vm.reshape(-1)
        for i, s in enumerate(VAR_SPECIALS):
            flat[1 + i * 3::13] = np.float32(s)
    return image, gt, vm


def inputs(name):
    return make_inputs(**case(name))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def restate(image, gt, vm, kind, full=False, sum=False, k=1.0, floor=FLOOR, eps=EPS, exclusive_clamp=False,  # noqa: A002
            zero_below_eps=False):
    """train_pan.py:434-440 (kind "mask") or gaussian_nll_loss (kind "var") in float64 on the float32 inputs, with the
    gradients for the upstream factor k on the loss and the magnitudes the bound is relative to. A negative variance is
    clamped to eps like any other below it (the stated deviation: torch raises). The two flags state WRONG rules, for the
    test that the bound rejects them: the clamp's gradient mask with exclusive bounds, d/dv zeroed below eps."""
    x, t, m = (np.asarray(a, np.float64) for a in (image, gt, vm))
    x, t = x.reshape((-1,) + x.shape[-2:]), t.reshape((-1,) + t.shape[-2:])
    if kind == "mask":
        m2 = m.reshape(m.shape[-2:])
        s = np.clip(m2, 0.0, 1.0) + floor
        v = (s * s)[None]
        inside = (m2 > 0.0) & (m2 < 1.0) if exclusive_clamp else (m2 >= 0.0) & (m2 <= 1.0)
        chain = 2.0 * s * inside
    else:
        v = m.reshape((-1,) + m.shape[-2:])
    with np.errstate(invalid="ignore", divide="ignore"):
        vc = np.broadcast_to(np.maximum(v, eps), x.shape)
        r = x - t
        l = 0.5 * (np.log(vc) + r * r / vc)
        lmag = 0.5 * (1.0 + np.abs(np.log(vc)) + r * r / vc)
        if full:
            l = l + 0.5 * np.log(2.0 * np.pi)
        N = l.size
        loss, loss_mag = (l.sum(), lmag.sum()) if sum else (l.mean(), lmag.mean())
        kn = float(k) / (1.0 if sum else N)
        g_input = kn * r / vc
        dv = kn * 0.5 * (1.0 / vc - r * r / (vc * vc))
        if zero_below_eps:
            dv = np.where(np.broadcast_to(v, x.shape) < eps, 0.0, dv)
        dmag = abs(kn) * 0.5 * (1.0 / vc + r * r / (vc * vc))
    if kind == "mask":
        g_vm, g_mag = dv.sum(0) * chain, dmag.sum(0) * chain
    elif v.shape[0] == 1:  # one variance shared by the planes
        g_vm, g_mag = dv.sum(0), dmag.sum(0)
    else:
        g_vm, g_mag = dv, dmag
    g_vm, g_mag = g_vm.reshape(m.shape), g_mag.reshape(m.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(((m - m.mean()) ** 2).sum() / (m.size - 1)) if m.size > 1 else np.float64("nan")
    return dict(loss=loss, g_input=g_input.reshape(np.shape(image)), g_vm=g_vm, mean=m.mean(), std=std, loss_mag=loss_mag,
                g_mag=g_mag, negative=float((m < 0).sum()) if kind == "var" else 0.0,
                clipped=float(((m < 0) | (m > 1)).sum()) if kind == "mask" else 0.0)


def _ratio(d, mag):
    """max |d| / (E mag) over the elements; an element of magnitude 0 must be exact (inf otherwise); NaN == NaN."""
    d, mag = np.abs(np.asarray(d, np.float64)).reshape(-1), np.abs(np.asarray(mag, np.float64)).reshape(-1)
    out = np.zeros_like(d)
    nz = mag > 0
    out[nz] = d[nz] / (E * mag[nz])
    out[~nz & (d != 0)] = np.inf
    out[np.isnan(d)] = np.inf
    return float(out.max()) if out.size else 0.0


def _diff(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got - ref
    return np.where(np.isnan(got) & np.isnan(ref), 0.0, d)  # (a NaN on one side only stays a NaN and fails)


def multiples(got, ref):
    """{quantity: the largest error in units of E x magnitude} for the quantities `got` holds (loss, g_input, g_vm, mean,
    std); `ref` is `restate`'s dict (or a fixture's float64 values beside its magnitudes)."""
    out = {}
    if "loss" in got:
        out["loss"] = _ratio(_diff(got["loss"], ref["loss"]), ref["loss_mag"] + abs(ref["loss"]) / 8.0)
    if "g_input" in got:
        out["g_input"] = _ratio(_diff(got["g_input"], ref["g_input"]), ref["g_input"])
    if "g_vm" in got:
        out["g_vm"] = _ratio(_diff(got["g_vm"], ref["g_vm"]), ref["g_mag"])
    for key in ("mean", "std"):
        if key in got:
            out[key] = _ratio(_diff(got[key], ref[key]), ref[key])
    return out


def check(got, ref, tag):
    """Asserts every quantity of `got` inside the bound; prints and returns the multiples reached."""
    mult = multiples(got, ref)
    print(f"{tag}: " + "  ".join(f"{k} {v:.3g} E" for k, v in mult.items()))
    for key, v in mult.items():
        assert v <= LIMIT[key], f"{tag}: {key} is {v:.4g} E x magnitude from the float64 reference, the bound is {LIMIT[key]:g}"
    return mult


def fixture_reference(name, fx=None):
    """(inputs, `restate`-shaped reference) of a fixture: the float64 values are torch's own (the file's @64 keys), the
    magnitudes the restatement's."""
    c = case(name)
    fx = load(name) if fx is None else fx
    image, gt, vm = inputs(name) if c["scalars_only"] else (fx["image"], fx["gt"], fx["vm"])
    ref = restate(image, gt, vm, c["kind"], c["full"], c["sum"])
    for key in ("loss", "mean", "std") + (() if c["scalars_only"] else ("g_input", "g_vm")):
        ref[key] = fx[key + "@64"]
    return (image, gt, vm), ref
