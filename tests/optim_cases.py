"""Shared by tests/golden/make_golden_optim.py, tests/test_optim_golden.py and tests/test_gpu_optim.py: the cases of the
optimizer / density-control lifecycle fixtures (tests/golden/optim/*.npz), the closed-form gradients every side feeds,
the reference's mask expressions, and the derived one-step error bound of fp32 Adam.

Nothing here is drawn from a random generator at test time. A gradient is a function of (iteration, the row's ORIGINAL id,
column), so a row keeps its gradient stream through prune, clone and split, the generator and the tests compute the same
values without storing 70 steps of [P, 14] arrays, and the float64 run of the generator sees the very same numbers.
"""
import json
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim")
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")  # the order of training_setup's list
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
# gs_config/train.yaml: position_lr_init, feature_lr (f_rest: / 20), opacity_lr, scaling_lr, rotation_lr, percent_dense
TRAIN_ARGS = dict(position_lr_init=1.6e-4, feature_lr=2.5e-3, opacity_lr=5e-2, scaling_lr=5e-3, rotation_lr=1e-3,
                  percent_dense=0.01)
BETAS, EPS = (0.9, 0.999), 1e-15  # torch.optim.Adam(l, lr=0.0, eps=1e-15)
MIN_OPACITY = -6.0  # train.yaml min_opacity: compared with the raw logit (train_pan.py:675)
DENSIFY_MIN_OPACITY = 0.005  # train_pan.py:703, compared with the activated opacity
RESET_CAP = 0.01
SPLIT_N = 2
MARGIN = 1e-3  # no thresholded quantity lies within this relative distance of its threshold, except the deliberate ties:
# the rows with id % 16 == 5 see the screen-space gradient (TIE_GRAD, 0, 0) in every iteration. Their mean gradient norm is
# TIE_GRAD exactly, in fp32 and in float64 on any device (a power of two: the norm, the sum and the quotient are exact), and
# TIE_GRAD is the gradient threshold of the cases (train.yaml has 2e-6 = 1.05 x 2^-19). They tell `>=` from `>`.
TIE_GRAD = 2.0 ** -19
MAX_FIXTURE_BYTES = 400 * 1024

# script: ("steps", n, with_stats) | ("tprune",) | ("reset",) | ("densify", max_screen_size)
CASES = {
    # (a) training as shipped (only_prune: True): steps, transparent prune, steps, opacity reset, steps
    "prune_only": dict(P=160, sh=0, seed=21, extent=5.0, grad_threshold=TIE_GRAD, opacity=(-9.0, 2.0),
                       script=[("steps", 25, False), ("tprune",), ("steps", 15, False), ("reset",), ("steps", 20, False)]),
    # (b) the full densify_and_prune, clone and split both selecting rows; max_screen_size None / set
    "densify": dict(P=128, sh=0, seed=12, extent=5.0, grad_threshold=TIE_GRAD, opacity=(-8.0, 3.0),
                    script=[("steps", 30, True), ("densify", None), ("tprune",), ("steps", 10, True)]),
    "densify_screen": dict(P=128, sh=0, seed=13, extent=5.0, grad_threshold=TIE_GRAD, opacity=(-8.0, 3.0),
                           script=[("steps", 30, True), ("densify", 20), ("tprune",), ("steps", 10, True)]),
    # (c) nothing selected anywhere: the split and clone masks, both prune masks are empty
    "empty_masks": dict(P=128, sh=0, seed=14, extent=5.0, grad_threshold=1.0, opacity=(-1.0, 3.0),
                        script=[("steps", 12, True), ("densify", None), ("tprune",), ("reset",), ("steps", 8, True)]),
    # (d) sh_degree 1: f_rest [P, 3, 3], a 36-byte row through compaction
    "sh1": dict(P=96, sh=1, seed=25, extent=5.0, grad_threshold=TIE_GRAD, opacity=(-8.0, 3.0),
                script=[("steps", 20, True), ("densify", 20), ("tprune",), ("reset",), ("steps", 10, True)]),
}


def shapes(sh):
    return {"xyz": (3,), "f_dc": (1, 3), "f_rest": ((sh + 1) ** 2 - 1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}


def lrs():
    a = TRAIN_ARGS
    return {"xyz": a["position_lr_init"], "f_dc": a["feature_lr"], "f_rest": a["feature_lr"] / 20.0, "opacity": a["opacity_lr"],
            "scaling": a["scaling_lr"], "rotation": a["rotation_lr"]}


# ---- closed-form inputs ----
def _mix(x):
    """splitmix64 finaliser on uint64 arrays (wraps)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _h(it, ids, col, salt):
    ids = np.asarray(ids, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = (np.uint64(it) * np.uint64(0x9E3779B97F4A7C15) + ids * np.uint64(0xC2B2AE3D27D4EB4F)
             + np.asarray(col, dtype=np.uint64) * np.uint64(0x165667B19E3779F9) + np.uint64(salt))
    return _mix(k)


def touched(it, ids):
    """Which rows a view touched in iteration `it`: a hashed half; the others get an exactly zero gradient."""
    return (_h(it, ids, 0, 7) >> np.uint64(17)) % np.uint64(2) == 0


VS_SALT = 7  # (chosen with the seeds of CASES: no mean gradient norm within MARGIN of the threshold)


def hashed_grad(it, ids, name, sh=0):
    """float32 tensor [K, *shape(name)]: the gradient of group `name` for the rows with original ids `ids` in iteration
    `it`. Every value is +-(1 + k / 16) * 2^e with k in 0..15 and e cycling over -27..7 (7.5e-9 .. 2.4e2), exact in fp32
    and in float64; untouched rows are zero in every group."""
    shp = shapes(sh)
    col0 = 0
    for n in GROUPS:
        if n == name:
            break
        col0 += int(np.prod(shp[n]))
    ids = np.asarray(ids, dtype=np.int64)
    ncol = int(np.prod(shp[name]))
    h = _h(it, ids[:, None], (col0 + np.arange(ncol))[None, :], 1)
    k = (h % np.uint64(16)).astype(np.float64)
    e = ((h >> np.uint64(8)) % np.uint64(35)).astype(np.int64) - 27
    sign = np.where((h >> np.uint64(20)) % np.uint64(2) == 0, 1.0, -1.0)
    g = sign * (1.0 + k / 16.0) * np.exp2(e.astype(np.float64))
    g = g * touched(it, ids)[:, None]
    g32 = g.astype(np.float32)
    assert np.array_equal(g32.astype(np.float64), g)
    return torch.from_numpy(g32.reshape((len(ids),) + shp[name]))


def viewspace_grad(it, ids):
    """float32 [K, 3]: the screen-space gradient add_densification_stats reads. A row's magnitude is 2^e(id), e in -26..-10,
    times (1 + k / 16) per iteration: the mean gradient norm of the rows spreads over five decades around the threshold."""
    ids = np.asarray(ids, dtype=np.int64)
    e = (_h(0, ids, 0, 3) % np.uint64(17)).astype(np.int64) - 26
    h = _h(it, ids[:, None], np.arange(3)[None, :], VS_SALT)
    k = (h % np.uint64(16)).astype(np.float64)
    sign = np.where((h >> np.uint64(20)) % np.uint64(2) == 0, 1.0, -1.0)
    g = sign * (1.0 + k / 16.0) * np.exp2(e.astype(np.float64))[:, None]
    g[ids % 16 == 5] = (TIE_GRAD, 0.0, 0.0)
    return torch.from_numpy(g.astype(np.float32))


def radii(it, ids):
    """float32 [K]: screen radii of the iteration's render, 0 (not visible) for the untouched rows, else 1..40."""
    ids = np.asarray(ids, dtype=np.int64)
    r = 1 + (_h(it, ids, 0, 9) % np.uint64(40)).astype(np.float64)
    return torch.from_numpy((r * touched(it, ids)).astype(np.float32))


def initial_params(cfg):
    """{group: float32 tensor}: positions in a 10-unit box, log-scales with exp() over 0.005..1 (both sides of
    percent_dense * extent and of 0.1 * extent), raw quaternions of any norm, opacity logits uniform over cfg['opacity']."""
    P, shp = cfg["P"], shapes(cfg["sh"])
    g = np.random.default_rng(cfg["seed"])
    lo, hi = cfg["opacity"]
    d = {"xyz": g.uniform(-5, 5, (P, 3)), "f_dc": g.normal(size=(P, 1, 3)), "f_rest": 0.1 * g.normal(size=(P,) + shp["f_rest"]),
         "opacity": g.uniform(lo, hi, (P, 1)), "scaling": np.log(0.005) + g.uniform(0, 1, (P, 3)) * np.log(200.0),
         "rotation": g.normal(size=(P, 4)) * np.exp(g.uniform(-1, 1, (P, 1)))}
    return {n: torch.from_numpy(np.ascontiguousarray(d[n], dtype=np.float32)) for n in GROUPS}


# ---- the reference's mask expressions (gaussian_model.py:581-586, 630-637, 705-713; train_pan.py:675) ----
def mean_grads(accum, denom):
    g = accum / denom
    g[g.isnan()] = 0.0
    return g


def clone_mask(grads, scaling_raw, grad_threshold, percent_dense, extent):
    return (torch.norm(grads, dim=-1) >= grad_threshold) & (torch.exp(scaling_raw).max(dim=1).values <= percent_dense * extent)


def split_mask(grads, n_rows, scaling_raw, grad_threshold, percent_dense, extent):
    """`grads` are the statistics of the rows before the clone; the clones appended since count as zero."""
    padded = torch.zeros(n_rows, dtype=grads.dtype, device=grads.device)
    padded[:grads.shape[0]] = grads.squeeze(-1)
    return (padded >= grad_threshold) & (torch.exp(scaling_raw).max(dim=1).values > percent_dense * extent)


def final_prune_mask(opacity_raw, scaling_raw, max_radii2D, max_screen_size, extent):
    m = (torch.sigmoid(opacity_raw) < DENSIFY_MIN_OPACITY).squeeze(-1)
    if max_screen_size:
        m = m | (max_radii2D > max_screen_size) | (torch.exp(scaling_raw).max(dim=1).values > 0.1 * extent)
    return m


def transparent_mask(opacity_raw):
    return opacity_raw.squeeze(-1) < MIN_OPACITY


def near(x, threshold, margin=MARGIN):
    """Rows whose quantity lies within `margin` relative of the threshold without being exactly on it (numpy / torch)."""
    return (abs(x - threshold) <= margin * abs(threshold)) & (x != threshold)


# ---- fixtures ----
def fixture_path(name, root=None):
    return os.path.join(root or GOLDEN_DIR, name + ".npz")


class Fixture:
    """One lifecycle fixture. `stages` is the recorded list of operations, each {"op", "src", "dst", ...} with `src` / `dst`
    naming snapshots. A snapshot `s` holds, per group n, `s/n/p`, `s/n/m`, `s/n/v` (float32; m and v only once the state
    exists), `s/step` ([6], -1 without state), `s/ids` and the three statistics; float64 twins end in `@64`."""

    def __init__(self, name, root=None):
        self.name = name
        self.path = fixture_path(name, root)
        self.z = dict(np.load(self.path))
        self.cfg = CASES[name]
        self.stages = json.loads(str(self.z["stages"]))

    def has(self, key):
        return key in self.z

    def t(self, key, device="cpu"):
        return torch.from_numpy(np.array(self.z[key], copy=True)).to(device)

    def ids(self, snap):
        return self.z[f"{snap}/ids"]


def make_optimizer(fx, snap, cls, device="cpu", **kw):
    """An optimizer of class `cls` over the six groups, holding the fp32 state of snapshot `snap`."""
    L = lrs()
    groups = [{"params": [torch.nn.Parameter(fx.t(f"{snap}/{n}/p", device))], "lr": L[n], "name": n} for n in GROUPS]
    opt = cls(groups, lr=0.0, eps=EPS, **kw)
    steps = fx.z[f"{snap}/step"]
    for g, n, s in zip(opt.param_groups, GROUPS, steps):
        if s >= 0:
            opt.state[g["params"][0]] = {"step": torch.tensor(float(s)), "exp_avg": fx.t(f"{snap}/{n}/m", device),
                                         "exp_avg_sq": fx.t(f"{snap}/{n}/v", device)}
    return opt


def stats_of(fx, snap, device="cpu"):
    return {k: fx.t(f"{snap}/{k}", device) for k in STATS}


def run_steps(opt, stage, ids, sh, stats=None, device="cpu"):
    """The Adam stretch of `stage` on `opt` with the hashed gradients; `stats` (a dict of the three statistics) is updated as
    train_pan.py:683-690 does when the stage records them."""
    for k in range(stage["n"]):
        it = stage["it0"] + k + 1
        for g in opt.param_groups:
            g["params"][0].grad = hashed_grad(it, ids, g["name"], sh).to(device)
        opt.step()
        opt.zero_grad(set_to_none=True)
        if stage["stats"] and stats is not None:
            r, vs = radii(it, ids).to(device), viewspace_grad(it, ids).to(device)
            vis = r > 0
            stats["max_radii2D"][vis] = torch.max(stats["max_radii2D"][vis], r[vis])
            stats["xyz_gradient_accum"][vis] += torch.norm(vs[vis, :2], dim=-1, keepdim=True)
            stats["denom"][vis] += 1


# ---- one Adam step: the derived bound ----
U = 2.0 ** -24      # unit roundoff of fp32
TINY = 2.0 ** -149  # smallest fp32 subnormal


def adam_step_f64(p, g, m, v, lr, betas, eps, step):
    """torch.optim.Adam's update in float64 from float64 copies of the given state: (p', m', v', d, upd)."""
    b1, b2 = betas
    p, g, m, v = (x.double() for x in (p, g, m, v))
    m2 = m + (1.0 - b1) * (g - m)
    v2 = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    d = v2.sqrt() / bc2 ** 0.5 + eps
    upd = (lr / bc1) * (m2 / d)
    return p - upd, m2, v2, d, upd


def adam_step_bound(p, g, m, v, lr, betas, eps, step):
    """Elementwise bounds (float64 tensors) on |fp32 result - float64 result| of ONE Adam step from an fp32 state, for an
    implementation that evaluates torch's formula in fp32 with one rounding per operation:

        m' = m + w1 (g - m);  v' = b2 v + w2 g g;  d = sqrt(v') / sqrt(bc2) + eps;  p' = p - (lr / bc1) m' / d

    u = 2^-24 (round to nearest), t = 2^-149 (what a result in the subnormal range can lose instead).

    * dm <= 3u (|m| + |g|) + 2t. Three roundings touch m': the difference g - m (<= u (|g| + |m|)), its product with w1,
      itself rounded from the double 1 - b1 (2u w1 |g - m|), and the final sum (u |m'|, |m'| <= |m| + |g|). w1 < 1, so
      the sum of the three stays under 3u (|m| + |g|); 2t for the product and the sum when they are subnormal.
    * dv <= 4u v' + 4t. Both terms of v' are non-negative, so relative errors carry over: b2 rounded and the product b2 v
      (2u), g g and its product with the rounded w2 (3u), the final sum (1u), each weighted by its term's share of v':
      at most 4u v' in all. A subnormal g g, w2 g g or b2 v loses up to t each, the sum one more: 4t.
    * dd = (sqrt(v' + dv) - sqrt(v')) / sqrt(bc2) + 3u d: the error of v' carried through the square root (written as a
      difference, so that v' = 0 with dv = 4t gives sqrt(4t), not 0/0), then the rounding of the square root, of the
      quotient by sqrt(bc2) and of the sum with eps: 3u d. (eps and sqrt(bc2) rounded to fp32 are part of that term for
      torch, which keeps them in double inside the op; an implementation that rounds them first pays u d more: see below.)
    * dp <= lr / bc1 (dm / d + |m'| / d dd / d) + 4u |upd| + u (|p| + |upd|): the errors of numerator and denominator to first
      order, the quotient m' / d, the step size lr / bc1 rounded to fp32 and its product with the quotient (together 4u |upd|
      with the second-order terms), and the final subtraction (u |p'|, |p'| <= |p| + |upd|).

    torch.optim.Adam itself (fp32, CPU) stays inside factor 1 of these bounds (tests/test_optim_golden.py). The HIP kernel
    forms its constants in fp32 before the launch (lr, 1 / bc1, sqrt(bc2), eps: up to 3u more on the update and u on d), so
    tests/test_gpu_optim.py grants it FACTOR_KERNEL = 2 on all three.

    Returns (bm, bv, bp)."""
    p2, m2, v2, d, upd = adam_step_f64(p, g, m, v, lr, betas, eps, step)
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    m, g, p = m.double().abs(), g.double().abs(), p.double().abs()
    bm = 3 * U * (m + g) + 2 * TINY
    bv = 4 * U * v2 + 4 * TINY
    dd = ((v2 + bv).sqrt() - v2.sqrt()) / bc2 ** 0.5 + 3 * U * d
    bp = (lr / bc1) * (bm / d + m2.abs() / d * dd / d) + 4 * U * upd.abs() + U * (p + upd.abs())
    return bm, bv, bp


FACTOR_TORCH, FACTOR_KERNEL = 1.0, 2.0
ADAM_GRID_STEPS = (1, 2, 10, 100, 1000, 5000, 30000)
ADAM_GRID_GSCALE = (1e-20, 1e-12, 1e-6, 1e-2, 1.0, 1e3, 1e15)
ADAM_GRID_EPS = (1e-15, 1e-8)


def adam_grid_state(gscale, n=3072, seed=0):
    """(p, g, m, v) float32 [n] for one grid point: gradients of scale `gscale` with a third exactly zero, first moments
    from zero to 1e3 x the gradient scale (both signs), second moments from zero to (1e3 gscale)^2, parameters of order 1."""
    r = np.random.default_rng(seed)
    g = r.normal(size=n) * gscale
    g[::3] = 0.0
    mfac = np.concatenate([[0.0], 10.0 ** r.uniform(-3, 3, n - 1)])
    m = r.choice([-1.0, 1.0], n) * mfac * gscale
    vfac = 10.0 ** r.uniform(-3, 3, n)
    vfac[1::5] = 0.0
    with np.errstate(over="ignore"):
        v = np.minimum((vfac * gscale) ** 2, 1e38)
    p = r.normal(size=n)
    return tuple(torch.from_numpy(x.astype(np.float32)) for x in (p, g, m, v))


def adam_check_one_step(cls, device, step, gscale, eps, factor, lr=1e-2, betas=BETAS):
    """One `cls.step()` from a grid state against float64; returns the worst error / bound ratios (m, v, p) after asserting
    every element within `factor` x its bound."""
    p, g, m, v = adam_grid_state(gscale, seed=step)
    par = torch.nn.Parameter(p.clone().to(device))
    opt = cls([{"params": [par], "lr": lr, "name": "x"}], lr=0.0, betas=betas, eps=eps)
    opt.state[par] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone().to(device), "exp_avg_sq": v.clone().to(device)}
    par.grad = g.clone().to(device)
    opt.step()
    st = opt.state[par]
    assert int(st["step"]) == step
    p2, m2, v2, _, _ = adam_step_f64(p, g, m, v, lr, betas, eps, step)
    bm, bv, bp = adam_step_bound(p, g, m, v, lr, betas, eps, step)
    worst = []
    for what, got, want, b in (("exp_avg", st["exp_avg"], m2, bm), ("exp_avg_sq", st["exp_avg_sq"], v2, bv), ("param", par.detach(), p2, bp)):
        got = got.detach().cpu().double()
        assert bool(torch.isfinite(got).all()), (what, step, gscale, eps)
        ratio = (got - want).abs() / b
        worst.append(float(ratio.max()))
        i = int(ratio.argmax())
        assert worst[-1] <= factor, (f"{what}[{i}] step={step} |g|~{gscale:g} eps={eps:g}: got {float(got[i])!r}, float64 {float(want[i])!r}, "
                                     f"error {float((got - want).abs()[i]):.3e} = {worst[-1]:.3f} x bound {float(b[i]):.3e}")
    return worst


# ---- replaying a fixture through eogs2_amd.optim ----
def _params(opt):
    return {g["name"]: g["params"][0] for g in opt.param_groups}


def _ulp32(x64):
    return np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)


def _computed_close(fx, key, got, rows=slice(None)):
    """`got` (fp32 numpy) against the fixture's float64 array, elementwise, within the larger of 4 x the reference's own
    fp32-to-float64 distance for that array and 4 ulp of the element; returns the worst error / bound."""
    f32, f64 = fx.z[key].astype(np.float64), fx.z[key + "@64"]
    dist = float(np.abs(f32 - f64).max()) if f64.size else 0.0
    bound = np.maximum(4 * dist, 4 * _ulp32(f64))[rows]
    err = np.abs(got.astype(np.float64)[rows] - f64[rows])
    assert (err <= bound).all(), (fx.name, key, float((err / bound).max()))
    return float((err / bound).max()) if err.size else 0.0


def steps_bound(fx, key):
    """Per tensor: the larger of 2e-6 of the tensor's scale and 4 x the distance between the reference's own fp32 and
    float64 arrays at that snapshot; both from the fixture."""
    f32, f64 = fx.z[key].astype(np.float64), fx.z[key + "@64"]
    if not f64.size:
        return 0.0, 0.0, 0.0
    scale, dist = float(np.abs(f64).max()), float(np.abs(f32 - f64).max())
    return max(2e-6 * scale, 4 * dist), scale, dist


def check_steps(fx, st, opt, stats, exact, log=None):
    dst = st["dst"]
    steps = fx.z[f"{dst}/step"]
    for (n, p), want_step in zip(_params(opt).items(), steps):
        state = opt.state[p]
        assert len(opt.state) == len(GROUPS) and int(state["step"]) == int(want_step), (fx.name, dst, n)
        for k, got in (("p", p.detach()), ("m", state["exp_avg"]), ("v", state["exp_avg_sq"])):
            key = f"{dst}/{n}/{k}"
            got = got.cpu().numpy()
            assert got.dtype == np.float32 and got.shape == fx.z[key].shape, key
            if exact:
                assert got.tobytes() == fx.z[key].tobytes(), (fx.name, key)
            else:
                bound, scale, dist = steps_bound(fx, key)
                err = float(np.abs(got.astype(np.float64) - fx.z[key + "@64"]).max()) if got.size else 0.0
                if log is not None:
                    log.append(f"{fx.name} {key}: error {err:.3e} bound {bound:.3e} (scale {scale:.3e}, fp32-to-float64 {dist:.3e})")
                assert err <= bound, (fx.name, key, err, bound)
    for k in STATS:
        got, key = stats[k].cpu().numpy(), f"{dst}/{k}"
        if exact or k != "xyz_gradient_accum":  # counts and radii are small integers: exact on any device
            assert got.tobytes() == fx.z[key].tobytes(), (fx.name, key)
        else:
            bound, _, _ = steps_bound(fx, key)
            assert float(np.abs(got.astype(np.float64) - fx.z[key + "@64"]).max()) <= bound, (fx.name, key)


class normal_returns:
    """Hands the recorded samples to the next `torch.normal` call (device generators differ from the CPU's)."""

    def __init__(self, samples):
        self.samples, self.calls = samples, 0

    def __enter__(self):
        self.orig = torch.normal

        def normal(mean=None, std=None, **k):
            self.calls += 1
            assert tuple(std.shape) == tuple(self.samples.shape) and float(mean.abs().sum()) == 0.0
            return self.samples.to(device=std.device, dtype=std.dtype)

        torch.normal = normal
        return self

    def __exit__(self, *exc):
        torch.normal = self.orig


def apply_stage(fx, st, device, cls, optim):
    """The structural stage `st` through the library's functions on the fixture's pre-stage state: (opt, stats, ids, radii)."""
    src, op = st["src"], st["op"]
    opt, stats, ids = make_optimizer(fx, src, cls, device), stats_of(fx, src, device), fx.t(f"{src}/ids", device)
    before = _params(opt)
    radii_out = None
    if op in ("tprune", "prune"):
        mask = fx.t(st["mask"], device)
        new, extra = optim.prune_optimizer(opt, ~mask, extra=[stats[k] for k in STATS] + [ids])
        stats, ids = dict(zip(STATS, extra[:3])), extra[3]
    elif op == "clone":
        mask = fx.t(st["mask"], device)
        new, radii_out = optim.densify_and_clone(opt, mask, tmp_radii=fx.t(st["radii"], device))
        _, ids = optim.densify_and_clone(make_optimizer(fx, src, cls, device), mask, tmp_radii=ids)  # the id column rides as tmp_radii
    elif op == "split":
        mask, samples = fx.t(st["mask"], device), fx.t(st["normal"], device)
        with normal_returns(samples) as nr:
            new, radii_out, keep = optim.densify_and_split(opt, mask, N=st["N"], tmp_radii=fx.t(st["radii"], device))
        assert nr.calls == 1 and torch.equal(keep[:mask.numel()], ~mask) and bool(keep[mask.numel():].all())
        with normal_returns(samples):
            _, ids, keep2 = optim.densify_and_split(make_optimizer(fx, src, cls, device), mask, N=st["N"], tmp_radii=ids)
        ids = ids[keep2]
    elif op == "reset":
        new = optim.reset_opacity(opt)
        after = _params(opt)
        assert set(new) == {"opacity"} and all((after[n] is before[n]) == (n != "opacity") for n in GROUPS)
    else:
        raise ValueError(op)
    if op in ("clone", "split"):  # densification_postfix: the caller restarts the three statistics at the new size
        n = _params(opt)["xyz"].shape[0]
        stats = {"xyz_gradient_accum": torch.zeros(n, 1, device=device), "denom": torch.zeros(n, 1, device=device),
                 "max_radii2D": torch.zeros(n, device=device)}
    after = _params(opt)
    assert all(new[n] is after[n] and after[n].requires_grad and isinstance(after[n], torch.nn.Parameter) for n in new)
    assert len(opt.state) == len(GROUPS) and all(after[n] in opt.state for n in GROUPS)  # one state entry per live parameter
    return opt, stats, ids, radii_out


def check_structural(fx, st, opt, stats, ids, radii_out, exact, log=None):
    """Everything the stage only moves equals the fixture bit for bit; what it computes (a split's new positions and
    log-scales, the reset's logits) is bit-equal too where `exact` (the CPU, the reference's own operations), else within
    `_computed_close` of the fixture's float64 arrays."""
    src, dst, op = st["src"], st["dst"], st["op"]
    n_old = 0
    if op == "split":
        n_old = int((~fx.z[st["mask"]]).sum())
    for (n, p), want_step in zip(_params(opt).items(), fx.z[f"{dst}/step"]):
        state = opt.state[p]
        assert int(state["step"]) == int(want_step) == int(fx.z[f"{src}/step"][GROUPS.index(n)]), (fx.name, dst, n, "step")
        for k, got in (("p", p.detach()), ("m", state["exp_avg"]), ("v", state["exp_avg_sq"])):
            key = f"{dst}/{n}/{k}"
            got, want = got.cpu().numpy(), fx.z[key]
            assert got.dtype == np.float32 and got.shape == want.shape, (fx.name, key, got.shape, want.shape)
            computed = k == "p" and ((op == "split" and n in ("xyz", "scaling")) or (op == "reset" and n == "opacity"))
            if computed and not exact:
                rows = slice(n_old, None) if op == "split" else slice(None)
                assert got[:n_old].tobytes() == want[:n_old].tobytes(), (fx.name, key, "kept rows")
                r = _computed_close(fx, key, got, rows)
                if log is not None:
                    log.append(f"{fx.name} {key}: computed rows at {r:.3f} of their bound")
            else:
                assert got.tobytes() == want.tobytes(), (fx.name, key)
    assert ids.dtype == torch.int32 and np.array_equal(ids.cpu().numpy(), fx.z[f"{dst}/ids"]), (fx.name, dst, "ids")
    for k in STATS:
        assert stats[k].cpu().numpy().tobytes() == fx.z[f"{dst}/{k}"].tobytes(), (fx.name, dst, k)
    if radii_out is not None:
        assert radii_out.cpu().numpy().tobytes() == fx.z[st["tmp_radii"]].tobytes(), (fx.name, dst, "tmp_radii")


def recomputed_mask(fx, st, opt, stats, carry):
    """The stage's mask from the given (replayed) state with the reference's expressions; `carry` keeps the mean gradients of
    the clone for the split that follows it."""
    cfg, par = fx.cfg, {n: p.detach() for n, p in _params(opt).items()}
    pd = TRAIN_ARGS["percent_dense"]
    if st["op"] == "tprune":
        return transparent_mask(par["opacity"])
    if st["op"] == "clone":
        carry["grads"] = mean_grads(stats["xyz_gradient_accum"], stats["denom"])
        return clone_mask(carry["grads"], par["scaling"], cfg["grad_threshold"], pd, cfg["extent"])
    if st["op"] == "split":
        return split_mask(carry["grads"], par["xyz"].shape[0], par["scaling"], cfg["grad_threshold"], pd, cfg["extent"])
    if st["op"] == "prune":
        return final_prune_mask(par["opacity"], par["scaling"], stats["max_radii2D"], st["max_screen_size"], cfg["extent"])
    if st["op"] == "reset":  # which logits the reset caps
        return (torch.sigmoid(par["opacity"]) > RESET_CAP).squeeze(-1)
    raise ValueError(st["op"])


def stored_mask(fx, st):
    if st["op"] == "reset":  # the capped rows all hold the one value logit(0.01); the others keep a smaller one
        post = fx.z[f"{st['dst']}/opacity/p"][:, 0]
        return post == post.max() if (post == post.max()).sum() > 1 else np.zeros_like(post, dtype=bool)
    return fx.z[st["mask"]]


def replay(fx, device, cls, optim, exact, log=None):
    """Every stage of the fixture through `cls` and the library's functions (see the module docstring of
    tests/test_optim_golden.py / test_gpu_optim.py for what is compared how). Each stage starts from the fixture's fp32
    state; each structural stage's mask is also recomputed from the replayed state before it and must equal the stored
    one on every row."""
    prev, carry, sh = None, {}, fx.cfg["sh"]
    for st in fx.stages:
        if st["op"] == "steps":
            opt, stats = make_optimizer(fx, st["src"], cls, device), stats_of(fx, st["src"], device)
            run_steps(opt, st, fx.ids(st["src"]), sh, stats, device)
            check_steps(fx, st, opt, stats, exact, log)
        else:
            assert prev is not None
            got = recomputed_mask(fx, st, prev[0], prev[1], carry).cpu().numpy()
            assert np.array_equal(got, stored_mask(fx, st)), (fx.name, st, "rows that differ", np.nonzero(got != stored_mask(fx, st))[0])
            opt, stats, ids, radii_out = apply_stage(fx, st, device, cls, optim)
            check_structural(fx, st, opt, stats, ids, radii_out, exact, log)
        prev = (opt, stats)
