"""The semantics of the training monitor (include/eogs_monitor.h) restated in plain Python and numpy, and the names of its
fixtures. Shared by tests/test_monitor.py (CPU) and tests/test_gpu_monitor.py.

`Monitor` is fed the four fp32 values of an observation — what the reference reads back with `.item()`, what the device
leaves in `last` — and keeps Python floats, as train_pan.py:423-429, 471-495, 512-597 does; its stopper is
utils/callback_utils.py:15-44. Python floats are IEEE doubles, so a device double accumulator fed the same fp32 values in the
same order must hold the same bits.
"""
import glob
import math
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "monitor")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))
METRICS = ("photometric", "L1", "pan_psnr", "pan_ssim", "msi_psnr", "msi_ssim")
RECORD_KEYS = ("interval", "iteration") + METRICS + ("ema_loss", "ema_photometric", "mean_opacity", "rows", "best", "counter",
                                                     "early_stop")
RING = 16


def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


def photometric_f32(l1, ssim, lam):
    """image_utils.py:28 as torch evaluates it on fp32 scalars: each Python scalar rounded to fp32 once."""
    f = np.float32
    return f(f(f(1.0 - lam) * f(l1)) + f(f(lam) * f(f(1.0) - f(ssim))))


def psnr_f64(img, gt):
    """image_utils.py:19-21 in float64, mean over planes; inf for an all-equal plane."""
    d = img.astype(np.float64) - gt.astype(np.float64)
    mse = (d * d).reshape(d.shape[0], -1).mean(1)
    with np.errstate(divide="ignore"):
        return float(np.mean(20.0 * np.log10(1.0 / np.sqrt(mse))))


class Monitor:
    def __init__(self, metric_name="photometric", operator="min", patience=5):
        if metric_name not in METRICS:
            raise ValueError(metric_name)
        if operator not in ("min", "max"):
            raise ValueError("operator should be either min or max")
        self.metric_name, self.operator, self.patience = metric_name, operator, patience
        self.best = math.inf if operator == "min" else -math.inf
        self.counter, self.early_stop = 0, False
        self.ema_loss = self.ema_photometric = 0.0
        self.iteration = self.intervals = 0
        self.mean_opacity, self.rows = 0.0, 0
        self.last_photometric = 0.0
        self.records = []
        self._clear()

    def _clear(self):
        self.sums = dict.fromkeys(METRICS, 0.0)
        self.n = {"photo": 0, "pan": 0, "msi": 0}

    def observe(self, l1, ssim, photometric, psnr, kind, photometric_on=True):
        if kind not in ("pan", "msi"):
            raise ValueError(f"Unknown camera type {kind}, should be either 'pan' or 'msi'")
        self.sums["L1"] += float(np.float32(l1))
        if photometric_on:
            self.sums["photometric"] += float(np.float32(photometric))
            self.n["photo"] += 1
        self.sums[kind + "_psnr"] += float(np.float32(psnr))
        self.sums[kind + "_ssim"] += float(np.float32(ssim))
        self.n[kind] += 1
        self.last_photometric = float(np.float32(photometric)) if photometric_on else 0.0

    def observe_model(self, mean_opacity, rows):
        self.mean_opacity, self.rows = float(np.float32(mean_opacity)), int(rows)

    def end_iteration(self, loss):
        self.ema_loss = 0.4 * float(np.float32(loss)) + 0.6 * self.ema_loss
        self.ema_photometric = 0.4 * self.last_photometric + 0.6 * self.ema_photometric
        self.iteration += 1

    def close_interval(self):
        den = {"photometric": "photo", "L1": "photo", "pan_psnr": "pan", "pan_ssim": "pan", "msi_psnr": "msi", "msi_ssim": "msi"}
        means = {k: self.sums[k] / max(1, self.n[den[k]]) for k in METRICS}
        if self.patience is not None:
            m = means[self.metric_name]
            if not m == 0:
                if (m < self.best) if self.operator == "min" else (m > self.best):
                    self.best, self.counter = m, 0
                else:
                    self.counter += 1
                    if self.counter >= self.patience:
                        self.early_stop = True
        self.intervals += 1
        rec = {"interval": self.intervals, "iteration": self.iteration, **means, "ema_loss": self.ema_loss,
               "ema_photometric": self.ema_photometric, "mean_opacity": self.mean_opacity, "rows": self.rows, "best": self.best,
               "counter": self.counter, "early_stop": self.early_stop}
        self.records.append(rec)
        self._clear()
        return rec


def bits(v):
    """A record value as comparable bits: doubles by their 64-bit pattern (NaN and inf included), the rest as integers."""
    if isinstance(v, (bool, np.bool_)):
        return int(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if math.isnan(v):
        return "nan"  # (a NaN's payload and sign are the adder's own; every NaN is the same value here)
    return int(np.float64(v).view(np.uint64))


def same_record(a, b):
    return all(bits(a[k]) == bits(b[k]) for k in RECORD_KEYS)


def record_diff(a, b):
    return {k: (a[k], b[k]) for k in RECORD_KEYS if bits(a[k]) != bits(b[k])}


def fixture_records(c):
    """The fixture's records as a list of dicts with RECORD_KEYS (mean_opacity and rows are not the reference's: 0)."""
    out = []
    for j in range(len(c["rec_iteration"])):
        r = {"interval": j + 1, "iteration": int(c["rec_iteration"][j]), "ema_loss": float(c["rec_ema_loss"][j]),
             "ema_photometric": float(c["rec_ema_photometric"][j]), "mean_opacity": 0.0, "rows": 0, "best": float(c["rec_best"][j]),
             "counter": int(c["rec_counter"][j]), "early_stop": bool(c["rec_early_stop"][j])}
        for k in METRICS:
            r[k] = float(c["rec_" + k][j])
        out.append(r)
    return out


def obs_image(c, i):
    """(image, gt) of observation i: gt is fixed per kind, the images are stacked per kind in the order they are observed."""
    kind = str(c["kinds"][i])
    j = sum(1 for k in c["kinds"][:i] if str(k) == kind)
    return c["img_" + kind][j], c["gt_" + kind]


def drive(c, observe, end_iteration, close_interval):
    """The loop of train_pan.py over fixture `c`: observe(i, kind, photometric_on) per camera, end_iteration(it) per
    iteration, close_interval() every `interval` iterations; the last interval may stay open."""
    interval, i = int(c["interval"]), 0
    for it in range(int(c["iterations"])):
        for _ in range(int(c["cams_per_iter"][it])):
            observe(i, str(c["kinds"][i]), bool(c["photometric_on"]))
            i += 1
        end_iteration(it)
        if (it + 1) % interval == 0:
            close_interval()


def replay(c, values=None):
    """A Monitor driven through `c` from per-observation fp32 values (default: the fixture's own, the reference's)."""
    v = values if values is not None else {k: c[k] for k in ("l1", "ssim", "photometric", "psnr")}
    patience = int(c["patience"])
    m = Monitor(str(c["metric_name"]), str(c["operator"]), None if patience < 0 else patience)
    drive(c, lambda i, kind, on: m.observe(v["l1"][i], v["ssim"][i], v["photometric"][i], v["psnr"][i], kind, on),
          lambda it: m.end_iteration(c["loss"][it]), m.close_interval)
    return m
