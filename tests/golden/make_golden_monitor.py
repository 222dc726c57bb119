"""Generates tests/golden/monitor/*.npz by running the REFERENCE's own functions, imported from a checkout:

    utils.image_utils.psnr, lphotom         utils/image_utils.py:19-21, 27-28
    utils.loss_utils.l1_loss, ssim          utils/loss_utils.py:18-19, 45-85
    utils.callback_utils.early_stopping     utils/callback_utils.py:1-44

through a loop written here that accumulates as train_pan.py:423-429, 471-495, 512-597 does: fp32 `.item()` values added
into Python floats per camera, two moving averages per iteration, means + early stopper + reset every `interval`
iterations. Only images, per-observation values, per-interval records and the stopper's state are stored. CPU only.

    python tests/golden/make_golden_monitor.py <reference checkout>/src/gaussiansplatting

Keys: `interval`, `iterations`, `lambda_dssim`, `photometric_on`, `metric_name`, `operator`, `patience`; `cams_per_iter`
[iterations]; per observation `kinds`, `l1`, `ssim`, `photometric`, `psnr` (fp32); `gt_pan` [1,h,w], `gt_msi` [3,h,w] and the
observed images stacked per kind in order, `img_pan`, `img_msi`; `loss` [iterations] (fp32: the iteration's total);
per closed interval `rec_iteration`, `rec_<metric>` for the six means, `rec_ema_loss`, `rec_ema_photometric`, `rec_best`,
`rec_counter`, `rec_early_stop`; `final_ema_loss`, `final_ema_photometric` after the last iteration; `stop_interval`: the
1-based interval at which the flag first fires, 0 = never.

Two guarantees, asserted: wherever the stopper compares a metric with its best, the two differ by more than 1e-3 relative
(a tolerance of 1e-5 on the values cannot change a decision), and every finite PSNR is positive (noise amplitude below 1:
sums of values within a relative tolerance stay within it).
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "monitor")
METRICS = ("photometric", "L1", "pan_psnr", "pan_ssim", "msi_psnr", "msi_ssim")
SHAPES = {"pan": (1, 13, 17), "msi": (3, 9, 14)}


def run(ref, name, *, interval, kinds_per_iter, amps, metric_name, operator, patience, photometric_on=True, lam=0.2, seed=0, special=None):
    """kinds_per_iter: one tuple of kinds per iteration; amps: the noise amplitude per iteration; special: {observation
    index: "equal" | "nan"}."""
    psnr, lphotom, l1_loss, ssim, early_stopping = ref
    g = torch.Generator().manual_seed(seed)
    gts = {k: torch.rand(s, generator=g) for k, s in SHAPES.items()}
    stopper = early_stopping(patience=patience, operator=operator, metric_name=metric_name)
    special = special or {}
    obs = {k: [] for k in ("kinds", "l1", "ssim", "photometric", "psnr")}
    imgs = {"pan": [], "msi": []}
    losses, recs = [], {k: [] for k in ("iteration", "ema_loss", "ema_photometric", "best", "counter", "early_stop") + METRICS}
    metric_dict = {"photometric": 0.0, "L1": 0.0, "n_photo": 0}
    pan_psnr = pan_ssim = msi_psnr = msi_ssim = 0
    n_pan = n_msi = 0
    ema_loss = ema_photo = 0.0
    stop_interval = 0
    for it, (kinds, amp) in enumerate(zip(kinds_per_iter, amps), start=1):
        loss = 0
        for kind in kinds:
            gt = gts[kind]
            image = (gt + amp * torch.randn(gt.shape, generator=g)).contiguous()
            what = special.get(len(obs["kinds"]))
            if what == "equal":
                image = gt.clone()
            elif what == "nan":
                image[0, 2, 3] = float("nan")
            Ll1 = l1_loss(image, gt)
            metric_dict["L1"] += Ll1.item()
            if photometric_on:
                Lphotometric = lphotom(image, gt, Ll1, lam)
                metric_dict["photometric"] += Lphotometric.item()
                metric_dict["n_photo"] += 1
                inter_loss = Lphotometric
            else:
                Lphotometric = torch.zeros(())
                inter_loss = Ll1
            loss = loss + inter_loss.mean().detach()
            p = psnr(image, gt).mean().float().item()
            s = ssim(image, gt).item()
            assert math.isnan(p) or math.isinf(p) or p > 0, (name, p)
            if kind == "pan":
                pan_psnr += p
                pan_ssim += s
                n_pan += 1
            elif kind == "msi":
                msi_psnr += p
                msi_ssim += s
                n_msi += 1
            else:
                raise ValueError(kind)
            obs["kinds"].append(kind)
            obs["l1"].append(Ll1.item())
            obs["ssim"].append(s)
            obs["photometric"].append(Lphotometric.item())
            obs["psnr"].append(p)
            imgs[kind].append(image.numpy())
        ema_loss = 0.4 * loss.item() + 0.6 * ema_loss
        ema_photo = 0.4 * Lphotometric.item() + 0.6 * ema_photo
        losses.append(loss.item())
        if it % interval == 0:
            metric_dict["photometric"] = metric_dict["photometric"] / max(1, metric_dict["n_photo"])
            metric_dict["L1"] = metric_dict["L1"] / max(1, metric_dict["n_photo"])
            metric_dict["pan_psnr"] = pan_psnr / max(1, n_pan)
            metric_dict["pan_ssim"] = pan_ssim / max(1, n_pan)
            metric_dict["msi_psnr"] = msi_psnr / max(1, n_msi)
            metric_dict["msi_ssim"] = msi_ssim / max(1, n_msi)
            m, best = metric_dict[metric_name], stopper.best_loss
            if m != 0 and math.isfinite(m) and math.isfinite(best):
                assert abs(m - best) > 1e-3 * max(abs(m), abs(best)), (name, it, m, best)
            if stopper(metric_dict=metric_dict) and not stop_interval:
                stop_interval = it // interval
            for k in METRICS:
                recs[k].append(float(metric_dict[k]))
            recs["iteration"].append(it)
            recs["ema_loss"].append(ema_loss)
            recs["ema_photometric"].append(ema_photo)
            recs["best"].append(float(stopper.best_loss))
            recs["counter"].append(stopper.counter)
            recs["early_stop"].append(bool(stopper.early_stop))
            pan_psnr = pan_ssim = msi_psnr = msi_ssim = 0
            n_pan = n_msi = 0
            metric_dict = {"photometric": 0.0, "L1": 0.0, "n_photo": 0}
    out = dict(interval=interval, iterations=len(kinds_per_iter), lambda_dssim=lam, photometric_on=photometric_on,
               metric_name=metric_name, operator=operator, patience=patience,
               cams_per_iter=np.array([len(k) for k in kinds_per_iter], dtype=np.int32), kinds=np.array(obs["kinds"]),
               gt_pan=gts["pan"].numpy(), gt_msi=gts["msi"].numpy(), loss=np.array(losses, dtype=np.float32),
               final_ema_loss=ema_loss, final_ema_photometric=ema_photo, stop_interval=stop_interval)
    for k in ("l1", "ssim", "photometric", "psnr"):
        out[k] = np.array(obs[k], dtype=np.float32)
        assert all(float(a) == b or (math.isnan(b) and math.isnan(a)) for a, b in zip(out[k], obs[k])), k  # fp32 values, stored exactly
    for k, s in SHAPES.items():
        out["img_" + k] = np.stack(imgs[k]).astype(np.float32) if imgs[k] else np.zeros((0,) + s, dtype=np.float32)
    for k, v in recs.items():
        out["rec_" + k] = np.array(v, dtype=np.int64 if k in ("iteration", "counter") else (np.bool_ if k == "early_stop" else np.float64))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, "observations", len(obs["kinds"]), "intervals", len(recs["iteration"]), "stop at interval", stop_interval,
          "counters", recs["counter"])
    return out


def main(refroot):
    sys.path.insert(0, refroot)
    from utils.callback_utils import early_stopping
    from utils.image_utils import lphotom, psnr
    from utils.loss_utils import l1_loss, ssim

    ref = (psnr, lphotom, l1_loss, ssim, early_stopping)
    both = ("pan", "msi")
    # (a) pan and msi cameras in turn, 37 iterations of interval 10: the last interval stays open
    run(ref, "alternating", interval=10, kinds_per_iter=[both] * 37, amps=[0.3 * 0.97**i for i in range(37)],
        metric_name="photometric", operator="min", patience=5, seed=1)
    # (b) max on pan_psnr, the patience of 2 is reached at interval 5 of 8 and the loop goes on
    amps = [0.25 * 0.9**i for i in range(15)] + [0.25 * 0.9**14 * 1.08**i for i in range(1, 26)]
    c = run(ref, "max_patience", interval=5, kinds_per_iter=[("pan",) if i % 3 else both for i in range(40)], amps=amps,
            metric_name="pan_psnr", operator="max", patience=2, seed=2)
    assert c["stop_interval"] == 5 and len(c["rec_counter"]) == 8
    # (c) an interval without a pan camera: its pan means are 0 and the stopper skips it
    kinds = [both] * 5 + [("msi",)] * 5 + [both] * 10
    c = run(ref, "no_pan_interval", interval=5, kinds_per_iter=kinds, amps=[0.2 * 0.95**i for i in range(20)],
            metric_name="pan_psnr", operator="max", patience=3, seed=3)
    assert c["rec_pan_psnr"][1] == 0 and c["rec_counter"][1] == c["rec_counter"][0] and c["rec_best"][1] == c["rec_best"][0]
    # (d) no photometric term: L1 is divided by max(1, 0)
    c = run(ref, "photometric_off", interval=5, kinds_per_iter=[("pan",), ("msi",), both] * 5, amps=[0.2 * 0.96**i for i in range(15)],
            metric_name="L1", operator="min", patience=4, photometric_on=False, seed=4)
    assert all(c["rec_photometric"] == 0) and c["rec_L1"][0] > 2 * c["l1"][0]
    # (e) an all-equal observation (+inf PSNR) in the first interval, a NaN pixel in the second
    c = run(ref, "inf_and_nan", interval=4, kinds_per_iter=[both] * 12, amps=[0.2 * 0.9**i for i in range(12)],
            metric_name="photometric", operator="min", patience=2, seed=5, special={2: "equal", 11: "nan"})
    assert math.isinf(c["rec_pan_psnr"][0]) and math.isnan(c["rec_photometric"][1]) and c["rec_counter"][1] == 1


if __name__ == "__main__":
    main(sys.argv[1])
