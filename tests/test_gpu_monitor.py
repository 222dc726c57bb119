"""GPU: the training monitor (eogs2_amd.monitor, include/eogs_monitor.h) against a float64 evaluation of the reference's
formulas (values), against the plain restatement of tests/monitor_cases.py fed the device's own fp32 values (accumulation:
bit for bit) and against the fixtures made by the reference's functions (stopper decisions, means)."""
import math

import numpy as np
import pytest
import torch

import monitor_cases as mc

pytestmark = pytest.mark.gpu

LAM = 0.2
PSNR_ATOL = 10.0 / math.log(10.0) * 1e-5  # the 1e-5 relative bar on the mse, carried through 10 log10: derived, not measured
SHAPES = [(1, 7, 9), (3, 5, 7), (1, 64, 64), (3, 33, 70), (3, 67, 131)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from eogs2_amd import _lib

    assert _lib.get().backend == "hip-gfx950"
    return torch.device("cuda:0")


def _close_val(a, b, what, rtol=1e-5):  # test_gpu_loss._close_val: the project's bar for loss values
    a, b = float(a), float(b)
    assert abs(a - b) <= rtol * max(abs(b), 1e-3), f"{what}: {a} vs {b}"


def _pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    return (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1), gt


def _f64(img, gt, lam=LAM):
    from oracle import loss_oracle as lo

    l1, ssim = float(lo.l1_loss(img, gt)), float(lo.ssim(img, gt))
    return {"l1": l1, "ssim": ssim, "photometric": (1.0 - lam) * l1 + lam * (1.0 - ssim), "psnr": mc.psnr_f64(img.numpy(), gt.numpy())}


def _observe(mon, img, gt, kind, with_loss_out, lam=LAM, on=True, gate=None):
    from eogs2_amd import losses

    if with_loss_out:
        out = losses.photometric_loss(img, gt, lam, return_out=True)[2]
        mon.observe(img, gt, kind, loss_out=out, lambda_dssim=lam, photometric_on=on, gate=gate)
    else:
        mon.observe(img, gt, kind, lambda_dssim=lam, photometric_on=on, gate=gate)


def _f32bits(v):
    return int(np.float32(v).view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES)
def test_values_match_float64_on_both_paths(dev, shape):
    from eogs2_amd.monitor import TrainingMonitor

    img, gt = _pair(shape, seed=sum(shape))
    want = _f64(img, gt)
    x, y = img.to(dev), gt.to(dev)
    last = {}
    for path in (True, False):
        mon = TrainingMonitor(dev)
        _observe(mon, x, y, "pan" if shape[0] == 1 else "msi", path)
        s = mon.snapshot()
        last[path] = s["last"]
        print(shape, "loss_out" if path else "stand-alone", {k: (v, want[k]) for k, v in s["last"].items()})
        for k in ("l1", "ssim", "photometric"):
            _close_val(s["last"][k], want[k], f"{shape}:{k}")
        assert abs(s["last"]["psnr"] - want["psnr"]) <= PSNR_ATOL, (shape, s["last"]["psnr"], want["psnr"])
        kind = "pan" if shape[0] == 1 else "msi"
        assert s["n_" + kind] == 1 and s["n_photo"] == 1 and s["sums"]["L1"] == s["last"]["l1"]
        assert s["sums"][kind + "_psnr"] == s["last"]["psnr"] and s["sums"]["photometric"] == s["last"]["photometric"]
    for k in ("l1", "ssim", "photometric", "psnr"):  # the two paths: the same bits
        assert _f32bits(last[True][k]) == _f32bits(last[False][k]), k
    # a base that is not 16-byte aligned takes scalar loads and the same order of sums: the same bits
    pad = lambda t: torch.cat([torch.zeros(1, device=dev), t.reshape(-1)])[1:].view(shape)  # noqa: E731
    xo, yo = pad(x), pad(y)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    mon = TrainingMonitor(dev)
    _observe(mon, xo, yo, "msi", True)
    assert _f32bits(mon.snapshot()["last"]["psnr"]) == _f32bits(last[True]["psnr"])


def test_inf_and_nan_come_out_as_the_references(dev):
    from eogs2_amd.monitor import TrainingMonitor

    img, gt = _pair((3, 33, 70), seed=7)
    img[1] = gt[1]  # one all-equal plane: its mse is 0, its PSNR +inf, and so is the mean
    want = _f64(img, gt)
    assert math.isinf(want["psnr"]) and want["psnr"] > 0
    for path in (True, False):
        mon = TrainingMonitor(dev)
        _observe(mon, img.to(dev), gt.to(dev), "msi", path)
        s = mon.snapshot()
        assert s["last"]["psnr"] == math.inf and s["sums"]["msi_psnr"] == math.inf
        _close_val(s["last"]["l1"], want["l1"], "l1")
        _close_val(s["last"]["ssim"], want["ssim"], "ssim")
    eq = gt[:1].clone()
    mon = TrainingMonitor(dev)
    _observe(mon, eq.to(dev), eq.to(dev), "pan", True)
    s = mon.snapshot()["last"]
    assert s["psnr"] == math.inf and s["l1"] == 0.0 and abs(s["ssim"] - 1.0) <= 1e-5
    bad = img.clone()
    bad[2, 32, 69] = float("nan")  # the plane's last element: the scalar tail of a plane whose base is not 16-byte aligned
    for path in (True, False):
        mon = TrainingMonitor(dev, metric_name="photometric", operator="min", patience=1)
        _observe(mon, bad.to(dev), gt.to(dev), "msi", path)
        mon.end_iteration(torch.zeros((), device=dev))
        mon.close_interval()
        s = mon.snapshot()
        assert all(math.isnan(v) for v in s["last"].values()), s["last"]
        r = s["ring"][0]
        assert math.isnan(r["photometric"]) and r["counter"] == 1 and r["early_stop"] and r["best"] == math.inf  # NaN: no improvement


@pytest.mark.parametrize("name", mc.FIXTURES)
def test_accumulation_is_exact(dev, name):
    from eogs2_amd.monitor import TrainingMonitor

    c = mc.load(name)
    lam, patience = float(c["lambda_dssim"]), int(c["patience"])
    mon = TrainingMonitor(dev, metric_name=str(c["metric_name"]), operator=str(c["operator"]), patience=patience)
    dev_img = {k: torch.from_numpy(c["img_" + k]).to(dev) for k in ("pan", "msi")}
    dev_gt = {k: torch.from_numpy(c["gt_" + k]).to(dev) for k in ("pan", "msi")}
    loss = torch.from_numpy(c["loss"]).to(dev)
    seen = {"pan": 0, "msi": 0}
    vals = {k: [] for k in ("l1", "ssim", "photometric", "psnr")}

    def observe(i, kind, on):
        _observe(mon, dev_img[kind][seen[kind]], dev_gt[kind], kind, with_loss_out=i % 2 == 0, lam=lam, on=on)
        seen[kind] += 1
        last = mon.snapshot()["last"]
        for k in vals:
            vals[k].append(np.float32(last[k]))

    mc.drive(c, observe, lambda it: mon.end_iteration(loss[it]), mon.close_interval)
    # the device's own fp32 values, through the plain restatement: the same records, bit for bit
    want = mc.replay(c, values={k: np.array(v, dtype=np.float32) for k, v in vals.items()})
    s = mon.snapshot()
    got = s["ring"]
    assert len(got) == len(want.records) == len(c["rec_iteration"])
    for a, b in zip(got, want.records):
        assert mc.same_record(a, b), mc.record_diff(a, b)
    assert mc.bits(s["ema_loss"]) == mc.bits(want.ema_loss) and mc.bits(s["ema_photometric"]) == mc.bits(want.ema_photometric)
    for k in mc.METRICS:
        assert mc.bits(s["sums"][k]) == mc.bits(want.sums[k]), k  # the interval left open
    assert (s["n_photo"], s["n_pan"], s["n_msi"]) == (want.n["photo"], want.n["pan"], want.n["msi"])
    newest = mon.fetch()
    assert mc.same_record(newest, got[-1]) if got else newest is None
    # against the reference's run: the same decisions, means within the bar for loss values
    ref = mc.fixture_records(c)
    for a, b in zip(got, ref):
        assert (a["iteration"], a["counter"], a["early_stop"]) == (b["iteration"], b["counter"], b["early_stop"]), (a, b)
        for k in mc.METRICS + ("best", "ema_loss", "ema_photometric"):
            print(name, a["interval"], k, a[k], b[k])
            if math.isfinite(b[k]):
                _close_val(a[k], b[k], f"{name}:{a['interval']}:{k}")
            else:
                assert mc.bits(a[k]) == mc.bits(b[k]), (k, a[k], b[k])
    assert next((r["interval"] for r in got if r["early_stop"]), 0) == int(c["stop_interval"])


@pytest.mark.parametrize("P", [1, 63, 64, 65, 4097, 70001])
def test_model_reduction(dev, P):
    from eogs2_amd.monitor import TrainingMonitor
    from eogs2_amd.optim import RETIRED_LOGIT

    g = torch.Generator().manual_seed(P)
    o = (torch.rand(P, 1, generator=g) * 24.0 - 12.0)
    o[::5] = 0.0
    o[1::3] = RETIRED_LOGIT  # a third of the rows retired (with P == 1 row 0 stays)
    alive = o.reshape(-1) > 0.5 * RETIRED_LOGIT
    want_rows = int(alive.sum())
    want_mean = float(torch.sigmoid(o.double().reshape(-1)[alive]).mean()) if want_rows else 0.0
    mon = TrainingMonitor(dev)
    mon.observe_model(o.to(dev))
    s = mon.snapshot()
    print(P, s["rows"], s["mean_opacity"], want_mean)
    assert s["rows"] == want_rows
    # fp32 sigmoid per row (all terms positive: the sum's relative error is at most a row's), double sum, one final rounding
    assert abs(s["mean_opacity"] - want_mean) <= 4 * 2.0**-24 * want_mean
    # a base that is not 16-byte aligned: scalar loads, the same order, the same bits; a (P,) view is accepted
    shifted = torch.cat([torch.zeros(1, 1), o]).to(dev)[1:]
    assert shifted.data_ptr() % 16 == 4
    mon2 = TrainingMonitor(dev)
    mon2.observe_model(shifted.view(-1))
    s2 = mon2.snapshot()
    assert s2["rows"] == want_rows and _f32bits(s2["mean_opacity"]) == _f32bits(s["mean_opacity"])
    # every row retired: no row, mean 0
    mon.observe_model(torch.full((P, 1), RETIRED_LOGIT, device=dev))
    s = mon.snapshot()
    assert s["rows"] == 0 and s["mean_opacity"] == 0.0


def _sequence(n, shape, P):
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(shape, generator=g)
    imgs = [(gt + (0.3 * 0.95**i) * torch.randn(shape, generator=g)).clamp(0, 1) for i in range(n)]
    logits = [torch.rand(P, 1, generator=g) * 8.0 - 4.0 for _ in range(n)]
    return gt, imgs, logits


def test_graph_replays_equal_the_eager_run_and_the_gate_holds(dev):
    from eogs2_amd import losses
    from eogs2_amd.monitor import TrainingMonitor

    N, shape, P = 25, (3, 33, 70), 4097
    gt, imgs, logits = _sequence(N, shape, P)
    gt_d = gt.to(dev)
    imgs_d, logits_d = [t.to(dev) for t in imgs], [t.to(dev) for t in logits]

    def step(mon, img, lg, gate):
        loss, _, out = losses.photometric_loss(img, gt_d, LAM, return_out=True)
        mon.observe(img, gt_d, "msi", loss_out=out, lambda_dssim=LAM, gate=gate)
        mon.observe_model(lg, gate=gate)
        mon.end_iteration(loss.detach(), gate=gate)

    def eager(stream):
        with torch.cuda.stream(stream):
            mon = TrainingMonitor(dev, metric_name="msi_psnr", operator="max", patience=1)
            gate = torch.ones(2, dtype=torch.int32, device=dev)
            for i in range(N):
                step(mon, imgs_d[i], logits_d[i], gate)
                if (i + 1) % 10 == 0:
                    mon.close_interval(gate=gate)
            stream.synchronize()
            return mon.snapshot()

    first = eager(torch.cuda.current_stream(dev))
    assert first["intervals"] == 2 and first["iteration"] == N and first["n_msi"] == 5 and first["rows"] == P
    second = eager(torch.cuda.Stream(dev))  # another stream: the same bits
    assert second["bytes"] == first["bytes"]

    # one linear graph of the step, one of the interval's close; static inputs refilled between replays
    mon = TrainingMonitor(dev, metric_name="msi_psnr", operator="max", patience=1)
    img_buf, lg_buf = torch.empty_like(imgs_d[0]), torch.empty_like(logits_d[0])
    gate = torch.ones(2, dtype=torch.int32, device=dev)
    img_buf.copy_(imgs_d[0])
    lg_buf.copy_(logits_d[0])
    step(mon, img_buf, lg_buf, gate)  # eager warm-up: workspaces exist before the recording
    mon.close_interval(gate=gate)
    mon.reset()
    torch.cuda.synchronize()
    g_step, g_close = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_step):
        step(mon, img_buf, lg_buf, gate)
    with torch.cuda.graph(g_close, pool=g_step.pool()):
        mon.close_interval(gate=gate)
    for i in range(N):
        img_buf.copy_(imgs_d[i])
        lg_buf.copy_(logits_d[i])
        g_step.replay()
        if (i + 1) % 10 == 0:
            g_close.replay()
    torch.cuda.synchronize()
    replayed = mon.snapshot()
    assert replayed["bytes"] == first["bytes"], {k: (replayed[k], first[k]) for k in replayed if k != "bytes" and replayed[k] != first[k]}
    assert len(replayed["ring"]) == 2 and replayed["ring"][1]["iteration"] == 20
    # a replay behind a closed gate leaves every byte of the state as it was
    gate.zero_()
    img_buf.copy_(imgs_d[3])
    g_step.replay()
    g_close.replay()
    torch.cuda.synchronize()
    assert mon.snapshot()["bytes"] == replayed["bytes"]
    gate.fill_(1)
    g_step.replay()
    torch.cuda.synchronize()
    after = mon.snapshot()
    assert after["iteration"] == N + 1 and after["n_msi"] == 6  # (and an open gate lets the same graph count again)


def test_fetch_async_and_poll(dev):
    from eogs2_amd.monitor import TrainingMonitor

    img, gt = _pair((1, 64, 64), seed=3)
    mon = TrainingMonitor(dev, metric_name="pan_ssim", operator="max", patience=2)
    assert mon.poll() is None and mon.fetch() is None  # nothing closed yet
    for k in range(3):
        _observe(mon, img.to(dev), gt.to(dev), "pan", True)
        mon.observe_model(torch.zeros(65, 1, device=dev))
        mon.end_iteration(torch.full((), 0.5, device=dev))
        mon.close_interval()
        mon.fetch_async()
    torch.cuda.synchronize()
    rec = mon.poll()
    assert rec == mon.fetch() and rec["interval"] == 3 and rec["iteration"] == 3 and rec["rows"] == 65 and rec["mean_opacity"] == 0.5
    assert rec["counter"] == 2 and rec["early_stop"]  # the same metric three times: strict > never holds again
    assert mon.poll() == rec  # nothing newer: the same record again
