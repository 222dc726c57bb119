"""GPU (MI355X): RAFT-large's fused encoders (eogs2_amd.raft.fold_batchnorm / FusedEncoderLarge / RAFT(encoder="fused_large")
over the eogs_flowres_* entries of eogs2_amd/csrc/flowenc.hip) under the protocols and bounds of tests/test_gpu_flowenc.py: the
fold against its float64 statement, every convolution of the two encoders per element under the bound of a float32 fma sum
with its statistics, a residual block, an encoder and the whole network against their float64 runs with torch's float32
modules as the yardstick, an encoder bit for bit against its chain written by hand, and the network behind
performOpticalmatching. Every batch norm is randomised first (tests/flowres_cases.py): a default one is the identity."""
import copy

import pytest
import torch

import flowenc_cases as ec
import flowres_cases as rc
import test_gpu_flowenc as ge

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def large(dev):
    """RAFT-large with seeded weights and randomised batch norms, in eval mode, and its float64 copy: shared, never changed."""
    from eogs2_amd import raft

    torch.manual_seed(90)
    model = raft.RAFT("large", corr="volume", update="torch", encoder="torch").eval()
    assert rc.randomise_batchnorms(model, 91) == 15
    model = model.to(dev)
    return model, copy.deepcopy(model).double()


# ---- 1. the fold ----

def ulp32(x64):
    """One float32 ulp at |x| (x float64), 2^-149 below the normals."""
    e = torch.floor(torch.log2(x64.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=x64.device), e - 23)


def run_fold(case):
    """The entry called by hand with the outputs pre-filled with NaN bytes: what the kernel does not write shows."""
    from eogs2_amd._host import call

    w, b, gamma, beta, mean, var = (t.contiguous() for t in case)
    dev = w.device
    w_out = torch.full(w.shape, float("nan"), dtype=torch.float32, device=dev)
    b_out = torch.full(b.shape, float("nan"), dtype=torch.float32, device=dev)
    call("eogs_flowres_fold", dev, w.shape[0], w.numel() // w.shape[0], w.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
         mean.data_ptr(), var.data_ptr(), 1e-5, w_out.data_ptr(), b_out.data_ptr())
    return w_out, b_out


@pytest.mark.parametrize("shape", rc.FOLD_SHAPES, ids=ge.ids)
def test_fold_against_its_statement(dev, shape):
    """w' bit for bit against the float64 product rounded to float32, b' within one float32 ulp of the float64 statement
    (one ulp, not half: a compiler may contract the multiply-add). gamma = 0 gives w' = +-0 and b' = beta exactly; var = 0
    is a channel like any other; a NaN or a negative var in one channel leaves the others' bits alone. The wrapper and a
    second run give the same bits."""
    from eogs2_amd import raft

    cout, per_out = shape
    case = tuple(t.to(dev) for t in rc.fold_case(cout, per_out, seed=600 + cout))
    assert float(case[2][0]) == 0.0  # (every 16th gamma, the first among them)
    if cout > 2:
        case[5][2] = 0.0  # var = 0: s = gamma / sqrt(eps)
    s, w64, b64 = rc.fold_oracle(*case)
    w_out, b_out = run_fold(case)
    assert bool(torch.isfinite(w_out).all()) and bool(torch.isfinite(b_out).all())
    assert torch.equal(w_out, w64), f"{int((w_out != w64).sum())} of {w64.numel()} weights differ"
    err = (b_out.double() - b64).abs()
    worst = float((err / ulp32(b64)).max())
    print(f"fold {shape}: b' at most {worst:.4f} ulp from the float64 statement")
    assert bool((err <= ulp32(b64)).all())
    zero = case[2] == 0
    assert int(zero.sum()) >= 1 and int(torch.count_nonzero(w_out[zero])) == 0 and torch.equal(b_out[zero], case[3][zero])
    if cout > 2:
        assert float(s[2]) == float((case[2][2].double() / torch.sqrt(torch.tensor(1e-5, dtype=torch.float64))).float())
    w2, b2 = raft.fold_batchnorm(*case)
    assert torch.equal(w2, w_out) and torch.equal(b2, b_out)
    again = run_fold(case)
    assert torch.equal(again[0], w_out) and torch.equal(again[1], b_out)
    for which, value in ((0, float("nan")), (1, float("nan")), (2, float("nan")), (3, float("nan")), (4, float("nan")), (5, float("nan")), (5, -1.0)):
        c = cout - 1
        bad = [t.clone() for t in case]
        if which == 0:
            bad[0][c, per_out - 1] = value
        else:
            bad[which][c] = value
        wb, bb = run_fold(tuple(bad))
        assert torch.equal(wb[:c], w_out[:c]) and torch.equal(bb[:c], b_out[:c]), which
        nan_w, nan_b = torch.isnan(wb[c]).flatten(), bool(torch.isnan(bb[c]))
        if which == 0:  # one weight: its product alone
            assert int(nan_w.sum()) == 1 and bool(nan_w[per_out - 1]) and not nan_b
        elif which in (2, 5):  # gamma or var: s, so everything of the channel
            assert bool(nan_w.all()) and nan_b
        else:  # the bias, beta or the mean: b' alone
            assert not bool(nan_w.any()) and nan_b


# ---- 2. every convolution of the table through the existing kernel ----

@pytest.mark.parametrize("config", rc.CASES, ids=ec.config_id)
@pytest.mark.parametrize("shape", ec.SHAPES + ("tile",), ids=ge.ids)
def test_convolution_against_float64(dev, shape, config):
    """tests/test_gpu_flowenc.py's check, its bounds (K + extra) U M, at RAFT-large's widths: 8 to 16 channel chunks and 2 to 8
    workgroups along Cout, which RAFT-small's encoders never gave the kernel."""
    for variant in ge.VARIANTS:
        ge.check_against_float64(dev, config, shape, variant)


@pytest.mark.parametrize("config", rc.CASES, ids=ec.config_id)
def test_statistics_against_float64(dev, config):
    """tests/test_gpu_flowenc.py's check of (mean, rstd) under its bounds; tests/test_flowres_cases.py asserts their condition
    on these very maps."""
    ge.test_statistics_against_float64(dev, config)


# ---- 3. a block, 4. an encoder: composed of the wrappers ----

def folded(unit):
    from eogs2_amd import raft

    conv, bn = unit[0], unit[1]
    return raft.fold_batchnorm(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)


def fused_block(block, x, instance):
    """One residual block over the wrappers, launch for launch what eogs_flowres_run does for it: channel-last in and out."""
    from eogs2_amd import raft

    u1, u2 = block.convnormrelu1, block.convnormrelu2
    down = None if isinstance(block.downsample, torch.nn.Identity) else block.downsample
    s = u1[0].stride[0]
    assert (s == 2) == (down is not None)
    if instance:
        r1, t1 = raft.conv2d_strided_cl(x, u1[0].weight, u1[0].bias, stride=s, stats=True)
        r2, t2 = raft.conv2d_strided_cl(r1, u2[0].weight, u2[0].bias, in_norm=t1, stats=True)
        if down is None:
            return raft.finish_cl(r2, t2, x)
        rd, td = raft.conv2d_strided_cl(x, down[0].weight, down[0].bias, stride=s, stats=True)
        return raft.finish_cl(r2, t2, rd, td)
    a = raft.conv2d_strided_cl(x, *folded(u1), stride=s, act="relu")
    res = x if down is None else raft.conv2d_strided_cl(x, *folded(down), stride=s)
    return raft.conv2d_strided_cl(a, *folded(u2), act="relu", res=res)


def fused_encoder(enc, image, instance):
    """A whole encoder over the wrappers: NCHW in and out."""
    from eogs2_amd import raft

    stem = enc.convnormrelu
    if instance:
        r, t = raft.conv2d_strided_cl(image, stem[0].weight, stem[0].bias, stride=2, stats=True, in_nchw=True)
        x = raft.finish_cl(r, t)
    else:
        x = raft.conv2d_strided_cl(image, *folded(stem), stride=2, act="relu", in_nchw=True)
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for block in layer:
            x = fused_block(block, x, instance)
    return raft.conv2d_strided_cl(x, enc.conv.weight, enc.conv.bias, out_nchw=True)


@pytest.mark.parametrize("kind", ["feature", "context"])
@pytest.mark.parametrize("where", ["layer1.1", "layer2.0"])
def test_a_block_against_its_float64_run(dev, large, kind, where):
    """One residual block without (layer1.1) and with (layer2.0) a downsample, of both encoders, composed of the wrappers,
    against the torch module in float32 and in float64 on the same device: the largest deviation from float64 is at most
    16 x the torch float32 module's own."""
    block = getattr(large[0], f"{kind}_encoder").get_submodule(where)
    block64 = getattr(large[1], f"{kind}_encoder").get_submodule(where)
    g = torch.Generator().manual_seed(93)
    x = torch.relu(torch.randn(2, 64, 17, 23, generator=g)).to(dev)  # (a block's input has been through a ReLU)
    with torch.inference_mode():
        got = fused_block(block, x.permute(0, 2, 3, 1).contiguous(), kind == "feature").permute(0, 3, 1, 2)
        t32, t64 = block(x.clone()), block64(x.double())
        o64 = rc.residual_block_oracle(block64, x.double())
    assert float((o64 - t64).abs().max()) <= 1e-12 * float(t64.abs().max())
    assert got.shape == t64.shape
    ge.report(f"block large {kind} {where}", got, t32, t64)


@pytest.mark.parametrize("kind", ["feature", "context"])
@pytest.mark.parametrize("image", rc.ENCODER_IMAGES, ids=ge.ids)
def test_an_encoder_against_its_float64_run_and_its_chain_by_hand(dev, large, image, kind):
    """FusedEncoderLarge against the torch module in float32 and float64 (the same protocol and margin), and bit for bit
    against the chain written by hand through fold_batchnorm, conv2d_strided_cl and finish_cl. The workspace is filled with
    0xFF between two calls: a call relies on nothing it did not write, and gives the same bits."""
    from eogs2_amd import raft

    enc, enc64 = getattr(large[0], f"{kind}_encoder"), getattr(large[1], f"{kind}_encoder")
    g = torch.Generator().manual_seed(94)
    x = (torch.rand(*image, generator=g) * 2 - 1).to(dev)
    fused = raft.FusedEncoderLarge(enc)
    with torch.inference_mode():
        got = fused(x)
        assert len(fused._ws) == 1
        for ws in fused._ws.values():
            assert ws.numel() >= fused.workspace_bytes(x.shape[0], x.shape[2], x.shape[3])
            ws.fill_(0xFF)
        again = fused(x)
        assert len(fused._ws) == 1
        by_hand = fused_encoder(enc, x, kind == "feature")
        t32, t64 = enc(x), enc64(x.double())
    assert got.shape == t64.shape and got.is_contiguous() and torch.equal(got, again)
    assert torch.equal(got, by_hand)
    ge.report(f"encoder large {kind} {image}", got, t32, t64)


def test_a_batch_is_its_images_and_a_nan_stays_in_its_image(dev, large):
    """A batch gives the bits of its images; under FEATURE the statistics are per image, so a NaN in image 0 makes its own map
    NaN and leaves image 1's bits alone."""
    from eogs2_amd import raft

    g = torch.Generator().manual_seed(95)
    x = (torch.rand(2, 3, 17, 23, generator=g) * 2 - 1).to(dev)
    for enc in (large[0].feature_encoder, large[0].context_encoder):
        fused = raft.FusedEncoderLarge(enc)
        clean = fused(x)
        for n in range(2):
            assert torch.equal(fused(x[n:n + 1].clone())[0], clean[n])
        bad = x.clone()
        bad[0, 1, 8, 11] = float("nan")
        out = fused(bad)
        assert bool(torch.isnan(out[0]).any()) and torch.equal(out[1], clean[1])


def test_an_encoder_keeps_a_bounded_number_of_workspaces(dev, large):
    from eogs2_amd import raft

    fused = raft.FusedEncoderLarge(large[0].context_encoder)
    g = torch.Generator().manual_seed(96)
    xs = [(torch.rand(1, 3, 16 + 3 * i, 24, generator=g) * 2 - 1).to(dev) for i in range(raft.FusedEncoderLarge.MAX_WORKSPACES + 2)]
    first = fused(xs[0])
    for x in xs[1:]:
        fused(x)
        assert len(fused._ws) <= raft.FusedEncoderLarge.MAX_WORKSPACES
    assert len(fused._ws) == raft.FusedEncoderLarge.MAX_WORKSPACES and torch.equal(fused(xs[0]), first)


def test_nothing_is_cached_and_training_mode_raises(dev, large):
    """Weights and batch-norm statistics edited in place between two calls change the result, and undoing the edit brings the
    first bits back: every call reads the module. A batch norm switched to train() raises."""
    from eogs2_amd import raft

    model = copy.deepcopy(large[0])
    g = torch.Generator().manual_seed(97)
    x = (torch.rand(1, 3, 40, 56, generator=g) * 2 - 1).to(dev)
    for enc, edits in ((model.feature_encoder, ("layer2.0.convnormrelu1.0.weight", "conv.bias")),
                       (model.context_encoder, ("layer2.0.convnormrelu1.0.weight", "layer3.1.convnormrelu2.1.running_mean",
                                                "layer1.0.convnormrelu1.1.running_var", "convnormrelu.1.weight", "layer2.0.downsample.1.bias"))):
        fused = raft.FusedEncoderLarge(enc)
        with torch.inference_mode():
            first = fused(x)
        for name in edits:
            mod, _, leaf = name.rpartition(".")
            t = getattr(enc.get_submodule(mod), leaf)
            keep = t.detach().clone()
            with torch.no_grad():
                t.mul_(1.5).add_(0.25)
            with torch.inference_mode():
                changed, want = fused(x), enc(x)
            assert not torch.equal(changed, first), name
            assert float((changed - want).abs().max()) <= 1e-3 * float(want.abs().max()), name  # (it follows the module)
            with torch.no_grad():
                t.copy_(keep)
            with torch.inference_mode():
                assert torch.equal(fused(x), first), name
    fused = raft.FusedEncoderLarge(model.context_encoder)
    model.context_encoder.layer2[1].convnormrelu2[1].train()
    with pytest.raises(RuntimeError, match="layer2.1.convnormrelu2.1 is in training mode"):
        fused(x)
    model.context_encoder.eval()
    fused(x)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model._fused_enc_large[1](x)
    model._fused_enc_large[0](x)  # (an instance norm without running statistics computes the same in both modes)


# ---- 5. the network ----

@pytest.mark.parametrize("size", [(128, 128), (128, 136)], ids=ge.ids)
def test_network_against_its_float64_run(dev, large, size):
    """RAFT("large") with the on-demand correlation, update="fused_large" and encoder="fused_large", 4 updates, against the
    plain-torch volume path in float32 and in float64, which arbitrates: at most 16 x the float32 volume path's own
    deviation, for return_all=True and for the last flow alone."""
    from eogs2_amd import raft

    model, model64 = large
    fused = raft.RAFT("large", corr="ondemand", update="fused_large", encoder="fused_large").eval().to(dev)
    fused.load_state_dict(model.state_dict())
    g = torch.Generator().manual_seed(21)
    H, W = size
    base = torch.rand(1, 3, H + 8, W + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev)
    with torch.inference_mode():
        fu = fused(a, b, num_flow_updates=4, return_all=True)
        fu_last = fused(a, b, num_flow_updates=4)
        v32 = model(a, b, num_flow_updates=4, return_all=True)
        v64 = model64(a.double(), b.double(), num_flow_updates=4, return_all=True)
    assert len(fu) == len(v32) == len(v64) == 4 and len(fu_last) == 1
    assert len(fused._fused_enc_large[0]._ws) == 1 and len(fused._fused_enc_large[1]._ws) == 1
    for f in fu:
        assert f.shape == (1, 2, H, W) and f.dtype == torch.float32 and bool(torch.isfinite(f).all())
    dev_fu = float((fu[-1].double() - v64[-1]).abs().max())
    dev_vol = float((v32[-1].double() - v64[-1]).abs().max())
    print(f"network large {size}: |fused - f64| {dev_fu:.3e}, |volume32 - f64| {dev_vol:.3e}, ratio {dev_fu / max(dev_vol, 1e-300):.3f}, "
          f"largest |flow| {float(v64[-1].abs().max()):.3f}")
    assert dev_fu <= 16 * dev_vol
    assert float((fu_last[-1].double() - v64[-1]).abs().max()) <= 16 * dev_vol
    assert not torch.equal(fu[0], fu[-1])


@pytest.mark.parametrize("mode", ["downscale", "upscale"])
def test_network_behind_perform_optical_matching(dev, large, mode):
    from eogs2_amd import flow as F
    from eogs2_amd import raft

    model = raft.raft_large(update="fused_large", encoder="fused_large").eval().to(dev)
    model.load_state_dict(large[0].state_dict())
    g = torch.Generator().manual_seed(31)
    gt, img = torch.rand(3, 130, 150, generator=g).to(dev), torch.rand(3, 130, 150, generator=g).to(dev)
    warper = F.performOpticalmatching(False, mode=mode, model_name="large", num_flow_updates=2, model=model)
    flow, gt2, img2 = warper.get_flow(gt, img)
    assert gt2.shape == img2.shape == ((3, 128, 144) if mode == "downscale" else (3, 130, 150))
    assert flow.shape == (1, 2) + tuple(gt2.shape[1:]) and flow.dtype == torch.float32 and bool(torch.isfinite(flow).all())
