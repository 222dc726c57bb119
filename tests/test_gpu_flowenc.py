"""GPU (MI355X): the flow network's fused encoders (eogs2_amd.raft.conv2d_strided_cl / finish_cl / FusedEncoder /
RAFT(encoder="fused") over eogs2_amd/csrc/flowenc.hip) against the float64 oracle of tests/flowenc_cases.py: every convolution of
RAFT-small's two encoders per element under the bound of a float32 fma sum, the statistics and the pointwise pass under
theirs, exact cases bit for bit, a block, an encoder and the whole network against their float64 runs with torch's float32
modules as the yardstick, an encoder bit for bit against its chain written by hand, and the network behind
performOpticalmatching."""
import copy
import ctypes

import pytest
import torch

import flowenc_cases as ec

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # half an ulp of 1: the unit of the bounds


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def ids(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


def input_shape(config, shape):
    from eogs2_amd import raft

    return ec.tile_input(config, *raft.conv_info()) if shape == "tile" else shape


def run_conv(x, weight, bias, stride=1, in_norm=None, res=None, act="none", in_nchw=False, out_nchw=False, stats=False):
    """The library's entries called by hand, with `out`, the packing, the partials and the norm table filled with NaN bytes
    before the call: what a kernel does not write, or reads without having been given, shows. Returns out, or (out, norm)."""
    from eogs2_amd import _abi, _lib
    from eogs2_amd._host import call, query_bytes

    dev = x.device
    N, h, w, cin = (x.shape[0], x.shape[2], x.shape[3], x.shape[1]) if in_nchw else tuple(x.shape)
    cout, k = weight.shape[0], weight.shape[2]
    ho, wo = ec.out_size(h, w, stride)
    seg = (ctypes.c_int * 1)(cin)
    size = query_bytes(_lib.get(), "flownet_conv_pack_bytes", k, 1, seg, cout)
    packed = torch.full((size,), 0xFF, dtype=torch.uint8, device=dev)
    call("eogs_flownet_conv_pack", dev, k, 1, seg, None, cin, cout, 0, cout, weight.contiguous().data_ptr(), packed.data_ptr(), size)
    out = torch.full((N, cout, ho, wo) if out_nchw else (N, ho, wo, cout), float("nan"), dtype=torch.float32, device=dev)
    partials, pbytes = None, 0
    if stats:
        rows, nb = ctypes.c_int(), ctypes.c_size_t()
        _lib.get().check(_lib.get().flowenc_conv_partials(N, ho, wo, cout, ctypes.byref(rows), ctypes.byref(nb)))
        pbytes = nb.value
        partials = torch.full((pbytes,), 0xFF, dtype=torch.uint8, device=dev)
    epi = _abi.FLOWENC_EPI_RESIDUAL if res is not None else _abi.FLOWENC_EPI_RELU if act == "relu" else _abi.FLOWENC_EPI_BIAS
    opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    call("eogs_flowenc_conv", dev, N, h, w, cin, cout, k, stride, x.contiguous().data_ptr(), opt(in_norm), packed.data_ptr(), size, opt(bias),
         opt(res), out.data_ptr(), opt(partials), pbytes, epi,
         (_abi.FLOWENC_IN_NCHW if in_nchw else 0) | (_abi.FLOWENC_OUT_NCHW if out_nchw else 0))
    if not stats:
        return out
    norm = torch.full((N, cout, 2), float("nan"), dtype=torch.float32, device=dev)
    call("eogs_flowenc_norm", dev, N, ho, wo, cout, partials.data_ptr(), pbytes, norm.data_ptr())
    return out, norm


def case_on(dev, config, shape, seed):
    return tuple(t.to(dev) for t in ec.conv_case(config, shape, seed))


VARIANTS = ("bias", "relu", "norm_relu", "residual")


def check_against_float64(dev, config, shape, variant):
    """Every element against float64, U = 2^-24, K = k k Cin, M = |bias| + conv(|x|, |W|):
      bias       (K + 2) U M: the standard bound of a length-K float32 fma sum in any fixed order, and the bias
      relu       the same: the ReLU epilogue is exact given its argument and 1-Lipschitz
      norm_relu  (K + 4) U M with M on |(x - mean) rstd| from the same float32 table: the subtraction and the product round
                 once each, the two ReLUs are exact given their arguments
      residual   (K + 3) U (M + |res|): the addition of res rounds once more
    The wrapper gives the bits of the entries called by hand, a second run the same bits."""
    from eogs2_amd import raft

    cin, cout, k, s, nchw = config
    shape = input_shape(config, shape)
    x, weight, bias, table, res = case_on(dev, config, shape, seed=100 + 7 * shape[1] + shape[2])
    kw = dict(stride=s, in_nchw=nchw)
    if variant == "norm_relu":
        kw.update(in_norm=table, act="relu")
    elif variant == "residual":
        kw.update(res=res, act="relu")
    elif variant == "relu":
        kw.update(act="relu")
    got = run_conv(x, weight, bias, **kw)
    want = ec.strided_oracle(x.double(), weight.double(), bias.double(), **{a: (b.double() if a == "res" else b) for a, b in kw.items()})
    mag = ec.strided_oracle(x.double(), weight.double(), bias.double(), magnitude=True,
                            **{a: (b.double() if a == "res" else b) for a, b in kw.items()})
    K = k * k * cin
    extra = {"bias": 2, "relu": 2, "norm_relu": 4, "residual": 3}[variant]
    ho, wo = ec.out_size(shape[1], shape[2], s)
    assert got.shape == want.shape == (shape[0], ho, wo, cout) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    err, bound = (got.double() - want).abs(), (K + extra) * U * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"conv {ec.config_id(config)} {variant} {shape}: largest multiple of the bound {worst:.4f}")
    assert bool((err <= bound).all()), f"{float((err - bound).max()):.3e} over the bound"
    assert torch.equal(raft.conv2d_strided_cl(x, weight, bias, **kw), got)
    assert torch.equal(run_conv(x, weight, bias, **kw), got)


@pytest.mark.parametrize("config", ec.CONFIGS, ids=ec.config_id)
@pytest.mark.parametrize("shape", ec.SHAPES + ("tile",), ids=ids)
def test_convolution_against_float64(dev, shape, config):
    for variant in VARIANTS:
        check_against_float64(dev, config, shape, variant)


@pytest.mark.parametrize("config", ec.CONFIGS, ids=ec.config_id)
def test_statistics_against_float64(dev, config):
    """(mean, rstd) against the float64 statistics of the STORED float32 map:
        |mean - mean64| <= U |mean64| + 2^-31 mean|v|,    |rstd - rstd64| <= 4 U rstd64
    for maps with var >= 2^-8 E[v^2] and at most 2^22 positions (tests/test_flowenc_cases.py asserts the condition on these
    very maps; DESIGN.md section 5 has the derivation). The map is the run without statistics bit for bit; the wrapper and a
    second run give the same table."""
    from eogs2_amd import raft

    cin, cout, k, s, nchw = config
    worst_mean = worst_rstd = 0.0
    for shape in ec.STATS_SHAPES + ("tile",):
        shape = input_shape(config, shape)
        x, weight, bias, _, _ = case_on(dev, config, shape, seed=500 + shape[1])
        out, norm = run_conv(x, weight, bias, stride=s, in_nchw=nchw, stats=True)
        assert torch.equal(out, run_conv(x, weight, bias, stride=s, in_nchw=nchw))
        assert ec.stats_condition(out.cpu()) >= 2.0 ** -8
        mean64, _, rstd64 = ec.stats_oracle(out)
        mean, rstd = norm[..., 0].double(), norm[..., 1].double()
        assert bool(torch.isfinite(norm).all())
        bound_mean = U * mean64.abs() + 2.0 ** -31 * out.double().abs().flatten(1, 2).mean(dim=1)
        bound_rstd = 4 * U * rstd64
        worst_mean = max(worst_mean, float(((mean - mean64).abs() / bound_mean.clamp_min(1e-300)).max()))
        worst_rstd = max(worst_rstd, float(((rstd - rstd64).abs() / bound_rstd).max()))
        assert bool(((mean - mean64).abs() <= bound_mean).all()) and bool(((rstd - rstd64).abs() <= bound_rstd).all()), shape
        o2, n2 = raft.conv2d_strided_cl(x, weight, bias, stride=s, in_nchw=nchw, stats=True)
        assert torch.equal(o2, out) and torch.equal(n2, norm)
        assert torch.equal(run_conv(x, weight, bias, stride=s, in_nchw=nchw, stats=True)[1], norm)
    print(f"statistics {ec.config_id(config)}: largest multiples of the bounds: mean {worst_mean:.4f}, rstd {worst_rstd:.4f}")


STRIDED = tuple(c for c in ec.CONFIGS if c[3] == 2)


@pytest.mark.parametrize("config", STRIDED + ((8, 8, 3, 1, False),), ids=ec.config_id)
def test_convolution_exact_cases(dev, config):
    """Bit for bit. An all-zero input returns the bias. A single 1.0 at each corner and at the centre of an odd-sized map, in
    the last channel, returns bias + the weight's tap at exactly the outputs that read it: out(oy, ox) reads
    in(s oy + ky - p, s ox + kx - p), so under stride 2 a position is read through the taps of its own parity only. One
    NaN (no statistics) gives NaN at exactly that footprint."""
    cin, cout, k, s, nchw = config
    shape = input_shape(config, "tile")
    N, h, w = shape
    ho, wo = ec.out_size(h, w, s)
    x, weight, bias, _, _ = case_on(dev, config, shape, seed=200)
    p = (k - 1) // 2
    zero = torch.zeros_like(x)
    assert torch.equal(run_conv(zero, weight, bias, stride=s, in_nchw=nchw), bias.expand(N, ho, wo, cout))
    ch = cin - 1
    for y, xx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2), (h // 2 + 1, w // 2 + 1)):
        xs = zero.clone()
        if nchw:
            xs[0, ch, y, xx] = 1.0
        else:
            xs[0, y, xx, ch] = 1.0
        want = bias.expand(N, ho, wo, cout).clone()
        foot = torch.zeros(ho, wo, dtype=torch.bool, device=dev)
        for ky in range(k):
            for kx in range(k):
                ny, nx = y - (ky - p), xx - (kx - p)  # s oy = ny, s ox = nx
                if ny % s == 0 and nx % s == 0 and 0 <= ny // s < ho and 0 <= nx // s < wo:
                    want[0, ny // s, nx // s] = weight[:, ch, ky, kx] + bias
                    foot[ny // s, nx // s] = True
        got = run_conv(xs, weight, bias, stride=s, in_nchw=nchw)
        assert torch.equal(got, want), (y, xx)
        if k == 1:
            assert int(foot.sum()) == (1 if y % s == 0 and xx % s == 0 else 0)
        if nchw:
            xs[0, ch, y, xx] = float("nan")
        else:
            xs[0, y, xx, ch] = float("nan")
        nan = torch.isnan(run_conv(xs, weight, bias, stride=s, in_nchw=nchw))
        assert bool((nan == foot[None, :, :, None].expand_as(nan)).all()), (y, xx)


@pytest.mark.parametrize("config", ec.CONFIGS, ids=ec.config_id)
def test_convolution_of_a_batch_is_its_images_and_layouts_agree(dev, config):
    """A batch gives the bits of its images, the statistics included; reading NCHW and writing NCHW give the bits of the
    channel-last run."""
    cin, cout, k, s, nchw = config
    x, weight, bias, table, res = case_on(dev, config, (2, 17, 19), seed=300)
    both, norm = run_conv(x, weight, bias, stride=s, in_nchw=nchw, stats=True)
    tail = run_conv(x, weight, bias, stride=s, in_nchw=nchw, in_norm=table, res=res, act="relu")
    for n in range(2):
        # (clones: a slice of the batch may start off a 16-byte boundary, which the library refuses)
        one, norm1 = run_conv(x[n:n + 1].clone(), weight, bias, stride=s, in_nchw=nchw, stats=True)
        assert torch.equal(one[0], both[n]) and torch.equal(norm1[0], norm[n]), n
        t1 = run_conv(x[n:n + 1].clone(), weight, bias, stride=s, in_nchw=nchw, in_norm=table[n:n + 1].clone(), res=res[n:n + 1].clone(), act="relu")
        assert torch.equal(t1[0], tail[n]), n
    other = x.permute(0, 2, 3, 1).contiguous() if nchw else x.permute(0, 3, 1, 2).contiguous()
    assert torch.equal(run_conv(other, weight, bias, stride=s, in_nchw=not nchw), both)
    planar = run_conv(x, weight, bias, stride=s, in_nchw=nchw, out_nchw=True)
    assert planar.shape == (2, cout) + tuple(both.shape[1:3]) and torch.equal(planar.permute(0, 2, 3, 1), both)


def test_a_constant_map_is_exactly_zero_after_normalisation(dev):
    """A zero input leaves the bias at every position: the double sums of n equal float32 values and of their squares are
    exact, so mean is the value, var is 0, rstd is 1 / sqrt(1e-5) rounded once, and the normalised map is exactly 0."""
    from eogs2_amd import raft

    config = (16, 16, 3, 2, False)
    x, weight, bias, _, _ = case_on(dev, config, (2, 17, 19), seed=310)
    out, norm = run_conv(torch.zeros_like(x), weight, bias, stride=2, stats=True)
    assert torch.equal(norm[..., 0], bias.expand(2, 16))
    assert torch.equal(norm[..., 1].cpu(), torch.full((2, 16), float(1.0 / torch.sqrt(torch.tensor(1e-5, dtype=torch.float64))), dtype=torch.float32))
    done = raft.finish_cl(out, norm)
    assert done.shape == out.shape and int(torch.count_nonzero(done)) == 0


@pytest.mark.parametrize("shape", [(1, 5, 7, 32), (2, 17, 19, 96), (1, 9, 33, 64)], ids=ids)
def test_finish_against_float64(dev, shape):
    """out = relu(S + relu((v - mean) rstd)) per element against float64 from the same float32 tables, within
    4 U (|S| + |(v - mean) rstd|): the subtraction, the product (twice for the normalised shortcut) and the addition round
    once each. The three shortcut forms; a second run gives the same bits."""
    from eogs2_amd import raft

    N, h, w, C = shape
    g = torch.Generator().manual_seed(320 + h)
    v, s = torch.randn(N, h, w, C, generator=g).to(dev), torch.randn(N, h, w, C, generator=g).to(dev)
    tv = torch.stack([torch.randn(N, C, generator=g) * 0.5, torch.rand(N, C, generator=g) * 1.5 + 0.5], dim=-1).to(dev)
    ts = torch.stack([torch.randn(N, C, generator=g) * 0.5, torch.rand(N, C, generator=g) * 1.5 + 0.5], dim=-1).to(dev)
    for name, args in (("none", (None, None)), ("plain", (s, None)), ("norm", (s, ts))):
        got = raft.finish_cl(v, tv, *args)
        d = [None if t is None else (t.double() if t is s else t) for t in args]
        want = ec.finish_oracle(v.double(), tv, *d)
        bound = 4 * U * ec.finish_oracle(v.double(), tv, *d, magnitude=True)
        err = (got.double() - want).abs()
        print(f"finish {name} {shape}: largest multiple of the bound {float((err / bound.clamp_min(1e-300)).max()):.4f}")
        assert got.shape == v.shape and bool((err <= bound).all()), name
        assert bool((got >= 0).all()) and torch.equal(raft.finish_cl(v, tv, *args), got)
    nan = v.clone()
    nan[0, 1, 2, 3] = float("nan")
    hit = torch.isnan(raft.finish_cl(nan, tv, s, ts))
    assert int(hit.sum()) == 1 and bool(hit[0, 1, 2, 3])


def fused_block(block, x, norm):
    """One bottleneck over the wrappers, launch for launch what eogs_flowenc_run does for it: channel-last in and out."""
    from eogs2_amd import raft

    c1, c2, c3 = block.convnormrelu1[0], block.convnormrelu2[0], block.convnormrelu3[0]
    down = None if isinstance(block.downsample, torch.nn.Identity) else block.downsample[0]
    s = c2.stride[0]
    if norm:
        r1, t1 = raft.conv2d_strided_cl(x, c1.weight, c1.bias, stats=True)
        r2, t2 = raft.conv2d_strided_cl(r1, c2.weight, c2.bias, stride=s, in_norm=t1, stats=True)
        r3, t3 = raft.conv2d_strided_cl(r2, c3.weight, c3.bias, in_norm=t2, stats=True)
        if down is None:
            return raft.finish_cl(r3, t3, x)
        rd, td = raft.conv2d_strided_cl(x, down.weight, down.bias, stride=s, stats=True)
        return raft.finish_cl(r3, t3, rd, td)
    a = raft.conv2d_strided_cl(x, c1.weight, c1.bias, act="relu")
    b = raft.conv2d_strided_cl(a, c2.weight, c2.bias, stride=s, act="relu")
    res = x if down is None else raft.conv2d_strided_cl(x, down.weight, down.bias, stride=s)
    return raft.conv2d_strided_cl(b, c3.weight, c3.bias, act="relu", res=res)


def fused_encoder(enc, image, norm):
    """A whole encoder over the wrappers, launch for launch what eogs_flowenc_run does: NCHW in and out."""
    from eogs2_amd import raft

    stem = enc.convnormrelu[0]
    if norm:
        r, t = raft.conv2d_strided_cl(image, stem.weight, stem.bias, stride=2, stats=True, in_nchw=True)
        x = raft.finish_cl(r, t)
    else:
        x = raft.conv2d_strided_cl(image, stem.weight, stem.bias, stride=2, act="relu", in_nchw=True)
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for block in layer:
            x = fused_block(block, x, norm)
    return raft.conv2d_strided_cl(x, enc.conv.weight, enc.conv.bias, out_nchw=True)


def report(name, got, t32, t64, margin=16):
    mine, theirs = float((got.double() - t64).abs().max()), float((t32.double() - t64).abs().max())
    print(f"{name}: |fused - f64| {mine:.3e}, |torch32 - f64| {theirs:.3e}, ratio {mine / max(theirs, 1e-300):.3f}, "
          f"largest |value| {float(t64.abs().max()):.3f}")
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert mine <= margin * theirs, name


@pytest.mark.parametrize("kind", ["feature", "context"])
@pytest.mark.parametrize("where", ["layer1.1", "layer2.0"])
def test_a_block_against_its_float64_run(dev, kind, where):
    """One bottleneck without (layer1.1) and with (layer2.0) a downsample, of both encoders, composed of the wrappers, against
    the torch module in float32 and in float64 on the same device, seeded default weights, eval mode: the largest deviation
    from float64 is at most 16 x the torch float32 module's own, tests/test_gpu_flownet.py's margin."""
    from eogs2_amd import raft

    torch.manual_seed(80)
    model = raft.raft_small(update="torch").eval().to(dev)
    block = getattr(model, f"{kind}_encoder").get_submodule(where)
    block64 = copy.deepcopy(block).double()
    g = torch.Generator().manual_seed(81)
    x = torch.relu(torch.randn(2, 32, 17, 23, generator=g)).to(dev)  # (a block's input has been through a ReLU)
    with torch.inference_mode():
        got = fused_block(block, x.permute(0, 2, 3, 1).contiguous(), kind == "feature").permute(0, 3, 1, 2)
        t32, t64 = block(x.clone()), block64(x.double())
        o64 = ec.block_oracle(block64, x.double(), kind == "feature")
    assert float((o64 - t64).abs().max()) <= 1e-12 * float(t64.abs().max())
    assert got.shape == t64.shape
    report(f"block {kind} {where}", got, t32, t64)


@pytest.mark.parametrize("kind", ["feature", "context"])
@pytest.mark.parametrize("image", ec.ENCODER_IMAGES, ids=ids)
def test_an_encoder_against_its_float64_run(dev, image, kind):
    """FusedEncoder against the torch module in float32 and float64 (the same protocol and margin), and bit for bit against the
    chain written by hand through conv2d_strided_cl and finish_cl. The workspace is filled with 0xFF between two calls: a call
    relies on nothing it did not write, and gives the same bits."""
    from eogs2_amd import raft

    torch.manual_seed(82)
    model = raft.raft_small(update="torch").eval().to(dev)
    enc = getattr(model, f"{kind}_encoder")
    enc64 = copy.deepcopy(enc).double()
    g = torch.Generator().manual_seed(83)
    x = (torch.rand(*image, generator=g) * 2 - 1).to(dev)
    fused = raft.FusedEncoder(enc)
    with torch.inference_mode():
        got = fused(x)
        assert len(fused._ws) == 1
        for ws in fused._ws.values():
            ws.fill_(0xFF)
        again = fused(x)
        assert len(fused._ws) == 1
        by_hand = fused_encoder(enc, x, kind == "feature")
        t32, t64 = enc(x), enc64(x.double())
    assert got.shape == t64.shape and got.is_contiguous() and torch.equal(got, again)
    assert torch.equal(got, by_hand)
    report(f"encoder {kind} {image}", got, t32, t64)


def test_an_encoder_keeps_a_bounded_number_of_workspaces(dev):
    """One workspace per image shape, at most FusedEncoder.MAX_WORKSPACES of them: a caller whose sizes vary does not collect
    one per size, and a shape whose workspace was dropped gives the same bits when it comes back."""
    from eogs2_amd import raft

    torch.manual_seed(86)
    fused = raft.FusedEncoder(raft.raft_small(update="torch").eval().to(dev).context_encoder)
    g = torch.Generator().manual_seed(87)
    xs = [(torch.rand(1, 3, 16 + 3 * i, 24, generator=g) * 2 - 1).to(dev) for i in range(raft.FusedEncoder.MAX_WORKSPACES + 2)]
    first = fused(xs[0])
    for x in xs[1:]:
        fused(x)
        assert len(fused._ws) <= raft.FusedEncoder.MAX_WORKSPACES
    assert len(fused._ws) == raft.FusedEncoder.MAX_WORKSPACES and torch.equal(fused(xs[0]), first)


def test_a_nan_in_one_image_leaves_the_other_untouched(dev):
    """Under FEATURE the statistics are per image: a NaN in image 0 makes its own map NaN and leaves image 1's bits alone;
    a batch gives the bits of its images."""
    from eogs2_amd import raft

    torch.manual_seed(84)
    model = raft.raft_small(update="torch").eval().to(dev)
    g = torch.Generator().manual_seed(85)
    x = (torch.rand(2, 3, 17, 23, generator=g) * 2 - 1).to(dev)
    for enc in (model.feature_encoder, model.context_encoder):
        fused = raft.FusedEncoder(enc)
        clean = fused(x)
        for n in range(2):
            assert torch.equal(fused(x[n:n + 1].clone())[0], clean[n])
        bad = x.clone()
        bad[0, 1, 8, 11] = float("nan")
        out = fused(bad)
        assert bool(torch.isnan(out[0]).any()) and torch.equal(out[1], clean[1])


@pytest.mark.parametrize("size", [(128, 128), (128, 136)], ids=ids)
def test_network_against_its_float64_run(dev, size):
    """tests/test_gpu_raft.py's protocol for RAFT-small with encoder="fused": seeded random weights, eval mode, 4 updates; the
    fused encoders and update over the on-demand correlation against the plain-torch volume path in float32 and in float64,
    which arbitrates. The same 16 x, for return_all=True and for the last flow alone."""
    from eogs2_amd import raft

    torch.manual_seed(20)
    model = raft.RAFT("small", corr="volume", update="torch", encoder="torch").eval().to(dev)
    g = torch.Generator().manual_seed(21)
    H, W = size
    base = torch.rand(1, 3, H + 8, W + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev)
    with torch.inference_mode():
        model.corr, model.update, model.encoder = "ondemand", "fused", "fused"
        fu = model(a, b, num_flow_updates=4, return_all=True)
        fu_last = model(a, b, num_flow_updates=4)
        model.corr, model.update, model.encoder = "volume", "torch", "torch"
        v32 = model(a, b, num_flow_updates=4, return_all=True)
        m64 = model.double()
        v64 = m64(a.double(), b.double(), num_flow_updates=4, return_all=True)
    assert len(fu) == len(v32) == len(v64) == 4 and len(fu_last) == 1
    for f in fu:
        assert f.shape == (1, 2, H, W) and f.dtype == torch.float32 and bool(torch.isfinite(f).all())
    dev_fu = float((fu[-1].double() - v64[-1]).abs().max())
    dev_vol = float((v32[-1].double() - v64[-1]).abs().max())
    print(f"network small {size}: |fused - f64| {dev_fu:.3e}, |volume32 - f64| {dev_vol:.3e}, ratio {dev_fu / max(dev_vol, 1e-300):.3f}, "
          f"largest |flow| {float(v64[-1].abs().max()):.3f}")
    assert dev_fu <= 16 * dev_vol
    assert float((fu_last[-1].double() - v64[-1]).abs().max()) <= 16 * dev_vol
    assert not torch.equal(fu[0], fu[-1])


@pytest.mark.parametrize("mode", ["downscale", "upscale"])
def test_network_behind_perform_optical_matching(dev, mode):
    from eogs2_amd import flow as F
    from eogs2_amd import raft

    torch.manual_seed(30)
    model = raft.raft_small(update="fused", encoder="fused").eval().to(dev)
    g = torch.Generator().manual_seed(31)
    gt, img = torch.rand(3, 130, 150, generator=g).to(dev), torch.rand(3, 130, 150, generator=g).to(dev)
    warper = F.performOpticalmatching(False, mode=mode, model_name="small", num_flow_updates=2, model=model)
    flow, gt2, img2 = warper.get_flow(gt, img)
    assert gt2.shape == img2.shape == ((3, 128, 144) if mode == "downscale" else (3, 130, 150))
    assert flow.shape == (1, 2) + tuple(gt2.shape[1:]) and flow.dtype == torch.float32 and bool(torch.isfinite(flow).all())
