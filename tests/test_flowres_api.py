"""CPU: the surface of RAFT-large's fused encoders (the eogs_flowres_* entries of include/eogs_resample.h,
eogs2_amd.raft.fold_batchnorm / FusedEncoderLarge / RAFT(encoder="fused_large")) without a device: header and binding table,
every stated refusal before a launch, what the wrappers refuse, and that encoder="torch" and "auto" off the GPU are today's
forward bit for bit."""
import copy
import ctypes
import functools
import os
import pickle
import re

import pytest
import torch

import abi_cases as AC
import flowres_cases as rc


@pytest.fixture(scope="module")
def lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


NAMES = ["eogs_flowres_bytes", "eogs_flowres_fold", "eogs_flowres_run"]


def test_header_table_and_constants_agree():
    from eogs2_amd import _abi

    assert _abi.ABI_VERSION == 8  # entry points were added, nothing changed
    decl = {k: v for k, v in AC.declared("eogs_resample.h").items() if k.startswith("eogs_flowres_")}
    table = {k: v for k, v in _abi.HEADERS["eogs_resample.h"].items() if k.startswith("eogs_flowres_")}
    assert sorted(decl) == sorted(table) == NAMES
    for name, (res, args) in table.items():
        assert decl[name] == len(args) and res is ctypes.c_int, name
        assert name in _abi.HIP_ONLY
    assert table["eogs_flowres_fold"][1][8] is ctypes.c_double  # eps
    defines = {k: int(v) for k, v in re.findall(r"#define (EOGS_FLOWRES_[A-Z0-9_]+) (\d+)u?\b", AC.header_text("eogs_resample.h"))}
    assert defines == {"EOGS_FLOWRES_PARAMS": _abi.FLOWRES_PARAMS, "EOGS_FLOWRES_BN": _abi.FLOWRES_BN} == {"EOGS_FLOWRES_PARAMS": 32, "EOGS_FLOWRES_BN": 60}
    with open(os.path.join(AC.INCLUDE, "eogs_resample.h")) as f:  # (the statement stands in a comment, which header_text strips)
        text = f.read()
    for line in ("s[c] = float(gamma[c] / sqrt(double(var[c]) + eps))", "w'[c, .] = w[c, .] * s[c]",
                 "b'[c] = float((double(b[c]) - double(mean[c])) * double(s[c]) + double(beta[c]))"):
        assert line in text, line


def test_library_refuses_before_a_launch(lib):
    """Every refusal comes back as a status with a message before anything touches a device (there is none here): the
    pointers are made up and never read."""
    from eogs2_amd._abi import FLOWENC_CONTEXT, FLOWENC_FEATURE, FLOWRES_BN, FLOWRES_PARAMS

    assert lib.cdll.eogs_rast_abi_version() == 8
    err = lib.cdll.eogs_rast_last_error
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)  # (never dereferenced: every call below is refused)
    n = ctypes.c_size_t()

    def fold(cout=64, per_out=147, w=p, b=p, gamma=p, beta=p, mean=p, var=p, eps=1e-5, w_out=p, b_out=p):
        return lib.flowres_fold(cout, per_out, w, b, gamma, beta, mean, var, eps, w_out, b_out, None)

    pointers = ("w", "b", "gamma", "beta", "mean", "var", "w_out", "b_out")
    for kw in [dict(cout=0), dict(per_out=0), dict(cout=-1), dict(cout=5000), dict(cout=4096, per_out=1 << 20)] + \
            [{k: None} for k in pointers] + [{k: odd} for k in pointers]:
        assert fold(**kw) == -1, kw
        assert b"flowres_fold" in err()

    lib.check(lib.flowres_bytes(1, 128, 136, FLOWENC_FEATURE, ctypes.byref(n)))
    maps = 64 * 68 * 4 * 64 * 4  # the block's input and output and its two convolutions' raw maps, at the stem's positions
    assert maps <= n.value <= maps + 32 * 34 * 4 * 96 + (8 << 20)
    feature_bytes = n.value
    lib.check(lib.flowres_bytes(1, 128, 136, FLOWENC_CONTEXT, ctypes.byref(n)))
    assert maps * 3 // 4 <= n.value <= maps * 3 // 4 + 32 * 34 * 4 * 96 + (12 << 20)  # (no second raw map; the folded weights)
    context_bytes = n.value
    for bad in ((0, 128, 128, 0), (1, 0, 128, 0), (1, 128, 0, 1), (70000, 128, 128, 0), (1, 1 << 14, 1 << 15, 1), (1, 128, 128, 2),
                (1, 128, 128, -1), (1, 8, 8, FLOWENC_FEATURE), (2, 1, 1, FLOWENC_FEATURE), (1, 8, 5, FLOWENC_FEATURE)):
        assert lib.flowres_bytes(*bad, ctypes.byref(n)) == -1, bad
        assert b"flowres_bytes" in err()
    assert b"single position" in err()
    lib.check(lib.flowres_bytes(1, 8, 8, FLOWENC_CONTEXT, ctypes.byref(n)))  # (no instance norm: a single position is a map like any other)
    lib.check(lib.flowres_bytes(1, 9, 8, FLOWENC_FEATURE, ctypes.byref(n)))  # (two positions)
    assert lib.flowres_bytes(1, 128, 128, 0, None) == -1
    for size in (1024, 2048):  # the sizes the documents state, MB of 10^6 bytes per image
        got = []
        for kind in (FLOWENC_FEATURE, FLOWENC_CONTEXT):
            lib.check(lib.flowres_bytes(1, size, size, kind, ctypes.byref(n)))
            got.append(round(n.value / 1e6))
        assert tuple(got) == {1024: (302, 236), 2048: (1189, 916)}[size]

    def table(count, *v):
        return (ctypes.c_void_p * count)(*v)

    full = table(FLOWRES_PARAMS, *([0x1000] * FLOWRES_PARAMS))
    hole = table(FLOWRES_PARAMS, *([0x1000] * 7 + [None] + [0x1000] * (FLOWRES_PARAMS - 8)))
    skew = table(FLOWRES_PARAMS, *([0x1000] * (FLOWRES_PARAMS - 1) + [0x1004]))
    bn = table(FLOWRES_BN, *([0x1000] * FLOWRES_BN))
    bn_hole = table(FLOWRES_BN, *([0x1000] * 59 + [None]))
    bn_skew = table(FLOWRES_BN, *([0x1004] + [0x1000] * 59))

    def run(N=1, H=128, W=136, kind=FLOWENC_FEATURE, params=full, norms=None, image=p, ws=p, size=feature_bytes, out=p):
        return lib.flowres_run(N, H, W, kind, params, norms, image, ws, size, out, None)

    for kw in (dict(N=0), dict(H=0), dict(W=0), dict(N=70000), dict(kind=2), dict(H=8, W=8), dict(params=None), dict(params=hole),
               dict(params=skew), dict(image=None), dict(ws=None), dict(out=None), dict(image=odd), dict(out=odd), dict(norms=bn),
               dict(kind=FLOWENC_CONTEXT), dict(kind=FLOWENC_CONTEXT, norms=bn_hole), dict(kind=FLOWENC_CONTEXT, norms=bn_skew),
               dict(kind=FLOWENC_CONTEXT, norms=bn, params=hole), dict(kind=FLOWENC_CONTEXT, norms=bn, image=None)):
        assert run(**kw) == -1, kw
        assert b"flowres_run" in err()
    assert run(norms=bn) == -1 and b"bn goes with CONTEXT" in err()
    assert run(kind=FLOWENC_CONTEXT) == -1 and b"CONTEXT takes bn" in err()
    assert run(size=feature_bytes - 1) == -3 and b"workspace" in err()
    assert run(kind=FLOWENC_CONTEXT, norms=bn, size=context_bytes - 1) == -3 and b"workspace" in err()


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import raft

    w, v = torch.zeros(8, 4, 3, 3), torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.fold_batchnorm(w, v, v, v, v, v)
    with pytest.raises(TypeError):
        raft.fold_batchnorm(w.double(), v, v, v, v, v)
    with pytest.raises(TypeError):
        raft.fold_batchnorm(w, v, v, v.double(), v, v)
    with pytest.raises(TypeError):
        raft.fold_batchnorm(w, v, [0.0] * 8, v, v, v)
    for kw in (dict(weight=torch.zeros(8, 36)), dict(weight=torch.zeros(0, 4, 3, 3)), dict(bias=torch.zeros(7)), dict(gamma=torch.zeros(8, 1)),
               dict(beta=torch.zeros(9)), dict(mean=torch.zeros(())), dict(var=torch.zeros(4)), dict(eps=-1.0), dict(eps=float("nan")),
               dict(eps=float("inf"))):
        args = dict(weight=w, bias=v, gamma=v, beta=v, mean=v, var=v)
        args.update(kw)
        with pytest.raises(ValueError):
            raft.fold_batchnorm(**args)

    small, large = raft.raft_small(), raft.raft_large()
    feature, context = raft.FusedEncoderLarge(large.feature_encoder), raft.FusedEncoderLarge(large.context_encoder)
    assert (feature.channels, context.channels) == (256, 256) and feature.kind != context.kind
    assert feature._norms is None and len(context._norms) == 15 and len(feature._convs) == len(context._convs) == 16
    assert raft.FusedEncoderLarge.MAX_WORKSPACES == raft.FusedEncoder.MAX_WORKSPACES == 2
    assert [round(feature.workspace_bytes(1, 1024, 1024) / 1e6), round(context.workspace_bytes(1, 1024, 1024) / 1e6)] == [302, 236]
    with pytest.raises(ValueError, match="BottleneckBlock"):
        raft.FusedEncoderLarge(small.feature_encoder)
    with pytest.raises(ValueError, match="BottleneckBlock"):
        raft.FusedEncoderLarge(small.context_encoder)
    with pytest.raises(ValueError, match="ResidualBlock"):  # FusedEncoder itself keeps refusing residual blocks
        raft.FusedEncoder(large.feature_encoder)
    with pytest.raises(TypeError, match="RAFT"):
        raft.FusedEncoderLarge(large)
    widths = (64, 64, 96, 128, 256)
    Res = raft.ResidualBlock
    with pytest.raises(ValueError, match="affine=True"):
        raft.FusedEncoderLarge(raft.FeatureEncoder(Res, widths, functools.partial(torch.nn.InstanceNorm2d, affine=True)))
    with pytest.raises(ValueError, match="track_running_stats=True"):
        raft.FusedEncoderLarge(raft.FeatureEncoder(Res, widths, functools.partial(torch.nn.InstanceNorm2d, track_running_stats=True)))
    with pytest.raises(ValueError, match="GroupNorm"):
        raft.FusedEncoderLarge(raft.FeatureEncoder(Res, widths, functools.partial(torch.nn.GroupNorm, 8)))
    with pytest.raises(ValueError, match="eps=0.001"):
        raft.FusedEncoderLarge(raft.FeatureEncoder(Res, widths, functools.partial(torch.nn.InstanceNorm2d, eps=1e-3)))
    with pytest.raises(ValueError, match="eps=0.001"):
        raft.FusedEncoderLarge(raft.FeatureEncoder(Res, widths, functools.partial(torch.nn.BatchNorm2d, eps=1e-3)))
    with pytest.raises(ValueError, match="affine=False"):
        raft.FusedEncoderLarge(raft.FeatureEncoder(Res, widths, functools.partial(torch.nn.BatchNorm2d, affine=False)))
    with pytest.raises(ValueError, match="track_running_stats=False"):
        raft.FusedEncoderLarge(raft.FeatureEncoder(Res, widths, functools.partial(torch.nn.BatchNorm2d, track_running_stats=False)))
    with pytest.raises(ValueError, match="none"):
        raft.FusedEncoderLarge(raft.FeatureEncoder(Res, widths, None))
    for wrong in ((64, 64, 96, 128, 128), (64, 64, 96, 160, 256), (32, 32, 64, 96, 256), (64, 64, 128, 128, 256)):
        with pytest.raises(ValueError, match="convolutions are"):
            raft.FusedEncoderLarge(raft.FeatureEncoder(Res, wrong, torch.nn.BatchNorm2d))
    mixed = raft.FeatureEncoder(Res, widths, torch.nn.BatchNorm2d)
    mixed.layer2[1].convnormrelu2[1] = torch.nn.InstanceNorm2d(96)
    with pytest.raises(ValueError, match="the same kind throughout"):
        raft.FusedEncoderLarge(mixed)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        feature(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        context(torch.zeros(1, 3, 16, 16))
    with pytest.raises(TypeError):
        feature(torch.zeros(1, 3, 16, 16).double())
    with pytest.raises(ValueError):
        context(torch.zeros(1, 4, 16, 16))
    with pytest.raises(ValueError, match="fused_large"):
        raft.RAFT("small", encoder="fused_large")
    with pytest.raises(ValueError, match="fused_large"):
        raft.raft_small(encoder="fused_large")
    with pytest.raises(ValueError, match="fused"):
        raft.RAFT("large", encoder="fused")
    with pytest.raises(ValueError, match="fused_large"):
        raft.RAFT("large", encoder="nope")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.raft_large(corr="volume", update="torch", encoder="fused_large").eval()(torch.zeros(1, 3, 128, 128), torch.zeros(1, 3, 128, 128),
                                                                                       num_flow_updates=1)
    assert raft.raft_large().encoder == "torch" and raft.raft_large(encoder="fused_large").encoder == "fused_large"
    auto = raft.raft_large(encoder="auto")
    assert auto._fused_enc is None and auto._fused_enc_large is not None and raft.raft_small()._fused_enc_large is None
    assert not auto._fused_encoder(torch.zeros(1, 3, 8, 8))  # "auto" runs the torch modules for RAFT-large


def _forward_by_hand(model, image1, image2, updates):
    """RAFT-large's forward written out with the module's own blocks: the volume path, the mask predictor, convex upsampling."""
    import torch.nn.functional as F

    from eogs2_amd import raft

    N, _, H, W = image1.shape
    h, w = H // 8, W // 8
    fmap1, fmap2 = torch.chunk(model.feature_encoder(torch.cat([image1, image2], dim=0)), 2, dim=0)
    pyramid = raft.volume_pyramid(fmap1, fmap2, model.corr_levels)
    hidden, context = torch.split(model.context_encoder(image1), [128, 128], dim=1)
    hidden, context = torch.tanh(hidden), F.relu(context)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    coords0 = torch.stack([xs, ys], dim=0)[None].repeat(N, 1, 1, 1)
    coords1 = coords0.clone()
    for _ in range(updates):
        corr = raft.volume_lookup(pyramid, coords1, model.corr_radius)
        hidden, delta = model.update_block(hidden, context, corr, coords1 - coords0)
        coords1 = coords1 + delta
    return raft.convex_upsample_torch(coords1 - coords0, model.mask_predictor(hidden))


def test_torch_and_auto_are_today_s_forward_on_the_cpu():
    """encoder="torch" is the path before this option existed, and "auto" is that path for RAFT-large: the same bits as the
    forward written out with the module's own blocks, with the batch norms randomised."""
    from eogs2_amd import raft

    torch.manual_seed(64)
    model = raft.raft_large(corr="volume", update="torch", encoder="torch").eval()
    rc.randomise_batchnorms(model, 65)
    g = torch.Generator().manual_seed(66)
    a, b = torch.rand(1, 3, 128, 136, generator=g) * 2 - 1, torch.rand(1, 3, 128, 136, generator=g) * 2 - 1
    with torch.inference_mode():
        want = _forward_by_hand(model, a, b, 2)
        got = model(a, b, num_flow_updates=2)[-1]
        auto = raft.raft_large(corr="volume", encoder="auto").eval()
        auto.load_state_dict(model.state_dict())
        assert auto.encoder == "auto"
        same = auto(a, b, num_flow_updates=2)[-1]
    assert torch.equal(got, want) and torch.equal(same, want)


def test_nothing_is_registered_and_every_name_is_exported():
    from eogs2_amd import raft

    torch.manual_seed(67)
    a = raft.raft_large(encoder="fused_large")
    torch.manual_seed(67)
    plain = raft.RAFT("large")
    assert sum(p.numel() for p in a.parameters()) == sum(p.numel() for p in plain.parameters()) == 5_257_536
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in plain.named_buffers()] and len(list(a.buffers())) == 45
    torch.manual_seed(68)
    b = raft.raft_large()
    missing, unexpected = b.load_state_dict(a.state_dict(), strict=True)
    assert not missing and not unexpected and list(a.state_dict()) == list(b.state_dict())
    for name in ("fold_batchnorm", "FusedEncoderLarge", "AUTO_ENCODER_LARGE_IS_FUSED"):
        assert name in raft.__all__ and hasattr(raft, name), name
    assert isinstance(raft.AUTO_ENCODER_LARGE_IS_FUSED, bool)
    c = copy.deepcopy(a)  # the copy's fused encoders hold the COPY's convolutions and norms, and no workspace
    assert c._fused_enc_large[0] is not a._fused_enc_large[0] and c._fused_enc_large[0]._convs[0] is c.feature_encoder.convnormrelu[0]
    assert c._fused_enc_large[1]._convs[-1] is c.context_encoder.conv and c._fused_enc_large[1]._norms[0] is c.context_encoder.convnormrelu[1]
    assert c._fused_enc_large[1]._norms[-1] is c.context_encoder.layer3[1].convnormrelu2[1] and len(c._fused_enc_large[0]._ws) == 0
    d = pickle.loads(pickle.dumps(a._fused_enc_large[1]))
    assert d.kind == a._fused_enc_large[1].kind and len(d._ws) == 0 and len(d._convs) == 16 and len(d._norms) == 15
    assert "fused_large" in raft.RAFT.__doc__ and "FusedEncoderLarge" in raft.raft_large.__doc__
