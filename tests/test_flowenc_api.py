"""CPU: the surface of the fused encoders (the eogs_flowenc_* entries of include/eogs_resample.h, eogs2_amd.raft.conv2d_strided_cl /
finish_cl / FusedEncoder / RAFT(encoder=...)) without a device: header and binding table, every stated refusal before a
launch, what the wrappers refuse, and that encoder="torch" and "auto" off the GPU are today's forward bit for bit."""
import copy
import ctypes
import functools
import pickle
import re

import pytest
import torch

import abi_cases as AC


@pytest.fixture(scope="module")
def lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


NAMES = ["eogs_flowenc_bytes", "eogs_flowenc_conv", "eogs_flowenc_conv_partials", "eogs_flowenc_finish", "eogs_flowenc_norm",
         "eogs_flowenc_run"]


def test_header_table_and_constants_agree():
    from eogs2_amd import _abi

    assert _abi.ABI_VERSION == 8  # entry points were added, nothing changed
    decl = {k: v for k, v in AC.declared("eogs_resample.h").items() if k.startswith("eogs_flowenc_")}
    table = {k: v for k, v in _abi.HEADERS["eogs_resample.h"].items() if k.startswith("eogs_flowenc_")}
    assert sorted(decl) == sorted(table) == NAMES
    for name, (res, args) in table.items():
        assert decl[name] == len(args) and res is ctypes.c_int, name
        assert name in _abi.HIP_ONLY
    defines = {k: int(v) for k, v in re.findall(r"#define (EOGS_FLOWENC_[A-Z0-9_]+) (\d+)u?\b", AC.header_text("eogs_resample.h"))}
    assert defines == {"EOGS_FLOWENC_EPI_BIAS": _abi.FLOWENC_EPI_BIAS, "EOGS_FLOWENC_EPI_RELU": _abi.FLOWENC_EPI_RELU,
                       "EOGS_FLOWENC_EPI_RESIDUAL": _abi.FLOWENC_EPI_RESIDUAL, "EOGS_FLOWENC_IN_NCHW": _abi.FLOWENC_IN_NCHW,
                       "EOGS_FLOWENC_OUT_NCHW": _abi.FLOWENC_OUT_NCHW, "EOGS_FLOWENC_SHORTCUT_NONE": _abi.FLOWENC_SHORTCUT_NONE,
                       "EOGS_FLOWENC_SHORTCUT_PLAIN": _abi.FLOWENC_SHORTCUT_PLAIN, "EOGS_FLOWENC_SHORTCUT_NORM": _abi.FLOWENC_SHORTCUT_NORM,
                       "EOGS_FLOWENC_FEATURE": _abi.FLOWENC_FEATURE, "EOGS_FLOWENC_CONTEXT": _abi.FLOWENC_CONTEXT,
                       "EOGS_FLOWENC_PARAMS": _abi.FLOWENC_PARAMS}


def test_library_refuses_before_a_launch(lib):
    """Every refusal comes back as a status with a message before anything touches a device (there is none here): the
    pointers are made up and never read."""
    assert lib.cdll.eogs_rast_abi_version() == 8
    err = lib.cdll.eogs_rast_last_error
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)  # (never dereferenced: every call below is refused)
    n, rows = ctypes.c_size_t(), ctypes.c_int()

    lib.check(lib.flowenc_conv_partials(2, 9, 17, 32, ctypes.byref(rows), ctypes.byref(n)))
    assert rows.value == 2 * 2 and n.value == 2 * rows.value * 32 * 2 * 8  # 16 x 8 tiles, (sum, sum of squares) in double
    for bad in ((0, 9, 17, 32), (2, 0, 17, 32), (2, 9, 0, 32), (2, 9, 17, 0), (2, 9, 17, 5000), (70000, 9, 17, 32), (1, 1 << 14, 1 << 14, 32)):
        assert lib.flowenc_conv_partials(*bad, ctypes.byref(rows), ctypes.byref(n)) == -1, bad
        assert b"flowenc_conv_partials" in err()
    assert lib.flowenc_conv_partials(2, 9, 17, 32, None, ctypes.byref(n)) == -1
    assert lib.flowenc_conv_partials(2, 9, 17, 32, ctypes.byref(rows), None) == -1

    seg = (ctypes.c_int * 1)(16)
    lib.check(lib.flownet_conv_pack_bytes(3, 1, seg, 24, ctypes.byref(n)))
    packed_bytes = n.value
    lib.check(lib.flowenc_conv_partials(1, 5, 6, 24, ctypes.byref(rows), ctypes.byref(n)))
    part_bytes = n.value

    def conv(N=1, h=9, w=11, cin=16, cout=24, k=3, stride=2, inp=p, in_norm=p, packed=p, size=packed_bytes, bias=p, res=None, out=p,
             partials=p, psize=part_bytes, epi=0, flags=0):
        return lib.flowenc_conv(N, h, w, cin, cout, k, stride, inp, in_norm, packed, size, bias, res, out, partials, psize, epi, flags, None)

    for kw in (dict(N=0), dict(h=0), dict(w=0), dict(cin=0), dict(cout=0), dict(cin=5000), dict(cout=5000), dict(N=70000),
               dict(h=1 << 14, w=1 << 14, stride=1), dict(k=0), dict(k=2), dict(k=5), dict(k=9), dict(stride=0), dict(stride=3), dict(epi=-1),
               dict(epi=3), dict(flags=2), dict(flags=16), dict(epi=1, flags=8, partials=None), dict(epi=1), dict(epi=2, res=p),
               dict(epi=2, partials=None), dict(res=p), dict(epi=1, res=p, partials=None), dict(inp=None), dict(packed=None), dict(out=None),
               dict(inp=odd), dict(in_norm=odd), dict(packed=odd), dict(bias=odd), dict(epi=2, res=odd, partials=None), dict(out=odd),
               dict(partials=odd)):
        assert conv(**kw) == -1, kw
        assert b"flowenc_conv" in err()
    assert conv(size=packed_bytes - 1) == -3 and b"too small" in err()
    assert conv(psize=part_bytes - 1) == -3 and b"partials" in err()
    assert conv(cout=100) == -3  # a wider convolution no longer fits the packing it was given

    def norm(N=1, h=5, w=6, C=24, partials=p, psize=part_bytes, out=p):
        return lib.flowenc_norm(N, h, w, C, partials, psize, out, None)

    for kw in (dict(N=0), dict(h=0), dict(w=0), dict(C=0), dict(C=5000), dict(N=70000), dict(h=1 << 14, w=1 << 14), dict(partials=None),
               dict(out=None), dict(partials=odd), dict(out=odd)):
        assert norm(**kw) == -1, kw
        assert b"flowenc_norm" in err()
    assert norm(psize=part_bytes - 1) == -3 and b"partials" in err()
    assert norm(w=17) == -3  # a second tile column asks for a second row of partials

    def finish(N=1, h=5, w=6, C=24, v=p, norm_v=p, s=p, norm_s=p, shortcut=2, out=p):
        return lib.flowenc_finish(N, h, w, C, v, norm_v, s, norm_s, shortcut, out, None)

    for kw in (dict(N=0), dict(h=0), dict(w=0), dict(C=0), dict(C=22), dict(N=70000), dict(h=1 << 14, w=1 << 14), dict(shortcut=-1),
               dict(shortcut=3), dict(shortcut=0), dict(shortcut=0, norm_s=None), dict(shortcut=0, s=None), dict(shortcut=1),
               dict(shortcut=1, s=None, norm_s=None), dict(shortcut=2, norm_s=None), dict(shortcut=2, s=None), dict(v=None),
               dict(norm_v=None), dict(out=None), dict(v=odd), dict(norm_v=odd), dict(s=odd), dict(norm_s=odd), dict(out=odd)):
        assert finish(**kw) == -1, kw
        assert b"flowenc_finish" in err()

    from eogs2_amd._abi import FLOWENC_CONTEXT, FLOWENC_FEATURE, FLOWENC_PARAMS

    lib.check(lib.flowenc_bytes(1, 128, 136, FLOWENC_FEATURE, ctypes.byref(n)))
    maps = 64 * 68 * 4 * (32 + 32 + 32 + 16 + 8)  # the block's two maps, the three units' outputs, at the stem's positions
    assert maps <= n.value <= maps + 64 * 68 * 4 * 16 + (4 << 20)
    ws_bytes = n.value
    for bad in ((0, 128, 128, 0), (1, 0, 128, 0), (1, 128, 0, 1), (70000, 128, 128, 0), (1, 1 << 14, 1 << 15, 1), (1, 128, 128, 2),
                (1, 128, 128, -1), (1, 8, 8, FLOWENC_FEATURE), (2, 1, 1, FLOWENC_FEATURE), (1, 8, 5, FLOWENC_FEATURE)):
        assert lib.flowenc_bytes(*bad, ctypes.byref(n)) == -1, bad
        assert b"flowenc_bytes" in err()
    assert b"single position" in err()
    lib.check(lib.flowenc_bytes(1, 8, 8, FLOWENC_CONTEXT, ctypes.byref(n)))  # (no norm: a single position is a map like any other)
    lib.check(lib.flowenc_bytes(1, 9, 8, FLOWENC_FEATURE, ctypes.byref(n)))  # (two positions)
    assert lib.flowenc_bytes(1, 128, 128, 0, None) == -1

    table = lambda *v: (ctypes.c_void_p * FLOWENC_PARAMS)(*v)  # noqa: E731
    full = table(*([0x1000] * FLOWENC_PARAMS))
    hole = table(*([0x1000] * 7 + [None] + [0x1000] * (FLOWENC_PARAMS - 8)))
    skew = table(*([0x1000] * (FLOWENC_PARAMS - 1) + [0x1004]))

    def run(N=1, H=128, W=136, kind=FLOWENC_FEATURE, params=full, image=p, ws=p, size=ws_bytes, out=p):
        return lib.flowenc_run(N, H, W, kind, params, image, ws, size, out, None)

    for kw in (dict(N=0), dict(H=0), dict(W=0), dict(N=70000), dict(kind=2), dict(H=8, W=8), dict(params=None), dict(params=hole),
               dict(params=skew), dict(image=None), dict(ws=None), dict(out=None), dict(image=odd), dict(out=odd)):
        assert run(**kw) == -1, kw
        assert b"flowenc_run" in err()
    assert run(size=ws_bytes - 1) == -3 and b"workspace" in err()


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import raft

    x, wt, b = torch.zeros(1, 5, 7, 4), torch.zeros(8, 4, 3, 3), torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.conv2d_strided_cl(x, wt, b, stride=2)
    with pytest.raises(TypeError):
        raft.conv2d_strided_cl([x], wt, b)
    with pytest.raises(TypeError):
        raft.conv2d_strided_cl(x.double(), wt, b)
    with pytest.raises(TypeError):
        raft.conv2d_strided_cl(x, wt.half(), b)
    for kw in (dict(input=x[0]), dict(weight=torch.zeros(8, 5, 3, 3)), dict(weight=torch.zeros(8, 4, 5, 5)), dict(weight=torch.zeros(8, 4, 3, 1)),
               dict(stride=3), dict(stride=0), dict(bias=torch.zeros(7)), dict(act="gelu"), dict(in_norm=torch.zeros(1, 4)),
               dict(in_norm=torch.zeros(1, 8, 2)), dict(res=torch.zeros(1, 5, 7, 8), stride=2, act="relu"), dict(res=torch.zeros(1, 5, 7, 8)),
               dict(stats=True, act="relu"), dict(out_nchw=True, act="relu"), dict(in_nchw=True)):
        args = dict(input=x, weight=wt, bias=b)
        args.update(kw)
        with pytest.raises(ValueError):
            raft.conv2d_strided_cl(**args)
    v, t = torch.zeros(1, 5, 7, 8), torch.zeros(1, 8, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.finish_cl(v, t)
    with pytest.raises(TypeError):
        raft.finish_cl(v.double(), t)
    for kw in (dict(v=torch.zeros(1, 5, 7, 6), norm_v=torch.zeros(1, 6, 2)), dict(norm_v=torch.zeros(1, 8)), dict(norm_s=t),
               dict(s=torch.zeros(1, 5, 8, 8)), dict(s=v, norm_s=torch.zeros(2, 8, 2))):
        args = dict(v=v, norm_v=t)
        args.update(kw)
        with pytest.raises(ValueError):
            raft.finish_cl(**args)

    small, large = raft.raft_small(), raft.raft_large()
    feature, context = raft.FusedEncoder(small.feature_encoder), raft.FusedEncoder(small.context_encoder)
    assert (feature.channels, context.channels) == (128, 160) and feature.kind != context.kind
    with pytest.raises(ValueError, match="ResidualBlock"):
        raft.FusedEncoder(large.feature_encoder)
    with pytest.raises(ValueError, match="ResidualBlock"):
        raft.FusedEncoder(large.context_encoder)
    with pytest.raises(TypeError, match="RAFT"):
        raft.FusedEncoder(small)
    widths = (32, 32, 64, 96, 128)
    with pytest.raises(ValueError, match="affine=True"):
        raft.FusedEncoder(raft.FeatureEncoder(raft.BottleneckBlock, widths, functools.partial(torch.nn.InstanceNorm2d, affine=True)))
    with pytest.raises(ValueError, match="BatchNorm2d"):
        raft.FusedEncoder(raft.FeatureEncoder(raft.BottleneckBlock, widths, torch.nn.BatchNorm2d))
    with pytest.raises(ValueError, match="eps=0.001"):
        raft.FusedEncoder(raft.FeatureEncoder(raft.BottleneckBlock, widths, functools.partial(torch.nn.InstanceNorm2d, eps=1e-3)))
    with pytest.raises(ValueError, match="160"):
        raft.FusedEncoder(raft.FeatureEncoder(raft.BottleneckBlock, (32, 32, 64, 96, 160), torch.nn.InstanceNorm2d))
    with pytest.raises(ValueError, match="convolutions are"):
        raft.FusedEncoder(raft.FeatureEncoder(raft.BottleneckBlock, (32, 32, 64, 128, 160), None))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        feature(torch.zeros(1, 3, 16, 16))
    with pytest.raises(TypeError):
        feature(torch.zeros(1, 3, 16, 16).double())
    with pytest.raises(ValueError):
        feature(torch.zeros(1, 4, 16, 16))
    with pytest.raises(ValueError, match="fused"):
        raft.RAFT("large", encoder="fused")
    with pytest.raises(ValueError, match="fused"):
        raft.raft_large(encoder="fused")
    with pytest.raises(ValueError, match="encoder"):
        raft.RAFT("small", encoder="nope")
    with pytest.raises(ValueError):
        raft.raft_small(encoder="nope")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.raft_small(corr="volume", update="torch", encoder="fused").eval()(torch.zeros(1, 3, 128, 128), torch.zeros(1, 3, 128, 128),
                                                                                 num_flow_updates=1)
    assert raft.raft_small().encoder == "torch" and raft.raft_large().encoder == "torch" and raft.RAFT().encoder == "torch"
    assert raft.raft_large(encoder="auto")._fused_enc is None


def test_torch_and_auto_are_today_s_forward_on_the_cpu():
    """encoder="torch" is the path before this option existed, and "auto" off the GPU is that path: the same bits as the
    forward written out with the module's own blocks."""
    from test_flownet_api import _forward_by_hand

    from eogs2_amd import raft

    torch.manual_seed(60)
    model = raft.raft_small(corr="volume", update="torch", encoder="torch").eval()
    g = torch.Generator().manual_seed(61)
    a, b = torch.rand(1, 3, 128, 136, generator=g) * 2 - 1, torch.rand(1, 3, 128, 136, generator=g) * 2 - 1
    with torch.inference_mode():
        want = _forward_by_hand(model, a, b, 2)
        got = model(a, b, num_flow_updates=2)[-1]
        auto = raft.raft_small(corr="volume", encoder="auto").eval()
        auto.load_state_dict(model.state_dict())
        assert auto.encoder == "auto"
        same = auto(a, b, num_flow_updates=2)[-1]
    assert torch.equal(got, want) and torch.equal(same, want)


def test_nothing_is_registered_and_every_name_is_exported():
    from eogs2_amd import raft

    torch.manual_seed(62)
    a = raft.raft_small(encoder="fused")
    assert sum(p.numel() for p in a.parameters()) == 990_162 and not list(a.buffers())
    torch.manual_seed(63)
    b = raft.raft_small()
    missing, unexpected = b.load_state_dict(a.state_dict(), strict=True)
    assert not missing and not unexpected and list(a.state_dict()) == list(b.state_dict())
    for name in ("conv2d_strided_cl", "finish_cl", "FusedEncoder", "AUTO_ENCODER_IS_FUSED"):
        assert name in raft.__all__ and hasattr(raft, name), name
    assert isinstance(raft.AUTO_ENCODER_IS_FUSED, bool)
    c = copy.deepcopy(a)  # the copy's fused encoders hold the COPY's convolutions, and no workspace
    assert c._fused_enc[0] is not a._fused_enc[0] and c._fused_enc[0]._convs[0] is c.feature_encoder.convnormrelu[0]
    assert c._fused_enc[1]._convs[-1] is c.context_encoder.conv and len(c._fused_enc[0]._ws) == 0
    d = pickle.loads(pickle.dumps(a._fused_enc[1]))
    assert d.kind == a._fused_enc[1].kind and len(d._ws) == 0 and len(d._convs) == 22
    assert "The encoders (convolutions, norms) are torch modules, and so is" not in raft.__doc__
