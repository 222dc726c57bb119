"""CPU: the surface of the fused update block (the eogs_flownet_* entries of include/eogs_resample.h, eogs2_amd.raft.conv2d_cl /
FusedUpdate / RAFT(update=...)) without a device: header and binding table, every stated refusal before a launch, what the
wrappers refuse, and that update="torch" and "auto" off the GPU are today's forward bit for bit."""
import ctypes
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


NAMES = ["eogs_flownet_conv", "eogs_flownet_conv_info", "eogs_flownet_conv_pack", "eogs_flownet_conv_pack_bytes",
         "eogs_flownet_update_begin", "eogs_flownet_update_bytes", "eogs_flownet_update_hidden_offset", "eogs_flownet_update_step"]


def test_header_table_and_constants_agree():
    from eogs2_amd import _abi

    assert _abi.ABI_VERSION == 8  # entry points were added, nothing changed
    decl = {k: v for k, v in AC.declared("eogs_resample.h").items() if k.startswith("eogs_flownet_")}
    table = {k: v for k, v in _abi.HEADERS["eogs_resample.h"].items() if k.startswith("eogs_flownet_")}
    assert sorted(decl) == sorted(table) == NAMES
    for name, (res, args) in table.items():
        assert decl[name] == len(args) and res is ctypes.c_int, name
        assert name in _abi.HIP_ONLY
    defines = {k: int(v) for k, v in re.findall(r"#define (EOGS_FLOWNET_[A-Z0-9_]+) (\d+)u?\b", AC.header_text("eogs_resample.h"))}
    assert defines == {"EOGS_FLOWNET_MAX_SEGMENTS": _abi.FLOWNET_MAX_SEGMENTS, "EOGS_FLOWNET_MAX_KERNEL": _abi.FLOWNET_MAX_KERNEL,
                       "EOGS_FLOWNET_EPI_BIAS": _abi.FLOWNET_EPI_BIAS, "EOGS_FLOWNET_EPI_RELU": _abi.FLOWNET_EPI_RELU,
                       "EOGS_FLOWNET_EPI_GATES": _abi.FLOWNET_EPI_GATES, "EOGS_FLOWNET_EPI_GRU": _abi.FLOWNET_EPI_GRU,
                       "EOGS_FLOWNET_IN0_NCHW": _abi.FLOWNET_IN0_NCHW, "EOGS_FLOWNET_OUT_NCHW": _abi.FLOWNET_OUT_NCHW,
                       "EOGS_FLOWNET_UPDATE_PARAMS": _abi.FLOWNET_UPDATE_PARAMS}


def test_library_refuses_before_a_launch(lib):
    """Every refusal comes back as a status with a message before anything touches a device (there is none here): the
    pointers are made up and never read."""
    assert lib.cdll.eogs_rast_abi_version() == 8
    err = lib.cdll.eogs_rast_last_error
    tw, th = ctypes.c_int(), ctypes.c_int()
    lib.check(lib.flownet_conv_info(ctypes.byref(tw), ctypes.byref(th)))
    assert tw.value == 16 and tw.value * th.value % 64 == 0  # a matrix instruction's 16 rows are 16 positions of one image row
    assert lib.flownet_conv_info(None, ctypes.byref(th)) == -1
    seg = lambda *c: (ctypes.c_int * len(c))(*c)  # noqa: E731
    n = ctypes.c_size_t()
    lib.check(lib.flownet_conv_pack_bytes(3, 2, seg(96, 82), 192, ctypes.byref(n)))
    assert 178 * 9 * 192 * 4 <= n.value <= 2 * 178 * 9 * 192 * 4  # the weights, padded to whole chunks and blocks
    packed_bytes = n.value
    for bad in ((0, 1, seg(4), 8), (2, 1, seg(4), 8), (4, 1, seg(4), 8), (9, 1, seg(4), 8), (3, 0, seg(4), 8), (3, 4, seg(4, 4, 4, 4), 8),
                (3, 1, seg(0), 8), (3, 2, seg(4, -1), 8), (3, 1, seg(4), 0), (3, 1, None, 8)):
        assert lib.flownet_conv_pack_bytes(*bad, ctypes.byref(n)) == -1, bad[:2]
        assert b"flownet_conv_pack_bytes" in err()
    assert lib.flownet_conv_pack_bytes(3, 1, seg(4), 8, None) == -1
    p = ctypes.c_void_p(0x1000)  # (never dereferenced: every call below is refused)
    odd = ctypes.c_void_p(0x1004)

    def pack(k=3, nseg=2, chans=seg(96, 82), offsets=None, cin=178, cout=192, cout_off=0, cout_n=192, weight=p, packed=p, size=packed_bytes):
        return lib.flownet_conv_pack(k, nseg, chans, offsets, cin, cout, cout_off, cout_n, weight, packed, size, None)

    for kw in (dict(k=2), dict(k=0), dict(nseg=0), dict(cin=177), dict(cin=242), dict(offsets=seg(0, 161), cin=242), dict(offsets=seg(-1, 96), cin=242),
               dict(cout=0), dict(cout_off=-1), dict(cout_n=0), dict(cout_off=96, cout_n=97), dict(weight=None), dict(packed=None),
               dict(weight=odd), dict(packed=odd)):
        assert pack(**kw) == -1, kw
        assert b"flownet_conv_pack" in err()
    assert pack(size=packed_bytes - 1) == -3 and b"too small" in err()

    def conv(N=1, h=5, w=7, k=3, nseg=2, chans=seg(96, 82), in0=p, in1=p, in2=None, cout=192, packed=p, size=packed_bytes, bias=p,
             add=p, aux=None, out=p, epi=0, flags=0):
        return lib.flownet_conv(N, h, w, k, nseg, chans, in0, in1, in2, cout, packed, size, bias, add, aux, out, epi, flags, None)

    for kw in (dict(N=0), dict(h=0), dict(w=0), dict(N=70000), dict(h=1 << 14, w=1 << 14), dict(k=2), dict(k=9), dict(nseg=0), dict(nseg=4),
               dict(chans=seg(96, 0)), dict(cout=0), dict(epi=-1), dict(epi=4), dict(flags=4), dict(flags=16), dict(epi=2, aux=p, flags=8),
               dict(epi=2, aux=p, cout=191), dict(epi=2), dict(epi=3), dict(aux=p), dict(in0=None), dict(in1=None), dict(in2=p),
               dict(packed=None), dict(out=None), dict(in0=odd), dict(in1=odd), dict(packed=odd), dict(bias=odd), dict(add=odd),
               dict(out=odd), dict(epi=3, aux=odd, cout=96)):
        assert conv(**kw) == -1, kw
        assert b"flownet_conv" in err()
    assert conv(size=packed_bytes - 1) == -3 and b"too small" in err()
    assert conv(chans=seg(96, 90)) == -3  # a wrong channel sum no longer fits the packing it was given
    assert conv(chans=seg(96, 82), cout=208) == -3

    lib.check(lib.flownet_update_bytes(1, 128, 128, ctypes.byref(n)))
    per_position = 4 * (288 + 96 + 96 + 64 + 32 + 80 + 192 + 128)  # the planes, the hidden state and the intermediates
    assert 128 * 128 * per_position <= n.value <= 128 * 128 * per_position + (8 << 20)
    ws_bytes = n.value
    off = ctypes.c_size_t()
    lib.check(lib.flownet_update_hidden_offset(1, 128, 128, ctypes.byref(off)))
    assert off.value % 256 == 0 and off.value + 128 * 128 * 96 * 4 <= ws_bytes
    for bad in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (70000, 16, 16), (1, 1 << 13, 1 << 13)):
        assert lib.flownet_update_bytes(*bad, ctypes.byref(n)) == -1, bad
        assert b"flownet_update_bytes" in err()
        assert lib.flownet_update_hidden_offset(*bad, ctypes.byref(off)) == -1, bad
    assert lib.flownet_update_bytes(1, 16, 16, None) == -1
    from eogs2_amd._abi import FLOWNET_UPDATE_PARAMS

    table = lambda *v: (ctypes.c_void_p * FLOWNET_UPDATE_PARAMS)(*v)  # noqa: E731
    full = table(*([0x1000] * FLOWNET_UPDATE_PARAMS))
    hole = table(*([0x1000] * 7 + [None] + [0x1000] * 10))
    skew = table(*([0x1000] * 17 + [0x1004]))

    def begin(N=1, h=128, w=128, params=full, hidden=p, context=p, ws=p, size=ws_bytes):
        return lib.flownet_update_begin(N, h, w, params, hidden, context, ws, size, None)

    for kw in (dict(N=0), dict(h=0), dict(w=0), dict(params=None), dict(params=hole), dict(params=skew), dict(hidden=None),
               dict(context=None), dict(ws=None), dict(hidden=odd), dict(context=odd)):
        assert begin(**kw) == -1, kw
        assert b"flownet_update_begin" in err()
    assert begin(size=ws_bytes - 1) == -3 and b"workspace" in err()

    def step(N=1, h=128, w=128, corr=p, flow=p, ws=p, size=ws_bytes, delta=p):
        return lib.flownet_update_step(N, h, w, corr, flow, ws, size, delta, None)

    for kw in (dict(N=0), dict(h=0), dict(w=0), dict(corr=None), dict(flow=None), dict(ws=None), dict(delta=None), dict(corr=odd),
               dict(flow=odd), dict(delta=odd)):
        assert step(**kw) == -1, kw
        assert b"flownet_update_step" in err()
    assert step(size=ws_bytes - 1) == -3 and b"workspace" in err()


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import raft

    x, wt, b = torch.zeros(1, 5, 7, 4), torch.zeros(8, 4, 3, 3), torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.conv2d_cl([x], wt, b)
    with pytest.raises(TypeError):
        raft.conv2d_cl(x, wt, b)
    with pytest.raises(TypeError):
        raft.conv2d_cl([x.double()], wt, b)
    with pytest.raises(TypeError):
        raft.conv2d_cl([x], wt.half(), b)
    with pytest.raises(TypeError):
        raft.conv2d_cl([x], wt, [0.0] * 8)
    for kw in (dict(inputs=[]), dict(inputs=[x] * 4), dict(inputs=[x, torch.zeros(1, 5, 8, 4)]), dict(inputs=[x[0]]),
               dict(weight=torch.zeros(8, 5, 3, 3)), dict(weight=torch.zeros(8, 4, 2, 2)), dict(weight=torch.zeros(8, 4, 9, 9)),
               dict(weight=torch.zeros(8, 4, 3, 1)), dict(bias=torch.zeros(7)), dict(act="gelu"), dict(add=torch.zeros(1, 5, 7, 4))):
        args = dict(inputs=[x], weight=wt, bias=b)
        args.update(kw)
        with pytest.raises(ValueError):
            raft.conv2d_cl(**args)
    small = raft.raft_small()
    fused = raft.FusedUpdate(small.update_block)
    with pytest.raises(RuntimeError, match="begin"):
        fused.step(torch.zeros(1, 196, 16, 16), torch.zeros(1, 2, 16, 16))
    with pytest.raises(RuntimeError, match="begin"):
        fused.hidden()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.begin(torch.zeros(1, 96, 16, 16), torch.zeros(1, 64, 16, 16))
    with pytest.raises(ValueError):
        fused.begin(torch.zeros(1, 64, 16, 16), torch.zeros(1, 64, 16, 16))
    with pytest.raises(ValueError):
        fused.begin(torch.zeros(1, 96, 16, 16), torch.zeros(1, 64, 16, 17))
    with pytest.raises(TypeError):
        fused.begin(torch.zeros(1, 96, 16, 16).double(), torch.zeros(1, 64, 16, 16))
    with pytest.raises(ValueError, match="RAFT-small"):
        raft.FusedUpdate(raft.raft_large().update_block)
    with pytest.raises(TypeError):
        raft.FusedUpdate(small)
    with pytest.raises(ValueError, match="fused"):
        raft.RAFT("large", update="fused")
    with pytest.raises(ValueError, match="update"):
        raft.RAFT("small", update="nope")
    with pytest.raises(ValueError):
        raft.raft_small(update="nope")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.raft_small(corr="volume", update="fused").eval()(torch.zeros(1, 3, 128, 128), torch.zeros(1, 3, 128, 128), num_flow_updates=1)
    assert isinstance(raft.conv_info(), tuple) and len(raft.conv_info()) == 2


def test_torch_and_auto_are_today_s_forward_on_the_cpu():
    """update="torch" is the path before this option existed, and "auto" off the GPU is that path: the same bits as the
    forward written out with the module's own blocks."""
    from eogs2_amd import raft

    torch.manual_seed(60)
    model = raft.raft_small(corr="volume", update="torch").eval()
    g = torch.Generator().manual_seed(61)
    a, b = torch.rand(1, 3, 128, 136, generator=g) * 2 - 1, torch.rand(1, 3, 128, 136, generator=g) * 2 - 1
    with torch.inference_mode():
        want = _forward_by_hand(model, a, b, 2)
        got = model(a, b, num_flow_updates=2)[-1]
        auto = raft.raft_small(corr="volume").eval()
        auto.load_state_dict(model.state_dict())
        assert auto.update == "auto"
        same = auto(a, b, num_flow_updates=2)[-1]
    assert torch.equal(got, want) and torch.equal(same, want)


def _forward_by_hand(model, image1, image2, updates):
    import torch.nn.functional as F

    from eogs2_amd import raft

    N, _, H, W = image1.shape
    h, w = H // 8, W // 8
    fmap1, fmap2 = torch.chunk(model.feature_encoder(torch.cat([image1, image2], dim=0)), 2, dim=0)
    pyramid = raft.volume_pyramid(fmap1, fmap2, model.corr_levels)
    hidden, context = torch.split(model.context_encoder(image1), [96, 64], dim=1)
    hidden, context = torch.tanh(hidden), F.relu(context)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    coords0 = torch.stack([xs, ys], dim=0)[None].repeat(N, 1, 1, 1)
    coords1 = coords0.clone()
    for _ in range(updates):
        corr = raft.volume_lookup(pyramid, coords1, model.corr_radius)
        hidden, delta = model.update_block(hidden, context, corr, coords1 - coords0)
        coords1 = coords1 + delta
    flow = coords1 - coords0
    return 8 * F.interpolate(flow, size=(H, W), mode="bilinear", align_corners=True)


def test_nothing_is_registered_and_every_name_is_exported():
    from eogs2_amd import raft

    torch.manual_seed(62)
    a = raft.raft_small(update="fused")
    assert sum(p.numel() for p in a.parameters()) == 990_162
    assert sum(p.numel() for p in raft.raft_small().parameters()) == 990_162
    assert not list(a.buffers())
    torch.manual_seed(63)
    b = raft.raft_small(update="torch")
    missing, unexpected = b.load_state_dict(a.state_dict(), strict=True)
    assert not missing and not unexpected
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert b.load_weights(a.torchvision_state_dict()) is b
    for name in ("conv2d_cl", "conv_info", "FusedUpdate", "AUTO_UPDATE_IS_FUSED", "RAFT", "raft_small", "raft_large"):
        assert name in raft.__all__ and hasattr(raft, name), name
    assert raft.raft_large().update == "auto" and raft.raft_large()._fused is None
    import copy

    c = copy.deepcopy(a)  # the copy's fused update holds the COPY's convolutions, and no workspace
    assert c._fused is not a._fused and c._fused._convs[0] is c.update_block.motion_encoder.convcorr1[0]
    assert c._fused._convs[0] is not a._fused._convs[0] and len(c._fused._ws) == 0
    assert "The convolutions, norms and GRUs are torch modules" not in raft.__doc__
