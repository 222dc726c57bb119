"""CPU: the surface of RAFT-large's fused update block (the entries of include/eogs_resample.h, eogs2_amd.raft.conv2d_rect_cl /
FusedUpdateLarge / RAFT(update="fused_large")) without a device: header and binding table, every stated refusal before a
launch, what the wrappers refuse, what was refused before and still is, and that nothing is registered."""
import copy
import ctypes
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


NAMES = ["eogs_flowlarge_begin", "eogs_flowlarge_bytes", "eogs_flowlarge_hidden_offset", "eogs_flowlarge_mask", "eogs_flowlarge_step",
         "eogs_flowrect_conv", "eogs_flowrect_pack", "eogs_flowrect_pack_bytes"]


def test_header_table_and_constants_agree():
    from eogs2_amd import _abi

    assert _abi.ABI_VERSION == 8  # entry points were added, nothing changed
    mine = lambda k: k.startswith(("eogs_flowrect_", "eogs_flowlarge_"))  # noqa: E731
    decl = {k: v for k, v in AC.declared("eogs_resample.h").items() if mine(k)}
    table = {k: v for k, v in _abi.HEADERS["eogs_resample.h"].items() if mine(k)}
    assert sorted(decl) == sorted(table) == NAMES
    assert not set(decl) & AC.elsewhere("eogs_resample.h")
    for name, (res, args) in table.items():
        assert decl[name] == len(args) and res is ctypes.c_int, name
        assert name in _abi.HIP_ONLY
    # the rectangular entries are the square ones with (kh, kw) in place of k: one more int, the rest the same
    sq = _abi.HEADERS["eogs_resample.h"]
    assert table["eogs_flowrect_pack_bytes"][1] == [ctypes.c_int] + sq["eogs_flownet_conv_pack_bytes"][1]
    assert table["eogs_flowrect_pack"][1] == [ctypes.c_int] + sq["eogs_flownet_conv_pack"][1]
    assert table["eogs_flowrect_conv"][1] == sq["eogs_flownet_conv"][1][:3] + [ctypes.c_int] + sq["eogs_flownet_conv"][1][3:]
    for name in ("bytes", "hidden_offset", "begin", "step"):
        assert table[f"eogs_flowlarge_{name}"] == sq[f"eogs_flownet_update_{name}"]
    defines = {k: int(v) for k, v in re.findall(r"#define (EOGS_FLOW(?:RECT|LARGE)_[A-Z0-9_]+) (\d+)u?\b", AC.header_text("eogs_resample.h"))}
    assert defines == {"EOGS_FLOWRECT_EPI_QUARTER": _abi.FLOWRECT_EPI_QUARTER, "EOGS_FLOWLARGE_PARAMS": _abi.FLOWLARGE_PARAMS}
    assert _abi.FLOWRECT_EPI_QUARTER == _abi.FLOWNET_EPI_GRU + 1 and _abi.FLOWLARGE_PARAMS == 30
    assert set(_abi.FLOWRECT_TAP_SHAPES) == {(1, 1), (3, 3), (5, 5), (7, 7), (1, 5), (5, 1)}


def test_library_refuses_before_a_launch(lib):
    """Every refusal of the new entries comes back as a status with a message before anything touches a device (there is none
    here): the pointers are made up and never read."""
    from eogs2_amd import _abi

    assert lib.cdll.eogs_rast_abi_version() == 8
    err = lib.cdll.eogs_rast_last_error
    seg = lambda *c: (ctypes.c_int * len(c))(*c)  # noqa: E731
    n, m = ctypes.c_size_t(), ctypes.c_size_t()
    segs, cin = seg(128, 126, 2), 256
    lib.check(lib.flowrect_pack_bytes(1, 5, 3, segs, 256, ctypes.byref(n)))
    assert cin * 5 * 256 * 4 <= n.value <= 2 * cin * 5 * 256 * 4  # the weights, padded to whole chunks and blocks
    lib.check(lib.flowrect_pack_bytes(5, 1, 3, segs, 256, ctypes.byref(m)))
    assert m.value == n.value
    packed_bytes = n.value
    for k in (1, 3, 5, 7):  # a square pair has the square entry's size
        lib.check(lib.flowrect_pack_bytes(k, k, 3, segs, 256, ctypes.byref(n)))
        lib.check(lib.flownet_conv_pack_bytes(k, 3, segs, 256, ctypes.byref(m)))
        assert n.value == m.value
    # tap pairs outside the six
    pairs = [(kh, kw) for kh in range(-1, 10) for kw in range(-1, 10) if (kh, kw) not in _abi.FLOWRECT_TAP_SHAPES]
    assert (3, 1) in pairs and (1, 3) in pairs and (1, 7) in pairs and (7, 1) in pairs and (5, 3) in pairs and (0, 0) in pairs and (9, 9) in pairs
    for kh, kw in pairs:
        assert lib.flowrect_pack_bytes(kh, kw, 1, seg(4), 8, ctypes.byref(n)) == -1, (kh, kw)
        assert b"flowrect_pack_bytes" in err() and b"1 x 5" in err()
    for bad in ((1, 5, 0, seg(4), 8), (1, 5, 4, seg(4, 4, 4, 4), 8), (1, 5, 1, seg(0), 8), (5, 1, 2, seg(4, -1), 8), (5, 1, 1, seg(4097), 8),
                (5, 1, 1, seg(4), 0), (5, 1, 1, seg(4), 4097), (1, 5, 1, None, 8)):
        assert lib.flowrect_pack_bytes(*bad, ctypes.byref(n)) == -1, bad[:3]
        assert b"flowrect_pack_bytes" in err()
    assert lib.flowrect_pack_bytes(1, 5, 1, seg(4), 8, None) == -1
    p = ctypes.c_void_p(0x1000)  # (never dereferenced: every call below is refused)
    odd = ctypes.c_void_p(0x1004)

    def pack(kh=1, kw=5, nseg=3, chans=segs, offsets=None, cin=cin, cout=256, cout_off=0, cout_n=256, weight=p, packed=p, size=packed_bytes):
        return lib.flowrect_pack(kh, kw, nseg, chans, offsets, cin, cout, cout_off, cout_n, weight, packed, size, None)

    for kw_ in (dict(kh=3, kw=1), dict(kh=1, kw=3), dict(kh=2, kw=2), dict(kh=0), dict(kw=0), dict(nseg=0),
                dict(cin=255), dict(cin=384), dict(offsets=seg(0, 256, 383), cin=384), dict(offsets=seg(-1, 256, 382), cin=384), dict(cout=0),
                dict(cout_off=-1), dict(cout_n=0), dict(cout_off=128, cout_n=129), dict(weight=None), dict(packed=None), dict(weight=odd),
                dict(packed=odd)):
        assert pack(**kw_) == -1, kw_
        assert b"flowrect_pack" in err()
    assert pack(size=packed_bytes - 1) == -3 and b"too small" in err()
    assert pack(kh=5, kw=5) == -3  # a 5 x 5 packing of these channels does not fit a 1 x 5 one

    def conv(N=1, h=5, w=7, kh=1, kw=5, nseg=3, chans=segs, in0=p, in1=p, in2=p, cout=256, packed=p, size=packed_bytes, bias=p, add=p,
             aux=None, out=p, epi=0, flags=0):
        return lib.flowrect_conv(N, h, w, kh, kw, nseg, chans, in0, in1, in2, cout, packed, size, bias, add, aux, out, epi, flags, None)

    Q = _abi.FLOWRECT_EPI_QUARTER
    for kw_ in (dict(N=0), dict(h=0), dict(w=0), dict(N=70000), dict(h=1 << 14, w=1 << 14), dict(kh=3, kw=1), dict(kh=1, kw=3), dict(kh=1, kw=7),
                dict(kh=2, kw=2), dict(kh=9, kw=9), dict(kh=0, kw=5), dict(nseg=0), dict(nseg=4), dict(chans=seg(128, 0, 2)), dict(cout=0),
                dict(epi=-1), dict(epi=Q + 1), dict(flags=16), dict(flags=32), dict(nseg=2, chans=seg(128, 128), in2=None, flags=4),
                dict(epi=2, aux=p, flags=8), dict(epi=3, aux=p, flags=8), dict(epi=2, aux=p, cout=255), dict(epi=2), dict(epi=3), dict(aux=p),
                dict(epi=1, aux=p), dict(epi=Q, aux=p), dict(in0=None), dict(in1=None), dict(in2=None),
                dict(nseg=2, chans=seg(128, 128)), dict(packed=None), dict(out=None), dict(in0=odd), dict(in1=odd), dict(in2=odd),
                dict(packed=odd), dict(bias=odd), dict(add=odd), dict(out=odd), dict(epi=3, aux=odd, cout=128)):
        assert conv(**kw_) == -1, kw_
        assert b"flowrect_conv" in err()
    assert conv(size=packed_bytes - 1) == -3 and b"too small" in err()
    assert conv(kh=5, kw=5) == -3
    assert conv(chans=seg(128, 134, 2)) == -3  # a wrong channel sum no longer fits the packing it was given
    assert conv(cout=320) == -3
    # the square entry still refuses what only the rectangular one takes
    assert lib.flownet_conv(1, 5, 7, 3, 3, segs, p, p, p, 256, p, 1 << 30, p, p, None, p, Q, 0, None) == -1 and b"epilogue" in err()

    lib.check(lib.flowlarge_bytes(1, 128, 128, ctypes.byref(n)))
    # the four planes, the hidden state, the shared 256-wide map, and the intermediates
    per_position = 4 * (768 + 128 + 256 + 192 + 128 + 64 + 126 + 256)
    assert 128 * 128 * per_position <= n.value <= 128 * 128 * per_position + (32 << 20)
    ws_bytes = n.value
    off = ctypes.c_size_t()
    lib.check(lib.flowlarge_hidden_offset(1, 128, 128, ctypes.byref(off)))
    assert off.value % 256 == 0 and off.value + 128 * 128 * 128 * 4 <= ws_bytes
    for bad in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (70000, 16, 16), (1, 1 << 11, 1 << 11)):  # (the last: 2^22 positions x 576 channels)
        assert lib.flowlarge_bytes(*bad, ctypes.byref(n)) == -1, bad
        assert b"flowlarge_bytes" in err()
        assert lib.flowlarge_hidden_offset(*bad, ctypes.byref(off)) == -1, bad
        assert b"flowlarge_hidden_offset" in err()
    assert lib.flowlarge_bytes(1, 16, 16, None) == -1
    assert lib.flowlarge_hidden_offset(1, 16, 16, None) == -1
    P = _abi.FLOWLARGE_PARAMS
    table = lambda *v: (ctypes.c_void_p * P)(*v)  # noqa: E731
    full = table(*([0x1000] * P))
    hole = table(*([0x1000] * 27 + [None] + [0x1000] * 2))
    skew = table(*([0x1000] * (P - 1) + [0x1004]))

    def begin(N=1, h=128, w=128, params=full, hidden=p, context=p, ws=p, size=ws_bytes):
        return lib.flowlarge_begin(N, h, w, params, hidden, context, ws, size, None)

    for kw_ in (dict(N=0), dict(h=0), dict(w=0), dict(N=70000), dict(h=1 << 11, w=1 << 11), dict(params=None), dict(params=hole), dict(params=skew),
                dict(hidden=None), dict(context=None), dict(ws=None), dict(hidden=odd), dict(context=odd)):
        assert begin(**kw_) == -1, kw_
        assert b"flowlarge_begin" in err()
    assert begin(size=ws_bytes - 1) == -3 and b"workspace" in err()

    def step(N=1, h=128, w=128, corr=p, flow=p, ws=p, size=ws_bytes, delta=p):
        return lib.flowlarge_step(N, h, w, corr, flow, ws, size, delta, None)

    for kw_ in (dict(N=0), dict(h=0), dict(w=0), dict(N=70000), dict(corr=None), dict(flow=None), dict(ws=None), dict(delta=None),
                dict(corr=odd), dict(flow=odd), dict(delta=odd)):
        assert step(**kw_) == -1, kw_
        assert b"flowlarge_step" in err()
    assert step(size=ws_bytes - 1) == -3 and b"workspace" in err()

    def mask(N=1, h=128, w=128, ws=p, size=ws_bytes, out=p):
        return lib.flowlarge_mask(N, h, w, ws, size, out, None)

    for kw_ in (dict(N=0), dict(h=0), dict(w=0), dict(N=70000), dict(h=1 << 11, w=1 << 11), dict(ws=None), dict(out=None), dict(out=odd)):
        assert mask(**kw_) == -1, kw_
        assert b"flowlarge_mask" in err()
    assert mask(size=ws_bytes - 1) == -3 and b"workspace" in err()


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import raft

    x, wt, b = torch.zeros(1, 5, 7, 4), torch.zeros(8, 4, 1, 5), torch.zeros(8)
    for weight in (wt, torch.zeros(8, 4, 5, 1), torch.zeros(8, 4, 3, 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            raft.conv2d_rect_cl([x], weight, b)
    with pytest.raises(TypeError):
        raft.conv2d_rect_cl(x, wt, b)
    with pytest.raises(TypeError):
        raft.conv2d_rect_cl([x.double()], wt, b)
    with pytest.raises(TypeError):
        raft.conv2d_rect_cl([x], wt.half(), b)
    with pytest.raises(TypeError):
        raft.conv2d_rect_cl([x], wt, [0.0] * 8)
    for kw in (dict(inputs=[]), dict(inputs=[x] * 4), dict(inputs=[x, torch.zeros(1, 5, 8, 4)]), dict(inputs=[x[0]]),
               dict(weight=torch.zeros(8, 5, 1, 5)), dict(weight=torch.zeros(8, 4, 2, 2)), dict(weight=torch.zeros(8, 4, 9, 9)),
               dict(weight=torch.zeros(8, 4, 3, 1)), dict(weight=torch.zeros(8, 4, 1, 3)), dict(weight=torch.zeros(8, 4, 1, 7)),
               dict(weight=torch.zeros(8, 4, 5, 3)), dict(weight=torch.zeros(8, 4, 5)), dict(bias=torch.zeros(7)), dict(act="gelu"),
               dict(add=torch.zeros(1, 5, 7, 4))):
        args = dict(inputs=[x], weight=wt, bias=b)
        args.update(kw)
        with pytest.raises(ValueError):
            raft.conv2d_rect_cl(**args)
    with pytest.raises(ValueError):  # the square wrapper still refuses a rectangular weight
        raft.conv2d_cl([x], torch.zeros(8, 4, 3, 1), b)
    with pytest.raises(ValueError):
        raft.conv2d_cl([x], wt, b)

    large = raft.raft_large()
    fused = raft.FusedUpdateLarge(large.update_block, large.mask_predictor)
    with pytest.raises(RuntimeError, match="begin"):
        fused.step(torch.zeros(1, 324, 16, 16), torch.zeros(1, 2, 16, 16))
    with pytest.raises(RuntimeError, match="begin"):
        fused.hidden()
    with pytest.raises(RuntimeError, match="begin"):
        fused.mask()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.begin(torch.zeros(1, 128, 16, 16), torch.zeros(1, 128, 16, 16))
    with pytest.raises(ValueError):
        fused.begin(torch.zeros(1, 96, 16, 16), torch.zeros(1, 128, 16, 16))
    with pytest.raises(ValueError):
        fused.begin(torch.zeros(1, 128, 16, 16), torch.zeros(1, 128, 16, 17))
    with pytest.raises(ValueError):
        fused.begin(torch.zeros(1, 128, 16, 16), torch.zeros(1, 64, 16, 16))
    with pytest.raises(TypeError):
        fused.begin(torch.zeros(1, 128, 16, 16).double(), torch.zeros(1, 128, 16, 16))
    with pytest.raises(TypeError):
        fused.begin([0.0], torch.zeros(1, 128, 16, 16))
    small = raft.raft_small()
    with pytest.raises(ValueError, match="RAFT-large"):
        raft.FusedUpdateLarge(small.update_block, large.mask_predictor)
    with pytest.raises(TypeError):
        raft.FusedUpdateLarge(large, large.mask_predictor)
    with pytest.raises(TypeError):
        raft.FusedUpdateLarge(large.update_block, None)
    other = raft.MaskPredictor(128, 256, multiplier=0.5)
    with pytest.raises(ValueError, match="0.25"):
        raft.FusedUpdateLarge(large.update_block, other)
    with pytest.raises(ValueError, match="RAFT-large"):
        raft.FusedUpdateLarge(large.update_block, raft.MaskPredictor(128, 128))
    with pytest.raises(ValueError, match="fused_large"):
        raft.RAFT("small", update="fused_large")
    with pytest.raises(ValueError, match="fused_large"):
        raft.raft_small(update="fused_large")
    with pytest.raises(ValueError, match="update"):
        raft.raft_large(update="nope")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.raft_large(corr="volume", update="fused_large").eval()(torch.zeros(1, 3, 128, 128), torch.zeros(1, 3, 128, 128), num_flow_updates=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.RAFT("large", "volume", "fused_large").double().eval()(torch.zeros(1, 3, 128, 128).double(), torch.zeros(1, 3, 128, 128).double(), num_flow_updates=1)
    switched = raft.raft_small(corr="volume")
    switched.update = "fused_large"  # (set after construction, as the GPU tests switch paths)
    with pytest.raises(ValueError, match="RAFT-large"):
        switched.eval()(torch.zeros(1, 3, 128, 128), torch.zeros(1, 3, 128, 128), num_flow_updates=1)
    # what was refused before this path existed still is
    with pytest.raises(ValueError, match="fused"):
        raft.RAFT("large", update="fused")
    with pytest.raises(ValueError, match="RAFT-small"):
        raft.FusedUpdate(large.update_block)
    with pytest.raises(ValueError):
        raft.RAFT("large", encoder="fused")


def test_the_example_refuses_the_wrong_pairs():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    base = ["--gaussians", "5000", "--size", "128", "--iters", "1", "--quiet", "--flow-matching"]
    for extra in (["--flow-network", "small", "--flow-update", "fused_large"], ["--flow-update", "fused_large"],
                  ["--flow-network", "large", "--flow-update", "fused"], ["--flow-network", "large", "--flow-update", "nope"]):
        with pytest.raises(SystemExit):
            train_synthetic.main(base + extra)


def test_nothing_is_registered_and_every_name_is_exported():
    from eogs2_amd import raft

    torch.manual_seed(64)
    a = raft.raft_large(update="fused_large")
    assert a.update == "fused_large" and a.corr == "auto" and a.encoder == "torch"
    assert sum(p.numel() for p in a.parameters()) == 5_257_536
    assert sum(p.numel() for p in raft.raft_large().parameters()) == 5_257_536
    torch.manual_seed(65)
    b = raft.raft_large()
    assert b.update == "auto" and b._fused is None and a._fused is None and a._fused_enc is None
    assert isinstance(a._fused_large, raft.FusedUpdateLarge) and isinstance(b._fused_large, raft.FusedUpdateLarge)
    assert raft.raft_small()._fused_large is None
    assert not isinstance(a._fused_large, torch.nn.Module)
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]  # (the context encoder's batch norms alone)
    assert all("fused" not in n for n in a.state_dict())
    missing, unexpected = b.load_state_dict(a.state_dict(), strict=True)
    assert not missing and not unexpected
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert b.load_weights(a.torchvision_state_dict()) is b
    for name in ("conv2d_cl", "conv2d_rect_cl", "conv_info", "FusedUpdate", "FusedUpdateLarge", "AUTO_UPDATE_IS_FUSED",
                 "AUTO_UPDATE_LARGE_IS_FUSED", "RAFT", "raft_small", "raft_large"):
        assert name in raft.__all__ and hasattr(raft, name), name
    public = {n for n, v in vars(raft).items() if not n.startswith("_") and getattr(v, "__module__", None) == raft.__name__
              and (isinstance(v, type) and not issubclass(v, torch.nn.Module) or callable(v) and not isinstance(v, type))}
    assert public <= set(raft.__all__), public - set(raft.__all__)
    assert len(raft.__all__) == len(set(raft.__all__))
    import inspect

    assert list(inspect.signature(raft.raft_large).parameters) == ["corr", "encoder", "update"]
    assert raft.raft_large("volume", "torch").update == "auto"  # the positional order of before
    # the fused object holds the modules' own convolutions, in the header's order
    f = a._fused_large
    assert len(f._convs) == 15 and f._convs[0] is a.update_block.motion_encoder.convcorr1[0]
    assert f._convs[5] is a.update_block.recurrent_block.convgru1.convz and f._convs[10] is a.update_block.recurrent_block.convgru2.convq
    assert f._convs[13] is a.mask_predictor.convrelu[0] and f._convs[14] is a.mask_predictor.conv
    c = copy.deepcopy(a)  # the copy's fused update holds the COPY's convolutions, and no workspace
    assert c._fused_large is not f and c._fused_large._convs[0] is c.update_block.motion_encoder.convcorr1[0]
    assert c._fused_large._convs[14] is c.mask_predictor.conv and c._fused_large._convs[0] is not f._convs[0]
    assert len(c._fused_large._ws) == 0 and c._fused_large._state is None
    f._ws["stale"], f._state = object, (1, 1, 1, None)  # a workspace and a begun state do not travel
    d = pickle.loads(pickle.dumps(f))
    assert len(d._ws) == 0 and d._state is None and len(d._convs) == 15 and d._names == f._names
    e = copy.deepcopy(f)
    assert len(e._ws) == 0 and e._state is None


def test_auto_for_large_is_the_torch_path_on_the_cpu():
    """update="auto" for RAFT-large is the torch modules, as before the option existed: the same bits as update="torch"."""
    from eogs2_amd import raft

    torch.manual_seed(66)
    model = raft.raft_large(corr="volume", update="torch").eval()
    auto = raft.raft_large(corr="volume").eval()
    auto.load_state_dict(model.state_dict())
    g = torch.Generator().manual_seed(67)
    a, b = torch.rand(1, 3, 128, 128, generator=g) * 2 - 1, torch.rand(1, 3, 128, 128, generator=g) * 2 - 1
    with torch.inference_mode():
        want = model(a, b, num_flow_updates=1)[-1]
        got = auto(a, b, num_flow_updates=1)[-1]
    assert auto.update == "auto" and torch.equal(got, want)
