"""CPU: the surface of the flow network (the eogs_raft_* entries of include/eogs_resample.h, eogs2_amd.raft) without a device — header and binding table,
every refusal before a launch, both published configurations, strict loading of a state dict, and the whole network's
forward on the CPU through its plain-torch correlation (corr="volume")."""
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


NAMES = ["eogs_raft_bytes", "eogs_raft_level_offset", "eogs_raft_lookup", "eogs_raft_pyramid", "eogs_raft_stage_info", "eogs_raft_upsample"]


def test_header_table_and_constants_agree():
    from eogs2_amd import _abi

    assert _abi.ABI_VERSION == 8  # entry points were added, nothing changed
    # the entries live beside the flow warp's, in the header of the flow-matching step
    decl = {k: v for k, v in AC.declared("eogs_resample.h").items() if k.startswith("eogs_raft_")}
    table = {k: v for k, v in _abi.HEADERS["eogs_resample.h"].items() if k.startswith("eogs_raft_")}
    assert sorted(decl) == sorted(table) == NAMES
    for name, (res, args) in table.items():
        assert decl[name] == len(args) and res is ctypes.c_int, name
        assert name in _abi.HIP_ONLY
    text = AC.header_text("eogs_resample.h")
    defines = {k: int(v) for k, v in re.findall(r"#define (EOGS_RAFT_[A-Z_]+) (\d+)u?\b", text)}
    assert defines == {"EOGS_RAFT_MAX_LEVELS": _abi.RAFT_MAX_LEVELS, "EOGS_RAFT_MAX_RADIUS": _abi.RAFT_MAX_RADIUS,
                       "EOGS_RAFT_NO_STAGE": _abi.RAFT_NO_STAGE, "EOGS_RAFT_UP_CONVEX": _abi.RAFT_UP_CONVEX,
                       "EOGS_RAFT_UP_BILINEAR": _abi.RAFT_UP_BILINEAR, "EOGS_RAFT_MASK_CHANNELS": _abi.RAFT_MASK_CHANNELS}
    taps = open(AC.ROOT + "/eogs2_amd/csrc/raft_taps.h").read()
    assert len(re.findall(r"#define EOGS_RAFT_X_OFFSET_IS_SLOW 1\b", taps)) == 1  # the tap order is ONE named constant


def test_library_refuses_before_a_launch(lib):
    """Every refusal comes back as a status with a message before anything touches a device (there is none here): the
    pointers are made up and never read."""
    assert lib.cdll.eogs_rast_abi_version() == 8
    n = ctypes.c_size_t()
    lib.check(lib.raft_bytes(1, 128, 128, 128, 4, ctypes.byref(n)))
    # 1.33 n C 4 bytes: linear in the number of positions
    cells = 128 * 128 + 64 * 64 + 32 * 32 + 16 * 16
    assert cells * 128 * 4 <= n.value <= cells * 128 * 4 + 4 * 256 + 512
    lib.check(lib.raft_bytes(2, 256, 17, 19, 4, ctypes.byref(n)))
    assert n.value >= 2 * 256 * 4 * (17 * 19 + 8 * 9 + 4 * 4 + 2 * 2)
    off = ctypes.c_size_t()
    lib.check(lib.raft_level_offset(2, 256, 17, 19, 0, ctypes.byref(off)))
    assert off.value == 0
    lib.check(lib.raft_level_offset(2, 256, 17, 19, 1, ctypes.byref(off)))
    assert off.value == 2 * 256 * 4 * 17 * 19 and off.value % 256 == 0
    for bad in ((0, 128, 16, 16, 4), (1, 0, 16, 16, 4), (1, 128, 0, 16, 4), (1, 128, 16, 0, 4), (1, 126, 16, 16, 4),
                (1, 128, 16, 16, 0), (1, 128, 16, 16, 5), (1, 128, 7, 16, 4), (1, 128, 16, 7, 4), (70000, 128, 16, 16, 4),
                (1, 128, 8192, 8192, 1)):
        assert lib.raft_bytes(*bad, ctypes.byref(n)) == -1, bad
        assert b"raft_bytes" in lib.cdll.eogs_rast_last_error()
    assert lib.raft_bytes(1, 128, 16, 16, 4, None) == -1
    p = ctypes.c_void_p(0x1000)  # (never dereferenced: every call below is refused)
    lib.check(lib.raft_bytes(1, 128, 16, 16, 4, ctypes.byref(n)))
    assert lib.raft_pyramid(1, 128, 16, 16, 4, None, p, n.value, None) == -1
    assert lib.raft_pyramid(1, 128, 16, 16, 4, p, None, n.value, None) == -1
    assert b"NULL" in lib.cdll.eogs_rast_last_error()
    assert lib.raft_pyramid(1, 128, 16, 16, 4, p, p, n.value - 1, None) == -3
    assert b"workspace" in lib.cdll.eogs_rast_last_error()
    assert lib.raft_pyramid(1, 130, 16, 16, 4, p, p, 1 << 30, None) == -1
    assert b"multiple of 4" in lib.cdll.eogs_rast_last_error()

    def lookup(N=1, C=128, h=16, w=16, levels=4, radius=3, f1=p, pyr=p, coords=p, out=p, flags=0):
        return lib.raft_lookup(N, C, h, w, levels, radius, f1, pyr, coords, out, flags, None)

    for kw in (dict(radius=0), dict(radius=5), dict(flags=2), dict(f1=None), dict(pyr=None), dict(coords=None), dict(out=None),
               dict(C=6), dict(levels=5), dict(h=7), dict(coords=ctypes.c_void_p(0x1004)), dict(out=ctypes.c_void_p(0x1008))):
        assert lookup(**kw) == -1, kw
        assert b"raft_lookup" in lib.cdll.eogs_rast_last_error()

    def up(N=1, h=5, w=7, mode=0, flow=p, mask=p, out=p):
        return lib.raft_upsample(N, h, w, mode, flow, mask, out, None)

    for kw in (dict(N=0), dict(h=0), dict(w=0), dict(h=8193), dict(mode=2), dict(mode=-1), dict(flow=None), dict(out=None),
               dict(mask=None), dict(mode=1), dict(out=ctypes.c_void_p(0x1004))):
        assert up(**kw) == -1, kw
        assert b"raft_upsample" in lib.cdll.eogs_rast_last_error()
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.check(lib.raft_stage_info(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    assert a.value * b.value % 64 == 0 and a.value >= 32  # whole waves, and a wave writes whole 128-byte lines per channel
    assert c.value * 80 <= 80 * 1024  # the staged box of a workgroup: at least two workgroups share a CU's 160 KiB
    assert lib.raft_stage_info(None, ctypes.byref(b), ctypes.byref(c)) == -1


def test_wrappers_refuse_what_they_cannot_run():
    from eogs2_amd import raft

    fmap, c = torch.zeros(1, 8, 16, 16), torch.zeros(1, 2, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.corr_pyramid(fmap)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.upsample_flow(c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.upsample_flow(c, torch.zeros(1, 576, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.raft_small(corr="ondemand")(torch.zeros(1, 3, 128, 128), torch.zeros(1, 3, 128, 128), num_flow_updates=1)
    for bad in (fmap.double(), fmap.half()):
        with pytest.raises(TypeError):
            raft.corr_pyramid(bad)
    with pytest.raises(TypeError):
        raft.corr_pyramid([1.0])
    for bad in (fmap[0], torch.zeros(1, 6, 16, 16), torch.zeros(0, 8, 16, 16), torch.zeros(1, 8, 7, 16)):
        with pytest.raises(ValueError):
            raft.corr_pyramid(bad)
    with pytest.raises(ValueError, match="levels"):
        raft.corr_pyramid(fmap, levels=5)
    with pytest.raises(TypeError, match="corr_pyramid returns"):
        raft.corr_lookup(fmap, fmap, c, 3)
    pyr = raft.CorrPyramid(torch.zeros(1 << 20, dtype=torch.uint8), 1, 8, 16, 16, 4)
    one = raft.CorrPyramid(torch.zeros(1 << 20, dtype=torch.uint8), 1, 8, 16, 16, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raft.corr_lookup(one, pyr, c, 3)
    for kw in (dict(radius=0), dict(radius=5)):
        with pytest.raises(ValueError, match="radius"):
            raft.corr_lookup(one, pyr, c, **kw)
    with pytest.raises(ValueError):
        raft.corr_lookup(one, pyr, torch.zeros(1, 2, 16, 17), 3)
    with pytest.raises(ValueError, match="differ in shape"):
        raft.corr_lookup(raft.CorrPyramid(one.buffer, 1, 8, 16, 17, 1), pyr, c, 3)
    with pytest.raises(TypeError):
        raft.corr_lookup(one, pyr, c.double(), 3)
    with pytest.raises(ValueError):
        raft.upsample_flow(torch.zeros(1, 3, 5, 7))
    with pytest.raises(ValueError, match="mask"):
        raft.upsample_flow(c, torch.zeros(1, 576, 16, 17))
    with pytest.raises(ValueError):
        raft.RAFT("medium")
    with pytest.raises(ValueError):
        raft.RAFT("small", corr="cudnn")


def test_both_configurations_build_as_published():
    import eogs2_amd
    from eogs2_amd import raft

    assert eogs2_amd.raft is raft
    small, large = raft.raft_small(), raft.raft_large()
    # the parameter counts torchvision documents for raft_small and raft_large
    assert sum(p.numel() for p in small.parameters()) == 990_162
    assert sum(p.numel() for p in large.parameters()) == 5_257_536
    assert (small.corr_levels, small.corr_radius, large.corr_levels, large.corr_radius) == (4, 3, 4, 4)
    assert small.mask_predictor is None and large.mask_predictor is not None
    assert small.feature_encoder.conv.out_channels == 128 and large.feature_encoder.conv.out_channels == 256
    assert small.context_encoder.conv.out_channels == 160 and large.context_encoder.conv.out_channels == 256
    assert small.update_block.motion_encoder.convcorr1[0].in_channels == 4 * 49
    assert large.update_block.motion_encoder.convcorr1[0].in_channels == 4 * 81
    assert small.update_block.motion_encoder.out_channels == 82 and large.update_block.motion_encoder.out_channels == 128
    assert small.update_block.hidden_state_size == 96 and large.update_block.hidden_state_size == 128
    assert small.update_block.recurrent_block.convgru1.convz.kernel_size == (3, 3)
    assert large.update_block.recurrent_block.convgru1.convz.kernel_size == (1, 5)
    assert large.update_block.recurrent_block.convgru2.convz.kernel_size == (5, 1)
    assert small.update_block.flow_head.conv1.out_channels == 128 and large.update_block.flow_head.conv1.out_channels == 256
    assert large.mask_predictor.conv.out_channels == 576 and large.mask_predictor.multiplier == 0.25
    keys = set(large.state_dict())
    for k in ("feature_encoder.convnormrelu.0.weight", "feature_encoder.layer2.0.downsample.0.bias", "feature_encoder.conv.weight",
              "context_encoder.layer1.0.convnormrelu1.1.running_mean", "update_block.motion_encoder.convcorr2.0.weight",
              "update_block.recurrent_block.convgru2.convq.bias", "update_block.flow_head.conv2.weight",
              "mask_predictor.convrelu.0.weight", "mask_predictor.conv.bias"):
        assert k in keys, k
    assert not any(k.startswith("feature_encoder") and "running_mean" in k for k in keys)  # instance norm: no state
    assert all(k.split(".")[0] in raft.TORCHVISION_NAMES for k in keys)


@pytest.mark.parametrize("name", ["small", "large"])
def test_state_dict_round_trips_strictly(name, tmp_path):
    from eogs2_amd import raft

    torch.manual_seed(0)
    a = raft.RAFT(name)
    sd = a.torchvision_state_dict()
    torch.manual_seed(1)
    b = raft.RAFT(name)
    assert b.load_weights(sd) is b and not b.training
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    path = str(tmp_path / "w.pth")
    torch.save(sd, path)
    c = raft.RAFT(name).load_weights(path)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), c.state_dict().values()))
    missing = dict(sd)
    missing.pop("update_block.flow_head.conv2.bias")
    with pytest.raises(RuntimeError, match="Missing key"):
        raft.RAFT(name).load_weights(missing)
    extra = dict(sd)
    extra["update_block.flow_head.conv3.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        raft.RAFT(name).load_weights(extra)
    other = raft.RAFT("large" if name == "small" else "small").torchvision_state_dict()
    with pytest.raises(RuntimeError):
        raft.RAFT(name).load_weights(other)


@pytest.mark.parametrize("name", ["small", "large"])
@pytest.mark.parametrize("size", [(128, 128), (128, 136)])
def test_forward_on_the_cpu(name, size):
    from eogs2_amd import raft

    torch.manual_seed(2)
    model = raft.RAFT(name, corr="volume").eval()
    g = torch.Generator().manual_seed(3)
    H, W = size
    a, b = torch.rand(1, 3, H, W, generator=g) * 2 - 1, torch.rand(1, 3, H, W, generator=g) * 2 - 1
    with torch.inference_mode():
        every = model(a, b, num_flow_updates=2, return_all=True)
        last = model(a, b, num_flow_updates=2)
        auto = raft.RAFT(name).eval()
        auto.load_state_dict(model.state_dict())
        same = auto(a, b, num_flow_updates=2)  # "auto" off the GPU is the volume path
    assert len(every) == 2 and len(last) == 1
    for f in every + last:
        assert f.shape == (1, 2, H, W) and f.dtype == torch.float32 and bool(torch.isfinite(f).all())
    assert torch.equal(every[-1], last[-1]) and torch.equal(same[-1], last[-1])
    assert not torch.equal(every[0], every[1])


def test_forward_refuses_torchvision_s_sizes():
    from eogs2_amd import raft

    model = raft.raft_small(corr="volume").eval()
    for H, W in ((120, 128), (128, 120)):
        with pytest.raises(ValueError, match="at least 128"):
            model(torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W))
    for H, W in ((130, 128), (128, 130)):
        with pytest.raises(ValueError, match="divisible by 8"):
            model(torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W))
    with pytest.raises(ValueError, match="same shape"):
        model(torch.zeros(1, 3, 128, 128), torch.zeros(1, 3, 128, 136))


def test_flow_module_keeps_raising_without_a_network():
    from eogs2_amd.flow import performOpticalmatching

    with pytest.raises(RuntimeError, match="the flow network is the caller's"):
        performOpticalmatching(True, model_name="small")._get_model()
