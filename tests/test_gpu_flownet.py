"""GPU (MI355X): the flow network's fused update block (eogs2_amd.raft.conv2d_cl / FusedUpdate / RAFT(update="fused") over
eogs2_amd/csrc/flownet.hip) against the float64 oracle of tests/flownet_cases.py: every convolution of RAFT-small's update
per element under the bound of a float32 fma sum, exact cases bit for bit, one update and the whole network against their
float64 runs with torch's float32 modules as the yardstick, and the network behind performOpticalmatching."""
import copy
import ctypes

import pytest
import torch

import flownet_cases as fc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # half an ulp of 1: the unit of the bound


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def ids(s):
    return "x".join(map(str, s))


def tile_shape():
    """One column and one row more than a whole number of the kernel's position tiles."""
    from eogs2_amd import raft

    tw, th = raft.conv_info()
    return (1, th + 1, 2 * tw + 1)


EPILOGUES = {"none": "FLOWNET_EPI_BIAS", "relu": "FLOWNET_EPI_RELU", "gates": "FLOWNET_EPI_GATES", "gru": "FLOWNET_EPI_GRU"}


def seg_array(chans):
    return (ctypes.c_int * len(chans))(*chans)


def new_packing(dev, chans, cout, k):
    """A packing of the library's size with every byte 0xFF (a NaN in every float): what a call does not write shows."""
    from eogs2_amd import _lib
    from eogs2_amd._host import query_bytes

    size = query_bytes(_lib.get(), "flownet_conv_pack_bytes", k, len(chans), seg_array(chans), cout)
    return torch.full((size,), 0xFF, dtype=torch.uint8, device=dev)


def pack_into(packed, chans, cout, k, weight, cout_off=0, offsets=None):
    """One eogs_flownet_conv_pack: `weight` [cout_n, cin, k, k] into the columns [cout_off, cout_off + cout_n) of `packed`, its
    channels read at `offsets` (None: in order)."""
    from eogs2_amd._host import call

    weight = weight.contiguous()
    assert weight.shape[2] == weight.shape[3] == k
    call("eogs_flownet_conv_pack", packed.device, k, len(chans), seg_array(chans), None if offsets is None else seg_array(offsets),
         weight.shape[1], cout, cout_off, weight.shape[0], weight.data_ptr(), packed.data_ptr(), packed.numel())
    return packed


def run_conv(inputs, weight, bias, act="none", add=None, flags=0, aux=None, out=None, packed=None):
    """The library's two entries with `out` and the packing filled with NaN before the call: what the kernel does not write,
    or reads without having been given, shows. `act` names the epilogue ("none", "relu", "gates" with aux = h, "gru" with
    aux = z and `out` holding h); bit s of `flags` says that inputs[s] is [N, C, h, w], FLOWNET_OUT_NCHW that `out` is;
    `packed` = (a packing made by the caller, Cout, k) stands in for `weight`; `out` given is written as it is (the caller
    prefills it), else it is [N, h, w, Cout], [N, Cout, h, w] or the gates' [2, N, h, w, Cout / 2]."""
    from eogs2_amd import _abi
    from eogs2_amd._host import call

    dev = inputs[0].device
    nchw = [bool(flags >> s & 1) for s in range(len(inputs))]
    N, h, w = (inputs[0].shape[0],) + tuple(inputs[0].shape[2:] if nchw[0] else inputs[0].shape[1:3])
    chans = [t.shape[1] if f else t.shape[3] for t, f in zip(inputs, nchw)]
    for t, f, c in zip(inputs, nchw, chans):
        assert tuple(t.shape) == ((N, c, h, w) if f else (N, h, w, c))
    if packed is None:
        cout, k = weight.shape[0], weight.shape[2]
        packed = pack_into(new_packing(dev, chans, cout, k), chans, cout, k, weight)
    else:
        packed, cout, k = packed
    if out is None:
        shape = (2, N, h, w, cout // 2) if act == "gates" else (N, cout, h, w) if flags & _abi.FLOWNET_OUT_NCHW else (N, h, w, cout)
        out = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    xs = [t.contiguous() for t in inputs] + [None] * (3 - len(inputs))
    call("eogs_flownet_conv", dev, N, h, w, k, len(chans), seg_array(chans), *(None if x is None else x.data_ptr() for x in xs), cout,
         packed.data_ptr(), packed.numel(), None if bias is None else bias.data_ptr(), None if add is None else add.data_ptr(),
         None if aux is None else aux.data_ptr(), out.data_ptr(), getattr(_abi, EPILOGUES[act]), flags)
    return out


def case_on(dev, config, shape, seed):
    inputs, weight, bias, add = fc.conv_case(config, shape, seed)
    return [t.to(dev) for t in inputs], weight.to(dev), bias.to(dev), None if add is None else add.to(dev)


def check_against_float64(dev, shape, config):
    """Every element: |hip - f64| <= (K + 2) 2^-24 M with K = k k sum C_i (+ 1 with `add`) and M = |add| + |bias| +
    conv(|x|, |W|) in float64: the standard bound of a length-K float32 fma sum in any fixed order, the bias and the plane.
    ReLU is exact given its argument. The wrapper gives the bits of the entries called by hand, a second run the same bits."""
    from eogs2_amd import raft

    shape = tile_shape() if shape == "tile" else shape
    segs, cout, k, with_add, act = config
    inputs, weight, bias, add = case_on(dev, config, shape, seed=100 + 7 * shape[1] + shape[2])
    got = run_conv(inputs, weight, bias, act, add)
    d = [t.double() for t in inputs]
    want = fc.conv_oracle(d, weight.double(), bias.double(), act, None if add is None else add.double())
    mag = fc.conv_oracle(d, weight.double(), bias.double(), act, None if add is None else add.double(), magnitude=True)
    K = k * k * sum(segs) + (1 if with_add else 0)
    assert got.shape == want.shape == shape + (cout,) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    err, bound = (got.double() - want).abs(), (K + 2) * U * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"conv {fc.config_id(config)} {shape}: largest multiple of the bound {worst:.4f}")
    assert bool((err <= bound).all()), f"{float((err - bound).max()):.3e} over the bound"
    assert torch.equal(raft.conv2d_cl(inputs, weight, bias, act, add), got)
    assert torch.equal(run_conv(inputs, weight, bias, act, add), got)


@pytest.mark.parametrize("config", fc.CONFIGS, ids=fc.config_id)
@pytest.mark.parametrize("shape", fc.SHAPES + ("tile",), ids=lambda s: s if isinstance(s, str) else ids(s))
def test_convolution_against_float64(dev, shape, config):
    check_against_float64(dev, shape, config)


def check_exact_cases(dev, config, lanes=False):
    """Bit for bit. An all-zero input returns the bias (plus `add`). A single 1.0 at each corner and at the centre, in the
    last channel of every segment, returns bias + the weight's tap at every position of its footprint: the tap orientation
    (a cross-correlation), the zero padding and the segment offsets. One NaN gives NaN at exactly the k x k footprint.
    With `lanes`, a segment that is no whole number of eight-channel chunks is also given the impulse in its channels 3 and 4,
    where it has them: the lanes on either side of the boundary between a chunk's two matrix instructions."""
    segs, cout, k, with_add, act = config
    shape = tile_shape()
    N, h, w = shape
    inputs, weight, bias, add = case_on(dev, config, shape, seed=200)
    p = (k - 1) // 2
    zeros = [torch.zeros_like(t) for t in inputs]
    plain = bias.expand(N, h, w, cout) if add is None else bias.expand(N, h, w, cout) + add
    fin = (lambda v: torch.relu(v)) if act == "relu" else (lambda v: v)
    assert torch.equal(run_conv(zeros, weight, bias, act, add), fin(plain))
    offset = 0
    for s, C in enumerate(segs):
        chs = sorted({C - 1} | ({c for c in (3, 4) if c < C} if lanes and C % 8 else set()))
        for ch, (y, x) in ((ch, yx) for ch in chs for yx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2))):
            xs = [z.clone() for z in zeros]
            xs[s][0, y, x, ch] = 1.0
            want = bias.expand(N, h, w, cout).clone()
            foot = torch.zeros(h, w, dtype=torch.bool, device=dev)
            for ky in range(k):
                for kx in range(k):
                    oy, ox = y - (ky - p), x - (kx - p)  # out(oy, ox) reads in(oy + ky - p, ox + kx - p)
                    if 0 <= oy < h and 0 <= ox < w:
                        want[0, oy, ox] = weight[:, offset + ch, ky, kx] + bias
                        foot[oy, ox] = True
            if add is not None:
                want = want + add
            got = run_conv(xs, weight, bias, act, add)
            assert torch.equal(got, fin(want)), (s, ch, y, x)
            if (y, x) == (h // 2, w // 2):
                xs[s][0, y, x, ch] = float("nan")
                nan = torch.isnan(run_conv(xs, weight, bias, act, add))
                assert bool((nan == foot[None, :, :, None].expand_as(nan)).all()), s
                assert int(foot.sum()) == min(k, h) * min(k, w) or k > min(h, w)
        offset += C


@pytest.mark.parametrize("config", fc.CONFIGS, ids=fc.config_id)
def test_convolution_exact_cases(dev, config):
    check_exact_cases(dev, config)


def check_batch_is_its_images(dev, config, shape):
    inputs, weight, bias, add = case_on(dev, config, shape, seed=300)
    both = run_conv(inputs, weight, bias, config[4], add)
    for n in range(2):
        # (clones: a slice of the batch may start off a 16-byte boundary, which the library refuses)
        one = run_conv([t[n:n + 1].clone() for t in inputs], weight, bias, config[4], None if add is None else add[n:n + 1].clone())
        assert torch.equal(one[0], both[n]), n


@pytest.mark.parametrize("config", fc.CONFIGS, ids=fc.config_id)
def test_convolution_of_a_batch_is_its_images(dev, config):
    check_batch_is_its_images(dev, config, (2, 17, 19))


@pytest.mark.parametrize("shape", fc.STEP_SHAPES, ids=ids)
def test_one_update_against_its_float64_run(dev, shape):
    """FusedUpdate (begin, step, step) against raft.UpdateBlock run by torch in float32 and in float64 on the same device,
    seeded default weights. For the hidden state and for delta, after each of two consecutive steps (the hidden state
    advances in place), the largest deviation from float64 may be at most 16 x the torch float32 module's own: the margin
    tests/test_gpu_raft.py states as the project's. The same bits on a second run, and the header's statement in float64
    (update_oracle) agrees with the module on the device too."""
    from eogs2_amd import raft

    torch.manual_seed(40)
    block = raft.raft_small(update="torch").eval().to(dev).update_block
    block64 = copy.deepcopy(block).double()
    hidden, context, corr, flow = (t.to(dev) for t in fc.update_inputs(*shape, seed=41))
    _, _, corr2, flow2 = (t.to(dev) for t in fc.update_inputs(*shape, seed=42))
    with torch.inference_mode():
        def fused_run():
            f = raft.FusedUpdate(block)
            f.begin(hidden, context)
            f._state[3].fill_(0xFF)  # the workspace as NaNs: begin and step rely on nothing they did not write
            f.begin(hidden, context)
            d1 = f.step(corr, flow)
            h1 = f.hidden()
            d2 = f.step(corr2, flow2)
            return h1, d1, f.hidden(), d2

        got = fused_run()
        h32, d32 = block(hidden, context, corr, flow)
        h32b, d32b = block(h32, context, corr2, flow2)
        h64, d64 = block64(hidden.double(), context.double(), corr.double(), flow.double())
        h64b, d64b = block64(h64, context.double(), corr2.double(), flow2.double())
        oh, od = fc.update_oracle(block64, hidden.double(), context.double(), corr.double(), flow.double())
        again = fused_run()
    assert float((oh - h64).abs().max()) <= 1e-12 * float(h64.abs().max()) and float((od - d64).abs().max()) <= 1e-12 * float(d64.abs().max())
    N, h, w = shape
    assert got[0].shape == (N, 96, h, w) and got[1].shape == (N, 2, h, w) and got[1].is_contiguous()
    for name, g, t32, t64 in (("hidden 1", got[0], h32, h64), ("delta 1", got[1], d32, d64), ("hidden 2", got[2], h32b, h64b),
                              ("delta 2", got[3], d32b, d64b)):
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all())
        mine, theirs = float((g.double() - t64).abs().max()), float((t32.double() - t64).abs().max())
        print(f"update {shape} {name}: |fused - f64| {mine:.3e}, |torch32 - f64| {theirs:.3e}, ratio {mine / max(theirs, 1e-300):.3f}, "
              f"largest |value| {float(t64.abs().max()):.3f}")
        assert mine <= 16 * theirs, name
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert not torch.equal(got[0], got[2])


@pytest.mark.parametrize("size", [(128, 128), (128, 136)], ids=ids)
def test_network_against_its_float64_run(dev, size):
    """tests/test_gpu_raft.py's protocol for RAFT-small with update="fused": seeded random weights, eval mode, 4 updates; the
    fused update over the on-demand correlation against the plain-torch volume path in float32 and in float64, which
    arbitrates. The same 16 x, for return_all=True and for the last flow alone."""
    from eogs2_amd import raft

    torch.manual_seed(20)
    model = raft.RAFT("small", corr="volume", update="torch").eval().to(dev)
    g = torch.Generator().manual_seed(21)
    H, W = size
    base = torch.rand(1, 3, H + 8, W + 8, generator=g)
    a, b = (base[:, :, 4:-4, 4:-4] * 2 - 1).to(dev), (base[:, :, 2:-6, 5:-3] * 2 - 1).to(dev)
    with torch.inference_mode():
        model.corr, model.update = "ondemand", "fused"
        fu = model(a, b, num_flow_updates=4, return_all=True)
        fu_last = model(a, b, num_flow_updates=4)
        model.corr, model.update = "volume", "torch"
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
    model = raft.raft_small(update="fused").eval().to(dev)
    g = torch.Generator().manual_seed(31)
    gt, img = torch.rand(3, 130, 150, generator=g).to(dev), torch.rand(3, 130, 150, generator=g).to(dev)
    warper = F.performOpticalmatching(False, mode=mode, model_name="small", num_flow_updates=2, model=model)
    flow, gt2, img2 = warper.get_flow(gt, img)
    assert gt2.shape == img2.shape == ((3, 128, 144) if mode == "downscale" else (3, 130, 150))
    assert flow.shape == (1, 2) + tuple(gt2.shape[1:]) and flow.dtype == torch.float32 and bool(torch.isfinite(flow).all())
