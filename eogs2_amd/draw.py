"""Per-iteration random draws on the device: the background and the virtual camera, over the C-ABI of include/eogs_draw.h.

The reference draws three things at random in every training iteration: the view (train_pan.py:252-257; here
`eogs2_amd.views`), the background — `bg = torch.rand(5)`, then `bg[3] = cam.altitude_bounds[0].item()` and `bg[4] = 0`
(train_pan.py:272-277) — and the virtual camera of the random-camera consistency loss, `cam.sample_random_camera(extent)`
(scene/cameras/affine_cameras.py:403-430, called at train_pan.py:375-378), which shears the view's affine by
`randn(2).clip(-1, 1) * extent`. Both of the latter wait for the device and build tensors on the host, so neither can sit in a
recorded step. Here ONE launch of one wave does both for up to eight cameras, from a counter-based generator keyed by the
iteration's index on the device:

    stream = DrawStream(seed, counter=schedule.cursor)       # or counter=None: the stream owns its counter
    draws = IterationDraws(stream)
    draws.add_camera(cam.affine, center, bg=bg, virt_affine=rnd.affine, cam2virt=cam2rnd, extent=0.02)

    def fn():                                                # the function of a GraphedStep
        bank.load()
        draws.draw()                                         # writes bg, rnd.affine, cam2rnd after the load filled them
        ... forwards, losses, backward, optimizer steps ...
        bank.store(gate)
        schedule.advance(gate)                               # moves the cursor, and with it the stream

Every draw is a pure function of (seed, iteration, camera slot): `draws_for` states it in Python integers, with no device. A
replay whose gate is closed does not move the cursor, so the replay recorded again sees the same view with the same draws;
a checkpoint holds the seed, the cursor holds the rest.

This is another generator than torch's: for one seed the sequences differ from the reference's. The statistics are the
reference's — uniforms of [0, 1), standard normals clipped to [-1, 1]. There is no CPU fallback.
"""
import ctypes
import math
import struct

import torch

from . import _lib
from ._abi import DRAW_BG, DRAW_BG_COPY_FIRST, DRAW_CAMERA, DRAW_MAX_CAMERAS, DRAW_NADIR, DrawCamera, DrawStreamDesc
from ._host import Ctx, ptr
from .views import _check_gate

PURPOSE_BG, PURPOSE_SHEAR = 0, 1
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 in Python integers: `counter` four and `key` two 32-bit words; returns four words. The restatement of
    eogs2_amd/csrc/draw_rng.h."""
    c0, c1, c2, c3 = (int(x) & _MASK for x in counter)
    k0, k1 = (int(x) & _MASK for x in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def block_for(seed, iteration, slot, purpose):
    """The four words of (seed, iteration, camera slot, purpose): key = the seed's low and high word, counter = (iteration
    low, iteration high, slot, purpose)."""
    seed, iteration = int(seed), int(iteration)
    if not 0 <= seed < 1 << 64:
        raise ValueError("draws: seed must fit 64 unsigned bits")
    if not 0 <= iteration < 1 << 64:
        raise ValueError("draws: iteration must fit 64 unsigned bits")
    if not 0 <= int(slot) < 1 << 32 or not 0 <= int(purpose) < 1 << 32:
        raise ValueError("draws: slot and purpose are 32-bit words")
    return philox4x32_10((iteration & _MASK, iteration >> 32, int(slot), int(purpose)), (seed & _MASK, seed >> 32))


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def uniform_of(word):
    """(w >> 8) * 2^-24: exact in fp32, in [0, 1)."""
    return (int(word) >> 8) * 2.0 ** -24


def normals_of(w0, w1):
    """One Box-Muller pair in double, each rounded to fp32 and clamped to [-1, 1] (as Python floats holding fp32 values)."""
    u1, u2 = (int(w0) + 0.5) * 2.0 ** -32, (int(w1) + 0.5) * 2.0 ** -32
    r = math.sqrt(-2.0 * math.log(u1))
    a = 2.0 * math.pi * u2
    return tuple(min(max(_f32(z), -1.0), 1.0) for z in (r * math.cos(a), r * math.sin(a)))


def draws_for(seed, iteration, slot):
    """(three background uniforms, two clipped normals) of camera `slot` at `iteration` of the stream `seed`: what
    `IterationDraws.draw()` uses on the device, computed here in Python integers and doubles. The uniforms are the device's
    bit for bit; the normals are the device's up to its double `log` / `sin` / `cos` (one fp32 ulp at most). The shear of a
    random camera is `normal * extent` in fp32."""
    bg = block_for(seed, iteration, slot, PURPOSE_BG)
    sh = block_for(seed, iteration, slot, PURPOSE_SHEAR)
    return tuple(uniform_of(w) for w in bg[:3]), normals_of(sh[0], sh[1])


def _require_device(dev, who):
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: tensors on '{dev.type}': the draws live on the GPU, there is no CPU fallback")


def check_stream(seed, counter, device):
    """The refusals of `DrawStream`, before anything touches a device. Returns (seed, device)."""
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError("DrawStream: seed must be an int")
    if not 0 <= seed < 1 << 64:
        raise ValueError("DrawStream: seed must fit 64 unsigned bits")
    if counter is not None:
        if not isinstance(counter, torch.Tensor):
            raise TypeError("DrawStream: counter must be a torch.Tensor (an int64 device scalar such as ViewSchedule.cursor)")
        if counter.dtype != torch.int64 or counter.numel() != 1:
            raise ValueError("DrawStream: counter must be one int64 element")
        if device is not None and torch.device(device).type != counter.device.type:
            raise RuntimeError(f"DrawStream: counter lives on {counter.device}, device is {device}")
        device = counter.device
    if device is None:
        raise ValueError("DrawStream: a stream that owns its counter needs a device")
    device = torch.device(device)
    _require_device(device, "DrawStream")
    return seed, device


class DrawStream:
    """A seed and the device int64 the iteration's index is read from (eogs_draw_stream). `counter`: an int64 device scalar,
    for example `ViewSchedule.cursor` — whoever owns it moves it; None: the stream owns one, starting at 0, and `advance`
    moves it."""

    def __init__(self, seed, counter=None, device=None):
        self.seed, device = check_stream(seed, counter, device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.shared = counter is not None
        self.counter = counter if self.shared else torch.zeros((), dtype=torch.int64, device=device)
        self._struct = DrawStreamDesc(self.seed, self.counter.data_ptr())

    def advance(self, gate=None):
        """counter += 1 on the device, unless `gate` (eogs2_amd.rasterizer.captured_gate()) is closed."""
        if self.shared:
            raise RuntimeError("DrawStream.advance: the counter is not this stream's own (a schedule's cursor): its owner advances it")
        _check_gate(gate, self.device, "DrawStream.advance")
        abi = _lib.get()
        with Ctx(abi, self.device) as cx:
            abi.check(abi.draw_advance(ptr(self.counter), ptr(gate), cx.stream))

    def seek(self, k):
        """counter = k: a device write, no wait."""
        if self.shared:
            raise RuntimeError("DrawStream.seek: the counter is not this stream's own (a schedule's cursor): seek its owner")
        if not 0 <= int(k) < 1 << 63:
            raise ValueError("DrawStream.seek: an iteration index lies in 0 .. 2^63 - 1")
        self.counter.fill_(int(k))

    def position(self):
        """The counter: one wait for the device."""
        return int(self.counter)

    def state_dict(self):
        return {"seed": self.seed, "counter": self.position(), "shared": self.shared}

    def load_state_dict(self, sd):
        if int(sd["seed"]) != self.seed:
            raise ValueError(f"DrawStream.load_state_dict: the state's seed {int(sd['seed'])} is not this stream's {self.seed}")
        if bool(sd["shared"]) != self.shared:
            raise ValueError("DrawStream.load_state_dict: one of the two streams owns its counter, the other does not")
        if not self.shared:  # (a shared counter comes back with its owner's state)
            self.seek(sd["counter"])


_SHAPES = {"affine": (4, 4), "center": (3,), "alt_floor": (1,), "bg": (5,), "virt_affine": (4, 4), "cam2virt": (3, 3), "shear": (2,)}
_OUTPUTS = ("bg", "virt_affine", "cam2virt", "shear")


def _overlap(a, b):
    if a.device != b.device or a.is_meta:  # (two devices share no memory; a meta tensor has none)
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def check_camera(device, affine, center, alt_floor=None, *, bg=None, copy_first=False, virt_affine=None, cam2virt=None, extent=None,
                 nadir=False, cam2virt_scale=1.0, shear=None, others=()):
    """The refusals of `IterationDraws.add_camera`, before anything touches a device: type, dtype, shape, contiguity, the
    parameters, what the flags need, aliasing of an output with an input (of this camera or of `others`, the tensors of the
    cameras added before: {name: tensor} each), and the device last. Returns the camera's flags."""
    t = {"affine": affine, "center": center, "alt_floor": alt_floor, "bg": bg, "virt_affine": virt_affine, "cam2virt": cam2virt,
         "shear": shear}
    for name, x in t.items():
        if x is None:
            continue
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"IterationDraws: {name} must be a torch.Tensor")
        if x.dtype != torch.float32:
            raise ValueError(f"IterationDraws: {name} must be float32, not {x.dtype}")
        want = _SHAPES[name]
        if tuple(x.shape) != want and not (name == "alt_floor" and x.numel() == 1):
            raise ValueError(f"IterationDraws: {name} must have shape {want}, not {tuple(x.shape)}")
        if not x.is_contiguous():
            raise ValueError(f"IterationDraws: {name} must be contiguous (a recorded step reads it by address)")
    for name, x in (("extent", extent), ("cam2virt_scale", cam2virt_scale)):
        if x is None:
            continue
        if isinstance(x, (bool, torch.Tensor)) or not isinstance(x, (int, float)):
            raise TypeError(f"IterationDraws: {name} must be a number (it becomes a kernel argument)")
        if not (math.isfinite(x) and x >= 0):
            raise ValueError(f"IterationDraws: {name} must be finite and not negative, not {x}")
    if cam2virt_scale is None:
        raise TypeError("IterationDraws: cam2virt_scale must be a number")
    flags = 0
    if bg is not None:
        flags |= DRAW_BG | (DRAW_BG_COPY_FIRST if copy_first else 0)
    elif copy_first:
        raise ValueError("IterationDraws: copy_first without bg")
    elif alt_floor is not None:
        raise ValueError("IterationDraws: alt_floor without bg")
    if nadir and extent is not None:
        raise ValueError("IterationDraws: nadir and extent together: a camera is either the nadir one or a sampled one")
    if nadir or extent is not None:
        flags |= DRAW_NADIR if nadir else DRAW_CAMERA
        if affine is None:
            raise ValueError("IterationDraws: a virtual camera needs affine")
        if virt_affine is None and cam2virt is None and shear is None:
            raise ValueError("IterationDraws: a virtual camera needs one of virt_affine, cam2virt, shear to write to")
        if virt_affine is not None and center is None:
            raise ValueError("IterationDraws: virt_affine needs center")
    elif virt_affine is not None or cam2virt is not None or shear is not None:
        raise ValueError("IterationDraws: virt_affine, cam2virt and shear need extent or nadir=True")
    if not flags:
        raise ValueError("IterationDraws: the camera asks for nothing: give bg, extent or nadir=True")
    mine = {k: v for k, v in t.items() if v is not None}
    for name in _OUTPUTS:  # this camera's outputs against everything else of the launch
        if name not in mine:
            continue
        for oname, x in mine.items():
            if oname != name and _overlap(mine[name], x):
                raise ValueError(f"IterationDraws: output {name} overlaps {oname}: an output aliases no other tensor of the launch")
        for other in others:
            for oname, x in other.items():
                if _overlap(mine[name], x):
                    raise ValueError(f"IterationDraws: output {name} overlaps {oname} of another camera: the lanes run side by side")
    for other in others:  # the earlier cameras' outputs against this camera's inputs
        for oname in _OUTPUTS:
            for iname, x in mine.items():
                if oname in other and iname not in _OUTPUTS and _overlap(other[oname], x):
                    raise ValueError(f"IterationDraws: input {iname} overlaps output {oname} of another camera: the lanes run side by side")
    for name, x in mine.items():
        if x.device != device:
            _require_device(x.device, f"IterationDraws: {name}")
            raise RuntimeError(f"IterationDraws: {name} lives on {x.device}, the stream on {device}")
    return flags


class IterationDraws:
    """The cameras of one iteration and the one launch that draws for all of them.

    add_camera(affine, center, alt_floor=None, *, bg=None, copy_first=False, virt_affine=None, cam2virt=None, extent=None,
               nadir=False, cam2virt_scale=1.0, shear=None)

        bg           float32[5]: [0..2] = three uniforms (copy_first: the first one three times, the reference's
                     copy_background_firschan), [3] = alt_floor[0] if given, else left alone, [4] = 0
        extent       virtual_camera_extent: the camera is `sample_random_camera(extent)` of the view `affine` (4 x 4, stored
                     transposed as the reference stores it) about `center` (centerofscene_ECEF)
        nadir        instead: `get_nadir_camera()`, the same formula with a deterministic shear; reads no generator
        virt_affine  float32[4, 4]: the virtual camera's affine, transposed like `affine`
        cam2virt     float32[3, 3]: the reference's myM, its two shear entries times `cam2virt_scale`
        shear        float32[2]: the two shear entries themselves

    Slots are numbered in the order they are added: the slot is part of the generator's counter, so two cameras of one
    iteration draw from different blocks. `affine` and `center` may be None for a camera that only asks for a background."""

    def __init__(self, stream):
        self.stream = stream
        self.device = stream.device
        self._cameras = []  # ({name: tensor}, DrawCamera fields)
        self._arr = None

    def __len__(self):
        return len(self._cameras)

    def add_camera(self, affine, center, alt_floor=None, *, bg=None, copy_first=False, virt_affine=None, cam2virt=None, extent=None,
                   nadir=False, cam2virt_scale=1.0, shear=None):
        if len(self._cameras) >= DRAW_MAX_CAMERAS:
            raise ValueError(f"IterationDraws: at most {DRAW_MAX_CAMERAS} cameras in one launch")
        flags = check_camera(self.device, affine, center, alt_floor, bg=bg, copy_first=copy_first, virt_affine=virt_affine,
                             cam2virt=cam2virt, extent=extent, nadir=nadir, cam2virt_scale=cam2virt_scale, shear=shear,
                             others=[t for t, _ in self._cameras])
        tensors = {k: v for k, v in (("affine", affine), ("center", center), ("alt_floor", alt_floor), ("bg", bg),
                                     ("virt_affine", virt_affine), ("cam2virt", cam2virt), ("shear", shear)) if v is not None}
        self._cameras.append((tensors, (float(extent or 0.0), float(cam2virt_scale), flags)))
        self._arr = None
        return len(self._cameras) - 1

    def _descriptors(self):
        if self._arr is None:
            arr = (DrawCamera * max(1, len(self._cameras)))()
            for a, (t, (extent, scale, flags)) in zip(arr, self._cameras):
                for name in _SHAPES:
                    setattr(a, name, t[name].data_ptr() if name in t else None)
                a.extent, a.cam2virt_scale, a.flags = extent, scale, flags
            self._arr = arr
        return self._arr

    def draw(self):
        """One launch: every camera's draws at the stream's current iteration."""
        abi = _lib.get()
        arr = self._descriptors()
        with Ctx(abi, self.device) as cx:
            abi.check(abi.draw_iteration(len(self._cameras), ctypes.cast(arr, ctypes.c_void_p), ctypes.byref(self.stream._struct), cx.stream))


__all__ = ["DrawStream", "IterationDraws", "draws_for", "block_for", "philox4x32_10", "uniform_of", "normals_of", "check_stream",
           "check_camera"]
