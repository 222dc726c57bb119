"""The rescalers every ground-truth image goes through, over the C-ABI of include/eogs_gtprep.h.

Same names as the reference's utils/rescaler/rescaler.py (under src/gaussiansplatting/): `clamper`, `standard_rescaler`,
`rescale_wrt_firstimage`, `histogram_equalizer`, `identity_rescaler`, `CLAHE_rescaler`, `load_rescaler`,
`perform_rescaling_listcam`, `perform_rescaling`, `compute_min_vals`, `compute_max_vals`. Images are (C, H, W) float32 on the
device; results are new tensors without gradient (ground truth). The three arithmetic rescalers equal the reference's fp32
torch result bit for bit (the library is built without contraction and with correctly rounded division); a channel that
holds a NaN has NaN extrema, as torch.min / torch.max, and comes out all NaN.

`rescale_wrt_firstimage` keeps `min_vals` / `max_vals` on the device and prints nothing (the reference's prints wait for
the device). `histogram_equalizer` restates torchvision's documented per-channel `equalize` rule in integers (torchvision
is not imported); float -> uint8 is x * 255 clamped to [0, 255] and truncated, a NaN becomes 0 (the reference's conversion
is undefined outside that range). `CLAHE_rescaler` raises NotImplementedError: kornia stays the caller's. CPU tensors
raise (no CPU fallback).
"""
import torch

from . import _lib
from ._host import call, nbytes, on_device


def _workspace(dev, C):
    n = nbytes(_lib.get(), "gtprep_bytes", C)
    return torch.empty((n,), dtype=torch.uint8, device=dev), n


def _image(x, what, dims=(3,)):
    if not torch.is_tensor(x):
        raise TypeError(f"rescaler {what}: the image is a tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise TypeError(f"rescaler {what}: the image is float32, not {x.dtype}")
    if (dims and x.ndim not in dims) or x.numel() == 0:
        raise ValueError(f"rescaler {what}: a non-empty (C, H, W) image, got {tuple(x.shape)}")
    on_device("rescaler", "ground-truth preparation runs", x, what)
    return x.detach().contiguous()


def channel_minmax(image):
    """f32[C, 2] = {min, max} of every channel of a (C, H, W) image, on the device (torch.min / torch.max's NaN rule)."""
    x = _image(image, "channel_minmax")
    C = x.shape[0]
    mm = torch.empty((C, 2), dtype=torch.float32, device=x.device)
    ws, n = _workspace(x.device, C)
    call("eogs_gtprep_minmax", x.device, C, x.numel() // C, x.data_ptr(), mm.data_ptr(), ws.data_ptr(), n)
    return mm


def compute_min_vals(image):
    return channel_minmax(image)[:, 0]


def compute_max_vals(image):
    return channel_minmax(image)[:, 1]


def _rescale(x, mm, what):
    x = _image(x, what)
    C = x.shape[0]
    if tuple(mm.shape) != (C, 2) or mm.device != x.device:
        raise ValueError(f"rescaler {what}: the extrema are those of {mm.shape[0]} channels, the image has {C}")
    out = torch.empty_like(x)
    call("eogs_gtprep_rescale", x.device, C, x.numel() // C, x.data_ptr(), mm.data_ptr(), out.data_ptr())
    return out


class base_rescaler:
    def __init__(self):
        pass

    def forward(self, x):
        return x

    def setup(self, list_cam):
        return self


class clamper(base_rescaler):
    def __init__(self, min_val=0, max_val=1):
        self.min_val = min_val
        self.max_val = max_val

    def forward(self, x):
        x = _image(x, "clamper", dims=())
        out = torch.empty_like(x)
        call("eogs_gtprep_clamp", x.device, x.numel(), x.data_ptr(), float(self.min_val), float(self.max_val), out.data_ptr())
        return out


class rescale_wrt_firstimage(base_rescaler):
    def __init__(self):
        self.min_vals = self.max_vals = self._mm = None

    def setup(self, list_cam):
        main_cam = next((cam for cam in list_cam if cam.is_reference_camera), None)
        assert main_cam is not None, "we didn't find the reference camera"
        self._mm = channel_minmax(main_cam.original_image)
        self.min_vals, self.max_vals = self._mm[:, 0], self._mm[:, 1]  # on the device, never printed
        return self

    def forward(self, x):
        assert self._mm is not None, "Call setup() before forward()"
        return _rescale(x, self._mm, "rescale_wrt_firstimage")


class standard_rescaler(base_rescaler):
    def __init__(self):
        pass

    def forward(self, x):
        return _rescale(x, channel_minmax(x), "standard_rescaler")


class histogram_equalizer(base_rescaler):
    def __init__(self):
        pass

    def forward(self, x):
        x = _image(x, "histogram_equalizer")
        C = x.shape[0]
        out = torch.empty_like(x)
        ws, n = _workspace(x.device, C)
        call("eogs_gtprep_equalize", x.device, C, x.numel() // C, x.data_ptr(), out.data_ptr(), ws.data_ptr(), n)
        return out


class identity_rescaler(base_rescaler):
    def __init__(self):
        pass

    def forward(self, x):
        return x


class CLAHE_rescaler(base_rescaler):
    def __init__(self):
        raise NotImplementedError("CLAHE_rescaler: kornia's equalize_clahe stays the caller's; use the reference's class")


_BY_NAME = {"standard_rescaler": standard_rescaler, "rescale_wrt_firstimage": rescale_wrt_firstimage, "clamper": clamper,
            "histogram_equalizer": histogram_equalizer, "CLAHE_rescaler": CLAHE_rescaler, "identity": identity_rescaler}


def load_rescaler(rescaler_name):
    """A new rescaler of that name; an unknown name raises the reference's ValueError."""
    if rescaler_name not in _BY_NAME:
        raise ValueError(f"Unknown rescaler name: {rescaler_name}")
    return _BY_NAME[rescaler_name]()


def perform_rescaling_listcam(list_cam, rescaler):
    """`cam.original_image` of every camera replaced by its rescaled image, after `rescaler.setup(list_cam)`."""
    ready = rescaler.setup(list_cam)
    for cam in list_cam:
        cam.original_image = ready.forward(cam.original_image)
    return list_cam


def perform_rescaling(train_cameras, rescaler, args):
    """The PAN cameras (`args.load_pan`) and the MSI cameras (`args.load_msi`) of the training set, each list on its own."""
    for wanted, getter in ((args.load_pan, "get_pan_cameras"), (args.load_msi, "get_msi_cameras")):
        if wanted:
            perform_rescaling_listcam([getattr(cam, getter)() for cam in train_cameras], rescaler)
    return train_cameras


__all__ = ["base_rescaler", "clamper", "standard_rescaler", "rescale_wrt_firstimage", "histogram_equalizer", "identity_rescaler",
           "CLAHE_rescaler", "load_rescaler", "perform_rescaling_listcam", "perform_rescaling", "compute_min_vals", "compute_max_vals",
           "channel_minmax"]
