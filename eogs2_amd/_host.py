"""What every module of the package needs to reach the library: pointers, the two ways to launch, size queries, the
device and dtype checks, cached workspaces. Modules import their plumbing from here and nowhere else.

Two calling conventions, with different host cost; which one a path uses is part of its measured speed:

* `Ctx` for a block that allocates under the device guard, or that may run over the CPU-oracle library.
* `call` for a single launch on a launch-floor path over the HIP library.
"""
import ctypes

import torch

from . import _lib


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Ctx:
    """device guard + stream for one call"""

    def __init__(self, abi, dev):
        self.abi = abi
        if dev.type != abi.device_type:
            raise RuntimeError(
                f"rasterizer tensors live on '{dev.type}' but the loaded library ({abi.backend}) works on "
                f"'{abi.device_type}' memory; there is no CPU fallback"
            )
        self.dev = dev
        self.guard = torch.cuda.device(dev) if dev.type == "cuda" else None

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()
            self.stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        else:
            self.stream = None
        return self

    def __exit__(self, *a):
        if self.guard is not None:
            self.guard.__exit__(*a)


# The calls sit at the launch floor (the kernels take a few microseconds), so the path of a launch through `call` is kept
# short: entry points resolved once, raw pointers, the current stream's handle without a Stream object, and a device guard
# only when the tensors' device is not the current one.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_entry = {}


def call(name, dev, *args):
    """One launch entry of the library on `dev`'s current stream (appended as the last argument)."""
    fn = _entry.get(name)
    if fn is None:
        fn = _entry[name] = getattr(_lib.get().cdll, name)
    idx = dev.index
    if idx is not None and idx != torch.cuda.current_device():
        with torch.cuda.device(idx):
            return call(name, torch.device("cuda"), *args)
    if idx is None:
        idx = torch.cuda.current_device()
    stream = _raw_stream(idx) if _raw_stream is not None else torch.cuda.current_stream(idx).cuda_stream
    rc = fn(*args, stream)
    if rc:
        _lib.get().check(rc)


def query_bytes(abi, query, *args):
    """A size query of the library, `abi.<query>(*args, &size)`, as an int."""
    n = ctypes.c_size_t()
    abi.check(getattr(abi, query)(*args, ctypes.byref(n)))
    return n.value


_sizes = {}


def nbytes(abi, query, *args):
    """`query_bytes`, asked once per (library, query, args): for sizes whose arguments recur (an image shape, a channel
    count), not for those that follow the scene (the rasterizer's)."""
    key = (abi, query, args)
    n = _sizes.get(key)
    if n is None:
        n = _sizes[key] = query_bytes(abi, query, *args)
    return n


def on_device(module, subject, t, what, non_tensor=None):
    """Refuses a tensor that is not on the GPU, in the words of `module` ("flow") about `subject` ("the flow warp runs");
    bound once per module with functools.partial. `non_tensor` ("not" or "got", the word of the module's message): what is
    not a tensor is refused too."""
    if non_tensor is not None and not torch.is_tensor(t):
        raise TypeError(f"{module} {what}: expected a tensor, {non_tensor} {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{module} {what}: tensors live on '{t.device.type}'; {subject} on the GPU only, there is no CPU fallback")


def f32c(t, dev, label):
    """`t` detached as contiguous fp32, refused under the caller's `label` ("loss input") if it is not on `dev`."""
    if t.device != dev:
        raise RuntimeError(f"{label} on {t.device}, expected {dev}")
    return t.detach().to(torch.float32).contiguous()


class Workspaces(dict):
    """One set of buffers per (device, stream, call shape), reused by later calls; clear() drops them all."""

    def of(self, key, dev, make):
        key = (dev, torch.cuda.current_stream(dev).cuda_stream) + key
        if key not in self:
            self[key] = make()
        return self[key]

    @staticmethod
    def bytes(dev, n):
        return torch.empty(max(int(n), 1), dtype=torch.uint8, device=dev)
