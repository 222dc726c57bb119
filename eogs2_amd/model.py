"""`GaussianModel` over this package: the class of the reference's scene/gaussian_model.py with its attribute and method
names, so that `from eogs2_amd.model import GaussianModel` in place of `from scene import GaussianModel` is the one line an
integrator changes. C-ABI: include/eogs_model.h.

* `create_from_pcd` (gaussian_model.py:159-221): `knn.distCUDA2`, then every tensor of the model in ONE launch
  (`init_tensors`, eogs_model_init); the opacity logit is formed as the reference forms it, on a one-element fp32 tensor.
* `training_setup` (:223-271): the six groups over `optim.FusedAdam(lr=0.0, eps=1e-15)`; `capturable=True` keeps step
  counts and learning rates on the device (a recorded step).
* `prune_points`, `add_densification_stats`, `densify_and_prune`, `densify_and_clone`, `densify_and_split`, `reset_opacity`,
  `replace_tensor_to_optimizer`, `cat_tensors_to_optimizer`: composition of `optim`, `density` and `reset`.
* `save_ply` / `load_ply` (:310-346, :354-449): one pack launch (`pack_rows`, eogs_model_rows_pack), one copy of the block
  into pinned host memory, one write; and the way back (`unpack_rows`). The header is written and parsed here
  (`ply_header`, `parse_ply_header`): a `binary_little_endian 1.0` PLY, one `vertex` element, `property float <name>` lines.
* `capture` / `restore` (:73-107): the reference's 12-tuple; the optimizer entry is `FusedAdam.state_dict()`.

Deviations, on purpose: numpy arrays are uploaded, tensors must already live on the GPU (no CPU fallback);
`reset_opacity` is in place by default (`in_place=False` is the reference's replacement); `densify_and_prune` is the one
pass of `density` and does not call `torch.cuda.empty_cache()`; `only_densify` raises the TypeError the reference's own
call raises; `training_setup` without `_exposure` (a model that came from `load_ply` or `restore`) builds no exposure
optimizer where the reference fails, and `replace_tensor_to_optimizer` takes a group without state; `load_ply` needs a first
element called `vertex` with float32 properties, three `scale_*` and four `rot_*` among them; the page-locked buffer of
`save_ply` / `load_ply` is one per process, kept up to PINNED_KEEP_BYTES, calls take turns on it.
"""
import json
import os
import re
import sys
import threading

import numpy as np
import torch
from torch import nn

from . import _lib
from . import density as _density
from . import optim as _optim
from . import reset as _reset
from ._abi import MODEL_MAX_REST
from ._host import Ctx, ptr

C0 = 0.28209479177387814  # utils/sh_utils.py
GROUPS = _optim.GROUPS
PARAM_ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
               "rotation": "_rotation"}  # optimizer group -> attribute
PLY_FLOAT_TYPES = ("float", "float32")
MAX_HEADER_BYTES = 1 << 24  # a PLY header longer than this is not looked through
# The host side of save_ply / load_ply: ONE page-locked buffer per process, grown when a model is larger, so that repeated
# saves pay no page-locking. It is kept only up to PINNED_KEEP_BYTES (a larger one is released when its call ends), and
# `_pinned_lock` makes save_ply / load_ply calls of several threads take turns on it.
_pinned = {}
_pinned_lock = threading.RLock()
PINNED_KEEP_BYTES = 256 << 20


def inverse_sigmoid(x):
    """utils/general_utils.py inverse_sigmoid"""
    return torch.log(x / (1 - x))


def RGB2SH(rgb):
    """utils/sh_utils.py RGB2SH"""
    return (rgb - 0.5) / C0


def n_rest_of(sh_degree):
    n = (int(sh_degree) + 1) ** 2 - 1
    if sh_degree < 0 or n > MODEL_MAX_REST:
        raise ValueError(f"sh_degree {sh_degree}: 0 .. 3")
    return n


def row_cols(n_rest):
    """EOGS_MODEL_ROW_COLS: floats per row of the packed block."""
    return 17 + 3 * n_rest


def attribute_names(n_rest):
    """construct_list_of_attributes (gaussian_model.py:296-308): the block's column names, in order."""
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(3 * n_rest)]
            + ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])


def opacity_logit(opacity_init_value=0.01):
    """inverse_sigmoid(opacity_init_value * ones) of gaussian_model.py:198-203 on a one-element CPU fp32 tensor: a Python
    float that holds the fp32 value every row gets."""
    return float(inverse_sigmoid(opacity_init_value * torch.ones((1, 1), dtype=torch.float)))


# ---- argument checks ----
def _need_gpu(dev, who):
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: tensors on '{dev.type}'; the HIP library works on device memory and there is no CPU fallback")


def _check(t, what, shape, dev=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be float32, not {t.dtype}")
    if t.ndim != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise RuntimeError(f"{what} must have shape {tuple('*' if s is None else s for s in shape)}, not {tuple(t.shape)}")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"{what} is on {t.device}, expected {dev}: all tensors of a call live on one device")
    return t.detach().contiguous()


def _six(xyz, f_dc, f_rest, opacity, scaling, rotation, who):
    xyz = _check(xyz, f"{who}: xyz", (None, 3))
    P, dev = xyz.shape[0], xyz.device
    f_rest = _check(f_rest, f"{who}: f_rest", (P, None, 3), dev)
    n_rest = f_rest.shape[1]
    if n_rest not in (0, 3, 8, 15):
        raise RuntimeError(f"{who}: f_rest of {tuple(f_rest.shape)}: (sh_degree + 1)^2 - 1 = 0, 3, 8 or 15 rows per Gaussian")
    return (P, dev, n_rest, xyz, _check(f_dc, f"{who}: f_dc", (P, 1, 3), dev), f_rest, _check(opacity, f"{who}: opacity", (P, 1), dev),
            _check(scaling, f"{who}: scaling", (P, 3), dev), _check(rotation, f"{who}: rotation", (P, 4), dev))


# ---- the three launches ----
def init_tensors(points, colors, dist2, sh_degree, opacity_init_value=0.01):
    """The tensors `create_from_pcd` makes, in one launch: {"xyz" [P,3], "f_dc" [P,1,3], "f_rest" [P,n_rest,3],
    "scaling" [P,3], "rotation" [P,4], "opacity" [P,1], "max_radii2D" [P]} from points f32[P,3], colors f32[P,3] and dist2
    f32[P] (what `distCUDA2` returned, not yet clamped) on one GPU."""
    n_rest = n_rest_of(sh_degree)
    points = _check(points, "init_tensors: points", (None, 3))
    P, dev = points.shape[0], points.device
    colors = _check(colors, "init_tensors: colors", (P, 3), dev)
    dist2 = _check(dist2, "init_tensors: dist2", (P,), dev)
    _need_gpu(dev, "init_tensors")
    logit = opacity_logit(opacity_init_value)
    abi = _lib.get()
    with Ctx(abi, dev) as cx, torch.no_grad():
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        out = {"xyz": new(P, 3), "f_dc": new(P, 1, 3), "f_rest": new(P, n_rest, 3), "scaling": new(P, 3), "rotation": new(P, 4),
               "opacity": new(P, 1), "max_radii2D": new(P)}
        ptr0 = lambda t: ptr(t) if t.numel() else None  # noqa: E731
        abi.check(abi.model_init(P, n_rest, ptr0(points), ptr0(colors), ptr0(dist2), logit, *(ptr0(out[k]) for k in
                                 ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity", "max_radii2D")), cx.stream))
    return out


def pack_rows(xyz, f_dc, f_rest, opacity, scaling, rotation, out=None):
    """The vertex payload of `save_ply` (gaussian_model.py:313-342) as one f32 [P, 17 + 3 n_rest] device tensor, in one
    launch: x y z, three zero normals, f_dc and f_rest channel-major, opacity, scale, rot. `out`: a tensor to write into."""
    P, dev, n_rest, *six = _six(xyz, f_dc, f_rest, opacity, scaling, rotation, "pack_rows")
    if out is not None:
        if _check(out, "pack_rows: out", (P, row_cols(n_rest)), dev).data_ptr() != out.data_ptr() or not out.is_contiguous():
            raise RuntimeError("pack_rows: out must be contiguous")
    _need_gpu(dev, "pack_rows")
    abi = _lib.get()
    with Ctx(abi, dev) as cx, torch.no_grad():
        rows = out if out is not None else torch.empty((P, row_cols(n_rest)), dtype=torch.float32, device=dev)
        ptr0 = lambda t: ptr(t) if t.numel() else None  # noqa: E731
        abi.check(abi.model_rows_pack(P, n_rest, *(ptr0(t) for t in six), ptr0(rows), cx.stream))
    return rows


def unpack_rows(rows, n_rest):
    """The way back: (xyz, f_dc, f_rest, opacity, scaling, rotation) from a block of `pack_rows`; the normals are skipped."""
    if n_rest not in (0, 3, 8, 15):
        raise RuntimeError(f"unpack_rows: n_rest {n_rest}: (sh_degree + 1)^2 - 1 = 0, 3, 8 or 15")
    rows = _check(rows, "unpack_rows: rows", (None, row_cols(n_rest)))
    P, dev = rows.shape[0], rows.device
    _need_gpu(dev, "unpack_rows")
    abi = _lib.get()
    with Ctx(abi, dev) as cx, torch.no_grad():
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        six = (new(P, 3), new(P, 1, 3), new(P, n_rest, 3), new(P, 1), new(P, 3), new(P, 4))
        ptr0 = lambda t: ptr(t) if t.numel() else None  # noqa: E731
        abi.check(abi.model_rows_unpack(P, n_rest, ptr0(rows), *(ptr0(t) for t in six), cx.stream))
    return six


# ---- the PLY header ----
def ply_header(names, count):
    """The header of a `binary_little_endian 1.0` PLY with one `vertex` element of `count` rows of float properties."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(count)}"]
    lines += [f"property float {n}" for n in names] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def parse_ply_header(data):
    """(property names of the `vertex` element, its row count, byte offset of its payload) from the first bytes of a PLY file.
    Raises ValueError for anything but a little-endian binary file whose first element is `vertex` with float32 scalar
    properties only (elements after it are not read)."""
    end = re.search(rb"(^|\n)end_header\r?\n", data)
    if end is None or not data.startswith(b"ply"):
        raise ValueError("not a PLY file: no `ply` ... `end_header` header")
    lines = [ln.strip() for ln in data[:end.start() + 1].decode("ascii", errors="replace").splitlines()]
    if lines[0] != "ply":
        raise ValueError("not a PLY file: the first line is not `ply`")
    fmt, elements = None, []
    for ln in lines[1:]:
        w = ln.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1:]
        elif w[0] == "element" and len(w) == 3:
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements:
            elements[-1][2].append(w[1:])
        else:
            raise ValueError(f"PLY header: cannot read the line {ln!r}")
    if fmt != ["binary_little_endian", "1.0"]:
        raise ValueError(f"PLY format {' '.join(fmt or ['(none)'])}: only binary_little_endian 1.0 is read")
    if not elements:
        raise ValueError("PLY header: no element")
    name, count, props = elements[0]
    if name != "vertex":
        raise ValueError(f"PLY file whose first element is {name!r}: the Gaussians are the rows of a first element `vertex`")
    for p in props:
        if len(p) != 2 or p[0] not in PLY_FLOAT_TYPES:
            raise ValueError(f"PLY element {name!r}: property {' '.join(p)!r}: only float32 scalar properties are read")
    names = [p[1] for p in props]
    if len(set(names)) != len(names):
        raise ValueError(f"PLY element {name!r}: a property name appears twice")
    if count < 0:
        raise ValueError(f"PLY element {name!r}: {count} rows")
    return names, count, end.end()


def ply_columns(names, sh_degree):
    """For every column of the canonical block (attribute_names) the file column that holds it, -1 for a normal the file does
    not carry: the reference's mapping BY NAME (gaussian_model.py:374-420), `f_rest_*`, `scale_*` and `rot*` sorted by their
    numeric suffix, with its assertion on the number of `f_rest_*` columns."""
    at = {n: i for i, n in enumerate(names)}
    for need in ("x", "y", "z", "opacity", "f_dc_0", "f_dc_1", "f_dc_2"):
        if need not in at:
            raise KeyError(f"PLY file without the property {need!r}")
    def family(prefix):  # the properties that start with `prefix`, by the number after their last underscore
        return sorted((n for n in names if n.startswith(prefix)), key=lambda n: int(n.rsplit("_", 1)[1]))

    rest, scales, rots = family("f_rest_"), family("scale_"), family("rot")
    assert len(rest) == 3 * (sh_degree + 1) ** 2 - 3
    if len(scales) != 3 or len(rots) != 4:
        raise ValueError(f"PLY file with {len(scales)} scale_* and {len(rots)} rot* properties: 3 and 4 are needed")
    order = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", *rest, "opacity", *scales, *rots]
    return [at.get(n, -1) for n in order]


def _read_exposures(json_path, dev):
    """{image name: f32 device tensor} from the `exposure.json` two directories above a point cloud, None without the file."""
    if not os.path.isfile(json_path):
        print(f"No exposure to be loaded at {json_path}")
        return None
    with open(json_path) as f:
        table = json.load(f)
    print("Pretrained exposures loaded.")
    return {name: torch.tensor(rows, dtype=torch.float32, device=dev) for name, rows in table.items()}


def _release_large_host_rows():
    buf = _pinned.get("rows")
    if buf is not None and buf.numel() * 4 > PINNED_KEEP_BYTES:
        del _pinned["rows"]


def _host_rows(P, C):
    """A page-locked f32 [P, C] view: one buffer per process, grown on demand (call under `_pinned_lock`)."""
    need = max(P * C, 1)
    buf = _pinned.get("rows")
    if buf is None or buf.numel() < need:
        buf = _pinned["rows"] = torch.empty((need,), dtype=torch.float32, pin_memory=True)
    return buf[:P * C].view(P, C)


def covariance_upper(scaling, rotation):
    """The six distinct entries (xx, xy, xz, yy, yz, zz) of R S S R^T per Gaussian, R from the raw quaternion (normalised by
    `optim.build_rotation`), S = diag(scaling): what the reference's covariance_activation hands the rasterizer."""
    M = _optim.build_rotation(rotation) * scaling[:, None, :]  # R S: column k of R times s_k
    cov = M @ M.transpose(1, 2)
    i, j = torch.triu_indices(3, 3, device=cov.device)
    return cov[:, i, j]


class GaussianModel:
    def setup_functions(self):
        """The activations, under the reference's attribute names (callers read them: `scaling_inverse_activation` ...)."""
        self.scaling_activation, self.scaling_inverse_activation = torch.exp, torch.log
        self.opacity_activation, self.inverse_opacity_activation = torch.sigmoid, inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize
        self.covariance_activation = lambda scaling, scaling_modifier, rotation: covariance_upper(scaling_modifier * scaling, rotation)

    def __init__(self, sh_degree, optimizer_type="default"):
        self.max_sh_degree, self.active_sh_degree, self.optimizer_type = sh_degree, 0, optimizer_type
        for name in tuple(PARAM_ATTRS.values()) + _density.STATS:  # empty until create_from_pcd / load_ply / restore
            setattr(self, name, torch.empty(0))
        self.optimizer, self.percent_dense, self.spatial_lr_scale = None, 0, 0
        self.setup_functions()

    # ---- checkpoints ----
    def capture(self):
        """The reference's 12-tuple, in its order (a checkpoint written there is read here and the other way round)."""
        par = [getattr(self, PARAM_ATTRS[n]) for n in ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")]
        return (self.active_sh_degree, *par, self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(),
                self.spatial_lr_scale)

    def restore(self, model_args, training_args, capturable=None):
        """gaussian_model.py:89-107. `capturable=None`: as the captured optimizer was (a tuple from the reference's
        `torch.optim.Adam` restores into the host-stepped FusedAdam). Step counts come back where this optimizer keeps them:
        device fp32 scalars when capturable, host scalars otherwise; the learning-rate tensors are uploaded at the next step."""
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity,
         self.max_radii2D, xyz_gradient_accum, denom, opt_dict, self.spatial_lr_scale) = model_args
        if capturable is None:
            capturable = any(bool(g.get("capturable")) for g in opt_dict["param_groups"])
        self.training_setup(training_args, capturable=capturable)
        self.xyz_gradient_accum = xyz_gradient_accum
        self.denom = denom
        self.optimizer.load_state_dict(opt_dict)
        for group in self.optimizer.param_groups:
            group["capturable"] = bool(capturable)
            group.pop("lr_tensor", None)  # (the captured run's tensor: this optimizer uploads its own at its first step)
            group.pop("lr_uploaded", None)
            for p in group["params"]:
                st = self.optimizer.state.get(p)
                if st and "step" in st:
                    step = torch.as_tensor(st["step"], dtype=torch.float32).reshape(()).clone()  # (not the captured tuple's)
                    st["step"] = step.to(p.device) if capturable else step.cpu()

    # ---- activations ----
    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_features_dc(self):
        return self._features_dc

    @property
    def get_features_rest(self):
        return self._features_rest

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    @property
    def get_exposure(self):
        return self._exposure

    def get_exposure_from_name(self, image_name):
        loaded = self.pretrained_exposures
        return loaded[image_name] if loaded is not None else self._exposure[self.exposure_mapping[image_name]]

    def get_covariance(self, scaling_modifier=1):
        return self.covariance_activation(self.get_scaling, scaling_modifier, self._rotation)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            print("Increase SH degree to ", self.active_sh_degree + 1)
            self.active_sh_degree += 1

    # ---- creation ----
    def _adopt(self, t):
        self._xyz, self._features_dc, self._features_rest = t["xyz"], t["f_dc"], t["f_rest"]
        self._opacity, self._scaling, self._rotation = t["opacity"], t["scaling"], t["rotation"]

    def create_from_pcd(self, pcd, cam_infos, spatial_lr_scale, opacity_init_value=0.01, dist2=None):
        """gaussian_model.py:159-221. `pcd.points` / `pcd.colors`: numpy arrays (uploaded to the current GPU, as the reference
        does) or float tensors on a GPU. `dist2`: the f32[P] result of `distCUDA2` on the same device when the caller already
        has it; else `knn.distCUDA2` runs first."""
        self.spatial_lr_scale = spatial_lr_scale

        def on_gpu(a, what):
            if isinstance(a, torch.Tensor):
                _need_gpu(a.device, f"create_from_pcd: {what}")
                return a.detach().float().contiguous()
            if not torch.cuda.is_available():
                raise RuntimeError("create_from_pcd: no GPU; the HIP library works on device memory and there is no CPU fallback")
            return torch.as_tensor(np.asarray(a)).to(device="cuda", dtype=torch.float32)

        points, colors = on_gpu(pcd.points, "pcd.points"), on_gpu(pcd.colors, "pcd.colors")
        print("Number of points at initialisation : ", points.shape[0])
        if dist2 is None:
            from .knn import distCUDA2

            dist2 = distCUDA2(points)
        elif not isinstance(dist2, torch.Tensor):
            raise TypeError("create_from_pcd: dist2 must be a torch.Tensor on the GPU")
        t = init_tensors(points, colors, dist2, self.max_sh_degree, opacity_init_value)
        self._adopt({n: nn.Parameter(t[n].requires_grad_(True)) for n in GROUPS})
        self.max_radii2D = t["max_radii2D"]
        # one 3 x 4 exposure matrix per camera, identity at the start, found by image name (gaussian_model.py:216-221)
        image_names = [cam.image_name for cam in cam_infos]
        self.exposure_mapping = {name: k for k, name in enumerate(image_names)}
        self.pretrained_exposures = None
        self._exposure = nn.Parameter(torch.eye(3, 4, device=points.device).expand(len(image_names), 3, 4).clone())

    def training_setup(self, training_args, capturable=False):
        if self.optimizer_type not in ("default", "sparse_adam"):
            raise ValueError(f"Unknown optimizer, got:{self.optimizer_type}")
        dev = self._xyz.device
        _need_gpu(dev, "training_setup")
        self.percent_dense = training_args.percent_dense
        self.xyz_gradient_accum = torch.zeros((self.get_xyz.shape[0], 1), device=dev)
        self.denom = torch.zeros((self.get_xyz.shape[0], 1), device=dev)

        l = [
            {"params": [self._xyz], "lr": training_args.position_lr_init * self.spatial_lr_scale, "name": "xyz"},
            {"params": [self._features_dc], "lr": training_args.feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": training_args.feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": training_args.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": training_args.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": training_args.rotation_lr, "name": "rotation"},
        ]
        # "sparse_adam": SparseGaussianAdam is not in the reference's tree; its `except` branch builds the dense optimizer
        self.optimizer = _optim.FusedAdam(l, lr=0.0, eps=1e-15, capturable=bool(capturable))
        exposure = getattr(self, "_exposure", None)
        self.exposure_optimizer = torch.optim.Adam([exposure]) if exposure is not None else None

    def update_learning_rate(self, iteration):
        return

    def construct_list_of_attributes(self):
        return attribute_names(self._features_rest.shape[1])

    # ---- files ----
    def save_ply(self, path):
        """gaussian_model.py:310-346 as one pack launch, one device-to-host copy into page-locked memory and one write."""
        if sys.byteorder != "little":
            raise RuntimeError("save_ply writes the host's float32 bytes into a binary_little_endian file")
        rows = pack_rows(self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation)
        header = ply_header(self.construct_list_of_attributes(), rows.shape[0])
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        with _pinned_lock:
            try:
                host = _host_rows(*rows.shape)
                host.copy_(rows)  # (a copy into page-locked memory returns once the bytes are there)
                torch.cuda.current_stream(rows.device).synchronize()
                with open(path, "wb") as f:
                    f.write(header)
                    f.write(host.numpy())  # (the buffer itself: no copy)
            finally:
                _release_large_host_rows()

    def load_ply(self, path, use_train_test_exp=False, device=None):
        """gaussian_model.py:354-449. The properties are found by name; a file in the canonical column order goes up as it is
        (one read into page-locked memory, one copy, one unpack launch), any other order is permuted on the host first."""
        if sys.byteorder != "little":
            raise RuntimeError("load_ply reads a binary_little_endian file as the host's float32 bytes")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() else torch.device(device or "cpu")
        _need_gpu(dev, "load_ply")
        if use_train_test_exp:
            self.pretrained_exposures = _read_exposures(os.path.join(os.path.dirname(path), "..", "..", "exposure.json"), dev)
        n_rest = n_rest_of(self.max_sh_degree)
        C = row_cols(n_rest)
        with _pinned_lock, open(path, "rb") as f:
            head = f.read(1 << 12)
            while b"end_header" not in head and len(head) < MAX_HEADER_BYTES:  # (a header with long comments: read on)
                more = f.read(len(head))
                if not more:
                    break
                head += more
            names, P, offset = parse_ply_header(head)
            cols = ply_columns(names, self.max_sh_degree)
            f.seek(0, os.SEEK_END)
            if f.tell() - offset < P * len(names) * 4:
                raise ValueError(f"{path}: {f.tell() - offset} bytes after the header, {P} rows of {len(names)} floats need {P * len(names) * 4}")
            f.seek(offset)
            host, dst, raw = _host_rows(P, C), None, None
            if cols == list(range(C)) and len(names) == C:
                if f.readinto(host.numpy()) != P * C * 4:
                    raise ValueError(f"{path}: short read")
            else:
                raw = np.fromfile(f, dtype="<f4", count=P * len(names)).reshape(P, len(names))
                dst = host.numpy()
                have = [j for j, c in enumerate(cols) if c >= 0]
                dst[:] = 0.0
                dst[:, have] = raw[:, [cols[j] for j in have]]
            rows = torch.empty((P, C), dtype=torch.float32, device=dev)
            rows.copy_(host)
            torch.cuda.current_stream(dev).synchronize()  # the page-locked buffer is reused by the next call
            del host, dst, raw
            _release_large_host_rows()
        six = unpack_rows(rows, n_rest)
        self._adopt({n: nn.Parameter(t.requires_grad_(True)) for n, t in zip(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), six)})
        self.active_sh_degree = self.max_sh_degree

    # ---- optimizer surgery ----
    def reset_opacity(self, in_place=True):
        """gaussian_model.py:347-352. in_place=True (`reset.reset_opacity_`): the logits are capped and the group's moments
        cleared in one launch, no tensor is replaced and a recorded step keeps replaying. in_place=False: the reference's
        replacement, a new Parameter under `_opacity`."""
        _need_gpu(self._opacity.device, "reset_opacity")
        if in_place:
            _reset.reset_opacity_(self.optimizer)
        else:
            self._opacity = _optim.reset_opacity(self.optimizer)["opacity"]

    def replace_tensor_to_optimizer(self, tensor, name):
        """gaussian_model.py:451-464 over `optim.replace_tensor`; a group that has not stepped yet (no state) is replaced too,
        where the reference fails on its missing state."""
        return _optim.replace_tensor(self.optimizer, tensor, name)

    def _stats(self):
        return (self.xyz_gradient_accum, self.denom, self.max_radii2D)

    def _prune_optimizer(self, mask):
        return _optim.prune_optimizer(self.optimizer, mask)[0]

    def prune_points(self, mask):
        _need_gpu(mask.device, "prune_points")
        valid_points_mask = ~mask
        t, (self.xyz_gradient_accum, self.denom, self.max_radii2D) = _optim.prune_optimizer(self.optimizer, valid_points_mask,
                                                                                            extra=self._stats())
        self._adopt(t)
        return valid_points_mask

    def cat_tensors_to_optimizer(self, tensors_dict):
        return _optim.cat_tensors_to_optimizer(self.optimizer, tensors_dict)

    def _zero_stats(self):
        P, dev = self.get_xyz.shape[0], self.get_xyz.device
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)
        self.max_radii2D = torch.zeros((P), device=dev)

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling, new_rotation, new_tmp_radii):
        d = {"xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest, "opacity": new_opacities, "scaling": new_scaling,
             "rotation": new_rotation}
        self._adopt(self.cat_tensors_to_optimizer(d))
        self.tmp_radii = torch.cat((self.tmp_radii, new_tmp_radii))
        self._zero_stats()

    def densify_and_split(self, grads, grad_threshold, screen_size_threshold, scene_extent, N=2):
        """gaussian_model.py:573-623 over `optim.densify_and_split`: the reference's selection (mean gradient at or above the
        threshold, largest scale above percent_dense x extent), its `torch.normal` draw, one compaction for the selection and
        one for the prune of the originals."""
        g = grads.reshape(-1)
        hot = torch.cat((g, g.new_zeros(self._xyz.shape[0] - g.numel()))) >= grad_threshold  # rows appended since count as 0
        selected_pts_mask = hot & (self.get_scaling.amax(dim=1) > self.percent_dense * scene_extent)
        t, self.tmp_radii, _ = _optim.densify_and_split(self.optimizer, selected_pts_mask, N=N, tmp_radii=self.tmp_radii)
        self._adopt(t)
        self._zero_stats()

    def densify_and_clone(self, grads, grad_threshold, screen_size_threshold, scene_extent):
        """gaussian_model.py:625-659 over `optim.densify_and_clone`."""
        selected_pts_mask = (grads.norm(dim=-1) >= grad_threshold) & (self.get_scaling.amax(dim=1) <= self.percent_dense * scene_extent)
        t, self.tmp_radii = _optim.densify_and_clone(self.optimizer, selected_pts_mask, tmp_radii=self.tmp_radii)
        self._adopt(t)
        self._zero_stats()

    def only_densify(self, grad_threshold, min_opacity, screen_size_threshold, max_screen_size, radii):
        """gaussian_model.py:661-683 calls `densify_and_split` without its `scene_extent`: in the reference this method
        cannot run, and it does not run here."""
        raise TypeError("GaussianModel.densify_and_split() missing 1 required positional argument: 'scene_extent'")

    def densify_and_prune(self, grad_threshold, min_opacity, screen_size_threshold, max_screen_size, radii, scene_extent):
        """gaussian_model.py:685-717 in the one pass of `density.densify_and_prune`: one decision launch, the reference's
        `torch.normal` draw, one build launch, one host wait. Returns the pass's `DensifyInfo`."""
        _need_gpu(self._xyz.device, "densify_and_prune")
        t, stats, info = _density.densify_and_prune(
            self.optimizer, self._stats(), grad_threshold, min_opacity=min_opacity, screen_size_threshold=screen_size_threshold,
            max_screen_size=max_screen_size, scene_extent=scene_extent, percent_dense=self.percent_dense, N=2, radii=radii)
        self._adopt(t)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = stats.tensors()
        self.tmp_radii = None
        return info

    def add_densification_stats(self, viewspace_point_tensor, update_filter, radii=None):
        """gaussian_model.py:719-723 in one launch (`density.add_densification_stats`), no `nonzero`, no wait. `update_filter`:
        the boolean mask [P] or the index tensor the renderer returns. With `radii` (the render's, int32 or float32 [P]) the
        launch also does train_pan.py:683-686, `max_radii2D = max(max_radii2D, radii)` on the rows with `radii > 0`, and
        `update_filter` is not read: those rows are the filter."""
        grad = viewspace_point_tensor.grad
        if radii is not None:
            _density.add_densification_stats(self.xyz_gradient_accum, self.denom, self.max_radii2D, grad, radii)
            return
        P, dev = self.max_radii2D.shape[0], self.max_radii2D.device
        if update_filter.dtype == torch.bool:
            on = update_filter.to(torch.float32)
        else:
            on = torch.zeros((P,), dtype=torch.float32, device=dev)
            on[update_filter] = 1.0
        _density.add_densification_stats(self.xyz_gradient_accum, self.denom, torch.zeros_like(self.max_radii2D), grad, on)


__all__ = ["GaussianModel", "init_tensors", "pack_rows", "unpack_rows", "ply_header", "parse_ply_header", "ply_columns",
           "attribute_names", "row_cols", "n_rest_of", "opacity_logit", "inverse_sigmoid", "RGB2SH", "GROUPS"]
