"""eogs2_amd — MI355X-native differentiable Gaussian-splatting rasterizer for EOGS++.

Drop-in for the hot path of gardiens/EOGS2: the `diff_gaussian_rasterization`
Python API (see `rasterizer.py`) over a C-ABI HIP library (`csrc/`, `include/eogs_rast.h`).
"""
from .rasterizer import (  # noqa: F401
    GaussianRasterizationSettings,
    GaussianRasterizer,
    rasterize_gaussians,
    RastError,
    NUM_CHANNELS,
)

from . import density  # noqa: F401,E402  (densification statistics and one-pass densify_and_prune: gaussian_model.py:685-723)
from . import dsm_eval  # noqa: F401,E402  (DSM registration and MAE: eval/dsmr.py, eval/eval_dsm.py)
from . import dsm_raster  # noqa: F401,E402  (cloud / view / TSDF surface -> DSM: utils/dsm_utils.py, tsdf.py:530-600)
from . import flow  # noqa: F401,E402  (flow-matching warp, statistics and criteria: flowmatching/flow_matching.py)
from . import mesh  # noqa: F401,E402  (marching cubes over the TSDF volume: tsdf.py:522-528 without mcubes)
from . import model  # noqa: F401,E402  (GaussianModel: create_from_pcd, training_setup, PLY and checkpoints: scene/gaussian_model.py)
from . import monitor  # noqa: F401,E402  (training monitor: interval means, PSNR/SSIM, early stopper: train_pan.py:423-597)
from . import pansharp  # noqa: F401,E402  (pansharpened PAN target, Lpan, Lgradient_pan, Pansharploss: pansharpening/, loss/PAN_loss.py)
from . import regularizers  # noqa: F401,E402  (opacity, effective-rank, TV and accumulated-opacity terms: loss/opacity.py, main_loss.py)
from . import rescaler  # noqa: F401,E402  (ground-truth rescalers: utils/rescaler/rescaler.py)
from . import reset  # noqa: F401,E402  (shadow-based colour reset, in-place opacity reset, render_all_views: color_reset_op.py)
from . import views  # noqa: F401,E402  (several views in one recorded step: device-side view bank, train_pan.py:135-138,252-257)
from . import draw  # noqa: F401,E402  (per-iteration random background and virtual camera on the device: train_pan.py:272-277,375-378)
from . import randomcam  # noqa: F401,E402  (RandomcamRendering_Loss in full: shadow-mapped render type, GT target: loss/main_loss.py:56-221)
from . import report  # noqa: F401,E402  (training_report's metrics, colour alignment before save_ply, cc train -> test, product packing: train_pan.py:838-1025, utils/save_utils.py)
from . import raft  # noqa: F401,E402  (the flow network, RAFT, with on-demand correlation lookup: flowmatching/flow_matching.py:76-86)
from . import uncertainty  # noqa: F401,E402  (transient-mask Gaussian NLL term and its statistics: train_pan.py:433-449)

__version__ = "0.1.0"
