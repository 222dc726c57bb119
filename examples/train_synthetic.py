"""End-to-end use of the MI355X path on synthetic data: the structure of one EOGS++ training iteration
(src/gaussiansplatting/train_pan.py:262-400,663-690) with every heavy step on the HIP library.

    python examples/train_synthetic.py [--gaussians 200000] [--size 512] [--iters 200]

Per iteration: render the view through `eogs2_amd.render.render` (raw-parameter front end, §8 f1), render a sun-like
virtual camera at twice the resolution and resample it onto the view (`eogs2_amd.resample`, §8 f2), run the camera's
render pipeline — learnable colour correction, shadow map from the altitude difference, in-shadow tint
(`eogs2_amd.shade.render_pipeline`, §8 f2) —, photometric loss against a target image
(`eogs2_amd.losses.photometric_loss`) plus the sun-camera consistency pair and the translucent-shadow regulariser
(`eogs2_amd.shade.suncamera_l`, `translucentshadows_l`), `FusedAdam` step on the Gaussians and Adam on the camera
parameters (§8 f3), transparent-Gaussian prune by stream compaction (`prune_optimizer`, §8 f3). The target is the shaded
render of the unperturbed scene under an identity colour correction, so the loss must fall. Initial scales come from
`simple_knn._C.distCUDA2` (§8 f4). `--flow-matching` adds the reference's flow-matching step between the render pipeline and
the photometric loss (`eogs2_amd.flow`), against a target displaced by a sub-pixel registration error. `--opacity-loss W` and
`--erank-loss W` add the reference's OpacityLoss (W = 0.1 in its shipped configuration) and erankLoss over the raw parameters
(`eogs2_amd.regularizers`). `--pan-map NAME` makes the camera a panchromatic one: its render pipeline ends in the MSI->PAN map NAME
(`eogs2_amd.pan.render_pipeline`, the reference's `PANAffineCamera`), the target goes through the same map and the photometric
loss runs on the one PAN plane; `--pan-first` is the reference's `weird_pan_setup` (map first, then a 1->1 colour correction).
`--densify-every K` is the reference's `only_prune: False` (train_pan.py:679-711): the densification statistics every iteration
(`eogs2_amd.density.DensityStats.update`, one launch, no wait) and `densify_and_prune` plus the transparent prune every K iterations.
`--monitor` keeps the reference's training metrics and early stopper on the device (`eogs2_amd.monitor.TrainingMonitor`;
train_pan.py:423-429,471-495,512-597): every iteration feeds it without a wait, every 10 iterations one record is fetched and printed.
`--dsm-mae-every N` scores the view's altitude against the unperturbed scene's (`eogs2_amd.dsm_eval.dsm_mae`); with `--dsm-resolution R`
both are first flattened into DSMs on the device (`eogs2_amd.dsm_raster.dsm_from_view`): render -> DSM -> registered MAE.
`--opacity-reset-every N` and `--color-reset-at N` are the two resets near the end of the reference's iteration (train_pan.py:726-736)
in place (`eogs2_amd.reset.reset_opacity_`, `color_reset`): no tensor is replaced, so a recorded step keeps replaying across them.
`--save-ply PATH` writes the trained Gaussians as the reference's `point_cloud.ply` (`eogs2_amd.model.GaussianModel.save_ply`: one pack
launch, one copy, one write); `--load-ply PATH` starts the trainee from such a file instead of the perturbed scene (`load_ply`).
`--pansharp-loss METHOD` adds 0.1 x the reference's Pansharploss (`eogs2_amd.pansharp.Pansharploss`; loss/pansharp_loss.py, w_L_pansharp):
a low-resolution MSI ground truth (the target image, averaged over 4 x 4 blocks) and a PAN ground truth are pansharpened on the fly by
METHOD (brovey, simple_brovey, ihs) inside the loss kernels, forward and backward, and compared with the rendered image.
`--views V` trains V views by the reference's protocol (train_pan.py:252-257,135-138): a view popped from a refilled stack every iteration,
every camera's parameters on their own Adam moments and step count. The views' ground truths, matrices, backgrounds, colour-camera
parameters and the camera optimizer's state sit in a device-side bank (`eogs2_amd.views.ViewBank`): one launch brings the current view
into the tensors the iteration reads, one writes the updated state back, so with `--graph --optimizer-in-graph` every replay trains
another view with no host work in between.
`--random-background` and `--virtual-camera-extent X` (with `--random-camera`) draw the background and the random virtual camera anew in
every iteration, as the reference does (train_pan.py:272-277,375-378), on the device (`eogs2_amd.draw.IterationDraws`): one launch
after `bank.load()`, keyed by `--draw-seed` and the iteration's index, so a recorded step renders against another background and
another virtual camera on every replay. Without them the background and the `rnd` camera are fixed, as before.
`--random-camera-type rawrender_wshadow` and `--random-camera-gt` (with `--random-camera`) are the reference's
`optimization.random_camera.randomcamera_render_type` and `use_gt` (`eogs2_amd.randomcam.RandomcamRendering_Loss`; loss/main_loss.py:56-221):
the virtual view goes through the view's whole render pipeline, with a shadow map of its own, before it is resampled and compared with the
shaded image, or with the ground truth. The loss takes the iteration's own sun render (`sun_render=`) instead of rendering the sun camera
a second time; `--no-share-sun-render` renders twice, as the reference does. The matrices of the shadow-mapped view are composed on the
device after `draws.draw()` (`virtual_to_sun`), so a recorded step follows the drawn camera.
`--test-views N --report-every K` hold out N synthetic views and every K iterations do what the reference's `training_report` does
(train_pan.py:838-951): the train cameras' colour correction goes to the test cameras by `--cc-to-test ref|average`
(`eogs2_amd.report.load_convert_color_correction_train_to_test`), then the test and the train views are rendered through sun resample
and render pipeline and their L1 and PSNR summed on the device (`evaluate_views`: no wait per camera, one copy per report).
`--normalize-colors` is the reference's `normalize_before_saving` before the final save (train_pan.py:614-620) in place, and
`--render-set DIR` writes `render_set`'s products of every view (render_pan.py) as DIR/<product>/<view>.npy — one packing launch and
one copy per view (`view_products`, `fetch_products`) — and render_video.py's frame `[final | elevation]` as DIR/frames/<view>.npy.
`--transient-nll W` adds the reference's transient-uncertainty term `w_L_nll * L_nll` (train_pan.py:433-449, `use_transient`) through
`eogs2_amd.uncertainty.transient_nll`: the camera owns an H x W trainable transient mask (`--transient-init V`, affine_cameras.py:282-289)
that sits in the camera optimizer — with `--views V` as a `ViewBank` state slot "transient_mask" per view, its Adam moments and step count
beside it — and the Gaussian negative log-likelihood of the shaded image under the variance (clip(mask, 0, 1) + 1e-3)^2 joins the loss.
The weight lives in a device tensor that is 0 until `--transient-from ITER` has passed (`iteration > iterstart_L_nll`) and W afterwards: a
write between two replays, so a recorded step keeps replaying across the switch. (Until then the mask receives exact zeros where the
reference's receives no gradient at all: its Adam step count runs from iteration 1 here.) A bright rectangle is painted into ONE view's
ground truth (`eogs2_amd.synthetic.paint_transient`: view 1 with `--views`, else the view) and the run prints that view's final mean mask
inside and outside of it.
"""
import argparse
import math
import os
import random
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eogs2_amd.losses import photometric_loss  # noqa: E402
from eogs2_amd.density import DensityStats, densify_and_prune  # noqa: E402
from eogs2_amd.optim import FusedAdam, alive_rows, prune_optimizer, retire_rows  # noqa: E402
from eogs2_amd.rasterizer import captured_gate  # noqa: E402
from eogs2_amd.reset import color_reset, reset_opacity_  # noqa: E402
from eogs2_amd.render import render  # noqa: E402
from eogs2_amd.graph import Branches  # noqa: E402
from eogs2_amd.resample import render_resample_virtual_camera, resample  # noqa: E402
from eogs2_amd.shade import randomcam_l, render_pipeline, suncamera_l, translucentshadows_l  # noqa: E402
from eogs2_amd.dsm_eval import dsm_mae  # noqa: E402
from eogs2_amd.dsm_raster import dsm_from_view  # noqa: E402
from eogs2_amd.flow import apply_flow, perform_flow_matching, performOpticalmatching  # noqa: E402
from eogs2_amd.regularizers import gaussian_regularizers  # noqa: E402
from eogs2_amd.model import GaussianModel, parse_ply_header  # noqa: E402
from eogs2_amd.monitor import MONITOR_METRICS, TrainingMonitor  # noqa: E402
from eogs2_amd.pansharp import METHODS as PANSHARP_METHODS, Pansharploss  # noqa: E402
from eogs2_amd.pan import FIXED_PARAMS, KINDS as PAN_KINDS, PanMap, render_pipeline as pan_render_pipeline  # noqa: E402
from eogs2_amd.synthetic import ALT_SCALE, make_camera, make_scene, paint_transient  # noqa: E402
from eogs2_amd.uncertainty import transient_nll, transient_parameters  # noqa: E402
from eogs2_amd.views import ViewBank, ViewSchedule, reference_order  # noqa: E402
from eogs2_amd.draw import DrawStream, IterationDraws  # noqa: E402
from eogs2_amd.randomcam import RENDER_TYPES, RandomcamRendering_Loss  # noqa: E402
from eogs2_amd.report import (evaluate_views, fetch_products, load_convert_color_correction_train_to_test, normalize_before_saving,  # noqa: E402
                              video_frame, view_products)
from eogs2_amd.reset import render_all_views  # noqa: E402
from simple_knn._C import distCUDA2  # noqa: E402

C0 = 0.28209479177387814
MONITOR_INTERVAL = 10  # --monitor: iterations per record (the reference's tb_log_interval)
FLOW_SHIFT = (0.6, -0.35)  # --flow-matching: the target's displacement in pixels (horizontal, vertical)


class Camera:
    """The attributes gaussian_renderer/renderer.py reads from an AffineCamera."""

    def __init__(self, vm, H, W):
        self.FoVx = self.FoVy = 1.0
        self.affine = self.world_view_transform = self.full_proj_transform = vm
        self.learn_wv_only_lastparam = False
        self.image_height, self.image_width = H, W
        self.camera_center = torch.zeros(3, device=vm.device)


class Gaussians:
    """The attributes renderer.py / gaussian_model.py use: raw parameters, one optimizer group each."""

    active_sh_degree = 0

    def __init__(self, xyz, rgb, opacity, scales, rotations, capturable=False):
        P = xyz.shape[0]
        self._xyz = torch.nn.Parameter(xyz.clone())
        self._features_dc = torch.nn.Parameter(((rgb - 0.5) / C0).reshape(P, 1, 3).contiguous())
        self._features_rest = torch.nn.Parameter(torch.zeros(P, 0, 3, device=xyz.device))
        self._opacity = torch.nn.Parameter(torch.log(opacity / (1 - opacity)))
        self._scaling = torch.nn.Parameter(torch.log(scales))
        self._rotation = torch.nn.Parameter(rotations.clone())
        lrs = dict(xyz=2e-5, f_dc=2.5e-3, f_rest=1.25e-4, opacity=2.5e-2, scaling=5e-3, rotation=1e-3)
        groups = [dict(params=[getattr(self, "_" + n)], lr=lr, name=k)
                  for k, n, lr in (("xyz", "xyz", lrs["xyz"]), ("f_dc", "features_dc", lrs["f_dc"]),
                                   ("f_rest", "features_rest", lrs["f_rest"]), ("opacity", "opacity", lrs["opacity"]),
                                   ("scaling", "scaling", lrs["scaling"]), ("rotation", "rotation", lrs["rotation"]))]
        # gaussian_model.py:262 with the fused step; capturable: step counts and learning rates on the device (--optimizer-in-graph)
        self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15, capturable=True) if capturable else FusedAdam(groups, lr=0.0, eps=1e-15)
        self.max_radii2D = torch.zeros(P, device=xyz.device)
        self.stats = None  # --densify-every: DensityStats (xyz_gradient_accum, denom and the max_radii2D above)

    get_xyz = property(lambda s: s._xyz)

    def _adopt(self, t):
        self._xyz, self._features_dc, self._features_rest = t["xyz"], t["f_dc"], t["f_rest"]
        self._opacity, self._scaling, self._rotation = t["opacity"], t["scaling"], t["rotation"]

    def track_density(self):
        self.stats = DensityStats(self._xyz.shape[0], self._xyz.device)
        self.max_radii2D = self.stats.max_radii2D

    def prune(self, keep):  # gaussian_model.py:488-505
        if self.stats is not None:
            t, extra = prune_optimizer(self.optimizer, keep, extra=self.stats.tensors())
            self.stats = DensityStats.of(extra)
            self.max_radii2D = self.stats.max_radii2D
        else:
            t, (self.max_radii2D,) = prune_optimizer(self.optimizer, keep, extra=(self.max_radii2D,))
        self._adopt(t)

    def densify_and_prune(self, **kw):  # gaussian_model.py:685-717, one pass (eogs2_amd.density)
        t, self.stats, info = densify_and_prune(self.optimizer, self.stats, **kw)
        self.max_radii2D = self.stats.max_radii2D
        self._adopt(t)
        return info


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=200_000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--graph", action="store_true",
                    help="record renders + losses + backward once into a HIP graph and replay it (eogs2_amd.graph.GraphedStep); "
                         "the optimizers stay outside unless --optimizer-in-graph, the graph is recorded again after every prune")
    ap.add_argument("--optimizer-in-graph", action="store_true",
                    help="both optimizers become FusedAdam(capturable=True): step counts and learning rates live on the device. "
                         "With --graph they are stepped INSIDE the recorded step, behind eogs2_amd.rasterizer.captured_gate() (a replay "
                         "that outgrew its list workspaces updates nothing and is recorded again); with --defer-prune K the "
                         "per-iteration retire of transparent Gaussians moves into the Adam launch (FusedAdam.retire_below) and the "
                         "compaction stays at its interval. Without --graph the same optimizers run eagerly")
    ap.add_argument("--sun-altitude-only", action="store_true",
                    help="the sun camera renders and resamples its altitude channel alone — what the reference's shipped "
                         "configuration consumes of it (iterstart_L_sun_resample is never reached, gs_config/train.yaml:123); "
                         "the sun-camera RGB consistency term is then absent, as it is there")
    ap.add_argument("--random-camera", action="store_true",
                    help="third render of the iteration: a random virtual camera at the view's size, resampled onto the view, "
                         "with the masked altitude / RGB consistency pair (train_pan.py:375-391, loss/main_loss.py:151-164)")
    ap.add_argument("--no-prune", action="store_true", help="keep every Gaussian (timing runs)")
    ap.add_argument("--prune-every", type=int, default=50, metavar="N",
                    help="iterations between prune points (the reference: 1, train_pan.py:673-678 — it asks the device "
                         "`transparent_mask.any()` every iteration)")
    ap.add_argument("--defer-prune", type=int, default=0, metavar="K",
                    help="at the prune points retire the transparent Gaussians (opacity 0: eogs2_amd.optim.retire_rows) and "
                         "compact only at every K-th of them and at the end: same renders, same updates, but no shape changes, "
                         "no wait for the device, and a recorded graph (--graph) keeps replaying in between")
    ap.add_argument("--parallel-renders", action="store_true",
                    help="the renders of the iteration (independent given the parameters: only the RESAMPLES need the view's "
                         "altitude) are queued on streams of their own, the largest first (eogs2_amd.graph.Branches); with --graph "
                         "they become parallel branches of the recorded graph, and autograd runs their backward passes on the same streams")
    ap.add_argument("--require-radii", action="store_true",
                    help="pipe.require_radii: every render also returns radii and `visibility_filter` = nonzero(radii > 0), which waits "
                         "for the device (renderer.py:128-130). The reference's shipped configuration has it OFF "
                         "(gs_config/train.yaml:39: require_radii = not only_prune, only_prune: True): off by default here too")
    ap.add_argument("--dsm-mae-every", type=int, default=0, metavar="N",
                    help="every N iterations score the altitude channel of the view's render as a DSM against the altitude render of "
                         "the unperturbed scene (the one that provides the target image): the reference's NCC registration, shift "
                         "and MAE (eogs2_amd.dsm_eval.dsm_mae; eval/dsmr.py, eval/eval_dsm.py:56-69), printed as `iteration dx dy mae` "
                         "and kept in main.last_dsm_mae (beside main.last_ms_per_iter: the returned tuple stays (first loss, last loss, "
                         "Gaussians), which callers compare between runs). Unit: the altitude channel is xyz @ affine[:3, 2] + affine[3, 2] "
                         f"(eogs2_amd/render.py), which for the synthetic Nadir camera is synthetic.ALT_SCALE ({ALT_SCALE:g}) x the scene's "
                         "normalised z, alpha-composited over bg[3]; divide the MAE by ALT_SCALE for normalised z. 0 = off")
    ap.add_argument("--dsm-resolution", type=float, default=0.0, metavar="R",
                    help="with --dsm-mae-every: score DSMs instead of altitude images. The altitude of the view's render and the "
                         "altitude of the unperturbed scene are each flattened into a DSM of cell size R on the device "
                         "(eogs2_amd.dsm_raster.dsm_from_view; utils/dsm_utils.py:7-51), both on the grid of the unperturbed scene's, "
                         f"and dsm_mae scores those over their filled cells. The scene's normalised coordinates times ALT_SCALE ({ALT_SCALE:g}) "
                         f"stand in for UTM metres, so R is in altitude units and the {ALT_SCALE:g}-unit-wide scene at --size 160 has about "
                         "one pixel per cell at R = 5. 0 = off: the altitude image is scored as it is")
    ap.add_argument("--flow-matching", action="store_true",
                    help="the flow-matching step of the reference's flagship configuration (train_pan.py:347-357, "
                         "optimization/flowmatching/raft_small.yaml): the target image is displaced by a fixed sub-pixel amount — a "
                         f"registration error of {FLOW_SHIFT} px — and every iteration warps the shaded image by the predicted flow before "
                         "the photometric loss (eogs2_amd.flow.perform_flow_matching, on_device=True, perform_cst_displacement=True: the "
                         "max_value_flow decision stays on the device, so --graph records it). The flow network is a stand-in that "
                         "answers that displacement as a field: RAFT, which the reference loads from torchvision, is the caller's")
    ap.add_argument("--flow-network", choices=["small", "large"], default=None, metavar="NAME",
                    help="with --flow-matching: eogs2_amd.raft.raft_small() or raft_large() (RAFT with the on-demand correlation "
                         "lookup of include/eogs_resample.h) takes the stand-in's place behind the same performOpticalmatching, 12 updates "
                         "per iteration. Without --flow-weights the network's weights are random: that demonstrates the plumbing "
                         "only, the max_value_flow criterion will reject the random flows and the image passes unwarped. Needs "
                         "--size of at least 121 (the network sees the size rounded up to a multiple of 8, at least 128); not "
                         "with --graph")
    ap.add_argument("--flow-update", choices=["auto", "torch", "fused", "fused_large"], default="auto", metavar="HOW",
                    help="with --flow-network: how RAFT's update block runs, eogs2_amd.raft.RAFT(update=...): 'torch' (torch "
                         "modules), 'fused' (the eogs_flownet_* convolutions of include/eogs_resample.h, RAFT-small only), "
                         "'fused_large' (RAFT-large's update block and mask predictor over the entries of include/eogs_resample.h, "
                         "RAFT-large only) or 'auto' (for RAFT-small what profiles/raft_update_probe.json measured as faster; for "
                         "RAFT-large the torch modules)")
    ap.add_argument("--flow-encoder", choices=["torch", "fused", "fused_large", "auto"], default="torch", metavar="HOW",
                    help="with --flow-network: how RAFT's two encoders run, eogs2_amd.raft.RAFT(encoder=...): 'torch' (torch "
                         "modules), 'fused' (the eogs_flowenc_* convolutions of include/eogs_resample.h, RAFT-small only), "
                         "'fused_large' (RAFT-large's residual encoders over the eogs_flowres_* entries, RAFT-large only) or 'auto' "
                         "(for RAFT-small what profiles/raft_encoder_probe.json measured as faster; for RAFT-large the torch modules)")
    ap.add_argument("--flow-weights", default=None, metavar="PATH",
                    help="with --flow-network: a torchvision RAFT checkpoint of that configuration (raft_small / raft_large state "
                         "dict), loaded strictly by eogs2_amd.raft.RAFT.load_weights; nothing is downloaded")
    ap.add_argument("--opacity-loss", type=float, default=0.0, metavar="W",
                    help="adds W x OpacityLoss (loss/opacity.py:14-17: the sum of the opacities over the initial number of Gaussians) "
                         "through eogs2_amd.regularizers.gaussian_regularizers; the reference's shipped configuration runs it on "
                         "every iteration with W = 0.1 (gs_config/train.yaml:118,141). 0 = absent")
    ap.add_argument("--erank-loss", type=float, default=0.0, metavar="W",
                    help="adds W x erankLoss (loss/main_loss.py:26-34) in the same launch group as --opacity-loss. 0 = absent")
    ap.add_argument("--pan-map", choices=[k for k in PAN_KINDS if k != "identity"], default=None, metavar="NAME",
                    help="a panchromatic camera (scene/cameras/PAN_affine_cameras.py): the render pipeline ends in the MSI->PAN map "
                         "NAME of the reference's load_msi_to_pan (only_one_channel, average, fixed, learnable_fixed, base, "
                         "fixedandtranslate) through eogs2_amd.pan.render_pipeline; the target image goes through the same map with its "
                         "default parameters and the photometric loss runs on one plane. The learnable maps start perturbed and are "
                         "unfrozen: their parameters join the camera's optimizer")
    ap.add_argument("--densify-every", type=int, default=0, metavar="K",
                    help="adaptive density control, the reference's `only_prune: False` (train_pan.py:679-711): every iteration "
                         "the densification statistics (eogs2_amd.density.DensityStats.update: one launch on the render's radii and "
                         "the screen-space gradient, no nonzero and no wait), every K iterations densify_and_prune in one pass "
                         "(eogs2_amd.density.densify_and_prune) followed by the transparent prune; implies radii; with --graph the "
                         "step is recorded again after each. 0 = off")
    ap.add_argument("--densify-grad-threshold", type=float, default=None, metavar="T",
                    help="with --densify-every: densify_grad_threshold (mean screen-space gradient norm at or above which a "
                         "Gaussian is cloned or split). The reference's value is tuned to its scenes; by default this example takes "
                         "the 0.95 quantile of the statistic over the rows seen so far at the first densification (one readback "
                         "there) and keeps it: about a twentieth of the Gaussians are densified each time")
    ap.add_argument("--pan-first", action="store_true",
                    help="with --pan-map: the reference's weird_pan_setup (PAN_affine_cameras.py:148-176): the map first, then a "
                         "Conv2d(1,1,1) colour correction and a scalar in-shadow tint")
    ap.add_argument("--monitor", action="store_true",
                    help="the reference's training metrics on the device (eogs2_amd.monitor.TrainingMonitor): per iteration the "
                         "photometric loss's own L1 and SSIM, the PSNR, the mean opacity and the two moving averages go into a device "
                         "buffer without a wait (inside the recorded step with --graph, behind the same gate as the optimizers); every "
                         f"{MONITOR_INTERVAL} iterations (tb_log_interval) the interval is closed and ONE record is fetched and printed. Off by default")
    ap.add_argument("--opacity-reset-every", type=int, default=0, metavar="N",
                    help="every N iterations the reference's reset_opacity (train_pan.py:726-732, gaussian_model.py:347-352; every 3000 "
                         "iterations in its flagship configuration) in place: eogs2_amd.reset.reset_opacity_ caps the logits at logit(0.01) "
                         "and clears the group's Adam moments in one launch, and replaces no tensor, so with --graph the recorded step "
                         "keeps replaying (main.last_recordings counts the recordings of the run). 0 = off")
    ap.add_argument("--color-reset-at", type=int, default=0, metavar="N",
                    help="at iteration N the reference's shadow-based colour reset (train_pan.py:733-736, color_reset_op.py; off in its "
                         "shipped configuration): eogs2_amd.reset.color_reset renders the training view with render_all_views, erodes its "
                         "shadow map, samples it at every Gaussian and resets opacity, colour and scale of the flagged rows and their "
                         "moments in place; no wait for the device and, with --graph, no new recording. 0 = off")
    ap.add_argument("--early-stop-patience", type=int, default=None, metavar="N",
                    help="with --monitor: the reference's early stopper (utils/callback_utils.py) with patience N intervals; the run "
                         "ends at the interval whose record carries the flag. Default: no early stopping (use_early_stopping: False)")
    ap.add_argument("--early-stop-metric", choices=MONITOR_METRICS, default="photometric", metavar="NAME",
                    help=f"with --monitor: the stopper's metric_name, one of {', '.join(MONITOR_METRICS)} (photometric: "
                         "optimization/early_stopping/l_photom.yaml); PSNR and SSIM are watched with operator max, the losses with min")
    ap.add_argument("--save-ply", default=None, metavar="PATH",
                    help="after the last iteration write the trainee as a binary little-endian PLY with the reference's vertex properties "
                         "(eogs2_amd.model.GaussianModel.save_ply; scene/gaussian_model.py:310-346): what its render_pan.py / tsdf.py chain loads")
    ap.add_argument("--load-ply", default=None, metavar="PATH",
                    help="start the trainee from a PLY written by --save-ply (or by the reference at sh_degree 0) instead of the perturbed "
                         "scene: the raw parameters are the file's, bit for bit (eogs2_amd.model.GaussianModel.load_ply). The file must "
                         "hold --gaussians rows (that count sizes the target scene and the run's per-row state): any other count is refused")
    ap.add_argument("--pansharp-loss", choices=sorted(PANSHARP_METHODS), default=None, metavar="METHOD",
                    help="adds 0.1 x Pansharploss (loss/pansharp_loss.py; pansharp_cfg.method METHOD: brovey, simple_brovey or ihs) through "
                         "eogs2_amd.pansharp: the ground truth is a synthetic pair, the target image averaged over 4 x 4 blocks as the "
                         "low-resolution MSI image and a PAN image at full size whose pansharpening gives the target image back up to the "
                         "upsampling; the pansharpened image is computed inside the loss's forward and backward kernels and never stored. "
                         "Both images are lifted to 0.9 x + 0.05 first, so that no bicubic undershoot meets brovey's clamp. The term sits "
                         "inside the recorded step with --graph; main.last_pansharp_loss keeps its first and last value. Default: absent")
    ap.add_argument("--views", type=int, default=1, metavar="V",
                    help="train V views as the reference does (train_pan.py:252-257: a random view popped from a stack that is refilled "
                         "when empty; :135-138: one camera-optimizer group per camera, so each camera's Adam moments and step count "
                         "advance only in the iterations that visit it). View v is the scene under make_camera(seed v) with a sun camera "
                         "and a perturbed colour camera of its own and a target rendered from the unperturbed scene. All per-view "
                         "tensors and the camera optimizer's state live in an eogs2_amd.views.ViewBank: bank.load() at the start of the "
                         "iteration, bank.store() and schedule.advance() after the optimizers, inside the recorded step with --graph "
                         "--optimizer-in-graph (behind the same gate). The camera optimizer is then a FusedAdam(capturable=True) in every "
                         "mode; main.view_bank exposes the bank. Default 1: one view, no bank")
    ap.add_argument("--random-background", action="store_true",
                    help="optimization.random_background (true in the reference's shipped configuration; train_pan.py:272-277): the three "
                         "colour channels of the background are drawn anew in every iteration, on the device, by a counter-based generator "
                         "keyed by --draw-seed and the iteration's index (eogs2_amd.draw; another generator than torch's: the sequence "
                         "differs from the reference's). bg[3], the view's lowest altitude, and bg[4] = 0 stay. One launch per iteration, "
                         "inside the recorded step with --graph. Default: the scene's one fixed background")
    ap.add_argument("--virtual-camera-extent", type=float, default=None, metavar="X",
                    help="with --random-camera: opt.virtual_camera_extent. The random virtual camera becomes the reference's "
                         "cam.sample_random_camera(X) (affine_cameras.py:403-430) of the current view, sampled anew in every iteration in "
                         "the same launch as --random-background: the view's affine sheared by randn(2).clip(-1, 1) * X about the "
                         "origin, cam2rnd its myM (times 350: this example's uva holds altitude / 350). Default: one fixed camera")
    ap.add_argument("--random-camera-type", choices=RENDER_TYPES, default="rawrender", metavar="TYPE",
                    help="with --random-camera: optimization.random_camera.randomcamera_render_type. rawrender_wshadow pushes the virtual "
                         "view through the view's render pipeline with a shadow map of its own (renderer_cc_shadow.py:57-145) and compares "
                         "it with the shaded image (eogs2_amd.randomcam.RandomcamRendering_Loss). Default: rawrender")
    ap.add_argument("--random-camera-gt", action="store_true",
                    help="with --random-camera: RandomcamRendering_Loss(use_gt=True): the comparison target is the ground-truth image, "
                         "which takes no gradient")
    ap.add_argument("--no-share-sun-render", action="store_true",
                    help="with --random-camera-type rawrender_wshadow: render the sun camera a second time inside the loss, as the "
                         "reference does, instead of handing it the iteration's own sun render (same camera, Gaussians and background)")
    ap.add_argument("--draw-seed", type=int, default=0, metavar="S", help="the 64-bit seed of --random-background and --virtual-camera-extent")
    ap.add_argument("--test-views", type=int, default=0, metavar="N",
                    help="hold out N synthetic views (make_camera(seed 100 + t), a sun camera and a perturbed colour camera of their own, "
                         "the target from the unperturbed scene) for --report-every and --render-set. Default 0: none")
    ap.add_argument("--report-every", type=int, default=0, metavar="K",
                    help="every K iterations the reference's training_report (train_pan.py:838-951) over the test and the train views: "
                         "--cc-to-test, then eogs2_amd.report.evaluate_views per set, printed as the reference prints it and kept in "
                         "main.last_reports. No wait per camera: the sums stay on the device until the one copy. 0 = off")
    ap.add_argument("--cc-to-test", choices=("ref", "average"), default="average", metavar="RULE",
                    help="with --report-every: scene.train_to_test_cc_converter, how the test cameras get their colour correction from the "
                         "train cameras (utils/convert_color_correction.py): view 0's (ref) or the mean over the train views (average)")
    ap.add_argument("--normalize-colors", action="store_true",
                    help="after the last iteration and before --save-ply the reference's normalize_before_saving (utils/save_utils.py; "
                         "train_pan.py:614-620) with view 0 as the reference camera: its colour correction becomes the identity, every "
                         "Gaussian's colour and every other view's correction are mapped so that renders stay the same. In place "
                         "(eogs2_amd.report): the parameter, its address and the optimizer state stay; main.last_alignment keeps the "
                         "colours before and after")
    ap.add_argument("--render-set", default=None, metavar="DIR",
                    help="after the last iteration write the products the reference's render_set writes per camera (render_pan.py:94-476) "
                         "for every train and test view as DIR/<product>/<view>.npy in file layout, and render_video.py's frame "
                         "[final | normalised elevation] (8-bit BGR) as DIR/frames/<view>.npy: eogs2_amd.report.view_products, "
                         "fetch_products (one packing launch and one copy per view) and video_frame")
    ap.add_argument("--transient-nll", type=float, default=0.0, metavar="W",
                    help="adds W x the transient-uncertainty term (train_pan.py:433-449: gaussian_nll_loss of the shaded image under the "
                         "variance (clip(transient_mask, 0, 1) + 1e-3)^2) through eogs2_amd.uncertainty.transient_nll: one forward launch "
                         "group and one backward launch, no wait. The H x W mask is a parameter of the camera optimizer, with --views a "
                         "ViewBank state slot per view; a bright rectangle is painted into one view's ground truth and the final mean mask "
                         "inside and outside of it is printed (main.last_transient). 0 = absent")
    ap.add_argument("--transient-init", type=float, default=0.01, metavar="V",
                    help="with --transient-nll: transient_params.init_value, what every camera's mask starts at (the reference's default)")
    ap.add_argument("--transient-from", type=int, default=0, metavar="ITER",
                    help="with --transient-nll: opt.iterstart_L_nll. The term's weight is a device tensor that holds 0 up to and including "
                         "iteration ITER and W after it: the switch is a write into that tensor, a recorded step is not recorded again")
    a = ap.parse_args(argv)
    if a.transient_nll < 0 or a.transient_from < 0:
        ap.error("--transient-nll and --transient-from are not negative")
    if (a.transient_from or a.transient_init != 0.01) and not a.transient_nll:
        ap.error("--transient-init and --transient-from belong to --transient-nll W")
    if a.test_views < 0 or a.report_every < 0:
        ap.error("--test-views and --report-every are not negative")
    if a.report_every and not a.test_views:
        ap.error("--report-every evaluates held-out views: give --test-views N")
    if a.normalize_colors and a.pan_first:
        ap.error("--normalize-colors recomposes 3 x 3 colour corrections: not with --pan-first, whose correction is 1 x 1")
    if a.virtual_camera_extent is not None and not a.random_camera:
        ap.error("--virtual-camera-extent samples the camera of --random-camera")
    if a.virtual_camera_extent is not None and not (a.virtual_camera_extent >= 0 and math.isfinite(a.virtual_camera_extent)):
        ap.error("--virtual-camera-extent must be finite and not negative")
    if (a.random_camera_type != "rawrender" or a.random_camera_gt) and not a.random_camera:
        ap.error("--random-camera-type and --random-camera-gt belong to --random-camera")
    if a.no_share_sun_render and a.random_camera_type != "rawrender_wshadow":
        ap.error("--no-share-sun-render belongs to --random-camera-type rawrender_wshadow")
    if not 0 <= a.draw_seed < 1 << 64:
        ap.error("--draw-seed must fit 64 unsigned bits")
    if a.views < 1:
        ap.error("--views must be at least 1")
    if a.views > 1 and (a.dsm_mae_every or a.pansharp_loss or a.flow_matching or a.color_reset_at or a.pan_map):
        ap.error("--views V > 1 keeps the views' data in one bank: not with --dsm-mae-every, --pansharp-loss, --flow-matching, "
                 "--color-reset-at or --pan-map, which hold per-view data of their own here")
    if a.pansharp_loss and a.pan_map:
        ap.error("--pansharp-loss compares three-plane images: not with --pan-map")
    if a.pansharp_loss and a.size % 4:
        ap.error("--pansharp-loss averages the target over 4 x 4 blocks: --size must be a multiple of 4")
    if a.early_stop_patience is not None and not a.monitor:
        ap.error("--early-stop-patience needs --monitor")
    if a.dsm_resolution and not a.dsm_mae_every:
        ap.error("--dsm-resolution needs --dsm-mae-every")
    if a.pan_first and not a.pan_map:
        ap.error("--pan-first needs --pan-map")
    if (a.flow_network or a.flow_weights) and not a.flow_matching:
        ap.error("--flow-network and --flow-weights belong to --flow-matching")
    if a.flow_weights and not a.flow_network:
        ap.error("--flow-weights needs --flow-network small|large")
    if a.flow_update == "fused" and a.flow_network != "small":
        ap.error("--flow-update fused needs --flow-network small")
    if a.flow_update == "fused_large" and a.flow_network != "large":
        ap.error("--flow-update fused_large needs --flow-network large")
    if a.flow_encoder == "fused" and a.flow_network != "small":
        ap.error("--flow-encoder fused needs --flow-network small")
    if a.flow_encoder == "fused_large" and a.flow_network != "large":
        ap.error("--flow-encoder fused_large needs --flow-network large")
    if a.flow_network and (a.size < 121 or a.graph):
        ap.error("--flow-network: RAFT needs images of at least 128 px after rounding up to a multiple of 8 (--size >= 121), and is "
                 "not recorded into a graph here (not with --graph)")
    if a.pan_map and a.flow_matching:
        ap.error("--flow-matching runs on the three-plane pipeline here: not with --pan-map")
    if a.load_ply:  # the scene, the noise and the statistics are sized by --gaussians: the file must hold as many rows
        with open(a.load_ply, "rb") as f:
            _, file_rows, _ = parse_ply_header(f.read(1 << 16))
        if file_rows != a.gaussians:
            ap.error(f"--load-ply: {a.load_ply} holds {file_rows} Gaussians, --gaussians is {a.gaussians}: give the file's count")
    dev = torch.device("cuda:0")
    P, H, W = a.gaussians, a.size, a.size
    sc = make_scene(P, H, W, seed=0, opacity="trained", device=dev)
    cam = Camera(sc["viewmatrix"], H, W)
    sun = Camera(make_camera(2 * H, 2 * W, seed=5, device=dev), 2 * H, 2 * W)
    cam2sun = torch.eye(3, device=dev)
    cam2sun[:2, 2] = (sun.affine[2, :2] - cam.affine[2, :2]) / 350.0  # altitude-dependent shift between the two views
    rnd = Camera(make_camera(H, W, seed=9, device=dev), H, W)
    cam2rnd = torch.eye(3, device=dev)
    cam2rnd[:2, 2] = (rnd.affine[2, :2] - cam.affine[2, :2]) / 350.0
    pipe = types.SimpleNamespace(debug=False, antialiasing=False, compute_cov3D_python=False, require_radii=a.require_radii or bool(a.densify_every),
                                 visibility_as_mask=bool(a.densify_every))  # (the statistics kernel reads radii: no index list, no wait)
    bg = sc["bg"]
    U, V = torch.meshgrid(torch.linspace(-1, 1, W, device=dev), torch.linspace(-1, 1, H, device=dev), indexing="xy")

    branches = Branches(3, device=dev) if a.parallel_renders else None
    # --random-camera-type rawrender_wshadow / --random-camera-gt: the reference's loss class; else the comparison alone, as before
    rc_loss = None
    if a.random_camera and (a.random_camera_type != "rawrender" or a.random_camera_gt):
        rc_loss = RandomcamRendering_Loss(1e-4, 1e-3, a.random_camera_type, use_gt=a.random_camera_gt)
    share_sun = a.random_camera_type == "rawrender_wshadow" and not a.no_share_sun_render

    def random_camera_loss(m, cc_cam, uva, altitude, img, shaded, sun_img, rnd_img):
        """train_pan.py:375-391 through RandomcamRendering_Loss: (L_new_altitude_resample, L_new_rgb_resample). The target's own
        views (no grad) have no use for it."""
        if not torch.is_grad_enabled():
            return None
        kw = dict(virtual_render=rnd_img)
        if a.random_camera_type == "rawrender_wshadow":
            kw.update(sun_render=sun_img if share_sun else None)
        return rc_loss(rnd, cc_cam, cam2rnd, uva, m, pipe, bg, altitude, img, gt, shaded["shaded"], **kw)

    def view(m, cc_cam):
        """train_pan.py:279-330: view render, sun render resampled onto the view, camera render pipeline."""
        if branches is not None:
            # the three renders side by side, the 2H x 2W one first; then what render_resample_virtual_camera does with them
            sun_img, out, rnd_img = branches.run([
                lambda: render(sun, m, pipe, bg, altitude_only=a.sun_altitude_only)["render"],
                lambda: render(cam, m, pipe, bg),
                lambda: render(rnd, m, pipe, bg)["render"] if a.random_camera else None],
                shared=())  # forwards only: the iteration's one backward() follows the join
            img, altitude = out["render"][:3], out["render"][3]
            uva = torch.stack((U, V, altitude / 350.0), dim=-1)
            if a.sun_altitude_only:
                smp, sun_uv = resample(sun_img, cam2sun, uva, n_out=1, fill_channel=0)
                sun_rgb, sun_alt = None, smp[0]
            else:
                smp, sun_uv = resample(sun_img, cam2sun, uva)
                sun_rgb, sun_alt = smp[:3], smp[3]
            sun_altitude_diff = altitude - sun_alt
            shaded = pipeline(cc_cam, img, sun_altitude_diff)
            new = None
            if rc_loss is not None:
                new = random_camera_loss(m, cc_cam, uva, altitude, img, shaded, sun_img, rnd_img)
            elif a.random_camera:
                smp, new_uv = resample(rnd_img, cam2rnd, uva)
                new = (altitude - smp[3], smp[:3], new_uv)
            return out, img, sun_rgb, sun_uv, sun_altitude_diff, shaded, new
        out = render(cam, m, pipe, bg)
        img, altitude = out["render"][:3], out["render"][3]
        uva = torch.stack((U, V, altitude / 350.0), dim=-1)
        sun_rgb, sun_alt, sun_uv, sun_img = render_resample_virtual_camera(sun, cam2sun, uva, m, pipe, bg, return_extra=True,
                                                                           altitude_only=a.sun_altitude_only)
        sun_altitude_diff = altitude - sun_alt
        shaded = pipeline(cc_cam, img, sun_altitude_diff)
        new = None
        if rc_loss is not None:  # (the virtual camera is rendered inside the loss)
            new = random_camera_loss(m, cc_cam, uva, altitude, img, shaded, sun_img, None)
        elif a.random_camera:  # train_pan.py:375-391 / loss/main_loss.py:123-164
            new_rgb, new_alt, new_uv = render_resample_virtual_camera(rnd, cam2rnd, uva, m, pipe, bg)
            new = (altitude - new_alt, new_rgb, new_uv)
        return out, img, sun_rgb, sun_uv, sun_altitude_diff, shaded, new

    pipeline = pan_render_pipeline if a.pan_map else render_pipeline

    def pan_map(perturb):
        """The MSI->PAN map of --pan-map with the reference's initial values (transf_msi_to_pan.py:11-14,116-117); the
        trainee's (perturb > 0) learnable tensors are Parameters that start off those values."""
        dflt = torch.tensor(FIXED_PARAMS, device=dev)
        param = lambda t, rel: torch.nn.Parameter(t + rel * perturb * torch.randn(t.shape, generator=gcam).to(dev)) if perturb else t  # noqa: E731
        if a.pan_map == "fixed":
            return PanMap("fixed", params=dflt)
        if a.pan_map == "learnable_fixed":
            return PanMap("learnable_fixed", params=param(dflt.clone(), 0.5))
        if a.pan_map == "base":
            return PanMap("base", weight=param(dflt[:3].clone(), 0.5), bias=param(dflt[4:].clone(), 0.5))
        if a.pan_map == "fixedandtranslate":
            return PanMap("fixedandtranslate", weight=param(torch.zeros(3, device=dev), 0.5), bias=param(torch.zeros(1, device=dev), 0.5),
                          fixed_weights=dflt[:3].clone(), fixed_bias=dflt[4:].clone(), learn_conv2d=True)
        return PanMap(a.pan_map)

    def pan_camera(perturb):
        c = types.SimpleNamespace(use_cc=True, use_exposure=False, use_shadow=True, weird_pan_setup=a.pan_first)
        n = 1 if a.pan_first else 3  # PAN_affine_cameras.py:46-60: the map-first order overrides the (3,3) conv with a (1,1) one
        c.color_correction = torch.nn.Conv2d(n, n, 1, bias=True).to(dev)
        with torch.no_grad():
            c.color_correction.weight.copy_((torch.eye(n) + perturb * torch.randn(n, n, generator=gcam)).reshape(n, n, 1, 1))
            c.color_correction.bias.zero_()
        c.inshadow_color_correction = torch.nn.Parameter(torch.full((n, 1, 1), 0.05, device=dev))
        c.msi_to_pan = pan_map(perturb)
        c.get_sun_camera = lambda: (sun, cam2sun)
        m = c.msi_to_pan
        c.map_parameters = [t for t in (m.params, m.weight, m.bias) if isinstance(t, torch.nn.Parameter)]
        return c

    def colour_camera(perturb):
        if a.pan_map:
            return pan_camera(perturb)
        c = types.SimpleNamespace(use_cc=True, use_exposure=False, use_shadow=True)
        c.color_correction = torch.nn.Conv2d(3, 3, 1, bias=True).to(dev)  # affine_cameras.py:219-231
        with torch.no_grad():
            c.color_correction.weight.copy_((torch.eye(3) + perturb * torch.randn(3, 3, generator=gcam)).reshape(3, 3, 1, 1))
            c.color_correction.bias.zero_()
        c.inshadow_color_correction = torch.nn.Parameter(torch.full((3, 1, 1), 0.05, device=dev))
        c.get_sun_camera = lambda: (sun, cam2sun)  # affine_cameras.py:350-370: what RandomcamRendering_Loss asks the true camera for
        return c

    gcam = torch.Generator().manual_seed(2)
    target_model = Gaussians(sc["means3D"], sc["colors"][:, :3], sc["opacities"].squeeze(1).clamp(1e-4, 1 - 1e-4),
                             sc["scales"], sc["rotations"])
    with torch.no_grad():
        target_view = view(target_model, colour_camera(0.0))
        gt = target_view[5]["final"].clone()
        transient_box = paint_transient(gt) if a.transient_nll and a.views == 1 else None
        gt_altitude = target_view[0]["render"][3].clone() if a.dsm_mae_every else None
        del target_view
    dsm_cam = dsm_scene = dsm_geometry = gt_dsm = None
    if a.dsm_mae_every and a.dsm_resolution:  # scene_params: a UTM-sized centre, normalised coordinates x ALT_SCALE as metres
        dsm_scene = [(5e5, 4.3e6, 0.0), ALT_SCALE]
        dsm_cam = types.SimpleNamespace(affine=cam.affine, Ainv=torch.inverse(cam.affine[:3, :3].T))  # affine_cameras.py:159
        profile, gt_dsm = dsm_from_view(gt_altitude, dsm_cam, dsm_scene, a.dsm_resolution)  # the one wait: the target's bounds
        dsm_geometry = (profile["transform"][2], profile["transform"][5], profile["width"], profile["height"])
    pansharp_term = None
    if a.pansharp_loss:  # train_pan.py:215-224: the MSI ground truth at a quarter of the PAN size, pansharpened by the loss itself
        lift = lambda x: 0.9 * x + 0.05  # noqa: E731
        with torch.no_grad():
            gt_msi_lr = torch.nn.functional.avg_pool2d(lift(gt)[None], 4)[0].contiguous()
            total = lift(gt).sum(dim=0)
            gt_pan_hr = {"brovey": 0.1 * total, "simple_brovey": total, "ihs": total / 3.0}[a.pansharp_loss].contiguous()
        pansharp_args = {"brovey": (gt_pan_hr, gt_msi_lr), "simple_brovey": (gt_pan_hr, gt_msi_lr[None]),
                         "ihs": (gt_pan_hr[None], gt_msi_lr)}[a.pansharp_loss]
        pansharp_term = Pansharploss(0.1, types.SimpleNamespace(method=a.pansharp_loss))
    warper = None
    if a.flow_matching:
        shift = torch.tensor(FLOW_SHIFT, device=dev).view(1, 2, 1, 1).expand(1, 2, H, W)
        with torch.no_grad():
            gt = apply_flow(gt, shift).clone()  # gt(x) <- gt(x + shift): what a flow of `shift` applied to the render undoes
        hp, wp = -(-H // 8) * 8, -(-W // 8) * 8  # the size the network is called with (mode "upscale")
        field = torch.tensor(FLOW_SHIFT, device=dev).view(1, 2, 1, 1).repeat(1, 1, hp, wp)
        flow_model = lambda gt_n, img_n, num_flow_updates=12: [field]  # noqa: E731  (the stand-in)
        if a.flow_network:
            from eogs2_amd import raft

            flow_model = raft.RAFT(a.flow_network, update=a.flow_update, encoder=a.flow_encoder).eval().to(dev)
            if a.flow_weights:
                flow_model.load_weights(a.flow_weights)
        warper = performOpticalmatching(True, mode="upscale", device=dev, model_name=a.flow_network or "small", criteria="max_value_flow",
                                        model=flow_model)
        flow_opt = types.SimpleNamespace(flowmatching=types.SimpleNamespace(max_value_flow=3.0))
    cc_cam = colour_camera(0.15)
    camera_parameters = [*cc_cam.color_correction.parameters(), cc_cam.inshadow_color_correction, *getattr(cc_cam, "map_parameters", ())]
    # --transient-nll: the camera's transient mask joins its optimizer (affine_cameras.py:282-289, train_pan.py:135-138); the weight
    # of the term is a device tensor, 0 until --transient-from has passed
    transient_mask = transient_weight = None
    optimizer_parameters = list(camera_parameters)
    if a.transient_nll:
        transient_mask = transient_parameters(H, W, a.transient_init, dev)
        transient_weight = torch.zeros(1, device=dev)
        optimizer_parameters.append(transient_mask)
    if a.optimizer_in_graph or a.views > 1:  # one prologue + one element launch for the handful of 3-12 element tensors
        camera_optimizer = FusedAdam(optimizer_parameters, lr=2e-3, capturable=True)  # (--views: the bank carries device step counts)
    else:
        camera_optimizer = torch.optim.Adam(optimizer_parameters, lr=2e-3)

    view_bank = view_schedule = None
    if a.views > 1:
        # View v: the scene under make_camera(seed v) (view 0 is the camera above), its own sun camera and altitude shifts, its
        # target from the unperturbed scene, its own perturbed colour camera. The tensors the iteration reads (cam.affine,
        # sun.affine, cam2sun, cam2rnd, bg, gt, the colour camera's parameters) stay where they are: they are the bank's working
        # tensors, and the rows are written through them here.
        n_views = a.views
        rows = {k: [] for k in ("viewmatrix", "sun_viewmatrix", "cam2sun", "cam2rnd", "bg", "gt")}
        identity_camera = colour_camera(0.0)
        for v in range(n_views):
            vm, sun_vm = make_camera(H, W, seed=v, device=dev), make_camera(2 * H, 2 * W, seed=5 + 10 * v, device=dev)
            c2s, c2r = torch.eye(3, device=dev), torch.eye(3, device=dev)
            c2s[:2, 2] = (sun_vm[2, :2] - vm[2, :2]) / 350.0
            c2r[:2, 2] = (rnd.affine[2, :2] - vm[2, :2]) / 350.0
            bg_v = bg.clone()
            bg_v[3] = (sc["means3D"] @ vm[:3, 2] + vm[3, 2]).min()  # train_pan.py:272-277: the view's lowest altitude
            for t, r in ((cam.affine, vm), (sun.affine, sun_vm), (cam2sun, c2s), (cam2rnd, c2r), (bg, bg_v)):
                t.copy_(r)
            with torch.no_grad():
                gt_v = view(target_model, identity_camera)[5]["final"].clone()
            if a.transient_nll and v == 1:  # the transient object: in this one view's ground truth only
                transient_box = paint_transient(gt_v)
            for k, r in zip(rows, (vm, sun_vm, c2s, c2r, bg_v, gt_v)):
                rows[k].append(r)
        cc_rows = [[p.detach().clone() for p in camera_parameters]]
        for v in range(1, n_views):
            c = colour_camera(0.15)
            cc_rows.append([p.detach().clone() for p in (*c.color_correction.parameters(), c.inshadow_color_correction)])
        view_schedule = ViewSchedule(reference_order(n_views, a.iters, random.Random(0)), n_views, dev)
        view_bank = ViewBank(view_schedule)
        for k, t in zip(rows, (cam.affine, sun.affine, cam2sun, cam2rnd, bg, gt)):
            view_bank.add_input(k, t, rows[k])
        for i, p in enumerate(camera_parameters):
            view_bank.add_state(f"camera.{i}", p, [cc_rows[v][i] for v in range(n_views)])
        if transient_mask is not None:  # every view's mask starts at --transient-init: the rows are copies of the working tensor
            view_bank.add_state("transient_mask", transient_mask)
        for p in optimizer_parameters:  # one eager step creates the optimizer's state; zero gradients move no parameter
            p.grad = torch.zeros_like(p)
        camera_optimizer.step()
        view_bank.attach_optimizer(camera_optimizer)  # every view starts at step 0 with zero moments, as torch's lazy state does
    main.view_bank = view_bank
    # --random-background / --virtual-camera-extent: one launch per iteration writes bg[0..2], bg[4] and the rnd camera's affine
    # and cam2rnd, after the bank's load filled them. The iteration's index is the schedule's cursor (--views) or a counter of
    # the stream's own, which then moves where the schedule would.
    draws = draw_stream = draw_shear = None
    if a.random_background or a.virtual_camera_extent is not None:
        draw_stream = DrawStream(a.draw_seed, counter=view_schedule.cursor) if view_schedule is not None else DrawStream(a.draw_seed, device=dev)
        draws = IterationDraws(draw_stream)
        kw = {}
        if a.random_background:
            kw.update(bg=bg)
        if a.virtual_camera_extent is not None:
            draw_shear = torch.zeros(2, device=dev)
            kw.update(virt_affine=rnd.affine, cam2virt=cam2rnd, shear=draw_shear, extent=a.virtual_camera_extent, cam2virt_scale=350.0)
        draws.add_camera(cam.affine, torch.zeros(3, device=dev), **kw)
        if not a.quiet:  # what was drawn, per iteration: device-to-device copies, read once after the run
            draw_log = torch.zeros(a.iters, 5, device=dev)
    main.draw_stream = draw_stream

    # --test-views / --report-every / --normalize-colors / --render-set: every view as a camera of the reference's kind, with what
    # training_report, normalize_before_saving and render_set read from one (a viewpoint here is its own MSI or PAN camera)
    train_viewpoints, test_viewpoints, report_opt, converter = [], [], None, None
    if a.test_views or a.normalize_colors or a.render_set:
        kind = "pan" if a.pan_map else "msi"
        report_opt = types.SimpleNamespace(load_msi=kind == "msi", load_pan=kind == "pan", random_background=False)
        converter = load_convert_color_correction_train_to_test(a.cc_to_test)

        def report_camera(name, vm, sun_vm, colour, bg3, is_reference=False):
            rc = Camera(vm, H, W)
            rc.image_name, rc.image_type, rc.is_reference_camera = name, kind, is_reference
            rc.altitude_bounds = torch.stack((bg3, bg3)).detach()  # (the lower bound becomes the altitude background, without a readback)
            rc.UV_grid = (U, V)
            for which, other in (("sun", Camera(sun_vm, 2 * H, 2 * W)), ("nadir", Camera(rnd.affine.clone(), H, W))):
                m = torch.eye(3, device=dev)  # (the report stacks the altitude itself, view() the altitude / 350: the same product)
                m[:2, 2] = (other.affine[2, :2] - vm[2, :2]) / 350.0 / 350.0
                setattr(rc, f"get_{which}_camera", lambda other=other, m=m: (other, m))
            rc.color_correction = colour.color_correction
            rc.render_pipeline = lambda raw_render, sun_altitude_diff=None: pipeline(colour, raw_render, sun_altitude_diff)
            rc.get_msi_cameras = rc.get_pan_cameras = lambda: rc
            return rc

        def target_image(rc_of):
            """The view's target: the unperturbed scene under an identity colour camera."""
            c = rc_of(colour_camera(0.0))
            return render_all_views([c], target_model, pipe, bg=bg.clone())[0]["render"].clone()

        if view_bank is not None:  # the views' colour parameters are the bank's rows: cameras over them, no copies
            for v in range(a.views):
                colour = types.SimpleNamespace(use_cc=True, use_exposure=False, use_shadow=True, inshadow_color_correction=view_bank.row("camera.2", v),
                                               color_correction=types.SimpleNamespace(weight=view_bank.row("camera.0", v), bias=view_bank.row("camera.1", v)))
                rc = report_camera(f"train_{v}", rows["viewmatrix"][v], rows["sun_viewmatrix"][v], colour, rows["bg"][v][3], is_reference=v == 0)
                rc.original_image = rows["gt"][v]
                train_viewpoints.append(rc)
        else:
            rc = report_camera("train_0", cam.affine, sun.affine, cc_cam, bg[3], is_reference=True)
            rc.original_image = gt
            train_viewpoints.append(rc)
        for k in range(a.test_views):
            vm, sun_vm = make_camera(H, W, seed=100 + k, device=dev), make_camera(2 * H, 2 * W, seed=105 + 10 * k, device=dev)
            bg3 = (sc["means3D"] @ vm[:3, 2] + vm[3, 2]).min()
            rc_of = lambda colour, k=k, vm=vm, sun_vm=sun_vm, bg3=bg3: report_camera(f"test_{k}", vm, sun_vm, colour, bg3)  # noqa: E731
            rc = rc_of(colour_camera(0.15))
            with torch.no_grad():
                rc.original_image = target_image(rc_of)
            test_viewpoints.append(rc)
    main.last_reports = []  # --report-every: (iteration, "test" | "train", evaluate_views' dict)

    # the trainee: perturbed colours / opacities / positions, scales re-initialised from the 3-NN statistic
    g = torch.Generator().manual_seed(1)
    noise = lambda *s: torch.randn(*s, generator=g).to(dev)
    dist2 = torch.clamp_min(distCUDA2(sc["means3D"]), 1e-7)  # gaussian_model.py:179-182
    model = Gaussians(sc["means3D"] + 2e-4 * noise(P, 3), (sc["colors"][:, :3] + 0.2 * noise(P, 3)).clamp(0.02, 0.98),
                      torch.full((P,), 0.3, device=dev), torch.sqrt(dist2)[:, None].repeat(1, 3), sc["rotations"],
                      capturable=a.optimizer_in_graph)
    if a.load_ply:  # the same class over the file's Gaussians; then the file's raw bits under its activations' round trip
        loaded = GaussianModel(0)
        loaded.load_ply(a.load_ply)
        with torch.no_grad():
            model = Gaussians(loaded.get_xyz, loaded._features_dc.reshape(-1, 3) * C0 + 0.5, loaded.get_opacity.squeeze(1), loaded.get_scaling,
                              loaded._rotation, capturable=a.optimizer_in_graph)
            for name in ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation"):
                getattr(model, name).copy_(getattr(loaded, name).reshape(getattr(model, name).shape))
    if a.virtual_camera_extent and a.graph:
        # A recorded step's list workspaces are sized from the counts the forwards before the recording have seen, plus a margin
        # (eogs_rast_capacity_token). The sampled camera's shear moves and widens every footprint, so its count varies from
        # replay to replay: render it once at the four corners of the shear's range for every view, so that the recording is
        # sized for the range and not for the one camera of its warm-up run.
        with torch.no_grad():
            for vm in (rows["viewmatrix"] if view_bank is not None else [cam.affine.clone()]):
                for d0, d1 in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
                    corner = vm.clone()  # (stored transposed: column i is row i of A; the centre is the origin, b stays)
                    corner[:3, 0] += d0 * a.virtual_camera_extent * vm[:3, 2]
                    corner[:3, 1] += d1 * a.virtual_camera_extent * vm[:3, 2]
                    rnd.affine.copy_(corner)
                    render(rnd, model, pipe, bg)
    min_logit = math.log(0.005 / 0.995)  # the transparent prune's threshold on the raw logit
    retire_in_step = bool(a.optimizer_in_graph and a.defer_prune and not a.no_prune)
    if retire_in_step:  # train_pan.py:673-678 in its deferred form, every iteration, inside the Adam launch
        model.optimizer.retire_below = {"opacity": min_logit}
    steps_inside = bool(a.optimizer_in_graph and a.graph)
    eager_run = {"on": False}  # --optimizer-in-graph --graph: the one iteration that runs fwd_bwd eagerly (the first)
    # the regularisers over the raw parameters: weights in a device tensor the kernels read (a schedule would write into it
    # between replays of a recorded graph), terms chosen once; init_number_of_gaussians is the constant P of the start
    extent, grad_threshold = 0.0, a.densify_grad_threshold
    if a.densify_every:
        model.track_density()
        torch.manual_seed(0)  # densify_and_prune draws the split samples from the device's default generator: the same run twice
        extent = 0.5 * float((sc["means3D"].max(dim=0).values - sc["means3D"].min(dim=0).values).max())  # cameras_extent's role
    reg_want = tuple(n for n, w in (("opacity", a.opacity_loss), ("erank", a.erank_loss)) if w)
    reg_weights = torch.tensor([a.opacity_loss, 0.0, a.erank_loss], device=dev) if reg_want else None
    mon = None
    if a.monitor:
        mon = TrainingMonitor(dev, metric_name=a.early_stop_metric, patience=a.early_stop_patience,
                              operator="max" if a.early_stop_metric.endswith(("psnr", "ssim")) else "min")
        mon.reset()  # the state exists (and is reset) before any recording: a recorded reset would run on every replay

    def feed_monitor(final, photo_out, loss, gate):
        """train_pan.py:423-429,471-495 without their .item() waits and without the second SSIM: four launch groups, no wait."""
        mon.observe(final, gt, "pan" if a.pan_map else "msi", loss_out=photo_out, lambda_dssim=0.2, gate=gate)
        mon.observe_model(model._opacity, gate=gate)  # (train_pan.py:331: the opacities the iteration rendered with)
        mon.end_iteration(loss, gate=gate)

    def fwd_bwd():
        """Everything between two optimizer steps; reads the model's and the camera's parameter tensors in place."""
        if view_bank is not None:  # --views: the current view's rows into the tensors everything below reads
            view_bank.load()
        if draws is not None:  # --random-background / --virtual-camera-extent: this iteration's background and virtual camera
            draws.draw()
        model.optimizer.zero_grad(set_to_none=True)
        camera_optimizer.zero_grad(set_to_none=True)
        out, img, sun_rgb, sun_uv, sun_altitude_diff, shaded, new = view(model, cc_cam)
        final = shaded["final"]
        if warper is not None:  # train_pan.py:347-357
            _, _, final = perform_flow_matching(flow_opt, warper, final, gt, on_device=True)
        if mon is None:
            loss, _ = photometric_loss(final, gt, 0.2)
        else:  # the same launches; out[3] = {loss, L1, SSIM} stays on the device for the monitor
            loss, _, photo_out = photometric_loss(final, gt, 0.2, return_out=True)
        loss = loss + 1e-3 * translucentshadows_l(shaded["shadowmap"])
        if sun_rgb is not None:
            L_sun_alt, L_sun_rgb = suncamera_l(img, sun_rgb, sun_altitude_diff, sun_uv)
            loss = loss + 1e-4 * L_sun_alt + 1e-3 * L_sun_rgb
        if new is not None:
            L_new_alt, L_new_rgb = new if rc_loss is not None else randomcam_l(new[0], img, new[1], new[2])
            loss = loss + 1e-4 * L_new_alt + 1e-3 * L_new_rgb
            if rc_loss is not None:
                kept["random_camera"] = (L_new_alt.detach(), L_new_rgb.detach())
        if reg_want:  # train_pan.py:450-465: w_L_opacity * L_opacity (+ w_L_erank * L_erank), summed in the kernel
            loss = loss + gaussian_regularizers(model._opacity, model._scaling, n_init=P, weights=reg_weights, want=reg_want)[0]
        if transient_mask is not None:  # w_L_nll * L_nll (train_pan.py:433-440,461): the weight is read on the device
            nll_total, _, kept["transient"] = transient_nll(final, gt, transient_mask, weight=transient_weight)
            loss = loss + nll_total
        if pansharp_term is not None:  # w_L_pansharp * L_pansharp: one forward and one backward kernel, no full-size temporaries
            kept["pansharp"] = pansharp_term(lift(final), *pansharp_args)
            loss = loss + pansharp_term.lambda_L_pansharp * kept["pansharp"]
            kept["pansharp"] = kept["pansharp"].detach()
        loss.backward()
        # --monitor: like the optimizers, inside the recorded step only with --optimizer-in-graph --graph (gated as they are:
        # an outgrown replay is not counted), else after it, from the tensors kept here (under --graph: refilled by a replay)
        if mon is not None:
            kept["monitor"] = (final.detach(), photo_out, loss.detach())
            if steps_inside and (eager_run["on"] or torch.cuda.is_current_stream_capturing()):
                feed_monitor(*kept["monitor"], captured_gate())
        # --optimizer-in-graph --graph: both optimizers inside the recorded step, gated by the device's own verdict on this
        # replay's forwards. (The eager warm-up runs of the recording skip them: a warm-up is not an iteration.)
        if steps_inside and (eager_run["on"] or torch.cuda.is_current_stream_capturing()):
            gate = captured_gate()  # None in the eager run
            model.optimizer.step(gate=gate)
            camera_optimizer.step(gate=gate)
            if view_bank is not None:  # the view's updated camera state back into its rows, the cursor on: gated like the steps
                view_bank.store(gate)
                view_schedule.advance(gate)
            elif draw_stream is not None:  # (one view: the stream counts the iterations itself)
                draw_stream.advance(gate)
        if a.dsm_mae_every:
            kept["altitude"] = out["render"][3].detach()  # (under --graph: the recorded step's output tensor, refilled by a replay)
        return loss.detach(), out.get("radii"), out["viewspace_points"].grad

    reset_cameras = []
    if a.color_reset_at:  # what render_all_views reads from a training camera (renderer_cc_shadow.py:148-193), over this example's pieces
        rc = Camera(cam.affine, H, W)
        rc.image_name = "view"
        rc.altitude_bounds = torch.stack((bg[3], bg[3]))  # (the lower bound becomes the altitude background, without a readback)
        rc.UV_grid = (U, V)
        uva2sun = cam2sun.clone()
        uva2sun[:2, 2] /= 350.0  # render_all_views stacks the altitude itself, view() the altitude / 350: the same product
        rc.get_sun_camera = lambda: (sun, uva2sun)
        rc.render_pipeline = lambda raw_render, sun_altitude_diff=None: pipeline(cc_cam, raw_render, sun_altitude_diff)
        reset_cameras = [rc]
    reset_log = []  # (iteration, which reset, recordings of the step so far)
    recordings = 0
    pansharp_values = []  # --pansharp-loss: the unweighted term where the loss is read
    kept, dsm_scores = {}, []  # --dsm-mae-every: the view's altitude of the last step; (iteration, dx, dy, mae)
    first = last = None
    stopped_at = 0  # --monitor --early-stop-patience: the iteration whose record carried the flag
    main.last_monitor_record = None
    step, stale = None, False  # the recorded graph of fwd_bwd; stale: recorded for parameter tensors that a prune replaced
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t_steady = None  # (the clock of the last `timed` iterations: without the first ones, which allocate and record)
    timed = max(1, a.iters // 2)
    a_iters_asked = a.iters
    stamps = []  # host clock (before, after) the iteration's fwd_bwd or replay: what tools/step_probe.py reads
    for it in range(1, a.iters + 1):
        if it == a.iters - timed + 1:
            torch.cuda.synchronize()
            t_steady = time.perf_counter()
        if transient_weight is not None and it == a.transient_from + 1:  # iteration > iterstart_L_nll: a device write, no recording
            transient_weight.fill_(a.transient_nll)
        t_in = time.perf_counter()
        if steps_inside and it == 1:
            # the first iteration runs eagerly: it creates the optimizers' state and uploads the learning rates, which a
            # recording reads from device tensors that must exist before it
            eager_run["on"] = True
            loss, radii, vs_grad = fwd_bwd()
            eager_run["on"] = False
        elif a.graph:
            if step is None:
                from eogs2_amd.graph import GraphedStep

                step = GraphedStep(fwd_bwd, warmup=1)  # (the eager warm-up run changes nothing: no optimizer step inside)
                recordings += 1
            elif stale:
                step.record_again()  # new parameter tensors, new shapes (fwd_bwd reads them from `model`); same memory pool
                recordings += 1
            stale = False
            loss, radii, vs_grad = step()
        else:
            loss, radii, vs_grad = fwd_bwd()
        stamps.append((t_in, time.perf_counter()))
        if draws is not None and not a.quiet:  # (before anything moves the cursor or the next draw overwrites them)
            draw_log[it - 1, :3].copy_(bg[:3])
            if draw_shear is not None:
                draw_log[it - 1, 3:].copy_(draw_shear)
        if not steps_inside:
            if mon is not None:
                feed_monitor(*kept["monitor"], None)
            model.optimizer.step()
            camera_optimizer.step()
            if view_bank is not None:
                view_bank.store()
                view_schedule.advance()
            elif draw_stream is not None:
                draw_stream.advance()
        with torch.no_grad():
            if model.stats is not None:  # train_pan.py:679-690 in one launch, outside the recorded step: once per iteration
                model.stats.update(vs_grad, radii)
                if it % a.densify_every == 0:  # train_pan.py:692-711
                    if grad_threshold is None:
                        seen = model.stats.denom > 0
                        mean_norm = (model.stats.xyz_gradient_accum[seen] / model.stats.denom[seen]).double()
                        grad_threshold = float(torch.quantile(mean_norm, 0.95)) if mean_norm.numel() else math.inf
                    model.densify_and_prune(grad_threshold=grad_threshold, min_opacity=0.005, screen_size_threshold=extent,
                                            max_screen_size=None, scene_extent=extent, radii=radii)
                    keep = model._opacity.reshape(-1) >= math.log(0.005 / 0.995)
                    if not bool(keep.all()):
                        model.prune(keep)
                    stale = True  # new parameter tensors, new shapes: record again
            elif radii is not None:  # train_pan.py:681-686 (densification statistics: only with require_radii)
                model.max_radii2D = torch.maximum(model.max_radii2D, radii.float())
            if it % a.prune_every == 0 and not a.no_prune:  # train_pan.py:673-678
                keep = model._opacity.squeeze() >= min_logit
                last_point = it + a.prune_every > a.iters
                if a.defer_prune and not last_point and (it // a.prune_every) % a.defer_prune:
                    if not retire_in_step:  # (else every step has already retired them)
                        retire_rows(model.optimizer, keep)
                elif a.defer_prune:
                    alive = alive_rows(model.optimizer) & keep
                    if not bool(alive.all()):
                        model.prune(alive)
                        stale = True
                elif not bool(keep.all()):
                    model.prune(keep)
                    stale = True  # new parameter tensors, new shapes: record again
        # train_pan.py:726-736, in place: the parameters and moments the recorded step reads keep their addresses
        if a.opacity_reset_every and it % a.opacity_reset_every == 0:
            reset_opacity_(model.optimizer)
            reset_log.append((it, "opacity", recordings + (step.recaptures if step is not None else 0)))
        if a.color_reset_at and it == a.color_reset_at:
            flagged = color_reset(model, reset_cameras, pipe)
            reset_log.append((it, "color", recordings + (step.recaptures if step is not None else 0)))
            if not a.quiet:
                print(f"iter {it:4d}  colour reset: {int(flagged.sum())} of {flagged.numel()} Gaussians")
        if a.dsm_mae_every and it % a.dsm_mae_every == 0:
            if dsm_geometry is not None:  # render -> DSM -> registered MAE, all on the device
                _, pred_dsm = dsm_from_view(kept["altitude"], dsm_cam, dsm_scene, a.dsm_resolution, geometry=dsm_geometry)
                mae, _, _, (sdx, sdy, _, _) = dsm_mae(pred_dsm[:, :, 0], gt_dsm[:, :, 0], clip="finite")  # empty cells are NaN
            else:
                mae, _, _, (sdx, sdy, _, _) = dsm_mae(kept["altitude"], gt_altitude)
            dsm_scores.append((it, sdx, sdy, mae))
            if not a.quiet:
                print(f"iter {it:4d}  DSM registration dx {sdx} dy {sdy}  MAE {mae:.5f} (altitude units = {ALT_SCALE:g} x normalised z)")
        if mon is not None and it % MONITOR_INTERVAL == 0:  # train_pan.py:512-597: means, early stopper, reset; ONE wait
            mon.close_interval()
            rec = mon.fetch()
            main.last_monitor_record = rec
            if not a.quiet:
                print(f"iter {it:4d}  monitor " + "  ".join(f"{k} {v:.5g}" if isinstance(v, float) else f"{k} {v}" for k, v in rec.items()))
            if rec["early_stop"]:
                if not a.quiet:
                    print(f"iter {it:4d}  early stop: {a.early_stop_metric} has not improved on {rec['best']:.5g} for {rec['counter']} intervals")
                stopped_at = it
        if a.report_every and it % a.report_every == 0:  # train_pan.py:838-951 (its nadir DSM tail is --dsm-mae-every's)
            converter.perform_cc_to_test(train_viewpoints=train_viewpoints, test_cameras=test_viewpoints, opt=report_opt)
            for name, cameras in (("test", test_viewpoints), ("train", train_viewpoints)):
                res = evaluate_views(cameras, model, pipe, report_opt, bg.clone())
                main.last_reports.append((it, name, res))
                if not a.quiet:
                    print(f"[ITER {it}] Evaluating {name}: L1 {res['l1']} PSNR {res['psnr']}")
        if it == 1 or it % 25 == 0 or it == a.iters or stopped_at:
            v = float(loss)
            first = v if first is None else first
            last = v
            if pansharp_term is not None:
                pansharp_values.append(float(kept["pansharp"]))
            if not a.quiet:
                print(f"iter {it:4d}  loss {v:.5f}  gaussians {model._xyz.shape[0]}  device memory in use "
                      f"{(lambda f, t: (t - f) / 2**20)(*torch.cuda.mem_get_info()):.0f} MiB")
        if stopped_at:  # train_pan.py:574-578: opt.iterations = iteration
            break
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    dt = t1 - t0
    if stopped_at:  # an early stop: the clocks of the iterations that ran
        a.iters = stopped_at
        if t_steady is None:
            t_steady, timed = t0, stopped_at
        else:
            timed = stopped_at - (a_iters_asked - timed)
    main.last_ms_per_iter = (t1 - t_steady) / timed * 1e3  # steady state: the last half of the run
    main.last_dsm_mae = dsm_scores
    main.last_stamps, main.last_step = stamps, step  # (step: the GraphedStep of --graph, else None)
    # --graph: how often the step was recorded (the first recording, after a prune, after an outgrown replay), and what the
    # count was at each reset: a reset that forced a recording would show as a larger count at the end or at the next reset
    main.last_recordings = recordings + (step.recaptures if step is not None else 0)
    main.last_resets = reset_log
    main.last_pansharp_loss = (pansharp_values[0], pansharp_values[-1]) if pansharp_values else None
    main.last_params = None
    if a.densify_every or a.views > 1:  # what callers compare between runs, beside the returned tuple
        main.last_params = {g["name"]: g["params"][0].detach().cpu() for g in model.optimizer.param_groups}
    main.last_alignment = None
    if a.normalize_colors:  # train_pan.py:614-620, in place: the same Parameter at the same address, the cameras' own storage
        ref_cc = train_viewpoints[0].color_correction
        main.last_alignment = dict(f_dc_before=model._features_dc.detach().cpu().clone(), A1=ref_cc.weight.detach().cpu().reshape(3, 3).clone(),
                                   b1=ref_cc.bias.detach().cpu().clone(), data_ptr=model._features_dc.data_ptr())
        normalize_before_saving(types.SimpleNamespace(getTrainCameras=lambda: train_viewpoints), model)
        main.last_alignment["f_dc_after"] = model._features_dc.detach().cpu().clone()
        if not a.quiet:
            print("colours aligned to view 0: its colour correction is now " + " ".join(f"{x:.6g}" for x in ref_cc.weight.detach().reshape(-1).tolist())
                  + " | " + " ".join(f"{x:.6g}" for x in ref_cc.bias.detach().tolist()))
    main.last_render_set = None
    if a.render_set:  # render_pan.py:94-476 per view, render_video.py:138-164's frame
        alt = sc["means3D"] @ cam.affine[:3, 2] + cam.affine[3, 2]
        alt_min, alt_max = float(alt.min()), float(alt.max())  # (render_video.py's altitude_min / altitude_max: once)
        written = []
        for rc in train_viewpoints + test_viewpoints:
            bg_v = bg.clone()
            bg_v[3], bg_v[4] = rc.altitude_bounds[0], 0.0
            products = view_products(rc, model, pipe, bg_v)
            frame = video_frame(products["final"], products["altitude"], alt_min, alt_max)
            arrays = fetch_products(products)  # one launch, one copy
            arrays["frames"] = frame.cpu().numpy()
            for key, arr in arrays.items():
                os.makedirs(os.path.join(a.render_set, key), exist_ok=True)
                np.save(os.path.join(a.render_set, key, rc.image_name + ".npy"), arr)
                written.append((key, rc.image_name, arr.shape, str(arr.dtype)))
        main.last_render_set = written
        if not a.quiet:
            print(f"render set: {len(written)} arrays of {len(train_viewpoints) + len(test_viewpoints)} views under {a.render_set}")
    if a.save_ply:  # (after the clocks: the file is no part of an iteration)
        out_model = GaussianModel(0)
        out_model._xyz, out_model._features_dc, out_model._features_rest = model._xyz, model._features_dc, model._features_rest
        out_model._opacity, out_model._scaling, out_model._rotation = model._opacity.reshape(-1, 1), model._scaling, model._rotation
        out_model.save_ply(a.save_ply)
    if not a.quiet:
        print(f"{a.iters} iterations in {dt:.2f} s ({dt / a.iters * 1e3:.2f} ms/iter over all, {main.last_ms_per_iter:.2f} ms/iter over the "
              f"last {timed}; {3 if a.random_camera else 2} renders + resample + render pipeline + losses + Adam each)")
    main.last_transient = None
    if transient_mask is not None:  # the painted view's mask inside and outside the rectangle: printed, not judged
        painted = view_bank.row("transient_mask", 1) if view_bank is not None else transient_mask.detach()
        y0, y1, x0, x1 = transient_box
        inside = painted[y0:y1, x0:x1]
        n_in = inside.numel()
        main.last_transient = dict(weight=float(transient_weight), init=a.transient_init, box=transient_box, inside=float(inside.mean()),
                                   outside=float((painted.sum() - inside.sum()) / (painted.numel() - n_in)),
                                   stats=[float(x) for x in kept["transient"]])
        if not a.quiet:
            t = main.last_transient
            print(f"transient mask of the painted view: mean {t['inside']:.6g} inside the rectangle {transient_box}, {t['outside']:.6g} outside "
                  f"(started at {a.transient_init:g}; weight {t['weight']:g} after iteration {a.transient_from}); last iteration's mask mean "
                  f"{t['stats'][0]:.6g} std {t['stats'][1]:.6g}, {int(t['stats'][3])} pixels outside [0, 1]")
    main.last_random_camera = tuple(float(v) for v in kept["random_camera"]) if "random_camera" in kept else None
    if rc_loss is not None and not a.quiet:
        print(f"random camera: {a.random_camera_type}, target {'ground truth' if a.random_camera_gt else 'the view itself'}, sun render "
              f"{'shared' if share_sun else 'rendered twice' if a.random_camera_type == 'rawrender_wshadow' else 'not used'}; last L_new_altitude_resample "
              f"{main.last_random_camera[0]:.6g} L_new_rgb_resample {main.last_random_camera[1]:.6g}; the step was recorded {main.last_recordings} time(s)")
    main.last_draws = None
    if draws is not None and not a.quiet:
        main.last_draws = draw_log[:a.iters].cpu().tolist()
        for k, row in enumerate(main.last_draws):  # iteration k + 1 drew at index k of the stream
            print(f"draw {k:4d}  bg " + " ".join(f"{x:.9g}" for x in row[:3]) + "  shear " + " ".join(f"{x:.9g}" for x in row[3:]))
        print(f"draws: seed {a.draw_seed}, random background {'on' if a.random_background else 'off'}, virtual camera extent "
              f"{a.virtual_camera_extent}; the step was recorded {main.last_recordings} time(s)")
    return first, last, model._xyz.shape[0]


if __name__ == "__main__":
    main()
