"""ctypes prototypes for the C-ABI declared in include/*.h: one table, `HEADERS`, keyed by header file.

One `RastABI` instance wraps one loaded shared library. The product path only
ever wraps the HIP library (see `_lib.py`); tests may wrap the CPU oracle, which
exports the symbols of include/eogs_rast.h over host pointers.
"""
import ctypes as C

ABI_VERSION = 8

EOGS_OK = 0
ERR_NAMES = {
    -1: "EOGS_ERR_INVALID_ARG",
    -2: "EOGS_ERR_DEVICE",
    -3: "EOGS_ERR_WORKSPACE",
    -4: "EOGS_ERR_ALTITUDE",
    -5: "EOGS_ERR_OVERFLOW",
    -6: "EOGS_ERR_NO_COLORS",
}
FLAG_ANTIALIASING = 1
FLAG_DEBUG = 2
FLAG_RAW_PARAMS = 4
FLAG_DEFER_COUNTS = 8
FLAG_NO_READBACK = 16
FLAG_ALT_ONLY = 32  # include/eogs_rast.h EOGS_FLAG_ALT_ONLY: an altitude-only render
MIRROR_BYTES = 64
LOSS_L1 = 1
LOSS_SSIM = 2
MLOSS_SUN = 0
MLOSS_RANDOM = 1
REG_OPACITY = 1  # include/eogs_reg.h EOGS_REG_*: the `want` bits, in the order of terms[] and weights[]
REG_OPACITY_RADII = 2
REG_ERANK = 4
REG_RETIRED_BELOW = -5.0e29
PAN_ONE_CHANNEL = 0  # include/eogs_pan.h EOGS_PAN_*: the map kinds
PAN_AVERAGE = 1
PAN_FIXED = 2
PAN_BASE = 3
PAN_BASE_SIGMOID = 4
PAN_TRANSLATE = 5
PAN_TRANSLATE_FROZEN = 6
PAN_ORDER_CC_FIRST = 0  # EOGS_PAN_ORDER_*
PAN_ORDER_MAP_FIRST = 1
PAN_NPARAMS = 20
REPORT_MAX_CAMERAS = 64  # EOGS_REPORT_MAX_CAMERAS
REPORT_MAX_CC_ELEMS = 16  # EOGS_REPORT_MAX_CC_ELEMS
REPORT_MAX_ITEMS = 16  # EOGS_REPORT_MAX_ITEMS
REPORT_MAX_CHANNELS = 4  # EOGS_REPORT_MAX_CHANNELS
REPORT_PACK_MAX_CHANNELS = 5  # EOGS_REPORT_PACK_MAX_CHANNELS
REPORT_CC_REF, REPORT_CC_AVERAGE = 0, 1  # EOGS_REPORT_CC_*
REPORT_KINDS = ("pan", "msi")  # EOGS_REPORT_KIND_*: the index
REPORT_FLOAT_HWC, REPORT_U8_ROUND, REPORT_U8_TRUNC = 0, 1, 2  # EOGS_REPORT_<MODE>
REPORT_REVERSE, REPORT_REPLICATE, REPORT_PREMAP = 1, 2, 4  # the flags of an item
CMLOSS_MAX_CHANNELS = 4  # EOGS_CMLOSS_MAX_CHANNELS
DRAW_MAX_CAMERAS = 8  # EOGS_DRAW_MAX_CAMERAS
DRAW_BG, DRAW_BG_COPY_FIRST, DRAW_CAMERA, DRAW_NADIR = 1, 2, 4, 8  # EOGS_DRAW_*: the flags of a camera
VIEWS_MAX_SLOTS = 32  # EOGS_VIEWS_MAX_SLOTS
VIEWS_LOAD, VIEWS_STORE = 1, 2  # EOGS_VIEWS_LOAD, _STORE
GTPREP_BROVEY, GTPREP_SIMPLE_BROVEY, GTPREP_IHS = 0, 1, 2  # EOGS_GTPREP_<METHOD>
GTPREP_MAX_CHANNELS = 8  # EOGS_GTPREP_MAX_CHANNELS
MODEL_TILE_ROWS = 64  # EOGS_MODEL_TILE_ROWS
MODEL_MAX_REST = 15  # EOGS_MODEL_MAX_REST
RESET_MAX_VIEWS = RESET_MAX_TENSORS = 16  # EOGS_RESET_MAX_*
RESET_MAX_ROW_ELEMS = 64  # EOGS_RESET_MAX_ROW_ELEMS
RESET_TILE_H, RESET_TILE_W = 32, 64  # EOGS_RESET_TILE_*: pixels per workgroup of eogs_reset_erode
MESH_MAX_VERTICES = 1 << 29  # EOGS_MESH_MAX_VERTICES
MESH_WG_VOXELS = 256  # EOGS_MESH_WG_VOXELS
MESH_SCAN_ROUND = 256  # EOGS_MESH_SCAN_ROUND
DSM_Z_QUANTUM = 2.0 ** -20  # EOGS_DSM_Z_QUANTUM
DSM_Z_MAX = 32768.0  # EOGS_DSM_Z_MAX
DSM_MAX_RADIUS = 4  # EOGS_DSM_MAX_RADIUS
DSM_SRC_CLOUD, DSM_SRC_VIEW, DSM_SRC_GRID = 0, 1, 2  # EOGS_DSM_SRC_*
MONITOR_RING = 16  # EOGS_MONITOR_RING
MONITOR_METRICS = ("photometric", "L1", "pan_psnr", "pan_ssim", "msi_psnr", "msi_ssim")  # EOGS_MONITOR_<NAME>: the index
MONITOR_KINDS = ("pan", "msi")  # EOGS_MONITOR_KIND_*
MONITOR_OPERATORS = ("min", "max")  # EOGS_MONITOR_MIN, _MAX
STEP_MAX_FORWARDS = STEP_MAX_TENSORS = 16  # EOGS_STEP_MAX_*
DENSITY_CLONE, DENSITY_SPLIT, DENSITY_PRUNE_SELF, DENSITY_PRUNE_SAMP = 1, 2, 4, 8  # EOGS_DENSITY_*: the flag byte
DENSITY_COPY, DENSITY_ZERO, DENSITY_XYZ, DENSITY_SCALING = 0, 1, 2, 3  # the tensor kinds of eogs_density_build
DENSITY_MAX_N = 8
NLL_MASK, NLL_FULL, NLL_SUM = 1, 2, 4  # include/eogs_nll.h EOGS_NLL_*: the mode bits
RAFT_MAX_LEVELS, RAFT_MAX_RADIUS = 4, 4  # include/eogs_resample.h EOGS_RAFT_MAX_*
RAFT_NO_STAGE = 1  # EOGS_RAFT_NO_STAGE: the lookup's flag
RAFT_UP_CONVEX, RAFT_UP_BILINEAR = 0, 1  # EOGS_RAFT_UP_*: the upsampling modes
RAFT_MASK_CHANNELS = 576  # EOGS_RAFT_MASK_CHANNELS
FLOWNET_MAX_SEGMENTS, FLOWNET_MAX_KERNEL = 3, 7  # EOGS_FLOWNET_MAX_*
FLOWNET_EPI_BIAS, FLOWNET_EPI_RELU, FLOWNET_EPI_GATES, FLOWNET_EPI_GRU = 0, 1, 2, 3  # EOGS_FLOWNET_EPI_*: the epilogues
FLOWNET_IN0_NCHW, FLOWNET_OUT_NCHW = 1, 8  # EOGS_FLOWNET_IN0_NCHW (<< i for segment i), _OUT_NCHW: the convolution's flags
FLOWNET_UPDATE_PARAMS = 18  # EOGS_FLOWNET_UPDATE_PARAMS
FLOWRECT_EPI_QUARTER = 4  # include/eogs_resample.h EOGS_FLOWRECT_EPI_QUARTER: the rectangular convolution's added epilogue
FLOWLARGE_PARAMS = 30  # EOGS_FLOWLARGE_PARAMS
FLOWRECT_TAP_SHAPES = ((1, 1), (3, 3), (5, 5), (7, 7), (1, 5), (5, 1))  # the (kh, kw) eogs_flowrect_conv takes
FLOWENC_EPI_BIAS, FLOWENC_EPI_RELU, FLOWENC_EPI_RESIDUAL = 0, 1, 2  # EOGS_FLOWENC_EPI_*: the strided convolution's epilogues
FLOWENC_IN_NCHW, FLOWENC_OUT_NCHW = 1, 8  # EOGS_FLOWENC_IN_NCHW, _OUT_NCHW: its flags
FLOWENC_SHORTCUT_NONE, FLOWENC_SHORTCUT_PLAIN, FLOWENC_SHORTCUT_NORM = 0, 1, 2  # EOGS_FLOWENC_SHORTCUT_*: eogs_flowenc_finish
FLOWENC_FEATURE, FLOWENC_CONTEXT = 0, 1  # EOGS_FLOWENC_FEATURE, _CONTEXT: the encoder kinds
FLOWENC_PARAMS = 44  # EOGS_FLOWENC_PARAMS
FLOWRES_PARAMS, FLOWRES_BN = 32, 60  # EOGS_FLOWRES_PARAMS, _BN: RAFT-large's encoders, (weight, bias) x 16 and (gamma, beta, mean, var) x 15

_p = C.c_void_p
_i = C.c_int
_f = C.c_float
_u = C.c_uint
_z = C.c_size_t
_i64 = C.c_int64

# header -> name -> (restype, argtypes), every header of include/ in the order of its declarations. The one table:
# tests/test_abi.py holds it against the headers and the built library, symbol by symbol.
HEADERS = {
    "eogs_rast.h": {
        "eogs_rast_last_error": (C.c_char_p, []),
        "eogs_rast_abi_version": (_i, []),
        "eogs_rast_backend": (C.c_char_p, []),
        "eogs_rast_geom_bytes": (_i, [_i, C.POINTER(_z)]),
        "eogs_rast_image_bytes": (_i, [_i, _i, C.POINTER(_z)]),
        "eogs_rast_binning_bytes": (_i, [_i, _i, _i, _i64, C.POINTER(_z)]),
        "eogs_rast_scratch_bytes": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_rast_forward_prepare": (
            _i,
            [_i, _i, _i, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _u, _p, _p, _z, _p, _z, C.POINTER(_i64), _p],
        ),
        "eogs_rast_forward_counts": (_i, [C.POINTER(_i64)]),
        "eogs_rast_read_counts": (_i, [_i, _i, _i, _p, _z, _i, _p, C.POINTER(_i64)]),
        "eogs_rast_mirror_arm": (_i, [_p]),
        "eogs_rast_mirror_counts": (_i, [_i, _p, _z, _p, _p]),
        "eogs_rast_mirror_token": (_i, [_i, _i, _i, _p, _i, C.POINTER(_i64), C.POINTER(_i)]),
        "eogs_rast_capacity_token": (_i, [_i, _i64, C.c_double, _i, _i64, C.POINTER(_i64), C.POINTER(_i)]),
        "eogs_rast_forward_render": (
            _i,
            [_i, _i, _i, _i64, _p, _u, _p, _z, _p, _z, _p, _z, _p, _z, _p, _p, _p],
        ),
        "eogs_rast_backward": (
            _i,
            [_i, _i, _i, _i64]
            + [_p] * 7  # bg, means3D, radii, colors, opacities, scales, rotations
            + [_f, _p, _p, _p, _p, _u]  # scale_modifier, cov3D_precomp, viewmatrix, projmatrix, alt_affine, flags
            + [_p] * 4  # out_color, out_invdepth, dL_dout_color, dL_dout_invdepth
            + [_p, _z, _p, _z, _p, _z]  # geom, binning, image workspaces
            + [_p] * 9  # 7 gradients + dL_dT_sum + dL_dvm_mean
            + [_p, _i]  # dL_dcolors_lead, lead_cols
            + [_p],  # stream
        ),
        "eogs_rast_backward_range": (
            _i,
            [_i, _i, _i, _i64]
            + [_p] * 7
            + [_f, _p, _p, _p, _p, _u]
            + [_p] * 4
            + [_p, _z, _p, _z, _p, _z]
            + [_p] * 9
            + [_p, _i]  # dL_dcolors_lead, lead_cols
            + [_i, _i]  # p_begin, p_end
            + [_p],
        ),
        "eogs_rast_mark_visible": (_i, [_i, _p, _p, _p, _p, _p]),
        "eogs_rast_path_info": (_i, [_i, _i64, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
        "eogs_rast_backward_info": (_i, [_i, _i64, C.POINTER(_i)]),
        "eogs_rast_profile_enable": (_i, [_i]),
        "eogs_rast_profile_select": (_i, [_u]),
        "eogs_rast_profile_reset": (_i, []),
        "eogs_rast_profile_slots": (_i, []),
        "eogs_rast_profile_get": (_i, [_i, C.POINTER(C.c_double), C.POINTER(_i64), C.POINTER(C.c_char_p)]),
        "eogs_rast_selftest": (_i, [_p, C.POINTER(_u), _p]),
    },
    "eogs_loss.h": {
        "eogs_loss_bytes": (_i, [_i, _i, _i, _u, C.POINTER(_z)]),
        "eogs_loss_tile_shape": (_i, [C.POINTER(_i), C.POINTER(_i)]),
        "eogs_loss_window": (_i, [C.POINTER(C.c_float)]),
        "eogs_loss_forward": (_i, [_i, _i, _i, _p, _p, _u, _f, _f, _f, _p, _p, _p, _z, _p]),
        "eogs_loss_backward": (_i, [_i, _i, _i, _p, _p, _u, _f, _f, _p, _p, _p, _z, _p, _p]),
    },
    "eogs_optim.h": {
        "eogs_adam_step": (_i, [_i, _p, C.c_double, C.c_double, C.c_double, _i64, _p]),
        "eogs_sum_into": (_i, [_i, _p, _i, _p]),
        "eogs_pack_columns": (_i, [_i64, _i, _p, _p, _i, _i, _p]),
        "eogs_compact_bytes": (_i, [_i64, C.POINTER(_z)]),
        "eogs_compact_plan": (_i, [_i64, _p, _p, _z, C.POINTER(_i64), _p]),
        "eogs_compact_apply": (_i, [_i64, _p, _i, _p, _p, _p, _p, _z, _p]),
    },
    "eogs_resample.h": {
        "eogs_resample_forward": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p, _i, _f, _p, _p, _p]),
        "eogs_resample_bytes": (_i, [_i, _i, C.POINTER(_z)]),
        "eogs_resample_backward": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _p, _p, _z, _p]),
        # the flow-matching warp
        "eogs_resample_flow_forward": (_i, [_i, _i, _i, _p, _p, _i64, _i64, _i64, _p, _p, _p]),
        "eogs_resample_flow_bytes": (_i, [_i, _i, C.POINTER(_z)]),
        "eogs_resample_flow_backward": (_i, [_i, _i, _i, _p, _i64, _i64, _i64, _p, _p, _p, _p, _z, _p]),
        "eogs_resample_flow_stats_bytes": (_i, [_i, _i, C.POINTER(_z)]),
        "eogs_resample_flow_stats": (_i, [_i, _i, _p, _i64, _i64, _i64, _p, _p, _z, _p]),
        # the flow network (RAFT): feature pyramid, on-demand correlation lookup, flow upsampling
        "eogs_raft_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(_z)]),
        "eogs_raft_level_offset": (_i, [_i, _i, _i, _i, _i, C.POINTER(_z)]),
        "eogs_raft_pyramid": (_i, [_i, _i, _i, _i, _i, _p, _p, _z, _p]),
        "eogs_raft_lookup": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _u, _p]),
        "eogs_raft_stage_info": (_i, [C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
        "eogs_raft_upsample": (_i, [_i, _i, _i, _i, _p, _p, _p, _p]),
        # the flow network's update block: the channel-last convolution and RAFT-small's step composed of it
        "eogs_flownet_conv_info": (_i, [C.POINTER(_i), C.POINTER(_i)]),
        "eogs_flownet_conv_pack_bytes": (_i, [_i, _i, C.POINTER(_i), _i, C.POINTER(_z)]),
        "eogs_flownet_conv_pack": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_i), _i, _i, _i, _i, _p, _p, _z, _p]),
        "eogs_flownet_conv": (_i, [_i, _i, _i, _i, _i, C.POINTER(_i), _p, _p, _p, _i, _p, _z, _p, _p, _p, _p, _i, _u, _p]),
        "eogs_flownet_update_bytes": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_flownet_update_hidden_offset": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_flownet_update_begin": (_i, [_i, _i, _i, C.POINTER(_p), _p, _p, _p, _z, _p]),
        "eogs_flownet_update_step": (_i, [_i, _i, _i, _p, _p, _p, _z, _p, _p]),
        # the flow network's convolution over kh x kw taps, and RAFT-large's update block and mask predictor composed of it
        "eogs_flowrect_pack_bytes": (_i, [_i, _i, _i, C.POINTER(_i), _i, C.POINTER(_z)]),
        "eogs_flowrect_pack": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i), _i, _i, _i, _i, _p, _p, _z, _p]),
        "eogs_flowrect_conv": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_i), _p, _p, _p, _i, _p, _z, _p, _p, _p, _p, _i, _u, _p]),
        "eogs_flowlarge_bytes": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_flowlarge_hidden_offset": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_flowlarge_begin": (_i, [_i, _i, _i, C.POINTER(_p), _p, _p, _p, _z, _p]),
        "eogs_flowlarge_step": (_i, [_i, _i, _i, _p, _p, _p, _z, _p, _p]),
        "eogs_flowlarge_mask": (_i, [_i, _i, _i, _p, _z, _p, _p]),
        "eogs_flowenc_conv_partials": (_i, [_i, _i, _i, _i, C.POINTER(_i), C.POINTER(_z)]),
        "eogs_flowenc_conv": (_i, [_i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _z, _p, _p, _p, _p, _z, _i, _u, _p]),
        "eogs_flowenc_norm": (_i, [_i, _i, _i, _i, _p, _z, _p, _p]),
        "eogs_flowenc_finish": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _p]),
        "eogs_flowenc_bytes": (_i, [_i, _i, _i, _i, C.POINTER(_z)]),
        "eogs_flowenc_run": (_i, [_i, _i, _i, _i, C.POINTER(_p), _p, _p, _z, _p, _p]),
        "eogs_flowres_fold": (_i, [_i, _i, _p, _p, _p, _p, _p, _p, C.c_double, _p, _p, _p]),
        "eogs_flowres_bytes": (_i, [_i, _i, _i, _i, C.POINTER(_z)]),
        "eogs_flowres_run": (_i, [_i, _i, _i, _i, C.POINTER(_p), C.POINTER(_p), _p, _p, _z, _p, _p]),
    },
    "eogs_knn.h": {
        "eogs_knn_bytes": (_i, [_i, C.POINTER(_z)]),
        "eogs_knn_mean_dist2": (_i, [_i, _p, _p, _p, _z, _p]),
    },
    "eogs_shade.h": {
        "eogs_shade_bytes": (_i, [_i, _i, C.POINTER(_z)]),
        "eogs_shade_forward": (_i, [_i, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
        "eogs_shade_backward": (_i, [_i, _i] + [_p] * 10 + [_p, _z, _p]),
        "eogs_mloss_forward": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _p, _z, _p]),
        "eogs_mloss_backward": (_i, [_i, _i, _i] + [_p] * 9 + [_p]),
        "eogs_tshadow_forward": (_i, [_i64, _p, _p, _p, _z, _p]),
        "eogs_tshadow_backward": (_i, [_i64, _p, _p, _p, _p]),
    },
    "eogs_tsdf.h": {
        "eogs_tsdf_integrate": (_i, [_i, _i, _i, _p, _p, _p, _p, _f, _f, _i, _i, _p, _p, _p, _p, _p]),
        "eogs_tsdf_normals": (_i, [_i, _i, _p, _p, _p, _p, _p, _p, _p]),
        "eogs_tsdf_prior_bytes": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_tsdf_prior": (_i, [_i, _i, _i, _p, _p, _p, _z, _p]),
        "eogs_tsdf_surface": (_i, [_i, _i, _i, _p, _p, _p, _p, _p]),
        # DSM evaluation
        "eogs_tsdf_dsm_downsample": (_i, [_i, _i, _p, _i, _p, _p]),
        "eogs_tsdf_dsm_ncc_bytes": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_tsdf_dsm_ncc": (_i, [_i, _i, _p, _i, _i, _p, _i, _i, _p, _i, _p, _p, _p, _z, _p]),
        "eogs_tsdf_dsm_shift_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(_z), C.POINTER(_i)]),
        "eogs_tsdf_dsm_shift": (_i, [_i, _i, _p, _i, _i, _p, _i, _i, _p, _p, _p, _z, _p]),
        "eogs_tsdf_dsm_apply_shift": (_i, [_i, _i, _p, _i, _i, _i, C.c_double, C.c_double, C.c_double, C.c_double, _p, _p]),
        "eogs_tsdf_dsm_mae_bytes": (_i, [C.POINTER(_z)]),
        "eogs_tsdf_dsm_mae": (_i, [_i, _i, _p, _i, _i, _p, _i, _i, _p, _p, _p, _z, _p]),
    },
    "eogs_reg.h": {
        "eogs_reg_gauss_bytes": (_i, [_i64, C.POINTER(_z)]),
        "eogs_reg_gauss_forward": (_i, [_i64, _u, _p, _p, _p, _f, _p, _p, _p, _z, _p]),
        "eogs_reg_gauss_backward": (_i, [_i64, _u, _p, _p, _p, _f] + [_p] * 6 + [_p]),
        "eogs_reg_image_bytes": (_i, [_i, _i, C.POINTER(_z)]),
        "eogs_reg_image_forward": (_i, [_i, _i, _p, _p, _p, _p, _p, _z, _p]),
        "eogs_reg_image_backward": (_i, [_i, _i] + [_p] * 7 + [_p]),
    },
    "eogs_pan.h": {
        "eogs_pan_bytes": (_i, [_i, _i, C.POINTER(_z)]),
        "eogs_pan_forward": (_i, [_i, _i, _i, _i] + [_p] * 8 + [_p]),
        "eogs_pan_backward": (_i, [_i, _i, _i, _i] + [_p] * 11 + [_p, _z, _p]),
    },
    "eogs_density.h": {
        "eogs_density_stats_update": (_i, [_i64, _p, _p, _i, _p, _p, _p, _p]),
        "eogs_density_bytes": (_i, [_i64, C.POINTER(_z)]),
        "eogs_density_decide": (_i, [_i64, _p, _p, _p, _p, _f, _f, _f, _i, _f, _f, _p, _p, _z, C.POINTER(_i64), _p]),
        "eogs_density_split_rows": (_i, [_i64, _p, _p, _p, _i, _p, _z, _p]),
        "eogs_density_build": (_i, [_i64, _i, _p, C.POINTER(_i64), _i, _p, _p, _p, _f, _p, _z, _p]),
    },
    "eogs_step.h": {
        "eogs_step_gate": (_i, [_i, _p, _i, _p, _p]),
        "eogs_step_adam_bytes": (_i, [_i, C.POINTER(_z)]),
        "eogs_step_adam": (_i, [_i, _p, C.c_double, C.c_double, C.c_double, _p, _p, _z, _p]),
    },
    "eogs_monitor.h": {
        "eogs_monitor_state_bytes": (_i, [C.POINTER(_z)]),
        "eogs_monitor_reset": (_i, [_p, _z, _i, _p]),
        "eogs_monitor_observe_bytes": (_i, [_i, _i, _i, _i, C.POINTER(_z)]),
        "eogs_monitor_observe": (_i, [_i, _i, _i, _p, _p, _p, C.c_double, _i, _i, _p, _p, _p, _z, _p]),
        "eogs_monitor_model_bytes": (_i, [_i64, C.POINTER(_z)]),
        "eogs_monitor_observe_model": (_i, [_i64, _p, _p, _p, _p, _z, _p]),
        "eogs_monitor_end_iteration": (_i, [_p, _p, _p, _p]),
        "eogs_monitor_close_interval": (_i, [_i, _i, _i64, _p, _p, _p]),
    },
    "eogs_dsm.h": {
        "eogs_dsm_bounds_bytes": (_i, [C.POINTER(_z)]),
        "eogs_dsm_bounds": (_i, [_p, _p, _p, _z, _p]),
        "eogs_dsm_raster_bytes": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_dsm_raster": (_i, [_p, C.c_double, C.c_double, C.c_double, _i, _i, _i, _p, _p, _p, _p, _z, _p]),
    },
    "eogs_mesh.h": {
        "eogs_mesh_bytes": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_mesh_count": (_i, [_i, _i, _i, _p, C.c_double, _p, _z, _p, _p]),
        "eogs_mesh_emit": (_i, [_i, _i, _i, _p, C.c_double, _p, _p, _p, C.POINTER(C.c_double), _p, _z, _p, _i64, _p, _i64, _p]),
        "eogs_mesh_case": (_i, [_i, C.POINTER(C.c_int8), C.POINTER(_i)]),
    },
    "eogs_reset.h": {
        "eogs_reset_erode": (_i, [_i, _i, _p, _p, _p]),
        "eogs_reset_flags": (_i, [_i64, _p, _p, _f, _i, _p, _i, _p, _p]),
        "eogs_reset_rows": (_i, [_i64, _p, _i, _p, _p]),
        "eogs_reset_opacity_cap": (_i, [_i64, _p, _p, _p, _f, _f, _p]),
    },
    "eogs_model.h": {
        "eogs_model_init": (_i, [_i64, _i, _p, _p, _p, _f] + [_p] * 7 + [_p]),
        "eogs_model_rows_pack": (_i, [_i64, _i] + [_p] * 6 + [_p, _p]),
        "eogs_model_rows_unpack": (_i, [_i64, _i, _p] + [_p] * 6 + [_p]),
    },
    "eogs_gtprep.h": {
        "eogs_gtprep_bytes": (_i, [_i, C.POINTER(_z)]),
        "eogs_gtprep_pansharp": (_i, [_i] * 6 + [_p, _p, _f, _p, _p]),
        "eogs_gtprep_pansharp_l2_forward": (_i, [_i] * 6 + [_p, _p, _p, _f, _p, _p, _z, _p]),
        "eogs_gtprep_pansharp_l2_backward": (_i, [_i] * 6 + [_p, _p, _p, _f, _p, _p, _p]),
        "eogs_gtprep_l2_forward": (_i, [_i64, _p, _p, _p, _p, _z, _p]),
        "eogs_gtprep_l2_backward": (_i, [_i64, _p, _p, _p, _p, _p]),
        "eogs_gtprep_grad_l2_forward": (_i, [_i64, _i, _i, _p, _p, _p, _p, _z, _p]),
        "eogs_gtprep_grad_l2_backward": (_i, [_i64, _i, _i, _p, _p, _p, _p, _p]),
        "eogs_gtprep_minmax": (_i, [_i, _i64, _p, _p, _p, _z, _p]),
        "eogs_gtprep_rescale": (_i, [_i, _i64, _p, _p, _p, _p]),
        "eogs_gtprep_clamp": (_i, [_i64, _p, _f, _f, _p, _p]),
        "eogs_gtprep_equalize": (_i, [_i, _i64, _p, _p, _p, _z, _p]),
    },
    "eogs_views.h": {
        "eogs_views_wg_bytes": (_i, [C.POINTER(_z)]),
        "eogs_views_load": (_i, [_i, _p, _p, _p]),
        "eogs_views_store": (_i, [_i, _p, _p, _p, _p]),
        "eogs_views_advance": (_i, [_p, _p, _p]),
    },
    "eogs_draw.h": {
        "eogs_draw_iteration": (_i, [_i, _p, _p, _p]),
        "eogs_draw_advance": (_i, [_p, _p, _p]),
    },
    "eogs_randomcam.h": {
        "eogs_randomcam_compose": (_i, [_p, _p, _p, _p]),
        "eogs_cmloss_bytes": (_i, [_i, _i, C.POINTER(_z)]),
        "eogs_cmloss_forward": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _p, _z, _p]),
        "eogs_cmloss_backward": (_i, [_i, _i, _i] + [_p] * 9 + [_p]),
    },
    "eogs_report.h": {
        "eogs_report_normalize_rows": (_i, [_i64, _p, _p, _p, _p]),
        "eogs_report_recompose": (_i, [_i, _p, _p, _p, _p]),
        "eogs_report_cc_to_test": (_i, [_i, _i, _p, _i, _p, _i, _i, _p]),
        "eogs_report_metrics_bytes": (_i, [C.POINTER(_z)]),
        "eogs_report_metrics_reset": (_i, [_p, _p]),
        "eogs_report_metrics_accumulate": (_i, [_i, _i, _i, _p, _p, _i, _p, _p, _p, _z, _p]),
        "eogs_report_pack": (_i, [_i, _p, _p, _z, _p]),
    },
    "eogs_nll.h": {
        "eogs_nll_bytes": (_i, [_i, _i, _i, C.POINTER(_z)]),
        "eogs_nll_forward": (_i, [_i, _i, _i, _u, _p, _p, _p, _i, _f, _f, _p, _p, _p, _z, _p]),
        "eogs_nll_backward": (_i, [_i, _i, _i, _u, _p, _p, _p, _i, _f, _f] + [_p] * 5 + [_p]),
    },
}
# name -> (restype, argtypes) of every header
SIGNATURES = {name: sig for table in HEADERS.values() for name, sig in table.items()}
# symbols only the HIP library exports: the CPU oracle is the twin of include/eogs_rast.h alone (the oracle of the loss, say,
# is oracle/loss_oracle.py, not a C-ABI twin)
HIP_ONLY = tuple(name for name in SIGNATURES if name not in HEADERS["eogs_rast.h"])


class PackTensor(C.Structure):
    """eogs_pack_tensor (include/eogs_optim.h)"""

    _fields_ = [("data", _p), ("width", _i), ("col0", _i), ("ncols", _i)]


class SumTensor(C.Structure):
    """eogs_sum_tensor (include/eogs_optim.h)"""

    _fields_ = [("dst", _p), ("src", _p * 4), ("numel", _i64)]


class DensityTensor(C.Structure):
    """eogs_density_tensor (include/eogs_density.h)"""

    _fields_ = [("src", _p), ("dst", _p), ("row_bytes", _i), ("kind", _i)]


class AdamTensor(C.Structure):
    """eogs_adam_tensor (include/eogs_optim.h)"""

    _fields_ = [("param", _p), ("grad", _p), ("exp_avg", _p), ("exp_avg_sq", _p), ("numel", _i64), ("lr", _f)]


class StepForward(C.Structure):
    """eogs_step_forward (include/eogs_step.h)"""

    _fields_ = [("geom", _p), ("geom_bytes", _z), ("P", _i), ("capacity", _i64)]


class StepAdamTensor(C.Structure):
    """eogs_step_adam_tensor (include/eogs_step.h)"""

    _fields_ = [("param", _p), ("grad", _p), ("exp_avg", _p), ("exp_avg_sq", _p), ("numel", _i64), ("lr", _p), ("step", _p),
                ("retire_below", _f)]


class StepAdamScalars(C.Structure):
    """eogs_step_adam_scalars (include/eogs_step.h): one row of the prologue's table"""

    _fields_ = [("lr", _f), ("inv_bc1", _f), ("sqrt_bc2", _f), ("skip", _f)]


class MonitorRecord(C.Structure):
    """eogs_monitor_record (include/eogs_monitor.h)"""

    _fields_ = [("interval", _i64), ("iteration", _i64), ("means", C.c_double * 6), ("ema_loss", C.c_double),
                ("ema_photometric", C.c_double), ("mean_opacity", C.c_double), ("rows", _i64), ("best", C.c_double),
                ("counter", _i64), ("early_stop", _i64), ("reserved", _i64)]


class MonitorState(C.Structure):
    """eogs_monitor_state (include/eogs_monitor.h)"""

    _fields_ = [("sums", C.c_double * 6), ("n_photo", _i64), ("n_pan", _i64), ("n_msi", _i64), ("ema_loss", C.c_double),
                ("ema_photometric", C.c_double), ("iteration", _i64), ("best", C.c_double), ("counter", _i64), ("early_stop", _i64),
                ("intervals", _i64), ("last", _f * 4), ("mean_opacity", _f), ("reserved0", _f), ("rows", _i64), ("reserved1", _i64),
                ("latest", MonitorRecord), ("ring", MonitorRecord * MONITOR_RING)]


class DsmSource(C.Structure):
    """eogs_dsm_source (include/eogs_dsm.h)"""

    _fields_ = [("kind", _i), ("H", _i), ("W", _i), ("N", _i64), ("cloud", _p), ("altitude", _p), ("u_axis", _p), ("v_axis", _p),
                ("affine", _p), ("scale", C.c_double), ("shift", C.c_double * 3)]


class DsmBounds(C.Structure):
    """eogs_dsm_bounds_result (include/eogs_dsm.h)"""

    _fields_ = [("xmin", C.c_double), ("xmax", C.c_double), ("ymin", C.c_double), ("ymax", C.c_double), ("nonfinite", _i64),
                ("count", _i64)]


class ResetView(C.Structure):
    """eogs_reset_view (include/eogs_reset.h)"""

    _fields_ = [("eroded", _p), ("affine", _p), ("H", _i), ("W", _i)]


class ResetTensor(C.Structure):
    """eogs_reset_tensor (include/eogs_reset.h)"""

    _fields_ = [("data", _p), ("row_elems", _i), ("value", _f)]


class ViewsSlot(C.Structure):
    """eogs_views_slot (include/eogs_views.h)"""

    _fields_ = [("table", _p), ("working", _p), ("row_stride", _z), ("row_bytes", _z), ("flags", C.c_uint32)]


class ViewsSchedule(C.Structure):
    """eogs_views_schedule (include/eogs_views.h)"""

    _fields_ = [("order", _p), ("order_len", _i64), ("cursor", _p), ("current", _p), ("n_views", C.c_int32)]


class DrawStreamDesc(C.Structure):
    """eogs_draw_stream (include/eogs_draw.h)"""

    _fields_ = [("seed", C.c_uint64), ("counter", _p)]


class DrawCamera(C.Structure):
    """eogs_draw_camera (include/eogs_draw.h)"""

    _fields_ = [("affine", _p), ("center", _p), ("alt_floor", _p), ("bg", _p), ("virt_affine", _p), ("cam2virt", _p), ("shear", _p),
                ("extent", _f), ("cam2virt_scale", _f), ("flags", C.c_uint32)]


class ReportCamera(C.Structure):
    """eogs_report_camera (include/eogs_report.h)"""

    _fields_ = [("weight", _p), ("bias", _p)]


class ReportTable(C.Structure):
    """eogs_report_table (include/eogs_report.h)"""

    _fields_ = [("l1", C.c_double * 2), ("psnr", C.c_double * 2), ("views", _i64 * 2), ("last_l1", _f), ("last_psnr", _f),
                ("reserved", _i64)]


class ReportItem(C.Structure):
    """eogs_report_item (include/eogs_report.h)"""

    _fields_ = [("src", _p), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("mode", C.c_int32), ("dst_offset", C.c_uint64),
                ("dst_pitch", C.c_uint64), ("flags", C.c_uint32), ("lo", _f), ("d", _f)]


class RastError(RuntimeError):
    """A C-ABI call returned a negative status."""

    def __init__(self, code, message):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {message}")
        self.code = code


class RastABI:
    def __init__(self, path):
        self.path = str(path)
        self.cdll = C.CDLL(self.path)
        self.cdll.eogs_rast_backend.restype = C.c_char_p
        oracle_lib = self.cdll.eogs_rast_backend().decode() == "cpu-oracle"
        for name, (res, args) in SIGNATURES.items():
            if oracle_lib and name in HIP_ONLY:
                continue
            fn = getattr(self.cdll, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        v = self.cdll.eogs_rast_abi_version()
        if v != ABI_VERSION:
            raise RuntimeError(f"{path}: ABI version {v}, expected {ABI_VERSION}")
        self.backend = self.cdll.eogs_rast_backend().decode()
        # which torch device type this library's pointers live on
        self.device_type = "cpu" if self.backend == "cpu-oracle" else "cuda"

    def check(self, code):
        if code != EOGS_OK:
            raise RastError(code, self.cdll.eogs_rast_last_error().decode())

    def __getattr__(self, name):
        """`abi.loss_forward` is eogs_loss_forward, `abi.geom_bytes` eogs_rast_geom_bytes: a name the table holds behind
        "eogs_", else the rasterizer's. Kept on the instance, so this runs once per name."""
        full = "eogs_" + name
        fn = getattr(self.cdll, full if full in SIGNATURES else "eogs_rast_" + name)
        setattr(self, name, fn)
        return fn

    def path_info(self, P, num_rendered):
        """(list block in pixels, forward kernel variant, backward kernel variant) of a forward (include/eogs_rast.h)."""
        b, f, w = _i(), _i(), _i()
        self.check(self.cdll.eogs_rast_path_info(int(P), int(num_rendered), C.byref(b), C.byref(f), C.byref(w)))
        return b.value, f.value, w.value

    def backward_info(self, P, num_rendered):
        """Which build of the per-Gaussian backward kernel a backward of this token would launch now (include/eogs_rast.h)."""
        w = _i()
        self.check(self.cdll.eogs_rast_backward_info(int(P), int(num_rendered), C.byref(w)))
        return w.value

    def profile_slot_names(self):
        names = []
        for i in range(self.cdll.eogs_rast_profile_slots()):
            ms, n, nm = C.c_double(), _i64(), C.c_char_p()
            self.check(self.cdll.eogs_rast_profile_get(i, C.byref(ms), C.byref(n), C.byref(nm)))
            names.append(nm.value.decode())
        return names

    def profile(self):
        """{group name: (total device ms, launches)} accumulated since the last profile_reset()."""
        out = {}
        for i in range(self.cdll.eogs_rast_profile_slots()):
            ms, n, nm = C.c_double(), _i64(), C.c_char_p()
            self.check(self.cdll.eogs_rast_profile_get(i, C.byref(ms), C.byref(n), C.byref(nm)))
            out[nm.value.decode()] = (ms.value, n.value)
        return out
