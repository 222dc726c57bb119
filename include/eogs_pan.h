/*
 * eogs_pan.h — C-ABI of the panchromatic camera's render pipeline: colour correction, shadow and the MSI->PAN map in
 * one forward and one backward kernel (plus the fixed-order reduction of the parameter gradients), where the reference
 * runs 15-25 elementwise PyTorch kernels and autograd replays them:
 *
 *   PANAffineCamera._render_pipeline         src/gaussiansplatting/scene/cameras/PAN_affine_cameras.py:83-146
 *   PANAffineCamera._render_pipeline_weird   scene/cameras/PAN_affine_cameras.py:148-176
 *   ShadowMap.forward                        scene/cameras/affine_cameras.py:33-40
 *   the maps of load_msi_to_pan              scene/msi_to_pan/transf_msi_to_pan.py:189-222
 *
 * Same conventions as eogs_shade.h: plain DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status
 * (0 ok, <0 error, message via eogs_rast_last_error()), the library never allocates device memory. Images are
 * contiguous fp32 planes [C][H][W]. Every sum is reduced per workgroup and then in a fixed order (no atomics): results
 * are bitwise reproducible. Planes are read and written 16 bytes at a time when H*W is a multiple of 4 and every image
 * pointer is 16-byte aligned, 4 bytes at a time otherwise; the results are the same bits either way per pixel.
 */
#ifndef EOGS_PAN_H_INCLUDED
#define EOGS_PAN_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the per-pixel MSI->PAN maps x[3] -> pan, with their parameter array map_params (f32, device) ------------------
 *   ONE_CHANNEL       x[0]                                        only_one_channel, transf_msi_to_pan.py:52-59; no params
 *   AVERAGE           (x[0] + x[1] + x[2]) / 3                    average_msitopan, :27-37; no params
 *   FIXED             p[3] (p[0] x[0] + p[1] x[1] + p[2] x[2] + p[4])     base_msi_to_pan and learnable_base_msi_to_pan,
 *                                                                 :5-24, :62-84; map_params = p[5]
 *   BASE              w[0] x[0] + w[1] x[1] + w[2] x[2] + b       MSI_TO_PAN with kernel_size 1 and remove_sigm, :87-131;
 *   BASE_SIGMOID      sigmoid(the same)                           map_params = {w[3], b}
 *   TRANSLATE         y + (w . x + b),  y = fw . x + fb           msi_to_pan_fixedandtranslate with learn_conv2d, :134-178;
 *                                                                 map_params = {fw[3], fb, w[3], b}. y is a constant of
 *                                                                 the backward (torch.no_grad, :167-170): the gradient
 *                                                                 flows through w . x + b only.
 *   TRANSLATE_FROZEN  y                                           the same module without learn_conv2d (:176-177):
 *                                                                 map_params = {fw[3], fb}; no gradient passes the map. */
#define EOGS_PAN_ONE_CHANNEL 0
#define EOGS_PAN_AVERAGE 1
#define EOGS_PAN_FIXED 2
#define EOGS_PAN_BASE 3
#define EOGS_PAN_BASE_SIGMOID 4
#define EOGS_PAN_TRANSLATE 5
#define EOGS_PAN_TRANSLATE_FROZEN 6

/* ---- the two orders of the pipeline -------------------------------------------------------------------------------
 * shadow = exp(0.4 * min(alt_diff, 0)), only when alt_diff != NULL (ShadowMap, affine_cameras.py:33-40).
 *
 * EOGS_PAN_ORDER_CC_FIRST (PAN_affine_cameras.py:83-146): M f32[3][4] row-major, inshadow f32[3]
 *   cc[c]      = M[c][0] raw[0] + M[c][1] raw[1] + M[c][2] raw[2] + M[c][3]            f32[3][H][W]  (:93-109)
 *   shaded3[c] = shadow cc[c] + (1 - shadow) inshadow[c] cc[c]   (= cc[c] when alt_diff == NULL)      (:114-121)
 *   shaded     = map(shaded3)                                                          f32[H][W]     (:129)
 *
 * EOGS_PAN_ORDER_MAP_FIRST (`weird_pan_setup`, PAN_affine_cameras.py:148-176): M f32[2] = {w, b} of the Conv2d(1,1,1),
 * inshadow f32[1]
 *   p0     = map(raw)                                                                                (:151)
 *   cc     = w p0 + b                                                                  f32[H][W]     (:157)
 *   shaded = shadow cc + (1 - shadow) inshadow cc                                      f32[H][W]     (:160-164)
 *   shaded = p0 when alt_diff == NULL: NOT cc. The reference keeps the map's result there (:165-167), while cc is still
 *            returned and still carries gradient to w and b. */
#define EOGS_PAN_ORDER_CC_FIRST 0
#define EOGS_PAN_ORDER_MAP_FIRST 1

/* Length of g_params (floats):
 *   [0..11]   dL/dM[3][4]            (MAP_FIRST: [0] = dL/dw, [1] = dL/db, the rest zero)
 *   [12..14]  dL/dinshadow[3]        (MAP_FIRST: [12] only; zero when alt_diff is NULL)
 *   [15..19]  dL/dmap_params: FIXED dL/dp[5]; BASE, BASE_SIGMOID and TRANSLATE {dL/dw[3], dL/db, 0}; zero otherwise */
#define EOGS_PAN_NPARAMS 20

/* Workspace for the per-workgroup partial sums of eogs_pan_backward on an H x W image. */
int eogs_pan_bytes(int H, int W, size_t* bytes);

/* raw f32[3][H][W]; alt_diff f32[H][W] or NULL; M, inshadow as the order says (inshadow is ignored when alt_diff is
 * NULL); map_params as the kind says (NULL for the kinds without).
 * Outputs: cc (3 planes CC_FIRST, where it may be NULL; 1 plane MAP_FIRST), shaded f32[H][W], shadow f32[H][W]
 * (NULL exactly when alt_diff is NULL). */
int eogs_pan_forward(int H, int W, int order, int kind, const float* raw, const float* alt_diff, const float* M,
                     const float* inshadow, const float* map_params, float* cc, float* shaded, float* shadow,
                     void* stream);

/* Backward. Upstream gradients g_shaded, g_cc, g_shadow with the shapes of the outputs; each may be NULL (= zero).
 *   g_raw      f32[3][H][W], fully overwritten
 *   g_alt_diff f32[H][W], fully overwritten (NULL exactly when alt_diff is NULL); clip(max=0) passes the gradient for
 *              alt_diff <= 0
 *   g_params   f32[EOGS_PAN_NPARAMS], fully overwritten, layout above */
int eogs_pan_backward(int H, int W, int order, int kind, const float* raw, const float* alt_diff, const float* M,
                      const float* inshadow, const float* map_params, const float* g_shaded, const float* g_cc,
                      const float* g_shadow, float* g_raw, float* g_alt_diff, float* g_params, void* ws, size_t ws_bytes,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_PAN_H_INCLUDED */
