/*
 * eogs_randomcam.h — C-ABI of what RandomcamRendering_Loss (src/gaussiansplatting/loss/main_loss.py:56-221) needs beyond the
 * resample, shade / pan and rasterizer entries, for render_type "rawrender_wshadow"
 * (gaussian_renderer/renderer_cc_shadow.py:57-145), use_gt and a panchromatic camera:
 *
 *   eogs_randomcam_compose   the two 3 x 3 matrices of the shadow-mapped virtual view, formed on the device
 *                            (renderer_cc_shadow.py:93-95 and the chained einsum of :85-87 with :32-34)
 *   eogs_cmloss_*            eogs_mloss_* in mode EOGS_MLOSS_RANDOM (eogs_shade.h) for 1 .. 4 channels, either side of the
 *                            comparison optionally without a gradient
 *
 * Same conventions as eogs_shade.h: plain DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status (0 ok, <0
 * error, message via eogs_rast_last_error()), the library never allocates device memory, arguments are checked before
 * anything is queued. Everything is kernel launches on `stream` alone: a stream capture records it. Every sum is reduced per
 * workgroup and then in a fixed order (no atomics): results are bitwise reproducible.
 */
#ifndef EOGS_RANDOMCAM_H_INCLUDED
#define EOGS_RANDOMCAM_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOGS_CMLOSS_MAX_CHANNELS 4

/* One launch of one wave. cam2virt (C) and camera_to_sun (S) are row-major 3 x 3 fp32 on the device; C is typically what
 * eogs_draw_iteration wrote on the same stream. In double:
 *
 *   virt_to_sun = C^-1 . S        C^-1 = adj(C) / det(C), closed form           (renderer_cc_shadow.py:93-95)
 *   K           = virt_to_sun . C  the matrix that takes the true camera's (u, v, altitude) to the sun camera's
 *
 * out[0..9) = virt_to_sun, out[9..18) = K, each element rounded to fp32 once. C = I gives virt_to_sun = K = S bit for bit.
 * det(C) == 0 or not finite gives NaN in all 18 (the reference's torch.inverse raises; a launch cannot). No host wait, no
 * workspace, no library call. Pointers are 4-byte aligned; `out` must not overlap an input. */
int eogs_randomcam_compose(const float* cam2virt, const float* camera_to_sun, float* out, void* stream);

/* Workspace for the per-workgroup partial sums of eogs_cmloss_forward on an H x W image. */
int eogs_cmloss_bytes(int H, int W, size_t* bytes);

/* The masked resample loss of eogs_shade.h in mode EOGS_MLOSS_RANDOM over C planes, 1 <= C <= EOGS_CMLOSS_MAX_CHANNELS:
 *   mask  = |alt_diff| < 0.30 & |u| < 1 & |v| < 1                               (main_loss.py:151-154), detached
 *   L_alt = sum(|alt_diff| mask) / sum(mask)
 *   L_rgb = sum over all C planes of (|rgb_a - rgb_b| mask) / sum(mask)         (the pixel count, main_loss.py:90-92)
 * alt_diff f32[H][W], rgb_a, rgb_b f32[C][H][W], uv f32[H][W][2]. out f32[3] = {L_alt, L_rgb, sum(mask)}; an empty mask
 * gives {0, 0, 0}. A pixel outside the mask is not read into the sums, as eogs_shade.h states. For C == 3 the results are
 * those of eogs_mloss_forward bit for bit. */
int eogs_cmloss_forward(int H, int W, int C, const float* alt_diff, const float* rgb_a, const float* rgb_b, const float* uv,
                        float* out, void* ws, size_t ws_bytes, void* stream);

/* Backward: `out` is forward's result (the count is read on the device), upstream f32[2] = dL/d{L_alt, L_rgb}.
 * g_alt_diff f32[H][W] fully overwritten. g_rgb_a and g_rgb_b f32[C][H][W] (g_rgb_b = -g_rgb_a) are fully overwritten when
 * given; EACH may be NULL — the side that takes no gradient (use_gt: rgb_a is the ground-truth image). The sign rules, the
 * zero outside the mask and the +0 of an empty mask are those of eogs_mloss_backward. */
int eogs_cmloss_backward(int H, int W, int C, const float* alt_diff, const float* rgb_a, const float* rgb_b, const float* uv,
                         const float* out, const float* upstream, float* g_alt_diff, float* g_rgb_a, float* g_rgb_b,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_RANDOMCAM_H_INCLUDED */
