/*
 * eogs_nll.h — C-ABI of the transient-uncertainty term of the training loss: the Gaussian negative log-likelihood of the
 * shaded image under a per-pixel variance that comes from the camera's trainable transient mask (train_pan.py:433-449,
 * scene/cameras/affine_cameras.py:280-292):
 *
 *   betaprime = (cam.transient_mask.clip(0, 1) + 1e-3).square()
 *   L_nll     = torch.nn.functional.gaussian_nll_loss(input=image, target=gt_image, var=betaprime repeated over the planes)
 *
 * One forward launch group and one backward launch where the reference materialises a C x H x W variance, runs about ten
 * elementwise PyTorch kernels each way and waits for the device in `torch.any(var < 0)`. The same entries serve torch's
 * gaussian_nll_loss with a variance given directly (1 plane shared by all planes, or one per plane).
 *
 * Same conventions as eogs_reg.h: plain DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status (0 ok,
 * <0 error, message via eogs_rast_last_error()), the library never allocates device memory, arguments are checked before
 * anything touches a device. Every sum is accumulated in float64 per workgroup and the partials are combined in a fixed
 * order by one workgroup (no atomics, a grid that depends on the shape alone): results are bitwise reproducible. The
 * weight and the upstream gradients live in DEVICE memory and are read by the kernels: a caller switches the term on by
 * writing into the weight, and a recorded graph keeps replaying across the switch.
 */
#ifndef EOGS_NLL_H_INCLUDED
#define EOGS_NLL_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Mode bits.
 *   EOGS_NLL_MASK  var_or_mask is the transient mask m f32[H][W] (var_planes must be 1); without the bit it is the variance
 *                  itself, f32[var_planes][H][W] with var_planes 1 (shared by the planes) or `planes`
 *   EOGS_NLL_FULL  add 0.5 log(2 pi) per element
 *   EOGS_NLL_SUM   the sum over the elements instead of their mean */
#define EOGS_NLL_MASK 1u
#define EOGS_NLL_FULL 2u
#define EOGS_NLL_SUM 4u

/* input, target f32[planes][H][W], contiguous. Per element
 *
 *   mask mode:  c = clip(m, 0, 1),  s = c + floor,  v = s s          otherwise  v = var
 *   vc = max(v, eps)                 (a NaN stays a NaN, as through torch's clamp)
 *   l  = 0.5 (log vc + (x - t)^2 / vc)
 *
 * v is never stored. A variance below zero is not refused (the reference raises after a wait for the device): it is
 * counted in out[4] and its element is clamped like any other, l = 0.5 (log eps + (x - t)^2 / eps).
 *
 * out f32[6]:
 *   [0] loss    mean (or sum) of l, plus 0.5 log(2 pi) per element with EOGS_NLL_FULL
 *   [1] total   weight[0] * loss; weight == NULL means 1; weight[0] == 0 gives exactly 0 (a select, not a product)
 *   [2] mean of m (of var without EOGS_NLL_MASK), over all its var_planes * H * W entries
 *   [3] their unbiased standard deviation (Tensor.std(): NaN for a single entry), from (n, mean, M2) partials combined by
 *       Chan's rule in double and in a fixed order: exactly 0 for a constant plane
 *   [4] entries with var < 0 (always 0 in mask mode)
 *   [5] mask pixels outside [0, 1] (0 without EOGS_NLL_MASK)
 *
 * Refused before any launch: planes, H or W below 1; a var_planes that does not fit the mode; unknown mode bits;
 * floor < 0 or eps <= 0 (or either not finite); a workspace below eogs_nll_bytes; NULL input, target, var_or_mask, out. */
int eogs_nll_bytes(int planes, int H, int W, size_t* bytes);

int eogs_nll_forward(int planes, int H, int W, unsigned mode, const float* input, const float* target,
                     const float* var_or_mask, int var_planes, float floor, float eps, const float* weight, float* out,
                     void* ws, size_t ws_bytes, void* stream);

/* Backward: one launch that recomputes from the inputs, one lane per pixel looping over the planes. Upstream gradients in
 * device memory, NULL = zero: g_loss f32[1] (d/d out[0]), g_total f32[1] (d/d out[1]). Every pixel sees
 *
 *   k = g_total * weight[0] + g_loss        (the first term exactly 0 when weight[0] == 0), divided by N = planes H W
 *                                           for the mean
 *   g_input f32[planes][H][W]        = k (x - t) / vc                                       fully overwritten
 *   d/dv                             = k 0.5 (1 / vc - (x - t)^2 / vc^2), passed on ALSO where v < eps (torch clamps a
 *                                      clone under no_grad)
 *   g_var_or_mask f32[var_planes][H][W]: d/dv, summed over the planes when the variance is shared; in mask mode
 *                                      sum over planes of d/dv * 2 s * [0 <= m <= 1] (inclusive, as torch's clamp
 *                                      backward: exactly 0 outside)                         fully overwritten
 *
 * k == 0 exactly (a term switched off by its weight and no g_loss) writes exact zeros everywhere: a NaN pixel is not
 * passed on. Either output may be NULL when it is not needed (not both). */
int eogs_nll_backward(int planes, int H, int W, unsigned mode, const float* input, const float* target,
                      const float* var_or_mask, int var_planes, float floor, float eps, const float* weight,
                      const float* g_loss, const float* g_total, float* g_input, float* g_var_or_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_NLL_H_INCLUDED */
