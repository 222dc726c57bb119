/*
 * eogs_reg.h — C-ABI of the training-loss regularisers that read the model or a render directly (the terms of
 * `inter_loss`, train_pan.py:450-465, that are neither photometric nor a resample consistency pair). Two groups, each one
 * forward and one backward launch group where the reference runs 3-20 elementwise PyTorch kernels and autograd replays
 * them:
 *
 *   eogs_reg_gauss_*   OpacityLoss, radiiOpacityLoss     src/gaussiansplatting/loss/opacity.py:14-17,30-35
 *                      erankLoss                         src/gaussiansplatting/loss/main_loss.py:26-34
 *   eogs_reg_image_*   Total_variation                   src/gaussiansplatting/loss/main_loss.py:46-50
 *                      AccumulatedOpacity                src/gaussiansplatting/loss/opacity.py:44-45
 *
 * Same conventions as eogs_shade.h: plain DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status (0 ok,
 * <0 error, message via eogs_rast_last_error()), the library never allocates device memory, arguments are checked before
 * anything touches a device. Every sum is accumulated in float64 per workgroup and the partials are combined in a fixed
 * order by one workgroup (no atomics, a grid that depends on the shape alone): results are bitwise reproducible.
 *
 * The weights of the terms and the upstream gradients live in DEVICE memory and are read by the kernels: a caller
 * switches a term on or off by writing into that tensor, and a recorded graph keeps replaying across the switch.
 */
#ifndef EOGS_REG_H_INCLUDED
#define EOGS_REG_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Gaussian-space terms ------------------------------------------------------------------------------------------
 * One lane per Gaussian over the RAW parameters: opacity logits o f32[P] ([P,1] contiguous), log-scales l f32[P][3],
 * radii i32[P]. sigmoid and exp are applied in the kernel; gradients are those of the raw parameters.
 *
 *   terms[0] = L_opacity       = sum_i sigmoid(o_i) / n_init
 *   terms[1] = L_opacity_radii = sum_{radii_i > 0} sigmoid(o_i) / n_init            (0 when no row is visible)
 *   terms[2] = L_erank         = mean_i ( max(-log(e_i + 1e-5), 0) + sqrt(min_k s2_ik) )
 *                                s2 = exp(l)^2 + 1e-5, q = s2 / sum_k s2, e = expm1(-sum_k q_k log(q_k + 1e-6))
 *   total    = sum_{k in want} weights[k] * terms[k]
 *
 * `want` selects the terms (bits below); a term that is not wanted is 0, is left out of `total` and receives no gradient.
 * EOGS_REG_OPACITY_RADII needs `radii`, EOGS_REG_ERANK needs `log_scales` (NULL otherwise allowed).
 *
 * Retired rows (eogs2_amd.optim.retire_rows parks pruned Gaussians at the logit -1e30): a row whose logit is
 * <= EOGS_REG_RETIRED_BELOW contributes exactly 0 to every term, receives exactly 0 gradient and is left out of the
 * erank mean, whose denominator is the number of remaining rows, counted on the device in the same pass (0 rows: the
 * term is 0). Without such rows the mean is over P, as the reference's.
 *
 * out f32[5] = {terms[0], terms[1], terms[2], total, number of rows that are not retired}. */
#define EOGS_REG_OPACITY 1u
#define EOGS_REG_OPACITY_RADII 2u
#define EOGS_REG_ERANK 4u
#define EOGS_REG_RETIRED_BELOW (-5.0e29f)

int eogs_reg_gauss_bytes(int64_t P, size_t* bytes);

int eogs_reg_gauss_forward(int64_t P, unsigned want, const float* opacity, const float* log_scales, const int32_t* radii,
                           float n_init, const float* weights, float* out, void* ws, size_t ws_bytes, void* stream);

/* Backward: one launch that recomputes from the inputs. `out` is forward's result (its row count is read on the device,
 * no host sync). Upstream gradients in device memory, NULL = zero: g_total f32[1] (d/d total), g_terms f32[3]
 * (d/d terms); row i sees c_k = g_total * weights[k] + g_terms[k] for the wanted terms.
 *   g_opacity f32[P]    fully overwritten
 *   g_scaling f32[P][3] fully overwritten when EOGS_REG_ERANK is wanted (must be NULL otherwise)
 * torch's rules are kept: amin splits its gradient evenly among exactly tied minima, clip(min=0) passes the gradient at
 * equality. */
int eogs_reg_gauss_backward(int64_t P, unsigned want, const float* opacity, const float* log_scales, const int32_t* radii,
                            float n_init, const float* weights, const float* out, const float* g_total,
                            const float* g_terms, float* g_opacity, float* g_scaling, void* stream);

/* ---- render-space terms --------------------------------------------------------------------------------------------
 * Contiguous fp32 planes [H][W]; either may be NULL (its term is then 0, left out of `total`, no gradient).
 *
 *   terms[0] = L_TV_altitude         = 0.5 ( sum |a[y+1][x] - a[y][x]| / ((H-1) W) + sum |a[y][x+1] - a[y][x]| / (H (W-1)) )
 *   terms[1] = L_accumulated_opacity = sum (1 - acc) / (H W)
 *   total    = weights[0] terms[0] + weights[1] terms[1]
 *
 * out f32[3] = {terms[0], terms[1], total}. H < 2 or W < 2 is refused (the reference's empty mean is NaN there). */
int eogs_reg_image_bytes(int H, int W, size_t* bytes);

int eogs_reg_image_forward(int H, int W, const float* altitude, const float* accumulated_opacity, const float* weights,
                           float* out, void* ws, size_t ws_bytes, void* stream);

/* Backward: a gather, one lane per pixel over its at most four differences; sign(0) = 0 as torch.abs'. g_total f32[1],
 * g_terms f32[2] in device memory, NULL = zero. g_altitude, g_accumulated_opacity f32[H][W] fully overwritten (NULL
 * exactly where the input is NULL). */
int eogs_reg_image_backward(int H, int W, const float* altitude, const float* accumulated_opacity, const float* weights,
                            const float* g_total, const float* g_terms, float* g_altitude, float* g_accumulated_opacity,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_REG_H_INCLUDED */
