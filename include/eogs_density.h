/*
 * eogs_density.h — C-ABI of adaptive density control (classic 3DGS densification, the reference's `only_prune: False`):
 *
 *   eogs_density_stats_update   the per-iteration statistics    train_pan.py:679-690, gaussian_model.py:719-723
 *   eogs_density_decide/_build  GaussianModel.densify_and_prune gaussian_model.py:685-717 as ONE decision pass over the
 *                               P original rows, one host wait for four counts, and ONE build pass that writes every
 *                               output tensor (densify_and_clone :625-660, densify_and_split :573-623,
 *                               densification_postfix :541-571, prune_points :488-505)
 *
 * Same conventions as eogs_optim.h: DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status (0 ok, <0 error,
 * message via eogs_rast_last_error()), no device allocation inside the library, arguments are checked before anything
 * touches a device. Only eogs_density_decide waits for the device (once); everything else is asynchronous, uses the
 * caller's addresses alone and can be recorded by a stream capture. No atomics: results are bitwise reproducible.
 */
#ifndef EOGS_DENSITY_H_INCLUDED
#define EOGS_DENSITY_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- statistics ----------------------------------------------------------------------------------------------------
 * Per row i with radii[i] > 0:
 *     max_radii2D[i] = max(max_radii2D[i], (float)radii[i])
 *     xyz_gradient_accum[i] += sqrt(g[i][0]^2 + g[i][1]^2)          (g = viewspace_grad f32[P][3]; g[i][2] is not read)
 *     denom[i] += 1
 * every other row keeps its bits (no nonzero(), no gather: one launch). `radii` is i32[P] (radii_is_float == 0: what the
 * rasterizer returns) or f32[P] (radii_is_float != 0). xyz_gradient_accum and denom are f32[P] ([P,1] contiguous).
 * P == 0 is a no-op. Asynchronous on `stream`. */
int eogs_density_stats_update(int64_t P, const float* viewspace_grad, const void* radii, int radii_is_float,
                              float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream);

/* ---- densify_and_prune ---------------------------------------------------------------------------------------------
 * One flag byte per ORIGINAL row: */
#define EOGS_DENSITY_CLONE 1u       /* the clone mask: g >= grad_threshold && smax <= dense_threshold                   */
#define EOGS_DENSITY_SPLIT 2u       /* the split mask: g >= grad_threshold && smax >  dense_threshold (disjoint)         */
#define EOGS_DENSITY_PRUNE_SELF 4u  /* the final prune drops the row and its clone:  low || big_self                     */
#define EOGS_DENSITY_PRUNE_SAMP 8u  /* the final prune drops the row's N samples:    low || big_samp                     */
/*     g        = xyz_gradient_accum / denom, NaN -> 0   (IEEE division)
 *     smax     = max_k exp(scaling[k])
 *     low      = 1 / (1 + exp(-opacity)) < min_opacity
 *     big_self = use_screen && smax > big_threshold
 *     big_samp = use_screen && max_k exp(log(exp(scaling[k]) / split_div)) > big_threshold      (split_div = 0.8 N)
 * The thresholds arrive rounded once to fp32 from the doubles the caller formed. The reference's third term of the final
 * prune, max_radii2D > max_screen_size, reads a statistic that densification_postfix has zeroed: it never fires and is
 * not evaluated. A row whose opacity logit is <= EOGS_DENSITY_RETIRED_BELOW (eogs2_amd.optim.retire_rows parks pruned
 * rows at -1e30) is never selected; `low` removes it. */
#define EOGS_DENSITY_RETIRED_BELOW (-5.0e29f)
#define EOGS_DENSITY_MAX_N 8
#define EOGS_DENSITY_MAX_ROWS ((int64_t)1 << 28)

/* The four counts eogs_density_decide returns, in this order. */
#define EOGS_DENSITY_N_KEPT 0         /* rows with neither SPLIT nor PRUNE_SELF                                    */
#define EOGS_DENSITY_N_KEPT_CLONES 1  /* rows with CLONE and not PRUNE_SELF                                        */
#define EOGS_DENSITY_N_SPLIT 2        /* rows with SPLIT: the normal draw holds N x this many rows                 */
#define EOGS_DENSITY_N_KEPT_SPLIT 3   /* rows with SPLIT and not PRUNE_SAMP                                        */

/* Workspace of decide / build: per-workgroup (256 rows) counts of the four kinds, then their exclusive prefixes. */
int eogs_density_bytes(int64_t P, size_t* bytes);

/* Writes flags[P] and the workspace, returns counts[4] on the HOST (synchronises `stream` once). */
int eogs_density_decide(int64_t P, const float* xyz_gradient_accum, const float* denom, const float* opacity,
                        const float* scaling, float grad_threshold, float dense_threshold, float min_opacity, int use_screen,
                        float big_threshold, float split_div, uint8_t* flags, void* ws, size_t ws_bytes, int64_t* counts,
                        void* stream);

/* The rows with EOGS_DENSITY_SPLIT of one row-major tensor (row_bytes a multiple of 4, <= 256), in order, to dst
 * (counts[EOGS_DENSITY_N_SPLIT] rows): the log-scales whose exp() are the standard deviations of the normal draw.
 * `flags` and `ws` are those of eogs_density_decide on the same rows. Asynchronous on `stream`. */
int eogs_density_split_rows(int64_t P, const uint8_t* flags, const void* src, void* dst, int row_bytes, const void* ws,
                            size_t ws_bytes, void* stream);

/* One tensor of the build: `src` holds P rows, `dst` n_out rows of row_bytes (a multiple of 4, <= 256). */
#define EOGS_DENSITY_COPY 0     /* new rows copy their origin's row                                                   */
#define EOGS_DENSITY_ZERO 1     /* new rows are zero (Adam moments)                                                   */
#define EOGS_DENSITY_XYZ 2      /* f32[.][3]: a sample's row is R(q / |q|) . sample + xyz                            */
#define EOGS_DENSITY_SCALING 3  /* f32[.][3]: a sample's row is log(exp(s) / split_div)                              */
typedef struct {
  const void* src;
  void* dst;
  int row_bytes;
  int kind;
} eogs_density_tensor;

/* Output rows, n_out = counts[0] + counts[1] + N counts[3], the reference's order after its four stages:
 *     [rows neither split nor pruned] [clones of the clone rows not pruned] N x [samples of the split rows whose samples
 *     are not pruned], copy-major (copy 0 of all rows, then copy 1, ...); inside every run the original row order.
 * `samples` is f32[N counts[2]][3], the draw for ALL split-selected rows: row c counts[2] + j belongs to copy c of the
 * j-th split-selected row. `rotation` f32[P][4] (raw quaternions). `tensors` is a HOST array (any length: chunks of 24 per
 * launch). `flags`, `ws` and `counts` are those of eogs_density_decide on the same rows. src and dst must not overlap.
 * Asynchronous on `stream`. */
int eogs_density_build(int64_t P, int N, const uint8_t* flags, const int64_t* counts, int n_tensors,
                       const eogs_density_tensor* tensors, const float* rotation, const float* samples, float split_div,
                       const void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_DENSITY_H_INCLUDED */
