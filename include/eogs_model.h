/*
 * eogs_model.h — C-ABI of the two per-row passes of scene/gaussian_model.py::GaussianModel that are arithmetic on P rows:
 *
 *   create_from_pcd  gaussian_model.py:159-215: the six parameter tensors and max_radii2D from a point cloud, its colours and
 *                    the 3-NN statistic of simple-knn (eogs_knn.h), in one launch
 *   save_ply / load_ply  gaussian_model.py:310-346, :354-449: the six parameter tensors <-> one row-major block of
 *                    EOGS_MODEL_ROW_COLS(n_rest) floats per Gaussian, the vertex payload of the PLY file
 *
 *   eogs_model_init         xyz, f_dc, f_rest, scaling, rotation, opacity, max_radii2D of a new model
 *   eogs_model_rows_pack    six tensors -> f32 [P][17 + 3 n_rest]
 *   eogs_model_rows_unpack  f32 [P][17 + 3 n_rest] -> six tensors
 *
 * n_rest = (sh_degree + 1)^2 - 1 is one of 0, 3, 8, 15 (sh_degree 0 .. 3).
 *
 * Init, per row i, every step one fp32 operation:
 *     xyz[i]         = points[i]
 *     f_dc[i][0][c]  = (colors[i][c] - 0.5f) / 0.28209479177387814f     RGB2SH, utils/sh_utils.py; IEEE division
 *     f_rest[i]      = 0
 *     scaling[i][k]  = logf(sqrtf(d)), d = dist2[i] < 1e-7f ? 1e-7f : dist2[i], k = 0, 1, 2   (a NaN stays a NaN, as clamp_min)
 *     rotation[i]    = (1, 0, 0, 0)
 *     opacity[i]     = opacity_logit       the caller forms it as the reference does (inverse_sigmoid on an fp32 tensor)
 *     max_radii2D[i] = 0
 * The subtraction, the division and the square root are correctly rounded and equal torch's CPU result bit for bit; logf is
 * the device's (within 1 ulp of the correctly rounded value).
 *
 * Rows: the column order of construct_list_of_attributes (gaussian_model.py:296-308):
 *     x y z | nx ny nz | f_dc_0..2 | f_rest_0 .. f_rest_{3 n_rest - 1} | opacity | scale_0..2 | rot_0..3
 * f_dc [P][1][3] and f_rest [P][n_rest][3] are stored channel-major, as `transpose(1, 2).flatten(start_dim=1)` leaves them:
 * f_rest_{c n_rest + k} = f_rest[i][k][c]. The normals are written as +0 by pack and skipped by unpack. Values are moved as
 * bits: NaN payloads and -0 survive both directions.
 *
 * Both row kernels take EOGS_MODEL_TILE_ROWS rows per workgroup and stage them in LDS in the block's own layout, so that
 * every global access of a wave is a run of consecutive dwords: the tensor side reads (writes) each tensor's slice of the
 * tile as one contiguous range, the block side moves the tile as one contiguous range in 16-byte pieces. Plain vector
 * loads and stores; no atomics.
 *
 * Same conventions as eogs_rast.h: plain DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status (0 ok,
 * <0 error, message via eogs_rast_last_error()), the library never allocates device memory, arguments are checked before
 * anything touches a device, and no entry waits for the device: each is one kernel launch and can be recorded. P == 0 is
 * a no-op. With n_rest == 0 the f_rest pointer is not read and may be NULL. The address range of an output may share no
 * address with the range of an input or of another output (the sizes follow from P and n_rest): such a call is refused.
 * Inputs may alias each other.
 */
#ifndef EOGS_MODEL_H_INCLUDED
#define EOGS_MODEL_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOGS_MODEL_TILE_ROWS 64                          /* rows per workgroup of the two row kernels */
#define EOGS_MODEL_MAX_REST 15                           /* sh_degree 3 */
#define EOGS_MODEL_ROW_COLS(n_rest) (17 + 3 * (n_rest)) /* floats per row of the block */

/* points, colors f32 [P][3]; dist2 f32 [P]; outputs: xyz [P][3], f_dc [P][1][3], f_rest [P][n_rest][3], scaling [P][3],
 * rotation [P][4], opacity [P][1], max_radii2D [P]. */
int eogs_model_init(int64_t P, int n_rest, const float* points, const float* colors, const float* dist2, float opacity_logit,
                    float* xyz, float* f_dc, float* f_rest, float* scaling, float* rotation, float* opacity, float* max_radii2D,
                    void* stream);

/* xyz [P][3], f_dc [P][1][3], f_rest [P][n_rest][3], opacity [P][1], scaling [P][3], rotation [P][4] -> rows
 * [P][EOGS_MODEL_ROW_COLS(n_rest)]. */
int eogs_model_rows_pack(int64_t P, int n_rest, const float* xyz, const float* f_dc, const float* f_rest, const float* opacity,
                         const float* scaling, const float* rotation, float* rows, void* stream);

/* rows [P][EOGS_MODEL_ROW_COLS(n_rest)] -> the six tensors; the three normal columns are not read. */
int eogs_model_rows_unpack(int64_t P, int n_rest, const float* rows, float* xyz, float* f_dc, float* f_rest, float* opacity,
                           float* scaling, float* rotation, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_MODEL_H_INCLUDED */
