/*
 * eogs_tsdf.h — C-ABI of the TSDF fusion of the DSM post-processing (second piece):
 *   TSDFVolume.integrate      src/gaussiansplatting/tsdf.py:459-498  (+ update_tsdf :500-520)
 *   RangeImageEOGS.sample_sdf src/gaussiansplatting/tsdf.py:325-368  (+ _world_to_view / _view_to_world :233-241)
 * One kernel per range image where the reference materialises ~25 voxel-sized temporaries (12 B/voxel coordinates,
 * grid_sample output, masks, three index gathers and two index scatters).
 * The stages around it:
 *   eogs_tsdf_normals  RangeImageEOGS.__init__ / reconstruct_normals / get_weights   tsdf.py:213-231, 243-323
 *   eogs_tsdf_prior    TSDFVolume.apply_prior                                         tsdf.py:602-638
 *   eogs_tsdf_surface  TSDFVolume.extract_dsm up to the plyflatten call               tsdf.py:530-562
 * and the scoring of the DSM that comes out of the chain (eogs_tsdf_dsm_*, further down):
 *   NCC registration, shift, clip and masked MAE          eval/dsmr.py, eval/eval_dsm.py:35-69, 334-341
 *
 * Same conventions as eogs_rast.h: plain DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status
 * (0 ok, <0 error, message via eogs_rast_last_error()), the library never allocates device memory.
 */
#ifndef EOGS_TSDF_H_INCLUDED
#define EOGS_TSDF_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Integrates one altitude image into the volume, in place.
 *   nx, ny, nz        voxels per dimension; volumes are f32[nx][ny][nz] (tsdf.py:451-456)
 *   ax, ay, az        f32[nx], f32[ny], f32[nz]: world coordinates of the voxel centres along each axis (the
 *                     reference's torch.linspace values, tsdf.py:402-407, so coordinates are bit-identical)
 *   affine            f32[24] = coef[3][3], intercept[3], inv(coef)[3][3], inv(coef) @ intercept [3]
 *                     (view = coef p + intercept, :234; world = inv(coef) view - inv(coef) intercept, :238-240)
 *   model_scale       points are divided by it before projection, distances multiplied by it (:341,366)
 *   trunc_margin      truncation distance (:385)
 *   H, W              image size; altitude f32[H][W], weight f32[H][W] (= get_weights(): clamp(angle, 0, 1), :322-323)
 * Per voxel: p = (x,y,z)/scale; (u,v,a) = view(p); bilinear sample (align_corners, zero padding) of altitude and weight
 * at (u,v); valid = |u| <= 1 & |v| <= 1; sdf = |world(u,v,alt_s) - p| sign(a - alt_s) scale; where valid & sdf >= -trunc:
 *   w_new = w_old + weight_s;  tsdf_new = (w_old tsdf_old + weight_s min(1, sdf/trunc)) / w_new      (:510-518)
 * (0/0 gives NaN exactly as in the reference when both weights are zero). */
int eogs_tsdf_integrate(int nx, int ny, int nz, const float* ax, const float* ay, const float* az, const float* affine,
                        float model_scale, float trunc_margin, int H, int W, const float* altitude, const float* weight,
                        float* tsdf_vol, float* weight_vol, void* stream);

/* Per-pixel normals, view angle and integration weights of one altitude image (the reference's RangeImageEOGS).
 *   H, W        image size; altitude f32[H][W]
 *   affine      f32[24], the layout eogs_tsdf_integrate takes (only inv(coef) and inv(coef) @ intercept are read)
 *   view_dir    f32[3] = normalize(solve(coef, e3), eps=1e-6) (tsdf.py:213-218)
 *   normals     f32[3][H][W] or NULL;  angle f32[H][W];  weights f32[H][W] or NULL
 * Pixel (r, c): world p = inv(coef) (u, v, alt) - inv(coef) intercept with u = ((c + 0.5) fp32(1/W)) 2 - 1,
 * v = ((r + 0.5) fp32(1/H)) 2 - 1 (tsdf.py:245-262). Taps outside the image are the vector (0, 0, 0) (F.unfold pads the
 * world-position image). Along x (W) and y (H), with taps p-2 .. p2: d = (p0 - p-2) / 2 if
 * |p-2 + 2 (p-1 - p-2) - p0| < |p2 + 2 (p1 - p2) - p0|, else (p2 - p0) / 2 (a tie and a NaN take the right branch);
 * n = normalize(cross(dx, dy), eps=1e-6); angle = n . (-view_dir); weights = clamp(angle, 0, 1), NaN kept. */
int eogs_tsdf_normals(int H, int W, const float* altitude, const float* affine, const float* view_dir, float* normals, float* angle,
                      float* weights, void* stream);

/* Workspace of eogs_tsdf_prior: one state byte per voxel + one int32 per (x, y) column (<= N + 4 nx ny + 256 bytes). */
int eogs_tsdf_prior_bytes(int nx, int ny, int nz, size_t* bytes);

/* Applies the reference's volume prior in place. Both masks are taken from the volume before anything is written:
 * occ = t <= 0, untouched = (w == 0) & (t == 1), cnt = occupied voxels in the 3x3x3 neighbourhood (outside voxels count 0),
 * top = the largest z with occ, 0 if none. Per voxel the first matching rule applies:
 *   occ & cnt == 1 -> (t, w) = (1, 0);   z == 0 -> (-1, 1);   untouched & z < top -> (-1, 1);   otherwise unchanged.
 * Only constants are written: the result is bit-exact. */
int eogs_tsdf_prior(int nx, int ny, int nz, float* tsdf_vol, float* weight_vol, void* ws, size_t ws_bytes, void* stream);

/* The DSM surface of the volume: index[x][y] = the largest z with t < 0, 0 if none (argmax((t < 0) * idx), tsdf.py:530-533);
 * height[x][y] = az[index] (NULL: not written). */
int eogs_tsdf_surface(int nx, int ny, int nz, const float* tsdf_vol, const float* az, int64_t* index, float* height, void* stream);

/* ---- DSM evaluation: the reference's registration and MAE (src/gaussiansplatting/eval/dsmr.py, eval/eval_dsm.py) ----
 * Images are row-major [H][W], float32 (`f64` = 0) or float64 (`f64` = 1); with two images both have the type `f64` names.
 * All arithmetic is float64 (numba types the reference's accumulators float64 whatever the image type). `u` is the
 * reference DSM (ground truth), `v` the DSM to be registered; v may be larger than u, not smaller in either dimension
 * (EOGS_ERR_INVALID_ARG; the reference reads out of bounds). Reductions are two-stage in a fixed order, without atomics:
 * the same inputs give the same bits. No call waits for the device. */

#define EOGS_TSDF_DSM_MAX_IRANGE 8 /* largest search radius: (2 * 8 + 1)^2 = 289 candidate shifts */

/* Result words of one NCC search, written on the device (plain stores). A following search reads `dx, dy` from here. */
typedef struct {
  int32_t dx, dy;   /* compute_ncc's winner (dsmr.py:146-163); the search centre if no candidate won */
  int32_t valid;    /* 1 if some candidate had a finite NCC */
  int32_t reserved;
  double count;     /* mean_std_base at (dx, dy) (dsmr.py:94-133): finite pairs in the overlap, ... */
  double muu, muv, sigu, sigv, xcorr;
  double ncc;       /* xcorr / (sigu sigv + 1e-8) (dsmr.py:143) */
} eogs_tsdf_dsm_result;

/* downsample2x (dsmr.py:15-43): out f64[ceil(H/2)][ceil(W/2)]. The reference writes out[j // 2][i // 2] for EVERY source
 * pixel, so the last writer wins: out[J][I] = mean over the finite pixels of the 2 x 2 block whose top-left corner is
 * (j, i) = (min(2J+1, H-1), min(2I+1, W-1)), clipped to the image, summed in the order (j,i), (j+1,i), (j,i+1),
 * (j+1,i+1) and divided once by their number; NaN if none is finite. Bit-exact. */
int eogs_tsdf_dsm_downsample(int H, int W, const void* in, int f64, double* out, void* stream);

/* Workspace of eogs_tsdf_dsm_ncc for a reference image of Hu x Wu and search radius irange (pivots, per-workgroup partial
 * sums of six moments per shift, the summed moments). */
int eogs_tsdf_dsm_ncc_bytes(int Hu, int Wu, int irange, size_t* bytes);

/* compute_ncc (dsmr.py:146-163) at one level: the NCC of every shift (x, y) with |x - cx| <= irange, |y - cy| <= irange in
 * ONE pass over the two images, and the winner.
 *   centre        DEVICE int32[2] = (dx, dy), e.g. the head of the result a coarser search wrote, or NULL for (0, 0);
 *                 (cx, cy) = centre_scale * (dx, dy) (2 when chaining from the level below, 1 for a given centre)
 *   irange        0 .. EOGS_TSDF_DSM_MAX_IRANGE (above: EOGS_ERR_INVALID_ARG)
 *   table         f64[2 irange + 1][2 irange + 1] or NULL: table[y - (cy - irange)][x - (cx - irange)] = ncc(u, v, x, y)
 *   result        the winner in the reference's scan order (y outer, x inner, strict `>`: the first of equal values
 *                 wins, a NaN never wins) and mean_std_base's tuple at the winner
 * mean_std_base (dsmr.py:94-133): over the pixels (j, i) of u with 0 <= i + x < Wu, 0 <= j + y < Hu (u's size) and both
 * u[j][i] and v[j + y][i + x] finite: count, the means, sig = sqrt(sum (. - mu)^2 / count), xcorr = sum (u - muu)(v - muv) /
 * count. The sums are taken in one pass about one pivot per image (the mean of a fixed sample of its finite pixels), which
 * keeps the digits of the reference's centred second pass. A shift without a finite pair has NaN moments and a NaN NCC.
 * NCCs that are equal only up to rounding are NOT ordered as the reference orders them: on a constant image or overlap (every
 * NCC is rounding noise around 0, in the reference's two-pass form as well) the winner may differ; the scan order decides
 * between values that are equal as computed here. */
int eogs_tsdf_dsm_ncc(int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int f64, int irange, const int32_t* centre,
                      int centre_scale, double* table, eogs_tsdf_dsm_result* result, void* ws, size_t ws_bytes, void* stream);

/* Workspace and pyramid depth of eogs_tsdf_dsm_shift: `levels` = 1 + the number of halvings recursive_ncc makes
 * (while min(H, W) > 100, dsmr.py:165-179); the workspace holds both float64 pyramids and the search's own workspace. */
int eogs_tsdf_dsm_shift_bytes(int Hu, int Wu, int Hv, int Wv, int irange, size_t* bytes, int* levels);

/* recursive_ncc + the final mean_std_base of compute_shift (dsmr.py:165-179, 198-225) as one stream-ordered chain: both
 * pyramids by eogs_tsdf_dsm_downsample's rule, then a search per level from the coarsest up, each reading its centre
 * 2 * (dx, dy) from the result the level below wrote on the device (the coarsest starts from (0, 0)).
 *   results   DEVICE eogs_tsdf_dsm_result[levels], [0] = full resolution: (dx, dy) and the moments compute_shift needs
 *             (a = sigu / sigv or 1, b = muu - muv a are the caller's two statements)
 *   tables    DEVICE f64[levels][2 irange + 1][2 irange + 1] or NULL */
int eogs_tsdf_dsm_shift(int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int f64, int irange, double* tables,
                        eogs_tsdf_dsm_result* results, void* ws, size_t ws_bytes, void* stream);

/* apply_shift (dsmr.py:182-192, 258-271): out[j][i] = a valnan(in, i + dx, j + dy) + b + c i + d j, evaluated in float64
 * from left to right and stored in the image's type; valnan is NaN outside the image. `out` must not alias `in`. */
int eogs_tsdf_dsm_apply_shift(int H, int W, const void* in, int f64, int dx, int dy, double a, double b, double c, double d,
                              void* out, void* stream);

/* Workspace of eogs_tsdf_dsm_mae (a constant: per-workgroup partials). */
int eogs_tsdf_dsm_mae_bytes(size_t* bytes);

/* The tail of dsm_pointwise_diff and _compute_mae (eval_dsm.py:60-69, 334-336), fused:
 *   pred      [Hp][Wp], the registered DSM, clipped IN PLACE to [min(gt) - 10, max(gt) + 10] (bounds evaluated in the
 *             image's type). clip_finite = 0: numpy's min / max, so one NaN in gt makes both bounds NaN and the clip
 *             returns NaN everywhere (the reference's behaviour); clip_finite = 1: the bounds skip NaN (ours)
 *   diff      [h][w] = pred[:h, :w] - gt[:h, :w] in the image's type, h = min(Hp, Hg), w = min(Wp, Wg)
 *   out       DEVICE f64[4] = sum |diff| over its non-NaN entries (float64), their number, the two clip bounds */
int eogs_tsdf_dsm_mae(int Hp, int Wp, void* pred, int Hg, int Wg, const void* gt, int f64, int clip_finite, void* diff, double* out,
                      void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_TSDF_H_INCLUDED */
