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

#ifdef __cplusplus
}
#endif
#endif /* EOGS_TSDF_H_INCLUDED */
