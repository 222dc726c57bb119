/*
 * eogs_dsm.h — C-ABI of the DSM raster: a point cloud, or the points of one rendered view, flattened into a Digital
 * Surface Model. It is the step between the render / the TSDF fusion and the score of the finished DSM (eogs_tsdf_dsm_*
 * of eogs_tsdf.h). The reference takes it in three places, always the same way: utils/dsm_utils.py:7-51 (every testing
 * iteration of train_pan.py:738-797 and render_pan.py:402) and tsdf.py:530-600 —
 *     a float64 cloud in UTM, four lines of grid geometry from its bounds,
 *     plyflatten(cloud, xoff, yoff, resolution, xsize, ysize, radius=1, sigma=inf), a profile dictionary.
 *
 *   eogs_dsm_bounds   min / max of x and y and the number of non-finite coordinates, in one pass over the points
 *   eogs_dsm_raster   scatter to home cells, then one stencil pass: the mean per cell, NaN where nothing fell
 *
 * `plyflatten` is third-party code that is not part of this project. What it computes for sigma = inf (every weight 1) is
 * STATED here, the way SURVEY.md §8c states CUB's and glm's arithmetic:
 *     home cell of (x, y, z):  i = floor((x - xoff) / res),  j = floor((yoff - y) / res)    IEEE double, a true division
 *     the point contributes (float)z to every cell (ii, jj) with |ii - i| <= radius, |jj - j| <= radius,
 *     0 <= ii < xsize, 0 <= jj < ysize: only the TARGET cell is range-checked, a home cell outside the raster reaches in
 *     out[jj][ii] = mean of the contributions, NaN without one; float32 [ysize][xsize]
 * Deviation, on purpose: plyflatten keeps a running float32 mean in point order; this returns the mean itself,
 *     |out - m| <= EOGS_DSM_Z_QUANTUM / 2 + ulp32(m),   m = the float64 mean of the narrowed z,
 * the same bits on every run and under any permutation of the points: each z is rounded to a multiple of
 * EOGS_DSM_Z_QUANTUM and added into a 64-bit INTEGER sum per cell (integer atomics commute; float atomics do not).
 * A non-finite z, or |z| > EOGS_DSM_Z_MAX, makes every cell of its footprint NaN. A point with a non-finite x or y is
 * skipped and counted.
 *
 * Capacity: a cell's neighbourhood holds up to 2^27 points at |z| = EOGS_DSM_Z_MAX before the sum could wrap, a home cell
 * up to 2^31 - 1 points.
 *
 * Because the weight is 1 and the footprint a box, a point is scattered to its HOME cell only, on a grid padded by `radius`
 * on every side (points whose home cell lies outside the padded grid reach no cell and are dropped); the stencil pass adds
 * the (2 radius + 1)^2 neighbourhood and divides. Same cells, same contributions, (2 radius + 1)^2 times fewer atomics.
 *
 * Same conventions as eogs_rast.h: plain DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status (0 ok,
 * <0 error, message via eogs_rast_last_error()), the library never allocates device memory, arguments are checked before
 * anything touches a device. Everything is asynchronous on `stream` and consists of kernel launches alone: a stream
 * capture records it.
 */
#ifndef EOGS_DSM_H_INCLUDED
#define EOGS_DSM_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOGS_DSM_Z_QUANTUM (1.0 / 1048576.0) /* 2^-20 m: what a z is rounded to before it is summed (exact for |z| >= 8) */
#define EOGS_DSM_Z_MAX 32768.0               /* |z| above it poisons the footprint                                     */
#define EOGS_DSM_MAX_RADIUS 4

#define EOGS_DSM_SRC_CLOUD 0 /* cloud: float64 [N][3]                                                                  */
#define EOGS_DSM_SRC_VIEW 1  /* one rendered view, no cloud is materialised. Pixel (r, c) of altitude f32 [H][W]:
                              *   uva = (u_axis[c], v_axis[r], altitude[r][c])      scene/cameras/affine_cameras.py:139-143
                              *   xyz = Ainv (uva - b) in double, Ainv and b widened from fp32          :440-447
                              *   xyz * scale + shift in double, one rounding each                 utils/dsm_utils.py:11
                              * point index r W + c                                                                     */
#define EOGS_DSM_SRC_GRID 2  /* the surface of a TSDF volume (tsdf.py:538-556): point (r, c) is
                              *   (v_axis[r], u_axis[c], altitude[r][c]) widened to double, + shift                     */

/* Where the points come from. A HOST structure; the pointers in it are device pointers. */
typedef struct {
  int kind;              /* EOGS_DSM_SRC_*                                                                              */
  int H, W;              /* VIEW, GRID                                                                                  */
  int64_t N;             /* CLOUD: number of points (0 is allowed: cloud may then be NULL)                              */
  const double* cloud;   /* CLOUD                                                                                       */
  const float* altitude; /* VIEW, GRID: f32 [H][W]                                                                      */
  const float* u_axis;   /* f32 [W]: VIEW torch.linspace(-1, 1, W); GRID the volume's second axis                       */
  const float* v_axis;   /* f32 [H]: VIEW torch.linspace(-1, 1, H); GRID the volume's first axis                        */
  const float* affine;   /* VIEW: f32 [12] = Ainv row-major, then b                                                     */
  double scale;          /* VIEW: scene_params[1]                                                                       */
  double shift[3];       /* VIEW, GRID: scene_params[0]                                                                 */
} eogs_dsm_source;

/* What eogs_dsm_bounds writes (device memory, 48 bytes). Without a finite point xmin = ymin = +inf, xmax = ymax = -inf. */
typedef struct {
  double xmin, xmax, ymin, ymax; /* over the points whose x and y are both finite                                      */
  int64_t nonfinite;             /* points with a non-finite x or y                                                    */
  int64_t count;                 /* points read                                                                        */
} eogs_dsm_bounds_result;

int eogs_dsm_bounds_bytes(size_t* bytes);
/* Two launches: per-workgroup partials with plain stores, then one workgroup. Min and max are exact in any order. */
int eogs_dsm_bounds(const eogs_dsm_source* src, eogs_dsm_bounds_result* result, void* ws, size_t ws_bytes, void* stream);

/* Workspace of eogs_dsm_raster: the padded grid's sums and counts. */
int eogs_dsm_raster_bytes(int xsize, int ysize, int radius, size_t* bytes);
/* Three launches (clear, scatter, stencil; an empty source skips the scatter). out f32 [ysize][xsize]; count (NULL =
 * not wanted) int32 [ysize][xsize]: the number of contributions of the cell, -1 where a poisoned footprint covers it;
 * skipped (NULL = not wanted): one int64, the number of points left out for a non-finite x or y.
 * 0 <= radius <= EOGS_DSM_MAX_RADIUS, res > 0 and finite, xoff and yoff finite, xsize, ysize >= 1 and
 * (xsize + 2 radius)(ysize + 2 radius) < 2^31. */
int eogs_dsm_raster(const eogs_dsm_source* src, double xoff, double yoff, double res, int xsize, int ysize, int radius,
                    float* out, int32_t* count, int64_t* skipped, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_DSM_H_INCLUDED */
