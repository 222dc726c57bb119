// dsm_raster.hip — the DSM raster (include/eogs_dsm.h): bounds of a point source, scatter to home cells, stencil finalise.
// What the reference does with plyflatten (utils/dsm_utils.py:7-51, tsdf.py:530-600); the raster's semantics are stated
// in the header.
//
// One device function, load_point, serves the three sources (a float64 cloud, the pixels of a rendered view, the surface of
// a TSDF volume), so the bounds pass and the scatter see the same points by construction. Coordinates are IEEE double with
// one rounding per operation (the library is built with -ffp-contract=off) and a true division: a lattice point lands in
// the cell numpy's floor((x - xoff) / res) puts it in.
//
// Accumulation: z, narrowed to fp32, is rounded to a multiple of 2^-20 (exact for |z| >= 8) and added into an int64 sum
// per HOME cell of a grid padded by `radius`; a uint32 counts the cell's points and its top bit marks a poisoned cell.
// Integer atomics commute: the same bits on every run and for every order of the points. The stencil pass adds the
// (2 radius + 1)^2 neighbourhood of each output cell and divides once, in double.
#include <math.h>

#include "api_util.h"
#include "reduce.h"

namespace {

constexpr int DT = 256;              // threads per workgroup
constexpr int DSM_BOUNDS_MAXBLK = 1024;  // workgroups of the bounds pass: a function of the point count alone
constexpr int DSM_SCATTER_MAXBLK = 4096;
constexpr uint32_t DSM_POISON = 0x80000000u;
constexpr double DSM_INV_QUANTUM = 1048576.0;  // 1 / EOGS_DSM_Z_QUANTUM
static_assert(EOGS_DSM_Z_QUANTUM * DSM_INV_QUANTUM == 1.0, "the quantum and its inverse");

struct DsmPartial { double xmin, xmax, ymin, ymax; int64_t nonfinite; int64_t pad; };
static_assert(sizeof(DsmPartial) == 48, "partials are carved 48 bytes apart");

__host__ __device__ inline int64_t src_points(const eogs_dsm_source& s) {
  return s.kind == EOGS_DSM_SRC_CLOUD ? s.N : (int64_t)s.H * (int64_t)s.W;
}

// Point `idx` of the source: x, y in double, z narrowed to fp32 (plyflatten's raster is float32).
__device__ inline void load_point(const eogs_dsm_source& s, int64_t idx, double& x, double& y, float& z) {
  if (s.kind == EOGS_DSM_SRC_CLOUD) {
    const double* p = s.cloud + 3 * idx;
    x = p[0];
    y = p[1];
    z = (float)p[2];
    return;
  }
  const int64_t r = idx / s.W, c = idx - r * s.W;
  const double u = (double)s.u_axis[c], v = (double)s.v_axis[r], a = (double)s.altitude[idx];
  if (s.kind == EOGS_DSM_SRC_GRID) {  // tsdf.py:538-556: the fp32 cloud widened, + scene_params[0]
    x = v + s.shift[0];
    y = u + s.shift[1];
    z = (float)(a + s.shift[2]);
    return;
  }
  const float* A = s.affine;
  const double d0 = u - (double)A[9], d1 = v - (double)A[10], d2 = a - (double)A[11];  // affine_cameras.py:443-446
  const double e0 = ((double)A[0] * d0 + (double)A[1] * d1) + (double)A[2] * d2;
  const double e1 = ((double)A[3] * d0 + (double)A[4] * d1) + (double)A[5] * d2;
  const double e2 = ((double)A[6] * d0 + (double)A[7] * d1) + (double)A[8] * d2;
  x = e0 * s.scale + s.shift[0];  // dsm_utils.py:11
  y = e1 * s.scale + s.shift[1];
  z = (float)(e2 * s.scale + s.shift[2]);
}

__device__ inline bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and +-inf

// The workgroup's result on thread 0. Only finite values enter the minima and maxima, so fmin / fmax never see a NaN.
__device__ inline DsmPartial wg_reduce(DsmPartial p, DsmPartial* s_red) {
  p.xmin = wave_min(p.xmin);
  p.xmax = wave_max(p.xmax);
  p.ymin = wave_min(p.ymin);
  p.ymax = wave_max(p.ymax);
  p.nonfinite = wave_sum(p.nonfinite);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < DT / 64; w++) {
      p.xmin = fmin(p.xmin, s_red[w].xmin);
      p.xmax = fmax(p.xmax, s_red[w].xmax);
      p.ymin = fmin(p.ymin, s_red[w].ymin);
      p.ymax = fmax(p.ymax, s_red[w].ymax);
      p.nonfinite += s_red[w].nonfinite;
    }
  return p;
}

__device__ inline DsmPartial partial_identity() {
  DsmPartial p;
  p.xmin = p.ymin = INFINITY;
  p.xmax = p.ymax = -INFINITY;
  p.nonfinite = 0;
  p.pad = 0;
  return p;
}

__global__ __launch_bounds__(DT) void dsm_bounds_kernel(eogs_dsm_source src, int64_t n, DsmPartial* __restrict__ partial) {
  __shared__ DsmPartial s_red[DT / 64];
  DsmPartial p = partial_identity();
  for (int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x; i < n; i += (int64_t)gridDim.x * DT) {
    double x, y;
    float z;
    load_point(src, i, x, y, z);
    if (finite_d(x) && finite_d(y)) {
      p.xmin = fmin(p.xmin, x);
      p.xmax = fmax(p.xmax, x);
      p.ymin = fmin(p.ymin, y);
      p.ymax = fmax(p.ymax, y);
    } else {
      p.nonfinite += 1;
    }
  }
  p = wg_reduce(p, s_red);
  if (threadIdx.x == 0) partial[blockIdx.x] = p;
}

__global__ __launch_bounds__(DT) void dsm_bounds_final_kernel(int nblk, int64_t n, const DsmPartial* __restrict__ partial,
                                                              eogs_dsm_bounds_result* __restrict__ out) {
  __shared__ DsmPartial s_red[DT / 64];
  DsmPartial p = partial_identity();
  for (int b = threadIdx.x; b < nblk; b += DT) {
    const DsmPartial q = partial[b];
    p.xmin = fmin(p.xmin, q.xmin);
    p.xmax = fmax(p.xmax, q.xmax);
    p.ymin = fmin(p.ymin, q.ymin);
    p.ymax = fmax(p.ymax, q.ymax);
    p.nonfinite += q.nonfinite;
  }
  p = wg_reduce(p, s_red);
  if (threadIdx.x == 0) {
    out->xmin = p.xmin;
    out->xmax = p.xmax;
    out->ymin = p.ymin;
    out->ymax = p.ymax;
    out->nonfinite = p.nonfinite;
    out->count = n;
  }
}

// `n16` 16-byte words of the workspace (sums, counts and the skipped counter), zeroed with full-width stores
__global__ __launch_bounds__(DT) void dsm_clear_kernel(size_t n16, uint4* __restrict__ ws) {
  for (size_t i = (size_t)blockIdx.x * DT + threadIdx.x; i < n16; i += (size_t)gridDim.x * DT) ws[i] = make_uint4(0u, 0u, 0u, 0u);
}

// One point per lane and trip. pw, ph: the padded grid. A point whose home cell is outside it reaches no output cell.
__global__ __launch_bounds__(DT) void dsm_scatter_kernel(eogs_dsm_source src, int64_t n, double xoff, double yoff, double res,
                                                         int radius, int pw, int ph, unsigned long long* __restrict__ sums,
                                                         uint32_t* __restrict__ counts, unsigned long long* __restrict__ skipped) {
  for (int64_t idx = (int64_t)blockIdx.x * DT + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * DT) {
    double x, y;
    float z;
    load_point(src, idx, x, y, z);
    if (!(finite_d(x) && finite_d(y))) {
      atomicAdd(skipped, 1ull);
      continue;
    }
    // compared as doubles: a far point never reaches the conversion to int
    const double fi = floor((x - xoff) / res) + (double)radius, fj = floor((yoff - y) / res) + (double)radius;
    if (!(fi >= 0. && fi < (double)pw && fj >= 0. && fj < (double)ph)) continue;
    const size_t cell = (size_t)(int)fj * (size_t)pw + (size_t)(int)fi;  // < pw * ph, which the entry point bounds
    if (!(fabsf(z) <= (float)EOGS_DSM_Z_MAX)) {  // NaN, +-inf, out of range
      atomicOr(&counts[cell], DSM_POISON);
    } else {
      const long long q = __double2ll_rn((double)z * DSM_INV_QUANTUM);  // |q| <= 2^35; the product is exact
      atomicAdd(&sums[cell], (unsigned long long)q);                  // two's complement: the wrapped sum is the signed sum
      atomicAdd(&counts[cell], 1u);
    }
  }
}

__global__ __launch_bounds__(DT) void dsm_stencil_kernel(int xsize, int ysize, int radius, int pw, const long long* __restrict__ sums,
                                                         const uint32_t* __restrict__ counts,
                                                         const unsigned long long* __restrict__ skipped, float* __restrict__ out,
                                                         int32_t* __restrict__ count_out, int64_t* __restrict__ skipped_out) {
  const int64_t cells = (int64_t)xsize * ysize;
  if (skipped_out && blockIdx.x == 0 && threadIdx.x == 0) *skipped_out = (int64_t)*skipped;  // the scatter has ended
  for (int64_t o = (int64_t)blockIdx.x * DT + threadIdx.x; o < cells; o += (int64_t)gridDim.x * DT) {
    const int jj = (int)(o / xsize), ii = (int)(o - (int64_t)jj * xsize);
    // output cell (ii, jj) is padded cell (ii + radius, jj + radius): its neighbourhood starts at padded (ii, jj)
    long long sum = 0;
    int64_t cnt = 0;
    uint32_t poison = 0u;
    for (int dj = 0; dj <= 2 * radius; dj++) {
      const size_t row = (size_t)(jj + dj) * (size_t)pw + (size_t)ii;
      for (int di = 0; di <= 2 * radius; di++) {
        const uint32_t c = counts[row + di];
        poison |= c;
        cnt += (int64_t)(c & ~DSM_POISON);
        sum += sums[row + di];
      }
    }
    const bool bad = (poison & DSM_POISON) != 0u;
    float v = NAN;
    if (!bad && cnt > 0) v = (float)(((double)sum * EOGS_DSM_Z_QUANTUM) / (double)cnt);
    out[o] = v;
    if (count_out) count_out[o] = bad ? -1 : (int32_t)(cnt > 0x7fffffff ? 0x7fffffff : cnt);
  }
}

inline int blocks_for(int64_t n, int maxblk) {
  const int64_t b = (n + DT - 1) / DT;
  return (int)(b < 1 ? 1 : (b > maxblk ? maxblk : b));
}

}  // namespace

static size_t dsm_bounds_ws_bytes() { return (size_t)DSM_BOUNDS_MAXBLK * sizeof(DsmPartial); }

struct DsmRasterWS {
  long long* sums;              // [ph][pw] fixed-point sums of the home cells, the grid padded by `radius`
  uint32_t* counts;             // [ph][pw] points per home cell; the top bit marks a poisoned cell
  unsigned long long* skipped;  // points left out for a non-finite x or y
  int pw, ph;
  size_t bytes;                 // a multiple of 256: the clear pass zeroes all of it
};
static DsmRasterWS dsm_raster_layout(char* base, int xsize, int ysize, int radius) {
  DsmRasterWS w;
  w.pw = xsize + 2 * radius;
  w.ph = ysize + 2 * radius;
  const size_t cells = (size_t)w.pw * (size_t)w.ph;
  const size_t sum_bytes = (cells * 8 + 255) & ~(size_t)255, cnt_bytes = (cells * 4 + 255) & ~(size_t)255;
  w.sums = reinterpret_cast<long long*>(base);
  w.counts = reinterpret_cast<uint32_t*>(base + sum_bytes);
  w.skipped = reinterpret_cast<unsigned long long*>(base + sum_bytes + cnt_bytes);
  w.bytes = sum_bytes + cnt_bytes + 256;
  return w;
}

static int dsm_source_check(const char* who, const eogs_dsm_source* src) {
  if (!src) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL source", who);
  if (src->kind == EOGS_DSM_SRC_CLOUD) {
    if (src->N < 0) return fail(EOGS_ERR_INVALID_ARG, "%s: negative point count", who);
    if (src->N > 0 && !src->cloud) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL cloud", who);
    if ((uintptr_t)src->cloud & 7u) return fail(EOGS_ERR_INVALID_ARG, "%s: cloud not 8-byte aligned", who);
    return EOGS_OK;
  }
  if (src->kind != EOGS_DSM_SRC_VIEW && src->kind != EOGS_DSM_SRC_GRID) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown source kind", who);
  if (src->H <= 0 || src->W <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad image size", who);
  if (!src->altitude || !src->u_axis || !src->v_axis) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL image or axis", who);
  if (src->kind == EOGS_DSM_SRC_VIEW) {
    if (!src->affine) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL affine", who);
    if (!(src->scale == src->scale)) return fail(EOGS_ERR_INVALID_ARG, "%s: scale is NaN", who);
  }
  return EOGS_OK;
}

static int dsm_grid_check(const char* who, int xsize, int ysize, int radius) {
  if (radius < 0 || radius > EOGS_DSM_MAX_RADIUS) return fail(EOGS_ERR_INVALID_ARG, "%s: radius out of range", who);
  if (xsize <= 0 || ysize <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: xsize and ysize must be positive", who);
  if (((int64_t)xsize + 2 * radius) * ((int64_t)ysize + 2 * radius) >= ((int64_t)1 << 31))
    return fail(EOGS_ERR_INVALID_ARG, "%s: raster too large", who);
  return EOGS_OK;
}

extern "C" {

int eogs_dsm_bounds_bytes(size_t* bytes) {
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_bounds_bytes: NULL argument");
  *bytes = 256 + dsm_bounds_ws_bytes();
  return EOGS_OK;
}

int eogs_dsm_bounds(const eogs_dsm_source* src, eogs_dsm_bounds_result* result, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const int rc = dsm_source_check("dsm_bounds", src);
  if (rc != EOGS_OK) return rc;
  if (!result || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_bounds: NULL argument");
  if ((uintptr_t)result & 7u) return fail(EOGS_ERR_INVALID_ARG, "dsm_bounds: result not 8-byte aligned");
  char* base = ws_base(ws);
  if ((size_t)(base - (char*)ws) + dsm_bounds_ws_bytes() > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "dsm_bounds: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = src_points(*src);
  const int nblk = blocks_for(n, DSM_BOUNDS_MAXBLK);
  DsmPartial* partial = reinterpret_cast<DsmPartial*>(base);
  hipLaunchKernelGGL(dsm_bounds_kernel, dim3(nblk), dim3(DT), 0, s, *src, n, partial);
  hipLaunchKernelGGL(dsm_bounds_final_kernel, dim3(1), dim3(DT), 0, s, nblk, n, partial, result);
  LAUNCH_TRY(s, false, "dsm_bounds");
  return EOGS_OK;
}

int eogs_dsm_raster_bytes(int xsize, int ysize, int radius, size_t* bytes) {
  const int rc = dsm_grid_check("dsm_raster_bytes", xsize, ysize, radius);
  if (rc != EOGS_OK) return rc;
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster_bytes: NULL argument");
  *bytes = 256 + dsm_raster_layout(nullptr, xsize, ysize, radius).bytes;
  return EOGS_OK;
}

int eogs_dsm_raster(const eogs_dsm_source* src, double xoff, double yoff, double res, int xsize, int ysize, int radius,
                    float* out, int32_t* count, int64_t* skipped, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  int rc = dsm_source_check("dsm_raster", src);
  if (rc != EOGS_OK) return rc;
  rc = dsm_grid_check("dsm_raster", xsize, ysize, radius);
  if (rc != EOGS_OK) return rc;
  const double big = 1.7976931348623157e308;
  if (!(res > 0. && res <= big)) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster: resolution must be positive and finite");
  if (!(xoff >= -big && xoff <= big && yoff >= -big && yoff <= big)) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster: xoff, yoff must be finite");
  if (!out || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster: NULL argument");
  if ((uintptr_t)skipped & 7u) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster: skipped not 8-byte aligned");
  char* base = ws_base(ws);
  const DsmRasterWS w = dsm_raster_layout(base, xsize, ysize, radius);
  if ((size_t)(base - (char*)ws) + w.bytes > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "dsm_raster: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t n16 = w.bytes / 16;
  hipLaunchKernelGGL(dsm_clear_kernel, dim3(blocks_for((int64_t)n16, 1024)), dim3(DT), 0, s, n16, reinterpret_cast<uint4*>(w.sums));
  const int64_t n = src_points(*src);
  if (n > 0)
    hipLaunchKernelGGL(dsm_scatter_kernel, dim3(blocks_for(n, DSM_SCATTER_MAXBLK)), dim3(DT), 0, s, *src, n, xoff, yoff, res, radius,
                       w.pw, w.ph, reinterpret_cast<unsigned long long*>(w.sums), w.counts, w.skipped);
  hipLaunchKernelGGL(dsm_stencil_kernel, dim3(blocks_for((int64_t)xsize * ysize, 4096)), dim3(DT), 0, s, xsize, ysize, radius, w.pw,
                     w.sums, w.counts, w.skipped, out, count, skipped);
  LAUNCH_TRY(s, false, "dsm_raster");
  return EOGS_OK;
}

}  // extern "C"
