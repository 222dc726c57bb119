// reset.hip — the two in-place resets near the end of a training iteration (include/eogs_reset.h):
//   color_reset   densification_pruning/color_reset_op.py:42-88: erode every view's shadow map, sample it at every Gaussian's
//                 projected position, OR the verdicts, fill the flagged rows of opacity / f_dc / scaling and of their moments
//   reset_opacity scene/gaussian_model.py:347-352 with replace_tensor_to_optimizer (:451-464): cap the logits, zero the moments
// Nothing here is arithmetic-bound. The erosion is a stencil over one map (a tile and its halo in LDS, the 5 x 5 maximum as a
// row pass and a column pass); the verdict is a gather: one thread per Gaussian, four views' sixteen taps loaded before the
// first is used, the per-view constants read from LDS and kernel arguments at wave-uniform addresses; the fills are stores.
#include "api_util.h"
#include "eogs_reset.h"

namespace {

constexpr int TH = EOGS_RESET_TILE_H, TW = EOGS_RESET_TILE_W, HALO = 2;
constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;  // the staged tile: 36 x 68
static_assert(TH * TW % BLK == 0, "a tile is a whole number of passes of the workgroup");

// torch's max pooling keeps `val` when (val > max) || isnan(val): a NaN, once taken, stays (DilatedMaxPool2d / max_pool2d)
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

__global__ __launch_bounds__(BLK) void erode_kernel(int H, int W, int tiles_x, const float* __restrict__ shadow,
                                                    float* __restrict__ eroded) {
  __shared__ float t[LH][LW];   // fl(1 - s), -inf outside the map
  __shared__ float hm[LH][TW];  // its maximum over the five columns x .. x + 4 of the staged tile
  const int y0 = (int)(blockIdx.x / (uint32_t)tiles_x) * TH, x0 = (int)(blockIdx.x % (uint32_t)tiles_x) * TW;
  for (int idx = threadIdx.x; idx < LH * LW; idx += BLK) {
    const int r = idx / LW, c = idx - r * LW;
    const int gy = y0 - HALO + r, gx = x0 - HALO + c;
    float v = -INFINITY;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = 1.0f - shadow[(size_t)gy * (size_t)W + (size_t)gx];
    t[r][c] = v;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < LH * TW; idx += BLK) {
    const int r = idx / TW, c = idx - r * TW;
    float m = t[r][c];
#pragma unroll
    for (int k = 1; k <= 2 * HALO; k++) m = nan_max(m, t[r][c + k]);
    hm[r][c] = m;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < TH * TW; idx += BLK) {
    const int r = idx / TW, c = idx - r * TW;
    const int gy = y0 + r, gx = x0 + c;
    if (gy >= H || gx >= W) continue;
    float m = hm[r][c];
#pragma unroll
    for (int k = 1; k <= 2 * HALO; k++) m = nan_max(m, hm[r + k][c]);
    eroded[(size_t)gy * (size_t)W + (size_t)gx] = 1.0f - m;  // (the pixel itself is in its window: m is never -inf)
  }
}

struct FlagsTable {
  eogs_reset_view v[EOGS_RESET_MAX_VIEWS];
  int n;
};

constexpr int VIEW_BATCH = 4;  // views whose taps are loaded before any is used

__global__ __launch_bounds__(BLK) void flags_kernel(int64_t P, const float* __restrict__ xyz, const float* __restrict__ logit,
                                                    float retired_below, FlagsTable tab, int accumulate,
                                                    uint8_t* __restrict__ flags) {
  // columns 0 and 1 of every view's matrix: coef[k] = {A00, A10, A20, A30, A01, A11, A21, A31}
  __shared__ float coef[EOGS_RESET_MAX_VIEWS][8];
  if ((int)threadIdx.x < tab.n * 8) {
    const int k = threadIdx.x >> 3, e = threadIdx.x & 7;
    coef[k][e] = tab.v[k].affine[(e & 3) * 4 + (e >> 2)];
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= P) return;
  const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  bool any = false;
  for (int k0 = 0; k0 < tab.n; k0 += VIEW_BATCH) {
    float tap[VIEW_BATCH][4], fx[VIEW_BATCH], fy[VIEW_BATCH], x0f[VIEW_BATCH], y0f[VIEW_BATCH];
    bool in[VIEW_BATCH][4], live[VIEW_BATCH];
#pragma unroll
    for (int j = 0; j < VIEW_BATCH; j++) {
      const int k = min(k0 + j, tab.n - 1);  // (a batch past the last view repeats it; `live` drops the repeat)
      const eogs_reset_view V = tab.v[k];
      const float* c = coef[k];
      const float u = ((x * c[0] + y * c[1]) + z * c[2]) + c[3];
      const float v = ((x * c[4] + y * c[5]) + z * c[6]) + c[7];
      live[j] = k0 + j < tab.n && __builtin_isfinite(u) && __builtin_isfinite(v);
      const float wmax = (float)(V.W - 1), hmax = (float)(V.H - 1);
      fx[j] = ((u + 1.0f) / 2.0f) * wmax;
      fy[j] = ((v + 1.0f) / 2.0f) * hmax;
      x0f[j] = floorf(fx[j]);
      y0f[j] = floorf(fy[j]);
      const float x1f = x0f[j] + 1.0f, y1f = y0f[j] + 1.0f;
      const bool ix0 = x0f[j] >= 0.0f && x0f[j] <= wmax, ix1 = x1f >= 0.0f && x1f <= wmax;
      const bool iy0 = y0f[j] >= 0.0f && y0f[j] <= hmax, iy1 = y1f >= 0.0f && y1f <= hmax;
      in[j][0] = ix0 && iy0; in[j][1] = ix1 && iy0; in[j][2] = ix0 && iy1; in[j][3] = ix1 && iy1;
      // every load goes to a pixel of the map: a tap outside it reads the clamped pixel and is dropped below
      const size_t cx0 = (size_t)fminf(fmaxf(x0f[j], 0.0f), wmax), cx1 = (size_t)fminf(fmaxf(x1f, 0.0f), wmax);
      const size_t cy0 = (size_t)fminf(fmaxf(y0f[j], 0.0f), hmax), cy1 = (size_t)fminf(fmaxf(y1f, 0.0f), hmax);
      const size_t w = (size_t)V.W;
      tap[j][0] = V.eroded[cy0 * w + cx0];
      tap[j][1] = V.eroded[cy0 * w + cx1];
      tap[j][2] = V.eroded[cy1 * w + cx0];
      tap[j][3] = V.eroded[cy1 * w + cx1];
    }
#pragma unroll
    for (int j = 0; j < VIEW_BATCH; j++) {
      const float x1f = x0f[j] + 1.0f, y1f = y0f[j] + 1.0f;
      float s = 0.0f;  // grid_sample's order: nw, ne, sw, se
      if (in[j][0]) s += tap[j][0] * ((x1f - fx[j]) * (y1f - fy[j]));
      if (in[j][1]) s += tap[j][1] * ((fx[j] - x0f[j]) * (y1f - fy[j]));
      if (in[j][2]) s += tap[j][2] * ((x1f - fx[j]) * (fy[j] - y0f[j]));
      if (in[j][3]) s += tap[j][3] * ((fx[j] - x0f[j]) * (fy[j] - y0f[j]));
      any = any || (live[j] && s < 0.5f);
    }
  }
  if (logit != nullptr && logit[i] < retired_below) any = false;
  uint8_t f = any ? 1 : 0;
  if (accumulate) f |= flags[i];
  flags[i] = f;
}

struct RowsTable {
  eogs_reset_tensor t[EOGS_RESET_MAX_TENSORS];
  int n;
};

__global__ __launch_bounds__(BLK) void rows_kernel(int64_t P, const uint8_t* __restrict__ flags, RowsTable tab) {
  const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= P || flags[i] == 0) return;
  for (int k = 0; k < tab.n; k++) {
    const eogs_reset_tensor T = tab.t[k];
    float* d = T.data + i * (int64_t)T.row_elems;
    for (int e = 0; e < T.row_elems; e++) d[e] = T.value;
  }
}

constexpr int CAP_VEC = 4;  // elements per thread

__global__ __launch_bounds__(BLK) void opacity_cap_kernel(int64_t n, float* __restrict__ logit, float* __restrict__ exp_avg,
                                                          float* __restrict__ exp_avg_sq, float cap, float retired_below) {
  const int64_t i0 = ((int64_t)blockIdx.x * BLK + threadIdx.x) * CAP_VEC;
  if (i0 >= n) return;
  // an element is stored only when it changes: NaN > cap is false, and a retired row is skipped by its own test
  if (i0 + CAP_VEC <= n && ((((uintptr_t)logit | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15u) == 0)) {
    float4 l = *reinterpret_cast<const float4*>(logit + i0);
    const bool c0 = l.x > cap && !(l.x < retired_below), c1 = l.y > cap && !(l.y < retired_below);
    const bool c2 = l.z > cap && !(l.z < retired_below), c3 = l.w > cap && !(l.w < retired_below);
    if (c0 || c1 || c2 || c3) {
      l.x = c0 ? cap : l.x; l.y = c1 ? cap : l.y; l.z = c2 ? cap : l.z; l.w = c3 ? cap : l.w;
      *reinterpret_cast<float4*>(logit + i0) = l;
    }
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (exp_avg) *reinterpret_cast<float4*>(exp_avg + i0) = zero;
    if (exp_avg_sq) *reinterpret_cast<float4*>(exp_avg_sq + i0) = zero;
  } else {
    for (int k = 0; k < CAP_VEC; k++)
      if (i0 + k < n) {
        const float l = logit[i0 + k];
        if (l > cap && !(l < retired_below)) logit[i0 + k] = cap;
        if (exp_avg) exp_avg[i0 + k] = 0.0f;
        if (exp_avg_sq) exp_avg_sq[i0 + k] = 0.0f;
      }
  }
}

constexpr int64_t MAX_ROWS = (int64_t)0x7FFFFFFF * 128;  // the row limit of the other per-Gaussian entries (eogs_compact_plan)

}  // namespace

extern "C" {

int eogs_reset_erode(int H, int W, const float* shadow, float* eroded, void* stream) {
  clear_error();
  if (H < 1 || W < 1) return fail(EOGS_ERR_INVALID_ARG, "reset_erode: H and W must be positive");
  if ((int64_t)H * W >= ((int64_t)1 << 31)) return fail(EOGS_ERR_INVALID_ARG, "reset_erode: the map must hold fewer than 2^31 pixels");
  if (!shadow || !eroded) return fail(EOGS_ERR_INVALID_ARG, "reset_erode: NULL argument");
  if (shadow == eroded) return fail(EOGS_ERR_INVALID_ARG, "reset_erode: the eroded map needs an array of its own");
  if (((uintptr_t)shadow | (uintptr_t)eroded) & 3u) return fail(EOGS_ERR_INVALID_ARG, "reset_erode: arrays not 4-byte aligned");
  const int64_t tiles_x = ((int64_t)W + TW - 1) / TW, tiles_y = ((int64_t)H + TH - 1) / TH;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(erode_kernel, dim3((uint32_t)(tiles_x * tiles_y)), dim3(BLK), 0, s, H, W, (int)tiles_x, shadow, eroded);
  LAUNCH_TRY(s, false, "reset_erode");
  return EOGS_OK;
}

int eogs_reset_flags(int64_t P, const float* xyz, const float* opacity_logit, float retired_below, int n_views,
                     const eogs_reset_view* views, int accumulate, uint8_t* flags, void* stream) {
  clear_error();
  if (P < 0 || P > MAX_ROWS) return fail(EOGS_ERR_INVALID_ARG, "reset_flags: bad row count");
  if (n_views < 0 || n_views > EOGS_RESET_MAX_VIEWS || (n_views > 0 && !views))
    return fail(EOGS_ERR_INVALID_ARG, "reset_flags: at most 16 views");
  if (retired_below != retired_below) return fail(EOGS_ERR_INVALID_ARG, "reset_flags: retired_below is NaN");
  FlagsTable tab;
  tab.n = n_views;
  for (int k = 0; k < EOGS_RESET_MAX_VIEWS; k++) tab.v[k] = eogs_reset_view{nullptr, nullptr, 1, 1};
  for (int k = 0; k < n_views; k++) {
    const eogs_reset_view& v = views[k];
    if (!v.eroded || !v.affine) return fail(EOGS_ERR_INVALID_ARG, "reset_flags: a view without its map or its matrix");
    if (v.H < 1 || v.W < 1 || v.H > (1 << 24) || v.W > (1 << 24) || (int64_t)v.H * v.W >= ((int64_t)1 << 31))
      return fail(EOGS_ERR_INVALID_ARG, "reset_flags: a view's H and W must be 1 .. 2^24 with H W < 2^31");
    if (((uintptr_t)v.eroded | (uintptr_t)v.affine) & 3u) return fail(EOGS_ERR_INVALID_ARG, "reset_flags: arrays not 4-byte aligned");
    tab.v[k] = v;
  }
  if (P == 0) return EOGS_OK;
  if (!xyz || !flags) return fail(EOGS_ERR_INVALID_ARG, "reset_flags: NULL argument");
  if (((uintptr_t)xyz | (uintptr_t)opacity_logit) & 3u) return fail(EOGS_ERR_INVALID_ARG, "reset_flags: arrays not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(flags_kernel, dim3((uint32_t)((P + BLK - 1) / BLK)), dim3(BLK), 0, s, P, xyz, opacity_logit, retired_below,
                     tab, accumulate, flags);
  LAUNCH_TRY(s, false, "reset_flags");
  return EOGS_OK;
}

int eogs_reset_rows(int64_t P, const uint8_t* flags, int n, const eogs_reset_tensor* tensors, void* stream) {
  clear_error();
  if (P < 0 || P > MAX_ROWS) return fail(EOGS_ERR_INVALID_ARG, "reset_rows: bad row count");
  if (n < 0 || n > EOGS_RESET_MAX_TENSORS || (n > 0 && !tensors)) return fail(EOGS_ERR_INVALID_ARG, "reset_rows: at most 16 tensors");
  RowsTable tab;
  tab.n = n;
  for (int k = 0; k < EOGS_RESET_MAX_TENSORS; k++) tab.t[k] = eogs_reset_tensor{nullptr, 0, 0.0f};
  for (int k = 0; k < n; k++) {
    const eogs_reset_tensor& t = tensors[k];
    if (t.row_elems < 1 || t.row_elems > EOGS_RESET_MAX_ROW_ELEMS)
      return fail(EOGS_ERR_INVALID_ARG, "reset_rows: rows of 1 .. 64 elements");
    if (P > 0 && (!t.data || ((uintptr_t)t.data & 3u))) return fail(EOGS_ERR_INVALID_ARG, "reset_rows: NULL or misaligned tensor");
    tab.t[k] = t;
  }
  if (P == 0 || n == 0) return EOGS_OK;
  if (!flags) return fail(EOGS_ERR_INVALID_ARG, "reset_rows: NULL flags");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rows_kernel, dim3((uint32_t)((P + BLK - 1) / BLK)), dim3(BLK), 0, s, P, flags, tab);
  LAUNCH_TRY(s, false, "reset_rows");
  return EOGS_OK;
}

int eogs_reset_opacity_cap(int64_t n, float* logit, float* exp_avg, float* exp_avg_sq, float cap_logit, float retired_below,
                           void* stream) {
  clear_error();
  if (n < 0 || n > MAX_ROWS) return fail(EOGS_ERR_INVALID_ARG, "reset_opacity_cap: bad element count");
  if (cap_logit != cap_logit || retired_below != retired_below) return fail(EOGS_ERR_INVALID_ARG, "reset_opacity_cap: NaN argument");
  if (n == 0) return EOGS_OK;
  if (!logit) return fail(EOGS_ERR_INVALID_ARG, "reset_opacity_cap: NULL argument");
  if (((uintptr_t)logit | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 3u)
    return fail(EOGS_ERR_INVALID_ARG, "reset_opacity_cap: arrays not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t per_block = (int64_t)BLK * CAP_VEC;
  hipLaunchKernelGGL(opacity_cap_kernel, dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(BLK), 0, s, n, logit, exp_avg,
                     exp_avg_sq, cap_logit, retired_below);
  LAUNCH_TRY(s, false, "reset_opacity_cap");
  return EOGS_OK;
}

}  // extern "C"
