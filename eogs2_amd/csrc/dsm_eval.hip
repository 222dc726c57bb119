// DSM evaluation (include/eogs_tsdf.h, eogs_tsdf_dsm_*): the reference's NCC registration, shift and masked MAE
//   src/gaussiansplatting/eval/dsmr.py, eval/eval_dsm.py:35-69, 334-341
// All arithmetic is float64, as numba types the reference's accumulators; -ffp-contract=off keeps every product and
// sum a rounding of its own. Every reduction is per-workgroup partials in the workspace plus a fixed-order second stage:
// no floating-point atomics, the same bits on every run.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "api_util.h"

#define DSM_TILE_W 64      // pixels of the reference image per tile of the NCC search
#define DSM_TILE_H 16
#define DSM_MOMENTS 6      // count, sum u', sum v', sum u'^2, sum v'^2, sum u'v' per shift
#define DSM_MAX_GRID 1024  // workgroups of the search and of the reductions (4 per CU): a function of the shape alone
#define DSM_MAX_LEVELS 32

namespace {

constexpr int kTW = DSM_TILE_W;    // pixels of u per tile, horizontally
constexpr int kTH = DSM_TILE_H;    // ... vertically: two halves of 8 rows, one per pair of waves
constexpr int kRMax = EOGS_TSDF_DSM_MAX_IRANGE;
constexpr int kQ = DSM_MOMENTS;    // count, sum u', sum v', sum u'^2, sum v'^2, sum u'v' (u' = u - pivot_u, v' = v - pivot_v)

__device__ inline bool finite64(double x) { return fabs(x) < INFINITY; }
__device__ inline double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---- downsample2x (dsmr.py:15-43) ----
// The reference writes out[j // 2][i // 2] for every source pixel (j, i): the last writer wins, which is the block whose
// top-left corner is (min(2J+1, H-1), min(2I+1, W-1)). One lane per output pixel.
template <typename T>
__global__ __launch_bounds__(256) void dsm_downsample_kernel(int H, int W, const T* __restrict__ in, int Ho, int Wo,
                                                             double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)Ho * Wo) return;
  const int J = (int)(idx / Wo), I = (int)(idx % Wo);
  const int j = min(2 * J + 1, H - 1), i = min(2 * I + 1, W - 1);
  double v = 0.0;
  int count = 0;
  for (int k = 0; k < 2; k++)      // columns outer, rows inner: the reference's order of summation
    for (int l = 0; l < 2; l++)
      if (i + k < W && j + l < H) {
        const double t = (double)in[(size_t)(j + l) * W + (i + k)];
        if (finite64(t)) { v = v + t; count++; }
      }
  out[idx] = count > 0 ? v / (double)count : nan64();
}

// ---- pivots ----
// The one-pass moments are accumulated about one pivot per image so that they keep the digits of the reference's
// centred two-pass form (DSM heights are UTM altitudes: mean >> spread). Pivot = mean of the finite ones among <= 4096
// evenly spaced samples (an odd stride over the flat index), summed in a fixed order; if none of them is finite, the first finite pixel; 0 for an image
// without one (every NCC is NaN then). Block 0: u, block 1: v.
template <typename T>
__global__ __launch_bounds__(256) void dsm_pivot_kernel(int64_t nu, const T* __restrict__ u, int64_t nv, const T* __restrict__ v,
                                                        double* __restrict__ pivots) {
  __shared__ double ssum[256];
  __shared__ int scnt[256];
  __shared__ int64_t wfirst[4];
  const T* img = blockIdx.x == 0 ? u : v;
  const int64_t n = blockIdx.x == 0 ? nu : nv;
  const int tid = threadIdx.x;
  const int64_t step = n > 4096 ? ((n / 4096) | 1) : 1;  // odd: the samples do not line up in a few columns of a 2^k-wide image
  double acc = 0.0;
  int cnt = 0;
  for (int k = 0; k < 16; k++) {
    const int64_t s = (int64_t)(k * 256 + tid);
    if (s < 4096 && s * step < n) {
      const double t = (double)img[s * step];
      if (finite64(t)) { acc = acc + t; cnt++; }
    }
  }
  ssum[tid] = acc;
  scnt[tid] = cnt;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { ssum[tid] = ssum[tid] + ssum[tid + off]; scnt[tid] += scnt[tid + off]; }
    __syncthreads();
  }
  if (scnt[0] > 0) {
    if (tid == 0) pivots[blockIdx.x] = ssum[0] / (double)scnt[0];
    return;
  }
  for (int64_t base = 0; base < n; base += 256) {  // rare: no finite sample; the lowest finite index, chunk by chunk
    const int64_t i = base + tid;
    const unsigned long long m = __ballot(i < n && finite64((double)img[i]));
    if ((tid & 63) == 0) wfirst[tid >> 6] = m ? base + (tid & ~63) + (__ffsll((long long)m) - 1) : -1;
    __syncthreads();
    int64_t first = -1;
    for (int w = 3; w >= 0; w--)
      if (wfirst[w] >= 0) first = wfirst[w];
    __syncthreads();
    if (first >= 0) {
      if (tid == 0) pivots[blockIdx.x] = (double)img[first];
      return;
    }
  }
  if (tid == 0) pivots[blockIdx.x] = 0.0;
}

// ---- moments of every shift in one pass (dsmr.py:94-133 for all (dx, dy) of compute_ncc :146-163 at once) ----
// A workgroup stages a 64 x 16 tile of u and the tile of v it meets under every shift (halo of R on each side) in LDS,
// both already minus their pivots and NaN outside u's extent (the reference's bounds test uses u's size for both).
// The SHIFTS are dealt to the lanes: lane s of a 128-lane half owns shift s (dy = s / n, dx = s % n; a second and third
// round for n*n > 128) and walks the pixels of its half of the tile, so the count and the five float64 sums of a shift are 11
// VGPRs of one lane and never cross lanes. The u pixel is one LDS broadcast; the v pixels of the lanes are consecutive
// doubles along dx and `stride` doubles apart along dy, and stride = 64 + n (= n mod 32) puts the 32 lanes of an LDS
// access group on 32 different banks. Accumulators live across the tiles a workgroup walks (grid-stride, the grid a
// function of the shape alone) and leave as one partial per (workgroup, half): plain stores, summed by
// dsm_reduce_kernel in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void dsm_moments_kernel(int Hu, int Wu, const T* __restrict__ u, int Wv,
                                                          const T* __restrict__ v, int R, const int* __restrict__ centre,
                                                          int centre_scale, const double* __restrict__ pivots, int tiles_x,
                                                          int num_tiles, double* __restrict__ partials, int P) {
  __shared__ double su[kTH * kTW];
  __shared__ double sv[(kTH + 2 * kRMax) * (kTW + 2 * kRMax + 1)];
  const int n = 2 * R + 1, nshift = n * n;
  const int cx = centre ? centre[0] * centre_scale : 0, cy = centre ? centre[1] * centre_scale : 0;
  const int stride = kTW + n;
  const int vrows = kTH + 2 * R, vcols = kTW + 2 * R;
  const double pu = pivots[0], pv = pivots[1];
  const int tid = threadIdx.x, half = tid >> 7, sl = tid & 127;
  for (int s0 = 0; s0 < nshift; s0 += 128) {
    const int s = s0 + sl;
    const bool live = s < nshift;
    const int sy = live ? s / n : 0, sx = live ? s % n : 0;
    double a_u = 0.0, a_v = 0.0, a_uu = 0.0, a_vv = 0.0, a_uv = 0.0;
    int a_n = 0;
    for (int tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
      const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
      __syncthreads();  // the previous tile has been read
      for (int idx = tid; idx < kTH * kTW; idx += 256) {
        const int j = y0 + idx / kTW, i = x0 + idx % kTW;
        su[idx] = (j < Hu && i < Wu) ? (double)u[(size_t)j * Wu + i] - pu : nan64();
      }
      for (int idx = tid; idx < vrows * vcols; idx += 256) {
        const int r = idx / vcols, c = idx % vcols;
        const int jj = y0 + cy - R + r, ii = x0 + cx - R + c;
        // inside u's extent, hence inside v's (v is at least as large as u in both dimensions)
        const bool inb = jj >= 0 && jj < Hu && ii >= 0 && ii < Wu;
        sv[r * stride + c] = inb ? (double)v[(size_t)jj * Wv + ii] - pv : nan64();
      }
      __syncthreads();
      const int th = min(kTH, Hu - y0), tw = min(kTW, Wu - x0);
      const int r_end = min(half * (kTH / 2) + kTH / 2, th);
      for (int r = half * (kTH / 2); r < r_end; r++) {
        const double* __restrict__ urow = su + r * kTW;
        const double* __restrict__ vrow = sv + (r + sy) * stride + sx;
#pragma unroll 4
        for (int c = 0; c < tw; c++) {
          const double a = urow[c], b = vrow[c];
          const bool ok = finite64(a) && finite64(b);
          const double a0 = ok ? a : 0.0, b0 = ok ? b : 0.0;
          a_n += ok ? 1 : 0;
          a_u = a_u + a0;
          a_v = a_v + b0;
          a_uu = a_uu + a0 * a0;
          a_vv = a_vv + b0 * b0;
          a_uv = a_uv + a0 * b0;
        }
      }
    }
    if (live) {
      double* dst = partials + (size_t)s * kQ * P + (blockIdx.x * 2 + half);
      dst[0] = (double)a_n;
      dst[(size_t)P] = a_u;
      dst[(size_t)2 * P] = a_v;
      dst[(size_t)3 * P] = a_uu;
      dst[(size_t)4 * P] = a_vv;
      dst[(size_t)5 * P] = a_uv;
    }
  }
}

// One workgroup per shift: partial p goes to thread p % 256 in ascending order, then a fixed tree.
__global__ __launch_bounds__(256) void dsm_reduce_kernel(const double* __restrict__ partials, int P, double* __restrict__ moments) {
  __shared__ double red[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  for (int q = 0; q < kQ; q++) {
    const double* src = partials + ((size_t)s * kQ + q) * P;
    double acc = 0.0;
    for (int p = tid; p < P; p += 256) acc = acc + src[p];
    red[tid] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) red[tid] = red[tid] + red[tid + off];
      __syncthreads();
    }
    if (tid == 0) moments[s * kQ + q] = red[0];
    __syncthreads();
  }
}

struct DsmStats { double count, muu, muv, sigu, sigv, xcorr, ncc; };

// mean_std_base's results from the sums about the pivots; NaN throughout for a shift without a finite pair.
__device__ inline DsmStats dsm_stats(const double* __restrict__ m, double pu, double pv) {
  DsmStats st;
  st.count = m[0];
  if (!(m[0] > 0.0)) {
    st.muu = st.muv = st.sigu = st.sigv = st.xcorr = st.ncc = nan64();
    return st;
  }
  const double n = m[0], mu = m[1] / n, mv = m[2] / n;
  const double varu = m[3] / n - mu * mu, varv = m[4] / n - mv * mv;
  st.muu = pu + mu;
  st.muv = pv + mv;
  st.sigu = sqrt(varu > 0.0 ? varu : (varu == varu ? 0.0 : varu));
  st.sigv = sqrt(varv > 0.0 ? varv : (varv == varv ? 0.0 : varv));
  st.xcorr = m[5] / n - mu * mv;
  st.ncc = st.xcorr / (st.sigu * st.sigv + 1e-8);  // dsmr.py:143
  return st;
}

// The NCC table and compute_ncc's winner (dsmr.py:146-163): y outer, x inner, strict `>` from -inf, start at the centre.
__global__ __launch_bounds__(256) void dsm_argmax_kernel(int R, const double* __restrict__ moments, const double* __restrict__ pivots,
                                                         const int* __restrict__ centre, int centre_scale,
                                                         double* __restrict__ table, eogs_tsdf_dsm_result* __restrict__ result) {
  __shared__ double sncc[(2 * kRMax + 1) * (2 * kRMax + 1)];
  const int n = 2 * R + 1, nshift = n * n;
  const double pu = pivots[0], pv = pivots[1];
  for (int s = threadIdx.x; s < nshift; s += 256) {
    const double c = dsm_stats(moments + s * kQ, pu, pv).ncc;
    sncc[s] = c;
    if (table) table[s] = c;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int cx = centre ? centre[0] * centre_scale : 0, cy = centre ? centre[1] * centre_scale : 0;
  int best = -1;
  double maxv = -INFINITY;
  for (int s = 0; s < nshift; s++)
    if (sncc[s] > maxv) { best = s; maxv = sncc[s]; }
  eogs_tsdf_dsm_result res;
  res.dx = best >= 0 ? cx - R + best % n : cx;
  res.dy = best >= 0 ? cy - R + best / n : cy;
  res.valid = best >= 0 ? 1 : 0;
  res.reserved = 0;
  const DsmStats st = dsm_stats(moments + (best >= 0 ? best : (R * n + R)) * kQ, pu, pv);
  res.count = st.count;
  res.muu = st.muu;
  res.muv = st.muv;
  res.sigu = st.sigu;
  res.sigv = st.sigv;
  res.xcorr = st.xcorr;
  res.ncc = st.ncc;
  *result = res;
}

// ---- apply_shift (dsmr.py:182-192) ----
template <typename T>
__global__ __launch_bounds__(256) void dsm_apply_shift_kernel(int H, int W, const T* __restrict__ in, int dx, int dy, double a, double b,
                                                              double c, double d, T* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)H * W) return;
  const int j = (int)(idx / W), i = (int)(idx % W);
  const int64_t ii = (int64_t)i + dx, jj = (int64_t)j + dy;
  const double val = (ii >= 0 && jj >= 0 && ii < W && jj < H) ? (double)in[(size_t)jj * W + ii] : nan64();
  out[idx] = (T)(((a * val + b) + c * (double)i) + d * (double)j);
}

// ---- clip bounds (eval_dsm.py:65-67): numpy's min / max (a NaN makes both NaN) or the NaN-skipping ones ----
template <typename T>
__global__ __launch_bounds__(256) void dsm_minmax_kernel(int64_t n, const T* __restrict__ gt, double* __restrict__ part) {
  __shared__ double smin[256], smax[256];
  __shared__ int snan[256];
  double lo = INFINITY, hi = -INFINITY;
  int any_nan = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double t = (double)gt[i];
    if (t != t) any_nan = 1;
    else { lo = t < lo ? t : lo; hi = t > hi ? t : hi; }
  }
  const int tid = threadIdx.x;
  smin[tid] = lo; smax[tid] = hi; snan[tid] = any_nan;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      smin[tid] = smin[tid + off] < smin[tid] ? smin[tid + off] : smin[tid];
      smax[tid] = smax[tid + off] > smax[tid] ? smax[tid + off] : smax[tid];
      snan[tid] |= snan[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) { part[blockIdx.x * 3] = smin[0]; part[blockIdx.x * 3 + 1] = smax[0]; part[blockIdx.x * 3 + 2] = (double)snan[0]; }
}

// out[2] = min - 10, out[3] = max + 10, evaluated in the image's type as numpy does for a scalar of that type
template <typename T>
__global__ __launch_bounds__(256) void dsm_bounds_kernel(int nblocks, const double* __restrict__ part, int finite_only,
                                                         double* __restrict__ out) {
  __shared__ double smin[256], smax[256];
  __shared__ int snan[256];
  const int tid = threadIdx.x;
  double lo = INFINITY, hi = -INFINITY;
  int any_nan = 0;
  for (int b = tid; b < nblocks; b += 256) {
    lo = part[b * 3] < lo ? part[b * 3] : lo;
    hi = part[b * 3 + 1] > hi ? part[b * 3 + 1] : hi;
    any_nan |= part[b * 3 + 2] > 0.0 ? 1 : 0;
  }
  smin[tid] = lo; smax[tid] = hi; snan[tid] = any_nan;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      smin[tid] = smin[tid + off] < smin[tid] ? smin[tid + off] : smin[tid];
      smax[tid] = smax[tid + off] > smax[tid] ? smax[tid + off] : smax[tid];
      snan[tid] |= snan[tid + off];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  lo = smin[0];
  hi = smax[0];
  if ((snan[0] && !finite_only) || lo > hi) { lo = nan64(); hi = nan64(); }  // lo > hi: nothing but NaN
  out[2] = (double)(T)((T)lo - (T)10);
  out[3] = (double)(T)((T)hi + (T)10);
}

// ---- clip + crop + diff + sum |diff| + count (eval_dsm.py:60-69, 334-336) ----
// pred is clipped in place over its whole extent; diff[h][w] covers the common top-left rectangle.
template <typename T>
__global__ __launch_bounds__(256) void dsm_mae_kernel(int Hp, int Wp, T* __restrict__ pred, int Wg, const T* __restrict__ gt, int h, int w,
                                                      const double* __restrict__ out, T* __restrict__ diff, double* __restrict__ part) {
  __shared__ double ssum[256];
  __shared__ double scnt[256];
  const T lo = (T)out[2], hi = (T)out[3];
  double acc = 0.0, cnt = 0.0;
  const int64_t n = (int64_t)Hp * Wp;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
    const int j = (int)(idx / Wp), i = (int)(idx % Wp);
    T x = pred[idx];
    // np.clip = minimum(maximum(x, lo), hi); both propagate a NaN of either operand
    if (x == x) x = (lo != lo) ? lo : (x < lo ? lo : x);
    if (x == x) x = (hi != hi) ? hi : (x > hi ? hi : x);
    pred[idx] = x;
    if (j < h && i < w) {
      const T dv = x - gt[(size_t)j * Wg + i];
      diff[(size_t)j * w + i] = dv;
      if (dv == dv) { acc = acc + fabs((double)dv); cnt = cnt + 1.0; }
    }
  }
  const int tid = threadIdx.x;
  ssum[tid] = acc; scnt[tid] = cnt;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { ssum[tid] = ssum[tid] + ssum[tid + off]; scnt[tid] = scnt[tid] + scnt[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) { part[blockIdx.x * 2] = ssum[0]; part[blockIdx.x * 2 + 1] = scnt[0]; }
}

__global__ __launch_bounds__(256) void dsm_mae_final_kernel(int nblocks, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double ssum[256];
  __shared__ double scnt[256];
  const int tid = threadIdx.x;
  double acc = 0.0, cnt = 0.0;
  for (int b = tid; b < nblocks; b += 256) { acc = acc + part[b * 2]; cnt = cnt + part[b * 2 + 1]; }
  ssum[tid] = acc; scnt[tid] = cnt;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { ssum[tid] = ssum[tid] + ssum[tid + off]; scnt[tid] = scnt[tid] + scnt[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) { out[0] = ssum[0]; out[1] = scnt[0]; }
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

static void launch_dsm_downsample(int H, int W, const void* in, int f64, double* out, hipStream_t s) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const unsigned g = blocks_for((int64_t)Ho * Wo);
  if (f64) hipLaunchKernelGGL(dsm_downsample_kernel<double>, dim3(g), dim3(256), 0, s, H, W, (const double*)in, Ho, Wo, out);
  else hipLaunchKernelGGL(dsm_downsample_kernel<float>, dim3(g), dim3(256), 0, s, H, W, (const float*)in, Ho, Wo, out);
}

struct DsmNccWS {
  double *pivots, *moments, *partials;  // [2], [n*n][6], [n*n][6][P]
  int tiles_x, num_tiles, grid, P;
  size_t bytes;
};
static DsmNccWS dsm_ncc_layout(char* base, int Hu, int Wu, int irange) {
  DsmNccWS ws;
  const int n = 2 * irange + 1;
  ws.tiles_x = (Wu + kTW - 1) / kTW;
  ws.num_tiles = ws.tiles_x * ((Hu + kTH - 1) / kTH);
  ws.grid = ws.num_tiles < DSM_MAX_GRID ? ws.num_tiles : DSM_MAX_GRID;
  ws.P = 2 * ws.grid;
  size_t off = 0;
  off = ws_carve(base, off, ws.pivots, 2);
  off = ws_carve(base, off, ws.moments, (size_t)n * n * kQ);
  off = ws_carve(base, off, ws.partials, (size_t)n * n * kQ * ws.P);
  ws.bytes = off + 256;  // the caller's pointer is rounded up to 256 B
  return ws;
}

static int dsm_check_pair(const char* what, int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int irange) {
  if (Hu <= 0 || Wu <= 0 || Hv <= 0 || Wv <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes", what);
  if (Hv < Hu || Wv < Wu) return fail(EOGS_ERR_INVALID_ARG, "%s: the image to register is smaller than the reference image", what);
  if ((uint64_t)Hv * Wv > ((uint64_t)1 << 31)) return fail(EOGS_ERR_OVERFLOW, "%s: image too large", what);
  if (irange < 0 || irange > EOGS_TSDF_DSM_MAX_IRANGE) return fail(EOGS_ERR_INVALID_ARG, "%s: irange outside 0 .. 8", what);
  if (!u || !v) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", what);
  return EOGS_OK;
}

// one level: pivots, the moments of every shift, their sum, the NCC table and its winner
static void dsm_search(int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int f64, int irange, const int32_t* centre,
                       int centre_scale, double* table, eogs_tsdf_dsm_result* result, const DsmNccWS& w, hipStream_t s) {
  const int64_t nu = (int64_t)Hu * Wu, nv = (int64_t)Hv * Wv;
  {
    ProfScope ps(PS_DSM_PIVOTS, s);
    if (f64) hipLaunchKernelGGL(dsm_pivot_kernel<double>, dim3(2), dim3(256), 0, s, nu, (const double*)u, nv, (const double*)v, w.pivots);
    else hipLaunchKernelGGL(dsm_pivot_kernel<float>, dim3(2), dim3(256), 0, s, nu, (const float*)u, nv, (const float*)v, w.pivots);
  }
  {
    ProfScope ps(PS_DSM_MOMENTS, s);
    if (f64)
      hipLaunchKernelGGL(dsm_moments_kernel<double>, dim3(w.grid), dim3(256), 0, s, Hu, Wu, (const double*)u, Wv, (const double*)v, irange,
                         centre, centre_scale, w.pivots, w.tiles_x, w.num_tiles, w.partials, w.P);
    else
      hipLaunchKernelGGL(dsm_moments_kernel<float>, dim3(w.grid), dim3(256), 0, s, Hu, Wu, (const float*)u, Wv, (const float*)v, irange,
                         centre, centre_scale, w.pivots, w.tiles_x, w.num_tiles, w.partials, w.P);
  }
  {
    ProfScope ps(PS_DSM_FINALIZE, s);
    const int n = 2 * irange + 1;
    hipLaunchKernelGGL(dsm_reduce_kernel, dim3(n * n), dim3(256), 0, s, w.partials, w.P, w.moments);
    hipLaunchKernelGGL(dsm_argmax_kernel, dim3(1), dim3(256), 0, s, irange, w.moments, w.pivots, centre, centre_scale, table, result);
  }
}

struct DsmShiftWS {
  int levels;
  int hu[DSM_MAX_LEVELS], wu[DSM_MAX_LEVELS], hv[DSM_MAX_LEVELS], wv[DSM_MAX_LEVELS];
  double *pu[DSM_MAX_LEVELS], *pv[DSM_MAX_LEVELS];  // float64 pyramid levels 1 .. levels-1 ([0] is the caller's image)
  char* ncc;
  size_t bytes;
};
static DsmShiftWS dsm_shift_layout(char* base, int Hu, int Wu, int Hv, int Wv, int irange) {
  DsmShiftWS w;
  w.levels = 1;
  w.hu[0] = Hu; w.wu[0] = Wu; w.hv[0] = Hv; w.wv[0] = Wv;
  w.pu[0] = w.pv[0] = nullptr;
  size_t off = 0;
  while ((Hu < Wu ? Hu : Wu) > 100 && w.levels < DSM_MAX_LEVELS) {  // dsmr.py:168
    Hu = (Hu + 1) / 2; Wu = (Wu + 1) / 2; Hv = (Hv + 1) / 2; Wv = (Wv + 1) / 2;
    const int k = w.levels++;
    w.hu[k] = Hu; w.wu[k] = Wu; w.hv[k] = Hv; w.wv[k] = Wv;
    off = ws_carve(base, off, w.pu[k], (size_t)Hu * Wu);
    off = ws_carve(base, off, w.pv[k], (size_t)Hv * Wv);
  }
  off = ws_align(off);
  w.ncc = base ? base + off : nullptr;
  w.bytes = off + dsm_ncc_layout(nullptr, w.hu[0], w.wu[0], irange).bytes + 256;
  return w;
}

static unsigned reduce_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < DSM_MAX_GRID ? b : DSM_MAX_GRID);
}

static size_t dsm_mae_ws_bytes() { return (size_t)DSM_MAX_GRID * 3 * sizeof(double) + 256; }

extern "C" {

int eogs_tsdf_dsm_downsample(int H, int W, const void* in, int f64, double* out, void* stream) {
  clear_error();
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "dsm_downsample: bad sizes");
  if ((uint64_t)H * W > ((uint64_t)1 << 31)) return fail(EOGS_ERR_OVERFLOW, "dsm_downsample: image too large");
  if (!in || !out) return fail(EOGS_ERR_INVALID_ARG, "dsm_downsample: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_DSM_DOWNSAMPLE, s); launch_dsm_downsample(H, W, in, f64, out, s); }
  LAUNCH_TRY(s, false, "dsm_downsample");
  return EOGS_OK;
}

int eogs_tsdf_dsm_ncc_bytes(int Hu, int Wu, int irange, size_t* bytes) {
  clear_error();
  if (Hu <= 0 || Wu <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_ncc_bytes: bad argument");
  if (irange < 0 || irange > EOGS_TSDF_DSM_MAX_IRANGE) return fail(EOGS_ERR_INVALID_ARG, "dsm_ncc_bytes: irange outside 0 .. 8");
  *bytes = dsm_ncc_layout(nullptr, Hu, Wu, irange).bytes;
  return EOGS_OK;
}

int eogs_tsdf_dsm_ncc(int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int f64, int irange, const int32_t* centre,
                      int centre_scale, double* table, eogs_tsdf_dsm_result* result, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const int rc = dsm_check_pair("dsm_ncc", Hu, Wu, u, Hv, Wv, v, irange);
  if (rc != EOGS_OK) return rc;
  if (!result || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_ncc: NULL argument");
  if (ws_bytes < dsm_ncc_layout(nullptr, Hu, Wu, irange).bytes) return fail(EOGS_ERR_WORKSPACE, "dsm_ncc: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  dsm_search(Hu, Wu, u, Hv, Wv, v, f64, irange, centre, centre_scale, table, result, dsm_ncc_layout(ws_base(ws), Hu, Wu, irange), s);
  LAUNCH_TRY(s, false, "dsm_ncc");
  return EOGS_OK;
}

int eogs_tsdf_dsm_shift_bytes(int Hu, int Wu, int Hv, int Wv, int irange, size_t* bytes, int* levels) {
  clear_error();
  if (Hu <= 0 || Wu <= 0 || Hv < Hu || Wv < Wu || !bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_shift_bytes: bad argument");
  if (irange < 0 || irange > EOGS_TSDF_DSM_MAX_IRANGE) return fail(EOGS_ERR_INVALID_ARG, "dsm_shift_bytes: irange outside 0 .. 8");
  const DsmShiftWS w = dsm_shift_layout(nullptr, Hu, Wu, Hv, Wv, irange);
  *bytes = w.bytes;
  if (levels) *levels = w.levels;
  return EOGS_OK;
}

int eogs_tsdf_dsm_shift(int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int f64, int irange, double* tables,
                        eogs_tsdf_dsm_result* results, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const int rc = dsm_check_pair("dsm_shift", Hu, Wu, u, Hv, Wv, v, irange);
  if (rc != EOGS_OK) return rc;
  if (!results || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_shift: NULL argument");
  const DsmShiftWS w = dsm_shift_layout(ws_base(ws), Hu, Wu, Hv, Wv, irange);
  if (ws_bytes < w.bytes) return fail(EOGS_ERR_WORKSPACE, "dsm_shift: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int n = 2 * irange + 1;
  {
    ProfScope ps(PS_DSM_DOWNSAMPLE, s);
    for (int k = 1; k < w.levels; k++) {
      const int src64 = k == 1 ? f64 : 1;
      launch_dsm_downsample(w.hu[k - 1], w.wu[k - 1], k == 1 ? u : (const void*)w.pu[k - 1], src64, w.pu[k], s);
      launch_dsm_downsample(w.hv[k - 1], w.wv[k - 1], k == 1 ? v : (const void*)w.pv[k - 1], src64, w.pv[k], s);
    }
  }
  for (int k = w.levels - 1; k >= 0; k--) {
    // recursive_ncc halves (0, 0) on its way down (dx // 2, dsmr.py:171-172): the coarsest level searches around (0, 0)
    const int32_t* centre = k == w.levels - 1 ? nullptr : &results[k + 1].dx;
    dsm_search(w.hu[k], w.wu[k], k == 0 ? u : (const void*)w.pu[k], w.hv[k], w.wv[k], k == 0 ? v : (const void*)w.pv[k],
               k == 0 ? f64 : 1, irange, centre, 2, tables ? tables + (size_t)k * n * n : nullptr, results + k,
               dsm_ncc_layout(w.ncc, w.hu[k], w.wu[k], irange), s);
  }
  LAUNCH_TRY(s, false, "dsm_shift");
  return EOGS_OK;
}

int eogs_tsdf_dsm_apply_shift(int H, int W, const void* in, int f64, int dx, int dy, double a, double b, double c, double d,
                              void* out, void* stream) {
  clear_error();
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "dsm_apply_shift: bad sizes");
  if ((uint64_t)H * W > ((uint64_t)1 << 31)) return fail(EOGS_ERR_OVERFLOW, "dsm_apply_shift: image too large");
  if (!in || !out || in == out) return fail(EOGS_ERR_INVALID_ARG, "dsm_apply_shift: NULL or aliased argument");
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = blocks_for((int64_t)H * W);
  {
    ProfScope ps(PS_DSM_APPLY, s);
    if (f64) hipLaunchKernelGGL(dsm_apply_shift_kernel<double>, dim3(g), dim3(256), 0, s, H, W, (const double*)in, dx, dy, a, b, c, d, (double*)out);
    else hipLaunchKernelGGL(dsm_apply_shift_kernel<float>, dim3(g), dim3(256), 0, s, H, W, (const float*)in, dx, dy, a, b, c, d, (float*)out);
  }
  LAUNCH_TRY(s, false, "dsm_apply_shift");
  return EOGS_OK;
}

int eogs_tsdf_dsm_mae_bytes(size_t* bytes) {
  clear_error();
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_mae_bytes: NULL argument");
  *bytes = dsm_mae_ws_bytes();
  return EOGS_OK;
}

int eogs_tsdf_dsm_mae(int Hp, int Wp, void* pred, int Hg, int Wg, const void* gt, int f64, int clip_finite, void* diff, double* out,
                      void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (Hp <= 0 || Wp <= 0 || Hg <= 0 || Wg <= 0) return fail(EOGS_ERR_INVALID_ARG, "dsm_mae: bad sizes");
  if ((uint64_t)Hp * Wp > ((uint64_t)1 << 31) || (uint64_t)Hg * Wg > ((uint64_t)1 << 31))
    return fail(EOGS_ERR_OVERFLOW, "dsm_mae: image too large");
  if (!pred || !gt || !diff || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_mae: NULL argument");
  if (ws_bytes < dsm_mae_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "dsm_mae: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws_base(ws);
  const int h = Hp < Hg ? Hp : Hg, w = Wp < Wg ? Wp : Wg;
  const unsigned gb = reduce_blocks((int64_t)Hg * Wg), pb = reduce_blocks((int64_t)Hp * Wp);
  {
    ProfScope ps(PS_DSM_MAE, s);
    if (f64) {
      hipLaunchKernelGGL(dsm_minmax_kernel<double>, dim3(gb), dim3(256), 0, s, (int64_t)Hg * Wg, (const double*)gt, part);
      hipLaunchKernelGGL(dsm_bounds_kernel<double>, dim3(1), dim3(256), 0, s, (int)gb, part, clip_finite, out);
      hipLaunchKernelGGL(dsm_mae_kernel<double>, dim3(pb), dim3(256), 0, s, Hp, Wp, (double*)pred, Wg, (const double*)gt, h, w, out,
                         (double*)diff, part);
    } else {
      hipLaunchKernelGGL(dsm_minmax_kernel<float>, dim3(gb), dim3(256), 0, s, (int64_t)Hg * Wg, (const float*)gt, part);
      hipLaunchKernelGGL(dsm_bounds_kernel<float>, dim3(1), dim3(256), 0, s, (int)gb, part, clip_finite, out);
      hipLaunchKernelGGL(dsm_mae_kernel<float>, dim3(pb), dim3(256), 0, s, Hp, Wp, (float*)pred, Wg, (const float*)gt, h, w, out,
                         (float*)diff, part);
    }
    hipLaunchKernelGGL(dsm_mae_final_kernel, dim3(1), dim3(256), 0, s, (int)pb, part, out);
  }
  LAUNCH_TRY(s, false, "dsm_mae");
  return EOGS_OK;
}

}  // extern "C"
