// gtprep.hip — ground-truth preparation (include/eogs_gtprep.h): pansharpening of the PAN target with the upsampled MSI
// image (pansharpening/algorithm/brovey.py, ihs.py), Pansharploss, Lpan and Lgradient_pan (loss/pansharp_loss.py,
// loss/PAN_loss.py) and the rescalers (utils/rescaler/rescaler.py), paths under src/gaussiansplatting/.
//
// One lane per output pixel in a grid-stride loop: the upsampling taps and weights are computed once per pixel and shared
// by the channels, the small MSI image is read through the caches, PAN / synthesised image are read once and the result
// (or the gradient) is written once with plain stores; the loss never stores the pansharpened image. Sums through
// reduce.h's two stages in float64 — no float atomics, a grid that depends on the shape alone, bitwise reproducible. The
// histogram counts with integer atomics (exact in any order).
#include "api_util.h"
#include "eogs_gtprep.h"
#include "reduce.h"

namespace {

constexpr int GT = 256;          // threads per workgroup
constexpr int GMAXBLK = 1024;    // workgroups per reduction launch: one float64 partial (two for Lgradient_pan) each
constexpr int GCBLK = 256;       // workgroups per channel of the min/max and histogram passes
constexpr int MAXC = EOGS_GTPREP_MAX_CHANNELS;
constexpr int M_TARGET = 3;      // "method" of the kernels below when the target is given (Lpan)

// ---- upsampling taps -------------------------------------------------------------------------------------------------
// torch's area_pixel_compute_source_index, align_corners = False. One rounding: the reference's builds contract the product
// and the subtraction, and simple_brovey's dark pixels (lambda ~ 1e-8 against the 1e-8 of its denominator) show which
__device__ inline float src_index(float scale, int dst) { return fmaf(scale, (float)dst + 0.5f, -0.5f); }

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// cubic convolution, A = -0.75 (torch's get_cubic_upsample_coefficients)
__device__ inline void cubic_taps(int dst, int in, float scale, int (&idx)[4], float (&wt)[4]) {
  const float A = -0.75f;
  const float src = src_index(scale, dst);
  const float fl = floorf(src);
  const int i = (int)fl;
  const float t = src - fl;
  const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
  wt[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  wt[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
  wt[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  wt[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
#pragma unroll
  for (int k = 0; k < 4; k++) idx[k] = clampi(i - 1 + k, 0, in - 1);
}

__device__ inline void linear_taps(int dst, int in, float scale, int (&idx)[4], float (&wt)[4]) {
  float src = src_index(scale, dst);
  if (src < 0.f) src = 0.f;
  int i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  const float lam = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  idx[0] = i0;
  idx[1] = i0 < in - 1 ? i0 + 1 : i0;
  wt[0] = 1.f - lam;
  wt[1] = lam;
  idx[2] = idx[3] = i0;
  wt[2] = wt[3] = 0.f;
}

__device__ inline float clamp_nan(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

struct Shape {
  int C, h, w, H, W;
  float sy, sx, weight;
};

// the pansharpened values of pixel (y, x): t[c] for c < C
template <int METHOD>
__device__ inline void fuse_pixel(const Shape& s, const float* __restrict__ msi, float pan, int y, int x, float (&t)[MAXC]) {
  constexpr bool CUBIC = METHOD == EOGS_GTPREP_BROVEY;
  constexpr int NT = CUBIC ? 4 : 2;
  int iy[4], ix[4];
  float wy[4], wx[4];
  if (CUBIC) {
    cubic_taps(y, s.h, s.sy, iy, wy);
    cubic_taps(x, s.w, s.sx, ix, wx);
  } else {
    linear_taps(y, s.h, s.sy, iy, wy);
    linear_taps(x, s.w, s.sx, ix, wx);
  }
  const size_t plane = (size_t)s.h * s.w;
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; c++) {
    if (c >= s.C) break;
    const float* __restrict__ m = msi + (size_t)c * plane;
    float u = 0.f;
#pragma unroll
    for (int j = 0; j < NT; j++) {
      const float* __restrict__ row = m + (size_t)iy[j] * s.w;
      float r = row[ix[0]] * wx[0];
#pragma unroll
      for (int i = 1; i < NT; i++) r += row[ix[i]] * wx[i];
      u = j == 0 ? r * wy[0] : u + r * wy[j];
    }
    t[c] = u;
    sum = c == 0 ? u : sum + u;
  }
  if (METHOD == EOGS_GTPREP_BROVEY) {
    const float ws = s.weight * sum;
    const float d = ws != ws ? ws : fmaxf(ws, 1e-8f);
    const float dnf = pan / d;
#pragma unroll
    for (int c = 0; c < MAXC; c++)
      if (c < s.C) t[c] = dnf * t[c];
  } else if (METHOD == EOGS_GTPREP_SIMPLE_BROVEY) {
    const float ratio = pan / (sum + 1e-8f);
#pragma unroll
    for (int c = 0; c < MAXC; c++)
      if (c < s.C) t[c] = t[c] * ratio;
  } else {
    const float delta = pan - sum / 3.f;
#pragma unroll
    for (int c = 0; c < MAXC; c++)
      if (c < s.C) t[c] = clamp_nan(t[c] + delta, 0.f, 1.f);
  }
}

enum { MODE_WRITE, MODE_LOSS, MODE_GRAD };

// MODE_WRITE: dst = target. MODE_LOSS: partial[block] = sum (syn - target)^2. MODE_GRAD: dst = (syn - target) * 2 up / N.
// METHOD == M_TARGET: `pan` is the given target of C * H * W elements (Lpan: C = 1, H * W = n).
template <int METHOD, int MODE>
__global__ __launch_bounds__(GT) void fuse_kernel(Shape s, const float* __restrict__ msi, const float* __restrict__ pan,
                                                  const float* __restrict__ syn, const float* __restrict__ upstream,
                                                  float* __restrict__ dst, double* __restrict__ partial) {
  const int64_t n = (int64_t)s.H * s.W;
  float coef = 0.f;
  if (MODE == MODE_GRAD) coef = (2.f / (float)((double)n * (double)s.C)) * (upstream ? upstream[0] : 1.f);
  double acc[1] = {0.};
  for (int64_t p = (int64_t)blockIdx.x * GT + threadIdx.x; p < n; p += (int64_t)gridDim.x * GT) {
    float t[MAXC];
    if (METHOD == M_TARGET) {
      t[0] = pan[p];
    } else {
      const int y = (int)(p / s.W), x = (int)(p - (int64_t)y * s.W);
      fuse_pixel<METHOD == M_TARGET ? 0 : METHOD>(s, msi, pan[p], y, x, t);
    }
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
      if (c >= s.C) break;
      const size_t q = (size_t)c * (size_t)n + (size_t)p;
      if (MODE == MODE_WRITE) {
        dst[q] = t[c];
      } else {
        const float d = syn[q] - t[c];
        if (MODE == MODE_LOSS) acc[0] += (double)d * (double)d;
        else dst[q] = d * coef;
      }
    }
  }
  if (MODE == MODE_LOSS) wg_partials<GT>(acc, partial + blockIdx.x);
}

// K columns of partials [nblk][K], summed by one workgroup in a fixed order; out = sum_k column_k / count
template <int K>
__global__ __launch_bounds__(GT) void mean_final_kernel(const double* __restrict__ partial, int nblk, double count,
                                                        float* __restrict__ out) {
  __shared__ double s_red[GT / 64];
  double res = 0.;
  for (int k = 0; k < K; k++) res += column_sum<GT>(partial + k, nblk, K, s_red) / count;
  if (threadIdx.x == 0) out[0] = (float)res;
}

// ---- Lgradient_pan -----------------------------------------------------------------------------------------------------
// torch.gradient (unit spacing, edge order 1) of d = pan - gt along one axis at position i of n; `o` = offset of position 0,
// `st` = stride of the axis
__device__ inline float diff_at(const float* __restrict__ pan, const float* __restrict__ gt, size_t q) { return pan[q] - gt[q]; }

__device__ inline float grad_at(const float* __restrict__ pan, const float* __restrict__ gt, size_t o, size_t st, int i, int n) {
  if (i == 0) return diff_at(pan, gt, o + st) - diff_at(pan, gt, o);
  if (i == n - 1) return diff_at(pan, gt, o + (size_t)(n - 1) * st) - diff_at(pan, gt, o + (size_t)(n - 2) * st);
  return (diff_at(pan, gt, o + (size_t)(i + 1) * st) - diff_at(pan, gt, o + (size_t)(i - 1) * st)) / 2.f;
}

// the coefficient of d[j] in the gradient at position i
__device__ inline float grad_coef(int i, int j, int n) {
  if (i == 0) return (j == 1 ? 1.f : 0.f) - (j == 0 ? 1.f : 0.f);
  if (i == n - 1) return (j == n - 1 ? 1.f : 0.f) - (j == n - 2 ? 1.f : 0.f);
  return 0.5f * ((j == i + 1 ? 1.f : 0.f) - (j == i - 1 ? 1.f : 0.f));
}

// sum over the gradients that read d[j] of gradient x coefficient: the transposed stencil as a gather
__device__ inline float grad_transposed(const float* __restrict__ pan, const float* __restrict__ gt, size_t o, size_t st, int j, int n) {
  float a = 0.f;
  for (int i = j - 1; i <= j + 1; i++) {
    if (i < 0 || i >= n) continue;
    const float c = grad_coef(i, j, n);
    if (c != 0.f) a += c * grad_at(pan, gt, o, st, i, n);
  }
  return a;
}

template <bool BACKWARD>
__global__ __launch_bounds__(GT) void grad_l2_kernel(int64_t B, int H, int W, const float* __restrict__ pan,
                                                     const float* __restrict__ gt, const float* __restrict__ upstream,
                                                     float* __restrict__ g_pan, double* __restrict__ partial) {
  const int64_t hw = (int64_t)H * W, n = B * hw;
  float coef = 0.f;
  if (BACKWARD) coef = (2.f / (float)(double)n) * (upstream ? upstream[0] : 1.f);
  double a[2] = {0., 0.};  // sums of the squared vertical and horizontal gradients
  for (int64_t p = (int64_t)blockIdx.x * GT + threadIdx.x; p < n; p += (int64_t)gridDim.x * GT) {
    const int64_t b = p / hw;
    const int64_t r = p - b * hw;
    const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
    const size_t col0 = (size_t)(b * hw) + (size_t)x;      // position 0 of the pixel's column, stride W
    const size_t row0 = (size_t)(b * hw) + (size_t)y * W;  // position 0 of the pixel's row, stride 1
    if (BACKWARD) {
      g_pan[p] = (grad_transposed(pan, gt, col0, (size_t)W, y, H) + grad_transposed(pan, gt, row0, 1, x, W)) * coef;
    } else {
      const float gy = grad_at(pan, gt, col0, (size_t)W, y, H), gx = grad_at(pan, gt, row0, 1, x, W);
      a[0] += (double)gy * (double)gy;
      a[1] += (double)gx * (double)gx;
    }
  }
  if (!BACKWARD) wg_partials<GT>(a, partial + (size_t)blockIdx.x * 2);
}

// ---- rescalers ---------------------------------------------------------------------------------------------------------
// torch.min / torch.max: a NaN on either side wins (fmin / fmax, and so wave_min / wave_max of reduce.h, pass over it)
__device__ inline float min_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fminf(a, b); }
__device__ inline float max_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

// min and max over the workgroup on thread 0; s_mm holds 2 * GT / 64 floats
__device__ inline void wg_minmax(float& lo, float& hi, float* s_mm) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    lo = min_nan(lo, __shfl_xor(lo, o, 64));
    hi = max_nan(hi, __shfl_xor(hi, o, 64));
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    s_mm[2 * wv] = lo;
    s_mm[2 * wv + 1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < GT / 64; k++) {
      lo = min_nan(lo, s_mm[2 * k]);
      hi = max_nan(hi, s_mm[2 * k + 1]);
    }
}

// grid (nblk, C): partial[c][block] = {min, max} of the block's share of channel c
__global__ __launch_bounds__(GT) void minmax_kernel(int64_t n, const float* __restrict__ x, float* __restrict__ partial) {
  __shared__ float s_mm[2 * GT / 64];
  const float* __restrict__ xc = x + (size_t)blockIdx.y * (size_t)n;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GT) {
    const float v = xc[i];
    lo = min_nan(lo, v);
    hi = max_nan(hi, v);
  }
  wg_minmax(lo, hi, s_mm);
  if (threadIdx.x == 0) {
    float* o = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    o[0] = lo;
    o[1] = hi;
  }
}

// grid (C): mm[c] = the extrema of channel c's nblk partials
__global__ __launch_bounds__(GT) void minmax_final_kernel(int nblk, const float* __restrict__ partial, float* __restrict__ mm) {
  __shared__ float s_mm[2 * GT / 64];
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int b = threadIdx.x; b < nblk; b += GT) {
    const float* p = partial + ((size_t)blockIdx.x * nblk + b) * 2;
    lo = min_nan(lo, p[0]);
    hi = max_nan(hi, p[1]);
  }
  wg_minmax(lo, hi, s_mm);
  if (threadIdx.x == 0) {
    mm[2 * blockIdx.x] = lo;
    mm[2 * blockIdx.x + 1] = hi;
  }
}

// grid (nblk, C)
__global__ __launch_bounds__(GT) void rescale_kernel(int64_t n, const float* __restrict__ x, const float* __restrict__ mm,
                                                     float* __restrict__ out) {
  const float lo = mm[2 * blockIdx.y], hi = mm[2 * blockIdx.y + 1];
  const float den = (hi - lo) + 1e-8f;
  const size_t base = (size_t)blockIdx.y * (size_t)n;
  for (int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GT) out[base + i] = (x[base + i] - lo) / den;
}

__global__ __launch_bounds__(GT) void clamp_kernel(int64_t n, const float* __restrict__ x, float lo, float hi, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GT) out[i] = clamp_nan(x[i], lo, hi);
}

// ---- histogram equalisation ----------------------------------------------------------------------------------------------
__device__ inline int to_level(float v) {
  const float y = v * 255.f;
  if (y != y) return 0;
  return (int)fminf(fmaxf(y, 0.f), 255.f);
}

__global__ __launch_bounds__(GT) void hist_zero_kernel(int count, unsigned* __restrict__ hist) {
  const int i = blockIdx.x * GT + threadIdx.x;
  if (i < count) hist[i] = 0u;
}

// grid (nblk, C): the block's histogram in LDS, then one integer atomic per non-empty bin
__global__ __launch_bounds__(GT) void hist_kernel(int64_t n, const float* __restrict__ x, unsigned* __restrict__ hist) {
  __shared__ unsigned s_hist[256];
  s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const float* __restrict__ xc = x + (size_t)blockIdx.y * (size_t)n;
  for (int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GT) atomicAdd(&s_hist[to_level(xc[i])], 1u);
  __syncthreads();
  const unsigned v = s_hist[threadIdx.x];
  if (v) atomicAdd(&hist[blockIdx.y * 256 + threadIdx.x], v);
}

// grid (C): the channel's lookup table from its histogram (one scan over 256 bins)
__global__ __launch_bounds__(GT) void hist_lut_kernel(const unsigned* __restrict__ hist, int* __restrict__ lut) {
  __shared__ long long s_cum[256];
  __shared__ long long s_step;
  const unsigned* h = hist + blockIdx.x * 256;
  if (threadIdx.x == 0) {
    long long total = 0, last = 0;
    for (int v = 0; v < 256; v++) {
      total += (long long)h[v];
      s_cum[v] = total;
      if (h[v]) last = (long long)h[v];
    }
    s_step = (total - last) / 255;
  }
  __syncthreads();
  const long long step = s_step;
  const int v = threadIdx.x;
  int r = v;
  if (step != 0) {
    r = 0;
    if (v > 0) {
      const long long q = (s_cum[v - 1] + step / 2) / step;
      r = (int)(q < 0 ? 0 : (q > 255 ? 255 : q));
    }
  }
  lut[blockIdx.x * 256 + v] = r;
}

// grid (nblk, C)
__global__ __launch_bounds__(GT) void hist_apply_kernel(int64_t n, const float* __restrict__ x, const int* __restrict__ lut,
                                                        float* __restrict__ out) {
  __shared__ int s_lut[256];
  s_lut[threadIdx.x] = lut[blockIdx.y * 256 + threadIdx.x];
  __syncthreads();
  const size_t base = (size_t)blockIdx.y * (size_t)n;
  for (int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GT)
    out[base + i] = (float)s_lut[to_level(x[base + i])] / 255.f;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
size_t gtprep_ws_bytes(int C) {
  const size_t loss = (size_t)GMAXBLK * 2 * sizeof(double);
  const size_t per_channel = (size_t)C * GCBLK * 2 * sizeof(float);  // min/max partials; the histogram + table need as much
  return (loss > per_channel ? loss : per_channel) + 256;
}

int shape_check(const char* who, int method, int C, int h, int w, int H, int W) {
  if (method != EOGS_GTPREP_BROVEY && method != EOGS_GTPREP_SIMPLE_BROVEY && method != EOGS_GTPREP_IHS)
    return fail(EOGS_ERR_INVALID_ARG, "%s: unknown method", who);
  if (C < 1 || C > MAXC) return fail(EOGS_ERR_INVALID_ARG, "%s: 1 to 8 MSI channels", who);
  if (method == EOGS_GTPREP_IHS && C != 3) return fail(EOGS_ERR_INVALID_ARG, "%s: ihs takes 3 MSI channels", who);
  if (h < 1 || w < 1 || H < 1 || W < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes", who);
  return EOGS_OK;
}

Shape make_shape(int C, int h, int w, int H, int W, float weight) {
  Shape s;
  s.C = C, s.h = h, s.w = w, s.H = H, s.W = W;
  s.sy = (float)h / (float)H;
  s.sx = (float)w / (float)W;
  s.weight = weight;
  return s;
}

template <int MODE>
void launch_fuse(int method, int nb, hipStream_t st, const Shape& s, const float* msi, const float* pan, const float* syn,
                 const float* upstream, float* dst, double* partial) {
  switch (method) {
    case EOGS_GTPREP_BROVEY:
      hipLaunchKernelGGL((fuse_kernel<EOGS_GTPREP_BROVEY, MODE>), dim3(nb), dim3(GT), 0, st, s, msi, pan, syn, upstream, dst, partial);
      break;
    case EOGS_GTPREP_SIMPLE_BROVEY:
      hipLaunchKernelGGL((fuse_kernel<EOGS_GTPREP_SIMPLE_BROVEY, MODE>), dim3(nb), dim3(GT), 0, st, s, msi, pan, syn, upstream, dst, partial);
      break;
    case EOGS_GTPREP_IHS:
      hipLaunchKernelGGL((fuse_kernel<EOGS_GTPREP_IHS, MODE>), dim3(nb), dim3(GT), 0, st, s, msi, pan, syn, upstream, dst, partial);
      break;
    default:
      hipLaunchKernelGGL((fuse_kernel<M_TARGET, MODE>), dim3(nb), dim3(GT), 0, st, s, msi, pan, syn, upstream, dst, partial);
  }
}

// Lpan's n elements as one channel of a (rows, cols) image whose sizes fit an int
int flat_shape(int64_t n, Shape& s) {
  if (n <= 0) return 0;
  int64_t cols = n, rows = 1;
  while (cols > 0x7fffffffll) {
    if (cols % 2) return 0;  // (more than 2^31 elements with an odd factor left: refused)
    cols /= 2, rows *= 2;
  }
  s = make_shape(1, 1, 1, (int)rows, (int)cols, 0.f);
  return 1;
}

}  // namespace

extern "C" {

int eogs_gtprep_bytes(int C, size_t* bytes) {
  clear_error();
  if (C < 1 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "gtprep_bytes: bad argument");
  *bytes = gtprep_ws_bytes(C);
  return EOGS_OK;
}

int eogs_gtprep_pansharp(int method, int C, int h, int w, int H, int W, const float* msi, const float* pan, float weight,
                         float* out, void* stream) {
  clear_error();
  const int rc = shape_check("gtprep_pansharp", method, C, h, w, H, W);
  if (rc != EOGS_OK) return rc;
  if (!msi || !pan || !out) return fail(EOGS_ERR_INVALID_ARG, "gtprep_pansharp: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  launch_fuse<MODE_WRITE>(method, capped_blocks((int64_t)H * W, GT, 1 << 20), s, make_shape(C, h, w, H, W, weight), msi, pan, nullptr, nullptr,
                          out, nullptr);
  LAUNCH_TRY(s, false, "gtprep_pansharp");
  return EOGS_OK;
}

int eogs_gtprep_pansharp_l2_forward(int method, int C, int h, int w, int H, int W, const float* syn, const float* msi,
                                    const float* pan, float weight, float* out, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const int rc = shape_check("gtprep_pansharp_l2_forward", method, C, h, w, H, W);
  if (rc != EOGS_OK) return rc;
  if (!syn || !msi || !pan || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "gtprep_pansharp_l2_forward: NULL argument");
  if (ws_bytes < gtprep_ws_bytes(C)) return fail(EOGS_ERR_WORKSPACE, "gtprep_pansharp_l2_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(ws_base(ws));
  const int nb = capped_blocks((int64_t)H * W, GT, GMAXBLK);
  launch_fuse<MODE_LOSS>(method, nb, s, make_shape(C, h, w, H, W, weight), msi, pan, syn, nullptr, nullptr, partial);
  hipLaunchKernelGGL(mean_final_kernel<1>, dim3(1), dim3(GT), 0, s, (const double*)partial, nb, (double)C * (double)H * (double)W, out);
  LAUNCH_TRY(s, false, "gtprep_pansharp_l2_fwd");
  return EOGS_OK;
}

int eogs_gtprep_pansharp_l2_backward(int method, int C, int h, int w, int H, int W, const float* syn, const float* msi,
                                     const float* pan, float weight, const float* upstream, float* g_syn, void* stream) {
  clear_error();
  const int rc = shape_check("gtprep_pansharp_l2_backward", method, C, h, w, H, W);
  if (rc != EOGS_OK) return rc;
  if (!syn || !msi || !pan || !g_syn) return fail(EOGS_ERR_INVALID_ARG, "gtprep_pansharp_l2_backward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  launch_fuse<MODE_GRAD>(method, capped_blocks((int64_t)H * W, GT, 1 << 20), s, make_shape(C, h, w, H, W, weight), msi, pan, syn, upstream,
                         g_syn, nullptr);
  LAUNCH_TRY(s, false, "gtprep_pansharp_l2_bwd");
  return EOGS_OK;
}

int eogs_gtprep_l2_forward(int64_t n, const float* image, const float* target, float* out, void* ws, size_t ws_bytes,
                           void* stream) {
  clear_error();
  Shape sh;
  if (!flat_shape(n, sh)) return fail(EOGS_ERR_INVALID_ARG, "gtprep_l2_forward: bad size");
  if (!image || !target || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "gtprep_l2_forward: NULL argument");
  if (ws_bytes < gtprep_ws_bytes(1)) return fail(EOGS_ERR_WORKSPACE, "gtprep_l2_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(ws_base(ws));
  const int nb = capped_blocks(n, GT, GMAXBLK);
  launch_fuse<MODE_LOSS>(M_TARGET, nb, s, sh, nullptr, target, image, nullptr, nullptr, partial);
  hipLaunchKernelGGL(mean_final_kernel<1>, dim3(1), dim3(GT), 0, s, (const double*)partial, nb, (double)n, out);
  LAUNCH_TRY(s, false, "gtprep_l2_fwd");
  return EOGS_OK;
}

int eogs_gtprep_l2_backward(int64_t n, const float* image, const float* target, const float* upstream, float* g_image,
                            void* stream) {
  clear_error();
  Shape sh;
  if (!flat_shape(n, sh)) return fail(EOGS_ERR_INVALID_ARG, "gtprep_l2_backward: bad size");
  if (!image || !target || !g_image) return fail(EOGS_ERR_INVALID_ARG, "gtprep_l2_backward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  launch_fuse<MODE_GRAD>(M_TARGET, capped_blocks(n, GT, 1 << 20), s, sh, nullptr, target, image, upstream, g_image, nullptr);
  LAUNCH_TRY(s, false, "gtprep_l2_bwd");
  return EOGS_OK;
}

int eogs_gtprep_grad_l2_forward(int64_t B, int H, int W, const float* pan, const float* gt, float* out, void* ws,
                                size_t ws_bytes, void* stream) {
  clear_error();
  if (B < 1 || H < 2 || W < 2) return fail(EOGS_ERR_INVALID_ARG, "gtprep_grad_l2_forward: bad sizes (H and W must be at least 2)");
  if (!pan || !gt || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "gtprep_grad_l2_forward: NULL argument");
  if (ws_bytes < gtprep_ws_bytes(1)) return fail(EOGS_ERR_WORKSPACE, "gtprep_grad_l2_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(ws_base(ws));
  const int64_t n = B * (int64_t)H * W;
  const int nb = capped_blocks(n, GT, GMAXBLK);
  hipLaunchKernelGGL(grad_l2_kernel<false>, dim3(nb), dim3(GT), 0, s, B, H, W, pan, gt, (const float*)nullptr, (float*)nullptr, partial);
  hipLaunchKernelGGL(mean_final_kernel<2>, dim3(1), dim3(GT), 0, s, (const double*)partial, nb, (double)n, out);
  LAUNCH_TRY(s, false, "gtprep_grad_l2_fwd");
  return EOGS_OK;
}

int eogs_gtprep_grad_l2_backward(int64_t B, int H, int W, const float* pan, const float* gt, const float* upstream,
                                 float* g_pan, void* stream) {
  clear_error();
  if (B < 1 || H < 2 || W < 2) return fail(EOGS_ERR_INVALID_ARG, "gtprep_grad_l2_backward: bad sizes (H and W must be at least 2)");
  if (!pan || !gt || !g_pan) return fail(EOGS_ERR_INVALID_ARG, "gtprep_grad_l2_backward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_l2_kernel<true>, dim3(capped_blocks(B * (int64_t)H * W, GT, 1 << 20)), dim3(GT), 0, s, B, H, W, pan, gt, upstream, g_pan,
                     (double*)nullptr);
  LAUNCH_TRY(s, false, "gtprep_grad_l2_bwd");
  return EOGS_OK;
}

int eogs_gtprep_minmax(int C, int64_t n, const float* x, float* mm, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (C < 1 || C > 65535 || n < 1) return fail(EOGS_ERR_INVALID_ARG, "gtprep_minmax: bad sizes");
  if (!x || !mm || !ws) return fail(EOGS_ERR_INVALID_ARG, "gtprep_minmax: NULL argument");
  if (ws_bytes < gtprep_ws_bytes(C)) return fail(EOGS_ERR_WORKSPACE, "gtprep_minmax: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* partial = reinterpret_cast<float*>(ws_base(ws));
  const int nb = capped_blocks(n, GT, GCBLK);
  hipLaunchKernelGGL(minmax_kernel, dim3(nb, C), dim3(GT), 0, s, n, x, partial);
  hipLaunchKernelGGL(minmax_final_kernel, dim3(C), dim3(GT), 0, s, nb, (const float*)partial, mm);
  LAUNCH_TRY(s, false, "gtprep_minmax");
  return EOGS_OK;
}

int eogs_gtprep_rescale(int C, int64_t n, const float* x, const float* mm, float* out, void* stream) {
  clear_error();
  if (C < 1 || C > 65535 || n < 1) return fail(EOGS_ERR_INVALID_ARG, "gtprep_rescale: bad sizes");
  if (!x || !mm || !out) return fail(EOGS_ERR_INVALID_ARG, "gtprep_rescale: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rescale_kernel, dim3(capped_blocks(n, GT, 1 << 16), C), dim3(GT), 0, s, n, x, mm, out);
  LAUNCH_TRY(s, false, "gtprep_rescale");
  return EOGS_OK;
}

int eogs_gtprep_clamp(int64_t n, const float* x, float lo, float hi, float* out, void* stream) {
  clear_error();
  if (n < 1) return fail(EOGS_ERR_INVALID_ARG, "gtprep_clamp: bad size");
  if (!x || !out) return fail(EOGS_ERR_INVALID_ARG, "gtprep_clamp: NULL argument");
  if (lo != lo || hi != hi) return fail(EOGS_ERR_INVALID_ARG, "gtprep_clamp: the bounds are numbers");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(clamp_kernel, dim3(capped_blocks(n, GT, 1 << 20)), dim3(GT), 0, s, n, x, lo, hi, out);
  LAUNCH_TRY(s, false, "gtprep_clamp");
  return EOGS_OK;
}

int eogs_gtprep_equalize(int C, int64_t n, const float* x, float* out, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (C < 1 || C > 65535 || n < 1 || n > 0x7fffffffll) return fail(EOGS_ERR_INVALID_ARG, "gtprep_equalize: bad sizes (n < 2^31)");
  if (!x || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "gtprep_equalize: NULL argument");
  if (x == out) return fail(EOGS_ERR_INVALID_ARG, "gtprep_equalize: out needs memory of its own");
  if (ws_bytes < gtprep_ws_bytes(C)) return fail(EOGS_ERR_WORKSPACE, "gtprep_equalize: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned* hist = reinterpret_cast<unsigned*>(ws_base(ws));
  int* lut = reinterpret_cast<int*>(hist + (size_t)C * 256);
  const int nb = capped_blocks(n, GT, GCBLK);
  hipLaunchKernelGGL(hist_zero_kernel, dim3(C), dim3(GT), 0, s, C * 256, hist);
  hipLaunchKernelGGL(hist_kernel, dim3(nb, C), dim3(GT), 0, s, n, x, hist);
  hipLaunchKernelGGL(hist_lut_kernel, dim3(C), dim3(GT), 0, s, (const unsigned*)hist, lut);
  hipLaunchKernelGGL(hist_apply_kernel, dim3(capped_blocks(n, GT, 1 << 16), C), dim3(GT), 0, s, n, x, (const int*)lut, out);
  LAUNCH_TRY(s, false, "gtprep_equalize");
  return EOGS_OK;
}

}  // extern "C"
