// nll.hip — the transient-uncertainty term of the training loss (include/eogs_nll.h): the Gaussian negative
// log-likelihood of an image under a per-pixel variance, the variance given directly or formed in the kernel from a
// camera's transient mask, v = (clip(m, 0, 1) + floor)^2. Reference semantics: train_pan.py:433-449 over
// torch.nn.functional.gaussian_nll_loss.
//
// Two streaming passes, HBM-bound by construction: the forward reads 2C+1 planes, the backward reads them again and writes
// C+1. A lane owns a UNIT of four neighbouring pixels and loops over the planes, so the per-pixel work (clip, square,
// reciprocal, log) is done once and the sum over the planes of the mask's gradient needs no cross-lane step. With H W a
// multiple of four and 16-byte aligned planes a unit is one 16-byte load or store per plane; otherwise the same unit is
// read with scalar loads (and a last unit of fewer than four pixels is the scalar tail). Which of the two paths runs
// changes no bit: the order of the arithmetic is the unit order in both.
//
// Arithmetic: the planes are float32, the per-element arithmetic is float64 (x - t, its square, the reciprocal of the
// variance, the sum over the planes), logf is taken of the float32-rounded clamped variance. That costs a dozen float64
// operations per element beside (2C+1) 4 loaded bytes. Sums: float64 per lane, per wave, per workgroup, then one workgroup
// combines the partials in a fixed order; the mask's standard deviation from (n, mean, M2) triples merged by Chan's rule,
// never from a sum of squares — a constant mask gives exactly 0. No atomics, a grid that depends on the shape alone.
#include "api_util.h"
#include "eogs_nll.h"
#include "reduce.h"

namespace {

constexpr int NT = 256;         // threads per workgroup
constexpr int NMAXBLK = 1024;   // workgroups of the forward (4 per CU); partials live in the caller's workspace
constexpr int NK = 6;           // doubles per workgroup partial: loss sum, negatives, outside [0, 1], then n, mean, M2
constexpr int UNIT = 4;         // pixels per lane and trip

struct Moments {
  double n, mean, m2;
};

// Chan et al.: the moments of the union of two samples. An empty side leaves the other untouched; equal means add nothing.
__device__ inline Moments chan(const Moments a, const Moments b) {
  if (b.n == 0.) return a;
  if (a.n == 0.) return b;
  const double n = a.n + b.n, d = b.mean - a.mean, r = b.n / n;
  return {n, a.mean + d * r, (a.m2 + b.m2) + (d * d) * (a.n * r)};
}

// the moments of up to four values: the mean first, then the squared distances from it
__device__ inline Moments unit_moments(const float (&x)[UNIT], int nb) {
  double s = 0.;
  for (int j = 0; j < nb; j++) s += (double)x[j];
  const double mean = nb == UNIT ? 0.25 * s : s / (double)nb;
  double m2 = 0.;
  for (int j = 0; j < nb; j++) {
    const double d = (double)x[j] - mean;
    m2 += d * d;
  }
  return {(double)nb, mean, m2};
}

// lane 0 of the wave returns the moments of all 64 lanes, merged pairwise in a fixed tree
__device__ inline Moments wave_moments(Moments a) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    Moments b;
    b.n = __shfl_down(a.n, o, 64);
    b.mean = __shfl_down(a.mean, o, 64);
    b.m2 = __shfl_down(a.m2, o, 64);
    a = chan(a, b);
  }
  return a;
}

// thread 0 returns the workgroup's moments: the wave tree, then waves 0, 1, 2, 3 left to right
__device__ inline Moments wg_moments(Moments a, Moments* s_mom) {
  a = wave_moments(a);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_mom[threadIdx.x >> 6] = a;
  __syncthreads();
  return chan(chan(chan(s_mom[0], s_mom[1]), s_mom[2]), s_mom[3]);
}

// pixels [p0, p0 + nb) of one plane; lanes past the end of a short unit read nothing
__device__ inline void load_unit(const float* __restrict__ plane, int64_t p0, int nb, bool vec, float (&o)[UNIT]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(plane + p0);
    o[0] = q.x, o[1] = q.y, o[2] = q.z, o[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < UNIT; j++) o[j] = j < nb ? plane[p0 + j] : 0.f;
  }
}

__device__ inline void store_unit(float* __restrict__ plane, int64_t p0, int nb, bool vec, const float (&v)[UNIT]) {
  if (vec) {
    *reinterpret_cast<float4*>(plane + p0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < UNIT; j++)
      if (j < nb) plane[p0 + j] = v[j];
  }
}

// What one entry of the mask or variance plane gives its pixel: 1 / vc, and 2 s [0 <= m <= 1] for the mask's gradient
// (mask mode; 1 otherwise). vc is returned through `vc32`, rounded to float32, for logf.
struct Variance {
  double inv, chain;
  float vc32;
};

__device__ inline Variance variance_of(float e, bool mask, double floor_, double eps) {
  double v, chain = 1.;
  if (mask) {
    const float c = e < 0.f ? 0.f : (e > 1.f ? 1.f : e);  // selects: a NaN stays, as through torch's clip
    const double s = (double)c + floor_;
    v = s * s;
    chain = (e >= 0.f && e <= 1.f) ? 2. * s : 0.;          // inclusive, as torch's clamp backward; -0 is inside
  } else {
    v = (double)e;
  }
  const double vc = v < eps ? eps : v;
  return {1. / vc, chain, (float)vc};
}

__global__ __launch_bounds__(NT) void nll_fwd_kernel(int planes, int64_t HW, bool mask, int var_planes, bool vec,
                                                     const float* __restrict__ input, const float* __restrict__ target,
                                                     const float* __restrict__ vm, float floor_, float eps,
                                                     double* __restrict__ partial) {
  __shared__ Moments s_mom[NT / 64];
  __shared__ double s_red[NT / 64];
  const int64_t units = (HW + UNIT - 1) / UNIT;
  const double fl = (double)floor_, ep = (double)eps;
  double loss = 0., neg = 0., outside = 0.;
  Moments mom = {0., 0., 0.};
  for (int64_t u = (int64_t)blockIdx.x * NT + threadIdx.x; u < units; u += (int64_t)gridDim.x * NT) {
    const int64_t p0 = u * UNIT;
    const int nb = (int)(HW - p0 < UNIT ? HW - p0 : UNIT);
    double inv[UNIT], lg[UNIT];
    for (int c = 0; c < planes; c++) {
      if (c == 0 || var_planes > 1) {  // this plane's own variance, or the one every plane shares
        float e[UNIT];
        load_unit(vm + (int64_t)c * HW, p0, nb, vec, e);
        mom = chan(mom, unit_moments(e, nb));
#pragma unroll
        for (int j = 0; j < UNIT; j++) {
          if (j >= nb) continue;
          if (mask) outside += (e[j] < 0.f || e[j] > 1.f) ? 1. : 0.;
          else neg += e[j] < 0.f ? 1. : 0.;
          const Variance q = variance_of(e[j], mask, fl, ep);
          inv[j] = q.inv;
          lg[j] = (double)logf(q.vc32);
        }
      }
      float x[UNIT], t[UNIT];
      load_unit(input + (int64_t)c * HW, p0, nb, vec, x);
      load_unit(target + (int64_t)c * HW, p0, nb, vec, t);
#pragma unroll
      for (int j = 0; j < UNIT; j++) {
        if (j >= nb) continue;
        const double d = (double)x[j] - (double)t[j];
        loss += 0.5 * (lg[j] + (d * d) * inv[j]);
      }
    }
  }
  // Three wg_sum calls, not wg_partials. The forward launch group (this kernel and nll_final_kernel) against the parent
  // build, alternating processes, three turns each, median [min, max] in microseconds at 3 x 1024^2, 3 x 2048^2 and
  // 1 x 4096^2. With wg_partials here and a pass per column in nll_final_kernel: 16.8 [16.7, 17.0] -> 18.4 [18.3, 18.5],
  // 31.0 [31.0, 31.8] -> 33.3 [33.2, 33.5], 64.6 [64.3, 64.9] -> 70.9 [70.8, 71.8]: the final kernel's grid is 1024 rows
  // at all three sizes, so what grows with the size is this kernel's (registers and occupancy were the same). As it
  // stands, five turns each: 16.4 [16.2, 16.7] -> 16.3 [16.2, 16.6], 30.4 [30.2, 30.6] -> 30.3 [30.2, 30.6],
  // 66.0 [65.4, 67.7] -> 67.0 [66.3, 67.7].
  loss = wg_sum(loss, s_red);
  neg = wg_sum(neg, s_red);
  outside = wg_sum(outside, s_red);
  mom = wg_moments(mom, s_mom);
  if (threadIdx.x == 0) {
    double* row = partial + (size_t)blockIdx.x * NK;
    row[0] = loss, row[1] = neg, row[2] = outside, row[3] = mom.n, row[4] = mom.mean, row[5] = mom.m2;
  }
}

// one workgroup: the three plain sums column by column; for the moments lane t merges the partials of workgroups t,
// t + NT, ... in that order, then the workgroup's tree
__global__ __launch_bounds__(NT) void nll_final_kernel(const double* __restrict__ partial, int nblk, double N, bool full,
                                                       bool sum, const float* __restrict__ weight, float* __restrict__ out) {
  __shared__ Moments s_mom[NT / 64];
  __shared__ double s_red[NT / 64];
  double tot[3];
  column_sums<NT>(partial, nblk, NK, tot, s_red);
  const double loss = tot[0], neg = tot[1], outside = tot[2];
  Moments mom = {0., 0., 0.};
  for (int b = threadIdx.x; b < nblk; b += NT) {
    const double* row = partial + (size_t)b * NK;
    mom = chan(mom, Moments{row[3], row[4], row[5]});
  }
  mom = wg_moments(mom, s_mom);
  if (threadIdx.x != 0) return;
  const double half_log_2pi = 0.91893853320467274178;
  double l = sum ? loss : loss / N;
  if (full) l += sum ? N * half_log_2pi : half_log_2pi;
  const float lf = (float)l;
  const float w = weight ? weight[0] : 1.f;
  out[0] = lf;
  out[1] = w == 0.f ? 0.f : w * lf;
  out[2] = (float)mom.mean;
  out[3] = (float)sqrt(mom.m2 / (mom.n - 1.));  // one entry: 0 / 0, Tensor.std()'s NaN
  out[4] = (float)neg;
  out[5] = (float)outside;
}

__global__ __launch_bounds__(NT) void nll_bwd_kernel(int planes, int64_t HW, bool mask, int var_planes, bool vec, bool sum,
                                                     const float* __restrict__ input, const float* __restrict__ target,
                                                     const float* __restrict__ vm, float floor_, float eps,
                                                     const float* __restrict__ weight, const float* __restrict__ g_loss,
                                                     const float* __restrict__ g_total, float* __restrict__ g_input,
                                                     float* __restrict__ g_vm) {
  const int64_t units = (HW + UNIT - 1) / UNIT;
  const float w = weight ? weight[0] : 1.f;
  const float k = ((g_total && w != 0.f) ? g_total[0] * w : 0.f) + (g_loss ? g_loss[0] : 0.f);
  const bool off = k == 0.f;  // nothing upstream: exact zeros, a NaN pixel is not passed on
  const double kn = sum ? (double)k : (double)k / ((double)planes * (double)HW);
  const double fl = (double)floor_, ep = (double)eps;
  for (int64_t u = (int64_t)blockIdx.x * NT + threadIdx.x; u < units; u += (int64_t)gridDim.x * NT) {
    const int64_t p0 = u * UNIT;
    const int nb = (int)(HW - p0 < UNIT ? HW - p0 : UNIT);
    double inv[UNIT], chain[UNIT], gv[UNIT] = {0., 0., 0., 0.};
    for (int c = 0; c < planes; c++) {
      if (c == 0 || var_planes > 1) {
        float e[UNIT];
        load_unit(vm + (int64_t)c * HW, p0, nb, vec, e);
#pragma unroll
        for (int j = 0; j < UNIT; j++) {
          const Variance q = variance_of(e[j], mask, fl, ep);
          inv[j] = q.inv;
          chain[j] = q.chain;
        }
      }
      float x[UNIT], t[UNIT], gi[UNIT], gp[UNIT];
      load_unit(input + (int64_t)c * HW, p0, nb, vec, x);
      load_unit(target + (int64_t)c * HW, p0, nb, vec, t);
#pragma unroll
      for (int j = 0; j < UNIT; j++) {
        const double d = (double)x[j] - (double)t[j];
        const double q = d * inv[j];
        const double dv = (0.5 * kn) * (inv[j] * (1. - d * q));  // passed on also where v < eps
        gi[j] = off ? 0.f : (float)(kn * q);
        gp[j] = off ? 0.f : (float)dv;
        gv[j] += dv;
      }
      if (g_input) store_unit(g_input + (int64_t)c * HW, p0, nb, vec, gi);
      if (g_vm && var_planes > 1) store_unit(g_vm + (int64_t)c * HW, p0, nb, vec, gp);
    }
    if (g_vm && var_planes == 1) {
      float g[UNIT];
#pragma unroll
      for (int j = 0; j < UNIT; j++) g[j] = (off || chain[j] == 0.) ? 0.f : (float)(gv[j] * chain[j]);
      store_unit(g_vm, p0, nb, vec, g);
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

static size_t nll_ws_bytes() { return (size_t)NMAXBLK * NK * sizeof(double) + 256; }

static int nll_check(const char* who, int planes, int H, int W, unsigned mode, const float* input, const float* target,
                     const float* var_or_mask, int var_planes, float floor_, float eps) {
  if (planes < 1 || H < 1 || W < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (planes, H and W must be at least 1)", who);
  if (mode & ~(EOGS_NLL_MASK | EOGS_NLL_FULL | EOGS_NLL_SUM)) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown mode bits", who);
  if ((mode & EOGS_NLL_MASK) ? var_planes != 1 : (var_planes != 1 && var_planes != planes))
    return fail(EOGS_ERR_INVALID_ARG, "%s: var_planes is 1 for a mask, 1 or `planes` for a variance", who);
  if (!(floor_ >= 0.f) || !(eps > 0.f) || !(floor_ < INFINITY) || !(eps < INFINITY))
    return fail(EOGS_ERR_INVALID_ARG, "%s: floor must be finite and not negative, eps finite and positive", who);
  if (!input || !target || !var_or_mask) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  return EOGS_OK;
}

extern "C" {

int eogs_nll_bytes(int planes, int H, int W, size_t* bytes) {
  clear_error();
  if (planes < 1 || H < 1 || W < 1 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "nll_bytes: bad argument");
  *bytes = nll_ws_bytes();
  return EOGS_OK;
}

int eogs_nll_forward(int planes, int H, int W, unsigned mode, const float* input, const float* target,
                     const float* var_or_mask, int var_planes, float floor_, float eps, const float* weight, float* out,
                     void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const int rc = nll_check("nll_forward", planes, H, W, mode, input, target, var_or_mask, var_planes, floor_, eps);
  if (rc != EOGS_OK) return rc;
  if (!out || !ws) return fail(EOGS_ERR_INVALID_ARG, "nll_forward: NULL argument");
  if (ws_bytes < nll_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "nll_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(ws_base(ws));
  const int64_t HW = (int64_t)H * W;
  const bool vec = HW % UNIT == 0 && aligned16(input) && aligned16(target) && aligned16(var_or_mask);
  const int nb = capped_blocks((HW + UNIT - 1) / UNIT, NT, NMAXBLK);
  hipLaunchKernelGGL(nll_fwd_kernel, dim3(nb), dim3(NT), 0, s, planes, HW, (mode & EOGS_NLL_MASK) != 0u, var_planes, vec, input,
                     target, var_or_mask, floor_, eps, partial);
  hipLaunchKernelGGL(nll_final_kernel, dim3(1), dim3(NT), 0, s, (const double*)partial, nb, (double)planes * (double)HW,
                     (mode & EOGS_NLL_FULL) != 0u, (mode & EOGS_NLL_SUM) != 0u, weight, out);
  LAUNCH_TRY(s, false, "nll_fwd");
  return EOGS_OK;
}

int eogs_nll_backward(int planes, int H, int W, unsigned mode, const float* input, const float* target,
                      const float* var_or_mask, int var_planes, float floor_, float eps, const float* weight,
                      const float* g_loss, const float* g_total, float* g_input, float* g_var_or_mask, void* stream) {
  clear_error();
  const int rc = nll_check("nll_backward", planes, H, W, mode, input, target, var_or_mask, var_planes, floor_, eps);
  if (rc != EOGS_OK) return rc;
  if (!g_input && !g_var_or_mask) return fail(EOGS_ERR_INVALID_ARG, "nll_backward: no gradient asked for (both outputs NULL)");
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const bool vec = HW % UNIT == 0 && aligned16(input) && aligned16(target) && aligned16(var_or_mask) && aligned16(g_input) &&
                   aligned16(g_var_or_mask);
  const int nb = capped_blocks((HW + UNIT - 1) / UNIT, NT, 1 << 20);  // (the loop strides)
  hipLaunchKernelGGL(nll_bwd_kernel, dim3(nb), dim3(NT), 0, s, planes, HW, (mode & EOGS_NLL_MASK) != 0u, var_planes, vec,
                     (mode & EOGS_NLL_SUM) != 0u, input, target, var_or_mask, floor_, eps, weight, g_loss, g_total, g_input,
                     g_var_or_mask);
  LAUNCH_TRY(s, false, "nll_bwd");
  return EOGS_OK;
}

}  // extern "C"
