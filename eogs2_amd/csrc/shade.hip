// shade.hip — the per-pixel image chain between the raw render and the scalar losses (include/eogs_shade.h, SURVEY.md
// §8 row f2): camera render pipeline (colour correction + shadow), masked resample losses, translucent-shadow regulariser.
// Reference semantics: scene/cameras/affine_cameras.py:33-40,303-348; loss/shadow.py:7-17,37-51; loss/main_loss.py:83-96,
// 151-164 (all under src/gaussiansplatting/).
//
// All of it is elementwise work over H x W planes plus a handful of sums: HBM-bound by construction. One lane per pixel in
// a grid-stride loop (dword-coalesced planar loads), nothing is saved between forward and backward (the few values
// backward needs are recomputed from the inputs), and every sum is reduced per workgroup and then by one small kernel in
// a fixed order — no atomics, bitwise reproducible.
#include "api_util.h"
#include "reduce.h"
#include "eogs_randomcam.h"

namespace {

constexpr int ST = 256;        // threads per workgroup
constexpr int SMAXBLK = 1024;  // workgroups per launch (4 per CU); partial sums live in the caller's workspace
constexpr int SK = 16;         // floats per workgroup partial (15 used by shade_bwd)
constexpr int MK = 4;          // ... of the masked losses (3 used): what eogs_cmloss_bytes covers

// sums the per-workgroup partials [nblk][pitch] column by column: out[k] = sum_b partial[b][k], k < K
template <int MODE>  // 0: plain sums (shade_bwd); 1: mloss {S_alt/N, S_rgb/N, N}; 2: tshadow -S/n
__global__ __launch_bounds__(ST) void shade_reduce_kernel(const float* __restrict__ partial, int nblk, int pitch, int K, float scale,
                                                          float* __restrict__ out) {
  __shared__ float s_red[4];
  float tot[SK];
  for (int k = 0; k < K; k++) tot[k] = column_sum<ST>(partial + k, nblk, pitch, s_red);
  if (threadIdx.x != 0) return;
  if (MODE == 0) {
    for (int k = 0; k < K; k++) out[k] = tot[k];
  } else if (MODE == 1) {
    const float n = tot[2];
    out[0] = n > 0.f ? tot[0] / n : 0.f;
    out[1] = n > 0.f ? tot[1] / n : 0.f;
    out[2] = n;
  } else {
    out[0] = -tot[0] * scale;
  }
}

// ---- camera render pipeline ----------------------------------------------------------------------------------------
struct ShadeParams {
  float M[12];
  float ins[3];
};

// Translucentshadows_L's `shadowmap.clip(0.05, 0.95)` (loss/shadow.py:15), NaN kept
__device__ inline float tshadow_clip(float x) { return x < 0.05f ? 0.05f : (x > 0.95f ? 0.95f : x); }

__global__ __launch_bounds__(ST) void shade_fwd_kernel(int64_t n, const float* __restrict__ raw, const float* __restrict__ alt_diff,
                                                       const float* __restrict__ Mp, const float* __restrict__ insp,
                                                       float* __restrict__ cc, float* __restrict__ shaded,
                                                       float* __restrict__ shadow) {
  float M[12], ins[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 12; i++) M[i] = Mp[i];
  if (alt_diff) {
#pragma unroll
    for (int i = 0; i < 3; i++) ins[i] = insp[i];
  }
  for (int64_t p = (int64_t)blockIdx.x * ST + threadIdx.x; p < n; p += (int64_t)gridDim.x * ST) {
    const float r0 = raw[p], r1 = raw[n + p], r2 = raw[2 * n + p];
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = M[4 * k] * r0 + M[4 * k + 1] * r1 + M[4 * k + 2] * r2 + M[4 * k + 3];
    if (cc) {
#pragma unroll
      for (int k = 0; k < 3; k++) cc[k * n + p] = c[k];
    }
    if (alt_diff) {
      const float s = expf(0.4f * shadow_clip(alt_diff[p]));
      shadow[p] = s;
#pragma unroll
      for (int k = 0; k < 3; k++) shaded[k * n + p] = s * c[k] + ((1.f - s) * ins[k]) * c[k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) shaded[k * n + p] = c[k];
    }
  }
}

// shaded_c = cc_c f_c, f_c = s + (1 - s) ins_c:
//   d/dcc_c = f_c g_c (+ g_cc_c);  d/ds = sum_c g_c cc_c (1 - ins_c) (+ g_shadow);  d/dins_c = sum_p g_c (1 - s) cc_c
//   d/dalt_diff = d/ds * 0.4 s [alt_diff <= 0]   (torch.clamp(max=0) passes the gradient at equality and gives 0 at a NaN,
//   where s and everything formed from it are NaN)
//   d/draw_k = sum_c M[c][k] d/dcc_c;  d/dM[c][k] = sum_p d/dcc_c raw_k;  d/dM[c][3] = sum_p d/dcc_c
__global__ __launch_bounds__(ST) void shade_bwd_kernel(int64_t n, const float* __restrict__ raw, const float* __restrict__ alt_diff,
                                                       const float* __restrict__ Mp, const float* __restrict__ insp,
                                                       const float* __restrict__ g_shaded, const float* __restrict__ g_cc,
                                                       const float* __restrict__ g_shadow, float* __restrict__ g_raw,
                                                       float* __restrict__ g_alt, float* __restrict__ partial) {
  float M[12], ins[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 12; i++) M[i] = Mp[i];
  if (alt_diff) {
#pragma unroll
    for (int i = 0; i < 3; i++) ins[i] = insp[i];
  }
  float acc[15];
#pragma unroll
  for (int i = 0; i < 15; i++) acc[i] = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * ST + threadIdx.x; p < n; p += (int64_t)gridDim.x * ST) {
    const float r[3] = {raw[p], raw[n + p], raw[2 * n + p]};
    float c[3], g[3], gcc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      c[k] = M[4 * k] * r[0] + M[4 * k + 1] * r[1] + M[4 * k + 2] * r[2] + M[4 * k + 3];
      g[k] = g_shaded[k * n + p];
    }
    if (alt_diff) {
      const float d = alt_diff[p];
      const float s = expf(0.4f * shadow_clip(d));
      float gs = g_shadow ? g_shadow[p] : 0.f;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        gcc[k] = g[k] * (s + (1.f - s) * ins[k]);
        gs += g[k] * c[k] * (1.f - ins[k]);
        acc[12 + k] += g[k] * (1.f - s) * c[k];
      }
      g_alt[p] = d <= 0.f ? gs * 0.4f * s : 0.f;
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) gcc[k] = g[k];
    }
    if (g_cc) {
#pragma unroll
      for (int k = 0; k < 3; k++) gcc[k] += g_cc[k * n + p];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      g_raw[k * n + p] = M[k] * gcc[0] + M[4 + k] * gcc[1] + M[8 + k] * gcc[2];
      acc[4 * k] += gcc[k] * r[0];
      acc[4 * k + 1] += gcc[k] * r[1];
      acc[4 * k + 2] += gcc[k] * r[2];
      acc[4 * k + 3] += gcc[k];
    }
  }
  wg_partials<ST>(acc, partial + (size_t)blockIdx.x * SK);
}

// ---- masked resample losses ----------------------------------------------------------------------------------------
// One kernel pair for eogs_mloss_* (three planes, either mode) and randomcam's eogs_cmloss_* (1 .. 4 planes, mode RANDOM,
// either side's gradient optional): the same launch shape, per-lane expression trees and reduction, so three planes in
// mode RANDOM give the same bits through either entry.
__device__ inline bool mloss_mask(int mode, float d, float2 uv) {  // main_loss.py:83-85, 151-153
  const bool alt_ok = mode == EOGS_MLOSS_SUN ? d > -1e-2f : fabsf(d) < 0.30f;
  return alt_ok && fabsf(uv.x) < 1.f && fabsf(uv.y) < 1.f;
}

template <int C>
__global__ __launch_bounds__(ST) void mloss_fwd_kernel(int64_t n, int mode, const float* __restrict__ alt_diff,
                                                       const float* __restrict__ a, const float* __restrict__ b,
                                                       const float2* __restrict__ uv, float* __restrict__ partial) {
  float acc[3] = {0.f, 0.f, 0.f};  // S_alt, S_rgb, N
  for (int64_t p = (int64_t)blockIdx.x * ST + threadIdx.x; p < n; p += (int64_t)gridDim.x * ST) {
    const float d = alt_diff[p];
    if (mloss_mask(mode, d, uv[p])) {
      acc[0] += fabsf(d);
      float t = fabsf(a[p] - b[p]);
#pragma unroll
      for (int k = 1; k < C; k++) t += fabsf(a[k * n + p] - b[k * n + p]);
      acc[1] += t;
      acc[2] += 1.f;  // at most 2^24 / gridDim.x per lane: exact
    }
  }
  wg_partials<ST>(acc, partial + (size_t)blockIdx.x * MK);
}

// g_a and g_b may each be NULL (uniform branches); eogs_mloss_backward refuses a NULL g_a at its entry
template <int C>
__global__ __launch_bounds__(ST) void mloss_bwd_kernel(int64_t n, int mode, const float* __restrict__ alt_diff,
                                                       const float* __restrict__ a, const float* __restrict__ b,
                                                       const float2* __restrict__ uv, const float* __restrict__ out,
                                                       const float* __restrict__ upstream, float* __restrict__ g_alt,
                                                       float* __restrict__ g_a, float* __restrict__ g_b) {
  const float cnt = out[2];
  if (!(cnt > 0.f)) {  // an empty mask: the losses are constants with no path to the inputs, +0 everywhere
    for (int64_t p = (int64_t)blockIdx.x * ST + threadIdx.x; p < n; p += (int64_t)gridDim.x * ST) {
      g_alt[p] = 0.f;
#pragma unroll
      for (int k = 0; k < C; k++) {
        if (g_a) g_a[k * n + p] = 0.f;
        if (g_b) g_b[k * n + p] = 0.f;
      }
    }
    return;
  }
  const float w_alt = upstream[0] / cnt, w_rgb = upstream[1] / cnt;
  for (int64_t p = (int64_t)blockIdx.x * ST + threadIdx.x; p < n; p += (int64_t)gridDim.x * ST) {
    const float d = alt_diff[p];
    // the reference's (grad * mask) * sign(x): outside the mask a zero with the sign of w sign(x) (NaN under a non-finite w)
    const float mf = mloss_mask(mode, d, uv[p]) ? 1.f : 0.f;
    g_alt[p] = (w_alt * mf) * sgn(d);
    if (!g_a && !g_b) continue;
    const float wr = w_rgb * mf;
#pragma unroll
    for (int k = 0; k < C; k++) {
      const float g = wr * sgn(a[k * n + p] - b[k * n + p]);
      if (g_a) g_a[k * n + p] = g;
      if (g_b) g_b[k * n + p] = -g;
    }
  }
}

// both entries' launches; `partial` holds SMAXBLK rows of MK floats
void mloss_launch_fwd(int C, int64_t n, int mode, const float* alt_diff, const float* a, const float* b, const float* uv, float* out,
                      float* partial, hipStream_t s) {
  const int nb = capped_blocks(n, ST, SMAXBLK);
  const float2* uv2 = reinterpret_cast<const float2*>(uv);
  switch (C) {
    case 1: hipLaunchKernelGGL(mloss_fwd_kernel<1>, dim3(nb), dim3(ST), 0, s, n, mode, alt_diff, a, b, uv2, partial); break;
    case 2: hipLaunchKernelGGL(mloss_fwd_kernel<2>, dim3(nb), dim3(ST), 0, s, n, mode, alt_diff, a, b, uv2, partial); break;
    case 3: hipLaunchKernelGGL(mloss_fwd_kernel<3>, dim3(nb), dim3(ST), 0, s, n, mode, alt_diff, a, b, uv2, partial); break;
    default: hipLaunchKernelGGL(mloss_fwd_kernel<4>, dim3(nb), dim3(ST), 0, s, n, mode, alt_diff, a, b, uv2, partial); break;
  }
  hipLaunchKernelGGL(shade_reduce_kernel<1>, dim3(1), dim3(ST), 0, s, partial, nb, MK, 3, 1.f, out);
}

void mloss_launch_bwd(int C, int64_t n, int mode, const float* alt_diff, const float* a, const float* b, const float* uv,
                      const float* out, const float* upstream, float* g_alt, float* g_a, float* g_b, hipStream_t s) {
  const int nb = capped_blocks(n, ST, SMAXBLK);
  const float2* uv2 = reinterpret_cast<const float2*>(uv);
  switch (C) {
    case 1: hipLaunchKernelGGL(mloss_bwd_kernel<1>, dim3(nb), dim3(ST), 0, s, n, mode, alt_diff, a, b, uv2, out, upstream, g_alt, g_a, g_b); break;
    case 2: hipLaunchKernelGGL(mloss_bwd_kernel<2>, dim3(nb), dim3(ST), 0, s, n, mode, alt_diff, a, b, uv2, out, upstream, g_alt, g_a, g_b); break;
    case 3: hipLaunchKernelGGL(mloss_bwd_kernel<3>, dim3(nb), dim3(ST), 0, s, n, mode, alt_diff, a, b, uv2, out, upstream, g_alt, g_a, g_b); break;
    default: hipLaunchKernelGGL(mloss_bwd_kernel<4>, dim3(nb), dim3(ST), 0, s, n, mode, alt_diff, a, b, uv2, out, upstream, g_alt, g_a, g_b); break;
  }
}

// ---- translucent-shadow regulariser ------------------------------------------------------------------------------
__global__ __launch_bounds__(ST) void tshadow_fwd_kernel(int64_t n, const float* __restrict__ a, float* __restrict__ partial) {
  float s[1] = {0.f};
  for (int64_t p = (int64_t)blockIdx.x * ST + threadIdx.x; p < n; p += (int64_t)gridDim.x * ST) {
    const float x = a[p];
    const float b = tshadow_clip(x);
    s[0] += x * log2f(b) + (1.f - x) * log2f(1.f - b);
  }
  wg_partials<ST>(s, partial + (size_t)blockIdx.x * SK);
}

__global__ __launch_bounds__(ST) void tshadow_bwd_kernel(int64_t n, const float* __restrict__ a, const float* __restrict__ upstream,
                                                         float* __restrict__ g_a) {
  const float w = -upstream[0] / (float)n;
  const float inv_ln2 = 1.4426950408889634f;
  for (int64_t p = (int64_t)blockIdx.x * ST + threadIdx.x; p < n; p += (int64_t)gridDim.x * ST) {
    const float x = a[p];
    const float b = tshadow_clip(x);
    float d = log2f(b) - log2f(1.f - b);
    if (x >= 0.05f && x <= 0.95f) d += (x / b - (1.f - x) / (1.f - b)) * inv_ln2;
    g_a[p] = w * d;
  }
}

}  // namespace

static size_t shade_ws_bytes() { return (size_t)SMAXBLK * SK * sizeof(float) + 256; }
static size_t cmloss_ws_bytes() { return (size_t)SMAXBLK * MK * sizeof(float) + 256; }

extern "C" {

int eogs_shade_bytes(int H, int W, size_t* bytes) {
  clear_error();
  if (H <= 0 || W <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "shade_bytes: bad argument");
  *bytes = shade_ws_bytes();
  return EOGS_OK;
}

int eogs_shade_forward(int H, int W, const float* raw, const float* alt_diff, const float* M, const float* inshadow,
                       float* cc, float* shaded, float* shadow, void* stream) {
  clear_error();
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "shade_forward: bad sizes");
  if (!raw || !M || !shaded) return fail(EOGS_ERR_INVALID_ARG, "shade_forward: NULL argument");
  if ((alt_diff != nullptr) != (shadow != nullptr) || (alt_diff && !inshadow))
    return fail(EOGS_ERR_INVALID_ARG, "shade_forward: alt_diff, inshadow and shadow go together");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  {
    ProfScope ps(PS_SHADE_FWD, s);
    hipLaunchKernelGGL(shade_fwd_kernel, dim3(capped_blocks(n, ST, SMAXBLK)), dim3(ST), 0, s, n, raw, alt_diff, M, inshadow, cc, shaded, shadow);
  }
  LAUNCH_TRY(s, false, "shade_fwd");
  return EOGS_OK;
}

int eogs_shade_backward(int H, int W, const float* raw, const float* alt_diff, const float* M, const float* inshadow,
                        const float* g_shaded, const float* g_cc, const float* g_shadow, float* g_raw,
                        float* g_alt_diff, float* g_params, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "shade_backward: bad sizes");
  if (!raw || !M || !g_shaded || !g_raw || !g_params || !ws) return fail(EOGS_ERR_INVALID_ARG, "shade_backward: NULL argument");
  if ((alt_diff != nullptr) != (g_alt_diff != nullptr) || (alt_diff && !inshadow) || (!alt_diff && g_shadow))
    return fail(EOGS_ERR_INVALID_ARG, "shade_backward: alt_diff, inshadow and g_alt_diff go together");
  if (ws_bytes < shade_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "shade_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  const int nb = capped_blocks(n, ST, SMAXBLK);
  float* partial = reinterpret_cast<float*>(ws_base(ws));
  {
    ProfScope ps(PS_SHADE_BWD, s);
    hipLaunchKernelGGL(shade_bwd_kernel, dim3(nb), dim3(ST), 0, s, n, raw, alt_diff, M, inshadow, g_shaded, g_cc, g_shadow, g_raw,
                       g_alt_diff, partial);
    hipLaunchKernelGGL(shade_reduce_kernel<0>, dim3(1), dim3(ST), 0, s, partial, nb, SK, 15, 1.f, g_params);
  }
  LAUNCH_TRY(s, false, "shade_bwd");
  return EOGS_OK;
}

int eogs_mloss_forward(int H, int W, int mode, const float* alt_diff, const float* rgb_a, const float* rgb_b,
                       const float* uv, float* out, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (H <= 0 || W <= 0 || (mode != EOGS_MLOSS_SUN && mode != EOGS_MLOSS_RANDOM))
    return fail(EOGS_ERR_INVALID_ARG, "mloss_forward: bad sizes or mode");
  if (!alt_diff || !rgb_a || !rgb_b || !uv || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "mloss_forward: NULL argument");
  if (ws_bytes < shade_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "mloss_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(PS_MLOSS_FWD, s);
    mloss_launch_fwd(3, (int64_t)H * W, mode, alt_diff, rgb_a, rgb_b, uv, out, reinterpret_cast<float*>(ws_base(ws)), s);
  }
  LAUNCH_TRY(s, false, "mloss_fwd");
  return EOGS_OK;
}

int eogs_mloss_backward(int H, int W, int mode, const float* alt_diff, const float* rgb_a, const float* rgb_b,
                        const float* uv, const float* out, const float* upstream, float* g_alt_diff, float* g_rgb_a,
                        float* g_rgb_b, void* stream) {
  clear_error();
  if (H <= 0 || W <= 0 || (mode != EOGS_MLOSS_SUN && mode != EOGS_MLOSS_RANDOM))
    return fail(EOGS_ERR_INVALID_ARG, "mloss_backward: bad sizes or mode");
  if (!alt_diff || !rgb_a || !rgb_b || !uv || !out || !upstream || !g_alt_diff || !g_rgb_a)
    return fail(EOGS_ERR_INVALID_ARG, "mloss_backward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(PS_MLOSS_BWD, s);
    mloss_launch_bwd(3, (int64_t)H * W, mode, alt_diff, rgb_a, rgb_b, uv, out, upstream, g_alt_diff, g_rgb_a, g_rgb_b, s);
  }
  LAUNCH_TRY(s, false, "mloss_bwd");
  return EOGS_OK;
}

// randomcam's comparison (include/eogs_randomcam.h): the same kernels in mode RANDOM for 1 .. 4 planes
int eogs_cmloss_bytes(int H, int W, size_t* bytes) {
  clear_error();
  if (H <= 0 || W <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "cmloss_bytes: bad argument");
  *bytes = cmloss_ws_bytes();
  return EOGS_OK;
}

int eogs_cmloss_forward(int H, int W, int C, const float* alt_diff, const float* rgb_a, const float* rgb_b, const float* uv,
                        float* out, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "cmloss_forward: bad sizes");
  if (C < 1 || C > EOGS_CMLOSS_MAX_CHANNELS) return fail(EOGS_ERR_INVALID_ARG, "cmloss_forward: 1 to 4 channels");
  if (!alt_diff || !rgb_a || !rgb_b || !uv || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "cmloss_forward: NULL argument");
  if (ws_bytes < cmloss_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "cmloss_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(PS_MLOSS_FWD, s);
    mloss_launch_fwd(C, (int64_t)H * W, EOGS_MLOSS_RANDOM, alt_diff, rgb_a, rgb_b, uv, out, reinterpret_cast<float*>(ws_base(ws)), s);
  }
  LAUNCH_TRY(s, false, "cmloss_fwd");
  return EOGS_OK;
}

int eogs_cmloss_backward(int H, int W, int C, const float* alt_diff, const float* rgb_a, const float* rgb_b, const float* uv,
                         const float* out, const float* upstream, float* g_alt_diff, float* g_rgb_a, float* g_rgb_b,
                         void* stream) {
  clear_error();
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "cmloss_backward: bad sizes");
  if (C < 1 || C > EOGS_CMLOSS_MAX_CHANNELS) return fail(EOGS_ERR_INVALID_ARG, "cmloss_backward: 1 to 4 channels");
  if (!alt_diff || !rgb_a || !rgb_b || !uv || !out || !upstream || !g_alt_diff)
    return fail(EOGS_ERR_INVALID_ARG, "cmloss_backward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(PS_MLOSS_BWD, s);
    mloss_launch_bwd(C, (int64_t)H * W, EOGS_MLOSS_RANDOM, alt_diff, rgb_a, rgb_b, uv, out, upstream, g_alt_diff, g_rgb_a, g_rgb_b, s);
  }
  LAUNCH_TRY(s, false, "cmloss_bwd");
  return EOGS_OK;
}

int eogs_tshadow_forward(int64_t n, const float* a, float* out, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (n <= 0) return fail(EOGS_ERR_INVALID_ARG, "tshadow_forward: bad size");
  if (!a || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "tshadow_forward: NULL argument");
  if (ws_bytes < shade_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "tshadow_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int nb = capped_blocks(n, ST, SMAXBLK);
  float* partial = reinterpret_cast<float*>(ws_base(ws));
  hipLaunchKernelGGL(tshadow_fwd_kernel, dim3(nb), dim3(ST), 0, s, n, a, partial);
  hipLaunchKernelGGL(shade_reduce_kernel<2>, dim3(1), dim3(ST), 0, s, partial, nb, SK, 1, 1.f / (float)n, out);
  LAUNCH_TRY(s, false, "tshadow_fwd");
  return EOGS_OK;
}

int eogs_tshadow_backward(int64_t n, const float* a, const float* upstream, float* g_a, void* stream) {
  clear_error();
  if (n <= 0) return fail(EOGS_ERR_INVALID_ARG, "tshadow_backward: bad size");
  if (!a || !upstream || !g_a) return fail(EOGS_ERR_INVALID_ARG, "tshadow_backward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tshadow_bwd_kernel, dim3(capped_blocks(n, ST, SMAXBLK)), dim3(ST), 0, s, n, a, upstream, g_a);
  LAUNCH_TRY(s, false, "tshadow_bwd");
  return EOGS_OK;
}

}  // extern "C"
