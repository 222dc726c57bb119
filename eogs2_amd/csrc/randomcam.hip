// randomcam.hip — what RandomcamRendering_Loss (loss/main_loss.py:56-221) needs beyond the resample, shade / pan and
// rasterizer kernels (include/eogs_randomcam.h): the composed matrices of the shadow-mapped virtual view
// (gaussian_renderer/renderer_cc_shadow.py:85-95), and the masked comparison of shade.hip's mloss kernels in mode RANDOM for
// 1 .. 4 planes with either side's gradient optional.
//
// compose is one wave and a few hundred bytes: latency-bound by construction; its point is that nothing on the host waits
// for a matrix the draw kernel has just written. The comparison is elementwise work over H x W planes plus three sums:
// HBM-bound, one lane per pixel in a grid-stride loop, sums per workgroup and then by one small kernel in a fixed order.
// The launch shape, the per-lane expression trees and the order of the reduction are those of shade.hip's mloss kernels,
// so that three planes give their bits.
#include "api_util.h"
#include "reduce.h"
#include "randomcam_compose.h"
#include "eogs_randomcam.h"

namespace {

constexpr int CT = 256;        // threads per workgroup (shade.hip: ST)
constexpr int CMAXBLK = 1024;  // workgroups per launch (shade.hip: SMAXBLK)
constexpr int CK = 4;          // floats per workgroup partial (3 used)

inline int cmloss_blocks(int64_t n) {
  const int64_t b = (n + CT - 1) / CT;
  return (int)(b < 1 ? 1 : (b > CMAXBLK ? CMAXBLK : b));
}

__global__ __launch_bounds__(64) void randomcam_compose_kernel(const float* __restrict__ cam2virt, const float* __restrict__ camera_to_sun,
                                                               float* __restrict__ out) {
  const int t = (int)threadIdx.x;
  if (blockIdx.x != 0) return;
  float c[9], s[9], o[18];
#pragma unroll
  for (int i = 0; i < 9; i++) {  // every lane reads both matrices (two cache lines) and forms all 18: no exchange
    c[i] = cam2virt[i];
    s[i] = camera_to_sun[i];
  }
  randomcam_compose(c, s, o);
  float mine = 0.f;
#pragma unroll
  for (int i = 0; i < 18; i++) mine = (t == i) ? o[i] : mine;
  if (t < 18) out[t] = mine;
}

__device__ inline bool cmloss_mask(float d, float2 uv) {  // main_loss.py:151-153
  return fabsf(d) < 0.30f && fabsf(uv.x) < 1.f && fabsf(uv.y) < 1.f;
}

template <int C>
__global__ __launch_bounds__(CT) void cmloss_fwd_kernel(int64_t n, const float* __restrict__ alt_diff, const float* __restrict__ a,
                                                        const float* __restrict__ b, const float2* __restrict__ uv,
                                                        float* __restrict__ partial) {
  __shared__ float s_red[4];
  float s_alt = 0.f, s_rgb = 0.f, cnt = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * CT + threadIdx.x; p < n; p += (int64_t)gridDim.x * CT) {
    const float d = alt_diff[p];
    if (cmloss_mask(d, uv[p])) {
      s_alt += fabsf(d);
      float t = fabsf(a[p] - b[p]);
#pragma unroll
      for (int k = 1; k < C; k++) t += fabsf(a[k * n + p] - b[k * n + p]);
      s_rgb += t;
      cnt += 1.f;  // at most 2^24 / gridDim.x per lane: exact
    }
  }
  const float t0 = wg_sum(s_alt, s_red), t1 = wg_sum(s_rgb, s_red), t2 = wg_sum(cnt, s_red);
  if (threadIdx.x == 0) {
    partial[(size_t)blockIdx.x * CK] = t0;
    partial[(size_t)blockIdx.x * CK + 1] = t1;
    partial[(size_t)blockIdx.x * CK + 2] = t2;
  }
}

// out = {S_alt / N, S_rgb / N, N} from the per-workgroup partials, column by column in a fixed order
__global__ __launch_bounds__(CT) void cmloss_reduce_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ out) {
  __shared__ float s_red[4];
  float tot[3];
  for (int k = 0; k < 3; k++) {
    float a = 0.f;
    for (int i = threadIdx.x; i < nblk; i += CT) a += partial[(size_t)i * CK + k];
    tot[k] = wg_sum(a, s_red);
  }
  if (threadIdx.x != 0) return;
  const float n = tot[2];
  out[0] = n > 0.f ? tot[0] / n : 0.f;
  out[1] = n > 0.f ? tot[1] / n : 0.f;
  out[2] = n;
}

template <int C>
__global__ __launch_bounds__(CT) void cmloss_bwd_kernel(int64_t n, const float* __restrict__ alt_diff, const float* __restrict__ a,
                                                        const float* __restrict__ b, const float2* __restrict__ uv,
                                                        const float* __restrict__ out, const float* __restrict__ upstream,
                                                        float* __restrict__ g_alt, float* __restrict__ g_a, float* __restrict__ g_b) {
  const float cnt = out[2];
  if (!(cnt > 0.f)) {  // an empty mask: the losses are constants with no path to the inputs, +0 everywhere
    for (int64_t p = (int64_t)blockIdx.x * CT + threadIdx.x; p < n; p += (int64_t)gridDim.x * CT) {
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
  for (int64_t p = (int64_t)blockIdx.x * CT + threadIdx.x; p < n; p += (int64_t)gridDim.x * CT) {
    const float d = alt_diff[p];
    // the reference's (grad * mask) * sign(x): outside the mask a zero with the sign of w sign(x) (NaN under a non-finite w)
    const float mf = cmloss_mask(d, uv[p]) ? 1.f : 0.f;
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

size_t cmloss_ws_bytes() { return (size_t)CMAXBLK * CK * sizeof(float) + 256; }
bool misaligned4(const void* p) { return ((uintptr_t)p & 3u) != 0; }
bool overlaps(const float* a, size_t na, const float* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

}  // namespace

extern "C" {

int eogs_randomcam_compose(const float* cam2virt, const float* camera_to_sun, float* out, void* stream) {
  clear_error();
  if (!cam2virt) return fail(EOGS_ERR_INVALID_ARG, "randomcam_compose: NULL cam2virt");
  if (!camera_to_sun) return fail(EOGS_ERR_INVALID_ARG, "randomcam_compose: NULL camera_to_sun");
  if (!out) return fail(EOGS_ERR_INVALID_ARG, "randomcam_compose: NULL out");
  if (misaligned4(cam2virt) || misaligned4(camera_to_sun) || misaligned4(out))
    return fail(EOGS_ERR_INVALID_ARG, "randomcam_compose: a pointer is not 4-byte aligned");
  if (overlaps(out, 18, cam2virt, 9) || overlaps(out, 18, camera_to_sun, 9))
    return fail(EOGS_ERR_INVALID_ARG, "randomcam_compose: out overlaps an input");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(randomcam_compose_kernel, dim3(1), dim3(64), 0, s, cam2virt, camera_to_sun, out);
  LAUNCH_TRY(s, false, "randomcam_compose");
  return EOGS_OK;
}

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
  const int64_t n = (int64_t)H * W;
  const int nb = cmloss_blocks(n);
  float* partial = reinterpret_cast<float*>(ws_base(ws));
  const float2* uv2 = reinterpret_cast<const float2*>(uv);
  {
    ProfScope ps(PS_MLOSS_FWD, s);
    switch (C) {
      case 1: hipLaunchKernelGGL(cmloss_fwd_kernel<1>, dim3(nb), dim3(CT), 0, s, n, alt_diff, rgb_a, rgb_b, uv2, partial); break;
      case 2: hipLaunchKernelGGL(cmloss_fwd_kernel<2>, dim3(nb), dim3(CT), 0, s, n, alt_diff, rgb_a, rgb_b, uv2, partial); break;
      case 3: hipLaunchKernelGGL(cmloss_fwd_kernel<3>, dim3(nb), dim3(CT), 0, s, n, alt_diff, rgb_a, rgb_b, uv2, partial); break;
      default: hipLaunchKernelGGL(cmloss_fwd_kernel<4>, dim3(nb), dim3(CT), 0, s, n, alt_diff, rgb_a, rgb_b, uv2, partial); break;
    }
    hipLaunchKernelGGL(cmloss_reduce_kernel, dim3(1), dim3(CT), 0, s, partial, nb, out);
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
  const int64_t n = (int64_t)H * W;
  const int nb = cmloss_blocks(n);
  const float2* uv2 = reinterpret_cast<const float2*>(uv);
  {
    ProfScope ps(PS_MLOSS_BWD, s);
    switch (C) {
      case 1: hipLaunchKernelGGL(cmloss_bwd_kernel<1>, dim3(nb), dim3(CT), 0, s, n, alt_diff, rgb_a, rgb_b, uv2, out, upstream, g_alt_diff, g_rgb_a, g_rgb_b); break;
      case 2: hipLaunchKernelGGL(cmloss_bwd_kernel<2>, dim3(nb), dim3(CT), 0, s, n, alt_diff, rgb_a, rgb_b, uv2, out, upstream, g_alt_diff, g_rgb_a, g_rgb_b); break;
      case 3: hipLaunchKernelGGL(cmloss_bwd_kernel<3>, dim3(nb), dim3(CT), 0, s, n, alt_diff, rgb_a, rgb_b, uv2, out, upstream, g_alt_diff, g_rgb_a, g_rgb_b); break;
      default: hipLaunchKernelGGL(cmloss_bwd_kernel<4>, dim3(nb), dim3(CT), 0, s, n, alt_diff, rgb_a, rgb_b, uv2, out, upstream, g_alt_diff, g_rgb_a, g_rgb_b); break;
    }
  }
  LAUNCH_TRY(s, false, "cmloss_bwd");
  return EOGS_OK;
}

}  // extern "C"
