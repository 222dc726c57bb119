// randomcam.hip — what RandomcamRendering_Loss (loss/main_loss.py:56-221) needs beyond the resample, shade / pan and
// rasterizer kernels (include/eogs_randomcam.h): the composed matrices of the shadow-mapped virtual view
// (gaussian_renderer/renderer_cc_shadow.py:85-95). Its masked comparison, eogs_cmloss_*, is shade.hip's masked-loss
// kernel pair and lives there.
//
// compose is one wave and a few hundred bytes: latency-bound by construction; its point is that nothing on the host waits
// for a matrix the draw kernel has just written.
#include "api_util.h"
#include "randomcam_compose.h"
#include "eogs_randomcam.h"

namespace {

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

}  // extern "C"
