// draw.hip — the per-iteration random draws (include/eogs_draw.h): the background's three uniforms and the virtual camera's
// shear from Philox4x32-10 keyed by the iteration's index on the device (draw_rng.h), and the sheared affine of
// sample_random_camera / get_nadir_camera (affine_cameras.py:372-430) as explicit fma. One wave: lane t does camera t; a
// lane reads all of its inputs before its first store. Latency-bound by construction, a few hundred bytes move.
#include "api_util.h"
#include "draw_rng.h"
#include "eogs_draw.h"

namespace {

struct DrawCameras {
  eogs_draw_camera cam[EOGS_DRAW_MAX_CAMERAS];
  int n;
};

__global__ __launch_bounds__(64) void draw_iteration_kernel(DrawCameras C, eogs_draw_stream S) {
  const int t = (int)threadIdx.x;
  if (blockIdx.x != 0 || t >= C.n || t >= EOGS_DRAW_MAX_CAMERAS) return;
  const eogs_draw_camera c = C.cam[t];
  const uint64_t iteration = (uint64_t)*S.counter;

  if (c.flags & EOGS_DRAW_BG) {
    const DrawBlock b = draw_block(S.seed, iteration, (uint32_t)t, DRAW_PURPOSE_BG);
    const float u0 = draw_uniform(b.w[0]), u1 = draw_uniform(b.w[1]), u2 = draw_uniform(b.w[2]);
    const bool first = (c.flags & EOGS_DRAW_BG_COPY_FIRST) != 0u;
    const bool floor_given = c.alt_floor != nullptr;
    const float alt = floor_given ? *c.alt_floor : 0.0f;
    c.bg[0] = u0;
    c.bg[1] = first ? u0 : u1;
    c.bg[2] = first ? u0 : u2;
    if (floor_given) c.bg[3] = alt;
    c.bg[4] = 0.0f;
  }

  if (c.flags & (EOGS_DRAW_CAMERA | EOGS_DRAW_NADIR)) {
    float a[16];
#pragma unroll
    for (int k = 0; k < 16; k++) a[k] = c.affine[k];  // A[i][j] = a[4 j + i], b[i] = a[12 + i]
    float d[2];
    if (c.flags & EOGS_DRAW_NADIR) {
      d[0] = -(a[8] / a[10]);  // q = A[:, 2] / A[2][2], myM[:2, 2] = -q[:2]
      d[1] = -(a[9] / a[10]);
    } else {
      const DrawBlock b = draw_block(S.seed, iteration, (uint32_t)t, DRAW_PURPOSE_SHEAR);
      float z[2];
      draw_normals(b.w[0], b.w[1], z);
      d[0] = z[0] * c.extent;
      d[1] = z[1] * c.extent;
    }
    if (c.virt_affine != nullptr) {
      const float c0 = c.center[0], c1 = c.center[1], c2 = c.center[2];
      const float s = fmaf(a[10], c2, fmaf(a[6], c1, a[2] * c0));  // A[2][:] . center
      float o[16];
#pragma unroll
      for (int j = 0; j < 3; j++) {
        o[4 * j + 0] = fmaf(d[0], a[4 * j + 2], a[4 * j + 0]);
        o[4 * j + 1] = fmaf(d[1], a[4 * j + 2], a[4 * j + 1]);
        o[4 * j + 2] = a[4 * j + 2];
        o[4 * j + 3] = 0.0f;
      }
      o[12] = fmaf(-d[0], s, a[12]);
      o[13] = fmaf(-d[1], s, a[13]);
      o[14] = a[14];
      o[15] = 1.0f;
#pragma unroll
      for (int k = 0; k < 16; k++) c.virt_affine[k] = o[k];
    }
    if (c.cam2virt != nullptr) {
      const float m02 = d[0] * c.cam2virt_scale, m12 = d[1] * c.cam2virt_scale;
      c.cam2virt[0] = 1.0f; c.cam2virt[1] = 0.0f; c.cam2virt[2] = m02;
      c.cam2virt[3] = 0.0f; c.cam2virt[4] = 1.0f; c.cam2virt[5] = m12;
      c.cam2virt[6] = 0.0f; c.cam2virt[7] = 0.0f; c.cam2virt[8] = 1.0f;
    }
    if (c.shear != nullptr) {
      c.shear[0] = d[0];
      c.shear[1] = d[1];
    }
  }
}

__global__ void draw_advance_kernel(int64_t* counter, const uint32_t* __restrict__ gate) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (gate != nullptr && gate[0] == 0u) return;
  *counter = (int64_t)((uint64_t)*counter + 1u);
}

bool misaligned(const void* p) { return ((uintptr_t)p & 3u) != 0; }
bool bad_scale(float x) { return !(x >= 0.0f) || x > 3.4028234663852886e38f; }  // negative, NaN or infinite

int check_camera(const eogs_draw_camera& c) {
  const uint32_t all = EOGS_DRAW_BG | EOGS_DRAW_BG_COPY_FIRST | EOGS_DRAW_CAMERA | EOGS_DRAW_NADIR;
  if (c.flags & ~all) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: unknown flags");
  if (!(c.flags & (EOGS_DRAW_BG | EOGS_DRAW_CAMERA | EOGS_DRAW_NADIR))) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: flags ask for nothing (BG, CAMERA or NADIR)");
  if ((c.flags & EOGS_DRAW_CAMERA) && (c.flags & EOGS_DRAW_NADIR)) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: contradictory flags: CAMERA and NADIR together");
  if ((c.flags & EOGS_DRAW_BG_COPY_FIRST) && !(c.flags & EOGS_DRAW_BG)) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: contradictory flags: BG_COPY_FIRST without BG");
  if (misaligned(c.affine) || misaligned(c.center) || misaligned(c.alt_floor) || misaligned(c.bg) || misaligned(c.virt_affine) ||
      misaligned(c.cam2virt) || misaligned(c.shear))
    return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: a pointer is not 4-byte aligned");
  if (bad_scale(c.extent)) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: extent must be finite and not negative");
  if (bad_scale(c.cam2virt_scale)) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: cam2virt_scale must be finite and not negative");
  if ((c.flags & EOGS_DRAW_BG) && !c.bg) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: BG without bg");
  if (c.flags & (EOGS_DRAW_CAMERA | EOGS_DRAW_NADIR)) {
    if (!c.affine) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: a camera flag without affine");
    if (!c.virt_affine && !c.cam2virt && !c.shear) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: a camera flag without any of virt_affine, cam2virt, shear");
    if (c.virt_affine && !c.center) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: virt_affine without center");
  }
  return EOGS_OK;
}

}  // namespace

extern "C" {

int eogs_draw_iteration(int n, const eogs_draw_camera* cams, const eogs_draw_stream* stream_desc, void* stream) {
  clear_error();
  if (n < 0 || n > EOGS_DRAW_MAX_CAMERAS) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: bad camera count (at most 8 cameras in one call)");
  if (!stream_desc) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: NULL stream_desc");
  if (!stream_desc->counter) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: NULL counter");
  if ((uintptr_t)stream_desc->counter & 7u) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: counter not 8-byte aligned");
  if (n > 0 && !cams) return fail(EOGS_ERR_INVALID_ARG, "draw_iteration: NULL cams");
  DrawCameras C;
  C.n = n;
  for (int i = 0; i < EOGS_DRAW_MAX_CAMERAS; i++) C.cam[i] = eogs_draw_camera{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0u};
  for (int i = 0; i < n; i++) {
    int rc = check_camera(cams[i]);
    if (rc) return rc;
    C.cam[i] = cams[i];
  }
  if (n == 0) return EOGS_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(draw_iteration_kernel, dim3(1), dim3(64), 0, s, C, *stream_desc);
  LAUNCH_TRY(s, false, "draw_iteration");
  return EOGS_OK;
}

int eogs_draw_advance(int64_t* counter, const uint32_t* gate, void* stream) {
  clear_error();
  if (!counter) return fail(EOGS_ERR_INVALID_ARG, "draw_advance: NULL counter");
  if ((uintptr_t)counter & 7u) return fail(EOGS_ERR_INVALID_ARG, "draw_advance: counter not 8-byte aligned");
  if ((uintptr_t)gate & 3u) return fail(EOGS_ERR_INVALID_ARG, "draw_advance: gate not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(draw_advance_kernel, dim3(1), dim3(64), 0, s, counter, gate);
  LAUNCH_TRY(s, false, "draw_advance");
  return EOGS_OK;
}

}  // extern "C"
