// resample.hip — fused virtual-camera resample: uv = cam2virt (u,v,alt), bilinear grid sample (align_corners=True,
// zeros padding) of the virtual render, out-of-view fill; forward and backward.
// Reference semantics: src/gaussiansplatting/gaussian_renderer/renderer_cc_shadow.py:32-50 on top of
// torch.nn.functional.grid_sample (ATen grid_sampler_2d: unnormalize ((x+1)/2)(size-1), floor corner, weights from
// the opposite corner, taps outside the image contribute zero and receive no gradient).
// One lane per output pixel; neighbouring lanes sample neighbouring taps, so the gathers coalesce in L2. HBM-bound.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "bucket_gather.h"
#include "api_util.h"

namespace {


struct Taps {
  int x0, y0;           // north-west corner
  float wx1, wy1;       // fractional parts: weight of the east / south neighbours
  bool in_x0, in_x1, in_y0, in_y1;
};

__device__ inline Taps make_taps(float u, float v, int Wv, int Hv) {
  Taps t;
  const float ix = (u + 1.f) * 0.5f * (float)(Wv - 1), iy = (v + 1.f) * 0.5f * (float)(Hv - 1);
  const float fx = floorf(ix), fy = floorf(iy);
  t.wx1 = ix - fx; t.wy1 = iy - fy;
  // clamp before the int conversion: far-away coordinates only need to end up out of bounds
  t.x0 = (int)fminf(fmaxf(fx, -2.f), (float)Wv + 1.f);
  t.y0 = (int)fminf(fmaxf(fy, -2.f), (float)Hv + 1.f);
  t.in_x0 = t.x0 >= 0 && t.x0 < Wv; t.in_x1 = t.x0 + 1 >= 0 && t.x0 + 1 < Wv;
  t.in_y0 = t.y0 >= 0 && t.y0 < Hv; t.in_y1 = t.y0 + 1 >= 0 && t.y0 + 1 < Hv;
  return t;
}

__global__ __launch_bounds__(BLK) void resample_fwd_kernel(int C, int Hv, int Wv, int HW, int n_out,
                                                           const float* __restrict__ vr, const float* __restrict__ uva,
                                                           const float* __restrict__ M, int fill_channel, float fill_value,
                                                           float* __restrict__ sample, float* __restrict__ uv) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= HW) return;
  const float a = uva[3 * (size_t)p], b = uva[3 * (size_t)p + 1], c = uva[3 * (size_t)p + 2];
  const float u = M[0] * a + M[1] * b + M[2] * c, v = M[3] * a + M[4] * b + M[5] * c;
  reinterpret_cast<float2*>(uv)[p] = make_float2(u, v);
  const Taps t = make_taps(u, v, Wv, Hv);
  const float wnw = (1.f - t.wx1) * (1.f - t.wy1), wne = t.wx1 * (1.f - t.wy1), wsw = (1.f - t.wx1) * t.wy1, wse = t.wx1 * t.wy1;
  const size_t plane = (size_t)Hv * Wv;
  const size_t o00 = (size_t)t.y0 * Wv + t.x0;
  const bool outside = fabsf(u) > 1.f || fabsf(v) > 1.f;
  // the taps of up to four channels are requested together (the reference resamples four; a runtime-bounded loop made every
  // channel wait for the previous one's four gathers)
  for (int c0 = 0; c0 < n_out; c0 += 4) {
    float v[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool on = c0 + k < n_out;
      const float* src = vr + (size_t)(on ? c0 + k : 0) * plane;
      v[k][0] = (on && t.in_y0 && t.in_x0) ? src[o00] : 0.f;
      v[k][1] = (on && t.in_y0 && t.in_x1) ? src[o00 + 1] : 0.f;
      v[k][2] = (on && t.in_y1 && t.in_x0) ? src[o00 + Wv] : 0.f;
      v[k][3] = (on && t.in_y1 && t.in_x1) ? src[o00 + Wv + 1] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int ch = c0 + k;
      if (ch >= n_out) break;
      float s = 0.f;
      if (t.in_y0 && t.in_x0) s += v[k][0] * wnw;
      if (t.in_y0 && t.in_x1) s += v[k][1] * wne;
      if (t.in_y1 && t.in_x0) s += v[k][2] * wsw;
      if (t.in_y1 && t.in_x1) s += v[k][3] * wse;
      if (ch == fill_channel && outside) s = fill_value;
      sample[(size_t)ch * HW + p] = s;
    }
  }
}

// ---- backward ----
// dL/duva needs only per-pixel data. dL/dvirtual_render is a scatter of four taps per output pixel; global fp32 atomics
// sustain only ~26 G/s here (0.7 ms for a 1024^2 grid), so the scatter is turned into a gather by VIRTUAL tile:
//   pixel kernel : per 16x16 output tile, dL/duva and the bounding box of the cells its pixels touch;
//   tile kernel  : one workgroup per virtual tile collects the taps of every output tile whose box meets it (recomputing the
//                  few coordinates involved), then writes its tile with plain stores. Two forms: resample_bwd_tile_kernel
//                  (round 2: ds_add_f32 into an LDS image of the tile) and resample_bwd_gather_kernel (round 4, the default:
//                  pixels bucketed by tap cell with integer atomics, cells gather their buckets; profiles/r04_resample_bwd.txt).
// No global atomics, no memset; every virtual pixel is written exactly once.

__device__ inline void lds_add(float* p, float v) {  // ds_add_f32, result unused
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
constexpr int VTX = 64, VTY = 32;  // virtual tile (32 KB of LDS for four channels)

// where an output pixel of the resample samples the virtual render (bucket_gather.h)
struct ResampleSrc {
  const float* __restrict__ uva;
  const float* __restrict__ M;
  struct Raw { float a, b, c; };
  __device__ Raw load(size_t pix, int, int) const { return Raw{uva[3 * pix], uva[3 * pix + 1], uva[3 * pix + 2]}; }
  __device__ void taps(const Raw& r, int Wv, int Hv, int& x0, int& y0, float& wx1, float& wy1, bool& outside) const {
    const float u = M[0] * r.a + M[1] * r.b + M[2] * r.c, v = M[3] * r.a + M[4] * r.b + M[5] * r.c;
    const Taps tp = make_taps(u, v, Wv, Hv);
    x0 = tp.x0; y0 = tp.y0; wx1 = tp.wx1; wy1 = tp.wy1;
    outside = fabsf(u) > 1.f || fabsf(v) > 1.f;
  }
  __device__ bool bypass() const { return false; }
};

template <bool ATOMIC_SCATTER>
__global__ __launch_bounds__(BLK) void resample_bwd_pixel_kernel(int Hv, int Wv, int H, int W, int n_out,
                                                                 const float* __restrict__ vr, const float* __restrict__ uva,
                                                                 const float* __restrict__ M, int fill_channel,
                                                                 const float* __restrict__ gs, const float* __restrict__ guv,
                                                                 float* __restrict__ gvr, float* __restrict__ guva,
                                                                 int4* __restrict__ bbox) {
  __shared__ int s_box[4][BLK / 64];
  const int tx = threadIdx.x & (OT - 1), ty = threadIdx.x >> 4;
  const int x = blockIdx.x * OT + tx, y = blockIdx.y * OT + ty;
  const bool live = x < W && y < H;
  const int HW = H * W;
  const size_t p = (size_t)y * W + x;
  int bx0 = 0x7FFFFFFF, by0 = 0x7FFFFFFF, bx1 = -0x7FFFFFFF, by1 = -0x7FFFFFFF;
  if (live) {
    const float a = uva[3 * p], b = uva[3 * p + 1], c = uva[3 * p + 2];
    const float u = M[0] * a + M[1] * b + M[2] * c, v = M[3] * a + M[4] * b + M[5] * c;
    const Taps t = make_taps(u, v, Wv, Hv);
    const float wx0 = 1.f - t.wx1, wy0 = 1.f - t.wy1;
    const size_t plane = (size_t)Hv * Wv;
    const size_t o00 = (size_t)t.y0 * Wv + t.x0;
    const bool outside = fabsf(u) > 1.f || fabsf(v) > 1.f;
    float gix = 0.f, giy = 0.f;
    // (gradients and taps of up to four channels requested together, as in the forward; sums in channel order as before)
    for (int c0 = 0; c0 < n_out; c0 += 4) {
      float gq[4], v[4][4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool on = c0 + k < n_out;
        const int ch = on ? c0 + k : 0;
        gq[k] = on ? gs[(size_t)ch * HW + p] : 0.f;
        const float* src = vr + (size_t)ch * plane;
        v[k][0] = (on && t.in_y0 && t.in_x0) ? src[o00] : 0.f;
        v[k][1] = (on && t.in_y0 && t.in_x1) ? src[o00 + 1] : 0.f;
        v[k][2] = (on && t.in_y1 && t.in_x0) ? src[o00 + Wv] : 0.f;
        v[k][3] = (on && t.in_y1 && t.in_x1) ? src[o00 + Wv + 1] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int ch = c0 + k;
        if (ch >= n_out) break;
        float g = gq[k];
        if (ch == fill_channel && outside) g = 0.f;  // the value was overwritten by a constant
        float* dst = gvr + (size_t)ch * plane;
        if (t.in_y0 && t.in_x0) {
          const float val = v[k][0];
          if (ATOMIC_SCATTER) unsafeAtomicAdd(dst + o00, g * wx0 * wy0);
          gix -= val * wy0 * g; giy -= val * wx0 * g;
        }
        if (t.in_y0 && t.in_x1) {
          const float val = v[k][1];
          if (ATOMIC_SCATTER) unsafeAtomicAdd(dst + o00 + 1, g * t.wx1 * wy0);
          gix += val * wy0 * g; giy -= val * t.wx1 * g;
        }
        if (t.in_y1 && t.in_x0) {
          const float val = v[k][2];
          if (ATOMIC_SCATTER) unsafeAtomicAdd(dst + o00 + Wv, g * wx0 * t.wy1);
          gix -= val * t.wy1 * g; giy += val * wx0 * g;
        }
        if (t.in_y1 && t.in_x1) {
          const float val = v[k][3];
          if (ATOMIC_SCATTER) unsafeAtomicAdd(dst + o00 + Wv + 1, g * t.wx1 * t.wy1);
          gix += val * t.wy1 * g; giy += val * t.wx1 * g;
        }
      }
    }
    // d(ix)/du = (Wv-1)/2 (align_corners=True)
    float gu = gix * (0.5f * (float)(Wv - 1)), gv = giy * (0.5f * (float)(Hv - 1));
    if (guv) {
      const float2 e = reinterpret_cast<const float2*>(guv)[p];
      gu += e.x; gv += e.y;
    }
    guva[3 * p] = M[0] * gu + M[3] * gv;
    guva[3 * p + 1] = M[1] * gu + M[4] * gv;
    guva[3 * p + 2] = M[2] * gu + M[5] * gv;
    if ((t.in_x0 || t.in_x1) && (t.in_y0 || t.in_y1)) {  // cells [x0, x0+1] x [y0, y0+1], clamped values
      bx0 = t.x0; bx1 = t.x0 + 1; by0 = t.y0; by1 = t.y0 + 1;
    }
  }
  if (!ATOMIC_SCATTER) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      bx0 = min(bx0, __shfl_xor(bx0, o, 64)); by0 = min(by0, __shfl_xor(by0, o, 64));
      bx1 = max(bx1, __shfl_xor(bx1, o, 64)); by1 = max(by1, __shfl_xor(by1, o, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_box[0][w] = bx0; s_box[1][w] = by0; s_box[2][w] = bx1; s_box[3][w] = by1; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < BLK / 64; k++) {
        bx0 = min(bx0, s_box[0][k]); by0 = min(by0, s_box[1][k]); bx1 = max(bx1, s_box[2][k]); by1 = max(by1, s_box[3][k]);
      }
      bbox[blockIdx.y * gridDim.x + blockIdx.x] = make_int4(bx0, by0, bx1, by1);  // empty: x0 > x1
    }
  }
}

template <int NACC>
__global__ __launch_bounds__(BLK) void resample_bwd_tile_kernel(int C, int Hv, int Wv, int H, int W, int n_out,
                                                                const float* __restrict__ uva, const float* __restrict__ M,
                                                                int fill_channel, const float* __restrict__ gs,
                                                                const int4* __restrict__ bbox, int ntx, int nty,
                                                                float* __restrict__ gvr) {
  __shared__ float s_acc[NACC][VTY][VTX];
  __shared__ uint32_t s_list[1024];
  __shared__ uint32_t s_n;
  const int vx0 = blockIdx.x * VTX, vy0 = blockIdx.y * VTY;
  for (int e = threadIdx.x; e < NACC * VTY * VTX; e += BLK) (&s_acc[0][0][0])[e] = 0.f;
  const int HW = H * W;
  const int nt = ntx * nty;
  for (int scanned = 0; scanned < nt; scanned += 1024) {  // candidate output tiles: 1024 boxes per round
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int lim = min(scanned + 1024, nt);
    for (int t = scanned + threadIdx.x; t < lim; t += BLK) {
      const int4 bb = bbox[t];
      if (bb.x <= vx0 + VTX - 1 && bb.z >= vx0 && bb.y <= vy0 + VTY - 1 && bb.w >= vy0)
        s_list[atomicAdd(&s_n, 1u)] = (uint32_t)t;
    }
    __syncthreads();
    const uint32_t n = s_n;
    for (uint32_t k = 0; k < n; k++) {
      const int t = (int)s_list[k];
      const int x = (t % ntx) * OT + (threadIdx.x & (OT - 1)), y = (t / ntx) * OT + (threadIdx.x >> 4);
      if (x >= W || y >= H) continue;
      const size_t p = (size_t)y * W + x;
      const float a = uva[3 * p], b = uva[3 * p + 1], c = uva[3 * p + 2];
      const float u = M[0] * a + M[1] * b + M[2] * c, v = M[3] * a + M[4] * b + M[5] * c;
      const Taps tp = make_taps(u, v, Wv, Hv);
      const int lx = tp.x0 - vx0, ly = tp.y0 - vy0;
      if (lx < -1 || lx >= VTX || ly < -1 || ly >= VTY) continue;
      const float wx0 = 1.f - tp.wx1, wy0 = 1.f - tp.wy1;
      const bool outside = fabsf(u) > 1.f || fabsf(v) > 1.f;
      const bool cx0 = lx >= 0 && tp.in_x0, cx1 = lx + 1 < VTX && tp.in_x1;
      const bool cy0 = ly >= 0 && tp.in_y0, cy1 = ly + 1 < VTY && tp.in_y1;
#pragma unroll
      for (int ch = 0; ch < NACC; ch++) {
        if (ch >= n_out) break;
        float g = gs[(size_t)ch * HW + p];
        if (ch == fill_channel && outside) g = 0.f;
        if (cy0 && cx0) lds_add(&s_acc[ch][ly][lx], g * wx0 * wy0);
        if (cy0 && cx1) lds_add(&s_acc[ch][ly][lx + 1], g * tp.wx1 * wy0);
        if (cy1 && cx0) lds_add(&s_acc[ch][ly + 1][lx], g * wx0 * tp.wy1);
        if (cy1 && cx1) lds_add(&s_acc[ch][ly + 1][lx + 1], g * tp.wx1 * tp.wy1);
      }
    }
    __syncthreads();
  }
  // every virtual pixel of the tile, every channel (channels >= n_out get zeros): plain coalesced stores
  const size_t plane = (size_t)Hv * Wv;
  for (int e = threadIdx.x; e < VTY * VTX; e += BLK) {
    const int ly = e / VTX, lx = e - ly * VTX;
    const int gx = vx0 + lx, gy = vy0 + ly;
    if (gx < Wv && gy < Hv) {
      for (int ch = 0; ch < C; ch++)
        gvr[ch * plane + (size_t)gy * Wv + gx] = (ch < NACC && ch < n_out) ? s_acc[ch < NACC ? ch : 0][ly][lx] : 0.f;
    }
  }
}


}  // namespace

static size_t resample_bwd_ws_bytes(int H, int W) {
  const size_t nt = (size_t)((W + OT - 1) / OT) * ((H + OT - 1) / OT);
  return (nt * sizeof(int4) + 255) / 256 * 256 + 256;
}

static void launch_resample_bwd(int C, int Hv, int Wv, int H, int W, int n_out, const float* vr, const float* uva,
                         const float* M, int fill_channel, const float* gs, const float* guv, float* gvr, float* guva,
                         void* ws, hipStream_t s) {
  const int ntx = (W + OT - 1) / OT, nty = (H + OT - 1) / OT;
  if (n_out > 4 || !ws) {  // more channels than the LDS tile holds (the reference keeps 4): atomic scatter
    (void)hipMemsetAsync(gvr, 0, (size_t)C * Hv * Wv * sizeof(float), s);
    hipLaunchKernelGGL(resample_bwd_pixel_kernel<true>, dim3(ntx, nty), dim3(BLK), 0, s, Hv, Wv, H, W, n_out, vr, uva, M,
                       fill_channel, gs, guv, gvr, guva, (int4*)nullptr);
    return;
  }
  int4* bbox = reinterpret_cast<int4*>(ws_base(ws));
  hipLaunchKernelGGL(resample_bwd_pixel_kernel<false>, dim3(ntx, nty), dim3(BLK), 0, s, Hv, Wv, H, W, n_out, vr, uva, M,
                     fill_channel, gs, guv, gvr, guva, bbox);
  static const int form = [] {  // EOGS_RESAMPLE_BWD=1: the first form (LDS float atomics); default: the bucketed gather
    const char* e = getenv("EOGS_RESAMPLE_BWD");
    return e ? atoi(e) : 2;
  }();
  if (form == 1) {
    hipLaunchKernelGGL(resample_bwd_tile_kernel<4>, dim3((Wv + VTX - 1) / VTX, (Hv + VTY - 1) / VTY), dim3(BLK), 0, s, C, Hv, Wv,
                       H, W, n_out, uva, M, fill_channel, gs, bbox, ntx, nty, gvr);
    return;
  }
  // virtual tile 64 x 32 for large virtual images, 32 x 32 below 1.5 M cells (a 1024^2 image would be 512 workgroups on 256 CUs)
  const bool big = (size_t)Hv * Wv > 1500000;
  auto* kern = n_out == 1 ? (big ? resample_bwd_gather_kernel<1, 64, 32, ResampleSrc> : resample_bwd_gather_kernel<1, 32, 32, ResampleSrc>)
                          : (big ? resample_bwd_gather_kernel<4, 64, 32, ResampleSrc> : resample_bwd_gather_kernel<4, 32, 32, ResampleSrc>);
  const int vx = big ? 64 : 32, vy = 32;
  hipLaunchKernelGGL(kern, dim3((Wv + vx - 1) / vx, (Hv + vy - 1) / vy), dim3(BLK), 0, s, C, Hv, Wv, H, W, n_out,
                     ResampleSrc{uva, M}, fill_channel, gs, bbox, ntx, nty, gvr);
}

static int resample_check(const char* who, int C, int Hv, int Wv, int H, int W, int n_out, int fill_channel) {
  if (C <= 0 || Hv <= 0 || Wv <= 0 || H <= 0 || W <= 0 || n_out <= 0 || n_out > C || fill_channel >= n_out ||
      (int64_t)H * W > 0x7FFFFFFF || (int64_t)Hv * Wv > 0x7FFFFFFF)
    return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes", who);
  return EOGS_OK;
}

extern "C" {

int eogs_resample_forward(int C, int Hv, int Wv, int H, int W, int n_out, const float* virtual_render, const float* uva,
                          const float* cam2virt, int fill_channel, float fill_value, float* sample, float* uv,
                          void* stream) {
  clear_error();
  const int rc = resample_check("resample_forward", C, Hv, Wv, H, W, n_out, fill_channel);
  if (rc != EOGS_OK) return rc;
  if (!virtual_render || !uva || !cam2virt || !sample || !uv) return fail(EOGS_ERR_INVALID_ARG, "resample_forward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  {
    ProfScope ps(PS_RESAMPLE_FWD, s);
    hipLaunchKernelGGL(resample_fwd_kernel, dim3((HW + BLK - 1) / BLK), dim3(BLK), 0, s, C, Hv, Wv, HW, n_out, virtual_render, uva,
                       cam2virt, fill_channel, fill_value, sample, uv);
  }
  LAUNCH_TRY(s, false, "resample_fwd");
  return EOGS_OK;
}

int eogs_resample_bytes(int H, int W, size_t* bytes) {
  if (H <= 0 || W <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "resample_bytes: bad argument");
  *bytes = resample_bwd_ws_bytes(H, W);
  return EOGS_OK;
}

int eogs_resample_backward(int C, int Hv, int Wv, int H, int W, int n_out, const float* virtual_render, const float* uva,
                           const float* cam2virt, int fill_channel, const float* dL_dsample, const float* dL_duv,
                           float* dL_dvirtual, float* dL_duva, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const int rc = resample_check("resample_backward", C, Hv, Wv, H, W, n_out, fill_channel);
  if (rc != EOGS_OK) return rc;
  if (!virtual_render || !uva || !cam2virt || !dL_dsample || !dL_dvirtual || !dL_duva)
    return fail(EOGS_ERR_INVALID_ARG, "resample_backward: NULL argument");
  if (ws && ws_bytes < resample_bwd_ws_bytes(H, W)) return fail(EOGS_ERR_WORKSPACE, "resample_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_RESAMPLE_BWD, s); launch_resample_bwd(C, Hv, Wv, H, W, n_out, virtual_render, uva, cam2virt, fill_channel, dL_dsample, dL_duv, dL_dvirtual, dL_duva, ws, s); }
  LAUNCH_TRY(s, false, "resample_bwd");
  return EOGS_OK;
}

}  // extern "C"
