// tsdf.hip — TSDF integration of one altitude image into the voxel volume (include/eogs_tsdf.h).
// Reference semantics: src/gaussiansplatting/tsdf.py:325-368 (sample_sdf), :459-520 (integrate, update_tsdf).
//
// One lane per voxel, z fastest (the volumes' contiguous axis): a wave covers 64 consecutive altitudes of one (x, y)
// column pair, which project to almost the same pixel under the near-nadir affine cameras, so the four bilinear taps are
// served by L1/L2; HBM traffic is the 8 B/voxel read + 8 B/voxel conditional write of the two volumes.
//
// The stages around it (eogs_tsdf_normals / _prior / _surface):
//   normals   RangeImageEOGS.__init__ / reconstruct_normals / get_weights (tsdf.py:213-231, 243-323): one lane per pixel,
//             coalesced along W; the 9 taps of the 5x5 cross are recomputed from the altitude image (L1/L2-served) instead
//             of the reference's unfold of the world-position image (75 floats per pixel).
//   prior     TSDFVolume.apply_prior (tsdf.py:602-638), two launches: one wave per (x, y) column writes a state byte per
//             voxel and the column's top occupied z; then one lane per voxel applies the rules from the state bytes only.
//   surface   TSDFVolume.extract_dsm up to plyflatten (tsdf.py:530-562): one wave per column, top-down 64-voxel chunks.
#include "api_util.h"

namespace {

struct TsdfAffine {
  float A[9], b[3], Ai[9], Aib[3];
};

__device__ inline float tap(const float* __restrict__ img, int H, int W, int x, int y) {
  return (x >= 0 && x < W && y >= 0 && y < H) ? img[(size_t)y * W + x] : 0.f;  // grid_sample padding_mode="zeros"
}

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(int nx, int ny, int nz, const float* __restrict__ ax,
                                                             const float* __restrict__ ay, const float* __restrict__ az,
                                                             const float* __restrict__ affine, float scale, float trunc,
                                                             int H, int W, const float* __restrict__ alt,
                                                             const float* __restrict__ wgt, float* __restrict__ tsdf,
                                                             float* __restrict__ wvol) {
  const size_t n = (size_t)nx * ny * nz;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int iz = (int)(i % nz), iy = (int)((i / nz) % ny), ix = (int)(i / ((size_t)nz * ny));
  const float* A = affine;
  const float* b = affine + 9;
  const float* Ai = affine + 12;
  const float* Aib = affine + 21;
  const float p[3] = {ax[ix] / scale, ay[iy] / scale, az[iz] / scale};
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; c++) v[c] = A[3 * c] * p[0] + A[3 * c + 1] * p[1] + A[3 * c + 2] * p[2] + b[c];
  // F.grid_sample(..., mode="bilinear", align_corners=True)
  const float fx = (v[0] + 1.f) * 0.5f * (float)(W - 1), fy = (v[1] + 1.f) * 0.5f * (float)(H - 1);
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float tx = fx - x0f, ty = fy - y0f;
  float a_s = 0.f, w_s = 0.f;
  if (fx > -2.f && fy > -2.f && fx < (float)W + 1.f && fy < (float)H + 1.f) {  // int conversion is safe
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float w00 = (1.f - tx) * (1.f - ty), w01 = tx * (1.f - ty), w10 = (1.f - tx) * ty, w11 = tx * ty;
    a_s = tap(alt, H, W, x0, y0) * w00 + tap(alt, H, W, x0 + 1, y0) * w01 + tap(alt, H, W, x0, y0 + 1) * w10 +
          tap(alt, H, W, x0 + 1, y0 + 1) * w11;
    w_s = tap(wgt, H, W, x0, y0) * w00 + tap(wgt, H, W, x0 + 1, y0) * w01 + tap(wgt, H, W, x0, y0 + 1) * w10 +
          tap(wgt, H, W, x0 + 1, y0 + 1) * w11;
  }
  const bool valid = fabsf(v[0]) <= 1.f && fabsf(v[1]) <= 1.f;
  const float vn[3] = {v[0], v[1], a_s};
  float d2 = 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float q = Ai[3 * c] * vn[0] + Ai[3 * c + 1] * vn[1] + Ai[3 * c + 2] * vn[2] - Aib[c];
    d2 += (q - p[c]) * (q - p[c]);
  }
  const float dz = v[2] - a_s;
  const float sgn = dz > 0.f ? 1.f : (dz < 0.f ? -1.f : 0.f);
  const float sdf = sqrtf(d2) * sgn * scale;
  if (valid && sdf >= -trunc) {
    const float t_new = fminf(1.f, sdf / trunc);
    const float w_old = wvol[i], t_old = tsdf[i];
    const float w_new = w_old + w_s;
    tsdf[i] = (w_old * t_old + w_s * t_new) / w_new;
    wvol[i] = w_new;
  }
}


// ---- range-image normals and weights (tsdf.py:243-323) ----

// On the device the reference's F.linear (world positions) and einsum (view angle) are GEMMs that accumulate with fused
// multiply-adds, and its vector norms are reductions compiled with contraction: those three are written here as explicit fmaf
// chains in the same order (the library's -ffp-contract=off leaves every other operation as written). The one-sided
// differences cancel most of a position's magnitude, so how the positions round decides how close the normals come to
// an exact evaluation.

// World position of pixel (r, c): view = ((c + 0.5) * (1/W) * 2 - 1, (r + 0.5) * (1/H) * 2 - 1, alt) (tsdf.py:252-258, the
// align_corners=False convention), world = inv(A) view - inv(A) b (F.linear, :238-240). F.unfold pads the WORLD-POSITION
// image with zeros, so a tap outside the image is (0, 0, 0).
__device__ inline void world_tap(const float* __restrict__ alt, const float* __restrict__ Ai, const float* __restrict__ Aib, int H,
                                 int W, float rW, float rH, int r, int c, float p[3]) {
  if (r < 0 || r >= H || c < 0 || c >= W) {
    p[0] = p[1] = p[2] = 0.f;
    return;
  }
  const float u = (((float)c + 0.5f) * rW) * 2.f - 1.f;
  const float v = (((float)r + 0.5f) * rH) * 2.f - 1.f;
  const float a = alt[(size_t)r * W + c];
#pragma unroll
  for (int k = 0; k < 3; k++) p[k] = fmaf(Ai[3 * k + 2], a, fmaf(Ai[3 * k + 1], v, Ai[3 * k] * u)) - Aib[k];
}

__device__ inline float norm3(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, x * x))); }

// One axis of tsdf.py:276-313: taps q[0..4] = p_{-2} .. p_{2}; the strict `<` sends a tie and a NaN to the right branch.
__device__ inline void one_sided_diff(const float q[5][3], float d[3]) {
  float pl[3], pr[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    pl[k] = q[0][k] + 2.f * (q[1][k] - q[0][k]) - q[2][k];
    pr[k] = q[4][k] + 2.f * (q[3][k] - q[4][k]) - q[2][k];
  }
  const bool left = norm3(pl[0], pl[1], pl[2]) < norm3(pr[0], pr[1], pr[2]);
#pragma unroll
  for (int k = 0; k < 3; k++) d[k] = left ? (q[2][k] - q[0][k]) * 0.5f : (q[4][k] - q[2][k]) * 0.5f;
}

__global__ __launch_bounds__(256) void tsdf_normals_kernel(int H, int W, float rW, float rH, const float* __restrict__ alt,
                                                           const float* __restrict__ affine, const float* __restrict__ view_dir,
                                                           float* __restrict__ normals, float* __restrict__ angle,
                                                           float* __restrict__ weights) {
  const size_t hw = (size_t)H * W;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int r = (int)(i / W), c = (int)(i % W);
  const float* Ai = affine + 12;
  const float* Aib = affine + 21;
  float qx[5][3], qy[5][3];
#pragma unroll
  for (int j = 0; j < 5; j++) world_tap(alt, Ai, Aib, H, W, rW, rH, r, c + j - 2, qx[j]);  // x runs along W (unfold k2)
#pragma unroll
  for (int j = 0; j < 5; j++) {  // y runs along H (unfold k1); the centre tap is shared
    if (j == 2) {
#pragma unroll
      for (int k = 0; k < 3; k++) qy[2][k] = qx[2][k];
    } else {
      world_tap(alt, Ai, Aib, H, W, rW, rH, r + j - 2, c, qy[j]);
    }
  }
  float dx[3], dy[3];
  one_sided_diff(qx, dx);
  one_sided_diff(qy, dy);
  // torch.cross(dx, dy, dim=1) (an elementwise kernel: a*b - c*d contracted to fma(a, b, -(c*d))), then F.normalize(eps=1e-6):
  // n / clamp_min(|n|, eps) (clamp keeps a NaN norm)
  float n[3] = {fmaf(dx[1], dy[2], -(dx[2] * dy[1])), fmaf(dx[2], dy[0], -(dx[0] * dy[2])), fmaf(dx[0], dy[1], -(dx[1] * dy[0]))};
  float len = norm3(n[0], n[1], n[2]);
  if (len < 1e-6f) len = 1e-6f;
#pragma unroll
  for (int k = 0; k < 3; k++) n[k] = n[k] / len;
  // einsum(normals, -view_direction) (:220-222); get_weights = clamp(angle, 0, 1) (:322-323) keeps a NaN
  const float a = fmaf(n[2], -view_dir[2], fmaf(n[1], -view_dir[1], n[0] * -view_dir[0]));
  if (normals) {
#pragma unroll
    for (int k = 0; k < 3; k++) normals[k * hw + i] = n[k];
  }
  angle[i] = a;
  if (weights) weights[i] = a < 0.f ? 0.f : (a > 1.f ? 1.f : a);
}

// ---- volume prior (tsdf.py:602-638) ----
// Both masks come from the volume BEFORE anything is written (:603-604), so the prior is a pure function of its input.
constexpr unsigned char kOcc = 1;        // t <= 0 (a NaN is not occupied)
constexpr unsigned char kUntouched = 2;  // w == 0 & t == 1

// (a) one wave per (x, y) column: state byte per voxel, and top = the largest z with occ, 0 if none (argmax(occ * idx)).
__global__ __launch_bounds__(256) void tsdf_prior_state_kernel(int64_t ncol, int nz, const float* __restrict__ tsdf,
                                                               const float* __restrict__ wvol, unsigned char* __restrict__ state,
                                                               int* __restrict__ top) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); col < ncol; col += waves) {
    const size_t base = (size_t)col * nz;
    int t_top = 0;
    for (int z0 = 0; z0 < nz; z0 += 64) {
      const int z = z0 + lane;
      bool occ = false;
      if (z < nz) {
        const float t = tsdf[base + z], w = wvol[base + z];
        occ = t <= 0.f;
        state[base + z] = (occ ? kOcc : 0) | ((w == 0.f && t == 1.f) ? kUntouched : 0);
      }
      const unsigned long long m = __ballot(occ);
      if (m) t_top = z0 + 63 - __clzll((long long)m);
    }
    if (lane == 0) top[col] = t_top;
  }
}

// (b) one lane per voxel, from the state bytes only; the first matching rule applies, and t / w are stored only there:
//   1. occ and no occupied voxel among the 26 neighbours (conv3d with zero padding == 1)   -> (1, 0)   (:615-620)
//   2. z == 0                                                                              -> (-1, 1)  (:606-608)
//   3. untouched and z < top                                                               -> (-1, 1)  (:622-638)
__global__ __launch_bounds__(256) void tsdf_prior_apply_kernel(int nx, int ny, int nz, const unsigned char* __restrict__ state,
                                                               const int* __restrict__ top, float* __restrict__ tsdf,
                                                               float* __restrict__ wvol) {
  const size_t n = (size_t)nx * ny * nz;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const unsigned char s = state[i];
    const int iz = (int)(i % nz);
    const size_t col = i / nz;
    const int iy = (int)(col % ny), ix = (int)(col / ny);
    if (s & kOcc) {
      bool neighbour = false;
      for (int dx = -1; dx <= 1 && !neighbour; dx++) {
        const int x = ix + dx;
        if (x < 0 || x >= nx) continue;
        for (int dy = -1; dy <= 1 && !neighbour; dy++) {
          const int y = iy + dy;
          if (y < 0 || y >= ny) continue;
          const size_t cb = ((size_t)x * ny + y) * nz;
          for (int dz = -1; dz <= 1; dz++) {
            const int z = iz + dz;
            if (z < 0 || z >= nz || (dx == 0 && dy == 0 && dz == 0)) continue;
            if (state[cb + z] & kOcc) { neighbour = true; break; }
          }
        }
      }
      if (!neighbour) {
        tsdf[i] = 1.f;
        wvol[i] = 0.f;
        continue;
      }
    }
    if (iz == 0 || ((s & kUntouched) && iz < top[col])) {
      tsdf[i] = -1.f;
      wvol[i] = 1.f;
    }
  }
}

// ---- DSM heights (tsdf.py:530-536) ----
// index = argmax((t < 0) * idx): the LARGEST z with t < 0, 0 if none. One wave per column, 64-voxel chunks top-down.
__global__ __launch_bounds__(256) void tsdf_surface_kernel(int64_t ncol, int nz, const float* __restrict__ tsdf,
                                                           const float* __restrict__ az, int64_t* __restrict__ index,
                                                           float* __restrict__ height) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); col < ncol; col += waves) {
    const size_t base = (size_t)col * nz;
    int found = 0;
    for (int z0 = ((nz - 1) / 64) * 64; z0 >= 0; z0 -= 64) {
      const int z = z0 + lane;
      const unsigned long long m = __ballot(z < nz && tsdf[base + z] < 0.f);
      if (m) {
        found = z0 + 63 - __clzll((long long)m);
        break;
      }
    }
    if (lane == 0) {
      index[col] = found;
      if (height) height[col] = az[found];
    }
  }
}

}  // namespace

static unsigned column_blocks(int64_t ncol) {  // 4 waves per block, grid-stride beyond 2^20 blocks
  const int64_t b = (ncol + 3) / 4;
  return (unsigned)(b < (1 << 20) ? b : (1 << 20));
}

static size_t tsdf_prior_ws_bytes(int nx, int ny, int nz) {  // state bytes (256-aligned) + int32 top per column
  const size_t n = (size_t)nx * ny * nz;
  return ((n + 255) / 256) * 256 + 4 * (size_t)nx * ny;
}

extern "C" {

int eogs_tsdf_integrate(int nx, int ny, int nz, const float* ax, const float* ay, const float* az, const float* affine,
                        float model_scale, float trunc_margin, int H, int W, const float* altitude, const float* weight,
                        float* tsdf_vol, float* weight_vol, void* stream) {
  clear_error();
  if (nx < 0 || ny < 0 || nz < 0 || H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "tsdf_integrate: bad sizes");
  if ((size_t)nx * ny * nz == 0) return EOGS_OK;
  if ((uint64_t)nx * ny * nz > ((uint64_t)1 << 40)) return fail(EOGS_ERR_OVERFLOW, "tsdf_integrate: volume too large");
  if (!ax || !ay || !az || !affine || !altitude || !weight || !tsdf_vol || !weight_vol)
    return fail(EOGS_ERR_INVALID_ARG, "tsdf_integrate: NULL argument");
  if (!(model_scale != 0.f) || !(trunc_margin > 0.f)) return fail(EOGS_ERR_INVALID_ARG, "tsdf_integrate: bad scale or truncation");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)nx * ny * nz;
  {
    ProfScope ps(PS_TSDF, s);
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, nx, ny, nz, ax, ay, az, affine,
                       model_scale, trunc_margin, H, W, altitude, weight, tsdf_vol, weight_vol);
  }
  LAUNCH_TRY(s, false, "tsdf_integrate");
  return EOGS_OK;
}

int eogs_tsdf_normals(int H, int W, const float* altitude, const float* affine, const float* view_dir, float* normals, float* angle,
                      float* weights, void* stream) {
  clear_error();
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "tsdf_normals: bad sizes");
  if (!altitude || !affine || !view_dir || !angle) return fail(EOGS_ERR_INVALID_ARG, "tsdf_normals: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  const size_t hw = (size_t)H * W;
  // torch.tensor([1 / W, 1 / H, 1]) (tsdf.py:256): the Python quotients rounded once to fp32
  const float rW = (float)(1.0 / W), rH = (float)(1.0 / H);
  {
    ProfScope ps(PS_TSDF_NORMALS, s);
    hipLaunchKernelGGL(tsdf_normals_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, s, H, W, rW, rH, altitude, affine,
                       view_dir, normals, angle, weights);
  }
  LAUNCH_TRY(s, false, "tsdf_normals");
  return EOGS_OK;
}

int eogs_tsdf_prior_bytes(int nx, int ny, int nz, size_t* bytes) {
  clear_error();
  if (nx < 0 || ny < 0 || nz < 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "tsdf_prior_bytes: bad argument");
  if ((uint64_t)nx * ny * nz > ((uint64_t)1 << 40)) return fail(EOGS_ERR_OVERFLOW, "tsdf_prior_bytes: volume too large");
  *bytes = tsdf_prior_ws_bytes(nx, ny, nz);
  return EOGS_OK;
}

int eogs_tsdf_prior(int nx, int ny, int nz, float* tsdf_vol, float* weight_vol, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (nx < 0 || ny < 0 || nz < 0) return fail(EOGS_ERR_INVALID_ARG, "tsdf_prior: bad sizes");
  if ((size_t)nx * ny * nz == 0) return EOGS_OK;
  if ((uint64_t)nx * ny * nz > ((uint64_t)1 << 40)) return fail(EOGS_ERR_OVERFLOW, "tsdf_prior: volume too large");
  if (!tsdf_vol || !weight_vol || !ws) return fail(EOGS_ERR_INVALID_ARG, "tsdf_prior: NULL argument");
  if (ws_bytes < tsdf_prior_ws_bytes(nx, ny, nz)) return fail(EOGS_ERR_WORKSPACE, "tsdf_prior: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)nx * ny * nz;
  const int64_t ncol = (int64_t)nx * ny;
  unsigned char* state = (unsigned char*)ws;
  int* top = (int*)(state + ((n + 255) / 256) * 256);
  const size_t b = (n + 255) / 256;
  {
    ProfScope ps(PS_TSDF_PRIOR, s);
    hipLaunchKernelGGL(tsdf_prior_state_kernel, dim3(column_blocks(ncol)), dim3(256), 0, s, ncol, nz, tsdf_vol, weight_vol, state, top);
    hipLaunchKernelGGL(tsdf_prior_apply_kernel, dim3((unsigned)(b < (1u << 20) ? b : (1u << 20))), dim3(256), 0, s, nx, ny, nz, state,
                       top, tsdf_vol, weight_vol);
  }
  LAUNCH_TRY(s, false, "tsdf_prior");
  return EOGS_OK;
}

int eogs_tsdf_surface(int nx, int ny, int nz, const float* tsdf_vol, const float* az, int64_t* index, float* height, void* stream) {
  clear_error();
  if (nx < 0 || ny < 0 || nz <= 0) return fail(EOGS_ERR_INVALID_ARG, "tsdf_surface: bad sizes");
  if ((size_t)nx * ny == 0) return EOGS_OK;
  if ((uint64_t)nx * ny * nz > ((uint64_t)1 << 40)) return fail(EOGS_ERR_OVERFLOW, "tsdf_surface: volume too large");
  if (!tsdf_vol || !az || !index) return fail(EOGS_ERR_INVALID_ARG, "tsdf_surface: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  const int64_t ncol = (int64_t)nx * ny;
  {
    ProfScope ps(PS_TSDF_SURFACE, s);
    hipLaunchKernelGGL(tsdf_surface_kernel, dim3(column_blocks(ncol)), dim3(256), 0, s, ncol, nz, tsdf_vol, az, index, height);
  }
  LAUNCH_TRY(s, false, "tsdf_surface");
  return EOGS_OK;
}

}  // extern "C"
