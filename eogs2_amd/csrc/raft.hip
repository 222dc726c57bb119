// raft.hip — the three operators RAFT needs beside convolutions (include/eogs_resample.h, eogs_raft_*): the channel-last feature pyramid,
// the on-demand correlation lookup, and the convex / bilinear upsampling of the 1/8-resolution flow.
//
// The lookup is the kernel that matters. A workgroup owns LT_W x LT_H pixels at ONE level, a lane one pixel. A lane keeps all
// (2r+2)^2 dot products of its pixel in registers and walks the channels in chunks of 16 (8 at radius 4): per chunk it loads
// those channels of its own fmap1 row (16-byte loads from the channel-last copy) and, per tap, of the tap's fmap2_l row, one
// fused multiply-add per channel in ascending order. Where the bounding box of the tile's windows holds at most LMAXPOS
// positions of the level the workgroup copies the chunk of the box into LDS first (rows padded by one float4: sixteen lanes
// that read neighbouring positions with ds_read_b128 then fall on sixteen different 16-byte bank groups) and every tap reads LDS;
// otherwise every tap reads the pyramid in global memory. For this application's flows (registration errors of a few
// pixels) neighbouring pixels read almost the same window and the box is the tile grown by the radius: every staged row is
// used (2r+2)^2 times. Both paths run ONE function template over the same operands in the same order, so they give the same
// bits. The blend then forms K^2 outputs from the (K+1)^2 dots with the pixel's one fractional offset per axis.
//
// Which path runs is the workgroup's decision alone (a min / max over its lanes' clamped floors, raft_taps.h), so it cannot
// depend on anything but the tile's own coordinates: bitwise reproducible.
#include "api_util.h"
#include "raft_taps.h"

namespace {

constexpr int LT_W = 32, LT_H = 4, LNT = LT_W * LT_H;  // lookup tile: a wave writes two 128-byte runs per channel
constexpr int LQ_MAX = 4;                               // float4 per position and chunk: 16 channels (8 at radius 4, whose 100
                                                        // running sums leave fewer registers for rows in flight)
constexpr int LMAXPOS = 768;                            // staged positions: 768 x (LQ_MAX + 1) x 16 B = 60 KiB, two workgroups per CU
static_assert(LNT % 64 == 0 && LNT / 64 == 2, "the box reduction combines two waves");

struct RaftLevels {
  int64_t off[EOGS_RAFT_MAX_LEVELS];  // in floats from the pyramid's (256-byte aligned) base
  int h[EOGS_RAFT_MAX_LEVELS], w[EOGS_RAFT_MAX_LEVELS];
  size_t bytes;
};

inline RaftLevels raft_levels(int N, int C, int h, int w, int levels) {
  RaftLevels t{};
  size_t o = 0;
  for (int l = 0; l < levels; l++) {
    t.h[l] = h >> l;
    t.w[l] = w >> l;
    o = ws_align(o);
    t.off[l] = (int64_t)(o / sizeof(float));
    o += (size_t)N * (size_t)t.h[l] * (size_t)t.w[l] * (size_t)C * sizeof(float);
  }
  t.bytes = ws_align(o) + 256;
  return t;
}

// ---- pyramid ----

// f32[N][C][P] -> f32[N][P][C] through a 32 x 32 tile
__global__ __launch_bounds__(256) void raft_to_cl_kernel(int C, int P, const float* __restrict__ in, float* __restrict__ out) {
  __shared__ float t[32][33];
  const int n = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, p = p0 + tx;
    if (c < C && p < P) t[i][tx] = in[((int64_t)n * C + c) * P + p];
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int p = p0 + i, c = c0 + tx;
    if (p < P && c < C) out[((int64_t)n * P + p) * C + c] = t[tx][i];
  }
}

// level l from level l - 1, both channel-last; one lane per (n, y, x, four channels)
__global__ __launch_bounds__(256) void raft_pool_kernel(int N, int C4, int hs, int ws, int hd, int wd, const float4* __restrict__ src,
                                                        float4* __restrict__ dst) {
  const int64_t total = (int64_t)N * hd * wd * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    int64_t r = i / C4;
    const int x = (int)(r % wd);
    r /= wd;
    const int y = (int)(r % hd), n = (int)(r / hd);
    const int64_t s0 = (((int64_t)n * hs + 2 * y) * ws + 2 * x) * C4 + c;
    const float4 a = src[s0], b = src[s0 + C4], e = src[s0 + (int64_t)ws * C4], d = src[s0 + (int64_t)ws * C4 + C4];
    float4 o;
    o.x = ((a.x + b.x) + (e.x + d.x)) * 0.25f;
    o.y = ((a.y + b.y) + (e.y + d.y)) * 0.25f;
    o.z = ((a.z + b.z) + (e.z + d.z)) * 0.25f;
    o.w = ((a.w + b.w) + (e.w + d.w)) * 0.25f;
    dst[i] = o;
  }
}

// ---- lookup ----

// min over the workgroup's two waves of four ints at once (negate for a max); every lane gets the result
__device__ inline int4 wg_min4(int4 v, int4* s_red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    v.x = min(v.x, __shfl_xor(v.x, o, 64));
    v.y = min(v.y, __shfl_xor(v.y, o, 64));
    v.z = min(v.z, __shfl_xor(v.z, o, 64));
    v.w = min(v.w, __shfl_xor(v.w, o, 64));
  }
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int4 a = s_red[0], b = s_red[1];
  return make_int4(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z), min(a.w, b.w));
}

// One chunk of the channels for one lane: acc[a][b] += <f1 chunk, row(a, b) chunk>, channels in ascending order. `rows` is
// LDS (the staged box, LPQ float4 per position) or the pyramid level (C / 4 float4 per position, already offset to the
// chunk); xo / yo are the taps' offsets in float4 along each axis. The one place the dot product is written.
template <int T, int LQ, class Ptr>
__device__ inline void accumulate_chunk(float (&acc)[T][T], const float4 (&f1)[LQ], Ptr rows, const int (&xo)[T], const int (&yo)[T], int nq) {
#pragma unroll
  for (int a = 0; a < T; a++) {
#pragma unroll
    for (int b = 0; b < T; b++) {
      Ptr p = rows + (xo[a] + yo[b]);
      float s = acc[a][b];
#pragma unroll
      for (int q = 0; q < LQ; q++) {
        if (q < nq) {
          const float4 v = p[q];
          s = fmaf(f1[q].x, v.x, s);
          s = fmaf(f1[q].y, v.y, s);
          s = fmaf(f1[q].z, v.z, s);
          s = fmaf(f1[q].w, v.w, s);
        }
      }
      acc[a][b] = s;
    }
  }
}

template <int R>
__global__ __launch_bounds__(LNT) void raft_lookup_kernel(int C, int h, int w, int levels, RaftLevels lt, const float4* __restrict__ f1cl,
                                                          const float* __restrict__ pyramid, const float* __restrict__ coords,
                                                          float* __restrict__ out, double inv_sqrt_c, int no_stage) {
  constexpr int K = 2 * R + 1, T = K + 1;
  constexpr int LQ = R >= 4 ? 2 : LQ_MAX;  // float4 per position and chunk
  constexpr int LPQ = LQ + 1;              // float4 per staged position: one of padding
  __shared__ float4 s_box[LMAXPOS * (LQ_MAX + 1)];
  __shared__ int4 s_red[LNT / 64];
  const int l = blockIdx.y, n = blockIdx.z;
  const int tiles_x = (w + LT_W - 1) / LT_W;
  const int px = (blockIdx.x % tiles_x) * LT_W + (threadIdx.x % LT_W), py = (blockIdx.x / tiles_x) * LT_H + (threadIdx.x / LT_W);
  const bool live = px < w && py < h;
  const int hl = lt.h[l], wl = lt.w[l], C4 = C >> 2;
  const float4* __restrict__ lvl = reinterpret_cast<const float4*>(pyramid + lt.off[l]) + (int64_t)n * hl * wl * C4;

  RaftAxisTap ax{0, 0.f}, ay{0, 0.f};
  if (live) {
    ax = raft_axis_tap(coords[(((int64_t)n * 2 + 0) * h + py) * w + px], l, wl, R);
    ay = raft_axis_tap(coords[(((int64_t)n * 2 + 1) * h + py) * w + px], l, hl, R);
  }
  // the bounding box of the tile's windows, cut to the level: [bx0, bx1] x [by0, by1]
  const int big = 0x3FFFFFFF;
  const int4 lo = wg_min4(make_int4(live ? ax.f : big, live ? ay.f : big, live ? -ax.f : big, live ? -ay.f : big), s_red);
  const int bx0 = max(lo.x - R, 0), by0 = max(lo.y - R, 0);
  const int bx1 = min(-lo.z + R + 1, wl - 1), by1 = min(-lo.w + R + 1, hl - 1);
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  const bool any = bw > 0 && bh > 0;  // false: every tap of every pixel lies outside, all outputs are 0
  const bool staged = any && !no_stage && (int64_t)bw * bh <= LMAXPOS;

  // the taps of this lane: offsets in float4 (clamped into the box, so that an outside tap reads something harmless), validity
  int xo[T], yo[T];
  unsigned vx = 0u, vy = 0u;
#pragma unroll
  for (int k = 0; k < T; k++) {
    const int x = raft_tap_pos(ax.f, R, k), y = raft_tap_pos(ay.f, R, k);
    if (live && raft_tap_inside(x, wl)) vx |= 1u << k;
    if (live && raft_tap_inside(y, hl)) vy |= 1u << k;
    const int xc = any ? min(max(x, bx0), bx1) : 0, yc = any ? min(max(y, by0), by1) : 0;
    xo[k] = staged ? (xc - bx0) * LPQ : xc * C4;
    yo[k] = staged ? (yc - by0) * bw * LPQ : yc * wl * C4;
  }

  float acc[T][T];
#pragma unroll
  for (int a = 0; a < T; a++)
#pragma unroll
    for (int b = 0; b < T; b++) acc[a][b] = 0.f;

  if (any) {
    const float4* __restrict__ f1p = f1cl + (((int64_t)n * h + (live ? py : 0)) * w + (live ? px : 0)) * C4;
    for (int c4 = 0; c4 < C4; c4 += LQ) {
      const int nq = min(LQ, C4 - c4);
      float4 f1[LQ];
#pragma unroll
      for (int q = 0; q < LQ; q++) f1[q] = q < nq ? f1p[c4 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
      if (staged) {
        __syncthreads();  // the previous chunk has been read
        const int items = bw * bh * nq;
        for (int i = threadIdx.x; i < items; i += LNT) {
          const int q = i % nq, pos = i / nq;
          const int by = pos / bw, bx = pos - by * bw;
          s_box[pos * LPQ + q] = lvl[((int64_t)(by0 + by) * wl + (bx0 + bx)) * C4 + c4 + q];
        }
        __syncthreads();
        accumulate_chunk<T, LQ>(acc, f1, (const float4*)s_box, xo, yo, nq);
      } else {
        accumulate_chunk<T, LQ>(acc, f1, lvl + c4, xo, yo, nq);
      }
    }
  }
  if (!live) return;

  // D = acc / sqrt(C), exactly 0 outside; then the 2 x 2 blend with the pixel's one fraction per axis. The blend and the scale
  // run in float64 and round once: beside the dot product's C roundings the output carries one more.
  const double wx1 = (double)ax.w, wy1 = (double)ay.w, wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
  const double w00 = wx0 * wy0, w10 = wx1 * wy0, w01 = wx0 * wy1, w11 = wx1 * wy1;
#pragma unroll
  for (int a = 0; a < T; a++)
#pragma unroll
    for (int b = 0; b < T; b++) acc[a][b] = ((vx >> a) & 1u) && ((vy >> b) & 1u) ? acc[a][b] : 0.f;
  const int64_t plane = (int64_t)h * w;
  float* __restrict__ o = out + ((int64_t)n * levels + l) * (K * K) * plane + (int64_t)py * w + px;
#pragma unroll
  for (int a = 0; a < K; a++)
#pragma unroll
    for (int b = 0; b < K; b++)
      o[(int64_t)raft_tap_channel(a, b, K) * plane] =
          (float)((((w00 * (double)acc[a][b] + w10 * (double)acc[a + 1][b]) + w01 * (double)acc[a][b + 1]) + w11 * (double)acc[a + 1][b + 1]) *
                  inv_sqrt_c);
}

// ---- upsampling ----

constexpr int UNT = 256;

// one lane per (n, y, x, i): the eight outputs (8y + i, 8x ... 8x + 7) of both planes, two 16-byte stores each; lanes run
// along x, so a mask channel is read in whole lines and the outputs of a wave are one contiguous run per plane
template <int MODE>
__global__ __launch_bounds__(UNT) void raft_upsample_kernel(int N, int h, int w, const float* __restrict__ flow,
                                                            const float* __restrict__ mask, float* __restrict__ out) {
  const int64_t total = (int64_t)N * h * 8 * w;
  const int64_t plane = (int64_t)h * w, oplane = plane * 64;
  for (int64_t t = (int64_t)blockIdx.x * UNT + threadIdx.x; t < total; t += (int64_t)gridDim.x * UNT) {
    const int x = (int)(t % w);
    int64_t r = t / w;
    const int i = (int)(r & 7);
    r >>= 3;
    const int y = (int)(r % h), n = (int)(r / h);
    const float* f0 = flow + (int64_t)n * 2 * plane;
    float res[2][8];
    if (MODE == EOGS_RAFT_UP_CONVEX) {
      float u[2][9];  // 8 flow over the zero-padded 3 x 3 neighbourhood
#pragma unroll
      for (int k = 0; k < 9; k++) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        u[0][k] = in ? 8.f * f0[(int64_t)yy * w + xx] : 0.f;
        u[1][k] = in ? 8.f * f0[plane + (int64_t)yy * w + xx] : 0.f;
      }
      const float* m0 = mask + ((int64_t)n * EOGS_RAFT_MASK_CHANNELS + i * 8) * plane + (int64_t)y * w + x;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        float v[9];
#pragma unroll
        for (int k = 0; k < 9; k++) v[k] = m0[(int64_t)(k * 64 + j) * plane];
        float m = v[0];
#pragma unroll
        for (int k = 1; k < 9; k++) m = fmaxf(m, v[k]);
        float S = 0.f, a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int k = 0; k < 9; k++) {
          const float e = expf(v[k] - m);
          S = S + e;
          a0 = a0 + e * u[0][k];
          a1 = a1 + e * u[1][k];
        }
        res[0][j] = a0 / S;
        res[1][j] = a1 / S;
      }
    } else {
      // source row Y (h - 1) / (8h - 1) as integer + fraction, both exact; the two weights one rounding each
      const int Y = 8 * y + i, dy = 8 * h - 1, dx = 8 * w - 1;
      const int ny = Y * (h - 1), y0 = ny / dy, ry = ny - y0 * dy, y1 = min(y0 + 1, h - 1);
      const float ly = (float)ry / (float)dy, hy = (float)(dy - ry) / (float)dy;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int X = 8 * x + j;
        const int nx = X * (w - 1), x0 = nx / dx, rx = nx - x0 * dx, x1 = min(x0 + 1, w - 1);
        const float lx = (float)rx / (float)dx, hx = (float)(dx - rx) / (float)dx;
#pragma unroll
        for (int c = 0; c < 2; c++) {
          const float* f = f0 + c * plane;
          const float top = hx * f[(int64_t)y0 * w + x0] + lx * f[(int64_t)y0 * w + x1];
          const float bot = hx * f[(int64_t)y1 * w + x0] + lx * f[(int64_t)y1 * w + x1];
          res[c][j] = 8.f * (hy * top + ly * bot);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 2; c++) {
      float4* o = reinterpret_cast<float4*>(out + ((int64_t)n * 2 + c) * oplane + (int64_t)(8 * y + i) * (8 * w) + 8 * x);
      o[0] = make_float4(res[c][0], res[c][1], res[c][2], res[c][3]);
      o[1] = make_float4(res[c][4], res[c][5], res[c][6], res[c][7]);
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int raft_check_shape(const char* who, int N, int C, int h, int w, int levels) {
  if (N < 1 || C < 1 || h < 1 || w < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (N, C, h and w must be at least 1)", who);
  if (C % 4) return fail(EOGS_ERR_INVALID_ARG, "%s: C must be a multiple of 4", who);
  if (levels < 1 || levels > EOGS_RAFT_MAX_LEVELS) return fail(EOGS_ERR_INVALID_ARG, "%s: levels must be 1 to 4", who);
  if ((h >> (levels - 1)) < 1 || (w >> (levels - 1)) < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: the map is too small for its levels (the last one would be empty)", who);
  if (N > 65535) return fail(EOGS_ERR_INVALID_ARG, "%s: N above 65535", who);
  if ((int64_t)N * C * h * w > 0x7FFFFFFFll) return fail(EOGS_ERR_INVALID_ARG, "%s: more than 2^31 - 1 elements in a map", who);
  return EOGS_OK;
}

template <int R>
void launch_lookup(int N, int C, int h, int w, int levels, const RaftLevels& lt, const float* f1, const float* pyr, const float* coords,
                   float* out, double inv, int no_stage, hipStream_t s) {
  const unsigned tiles = (unsigned)(((w + LT_W - 1) / LT_W) * ((h + LT_H - 1) / LT_H));
  hipLaunchKernelGGL(raft_lookup_kernel<R>, dim3(tiles, levels, N), dim3(LNT), 0, s, C, h, w, levels, lt,
                     reinterpret_cast<const float4*>(f1), pyr, coords, out, inv, no_stage);
}

}  // namespace

extern "C" {

int eogs_raft_bytes(int N, int C, int h, int w, int levels, size_t* bytes) {
  clear_error();
  const int rc = raft_check_shape("raft_bytes", N, C, h, w, levels);
  if (rc != EOGS_OK) return rc;
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "raft_bytes: NULL argument");
  *bytes = raft_levels(N, C, h, w, levels).bytes;
  return EOGS_OK;
}

int eogs_raft_level_offset(int N, int C, int h, int w, int level, size_t* offset) {
  clear_error();
  const int rc = raft_check_shape("raft_level_offset", N, C, h, w, level + 1);
  if (rc != EOGS_OK) return rc;
  if (!offset) return fail(EOGS_ERR_INVALID_ARG, "raft_level_offset: NULL argument");
  *offset = (size_t)raft_levels(N, C, h, w, level + 1).off[level] * sizeof(float);
  return EOGS_OK;
}

int eogs_raft_pyramid(int N, int C, int h, int w, int levels, const float* fmap, void* pyramid, size_t pyramid_bytes, void* stream) {
  clear_error();
  const int rc = raft_check_shape("raft_pyramid", N, C, h, w, levels);
  if (rc != EOGS_OK) return rc;
  if (!fmap || !pyramid) return fail(EOGS_ERR_INVALID_ARG, "raft_pyramid: NULL argument");
  const RaftLevels lt = raft_levels(N, C, h, w, levels);
  if (pyramid_bytes < lt.bytes) return fail(EOGS_ERR_WORKSPACE, "raft_pyramid: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* base = reinterpret_cast<float*>(ws_base(pyramid));
  const int P = h * w;
  hipLaunchKernelGGL(raft_to_cl_kernel, dim3((P + 31) / 32, (C + 31) / 32, N), dim3(256), 0, s, C, P, fmap, base + lt.off[0]);
  for (int l = 1; l < levels; l++) {
    const int64_t total = (int64_t)N * lt.h[l] * lt.w[l] * (C / 4);
    const int blocks = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
    hipLaunchKernelGGL(raft_pool_kernel, dim3(blocks), dim3(256), 0, s, N, C / 4, lt.h[l - 1], lt.w[l - 1], lt.h[l], lt.w[l],
                       reinterpret_cast<const float4*>(base + lt.off[l - 1]), reinterpret_cast<float4*>(base + lt.off[l]));
  }
  LAUNCH_TRY(s, false, "raft_pyramid");
  return EOGS_OK;
}

int eogs_raft_lookup(int N, int C, int h, int w, int levels, int radius, const float* fmap1_cl, const void* pyramid,
                     const float* coords, float* out, unsigned flags, void* stream) {
  clear_error();
  const int rc = raft_check_shape("raft_lookup", N, C, h, w, levels);
  if (rc != EOGS_OK) return rc;
  if (radius < 1 || radius > EOGS_RAFT_MAX_RADIUS) return fail(EOGS_ERR_INVALID_ARG, "raft_lookup: radius must be 1 to 4");
  if (flags & ~EOGS_RAFT_NO_STAGE) return fail(EOGS_ERR_INVALID_ARG, "raft_lookup: unknown flags");
  if (!fmap1_cl || !pyramid || !coords || !out) return fail(EOGS_ERR_INVALID_ARG, "raft_lookup: NULL argument");
  const int K = 2 * radius + 1;
  if ((int64_t)N * levels * K * K * h * w > 0x7FFFFFFFll) return fail(EOGS_ERR_INVALID_ARG, "raft_lookup: more than 2^31 - 1 output elements");
  const float* f1 = reinterpret_cast<const float*>(ws_base(fmap1_cl));
  const float* pyr = reinterpret_cast<const float*>(ws_base(pyramid));
  if (!aligned16(coords) || !aligned16(out)) return fail(EOGS_ERR_INVALID_ARG, "raft_lookup: a pointer is not 16-byte aligned");
  const RaftLevels lt = raft_levels(N, C, h, w, levels);
  const double inv = 1.0 / sqrt((double)C);
  const int ns = (flags & EOGS_RAFT_NO_STAGE) ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  switch (radius) {
    case 1: launch_lookup<1>(N, C, h, w, levels, lt, f1, pyr, coords, out, inv, ns, s); break;
    case 2: launch_lookup<2>(N, C, h, w, levels, lt, f1, pyr, coords, out, inv, ns, s); break;
    case 3: launch_lookup<3>(N, C, h, w, levels, lt, f1, pyr, coords, out, inv, ns, s); break;
    default: launch_lookup<4>(N, C, h, w, levels, lt, f1, pyr, coords, out, inv, ns, s); break;
  }
  LAUNCH_TRY(s, false, "raft_lookup");
  return EOGS_OK;
}

int eogs_raft_stage_info(int* tile_w, int* tile_h, int* max_positions) {
  clear_error();
  if (!tile_w || !tile_h || !max_positions) return fail(EOGS_ERR_INVALID_ARG, "raft_stage_info: NULL argument");
  *tile_w = LT_W;
  *tile_h = LT_H;
  *max_positions = LMAXPOS;
  return EOGS_OK;
}

int eogs_raft_upsample(int N, int h, int w, int mode, const float* flow, const float* mask, float* out, void* stream) {
  clear_error();
  if (N < 1 || h < 1 || w < 1) return fail(EOGS_ERR_INVALID_ARG, "raft_upsample: bad sizes (N, h and w must be at least 1)");
  if (h > 8192 || w > 8192 || N > 65535) return fail(EOGS_ERR_INVALID_ARG, "raft_upsample: bad sizes (h and w at most 8192, N at most 65535)");
  if (mode != EOGS_RAFT_UP_CONVEX && mode != EOGS_RAFT_UP_BILINEAR) return fail(EOGS_ERR_INVALID_ARG, "raft_upsample: unknown mode");
  if (!flow || !out) return fail(EOGS_ERR_INVALID_ARG, "raft_upsample: NULL argument");
  if ((mode == EOGS_RAFT_UP_CONVEX) != (mask != nullptr))
    return fail(EOGS_ERR_INVALID_ARG, "raft_upsample: the convex mode takes a mask, the bilinear mode none");
  if (!aligned16(out)) return fail(EOGS_ERR_INVALID_ARG, "raft_upsample: a pointer is not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)N * h * 8 * w;
  const int blocks = (int)((total + UNT - 1) / UNT > 4096 ? 4096 : (total + UNT - 1) / UNT);
  if (mode == EOGS_RAFT_UP_CONVEX)
    hipLaunchKernelGGL(raft_upsample_kernel<EOGS_RAFT_UP_CONVEX>, dim3(blocks), dim3(UNT), 0, s, N, h, w, flow, mask, out);
  else
    hipLaunchKernelGGL(raft_upsample_kernel<EOGS_RAFT_UP_BILINEAR>, dim3(blocks), dim3(UNT), 0, s, N, h, w, flow, mask, out);
  LAUNCH_TRY(s, false, "raft_upsample");
  return EOGS_OK;
}

}  // extern "C"
