// flowenc.hip — RAFT-small's two encoders (include/eogs_resample.h, eogs_flowenc_*): flownet.hip's channel-last implicit-GEMM
// convolution on v_mfma_f32_16x16x4_f32 with a stride of 1 or 2, the producer's instance norm and ReLU applied while the
// input is staged, the bottleneck's residual tail as an epilogue and the map's statistics as double-precision partials of the
// two-stage sum (reduce.h); the kernel that turns the partials into (mean, rstd); the pointwise pass that closes a
// normalised block; and the encoders composed of them, one call each.
//
// The convolution keeps flownet.hip's tile (FT_W x FT_H OUTPUT positions, four waves of two rows, NB <= 3 blocks of 16 output
// channels), its chunks of FCK = 8 input channels, its packed weights and its sum order: chunks in order, per chunk the taps
// row-major, per tap the channels ascending. What differs is the staged window. A k x k convolution of stride s reads
// (FT_H - 1) s + k rows of (FT_W - 1) s + k columns; under stride 2 the columns of a staged row are stored by parity, the even
// ones first, so that the 16 positions of a matrix row, which lie two columns apart, are again 16 neighbouring floats and
// the A operand stays one conflict-free ds_read_b32. A 1 x 1 convolution stages only the positions it reads.
#include "flownet_conv.h"
#include "reduce.h"

namespace {

static_assert(FNT % FCK == 0, "channel-last, a thread stages one channel of a chunk");
constexpr bool fe_split(int k, int s) { return s == 2 && k > 1; }                          // columns stored by parity
constexpr int fe_hh(int k, int s) { return k == 1 ? FT_H : (FT_H - 1) * s + k; }            // staged rows
constexpr int fe_hw(int k, int s) { return k == 1 ? FT_W : (FT_W - 1) * s + k; }            // staged columns
constexpr int fe_half(int k, int s) { return (fe_hw(k, s) + 1) / 2; }                       // columns of one parity
constexpr int fe_pitch(int k, int s) { return fe_split(k, s) ? 2 * fe_half(k, s) : fe_hw(k, s); }
constexpr int fe_ps(int k, int s) { return (fe_hh(k, s) * fe_pitch(k, s) - 16 + 63) / 64 * 64 + 16; }  // plane stride, 16 mod 64

struct EncConvArgs {
  const float* in;
  const float* in_norm;  // (mean, rstd) per (image, input channel), or NULL
  int C, h, w, ho, wo, cout, epi;
  unsigned flags;
  const float* wp;
  const float* bias;
  const float* res;
  float* out;
  double* partials;  // [N][tiles][cout][2], or NULL
};

template <int NB, int K, int S>
__global__ __launch_bounds__(FNT) void flowenc_conv_kernel(EncConvArgs a) {
  constexpr int WS = fn_ws(NB), PAD = (K - 1) / 2, HH = fe_hh(K, S), HW = fe_hw(K, S), HALF = fe_half(K, S), PITCH = fe_pitch(K, S),
                NPOS = HH * HW, PS = fe_ps(K, S), TAPS = K * K, TG = fn_tg(K);
  constexpr bool SPLIT = fe_split(K, S);
  constexpr int STEP = K == 1 ? S : 1;  // input positions between two staged ones
  __shared__ float s_in[FCK * PS];
  __shared__ __attribute__((aligned(16))) float s_w[TG * FCK * WS];
  __shared__ double s_stat[4][NB * 16][2];
  const int h = a.h, w = a.w, ho = a.ho, wo = a.wo, C = a.C;
  const int tiles_x = (wo + FT_W - 1) / FT_W;
  const int tx0 = (int)(blockIdx.x % tiles_x) * FT_W, ty0 = (int)(blockIdx.x / tiles_x) * FT_H;
  const int iy0 = ty0 * S - (K == 1 ? 0 : PAD), ix0 = tx0 * S - (K == 1 ? 0 : PAD);  // the window's first input position
  const int cc = blockIdx.y, chunks = gridDim.y, n = blockIdx.z;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, m = lane & 15;
  const bool nchw = a.flags & EOGS_FLOWENC_IN_NCHW;

  f32x4 acc[2][NB];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NB; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // The loads of a stage are issued into registers while the stage before is multiplied, and stored to LDS after it.
  constexpr int NI = (FCK * NPOS + FNT - 1) / FNT, NW = (TG * FCK * WS / 4 + FNT - 1) / FNT, NG = TAPS / TG;
  float rin[NI];
  f32x4 rw[NW];
  auto load_in = [&](int c0) {
    const int creal = C - c0 < FCK ? C - c0 : FCK;
    const float* __restrict__ in = a.in;
    // channel-last, a thread stages ONE channel of the chunk (FNT is a multiple of FCK): its (mean, rstd) is read once
    float mean = 0.f, rstd = 0.f;
    if (a.in_norm && !nchw && (int)(threadIdx.x & (FCK - 1)) < creal) {
      const float* __restrict__ t = a.in_norm + ((int64_t)n * C + c0 + (threadIdx.x & (FCK - 1))) * 2;
      mean = t[0];
      rstd = t[1];
    }
#pragma unroll
    for (int j = 0; j < NI; j++) {
      const int i = threadIdx.x + j * FNT;
      int c, p;
      if (nchw) { c = i / NPOS; p = i - c * NPOS; } else { c = i & (FCK - 1); p = i / FCK; }
      const int py = p / HW, yy = iy0 + py * STEP, xx = ix0 + (p - py * HW) * STEP;
      float v = 0.f;
      if (i < FCK * NPOS && c < creal && yy >= 0 && yy < h && xx >= 0 && xx < w) {
        v = nchw ? in[(((int64_t)n * C + c0 + c) * h + yy) * w + xx] : in[(((int64_t)n * h + yy) * w + xx) * C + c0 + c];
        if (a.in_norm) {  // the producer's instance norm and ReLU: two roundings and a select that keeps a NaN
          if (nchw) {
            const float* __restrict__ t = a.in_norm + ((int64_t)n * C + c0 + c) * 2;
            mean = t[0];
            rstd = t[1];
          }
          const float d = v - mean;
          const float u = d * rstd;
          v = u < 0.f ? 0.f : u;
        }
      }
      rin[j] = v;
    }
  };
  auto load_w = [&](int q, int grp) {
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(a.wp + (((int64_t)q * chunks + cc) * TAPS + grp * TG) * (FCK * WS));
#pragma unroll
    for (int j = 0; j < NW; j++) {
      const int i = threadIdx.x + j * FNT;
      rw[j] = i < TG * FCK * WS / 4 ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  const int nq = (C + FCK - 1) / FCK;
  load_in(0);
  load_w(0, 0);
  for (int q = 0; q < nq; q++) {
    const int c0 = q * FCK, creal = C - c0 < FCK ? C - c0 : FCK;
    __syncthreads();  // the chunk before has been read
#pragma unroll
    for (int j = 0; j < NI; j++) {
      const int i = threadIdx.x + j * FNT;
      int c, p;
      if (nchw) { c = i / NPOS; p = i - c * NPOS; } else { c = i & (FCK - 1); p = i / FCK; }
      const int py = p / HW, px = p - py * HW;
      if (i < FCK * NPOS) s_in[c * PS + py * PITCH + (SPLIT ? (px & 1) * HALF + (px >> 1) : px)] = rin[j];
    }
    for (int grp = 0; grp < NG; grp++) {
      if (grp) __syncthreads();  // the taps before have been read
#pragma unroll
      for (int j = 0; j < NW; j++) {
        const int i = threadIdx.x + j * FNT;
        if (i < TG * FCK * WS / 4) reinterpret_cast<f32x4*>(s_w)[i] = rw[j];
      }
      __syncthreads();
      if (grp + 1 < NG) {
        load_w(q, grp + 1);
      } else if (q + 1 < nq) {
        load_in(c0 + FCK);
        load_w(q + 1, 0);
      }
      // tile row r, tap (ky, kx): staged row r s + ky, staged column m s + kx (K == 1: row r, column m)
      constexpr int RS = K == 1 ? 1 : S;
      const float* ai = s_in + g * PS + (2 * wv) * RS * PITCH + m;
      const float* bi = s_w + g * WS + m;
#pragma unroll
      for (int t = 0; t < TG; t++) {
        const int tap = grp * TG + t, ky = tap / K, kx = tap - ky * K;
        const int off = ky * PITCH + (SPLIT ? (kx & 1) * HALF + (kx >> 1) : kx);
#pragma unroll
        for (int kk = 0; kk < FCK / 4; kk++) {
          if (kk * 4 < creal) {  // (a chunk's last instruction is skipped when its four channel lanes are all padding)
            const float a0 = ai[kk * 4 * PS + off], a1 = ai[kk * 4 * PS + RS * PITCH + off];
#pragma unroll
            for (int nb = 0; nb < NB; nb++) {
              const float b = bi[(t * FCK + kk * 4) * WS + nb * 16];
              acc[0][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][nb], 0, 0, 0);
              acc[1][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][nb], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // epilogue: lane (g, m) holds column m of rows 4 g .. 4 g + 3 of each 16 x 16 block
  const int cout = a.cout;
  const bool stats = a.partials != nullptr;  // (uniform over the workgroup)
  double st[NB][2];
#pragma unroll
  for (int nb = 0; nb < NB; nb++) st[nb][0] = st[nb][1] = 0.0;
#pragma unroll
  for (int mb = 0; mb < 2; mb++) {
    const int y = ty0 + 2 * wv + mb;
    if (y >= ho) continue;
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
      const int c = (cc * NB + nb) * 16 + m;
      if (c >= cout) continue;
      const float bias = a.bias ? a.bias[c] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int x = tx0 + g * 4 + r;
        if (x >= wo) continue;
        const int64_t pos = ((int64_t)n * ho + y) * wo + x;
        float v = acc[mb][nb][r];
        if (a.bias) v += bias;
        if (a.epi != EOGS_FLOWENC_EPI_BIAS) v = v < 0.f ? 0.f : v;  // (a NaN stays a NaN)
        if (a.epi == EOGS_FLOWENC_EPI_RESIDUAL) {
          v = a.res[pos * cout + c] + v;
          v = v < 0.f ? 0.f : v;
        }
        if (a.flags & EOGS_FLOWENC_OUT_NCHW) a.out[(((int64_t)n * cout + c) * ho + y) * wo + x] = v;
        else a.out[pos * cout + c] = v;
        if (stats) {  // rows ascending, per row the four positions ascending
          st[nb][0] += (double)v;
          st[nb][1] += (double)v * (double)v;
        }
      }
    }
  }
  if (stats) {
    // the four position groups of a channel by the butterfly's last two steps, then the four waves left to right
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        double v = st[nb][j];
        v += __shfl_xor(v, 32, 64);
        v += __shfl_xor(v, 16, 64);
        if (g == 0) s_stat[wv][nb * 16 + m][j] = v;
      }
    __syncthreads();
    if (threadIdx.x < NB * 16 * 2) {
      const int col = threadIdx.x >> 1, j = threadIdx.x & 1, c = cc * NB * 16 + col;
      if (c < cout)
        a.partials[(((int64_t)n * gridDim.x + blockIdx.x) * cout + c) * 2 + j] =
            ((s_stat[0][col][j] + s_stat[1][col][j]) + s_stat[2][col][j]) + s_stat[3][col][j];
    }
  }
}

// stage 2 of the two-stage sum over a convolution's partials: one workgroup per (channel, image)
__global__ __launch_bounds__(256) void flowenc_norm_kernel(int C, int rows, double count, const double* __restrict__ partials,
                                                           float* __restrict__ out) {
  __shared__ double s_red[4];
  const int c = blockIdx.x, n = blockIdx.y;
  double tot[2];
  column_sums<256>(partials + ((size_t)n * rows * C + c) * 2, rows, (size_t)C * 2, tot, s_red);
  if (threadIdx.x == 0) {
    const double mean = tot[0] / count;
    const double t = tot[1] / count - mean * mean;
    const double var = t < 0.0 ? 0.0 : t;  // (a NaN stays a NaN)
    out[((size_t)n * C + c) * 2] = (float)mean;
    out[((size_t)n * C + c) * 2 + 1] = (float)(1.0 / sqrt(var + 1e-5));
  }
}

// out = relu(S + relu((v - mean_v) rstd_v)), four channels of one position per thread
__global__ __launch_bounds__(256) void flowenc_finish_kernel(int64_t quads, int C, int64_t per_image, int shortcut,
                                                             const float* __restrict__ v, const float* __restrict__ norm_v,
                                                             const float* __restrict__ s, const float* __restrict__ norm_s,
                                                             float* __restrict__ out) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    const int64_t e = q * 4;
    const int c = (int)(e % C);
    const int64_t n = e / per_image;
    const f32x4 x = *reinterpret_cast<const f32x4*>(v + e);
    f32x4 sc{0.f, 0.f, 0.f, 0.f}, o;
    if (shortcut != EOGS_FLOWENC_SHORTCUT_NONE) sc = *reinterpret_cast<const f32x4*>(s + e);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float* __restrict__ tv = norm_v + (n * C + c + j) * 2;
      const float d = x[j] - tv[0];
      const float u = d * tv[1];
      float y = u < 0.f ? 0.f : u;  // (a NaN stays a NaN)
      if (shortcut != EOGS_FLOWENC_SHORTCUT_NONE) {
        float sh = sc[j];
        if (shortcut == EOGS_FLOWENC_SHORTCUT_NORM) {
          const float* __restrict__ ts = norm_s + (n * C + c + j) * 2;
          const float ds = sh - ts[0];
          sh = ds * ts[1];
        }
        y = sh + y;
        y = y < 0.f ? 0.f : y;
      }
      o[j] = y;
    }
    *reinterpret_cast<f32x4*>(out + e) = o;
  }
}

inline int64_t tiles_of(int h, int w) { return (int64_t)((w + FT_W - 1) / FT_W) * ((h + FT_H - 1) / FT_H); }

template <int NB, int K>
void launch_enc_s(int stride, dim3 grid, hipStream_t s, const EncConvArgs& a) {
  if (stride == 1) hipLaunchKernelGGL((flowenc_conv_kernel<NB, K, 1>), grid, dim3(FNT), 0, s, a);
  else hipLaunchKernelGGL((flowenc_conv_kernel<NB, K, 2>), grid, dim3(FNT), 0, s, a);
}

template <int NB>
void launch_enc_k(int k, int stride, dim3 grid, hipStream_t s, const EncConvArgs& a) {
  switch (k) {
    case 1: launch_enc_s<NB, 1>(stride, grid, s, a); break;
    case 3: launch_enc_s<NB, 3>(stride, grid, s, a); break;
    default: launch_enc_s<NB, 7>(stride, grid, s, a); break;
  }
}

int check_map(const char* who, int N, int h, int w, int c) {
  if (N < 1 || h < 1 || w < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (N, h and w must be at least 1)", who);
  if (c < 1 || c > 4096) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (a map has 1 to 4096 channels)", who);
  if (N > 65535) return fail(EOGS_ERR_INVALID_ARG, "%s: N above 65535", who);
  if ((int64_t)N * h * w * c > 0x7FFFFFFFll) return fail(EOGS_ERR_INVALID_ARG, "%s: more than 2^31 - 1 elements in a map", who);
  return EOGS_OK;
}

// every argument checked, then one launch (no launch check: the caller's LAUNCH_TRY covers a group)
int enc_conv_checked(const char* who, int N, int h, int w, int cin, int cout, int k, int stride, const float* in, const float* in_norm,
                     const void* packed, size_t packed_bytes, const float* bias, const float* res, float* out, double* partials,
                     size_t partials_bytes, int epi, unsigned flags, hipStream_t s) {
  if (k != 1 && k != 3 && k != 7) return fail(EOGS_ERR_INVALID_ARG, "%s: the kernel size is 1, 3 or 7", who);
  if (stride != 1 && stride != 2) return fail(EOGS_ERR_INVALID_ARG, "%s: the stride is 1 or 2", who);
  RC_TRY(check_map(who, N, h, w, cin));
  const int ho = (h + stride - 1) / stride, wo = (w + stride - 1) / stride;
  RC_TRY(check_map(who, N, ho, wo, cout));
  if (epi < EOGS_FLOWENC_EPI_BIAS || epi > EOGS_FLOWENC_EPI_RESIDUAL) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown epilogue", who);
  if (flags & ~(EOGS_FLOWENC_IN_NCHW | EOGS_FLOWENC_OUT_NCHW)) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown flags", who);
  if ((flags & EOGS_FLOWENC_OUT_NCHW) && epi != EOGS_FLOWENC_EPI_BIAS) return fail(EOGS_ERR_INVALID_ARG, "%s: OUT_NCHW goes with the BIAS epilogue only", who);
  if (partials && epi != EOGS_FLOWENC_EPI_BIAS) return fail(EOGS_ERR_INVALID_ARG, "%s: statistics go with the BIAS epilogue only", who);
  if ((epi == EOGS_FLOWENC_EPI_RESIDUAL) != (res != nullptr)) return fail(EOGS_ERR_INVALID_ARG, "%s: the RESIDUAL epilogue takes res, the others none", who);
  if (!in || !packed || !out) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(in) || !aligned16(in_norm) || !aligned16(packed) || !aligned16(bias) || !aligned16(res) || !aligned16(out) || !aligned16(partials))
    return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const ConvPlan pl = conv_plan(k, 1, &cin, cout);
  if (packed_bytes < pl.floats * sizeof(float)) return fail(EOGS_ERR_WORKSPACE, "%s: packed weights too small", who);
  const int64_t tiles = tiles_of(ho, wo);
  if (partials && partials_bytes < (size_t)N * tiles * cout * 2 * sizeof(double)) return fail(EOGS_ERR_WORKSPACE, "%s: partials too small", who);
  EncConvArgs a{};
  a.in = in; a.in_norm = in_norm; a.C = cin; a.h = h; a.w = w; a.ho = ho; a.wo = wo; a.cout = cout; a.epi = epi; a.flags = flags;
  a.wp = reinterpret_cast<const float*>(packed); a.bias = bias; a.res = res; a.out = out; a.partials = partials;
  const dim3 grid((unsigned)tiles, (unsigned)pl.chunks, (unsigned)N);
  switch (pl.nb) {
    case 1: launch_enc_k<1>(k, stride, grid, s, a); break;
    case 2: launch_enc_k<2>(k, stride, grid, s, a); break;
    default: launch_enc_k<3>(k, stride, grid, s, a); break;
  }
  return EOGS_OK;
}

int norm_checked(const char* who, int N, int h, int w, int C, const double* partials, size_t partials_bytes, float* norm, hipStream_t s) {
  RC_TRY(check_map(who, N, h, w, C));
  if (!partials || !norm) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(partials) || !aligned16(norm)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const int64_t tiles = tiles_of(h, w);
  if (partials_bytes < (size_t)N * tiles * C * 2 * sizeof(double)) return fail(EOGS_ERR_WORKSPACE, "%s: partials too small", who);
  hipLaunchKernelGGL(flowenc_norm_kernel, dim3((unsigned)C, (unsigned)N), dim3(256), 0, s, C, (int)tiles, (double)h * (double)w, partials, norm);
  return EOGS_OK;
}

int finish_checked(const char* who, int N, int h, int w, int C, const float* v, const float* norm_v, const float* sc, const float* norm_s,
                   int shortcut, float* out, hipStream_t s) {
  RC_TRY(check_map(who, N, h, w, C));
  if (C % 4) return fail(EOGS_ERR_INVALID_ARG, "%s: the channel count is a multiple of 4", who);
  if (shortcut < EOGS_FLOWENC_SHORTCUT_NONE || shortcut > EOGS_FLOWENC_SHORTCUT_NORM) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown shortcut", who);
  if ((shortcut != EOGS_FLOWENC_SHORTCUT_NONE) != (sc != nullptr) || (shortcut == EOGS_FLOWENC_SHORTCUT_NORM) != (norm_s != nullptr))
    return fail(EOGS_ERR_INVALID_ARG, "%s: PLAIN takes s, NORM takes s and norm_s, NONE neither", who);
  if (!v || !norm_v || !out) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(v) || !aligned16(norm_v) || !aligned16(sc) || !aligned16(norm_s) || !aligned16(out))
    return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const int64_t quads = (int64_t)N * h * w * C / 4;
  hipLaunchKernelGGL(flowenc_finish_kernel, dim3(capped_blocks(quads, 256, 8192)), dim3(256), 0, s, quads, C, (int64_t)h * w * C, shortcut, v,
                     norm_v, sc, norm_s, out);
  return EOGS_OK;
}

// ---- RAFT-large's batch norms (eogs_flowres_fold) ----

// a batch norm in eval mode folded into its convolution: one workgroup per output channel, every thread forms the same s
__global__ __launch_bounds__(256) void flowres_fold_kernel(int per_out, const float* __restrict__ w, const float* __restrict__ b,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ mean, const float* __restrict__ var, double eps,
                                                           float* __restrict__ w_out, float* __restrict__ b_out) {
  const int c = blockIdx.x;
  const float s = (float)((double)gamma[c] / sqrt((double)var[c] + eps));  // (a negative var: NaN)
  const float* __restrict__ src = w + (int64_t)c * per_out;
  float* __restrict__ dst = w_out + (int64_t)c * per_out;
  for (int i = threadIdx.x; i < per_out; i += 256) dst[i] = src[i] * s;
  if (threadIdx.x == 0) b_out[c] = (float)(((double)b[c] - (double)mean[c]) * (double)s + (double)beta[c]);
}

int fold_checked(const char* who, int cout, int per_out, const float* w, const float* b, const float* gamma, const float* beta,
                 const float* mean, const float* var, double eps, float* w_out, float* b_out, hipStream_t s) {
  if (cout < 1 || per_out < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (cout and per_out must be at least 1)", who);
  if (cout > 4096) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (a convolution has 1 to 4096 output channels)", who);
  if ((int64_t)cout * per_out > 0x7FFFFFFFll) return fail(EOGS_ERR_INVALID_ARG, "%s: more than 2^31 - 1 weights", who);
  if (!w || !b || !gamma || !beta || !mean || !var || !w_out || !b_out) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(w) || !aligned16(b) || !aligned16(gamma) || !aligned16(beta) || !aligned16(mean) || !aligned16(var) || !aligned16(w_out) ||
      !aligned16(b_out))
    return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  hipLaunchKernelGGL(flowres_fold_kernel, dim3((unsigned)cout), dim3(256), 0, s, per_out, w, b, gamma, beta, mean, var, eps, w_out, b_out);
  return EOGS_OK;
}

// ---- the encoders: RAFT-small's (eogs_flowenc_run) and RAFT-large's (eogs_flowres_run) ----

// An encoder, stated once: a 7 x 7 stem at stride 2, three layers of two blocks (the first block of layers 2 and 3 halves the
// map, at its convolution `strided`, and carries a 1 x 1 downsample), a 1 x 1 head. A block is `nblock` convolutions of
// kernel sizes bk, with cout / mid_div channels between them: RAFT-small's 1-3-1 bottleneck, RAFT-large's 3-3 residual block.
// FEATURE normalises every map but the head's by instance; CONTEXT has no norm, or (fold) eval-mode batch norms folded first.
struct EncDesc {
  int width[4];  // the stem's and the three layers' channels
  int head[2];   // the head's, by kind
  int nblock, bk[3], mid_div, strided;
  bool fold;
};
constexpr EncDesc E_SMALL = {{32, 32, 64, 96}, {128, 160}, 3, {1, 3, 1}, 4, 1, false};
constexpr EncDesc E_LARGE = {{64, 64, 96, 128}, {256, 256}, 2, {3, 3, 0}, 1, 0, true};
static_assert(EOGS_FLOWENC_FEATURE == 0 && EOGS_FLOWENC_CONTEXT == 1, "head[] is indexed by the kind");
constexpr int enc_convs(const EncDesc& d) { return 1 + 6 * d.nblock + 2 + 1; }  // stem, blocks, two downsamples, head
constexpr int E_MAX = enc_convs(E_SMALL);
static_assert(2 * enc_convs(E_SMALL) == EOGS_FLOWENC_PARAMS && 2 * enc_convs(E_LARGE) == EOGS_FLOWRES_PARAMS && enc_convs(E_LARGE) <= E_MAX,
              "a description reads exactly the params table of its entry");
static_assert(4 * (enc_convs(E_LARGE) - 1) == EOGS_FLOWRES_BN, "every convolution but the head has a norm");

struct EConv { int cin, cout, k, s; };

struct EncPlan {
  EConv conv[E_MAX];
  int nconv;
  int h[4], w[4];  // the image, then the maps after the stem, layer2 and layer3
  float* pw[E_MAX];
  size_t pw_bytes[E_MAX];
  float *fw[E_MAX], *fb[E_MAX];  // fold: the folded weights and biases
  float *x, *y, *r[3], *rd, *tab[4];  // the blocks' ping-pong; block convolution j's map and (mean, rstd) table; the downsample's (tab[nblock])
  double* partials;
  size_t partials_bytes, bytes;
};

inline EncPlan enc_plan(const EncDesc& d, void* ws, int N, int H, int W, int kind) {
  EncPlan p{};
  const bool normed = kind == EOGS_FLOWENC_FEATURE;
  const int n = d.nblock;
  p.h[0] = H; p.w[0] = W;
  for (int i = 1; i < 4; i++) { p.h[i] = (p.h[i - 1] + 1) / 2; p.w[i] = (p.w[i - 1] + 1) / 2; }
  // The table, in the order eogs_*_run walks it, and with it each scratch buffer's size: the largest map any convolution
  // (or, for x and y, any block's tail) writes into it. `dst`: that buffer's size; none for the head, which writes `out`.
  size_t xy = 0, r[3] = {}, rd = 0, rows = 0;  // floats; rows: of (tile, channel) partial sums per image
  int widest = 0;                               // normalised map, in channels
  auto grow = [](size_t& a, size_t b) { if (b > a) a = b; };
  auto put = [&](int cin, int cout, int k, int s, int lv, size_t* dst) {
    p.conv[p.nconv++] = {cin, cout, k, s};
    const int lo = lv + (s == 2);
    if (!dst) return;
    grow(*dst, (size_t)N * p.h[lo] * p.w[lo] * cout);
    grow(rows, (size_t)tiles_of(p.h[lo], p.w[lo]) * cout);
    if (cout > widest) widest = cout;
  };
  put(3, d.width[0], 7, 2, 0, normed ? &r[n - 1] : &xy);
  grow(xy, (size_t)N * p.h[1] * p.w[1] * d.width[0]);
  int lv = 1;
  for (int b = 0; b < 6; b++) {
    const int L = b / 2, first = b % 2 == 0, cin = first ? d.width[L] : d.width[L + 1], cout = d.width[L + 1], s = first && L > 0 ? 2 : 1;
    const int mid = cout / d.mid_div, lo = lv + (s == 2);
    for (int j = 0; j < n; j++)  // (without a norm the last convolution closes the block itself, into y)
      put(j ? mid : cin, j < n - 1 ? mid : cout, d.bk[j], j == d.strided ? s : 1, j <= d.strided ? lv : lo, !normed && j == n - 1 ? &xy : &r[j]);
    if (s == 2) put(cin, cout, 1, 2, lv, &rd);
    grow(xy, (size_t)N * p.h[lo] * p.w[lo] * cout);
    lv = lo;
  }
  put(d.width[3], d.head[kind], 1, 1, 3, nullptr);
  char* base = ws ? ws_base(ws) : nullptr;
  size_t o = 0;
  for (int j = 0; j < p.nconv; j++) {
    const EConv& c = p.conv[j];
    const size_t floats = conv_plan(c.k, 1, &c.cin, c.cout).floats;
    p.pw_bytes[j] = floats * sizeof(float);
    o = ws_carve(base, o, p.pw[j], floats);
    if (d.fold && !normed && j < p.nconv - 1) {
      o = ws_carve(base, o, p.fw[j], (size_t)c.cout * c.cin * c.k * c.k);
      o = ws_carve(base, o, p.fb[j], (size_t)c.cout);
    }
  }
  o = ws_carve(base, o, p.x, xy);
  o = ws_carve(base, o, p.y, xy);
  for (int j = 0; j < n - 1 + normed; j++) o = ws_carve(base, o, p.r[j], r[j]);
  o = ws_carve(base, o, p.rd, rd);
  if (normed) {  // every table the same size, the widest map's
    for (int j = 0; j <= n; j++) o = ws_carve(base, o, p.tab[j], (size_t)N * widest * 2);
    p.partials_bytes = (size_t)N * rows * 2 * sizeof(double);
    o = ws_carve(base, o, p.partials, p.partials_bytes / sizeof(double));
  }
  p.bytes = ws_align(o) + 256;
  return p;
}

int check_enc_shape(const char* who, const EncDesc& d, int N, int H, int W, int kind) {
  if (kind != EOGS_FLOWENC_FEATURE && kind != EOGS_FLOWENC_CONTEXT) return fail(EOGS_ERR_INVALID_ARG, "%s: the kind is FEATURE or CONTEXT", who);
  if (N < 1 || H < 1 || W < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (N, H and W must be at least 1)", who);
  if (N > 65535) return fail(EOGS_ERR_INVALID_ARG, "%s: N above 65535", who);
  const int64_t h1 = (H + 1) / 2, w1 = (W + 1) / 2, h2 = (h1 + 1) / 2, w2 = (w1 + 1) / 2, h3 = (h2 + 1) / 2, w3 = (w2 + 1) / 2;
  const int head = d.head[0] > d.head[1] ? d.head[0] : d.head[1];  // (one bound for both kinds)
  if ((int64_t)N * 3 * H * W > 0x7FFFFFFFll || (int64_t)N * h1 * w1 * d.width[1] > 0x7FFFFFFFll || (int64_t)N * h2 * w2 * d.width[2] > 0x7FFFFFFFll ||
      (int64_t)N * h3 * w3 * head > 0x7FFFFFFFll)
    return fail(EOGS_ERR_INVALID_ARG, "%s: more than 2^31 - 1 elements in a map", who);
  if (kind == EOGS_FLOWENC_FEATURE && h3 * w3 == 1)
    return fail(EOGS_ERR_INVALID_ARG, "%s: the feature encoder's last map is a single position, which an instance norm cannot normalise", who);
  return EOGS_OK;
}

int enc_bytes(const char* who, const EncDesc& d, int N, int H, int W, int kind, size_t* bytes) {
  RC_TRY(check_enc_shape(who, d, N, H, W, kind));
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  *bytes = enc_plan(d, nullptr, N, H, W, kind).bytes;
  return EOGS_OK;
}

// `bn`: the batch norms of a `fold` description's CONTEXT kind, NULL otherwise
int enc_run(const char* who, const EncDesc& d, int N, int H, int W, int kind, const float* const* params, const float* const* bn,
            const float* image, void* ws, size_t ws_bytes, float* out, hipStream_t s) {
  RC_TRY(check_enc_shape(who, d, N, H, W, kind));
  const bool normed = kind == EOGS_FLOWENC_FEATURE, fold = d.fold && !normed;
  const int n = d.nblock, nconv = enc_convs(d);
  if (d.fold && normed && bn) return fail(EOGS_ERR_INVALID_ARG, "%s: bn goes with CONTEXT only (FEATURE normalises by instance)", who);
  if (fold && !bn) return fail(EOGS_ERR_INVALID_ARG, "%s: CONTEXT takes bn, the batch norms of its convolutions", who);
  if (!params || !image || !ws || !out) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  for (int i = 0; i < 2 * nconv; i++) {
    if (!params[i]) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!aligned16(params[i])) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  }
  for (int i = 0; fold && i < 4 * (nconv - 1); i++) {
    if (!bn[i]) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!aligned16(bn[i])) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  }
  if (!aligned16(image) || !aligned16(out)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const EncPlan p = enc_plan(d, ws, N, H, W, kind);
  if (ws_bytes < p.bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  const int BIAS = EOGS_FLOWENC_EPI_BIAS, RELU = EOGS_FLOWENC_EPI_RELU, RESIDUAL = EOGS_FLOWENC_EPI_RESIDUAL;
  const float *wsrc[E_MAX], *bsrc[E_MAX];  // what a convolution multiplies by and adds: the parameters, or their fold
  for (int i = 0; i < nconv; i++) {
    const EConv& c = p.conv[i];
    wsrc[i] = params[2 * i];
    bsrc[i] = params[2 * i + 1];
    if (fold && i < nconv - 1) {
      RC_TRY(fold_checked(who, c.cout, c.cin * c.k * c.k, params[2 * i], params[2 * i + 1], bn[4 * i], bn[4 * i + 1], bn[4 * i + 2], bn[4 * i + 3],
                          1e-5, p.fw[i], p.fb[i], s));
      wsrc[i] = p.fw[i];
      bsrc[i] = p.fb[i];
    }
    RC_TRY(pack_checked(who, c.k, 1, &c.cin, nullptr, c.cin, c.cout, 0, c.cout, wsrc[i], p.pw[i], p.pw_bytes[i], s));
  }
  // one convolution of the table on an h x w map; with `tab` its statistics become that (mean, rstd) table
  auto conv = [&](int i, int h, int w, const float* in, const float* in_norm, const float* res, float* o, float* tab, int epi, unsigned flags) {
    const EConv& c = p.conv[i];
    RC_TRY(enc_conv_checked(who, N, h, w, c.cin, c.cout, c.k, c.s, in, in_norm, p.pw[i], p.pw_bytes[i], bsrc[i], res, o,
                            tab ? p.partials : nullptr, tab ? p.partials_bytes : 0, epi, flags, s));
    if (tab) RC_TRY(norm_checked(who, N, (h + c.s - 1) / c.s, (w + c.s - 1) / c.s, c.cout, p.partials, p.partials_bytes, tab, s));
    return (int)EOGS_OK;
  };
  int i = 0, lv = 1;
  float *x = p.x, *y = p.y;
  if (normed) {
    RC_TRY(conv(i++, H, W, image, nullptr, nullptr, p.r[n - 1], p.tab[n - 1], BIAS, EOGS_FLOWENC_IN_NCHW));
    RC_TRY(finish_checked(who, N, p.h[1], p.w[1], d.width[0], p.r[n - 1], p.tab[n - 1], nullptr, nullptr, EOGS_FLOWENC_SHORTCUT_NONE, x, s));
  } else {
    RC_TRY(conv(i++, H, W, image, nullptr, nullptr, x, nullptr, RELU, EOGS_FLOWENC_IN_NCHW));
  }
  for (int b = 0; b < 6; b++) {
    const bool down = p.conv[i + d.strided].s == 2;
    const int h = p.h[lv], w = p.w[lv], ho = down ? p.h[lv + 1] : h, wo = down ? p.w[lv + 1] : w, cout = p.conv[i + n - 1].cout;
    // the block's convolutions in turn, each reading the one before it (normalised: through its table); the map halves after `strided`
    const float *in = x, *in_tab = nullptr;
    for (int j = 0; j < n - 1 + normed; j++) {
      RC_TRY(conv(i + j, j <= d.strided ? h : ho, j <= d.strided ? w : wo, in, in_tab, nullptr, p.r[j], normed ? p.tab[j] : nullptr, normed ? BIAS : RELU, 0u));
      in = p.r[j];
      in_tab = normed ? p.tab[j] : nullptr;
    }
    if (down) RC_TRY(conv(i + n, h, w, x, nullptr, nullptr, p.rd, normed ? p.tab[n] : nullptr, BIAS, 0u));
    if (normed)
      RC_TRY(finish_checked(who, N, ho, wo, cout, in, in_tab, down ? p.rd : x, down ? p.tab[n] : nullptr,
                            down ? EOGS_FLOWENC_SHORTCUT_NORM : EOGS_FLOWENC_SHORTCUT_PLAIN, y, s));
    else  // the last convolution closes the block: relu(shortcut + relu(v))
      RC_TRY(conv(i + n - 1, ho, wo, in, nullptr, down ? p.rd : x, y, nullptr, RESIDUAL, 0u));
    i += n + down;
    if (down) lv++;
    float* t = x; x = y; y = t;
  }
  RC_TRY(conv(i, p.h[3], p.w[3], x, nullptr, nullptr, out, nullptr, BIAS, EOGS_FLOWENC_OUT_NCHW));
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
}

}  // namespace

extern "C" {

int eogs_flowres_fold(int cout, int per_out, const float* w, const float* b, const float* gamma, const float* beta, const float* mean,
                      const float* var, double eps, float* w_out, float* b_out, void* stream) {
  clear_error();
  hipStream_t s = (hipStream_t)stream;
  RC_TRY(fold_checked("flowres_fold", cout, per_out, w, b, gamma, beta, mean, var, eps, w_out, b_out, s));
  LAUNCH_TRY(s, false, "flowres_fold");
  return EOGS_OK;
}

int eogs_flowres_bytes(int N, int H, int W, int kind, size_t* bytes) {
  clear_error();
  return enc_bytes("flowres_bytes", E_LARGE, N, H, W, kind, bytes);
}

int eogs_flowres_run(int N, int H, int W, int kind, const float* const* params, const float* const* bn, const float* image, void* ws,
                     size_t ws_bytes, float* out, void* stream) {
  clear_error();
  return enc_run("flowres_run", E_LARGE, N, H, W, kind, params, bn, image, ws, ws_bytes, out, (hipStream_t)stream);
}

int eogs_flowenc_conv_partials(int N, int h, int w, int cout, int* rows, size_t* bytes) {
  clear_error();
  const char* who = "flowenc_conv_partials";
  RC_TRY(check_map(who, N, h, w, cout));
  if (!rows || !bytes) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  const int64_t tiles = tiles_of(h, w);
  *rows = (int)tiles;
  *bytes = (size_t)N * tiles * cout * 2 * sizeof(double);
  return EOGS_OK;
}

int eogs_flowenc_conv(int N, int h, int w, int cin, int cout, int k, int stride, const float* in, const float* in_norm,
                      const void* packed, size_t packed_bytes, const float* bias, const float* res, float* out, double* partials,
                      size_t partials_bytes, int epilogue, unsigned flags, void* stream) {
  clear_error();
  hipStream_t s = (hipStream_t)stream;
  RC_TRY(enc_conv_checked("flowenc_conv", N, h, w, cin, cout, k, stride, in, in_norm, packed, packed_bytes, bias, res, out, partials,
                          partials_bytes, epilogue, flags, s));
  LAUNCH_TRY(s, false, "flowenc_conv");
  return EOGS_OK;
}

int eogs_flowenc_norm(int N, int h, int w, int C, const double* partials, size_t partials_bytes, float* norm, void* stream) {
  clear_error();
  hipStream_t s = (hipStream_t)stream;
  RC_TRY(norm_checked("flowenc_norm", N, h, w, C, partials, partials_bytes, norm, s));
  LAUNCH_TRY(s, false, "flowenc_norm");
  return EOGS_OK;
}

int eogs_flowenc_finish(int N, int h, int w, int C, const float* v, const float* norm_v, const float* s, const float* norm_s,
                        int shortcut, float* out, void* stream) {
  clear_error();
  hipStream_t st = (hipStream_t)stream;
  RC_TRY(finish_checked("flowenc_finish", N, h, w, C, v, norm_v, s, norm_s, shortcut, out, st));
  LAUNCH_TRY(st, false, "flowenc_finish");
  return EOGS_OK;
}

int eogs_flowenc_bytes(int N, int H, int W, int kind, size_t* bytes) {
  clear_error();
  return enc_bytes("flowenc_bytes", E_SMALL, N, H, W, kind, bytes);
}

int eogs_flowenc_run(int N, int H, int W, int kind, const float* const* params, const float* image, void* ws, size_t ws_bytes,
                     float* out, void* stream) {
  clear_error();
  return enc_run("flowenc_run", E_SMALL, N, H, W, kind, params, nullptr, image, ws, ws_bytes, out, (hipStream_t)stream);
}

}  // extern "C"
