// flownet.hip — the convolutions of RAFT's update block (include/eogs_resample.h: eogs_flownet_*, eogs_flowrect_*, eogs_flowlarge_*):
// one channel-last stride-1 convolution on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32 over kh x kw taps (the
// squares 1, 3, 5, 7 and RAFT-large's 1 x 5 and 5 x 1), its epilogues, RAFT-small's update step composed of eight launches of
// it, and RAFT-large's of eleven with two more for its mask predictor.
//
// A convolution is an implicit GEMM: rows are positions, columns output channels, the sum runs over (segment, channel, tap).
// A workgroup of four waves owns FT_W x FT_H = 16 x 8 positions and NB <= 3 blocks of 16 output channels (grid.y walks the blocks of
// Cout, grid.z the batch). A wave owns two rows of the tile, 16 positions each, so it keeps 2 NB independent accumulators
// (the instruction's dependent latency is 40 cycles at a 32-cycle issue: two already reach the issue rate). Per chunk of
// FCK = 8 input channels the workgroup stages the tile's halo, (FT_H + kh - 1)(FT_W + kw - 1) positions, into LDS channel-planar
// with a plane stride of 16 mod 64 floats, and the chunk's packed weights tap by tap with a row stride of 16 or 48 mod 64:
// the A operand (lane l: position l & 15, channel l >> 4) and the B operand (lane l: channel l >> 4, column l & 15) are then
// one conflict-free ds_read_b32 each. Positions outside the map and channel lanes beyond a segment's count are staged as
// ZEROS, and the packed weights of those lanes are zeros too, so no lane ever multiplies uninitialised memory.
//
// The order of an output element's sum is fixed: segments in order, chunks of eight channels in order, taps in row-major
// order, four channels per instruction in ascending order; the instruction itself is a k-ordered fma chain. It does not
// depend on the tile, the batch index or NB: bitwise reproducible, and a batch gives the bits of its single images.
#include "flownet_conv.h"  // the tile, the chunk, the packing and its kernel: shared with flowenc.hip

namespace {

constexpr int fn_hp(int kh, int kw) { return (FT_H + kh - 1) * (FT_W + kw - 1); }
constexpr int fn_ps(int kh, int kw) { return (fn_hp(kh, kw) - 16 + 63) / 64 * 64 + 16; }  // plane stride: the least 16 mod 64 that holds the halo

struct ConvArgs {
  const float* in[EOGS_FLOWNET_MAX_SEGMENTS];
  int C[EOGS_FLOWNET_MAX_SEGMENTS];
  int nseg, h, w, cout, epi;
  unsigned flags;
  const float* wp;
  const float* bias;
  const float* add;
  const float* aux;
  float* out;
};

__device__ inline float fn_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

template <int NB, int KH, int KW>
__global__ __launch_bounds__(FNT) void flownet_conv_kernel(ConvArgs a) {
  constexpr int WS = fn_ws(NB), PADY = (KH - 1) / 2, PADX = (KW - 1) / 2, HW = FT_W + KW - 1, HP = fn_hp(KH, KW), PS = fn_ps(KH, KW),
                TAPS = KH * KW, TG = fn_tg(KH, KW);
  static_assert(TAPS % TG == 0, "a weight stage holds whole taps and the stages cover them");
  __shared__ float s_in[FCK * PS];
  __shared__ __attribute__((aligned(16))) float s_w[TG * FCK * WS];
  const int h = a.h, w = a.w;
  const int tiles_x = (w + FT_W - 1) / FT_W;
  const int tx0 = (int)(blockIdx.x % tiles_x) * FT_W, ty0 = (int)(blockIdx.x / tiles_x) * FT_H;
  const int cc = blockIdx.y, chunks = gridDim.y, n = blockIdx.z;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, m = lane & 15;

  f32x4 acc[2][NB];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NB; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // The loads of a stage are issued into registers while the stage before is multiplied, and stored to LDS after it.
  constexpr int NI = (FCK * HP + FNT - 1) / FNT, NW = (TG * FCK * WS / 4 + FNT - 1) / FNT, NG = TAPS / TG;
  float rin[NI];
  f32x4 rw[NW];
  auto load_in = [&](int s, int c0) {
    const int C = a.C[s], creal = C - c0 < FCK ? C - c0 : FCK;
    const float* __restrict__ in = a.in[s];
    const bool nchw = (a.flags >> s) & 1u;
#pragma unroll
    for (int j = 0; j < NI; j++) {
      const int i = threadIdx.x + j * FNT;
      int c, p;
      if (nchw) { c = i / HP; p = i - c * HP; } else { c = i & (FCK - 1); p = i / FCK; }
      const int py = p / HW, yy = ty0 - PADY + py, xx = tx0 - PADX + (p - py * HW);
      float v = 0.f;
      if (i < FCK * HP && c < creal && yy >= 0 && yy < h && xx >= 0 && xx < w)
        v = nchw ? in[(((int64_t)n * C + c0 + c) * h + yy) * w + xx] : in[(((int64_t)n * h + yy) * w + xx) * C + c0 + c];
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

  int s = 0, c0 = 0;
  load_in(0, 0);
  load_w(0, 0);
  for (int q = 0; s < a.nseg; q++) {
    const int C = a.C[s], creal = C - c0 < FCK ? C - c0 : FCK;
    int ns = s, nc0 = c0 + FCK;  // the chunk after this one
    if (nc0 >= C) { ns = s + 1; nc0 = 0; }
    __syncthreads();  // the chunk before has been read
#pragma unroll
    for (int j = 0; j < NI; j++) {
      const int i = threadIdx.x + j * FNT;
      int c, p;
      if ((a.flags >> s) & 1u) { c = i / HP; p = i - c * HP; } else { c = i & (FCK - 1); p = i / FCK; }
      if (i < FCK * HP) s_in[c * PS + p] = rin[j];
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
      } else if (ns < a.nseg) {
        load_in(ns, nc0);
        load_w(q + 1, 0);
      }
      const float* ai = s_in + g * PS + (2 * wv) * HW + m;
      const float* bi = s_w + g * WS + m;
#pragma unroll
      for (int t = 0; t < TG; t++) {
        const int tap = grp * TG + t, ky = tap / KW, kx = tap - ky * KW;
#pragma unroll
        for (int kk = 0; kk < FCK / 4; kk++) {
          if (kk * 4 < creal) {  // (a chunk's last instruction is skipped when its four channel lanes are all padding)
            const float a0 = ai[kk * 4 * PS + ky * HW + kx], a1 = ai[kk * 4 * PS + (ky + 1) * HW + kx];
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
    s = ns;
    c0 = nc0;
  }

  // epilogue: lane (g, m) holds column m of rows 4 g .. 4 g + 3 of each 16 x 16 block
  const int cout = a.cout, half = cout >> 1;
  const int64_t P = (int64_t)gridDim.z * h * w;
#pragma unroll
  for (int mb = 0; mb < 2; mb++) {
    const int y = ty0 + 2 * wv + mb;
    if (y >= h) continue;
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
      const int c = (cc * NB + nb) * 16 + m;
      if (c >= cout) continue;
      const float bias = a.bias ? a.bias[c] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int x = tx0 + g * 4 + r;
        if (x >= w) continue;
        const int64_t pos = ((int64_t)n * h + y) * w + x;
        float v = acc[mb][nb][r];
        if (a.bias) v += bias;
        if (a.add) v += a.add[pos * cout + c];
        if (a.epi == EOGS_FLOWNET_EPI_GATES) {
          if (c < half) a.out[pos * half + c] = fn_sigmoid(v);
          else a.out[(P + pos) * half + (c - half)] = fn_sigmoid(v) * a.aux[pos * half + (c - half)];
        } else if (a.epi == EOGS_FLOWNET_EPI_GRU) {
          const float z = a.aux[pos * cout + c], hh = a.out[pos * cout + c];
          a.out[pos * cout + c] = (1.0f - z) * hh + z * tanhf(v);
        } else {
          if (a.epi == EOGS_FLOWNET_EPI_RELU) v = v < 0.f ? 0.f : v;  // (a NaN stays a NaN)
          if (a.epi == EOGS_FLOWRECT_EPI_QUARTER) v = 0.25f * v;       // (exact: a power of two)
          if (a.flags & EOGS_FLOWNET_OUT_NCHW) a.out[(((int64_t)n * cout + c) * h + y) * w + x] = v;
          else a.out[pos * cout + c] = v;
        }
      }
    }
  }
}

// f32[N][C][P] -> f32[N][P][C]
__global__ __launch_bounds__(256) void flownet_to_cl_kernel(int64_t total, int C, int P, const float* __restrict__ in, float* __restrict__ out) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int c = (int)(idx % C);
    const int64_t np = idx / C;
    out[idx] = in[((np / P) * C + c) * P + np % P];
  }
}

__global__ __launch_bounds__(256) void flownet_copy_kernel(int n, const float* __restrict__ in, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = in[i];
}

// the six tap shapes (check_conv_shape has refused every other): 3 x 6 = 18 instantiations
template <int NB>
void launch_conv_k(int kh, int kw, dim3 grid, hipStream_t s, const ConvArgs& a) {
  switch (kh * 8 + kw) {
    case 1 * 8 + 1: hipLaunchKernelGGL((flownet_conv_kernel<NB, 1, 1>), grid, dim3(FNT), 0, s, a); break;
    case 3 * 8 + 3: hipLaunchKernelGGL((flownet_conv_kernel<NB, 3, 3>), grid, dim3(FNT), 0, s, a); break;
    case 5 * 8 + 5: hipLaunchKernelGGL((flownet_conv_kernel<NB, 5, 5>), grid, dim3(FNT), 0, s, a); break;
    case 1 * 8 + 5: hipLaunchKernelGGL((flownet_conv_kernel<NB, 1, 5>), grid, dim3(FNT), 0, s, a); break;
    case 5 * 8 + 1: hipLaunchKernelGGL((flownet_conv_kernel<NB, 5, 1>), grid, dim3(FNT), 0, s, a); break;
    default: hipLaunchKernelGGL((flownet_conv_kernel<NB, 7, 7>), grid, dim3(FNT), 0, s, a); break;
  }
}

// every argument checked, then one launch (no launch check: the caller's LAUNCH_TRY covers a group). `rect`: the
// eogs_flowrect_conv entry, which also takes 1 x 5 and 5 x 1 taps and the QUARTER epilogue
int conv_checked(const char* who, int N, int h, int w, int kh, int kw, bool rect, int nseg, const int* C, const float* const* in, int cout,
                 const void* packed, size_t packed_bytes, const float* bias, const float* add, const float* aux, float* out,
                 int epi, unsigned flags, hipStream_t s) {
  if (N < 1 || h < 1 || w < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (N, h and w must be at least 1)", who);
  const int rc = check_conv_shape(who, kh, kw, rect, nseg, C, cout);
  if (rc != EOGS_OK) return rc;
  if (N > 65535) return fail(EOGS_ERR_INVALID_ARG, "%s: N above 65535", who);
  int cmax = cout;
  for (int i = 0; i < nseg; i++) cmax = C[i] > cmax ? C[i] : cmax;
  if ((int64_t)N * h * w * cmax > 0x7FFFFFFFll) return fail(EOGS_ERR_INVALID_ARG, "%s: more than 2^31 - 1 elements in a map", who);
  if (epi < EOGS_FLOWNET_EPI_BIAS || epi > (rect ? EOGS_FLOWRECT_EPI_QUARTER : EOGS_FLOWNET_EPI_GRU))
    return fail(EOGS_ERR_INVALID_ARG, "%s: unknown epilogue", who);
  if (flags & ~((1u << nseg) - 1u) & ~EOGS_FLOWNET_OUT_NCHW) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown flags", who);
  const bool gated = epi == EOGS_FLOWNET_EPI_GATES || epi == EOGS_FLOWNET_EPI_GRU;
  if (gated && (flags & EOGS_FLOWNET_OUT_NCHW)) return fail(EOGS_ERR_INVALID_ARG, "%s: the gate epilogues write channel-last", who);
  if (epi == EOGS_FLOWNET_EPI_GATES && cout % 2) return fail(EOGS_ERR_INVALID_ARG, "%s: the gates epilogue takes an even Cout", who);
  if (gated != (aux != nullptr)) return fail(EOGS_ERR_INVALID_ARG, "%s: the gate epilogues take aux, the others none", who);
  if (!packed || !out) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  for (int i = 0; i < nseg; i++)
    if (!in[i]) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  for (int i = nseg; i < EOGS_FLOWNET_MAX_SEGMENTS; i++)
    if (in[i]) return fail(EOGS_ERR_INVALID_ARG, "%s: an input beyond the segment count", who);
  if (!aligned16(packed) || !aligned16(out) || !aligned16(bias) || !aligned16(add) || !aligned16(aux) || !aligned16(in[0]) ||
      !aligned16(in[1]) || !aligned16(in[2]))
    return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const ConvPlan pl = conv_plan(kh, kw, nseg, C, cout);
  if (packed_bytes < pl.floats * sizeof(float)) return fail(EOGS_ERR_WORKSPACE, "%s: packed weights too small", who);
  const int64_t tiles = (int64_t)((w + FT_W - 1) / FT_W) * ((h + FT_H - 1) / FT_H);
  ConvArgs a{};
  for (int i = 0; i < nseg; i++) { a.in[i] = in[i]; a.C[i] = C[i]; }
  a.nseg = nseg; a.h = h; a.w = w; a.cout = cout; a.epi = epi; a.flags = flags;
  a.wp = reinterpret_cast<const float*>(packed); a.bias = bias; a.add = add; a.aux = aux; a.out = out;
  const dim3 grid((unsigned)tiles, (unsigned)pl.chunks, (unsigned)N);
  switch (pl.nb) {
    case 1: launch_conv_k<1>(kh, kw, grid, s, a); break;
    case 2: launch_conv_k<2>(kh, kw, grid, s, a); break;
    default: launch_conv_k<3>(kh, kw, grid, s, a); break;
  }
  return EOGS_OK;
}

// ---- RAFT-small's update block ----

constexpr int U_CORR = 196, U_HID = 96, U_CTX = 64, U_F1 = 64, U_F2 = 32, U_MOT = 80, U_FH = 128;
constexpr int U_GRU_IN = U_HID + U_CTX + U_MOT + 2;  // convz / convr / convq read [h | context | motion | flow]: 242 channels
enum { UC_CORR1, UC_FLOW1, UC_FLOW2, UC_CONV, UC_HOIST_ZR, UC_HOIST_Q, UC_GATES, UC_Q, UC_FH1, UC_FH2, UC_COUNT };

struct UConv { int kh, kw, nseg, C[3], cout; };
constexpr UConv U_CONVS[UC_COUNT] = {
    {1, 1, 1, {U_CORR, 0, 0}, U_HID},          {7, 7, 1, {2, 0, 0}, U_F1},           {3, 3, 1, {U_F1, 0, 0}, U_F2},
    {3, 3, 2, {U_HID, U_F2, 0}, U_MOT},        {3, 3, 1, {U_CTX, 0, 0}, 2 * U_HID},  {3, 3, 1, {U_CTX, 0, 0}, U_HID},
    {3, 3, 3, {U_HID, U_MOT, 2}, 2 * U_HID},   {3, 3, 3, {U_HID, U_MOT, 2}, U_HID},  {3, 3, 1, {U_HID, 0, 0}, U_FH},
    {3, 3, 1, {U_FH, 0, 0}, 2}};

struct UpdateLayout {
  float* pw[UC_COUNT];
  size_t pw_bytes[UC_COUNT];
  float* bias[UC_COUNT];  // a convolution's bias, copied at begin (the hoisted ones: convz | convr, and convq; the GRU's two: none)
  float *plane_zr, *plane_q, *hidden, *corr1, *flow1, *flow2, *motion, *gates, *fh1;
  size_t hidden_off, bytes;
};

inline UpdateLayout update_layout(void* ws, int N, int h, int w) {
  UpdateLayout u{};
  char* base = ws ? ws_base(ws) : nullptr;
  const size_t P = (size_t)N * h * w;
  size_t o = 0;
  for (int i = 0; i < UC_COUNT; i++) {
    const size_t n = conv_plan(U_CONVS[i].kh, U_CONVS[i].kw, U_CONVS[i].nseg, U_CONVS[i].C, U_CONVS[i].cout).floats;
    u.pw_bytes[i] = n * sizeof(float);
    o = ws_carve(base, o, u.pw[i], n);
  }
  for (int i = 0; i < UC_COUNT; i++) o = ws_carve(base, o, u.bias[i], (size_t)U_CONVS[i].cout);
  o = ws_carve(base, o, u.plane_zr, P * 2 * U_HID);
  o = ws_carve(base, o, u.plane_q, P * U_HID);
  u.hidden_off = ws_align(o);
  o = ws_carve(base, o, u.hidden, P * U_HID);
  o = ws_carve(base, o, u.corr1, P * U_HID);
  o = ws_carve(base, o, u.flow1, P * U_F1);
  o = ws_carve(base, o, u.flow2, P * U_F2);
  o = ws_carve(base, o, u.motion, P * U_MOT);
  o = ws_carve(base, o, u.gates, P * 2 * U_HID);
  o = ws_carve(base, o, u.fh1, P * U_FH);
  u.bytes = ws_align(o) + 256;
  return u;
}

int check_update_shape(const char* who, int N, int h, int w) {
  if (N < 1 || h < 1 || w < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (N, h and w must be at least 1)", who);
  if (N > 65535) return fail(EOGS_ERR_INVALID_ARG, "%s: N above 65535", who);
  if ((int64_t)N * h * w * (2 * U_HID) > 0x7FFFFFFFll) return fail(EOGS_ERR_INVALID_ARG, "%s: more than 2^31 - 1 elements in a map", who);
  return EOGS_OK;
}

// one convolution of a step: the table's shape and packing, this call's operands
int tconv(const char* who, const UConv& c, const float* pw, size_t pw_bytes, int N, int h, int w, const float* in0, const float* in1,
          const float* in2, const float* bias, const float* add, const float* aux, float* out, int epi, unsigned flags, hipStream_t s) {
  const float* in[3] = {in0, in1, in2};
  return conv_checked(who, N, h, w, c.kh, c.kw, true, c.nseg, c.C, in, c.cout, pw, pw_bytes, bias, add, aux, out, epi, flags, s);
}

int uconv(const char* who, const UpdateLayout& u, int i, int N, int h, int w, const float* in0, const float* in1, const float* in2,
          const float* bias, const float* add, const float* aux, float* out, int epi, unsigned flags, hipStream_t s) {
  return tconv(who, U_CONVS[i], u.pw[i], u.pw_bytes[i], N, h, w, in0, in1, in2, bias, add, aux, out, epi, flags, s);
}

// ---- RAFT-large's update block and mask predictor ----

constexpr int L_CORR = 324, L_HID = 128, L_CTX = 128, L_C1 = 256, L_C2 = 192, L_F1 = 128, L_F2 = 64, L_MOT = 126, L_FH = 256,
              L_MH = 256, L_MASK = EOGS_RAFT_MASK_CHANNELS;
constexpr int L_GRU_IN = L_HID + L_CTX + L_MOT + 2;  // [h | context | motion | flow]: 384 channels
enum { LC_CORR1, LC_CORR2, LC_FLOW1, LC_FLOW2, LC_CONV, LC_HOIST_ZR1, LC_HOIST_Q1, LC_GATES1, LC_Q1, LC_HOIST_ZR2, LC_HOIST_Q2,
       LC_GATES2, LC_Q2, LC_FH1, LC_FH2, LC_MASK1, LC_MASK2, LC_COUNT };
constexpr UConv L_CONVS[LC_COUNT] = {
    {1, 1, 1, {L_CORR, 0, 0}, L_C1},           {3, 3, 1, {L_C1, 0, 0}, L_C2},             {7, 7, 1, {2, 0, 0}, L_F1},
    {3, 3, 1, {L_F1, 0, 0}, L_F2},             {3, 3, 2, {L_C2, L_F2, 0}, L_MOT},
    {1, 5, 1, {L_CTX, 0, 0}, 2 * L_HID},       {1, 5, 1, {L_CTX, 0, 0}, L_HID},
    {1, 5, 3, {L_HID, L_MOT, 2}, 2 * L_HID},   {1, 5, 3, {L_HID, L_MOT, 2}, L_HID},
    {5, 1, 1, {L_CTX, 0, 0}, 2 * L_HID},       {5, 1, 1, {L_CTX, 0, 0}, L_HID},
    {5, 1, 3, {L_HID, L_MOT, 2}, 2 * L_HID},   {5, 1, 3, {L_HID, L_MOT, 2}, L_HID},
    {3, 3, 1, {L_HID, 0, 0}, L_FH},            {3, 3, 1, {L_FH, 0, 0}, 2},
    {3, 3, 1, {L_HID, 0, 0}, L_MH},            {1, 1, 1, {L_MH, 0, 0}, L_MASK}};
static_assert(L_C1 == L_FH && L_C1 == L_MH, "convcorr1's output, the flow head's and the mask head's hidden map share one buffer");

struct LargeLayout {
  float* pw[LC_COUNT];
  size_t pw_bytes[LC_COUNT];
  float* bias[LC_COUNT];  // as UpdateLayout's: the hoisted ones hold convz | convr and convq, the GRUs' own none
  float *plane_zr[2], *plane_q[2], *hidden, *wide, *corr2, *flow1, *flow2, *motion, *gates;
  size_t hidden_off, bytes;
};

inline LargeLayout large_layout(void* ws, int N, int h, int w) {
  LargeLayout u{};
  char* base = ws ? ws_base(ws) : nullptr;
  const size_t P = (size_t)N * h * w;
  size_t o = 0;
  for (int i = 0; i < LC_COUNT; i++) {
    const size_t n = conv_plan(L_CONVS[i].kh, L_CONVS[i].kw, L_CONVS[i].nseg, L_CONVS[i].C, L_CONVS[i].cout).floats;
    u.pw_bytes[i] = n * sizeof(float);
    o = ws_carve(base, o, u.pw[i], n);
  }
  for (int i = 0; i < LC_COUNT; i++) o = ws_carve(base, o, u.bias[i], (size_t)L_CONVS[i].cout);
  for (int g = 0; g < 2; g++) {
    o = ws_carve(base, o, u.plane_zr[g], P * 2 * L_HID);
    o = ws_carve(base, o, u.plane_q[g], P * L_HID);
  }
  u.hidden_off = ws_align(o);
  o = ws_carve(base, o, u.hidden, P * L_HID);
  o = ws_carve(base, o, u.wide, P * L_C1);  // convcorr1's output, then flow_head.conv1's, then the mask head's: each dead before the next
  o = ws_carve(base, o, u.corr2, P * L_C2);
  o = ws_carve(base, o, u.flow1, P * L_F1);
  o = ws_carve(base, o, u.flow2, P * L_F2);
  o = ws_carve(base, o, u.motion, P * L_MOT);
  o = ws_carve(base, o, u.gates, P * 2 * L_HID);
  u.bytes = ws_align(o) + 256;
  return u;
}

int check_large_shape(const char* who, int N, int h, int w) {
  if (N < 1 || h < 1 || w < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (N, h and w must be at least 1)", who);
  if (N > 65535) return fail(EOGS_ERR_INVALID_ARG, "%s: N above 65535", who);
  if ((int64_t)N * h * w * L_MASK > 0x7FFFFFFFll) return fail(EOGS_ERR_INVALID_ARG, "%s: more than 2^31 - 1 elements in a map", who);
  return EOGS_OK;
}

int large_conv(const char* who, const LargeLayout& u, int i, int N, int h, int w, const float* in0, const float* in1, const float* in2,
          const float* bias, const float* add, const float* aux, float* out, int epi, unsigned flags, hipStream_t s) {
  return tconv(who, L_CONVS[i], u.pw[i], u.pw_bytes[i], N, h, w, in0, in1, in2, bias, add, aux, out, epi, flags, s);
}

void copy_bias(hipStream_t s, int n, const float* src, float* dst) {
  hipLaunchKernelGGL(flownet_copy_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, src, dst);
}

}  // namespace

extern "C" {

int eogs_flownet_conv_info(int* tile_w, int* tile_h) {
  clear_error();
  if (!tile_w || !tile_h) return fail(EOGS_ERR_INVALID_ARG, "flownet_conv_info: NULL argument");
  *tile_w = FT_W;
  *tile_h = FT_H;
  return EOGS_OK;
}

int eogs_flownet_conv_pack_bytes(int k, int nseg, const int* seg_channels, int cout, size_t* bytes) {
  clear_error();
  const int rc = check_conv_shape("flownet_conv_pack_bytes", k, nseg, seg_channels, cout);
  if (rc != EOGS_OK) return rc;
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "flownet_conv_pack_bytes: NULL argument");
  *bytes = conv_plan(k, nseg, seg_channels, cout).floats * sizeof(float);
  return EOGS_OK;
}

int eogs_flownet_conv_pack(int k, int nseg, const int* seg_channels, const int* seg_offsets, int cin, int cout, int cout_off,
                           int cout_n, const float* weight, void* packed, size_t packed_bytes, void* stream) {
  clear_error();
  hipStream_t s = (hipStream_t)stream;
  RC_TRY(pack_checked("flownet_conv_pack", k, nseg, seg_channels, seg_offsets, cin, cout, cout_off, cout_n, weight, packed, packed_bytes, s));
  LAUNCH_TRY(s, false, "flownet_conv_pack");
  return EOGS_OK;
}

int eogs_flownet_conv(int N, int h, int w, int k, int nseg, const int* seg_channels, const float* in0, const float* in1,
                      const float* in2, int cout, const void* packed, size_t packed_bytes, const float* bias, const float* add,
                      const float* aux, float* out, int epilogue, unsigned flags, void* stream) {
  clear_error();
  hipStream_t s = (hipStream_t)stream;
  const float* in[3] = {in0, in1, in2};
  RC_TRY(conv_checked("flownet_conv", N, h, w, k, k, false, nseg, seg_channels, in, cout, packed, packed_bytes, bias, add, aux, out, epilogue, flags, s));
  LAUNCH_TRY(s, false, "flownet_conv");
  return EOGS_OK;
}

int eogs_flowrect_pack_bytes(int kh, int kw, int nseg, const int* seg_channels, int cout, size_t* bytes) {
  clear_error();
  const int rc = check_conv_shape("flowrect_pack_bytes", kh, kw, true, nseg, seg_channels, cout);
  if (rc != EOGS_OK) return rc;
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "flowrect_pack_bytes: NULL argument");
  *bytes = conv_plan(kh, kw, nseg, seg_channels, cout).floats * sizeof(float);
  return EOGS_OK;
}

int eogs_flowrect_pack(int kh, int kw, int nseg, const int* seg_channels, const int* seg_offsets, int cin, int cout,
                                int cout_off, int cout_n, const float* weight, void* packed, size_t packed_bytes, void* stream) {
  clear_error();
  hipStream_t s = (hipStream_t)stream;
  RC_TRY(pack_checked("flowrect_pack", kh, kw, true, nseg, seg_channels, seg_offsets, cin, cout, cout_off, cout_n, weight, packed,
                      packed_bytes, s));
  LAUNCH_TRY(s, false, "flowrect_pack");
  return EOGS_OK;
}

int eogs_flowrect_conv(int N, int h, int w, int kh, int kw, int nseg, const int* seg_channels, const float* in0, const float* in1,
                           const float* in2, int cout, const void* packed, size_t packed_bytes, const float* bias, const float* add,
                           const float* aux, float* out, int epilogue, unsigned flags, void* stream) {
  clear_error();
  hipStream_t s = (hipStream_t)stream;
  const float* in[3] = {in0, in1, in2};
  RC_TRY(conv_checked("flowrect_conv", N, h, w, kh, kw, true, nseg, seg_channels, in, cout, packed, packed_bytes, bias, add, aux, out,
                      epilogue, flags, s));
  LAUNCH_TRY(s, false, "flowrect_conv");
  return EOGS_OK;
}

int eogs_flownet_update_bytes(int N, int h, int w, size_t* bytes) {
  clear_error();
  RC_TRY(check_update_shape("flownet_update_bytes", N, h, w));
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "flownet_update_bytes: NULL argument");
  *bytes = update_layout(nullptr, N, h, w).bytes;
  return EOGS_OK;
}

int eogs_flownet_update_hidden_offset(int N, int h, int w, size_t* offset) {
  clear_error();
  RC_TRY(check_update_shape("flownet_update_hidden_offset", N, h, w));
  if (!offset) return fail(EOGS_ERR_INVALID_ARG, "flownet_update_hidden_offset: NULL argument");
  *offset = update_layout(nullptr, N, h, w).hidden_off;
  return EOGS_OK;
}

int eogs_flownet_update_begin(int N, int h, int w, const float* const* params, const float* hidden, const float* context, void* ws,
                              size_t ws_bytes, void* stream) {
  clear_error();
  const char* who = "flownet_update_begin";
  RC_TRY(check_update_shape(who, N, h, w));
  if (!params || !hidden || !context || !ws) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  for (int i = 0; i < EOGS_FLOWNET_UPDATE_PARAMS; i++) {
    if (!params[i]) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!aligned16(params[i])) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  }
  if (!aligned16(hidden) || !aligned16(context)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const UpdateLayout u = update_layout(ws, N, h, w);
  if (ws_bytes < u.bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t s = (hipStream_t)stream;
  // params: weight, bias of convcorr1, convflow1, convflow2, conv, convz, convr, convq, flow_head.conv1, flow_head.conv2
  const float *wz = params[8], *bz = params[9], *wr = params[10], *br = params[11], *wq = params[12], *bq = params[13];
  const int plain[][2] = {{UC_CORR1, 0}, {UC_FLOW1, 2}, {UC_FLOW2, 4}, {UC_CONV, 6}, {UC_FH1, 14}, {UC_FH2, 16}};
  for (const auto& pc : plain) {
    const UConv& c = U_CONVS[pc[0]];
    int cin = 0;
    for (int i = 0; i < c.nseg; i++) cin += c.C[i];
    RC_TRY(pack_checked(who, c.kh, c.nseg, c.C, nullptr, cin, c.cout, 0, c.cout, params[pc[1]], u.pw[pc[0]], u.pw_bytes[pc[0]], s));
    hipLaunchKernelGGL(flownet_copy_kernel, dim3(1), dim3(256), 0, s, c.cout, params[pc[1] + 1], u.bias[pc[0]]);
  }
  // the GRU's three convolutions split by input channel: the context's 64 (once per forward, here) and the rest (every step)
  const int ctx_off[1] = {U_HID}, rest_off[3] = {0, U_HID + U_CTX, U_HID + U_CTX + U_MOT};
  const UConv &hz = U_CONVS[UC_HOIST_ZR], &hq = U_CONVS[UC_HOIST_Q], &gz = U_CONVS[UC_GATES], &gq = U_CONVS[UC_Q];
  RC_TRY(pack_checked(who, 3, hz.nseg, hz.C, ctx_off, U_GRU_IN, hz.cout, 0, U_HID, wz, u.pw[UC_HOIST_ZR], u.pw_bytes[UC_HOIST_ZR], s));
  RC_TRY(pack_checked(who, 3, hz.nseg, hz.C, ctx_off, U_GRU_IN, hz.cout, U_HID, U_HID, wr, u.pw[UC_HOIST_ZR], u.pw_bytes[UC_HOIST_ZR], s));
  RC_TRY(pack_checked(who, 3, hq.nseg, hq.C, ctx_off, U_GRU_IN, hq.cout, 0, U_HID, wq, u.pw[UC_HOIST_Q], u.pw_bytes[UC_HOIST_Q], s));
  RC_TRY(pack_checked(who, 3, gz.nseg, gz.C, rest_off, U_GRU_IN, gz.cout, 0, U_HID, wz, u.pw[UC_GATES], u.pw_bytes[UC_GATES], s));
  RC_TRY(pack_checked(who, 3, gz.nseg, gz.C, rest_off, U_GRU_IN, gz.cout, U_HID, U_HID, wr, u.pw[UC_GATES], u.pw_bytes[UC_GATES], s));
  RC_TRY(pack_checked(who, 3, gq.nseg, gq.C, rest_off, U_GRU_IN, gq.cout, 0, U_HID, wq, u.pw[UC_Q], u.pw_bytes[UC_Q], s));
  hipLaunchKernelGGL(flownet_copy_kernel, dim3(1), dim3(256), 0, s, U_HID, bz, u.bias[UC_HOIST_ZR]);
  hipLaunchKernelGGL(flownet_copy_kernel, dim3(1), dim3(256), 0, s, U_HID, br, u.bias[UC_HOIST_ZR] + U_HID);
  hipLaunchKernelGGL(flownet_copy_kernel, dim3(1), dim3(256), 0, s, U_HID, bq, u.bias[UC_HOIST_Q]);
  const int64_t total = (int64_t)N * h * w * U_HID;
  hipLaunchKernelGGL(flownet_to_cl_kernel, dim3(capped_blocks(total, 256, 4096)), dim3(256), 0, s, total, U_HID, h * w, hidden, u.hidden);
  // the hoisted planes: conv3x3(context, W[:, context's channels]) + bias, linear under zero padding
  RC_TRY(uconv(who, u, UC_HOIST_ZR, N, h, w, context, nullptr, nullptr, u.bias[UC_HOIST_ZR], nullptr, nullptr, u.plane_zr, EOGS_FLOWNET_EPI_BIAS, 1u, s));
  RC_TRY(uconv(who, u, UC_HOIST_Q, N, h, w, context, nullptr, nullptr, u.bias[UC_HOIST_Q], nullptr, nullptr, u.plane_q, EOGS_FLOWNET_EPI_BIAS, 1u, s));
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
}

int eogs_flownet_update_step(int N, int h, int w, const float* corr, const float* flow, void* ws, size_t ws_bytes, float* delta,
                             void* stream) {
  clear_error();
  const char* who = "flownet_update_step";
  RC_TRY(check_update_shape(who, N, h, w));
  if (!corr || !flow || !ws || !delta) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(corr) || !aligned16(flow) || !aligned16(delta)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const UpdateLayout u = update_layout(ws, N, h, w);
  if (ws_bytes < u.bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t s = (hipStream_t)stream;
  const int BIAS = EOGS_FLOWNET_EPI_BIAS, RELU = EOGS_FLOWNET_EPI_RELU;
  const size_t half = (size_t)N * h * w * U_HID;  // the gates' two maps: z, then r * h
  // motion encoder (corr and flow are read as NCHW planes)
  RC_TRY(uconv(who, u, UC_CORR1, N, h, w, corr, nullptr, nullptr, u.bias[UC_CORR1], nullptr, nullptr, u.corr1, RELU, 1u, s));
  RC_TRY(uconv(who, u, UC_FLOW1, N, h, w, flow, nullptr, nullptr, u.bias[UC_FLOW1], nullptr, nullptr, u.flow1, RELU, 1u, s));
  RC_TRY(uconv(who, u, UC_FLOW2, N, h, w, u.flow1, nullptr, nullptr, u.bias[UC_FLOW2], nullptr, nullptr, u.flow2, RELU, 0u, s));
  RC_TRY(uconv(who, u, UC_CONV, N, h, w, u.corr1, u.flow2, nullptr, u.bias[UC_CONV], nullptr, nullptr, u.motion, RELU, 0u, s));
  // GRU over [h | motion | flow], the context's share added as a plane
  RC_TRY(uconv(who, u, UC_GATES, N, h, w, u.hidden, u.motion, flow, nullptr, u.plane_zr, u.hidden, u.gates, EOGS_FLOWNET_EPI_GATES, 4u, s));
  RC_TRY(uconv(who, u, UC_Q, N, h, w, u.gates + half, u.motion, flow, nullptr, u.plane_q, u.gates, u.hidden, EOGS_FLOWNET_EPI_GRU, 4u, s));
  // flow head
  RC_TRY(uconv(who, u, UC_FH1, N, h, w, u.hidden, nullptr, nullptr, u.bias[UC_FH1], nullptr, nullptr, u.fh1, RELU, 0u, s));
  RC_TRY(uconv(who, u, UC_FH2, N, h, w, u.fh1, nullptr, nullptr, u.bias[UC_FH2], nullptr, nullptr, delta, BIAS, EOGS_FLOWNET_OUT_NCHW, s));
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
}

int eogs_flowlarge_bytes(int N, int h, int w, size_t* bytes) {
  clear_error();
  RC_TRY(check_large_shape("flowlarge_bytes", N, h, w));
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "flowlarge_bytes: NULL argument");
  *bytes = large_layout(nullptr, N, h, w).bytes;
  return EOGS_OK;
}

int eogs_flowlarge_hidden_offset(int N, int h, int w, size_t* offset) {
  clear_error();
  RC_TRY(check_large_shape("flowlarge_hidden_offset", N, h, w));
  if (!offset) return fail(EOGS_ERR_INVALID_ARG, "flowlarge_hidden_offset: NULL argument");
  *offset = large_layout(nullptr, N, h, w).hidden_off;
  return EOGS_OK;
}

int eogs_flowlarge_begin(int N, int h, int w, const float* const* params, const float* hidden, const float* context,
                                    void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const char* who = "flowlarge_begin";
  RC_TRY(check_large_shape(who, N, h, w));
  if (!params || !hidden || !context || !ws) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  for (int i = 0; i < EOGS_FLOWLARGE_PARAMS; i++) {
    if (!params[i]) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!aligned16(params[i])) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  }
  if (!aligned16(hidden) || !aligned16(context)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const LargeLayout u = large_layout(ws, N, h, w);
  if (ws_bytes < u.bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t s = (hipStream_t)stream;
  // params: weight, bias of convcorr1, convcorr2, convflow1, convflow2, conv, convgru1.{convz, convr, convq}, convgru2.{convz, convr,
  // convq}, flow_head.{conv1, conv2}, mask_predictor.{convrelu.0, conv}
  const int plain[][2] = {{LC_CORR1, 0}, {LC_CORR2, 2}, {LC_FLOW1, 4}, {LC_FLOW2, 6}, {LC_CONV, 8}, {LC_FH1, 22}, {LC_FH2, 24},
                          {LC_MASK1, 26}, {LC_MASK2, 28}};
  for (const auto& pc : plain) {
    const UConv& c = L_CONVS[pc[0]];
    int cin = 0;
    for (int i = 0; i < c.nseg; i++) cin += c.C[i];
    RC_TRY(pack_checked(who, c.kh, c.kw, true, c.nseg, c.C, nullptr, cin, c.cout, 0, c.cout, params[pc[1]], u.pw[pc[0]], u.pw_bytes[pc[0]], s));
    copy_bias(s, c.cout, params[pc[1] + 1], u.bias[pc[0]]);
  }
  const int64_t total = (int64_t)N * h * w * L_HID;
  hipLaunchKernelGGL(flownet_to_cl_kernel, dim3(capped_blocks(total, 256, 4096)), dim3(256), 0, s, total, L_HID, h * w, hidden, u.hidden);
  // each GRU's three convolutions split by input channel: the context's 128 (once per forward, here) and the rest (every step)
  const int ctx_off[1] = {L_HID}, rest_off[3] = {0, L_HID + L_CTX, L_HID + L_CTX + L_MOT};
  for (int g = 0; g < 2; g++) {
    const int hzr = g ? LC_HOIST_ZR2 : LC_HOIST_ZR1, hq = g ? LC_HOIST_Q2 : LC_HOIST_Q1, gz = g ? LC_GATES2 : LC_GATES1, gq = g ? LC_Q2 : LC_Q1;
    const float *wz = params[10 + 6 * g], *bz = params[11 + 6 * g], *wr = params[12 + 6 * g], *br = params[13 + 6 * g],
                *wq = params[14 + 6 * g], *bq = params[15 + 6 * g];
    const int kh = L_CONVS[gz].kh, kw = L_CONVS[gz].kw;
    RC_TRY(pack_checked(who, kh, kw, true, 1, L_CONVS[hzr].C, ctx_off, L_GRU_IN, 2 * L_HID, 0, L_HID, wz, u.pw[hzr], u.pw_bytes[hzr], s));
    RC_TRY(pack_checked(who, kh, kw, true, 1, L_CONVS[hzr].C, ctx_off, L_GRU_IN, 2 * L_HID, L_HID, L_HID, wr, u.pw[hzr], u.pw_bytes[hzr], s));
    RC_TRY(pack_checked(who, kh, kw, true, 1, L_CONVS[hq].C, ctx_off, L_GRU_IN, L_HID, 0, L_HID, wq, u.pw[hq], u.pw_bytes[hq], s));
    RC_TRY(pack_checked(who, kh, kw, true, 3, L_CONVS[gz].C, rest_off, L_GRU_IN, 2 * L_HID, 0, L_HID, wz, u.pw[gz], u.pw_bytes[gz], s));
    RC_TRY(pack_checked(who, kh, kw, true, 3, L_CONVS[gz].C, rest_off, L_GRU_IN, 2 * L_HID, L_HID, L_HID, wr, u.pw[gz], u.pw_bytes[gz], s));
    RC_TRY(pack_checked(who, kh, kw, true, 3, L_CONVS[gq].C, rest_off, L_GRU_IN, L_HID, 0, L_HID, wq, u.pw[gq], u.pw_bytes[gq], s));
    copy_bias(s, L_HID, bz, u.bias[hzr]);
    copy_bias(s, L_HID, br, u.bias[hzr] + L_HID);
    copy_bias(s, L_HID, bq, u.bias[hq]);
    // the hoisted planes: conv(context, W[:, context's channels]) + bias, linear under zero padding
    RC_TRY(large_conv(who, u, hzr, N, h, w, context, nullptr, nullptr, u.bias[hzr], nullptr, nullptr, u.plane_zr[g], EOGS_FLOWNET_EPI_BIAS, 1u, s));
    RC_TRY(large_conv(who, u, hq, N, h, w, context, nullptr, nullptr, u.bias[hq], nullptr, nullptr, u.plane_q[g], EOGS_FLOWNET_EPI_BIAS, 1u, s));
  }
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
}

int eogs_flowlarge_step(int N, int h, int w, const float* corr, const float* flow, void* ws, size_t ws_bytes, float* delta,
                                   void* stream) {
  clear_error();
  const char* who = "flowlarge_step";
  RC_TRY(check_large_shape(who, N, h, w));
  if (!corr || !flow || !ws || !delta) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(corr) || !aligned16(flow) || !aligned16(delta)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const LargeLayout u = large_layout(ws, N, h, w);
  if (ws_bytes < u.bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t s = (hipStream_t)stream;
  const int BIAS = EOGS_FLOWNET_EPI_BIAS, RELU = EOGS_FLOWNET_EPI_RELU;
  const size_t half = (size_t)N * h * w * L_HID;  // the gates' two maps: z, then r * h
  // motion encoder (corr and flow are read as NCHW planes)
  RC_TRY(large_conv(who, u, LC_CORR1, N, h, w, corr, nullptr, nullptr, u.bias[LC_CORR1], nullptr, nullptr, u.wide, RELU, 1u, s));
  RC_TRY(large_conv(who, u, LC_CORR2, N, h, w, u.wide, nullptr, nullptr, u.bias[LC_CORR2], nullptr, nullptr, u.corr2, RELU, 0u, s));
  RC_TRY(large_conv(who, u, LC_FLOW1, N, h, w, flow, nullptr, nullptr, u.bias[LC_FLOW1], nullptr, nullptr, u.flow1, RELU, 1u, s));
  RC_TRY(large_conv(who, u, LC_FLOW2, N, h, w, u.flow1, nullptr, nullptr, u.bias[LC_FLOW2], nullptr, nullptr, u.flow2, RELU, 0u, s));
  RC_TRY(large_conv(who, u, LC_CONV, N, h, w, u.corr2, u.flow2, nullptr, u.bias[LC_CONV], nullptr, nullptr, u.motion, RELU, 0u, s));
  // the 1 x 5 GRU, then the 5 x 1 one, each over [h | motion | flow] with the context's share added as a plane
  for (int g = 0; g < 2; g++) {
    const int gz = g ? LC_GATES2 : LC_GATES1, gq = g ? LC_Q2 : LC_Q1;
    RC_TRY(large_conv(who, u, gz, N, h, w, u.hidden, u.motion, flow, nullptr, u.plane_zr[g], u.hidden, u.gates, EOGS_FLOWNET_EPI_GATES, 4u, s));
    RC_TRY(large_conv(who, u, gq, N, h, w, u.gates + half, u.motion, flow, nullptr, u.plane_q[g], u.gates, u.hidden, EOGS_FLOWNET_EPI_GRU, 4u, s));
  }
  // flow head
  RC_TRY(large_conv(who, u, LC_FH1, N, h, w, u.hidden, nullptr, nullptr, u.bias[LC_FH1], nullptr, nullptr, u.wide, RELU, 0u, s));
  RC_TRY(large_conv(who, u, LC_FH2, N, h, w, u.wide, nullptr, nullptr, u.bias[LC_FH2], nullptr, nullptr, delta, BIAS, EOGS_FLOWNET_OUT_NCHW, s));
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
}

int eogs_flowlarge_mask(int N, int h, int w, void* ws, size_t ws_bytes, float* mask, void* stream) {
  clear_error();
  const char* who = "flowlarge_mask";
  RC_TRY(check_large_shape(who, N, h, w));
  if (!ws || !mask) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(mask)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const LargeLayout u = large_layout(ws, N, h, w);
  if (ws_bytes < u.bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t s = (hipStream_t)stream;
  RC_TRY(large_conv(who, u, LC_MASK1, N, h, w, u.hidden, nullptr, nullptr, u.bias[LC_MASK1], nullptr, nullptr, u.wide, EOGS_FLOWNET_EPI_RELU, 0u, s));
  RC_TRY(large_conv(who, u, LC_MASK2, N, h, w, u.wide, nullptr, nullptr, u.bias[LC_MASK2], nullptr, nullptr, mask, EOGS_FLOWRECT_EPI_QUARTER,
               EOGS_FLOWNET_OUT_NCHW, s));
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
}

}  // extern "C"
