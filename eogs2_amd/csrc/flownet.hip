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

// ---- the update block: RAFT-small's, and RAFT-large's with its mask predictor ----

// A convolution of the block. `param`: where its weight stands in the caller's params table, its bias right after it (for a
// GRU's gates and hoisted z | r plane: convz's weight, convr's two places on; for its q: convq's)
struct UConv { int kh, kw, nseg, C[3], cout, param; };
// the block's convolutions by role; a GRU g owns the four from UC_GRU + 4 g
enum { UC_CORR1, UC_CORR2, UC_FLOW1, UC_FLOW2, UC_CONV, UC_FH1, UC_FH2, UC_MASK1, UC_MASK2, UC_GRU, UC_MAX = UC_GRU + 4 * 2 };
enum { UG_HOIST_ZR, UG_HOIST_Q, UG_GATES, UG_Q };

// An update block, stated once. RAFT-small's is RAFT-large's without convcorr2, the second GRU and the mask head.
struct UGru { int kh, kw, param; };  // param: convz's weight; then its bias, convr's pair, convq's pair
struct UpdateDesc {
  int corr, hid, ctx, c1, c2, f1, f2, mot, fh, mh, mask;  // the widths; c2 = 0: no convcorr2, mh = mask = 0: no mask head
  int ngru;
  UGru gru[2];
  int p_corr1, p_corr2, p_flow1, p_flow2, p_conv, p_fh1, p_fh2, p_mask1, p_mask2;  // the plain convolutions in params (-1: none)
  int bound;             // channels the 2^31 - 1 element bound of a map is taken at
  UConv conv[UC_MAX];    // filled by update_desc from the above; cout = 0: the block has no such convolution
};

constexpr UpdateDesc update_desc(UpdateDesc d) {
  d.conv[UC_CORR1] = UConv{1, 1, 1, {d.corr, 0, 0}, d.c1, d.p_corr1};
  if (d.c2) d.conv[UC_CORR2] = UConv{3, 3, 1, {d.c1, 0, 0}, d.c2, d.p_corr2};
  d.conv[UC_FLOW1] = UConv{7, 7, 1, {2, 0, 0}, d.f1, d.p_flow1};
  d.conv[UC_FLOW2] = UConv{3, 3, 1, {d.f1, 0, 0}, d.f2, d.p_flow2};
  d.conv[UC_CONV] = UConv{3, 3, 2, {d.c2 ? d.c2 : d.c1, d.f2, 0}, d.mot, d.p_conv};
  d.conv[UC_FH1] = UConv{3, 3, 1, {d.hid, 0, 0}, d.fh, d.p_fh1};
  d.conv[UC_FH2] = UConv{3, 3, 1, {d.fh, 0, 0}, 2, d.p_fh2};
  if (d.mh) {
    d.conv[UC_MASK1] = UConv{3, 3, 1, {d.hid, 0, 0}, d.mh, d.p_mask1};
    d.conv[UC_MASK2] = UConv{1, 1, 1, {d.mh, 0, 0}, d.mask, d.p_mask2};
  }
  // convz / convr / convq read [h | context | motion | flow], split by input channel: the context's share is hoisted out of the steps
  for (int g = 0; g < d.ngru; g++) {
    const UGru& r = d.gru[g];
    UConv* c = d.conv + UC_GRU + 4 * g;
    c[UG_HOIST_ZR] = UConv{r.kh, r.kw, 1, {d.ctx, 0, 0}, 2 * d.hid, r.param};
    c[UG_HOIST_Q] = UConv{r.kh, r.kw, 1, {d.ctx, 0, 0}, d.hid, r.param + 4};
    c[UG_GATES] = UConv{r.kh, r.kw, 3, {d.hid, d.mot, 2}, 2 * d.hid, r.param};
    c[UG_Q] = UConv{r.kh, r.kw, 3, {d.hid, d.mot, 2}, d.hid, r.param + 4};
  }
  return d;
}

// the length of the params table the description reads: every weight and bias once, none left over (0 where they do not tile it)
constexpr int update_params(const UpdateDesc& d) {
  bool used[64] = {};
  int n = 0;
  for (int i = 0; i < UC_GRU + 3 * d.ngru; i++) {  // the plain convolutions, then convz, convr and convq of each GRU
    if (i < UC_GRU && !d.conv[i].cout) continue;
    const int p = i < UC_GRU ? d.conv[i].param : d.gru[(i - UC_GRU) / 3].param + 2 * ((i - UC_GRU) % 3);
    if (p < 0 || p % 2 || p >= 64 || used[p]) return 0;
    used[p] = true;
    n += 2;
  }
  for (int p = 0; p < n; p += 2)
    if (!used[p]) return 0;
  return n;
}

constexpr UpdateDesc U_SMALL = update_desc({
    /* corr hid ctx */ 196, 96, 64, /* c1 c2 */ 96, 0, /* f1 f2 mot */ 64, 32, 80, /* fh mh mask */ 128, 0, 0,
    /* one 3 x 3 GRU */ 1, {{3, 3, 8}},
    /* corr1 corr2 flow1 flow2 conv fh1 fh2 mask1 mask2 */ 0, -1, 2, 4, 6, 14, 16, -1, -1,
    /* bound: the gates' z | r */ 2 * 96});
constexpr UpdateDesc U_LARGE = update_desc({
    /* corr hid ctx */ 324, 128, 128, /* c1 c2 */ 256, 192, /* f1 f2 mot */ 128, 64, 126, /* fh mh mask */ 256, 256, EOGS_RAFT_MASK_CHANNELS,
    /* a 1 x 5 GRU, then a 5 x 1 one */ 2, {{1, 5, 10}, {5, 1, 16}},
    /* corr1 corr2 flow1 flow2 conv fh1 fh2 mask1 mask2 */ 0, 2, 4, 6, 8, 22, 24, 26, 28,
    /* bound: the mask */ EOGS_RAFT_MASK_CHANNELS});
static_assert(update_params(U_SMALL) == EOGS_FLOWNET_UPDATE_PARAMS && update_params(U_LARGE) == EOGS_FLOWLARGE_PARAMS,
              "a description reads exactly the params table of its entries");
static_assert(U_LARGE.c1 == U_LARGE.fh && U_LARGE.c1 == U_LARGE.mh, "convcorr1's output, the flow head's and the mask head's hidden map share one buffer");

struct UpdateLayout {
  float* pw[UC_MAX];
  size_t pw_bytes[UC_MAX];
  float* bias[UC_MAX];  // a convolution's bias, copied at begin (the hoisted ones: convz | convr, and convq; a GRU's own two: none)
  float *plane_zr[2], *plane_q[2], *hidden, *wide, *corr2, *flow1, *flow2, *motion, *gates, *fh1;
  size_t hidden_off, bytes;
};

inline UpdateLayout update_layout(const UpdateDesc& d, void* ws, int N, int h, int w) {
  UpdateLayout u{};
  char* base = ws ? ws_base(ws) : nullptr;
  const size_t P = (size_t)N * h * w;
  size_t o = 0;
  for (int i = 0; i < UC_MAX; i++) {
    const UConv& c = d.conv[i];
    if (!c.cout) continue;
    const size_t n = conv_plan(c.kh, c.kw, c.nseg, c.C, c.cout).floats;
    u.pw_bytes[i] = n * sizeof(float);
    o = ws_carve(base, o, u.pw[i], n);
  }
  for (int i = 0; i < UC_MAX; i++)
    if (d.conv[i].cout) o = ws_carve(base, o, u.bias[i], (size_t)d.conv[i].cout);
  for (int g = 0; g < d.ngru; g++) {
    o = ws_carve(base, o, u.plane_zr[g], P * 2 * d.hid);
    o = ws_carve(base, o, u.plane_q[g], P * d.hid);
  }
  u.hidden_off = ws_align(o);
  o = ws_carve(base, o, u.hidden, P * d.hid);
  o = ws_carve(base, o, u.wide, P * d.c1);  // convcorr1's output; where the widths agree, then flow_head.conv1's and the mask head's: each dead before the next
  if (d.c2) o = ws_carve(base, o, u.corr2, P * d.c2);
  o = ws_carve(base, o, u.flow1, P * d.f1);
  o = ws_carve(base, o, u.flow2, P * d.f2);
  o = ws_carve(base, o, u.motion, P * d.mot);
  o = ws_carve(base, o, u.gates, P * 2 * d.hid);
  u.fh1 = u.wide;
  if (d.fh != d.c1) o = ws_carve(base, o, u.fh1, P * d.fh);
  u.bytes = ws_align(o) + 256;
  return u;
}

int check_update_shape(const char* who, const UpdateDesc& d, int N, int h, int w) {
  if (N < 1 || h < 1 || w < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (N, h and w must be at least 1)", who);
  if (N > 65535) return fail(EOGS_ERR_INVALID_ARG, "%s: N above 65535", who);
  if ((int64_t)N * h * w * d.bound > 0x7FFFFFFFll) return fail(EOGS_ERR_INVALID_ARG, "%s: more than 2^31 - 1 elements in a map", who);
  return EOGS_OK;
}

// one convolution of the table: its shape and packing, this call's operands
int uconv(const char* who, const UpdateDesc& d, const UpdateLayout& u, int i, int N, int h, int w, const float* in0, const float* in1,
          const float* in2, const float* bias, const float* add, const float* aux, float* out, int epi, unsigned flags, hipStream_t s) {
  const UConv& c = d.conv[i];
  const float* in[3] = {in0, in1, in2};
  return conv_checked(who, N, h, w, c.kh, c.kw, true, c.nseg, c.C, in, c.cout, u.pw[i], u.pw_bytes[i], bias, add, aux, out, epi, flags, s);
}

void copy_bias(hipStream_t s, int n, const float* src, float* dst) {
  hipLaunchKernelGGL(flownet_copy_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, src, dst);
}

// eogs_*_bytes and eogs_*_hidden_offset: one field of the layout
int update_query(const char* who, const UpdateDesc& d, int N, int h, int w, size_t* out, size_t UpdateLayout::*field) {
  RC_TRY(check_update_shape(who, d, N, h, w));
  if (!out) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  *out = update_layout(d, nullptr, N, h, w).*field;
  return EOGS_OK;
}

int update_begin(const char* who, const UpdateDesc& d, int N, int h, int w, const float* const* params, const float* hidden,
                 const float* context, void* ws, size_t ws_bytes, hipStream_t s) {
  RC_TRY(check_update_shape(who, d, N, h, w));
  if (!params || !hidden || !context || !ws) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  for (int i = 0; i < update_params(d); i++) {
    if (!params[i]) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!aligned16(params[i])) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  }
  if (!aligned16(hidden) || !aligned16(context)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const UpdateLayout u = update_layout(d, ws, N, h, w);
  if (ws_bytes < u.bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  for (int i = 0; i < UC_GRU; i++) {  // the plain convolutions: packed whole, the bias copied
    const UConv& c = d.conv[i];
    if (!c.cout) continue;
    int cin = 0;
    for (int j = 0; j < c.nseg; j++) cin += c.C[j];
    RC_TRY(pack_checked(who, c.kh, c.kw, true, c.nseg, c.C, nullptr, cin, c.cout, 0, c.cout, params[c.param], u.pw[i], u.pw_bytes[i], s));
    copy_bias(s, c.cout, params[c.param + 1], u.bias[i]);
  }
  const int64_t total = (int64_t)N * h * w * d.hid;
  hipLaunchKernelGGL(flownet_to_cl_kernel, dim3(capped_blocks(total, 256, 4096)), dim3(256), 0, s, total, d.hid, h * w, hidden, u.hidden);
  // each GRU's three convolutions split by input channel: the context's (once per forward, here) and the rest (every step)
  const int gin = d.hid + d.ctx + d.mot + 2, ctx_off[1] = {d.hid}, rest_off[3] = {0, d.hid + d.ctx, d.hid + d.ctx + d.mot};
  for (int g = 0; g < d.ngru; g++) {
    const int hzr = UC_GRU + 4 * g + UG_HOIST_ZR, hq = UC_GRU + 4 * g + UG_HOIST_Q, gz = UC_GRU + 4 * g + UG_GATES, gq = UC_GRU + 4 * g + UG_Q;
    const float* const* p = params + d.gru[g].param;
    const float *wz = p[0], *bz = p[1], *wr = p[2], *br = p[3], *wq = p[4], *bq = p[5];
    const int kh = d.gru[g].kh, kw = d.gru[g].kw, H = d.hid;
    RC_TRY(pack_checked(who, kh, kw, true, 1, d.conv[hzr].C, ctx_off, gin, 2 * H, 0, H, wz, u.pw[hzr], u.pw_bytes[hzr], s));
    RC_TRY(pack_checked(who, kh, kw, true, 1, d.conv[hzr].C, ctx_off, gin, 2 * H, H, H, wr, u.pw[hzr], u.pw_bytes[hzr], s));
    RC_TRY(pack_checked(who, kh, kw, true, 1, d.conv[hq].C, ctx_off, gin, H, 0, H, wq, u.pw[hq], u.pw_bytes[hq], s));
    RC_TRY(pack_checked(who, kh, kw, true, 3, d.conv[gz].C, rest_off, gin, 2 * H, 0, H, wz, u.pw[gz], u.pw_bytes[gz], s));
    RC_TRY(pack_checked(who, kh, kw, true, 3, d.conv[gz].C, rest_off, gin, 2 * H, H, H, wr, u.pw[gz], u.pw_bytes[gz], s));
    RC_TRY(pack_checked(who, kh, kw, true, 3, d.conv[gq].C, rest_off, gin, H, 0, H, wq, u.pw[gq], u.pw_bytes[gq], s));
    copy_bias(s, H, bz, u.bias[hzr]);
    copy_bias(s, H, br, u.bias[hzr] + H);
    copy_bias(s, H, bq, u.bias[hq]);
    // the hoisted planes: conv(context, W[:, context's channels]) + bias, linear under zero padding
    RC_TRY(uconv(who, d, u, hzr, N, h, w, context, nullptr, nullptr, u.bias[hzr], nullptr, nullptr, u.plane_zr[g], EOGS_FLOWNET_EPI_BIAS, 1u, s));
    RC_TRY(uconv(who, d, u, hq, N, h, w, context, nullptr, nullptr, u.bias[hq], nullptr, nullptr, u.plane_q[g], EOGS_FLOWNET_EPI_BIAS, 1u, s));
  }
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
}

int update_step(const char* who, const UpdateDesc& d, int N, int h, int w, const float* corr, const float* flow, void* ws, size_t ws_bytes,
                float* delta, hipStream_t s) {
  RC_TRY(check_update_shape(who, d, N, h, w));
  if (!corr || !flow || !ws || !delta) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(corr) || !aligned16(flow) || !aligned16(delta)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const UpdateLayout u = update_layout(d, ws, N, h, w);
  if (ws_bytes < u.bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  const int BIAS = EOGS_FLOWNET_EPI_BIAS, RELU = EOGS_FLOWNET_EPI_RELU;
  const size_t half = (size_t)N * h * w * d.hid;  // the gates' two maps: z, then r * h
  // motion encoder (corr and flow are read as NCHW planes)
  RC_TRY(uconv(who, d, u, UC_CORR1, N, h, w, corr, nullptr, nullptr, u.bias[UC_CORR1], nullptr, nullptr, u.wide, RELU, 1u, s));
  if (d.c2) RC_TRY(uconv(who, d, u, UC_CORR2, N, h, w, u.wide, nullptr, nullptr, u.bias[UC_CORR2], nullptr, nullptr, u.corr2, RELU, 0u, s));
  RC_TRY(uconv(who, d, u, UC_FLOW1, N, h, w, flow, nullptr, nullptr, u.bias[UC_FLOW1], nullptr, nullptr, u.flow1, RELU, 1u, s));
  RC_TRY(uconv(who, d, u, UC_FLOW2, N, h, w, u.flow1, nullptr, nullptr, u.bias[UC_FLOW2], nullptr, nullptr, u.flow2, RELU, 0u, s));
  RC_TRY(uconv(who, d, u, UC_CONV, N, h, w, d.c2 ? u.corr2 : u.wide, u.flow2, nullptr, u.bias[UC_CONV], nullptr, nullptr, u.motion, RELU, 0u, s));
  // each GRU in turn over [h | motion | flow], the context's share added as a plane
  for (int g = 0; g < d.ngru; g++) {
    const int gz = UC_GRU + 4 * g + UG_GATES, gq = UC_GRU + 4 * g + UG_Q;
    RC_TRY(uconv(who, d, u, gz, N, h, w, u.hidden, u.motion, flow, nullptr, u.plane_zr[g], u.hidden, u.gates, EOGS_FLOWNET_EPI_GATES, 4u, s));
    RC_TRY(uconv(who, d, u, gq, N, h, w, u.gates + half, u.motion, flow, nullptr, u.plane_q[g], u.gates, u.hidden, EOGS_FLOWNET_EPI_GRU, 4u, s));
  }
  // flow head
  RC_TRY(uconv(who, d, u, UC_FH1, N, h, w, u.hidden, nullptr, nullptr, u.bias[UC_FH1], nullptr, nullptr, u.fh1, RELU, 0u, s));
  RC_TRY(uconv(who, d, u, UC_FH2, N, h, w, u.fh1, nullptr, nullptr, u.bias[UC_FH2], nullptr, nullptr, delta, BIAS, EOGS_FLOWNET_OUT_NCHW, s));
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
}

int update_mask(const char* who, const UpdateDesc& d, int N, int h, int w, void* ws, size_t ws_bytes, float* mask, hipStream_t s) {
  RC_TRY(check_update_shape(who, d, N, h, w));
  if (!ws || !mask) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(mask)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const UpdateLayout u = update_layout(d, ws, N, h, w);
  if (ws_bytes < u.bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  RC_TRY(uconv(who, d, u, UC_MASK1, N, h, w, u.hidden, nullptr, nullptr, u.bias[UC_MASK1], nullptr, nullptr, u.wide, EOGS_FLOWNET_EPI_RELU, 0u, s));
  RC_TRY(uconv(who, d, u, UC_MASK2, N, h, w, u.wide, nullptr, nullptr, u.bias[UC_MASK2], nullptr, nullptr, mask, EOGS_FLOWRECT_EPI_QUARTER,
               EOGS_FLOWNET_OUT_NCHW, s));
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
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

// RAFT-small's update block. params: weight, bias of convcorr1, convflow1, convflow2, conv, convz, convr, convq, flow_head.conv1,
// flow_head.conv2 (U_SMALL's positions)
int eogs_flownet_update_bytes(int N, int h, int w, size_t* bytes) {
  clear_error();
  return update_query("flownet_update_bytes", U_SMALL, N, h, w, bytes, &UpdateLayout::bytes);
}

int eogs_flownet_update_hidden_offset(int N, int h, int w, size_t* offset) {
  clear_error();
  return update_query("flownet_update_hidden_offset", U_SMALL, N, h, w, offset, &UpdateLayout::hidden_off);
}

int eogs_flownet_update_begin(int N, int h, int w, const float* const* params, const float* hidden, const float* context, void* ws,
                              size_t ws_bytes, void* stream) {
  clear_error();
  return update_begin("flownet_update_begin", U_SMALL, N, h, w, params, hidden, context, ws, ws_bytes, (hipStream_t)stream);
}

int eogs_flownet_update_step(int N, int h, int w, const float* corr, const float* flow, void* ws, size_t ws_bytes, float* delta,
                             void* stream) {
  clear_error();
  return update_step("flownet_update_step", U_SMALL, N, h, w, corr, flow, ws, ws_bytes, delta, (hipStream_t)stream);
}

// RAFT-large's update block and mask predictor. params: weight, bias of convcorr1, convcorr2, convflow1, convflow2, conv,
// convgru1.{convz, convr, convq}, convgru2.{convz, convr, convq}, flow_head.{conv1, conv2}, mask_predictor.{convrelu.0, conv}
// (U_LARGE's positions)
int eogs_flowlarge_bytes(int N, int h, int w, size_t* bytes) {
  clear_error();
  return update_query("flowlarge_bytes", U_LARGE, N, h, w, bytes, &UpdateLayout::bytes);
}

int eogs_flowlarge_hidden_offset(int N, int h, int w, size_t* offset) {
  clear_error();
  return update_query("flowlarge_hidden_offset", U_LARGE, N, h, w, offset, &UpdateLayout::hidden_off);
}

int eogs_flowlarge_begin(int N, int h, int w, const float* const* params, const float* hidden, const float* context,
                                    void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  return update_begin("flowlarge_begin", U_LARGE, N, h, w, params, hidden, context, ws, ws_bytes, (hipStream_t)stream);
}

int eogs_flowlarge_step(int N, int h, int w, const float* corr, const float* flow, void* ws, size_t ws_bytes, float* delta,
                                   void* stream) {
  clear_error();
  return update_step("flowlarge_step", U_LARGE, N, h, w, corr, flow, ws, ws_bytes, delta, (hipStream_t)stream);
}

int eogs_flowlarge_mask(int N, int h, int w, void* ws, size_t ws_bytes, float* mask, void* stream) {
  clear_error();
  return update_mask("flowlarge_mask", U_LARGE, N, h, w, ws, ws_bytes, mask, (hipStream_t)stream);
}

}  // extern "C"
