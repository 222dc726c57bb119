// flownet_conv.h — what the two convolution files of the flow network share (flownet.hip: the update block's stride-1
// kernel; flowenc.hip: the encoders' strided one): the position tile, the eight-channel chunk, the LDS strides, the plan of
// a packing and the kernel that fills it. Both kernels read ONE packed layout and sum in ONE order (chunks of FCK channels,
// per chunk the taps row-major, per tap the channels ascending), so a packing made for one serves the other.
#pragma once
#include "api_util.h"

namespace {

constexpr int FT_W = 16, FT_H = 8, FNT = 256;  // the position tile; four waves, two tile rows each
constexpr int FCK = 8;                         // input channels per staged chunk: two instructions deep
static_assert(FNT / 64 * 2 == FT_H && FT_W == 16, "a wave owns two 16-position rows of the tile");

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int fn_ws(int nb) { return nb == 1 ? 16 : 48; }  // packed row stride: 16 or 48 mod 64 floats
constexpr int fn_tg(int kh, int kw) { return kh * kw <= 9 ? kh * kw : kw; }  // taps per weight stage: all of up to nine, else one row
constexpr int fn_tg(int k) { return fn_tg(k, k); }

struct ConvPlan {
  int nb, chunks, ws, cchunks;  // blocks per workgroup, workgroups along Cout, packed row stride, chunks of FCK over all segments
  size_t floats;                // of the packed weights
};

inline ConvPlan conv_plan(int kh, int kw, int nseg, const int* C, int cout) {
  ConvPlan p{};
  const int nbt = (cout + 15) / 16;
  // the fewest padded blocks, three per workgroup on a tie
  p.nb = nbt == 1 ? 1 : (((nbt + 2) / 3) * 3 <= ((nbt + 1) / 2) * 2 ? 3 : 2);
  p.chunks = (nbt + p.nb - 1) / p.nb;
  p.ws = fn_ws(p.nb);
  for (int s = 0; s < nseg; s++) p.cchunks += (C[s] + FCK - 1) / FCK;
  p.floats = (size_t)p.cchunks * p.chunks * kh * kw * FCK * p.ws;
  return p;
}
inline ConvPlan conv_plan(int k, int nseg, const int* C, int cout) { return conv_plan(k, k, nseg, C, cout); }

struct PackArgs {
  int C[EOGS_FLOWNET_MAX_SEGMENTS], off[EOGS_FLOWNET_MAX_SEGMENTS];
  int nseg, taps, cin, cout, cout_off, cout_n, nb, chunks, ws;
  int64_t total;
  const float* weight;
  float* packed;
};

// torch's [cout_n][cin][kh][kw] (taps = kh kw, row-major) into [chunk of FCK channels][workgroup along Cout][tap][FCK][ws]: the columns this call owns,
// and zeros in every padded column; padded channel lanes of its columns are zeros
__global__ __launch_bounds__(256) void flownet_pack_kernel(PackArgs p) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < p.total; idx += (int64_t)gridDim.x * 256) {
    int64_t r = idx;
    const int nw = (int)(r % p.ws); r /= p.ws;
    const int c8 = (int)(r % FCK); r /= FCK;
    const int tap = (int)(r % p.taps); r /= p.taps;
    const int cc = (int)(r % p.chunks);
    int q = (int)(r / p.chunks);
    const int col = cc * p.nb * 16 + nw;
    if (nw >= p.nb * 16 || col >= p.cout) { p.packed[idx] = 0.f; continue; }
    if (col < p.cout_off || col >= p.cout_off + p.cout_n) continue;
    float v = 0.f;
    for (int s = 0; s < p.nseg; s++) {
      const int qs = (p.C[s] + FCK - 1) / FCK;
      if (q < qs) {
        const int ch = q * FCK + c8;
        if (ch < p.C[s]) v = p.weight[((int64_t)(col - p.cout_off) * p.cin + p.off[s] + ch) * p.taps + tap];
        break;
      }
      q -= qs;
    }
    p.packed[idx] = v;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the taps: a square of 1, 3, 5 or 7, or (with `rect`, the eogs_flowrect_* entries) 1 x 5 or 5 x 1 as well
inline int check_conv_shape(const char* who, int kh, int kw, bool rect, int nseg, const int* C, int cout) {
  const bool square = kh == kw && kh >= 1 && kh <= EOGS_FLOWNET_MAX_KERNEL && kh % 2 == 1;
  if (!rect && !square) return fail(EOGS_ERR_INVALID_ARG, "%s: the kernel size is 1, 3, 5 or 7", who);
  if (!square && !((kh == 1 && kw == 5) || (kh == 5 && kw == 1)))
    return fail(EOGS_ERR_INVALID_ARG, "%s: the kernel shape is 1 x 1, 3 x 3, 5 x 5, 7 x 7, 1 x 5 or 5 x 1", who);
  if (nseg < 1 || nseg > EOGS_FLOWNET_MAX_SEGMENTS || !C) return fail(EOGS_ERR_INVALID_ARG, "%s: one to three input segments", who);
  for (int s = 0; s < nseg; s++)
    if (C[s] < 1 || C[s] > 4096) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (a segment has 1 to 4096 channels)", who);
  if (cout < 1 || cout > 4096) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (Cout is 1 to 4096)", who);
  return EOGS_OK;
}
inline int check_conv_shape(const char* who, int k, int nseg, const int* C, int cout) { return check_conv_shape(who, k, k, false, nseg, C, cout); }

inline int pack_checked(const char* who, int kh, int kw, bool rect, int nseg, const int* C, const int* offsets, int cin, int cout,
                        int cout_off, int cout_n, const float* weight, void* packed, size_t packed_bytes, hipStream_t s) {
  const int rc = check_conv_shape(who, kh, kw, rect, nseg, C, cout);
  if (rc != EOGS_OK) return rc;
  int sum = 0;
  for (int i = 0; i < nseg; i++) sum += C[i];
  if (offsets) {
    for (int i = 0; i < nseg; i++)
      if (offsets[i] < 0 || offsets[i] > cin - C[i]) return fail(EOGS_ERR_INVALID_ARG, "%s: a segment lies outside the weight's Cin", who);
  } else if (sum != cin) {
    return fail(EOGS_ERR_INVALID_ARG, "%s: the segments' channels do not sum to the weight's Cin", who);
  }
  if (cout_off < 0 || cout_n < 1 || cout_off > cout - cout_n) return fail(EOGS_ERR_INVALID_ARG, "%s: the columns lie outside Cout", who);
  if (!weight || !packed) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (!aligned16(weight) || !aligned16(packed)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 16-byte aligned", who);
  const ConvPlan pl = conv_plan(kh, kw, nseg, C, cout);
  if (packed_bytes < pl.floats * sizeof(float)) return fail(EOGS_ERR_WORKSPACE, "%s: packed weights too small", who);
  PackArgs p{};
  int o = 0;
  for (int i = 0; i < nseg; i++) { p.C[i] = C[i]; p.off[i] = offsets ? offsets[i] : o; o += C[i]; }
  p.nseg = nseg; p.taps = kh * kw; p.cin = cin; p.cout = cout; p.cout_off = cout_off; p.cout_n = cout_n;
  p.nb = pl.nb; p.chunks = pl.chunks; p.ws = pl.ws; p.total = (int64_t)pl.floats;
  p.weight = weight; p.packed = reinterpret_cast<float*>(packed);
  hipLaunchKernelGGL(flownet_pack_kernel, dim3(capped_blocks(p.total, 256, 2048)), dim3(256), 0, s, p);
  return EOGS_OK;
}
inline int pack_checked(const char* who, int k, int nseg, const int* C, const int* offsets, int cin, int cout, int cout_off, int cout_n,
                        const float* weight, void* packed, size_t packed_bytes, hipStream_t s) {
  return pack_checked(who, k, k, false, nseg, C, offsets, cin, cout, cout_off, cout_n, weight, packed, packed_bytes, s);
}

#ifndef RC_TRY
#define RC_TRY(expr)                \
  do {                              \
    const int rc_ = (expr);         \
    if (rc_ != EOGS_OK) return rc_; \
  } while (0)
#endif

}  // namespace
