// reduce.h — the fixed-order wave64 / workgroup reductions and the scalar helpers the side modules share (device only).
// The library is built without fast-math and with -ffp-contract=off: each of these is ONE expression tree, so every kernel
// that sums through it rounds in the same order — what the modules' "same bits on every run" (and monitor.hip's "same
// bits as reg.hip") rest on.
//
// The two-stage sum every side module's scalars go through, in words (tests/reduce_cases.py restates it from here):
//   Stage 1. Workgroups of 256 threads, the grid capped (api_util.h: capped_blocks). Thread t of workgroup g adds its
//            elements g * 256 + t, + grid * 256, ... in that order into its own accumulator. The 64 lanes of a wave
//            combine by the xor butterfly (offsets 32, 16, ..., 1: v += v of lane ^ offset), the workgroup adds its four
//            wave sums left to right, ((w0 + w1) + w2) + w3, and stores one row of partials (wg_partials).
//   Stage 2. One workgroup of 256 threads per column of the partials: thread t adds rows t, t + 256, ... in that order,
//            then the same butterfly and the same four waves (column_sum, column_sums). What follows the sum — a
//            division, a weight, a table update — is the kernel's own epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// butterfly over the 64 lanes (float, double, int64_t): every lane returns the same value
template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// ... its minimum / maximum counterparts (float, double; fmin / fmax pass over a NaN)
template <typename T>
__device__ inline T wave_min(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
template <typename T>
__device__ inline T wave_max(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// The sum over a workgroup of four waves, returned on every thread: lanes by the butterfly, then waves 0, 1, 2, 3 left to
// right. `s_red` holds four values; the leading barrier lets a kernel reuse it from one call to the next.
template <typename T>
__device__ inline T wg_sum(T v, T* s_red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// Stage 1's end: the workgroup's sum of each of K per-lane accumulators (float or double), stored by its first K threads
// to row[k] — the caller passes its own row, partial + blockIdx.x * pitch. One barrier; the bits of K wg_sum calls and a
// store. Its LDS has no leading barrier: one call per kernel. THREADS is the caller's workgroup size: four waves.
template <int THREADS, int K, typename T>
__device__ inline void wg_partials(const T (&a)[K], T* __restrict__ row) {
  static_assert(THREADS == 4 * 64 && K <= 64, "four waves of 64 lanes; the first wave stores");
  __shared__ T s_part[4][K];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) {
    T v = a[k];  // wave_sum's butterfly written out: as a call it is unrolled before it is inlined and the K chains are
                 // scheduled together, which cost pan_bwd_kernel 39 VGPRs and three waves of occupancy
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) s_part[wv][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) row[threadIdx.x] = ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
}

// Stage 2: K neighbouring columns of `nblk` rows of partials, tot[k] = the sum over b of rows[b * stride + k], formed by one
// workgroup and returned on every thread: thread t takes b = t, t + THREADS, ... in that order, then wg_sum per column.
// One trip over the rows serves the K columns (a pass of dependent loads per column is what a final kernel's time is).
// `s_red` as for wg_sum.
template <int THREADS, int K, typename T>
__device__ inline void column_sums(const T* __restrict__ rows, int nblk, size_t stride, T (&tot)[K], T* s_red) {
  static_assert(THREADS == 4 * 64, "four waves of 64 lanes");
  T a[K];
#pragma unroll
  for (int k = 0; k < K; k++) a[k] = 0;
  for (int b = threadIdx.x; b < nblk; b += THREADS) {
#pragma unroll
    for (int k = 0; k < K; k++) a[k] += rows[(size_t)b * stride + k];
  }
#pragma unroll
  for (int k = 0; k < K; k++) tot[k] = wg_sum(a[k], s_red);
}
// ... one column: element b at col[b * stride]
template <int THREADS, typename T>
__device__ inline T column_sum(const T* __restrict__ col, int nblk, size_t stride, T* s_red) {
  T tot[1];
  column_sums<THREADS>(col, nblk, stride, tot, s_red);
  return tot[0];
}

// the float sum on the DPP path: four rotations inside each row of 16 lanes, the row totals handed on by row_bcast15 /
// row_bcast31, lane 63 read back — seven VALU instructions and no LDS round trip (__shfl_xor is a ds_bpermute_b32: six
// dependent ones cost the quad forward 4 % when this sum sat in its chunk loop, profiles/r05_ab_plain_trips.txt)
__device__ inline float wave_sum_dpp(float v) {
#define WS_DPP(x, ctrl, rows) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), ctrl, rows, 0xF, true))
  v += WS_DPP(v, 0x121, 0xF);  // row_ror:1
  v += WS_DPP(v, 0x122, 0xF);  // row_ror:2
  v += WS_DPP(v, 0x124, 0xF);  // row_ror:4
  v += WS_DPP(v, 0x128, 0xF);  // row_ror:8: every lane holds its row's sum
  v += WS_DPP(v, 0x142, 0xA);  // row_bcast15 into rows 1 and 3
  v += WS_DPP(v, 0x143, 0xC);  // row_bcast31 into rows 2 and 3
#undef WS_DPP
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

__device__ inline float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
// ShadowMap.forward's `alt_diff.clip(max=0)` (affine_cameras.py:38) for shade.hip and pan.hip, which must agree to the bit: a clamp
// that keeps a NaN, written as a select (fminf returns its other operand for a NaN). -0 passes, as through torch's clamp.
__device__ inline float shadow_clip(float d) { return d > 0.f ? 0.f : d; }
// reg.hip's opacity terms and monitor.hip's mean opacity must agree to the bit
__device__ inline float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
