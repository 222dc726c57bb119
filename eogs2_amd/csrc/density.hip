// density.hip — adaptive density control on the Gaussian parameter tensors (include/eogs_density.h).
// Reference semantics: the statistics of train_pan.py:679-690 / gaussian_model.py:719-723 and GaussianModel.densify_and_prune
// (gaussian_model.py:685-717 with :625-660, :573-623, :541-571, :488-505) computed from the P ORIGINAL rows:
//   stats_kernel   one lane per row, ~40 B per row (12 gradient, 4 radius, 3 x 8 statistics), no nonzero() and no gather
//   decide_kernel  one flag byte per row + per-workgroup counts of the four kinds of output rows
//   scan_kernel    exclusive prefixes of those counts (one workgroup per kind), totals behind them: the ONE host readback
//   build_kernel   one workgroup = 256 consecutive original rows; each of its three output segments (kept rows, kept
//                  clones, kept samples per copy) is one contiguous run in every tensor — the shape of compact_apply_kernel
// No atomics anywhere: ranks come from ballots, offsets from the scan. The build (-ffp-contract=off) keeps every product
// and sum of the 3 x 3 rotation rounded on its own, as the reference's elementwise build_rotation does.
#include "api_util.h"

namespace {

constexpr int DROWS = BLK;  // rows per workgroup of decide / build

template <bool RADII_F32>
__global__ __launch_bounds__(BLK) void density_stats_kernel(int64_t P, const float* __restrict__ vg, const void* __restrict__ radii,
                                                            float* __restrict__ accum, float* __restrict__ denom,
                                                            float* __restrict__ maxr) {
  const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= P) return;
  const float r = RADII_F32 ? static_cast<const float*>(radii)[i] : (float)static_cast<const int32_t*>(radii)[i];
  if (!(r > 0.f)) return;  // every other row keeps its bits
  const float gx = vg[3 * i], gy = vg[3 * i + 1];
  const float m = maxr[i];
  maxr[i] = r > m ? r : m;  // torch.max: a NaN statistic stays NaN
  accum[i] += sqrtf(gx * gx + gy * gy);
  denom[i] += 1.f;
}

__device__ inline float max_nan(float a, float b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }  // torch.max

// the four kinds of output rows a flag byte stands for (the order of the counts, EOGS_DENSITY_N_*)
__device__ inline void kinds_of(uint32_t f, bool in, bool k[4]) {
  k[0] = in && !(f & EOGS_DENSITY_SPLIT) && !(f & EOGS_DENSITY_PRUNE_SELF);
  k[1] = in && (f & EOGS_DENSITY_CLONE) && !(f & EOGS_DENSITY_PRUNE_SELF);
  k[2] = in && (f & EOGS_DENSITY_SPLIT);
  k[3] = in && (f & EOGS_DENSITY_SPLIT) && !(f & EOGS_DENSITY_PRUNE_SAMP);
}

__global__ __launch_bounds__(BLK) void density_decide_kernel(int64_t P, const float* __restrict__ accum, const float* __restrict__ denom,
                                                             const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                             float thr_grad, float thr_dense, float min_opacity, int use_screen,
                                                             float thr_big, float split_div, uint8_t* __restrict__ flags,
                                                             uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_w[4][BLK / 64];
  const int64_t i = (int64_t)blockIdx.x * DROWS + threadIdx.x;
  const bool in = i < P;
  uint32_t f = 0;
  if (in) {
    float g = accum[i] / denom[i];  // IEEE division
    if (g != g) g = 0.f;
    const float e0 = expf(scaling[3 * i]), e1 = expf(scaling[3 * i + 1]), e2 = expf(scaling[3 * i + 2]);
    const float smax = max_nan(max_nan(e0, e1), e2);
    const float o = opacity[i];
    const bool sel = g >= thr_grad && !(o <= EOGS_DENSITY_RETIRED_BELOW);
    const bool low = 1.f / (1.f + expf(-o)) < min_opacity;
    bool big_self = false, big_samp = false;
    if (use_screen) {
      big_self = smax > thr_big;
      // the reference stores log(exp(s) / (0.8 N)) and activates it again for the final prune: the same round trip
      const float t0 = expf(logf(e0 / split_div)), t1 = expf(logf(e1 / split_div)), t2 = expf(logf(e2 / split_div));
      big_samp = max_nan(max_nan(t0, t1), t2) > thr_big;
    }
    if (sel && smax <= thr_dense) f |= EOGS_DENSITY_CLONE;
    if (sel && smax > thr_dense) f |= EOGS_DENSITY_SPLIT;
    if (low || big_self) f |= EOGS_DENSITY_PRUNE_SELF;
    if (low || big_samp) f |= EOGS_DENSITY_PRUNE_SAMP;
    flags[i] = (uint8_t)f;
  }
  bool k[4];
  kinds_of(f, in, k);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const unsigned long long b = __ballot(k[j]);
    if ((threadIdx.x & 63) == 0) s_w[j][threadIdx.x >> 6] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x < 4) cnt[4 * (size_t)blockIdx.x + threadIdx.x] = s_w[threadIdx.x][0] + s_w[threadIdx.x][1] + s_w[threadIdx.x][2] + s_w[threadIdx.x][3];
}

// workgroup k: exclusive scan in place of the counts of kind k (cnt[4 b + k], b < nblk), the total at cnt[4 nblk + k]
__global__ __launch_bounds__(BLK) void density_scan_kernel(uint32_t* __restrict__ cnt, uint32_t nblk) {
  __shared__ uint32_t s_w[BLK / 64];
  __shared__ uint32_t s_carry;
  const uint32_t kind = blockIdx.x;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t b0 = 0; b0 < nblk; b0 += BLK) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nblk ? cnt[4 * (size_t)i + kind] : 0u;
    const uint32_t inc = wave_incl_scan_u32(v);
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    const uint32_t pre = (w > 0 ? s_w[0] : 0u) + (w > 1 ? s_w[1] : 0u) + (w > 2 ? s_w[2] : 0u);
    const uint32_t carry = s_carry;
    if (i < nblk) cnt[4 * (size_t)i + kind] = carry + pre + inc - v;
    __syncthreads();
    if (threadIdx.x == BLK - 1) s_carry = carry + pre + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) cnt[4 * (size_t)nblk + kind] = s_carry;
}

#define DENSITY_TENSORS_PER_LAUNCH 24
struct BuildTable {
  const uint32_t* src[DENSITY_TENSORS_PER_LAUNCH];
  uint32_t* dst[DENSITY_TENSORS_PER_LAUNCH];
  uint16_t row_words[DENSITY_TENSORS_PER_LAUNCH];
  uint16_t kind[DENSITY_TENSORS_PER_LAUNCH];
  int n;
};

// `rows` output rows of rw words: row r is source row map[r] of the workgroup's block (or zeros), consecutive lanes ->
// consecutive output words
__device__ inline void write_run(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, const uint16_t* map, uint32_t rows,
                                 uint32_t rw, bool zero) {
  const uint32_t words = rows * rw;
  for (uint32_t e = threadIdx.x; e < words; e += BLK) {
    const uint32_t r = e / rw, c = e - r * rw;
    dst[e] = zero ? 0u : src[(size_t)map[r] * rw + c];
  }
}

__global__ __launch_bounds__(BLK) void density_build_kernel(BuildTable tab, int64_t P, int N, const uint8_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ pre, uint32_t nA, uint32_t nB, uint32_t nS,
                                                            uint32_t nC, const float* __restrict__ rotation,
                                                            const float* __restrict__ samples, float split_div) {
  __shared__ uint32_t s_w[4][BLK / 64];
  __shared__ uint16_t s_map[3][BLK];  // rank inside the workgroup's segment -> local source row: kept, kept clones, kept split
  __shared__ uint16_t s_srank[BLK];   // kept split rank -> rank among the workgroup's split-selected rows (the sample's row)
  __shared__ float s_stage[BLK * 3];  // computed rows of one copy, in output order
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * DROWS;
  const int64_t i = row0 + threadIdx.x;
  const bool in = i < P;
  const uint32_t f = in ? flags[i] : 0u;
  bool k[4];
  kinds_of(f, in, k);
  unsigned long long b[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    b[j] = __ballot(k[j]);
    if (lane == 0) s_w[j][w] = (uint32_t)__popcll(b[j]);
  }
  __syncthreads();
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  uint32_t rank[4], total[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    rank[j] = (w > 0 ? s_w[j][0] : 0u) + (w > 1 ? s_w[j][1] : 0u) + (w > 2 ? s_w[j][2] : 0u) + (uint32_t)__popcll(b[j] & below);
    total[j] = s_w[j][0] + s_w[j][1] + s_w[j][2] + s_w[j][3];
  }
  if (k[0]) s_map[0][rank[0]] = (uint16_t)threadIdx.x;
  if (k[1]) s_map[1][rank[1]] = (uint16_t)threadIdx.x;
  if (k[3]) {
    s_map[2][rank[3]] = (uint16_t)threadIdx.x;
    s_srank[rank[3]] = (uint16_t)rank[2];
  }
  __syncthreads();
  const size_t outA = pre[4 * (size_t)blockIdx.x + 0];
  const size_t outB = (size_t)nA + pre[4 * (size_t)blockIdx.x + 1];
  const size_t preS = pre[4 * (size_t)blockIdx.x + 2];
  const size_t preC = pre[4 * (size_t)blockIdx.x + 3];
  for (int t = 0; t < tab.n; t++) {
    const uint32_t rw = tab.row_words[t], kind = tab.kind[t];
    const uint32_t* src = tab.src[t] + (size_t)row0 * rw;
    uint32_t* dst = tab.dst[t];
    const bool zero_new = kind == EOGS_DENSITY_ZERO;
    write_run(dst + outA * rw, src, s_map[0], total[0], rw, false);
    write_run(dst + outB * rw, src, s_map[1], total[1], rw, zero_new);
    if (total[3] == 0) continue;  // (uniform over the workgroup, like everything that guards a barrier below)
    for (int c = 0; c < N; c++) {
      uint32_t* d = dst + ((size_t)nA + nB + (size_t)c * nC + preC) * rw;
      if (kind == EOGS_DENSITY_XYZ || kind == EOGS_DENSITY_SCALING) {
        __syncthreads();  // the stage of the copy (or tensor) before is written out
        if (threadIdx.x < total[3]) {
          const uint32_t lr = s_map[2][threadIdx.x];
          const float* v = reinterpret_cast<const float*>(src) + (size_t)lr * 3;
          float o0, o1, o2;
          if (kind == EOGS_DENSITY_SCALING) {
            o0 = logf(expf(v[0]) / split_div);
            o1 = logf(expf(v[1]) / split_div);
            o2 = logf(expf(v[2]) / split_div);
          } else {
            // utils/general_utils.py:82-105 build_rotation on the raw quaternion, then R . sample + xyz
            const float* q = rotation + (size_t)(row0 + lr) * 4;
            const float* sm = samples + ((size_t)c * nS + preS + s_srank[threadIdx.x]) * 3;
            const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            const float r = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
            const float s0 = sm[0], s1 = sm[1], s2 = sm[2];
            o0 = ((1.f - 2.f * (y * y + z * z)) * s0 + (2.f * (x * y - r * z)) * s1 + (2.f * (x * z + r * y)) * s2) + v[0];
            o1 = ((2.f * (x * y + r * z)) * s0 + (1.f - 2.f * (x * x + z * z)) * s1 + (2.f * (y * z - r * x)) * s2) + v[1];
            o2 = ((2.f * (x * z - r * y)) * s0 + (2.f * (y * z + r * x)) * s1 + (1.f - 2.f * (x * x + y * y)) * s2) + v[2];
          }
          s_stage[threadIdx.x * 3 + 0] = o0;
          s_stage[threadIdx.x * 3 + 1] = o1;
          s_stage[threadIdx.x * 3 + 2] = o2;
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < total[3] * 3u; e += BLK) d[e] = __float_as_uint(s_stage[e]);
      } else {
        write_run(d, src, s_map[2], total[3], rw, zero_new);
      }
    }
  }
}

// the split-selected rows of one tensor, in order: the workgroup's rows are one contiguous run of the destination
__global__ __launch_bounds__(BLK) void density_split_rows_kernel(int64_t P, const uint8_t* __restrict__ flags,
                                                                 const uint32_t* __restrict__ pre, const uint32_t* __restrict__ src,
                                                                 uint32_t* __restrict__ dst, uint32_t rw) {
  __shared__ uint32_t s_w[BLK / 64];
  __shared__ uint16_t s_map[BLK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * DROWS;
  const int64_t i = row0 + threadIdx.x;
  const bool k = i < P && (flags[i] & EOGS_DENSITY_SPLIT);
  const unsigned long long b = __ballot(k);
  if (lane == 0) s_w[w] = (uint32_t)__popcll(b);
  __syncthreads();
  const uint32_t rank = (w > 0 ? s_w[0] : 0u) + (w > 1 ? s_w[1] : 0u) + (w > 2 ? s_w[2] : 0u) +
                        (uint32_t)__popcll(b & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
  const uint32_t total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  if (k) s_map[rank] = (uint16_t)threadIdx.x;
  __syncthreads();
  write_run(dst + (size_t)pre[4 * (size_t)blockIdx.x + 2] * rw, src + (size_t)row0 * rw, s_map, total, rw, false);
}

}  // namespace

struct DensityWS {
  uint32_t* cnt;  // [nblk + 1][4] rows of the four kinds per 256-row workgroup -> exclusive prefixes, totals at [nblk]
  uint32_t nblk;
  size_t bytes;
};
static DensityWS density_layout(char* base, int64_t P) {
  DensityWS w;
  w.nblk = (uint32_t)((P + DROWS - 1) / DROWS);
  w.cnt = reinterpret_cast<uint32_t*>(base);
  w.bytes = (((size_t)w.nblk + 1) * 4 * sizeof(uint32_t) + 255) / 256 * 256 + 256;
  return w;
}

static void launch_density_build(const DensityWS& w, int64_t P, int N, const uint8_t* flags, const int64_t* counts, int n_tensors,
                          const eogs_density_tensor* tensors, const float* rotation, const float* samples, float split_div,
                          hipStream_t s) {
  if (!w.nblk) return;
  int t = 0;
  while (t < n_tensors) {
    BuildTable tab;
    tab.n = 0;
    for (; t < n_tensors && tab.n < DENSITY_TENSORS_PER_LAUNCH; t++) {
      if (tensors[t].row_bytes == 0) continue;
      tab.src[tab.n] = static_cast<const uint32_t*>(tensors[t].src);
      tab.dst[tab.n] = static_cast<uint32_t*>(tensors[t].dst);
      tab.row_words[tab.n] = (uint16_t)(tensors[t].row_bytes / 4);
      tab.kind[tab.n] = (uint16_t)tensors[t].kind;
      tab.n++;
    }
    if (tab.n)
      hipLaunchKernelGGL(density_build_kernel, dim3(w.nblk), dim3(BLK), 0, s, tab, P, N, flags, w.cnt, (uint32_t)counts[0],
                         (uint32_t)counts[1], (uint32_t)counts[2], (uint32_t)counts[3], rotation, samples, split_div);
  }
}

static int density_check(const char* who, int64_t P, const void* flags, const void* ws, size_t ws_bytes, DensityWS* w) {
  if (P < 0 || P > EOGS_DENSITY_MAX_ROWS) return fail(EOGS_ERR_INVALID_ARG, "%s: bad row count", who);
  if ((P > 0 && !flags) || !ws) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  char* base = ws_base(const_cast<void*>(ws));
  *w = density_layout(base, P);
  if ((size_t)(base - (const char*)ws) + w->bytes - 256 > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  return EOGS_OK;
}

extern "C" {

int eogs_density_stats_update(int64_t P, const float* viewspace_grad, const void* radii, int radii_is_float,
                              float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream) {
  clear_error();
  if (P < 0 || P > EOGS_DENSITY_MAX_ROWS) return fail(EOGS_ERR_INVALID_ARG, "density_stats_update: bad row count");
  if (P > 0 && (!viewspace_grad || !radii || !xyz_gradient_accum || !denom || !max_radii2D))
    return fail(EOGS_ERR_INVALID_ARG, "density_stats_update: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((P + BLK - 1) / BLK);
  if (P > 0 && radii_is_float)
    hipLaunchKernelGGL(density_stats_kernel<true>, dim3(blocks), dim3(BLK), 0, s, P, viewspace_grad, radii, xyz_gradient_accum, denom,
                       max_radii2D);
  else if (P > 0)
    hipLaunchKernelGGL(density_stats_kernel<false>, dim3(blocks), dim3(BLK), 0, s, P, viewspace_grad, radii, xyz_gradient_accum, denom,
                       max_radii2D);
  LAUNCH_TRY(s, false, "density_stats_update");
  return EOGS_OK;
}

int eogs_density_bytes(int64_t P, size_t* bytes) {
  clear_error();
  if (P < 0 || P > EOGS_DENSITY_MAX_ROWS || !bytes) return fail(EOGS_ERR_INVALID_ARG, "density_bytes: bad argument");
  *bytes = density_layout(nullptr, P).bytes;
  return EOGS_OK;
}

int eogs_density_decide(int64_t P, const float* xyz_gradient_accum, const float* denom, const float* opacity,
                        const float* scaling, float grad_threshold, float dense_threshold, float min_opacity, int use_screen,
                        float big_threshold, float split_div, uint8_t* flags, void* ws, size_t ws_bytes, int64_t* counts,
                        void* stream) {
  clear_error();
  DensityWS w;
  const int rc = density_check("density_decide", P, flags, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (!counts) return fail(EOGS_ERR_INVALID_ARG, "density_decide: NULL counts");
  if (P > 0 && (!xyz_gradient_accum || !denom || !opacity || !scaling)) return fail(EOGS_ERR_INVALID_ARG, "density_decide: NULL argument");
  if (!(split_div > 0.f)) return fail(EOGS_ERR_INVALID_ARG, "density_decide: split_div must be positive");
  hipStream_t s = (hipStream_t)stream;
  if (w.nblk)
    hipLaunchKernelGGL(density_decide_kernel, dim3(w.nblk), dim3(BLK), 0, s, P, xyz_gradient_accum, denom, opacity, scaling,
                       grad_threshold, dense_threshold, min_opacity, use_screen, big_threshold, split_div, flags, w.cnt);
  hipLaunchKernelGGL(density_scan_kernel, dim3(4), dim3(BLK), 0, s, w.cnt, w.nblk);
  LAUNCH_TRY(s, false, "density_decide");
  uint32_t total[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(total, w.cnt + 4 * (size_t)w.nblk, sizeof total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 4; k++) counts[k] = (int64_t)total[k];
  return EOGS_OK;
}

int eogs_density_split_rows(int64_t P, const uint8_t* flags, const void* src, void* dst, int row_bytes, const void* ws,
                            size_t ws_bytes, void* stream) {
  clear_error();
  DensityWS w;
  const int rc = density_check("density_split_rows", P, flags, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (row_bytes < 0 || row_bytes > 256 || (row_bytes & 3))
    return fail(EOGS_ERR_INVALID_ARG, "density_split_rows: row sizes must be multiples of 4 up to 256 bytes");
  if (row_bytes > 0 && P > 0 && (!src || !dst)) return fail(EOGS_ERR_INVALID_ARG, "density_split_rows: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  if (w.nblk && row_bytes != 0)
    hipLaunchKernelGGL(density_split_rows_kernel, dim3(w.nblk), dim3(BLK), 0, s, P, flags, w.cnt, static_cast<const uint32_t*>(src),
                       static_cast<uint32_t*>(dst), (uint32_t)(row_bytes / 4));
  LAUNCH_TRY(s, false, "density_split_rows");
  return EOGS_OK;
}

int eogs_density_build(int64_t P, int N, const uint8_t* flags, const int64_t* counts, int n_tensors,
                       const eogs_density_tensor* tensors, const float* rotation, const float* samples, float split_div,
                       const void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  DensityWS w;
  const int rc = density_check("density_build", P, flags, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (N < 1 || N > EOGS_DENSITY_MAX_N) return fail(EOGS_ERR_INVALID_ARG, "density_build: N out of range");
  if (!counts) return fail(EOGS_ERR_INVALID_ARG, "density_build: NULL counts");
  for (int k = 0; k < 4; k++)
    if (counts[k] < 0 || counts[k] > P) return fail(EOGS_ERR_INVALID_ARG, "density_build: counts are not those of density_decide on these rows");
  if (counts[EOGS_DENSITY_N_KEPT_SPLIT] > counts[EOGS_DENSITY_N_SPLIT] || counts[EOGS_DENSITY_N_KEPT] + counts[EOGS_DENSITY_N_SPLIT] > P)
    return fail(EOGS_ERR_INVALID_ARG, "density_build: counts are not those of density_decide on these rows");
  if (n_tensors < 0 || (n_tensors > 0 && !tensors)) return fail(EOGS_ERR_INVALID_ARG, "density_build: bad tensor list");
  if (!(split_div > 0.f)) return fail(EOGS_ERR_INVALID_ARG, "density_build: split_div must be positive");
  const int64_t n_out = counts[0] + counts[1] + (int64_t)N * counts[3];
  bool computed = false;
  for (int t = 0; t < n_tensors; t++) {
    const eogs_density_tensor& T = tensors[t];
    if (T.row_bytes < 0 || T.row_bytes > 256 || (T.row_bytes & 3))
      return fail(EOGS_ERR_INVALID_ARG, "density_build: row sizes must be multiples of 4 up to 256 bytes");
    if (T.kind < EOGS_DENSITY_COPY || T.kind > EOGS_DENSITY_SCALING) return fail(EOGS_ERR_INVALID_ARG, "density_build: unknown tensor kind");
    if ((T.kind == EOGS_DENSITY_XYZ || T.kind == EOGS_DENSITY_SCALING) && T.row_bytes != 12)
      return fail(EOGS_ERR_INVALID_ARG, "density_build: xyz and scaling rows hold three floats");
    if (T.row_bytes > 0 && ((P > 0 && !T.src) || (n_out > 0 && !T.dst))) return fail(EOGS_ERR_INVALID_ARG, "density_build: NULL tensor pointer");
    computed = computed || T.kind == EOGS_DENSITY_XYZ;
  }
  if (computed && counts[EOGS_DENSITY_N_KEPT_SPLIT] > 0 && (!rotation || !samples))
    return fail(EOGS_ERR_INVALID_ARG, "density_build: split rows need rotation and samples (NULL argument)");
  hipStream_t s = (hipStream_t)stream;
  launch_density_build(w, P, N, flags, counts, n_tensors, tensors, rotation, samples, split_div, s);
  LAUNCH_TRY(s, false, "density_build");
  return EOGS_OK;
}

}  // extern "C"
