// optim.hip — multi-tensor Adam and row compaction for the Gaussian parameter tensors.
// Reference semantics: torch.optim.Adam as configured at src/gaussiansplatting/scene/gaussian_model.py:228-262, and the
// boolean-mask gathers of _prune_optimizer / prune_points (gaussian_model.py:466-505).
// Both are pure HBM streams: Adam reads 16 and writes 12 bytes per element in one launch for all groups; compaction
// reads each kept row once and writes it once, all tensors in one launch, positions from one ballot/prefix scan.
// include/eogs_step.h: the same Adam stream with t and lr read from device scalars (a one-workgroup prologue forms the bias
// corrections), and the single-wave gate over the forwards' count words: the optimizer step inside a recorded graph.
#include "api_util.h"

#define EOGS_COMPACT_MAX_TENSORS 24  // tensors per compaction launch (more are split over launches)

namespace {

constexpr int ADAM_VEC = 4;               // elements per thread
constexpr int ADAM_CHUNK = BLK * ADAM_VEC;  // elements per workgroup

struct AdamTable {
  eogs_adam_tensor t[EOGS_ADAM_MAX_TENSORS];
  uint32_t first_block[EOGS_ADAM_MAX_TENSORS + 1];  // workgroup range of each tensor
  int n;
};

// The elements of one thread, shared by adam_kernel and step_adam_kernel: one body, so equal fp32 scalars give equal bits.
// RETIRE: after the update an element < retire_below is stored as EOGS_STEP_RETIRED_LOGIT (include/eogs_step.h).
template <bool RETIRE>
__device__ __forceinline__ void adam_elements(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ exp_avg,
                                              float* __restrict__ exp_avg_sq, int64_t numel, int64_t i0, float lr, float w1,
                                              float beta2, float w2, float eps, float inv_bc1, float sqrt_bc2, float retire_below) {
  const float step_size = lr * inv_bc1;
  float p[ADAM_VEC], g[ADAM_VEC], m[ADAM_VEC], v[ADAM_VEC];
  const bool full = i0 + ADAM_VEC <= numel && ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg |
                                                 (uintptr_t)exp_avg_sq) & 15u) == 0);
  if (full) {
    const float4 a = *reinterpret_cast<const float4*>(param + i0), b = *reinterpret_cast<const float4*>(grad + i0);
    const float4 c = *reinterpret_cast<const float4*>(exp_avg + i0), d = *reinterpret_cast<const float4*>(exp_avg_sq + i0);
    p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; g[0] = b.x; g[1] = b.y; g[2] = b.z; g[3] = b.w;
    m[0] = c.x; m[1] = c.y; m[2] = c.z; m[3] = c.w; v[0] = d.x; v[1] = d.y; v[2] = d.z; v[3] = d.w;
  } else {
#pragma unroll
    for (int k = 0; k < ADAM_VEC; k++) {
      const bool in = i0 + k < numel;
      p[k] = in ? param[i0 + k] : 0.f; g[k] = in ? grad[i0 + k] : 0.f;
      m[k] = in ? exp_avg[i0 + k] : 0.f; v[k] = in ? exp_avg_sq[i0 + k] : 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < ADAM_VEC; k++) {
    // torch: exp_avg.lerp_(grad, 1-b1); exp_avg_sq.mul_(b2).addcmul_(grad, grad, 1-b2);
    //        denom = exp_avg_sq.sqrt() / sqrt(bc2) + eps; param.addcdiv_(exp_avg, denom, value=-step_size)
    m[k] = m[k] + w1 * (g[k] - m[k]);
    v[k] = v[k] * beta2 + w2 * (g[k] * g[k]);
    const float denom = sqrtf(v[k]) / sqrt_bc2 + eps;
    p[k] = p[k] - step_size * (m[k] / denom);
    if (RETIRE && p[k] < retire_below) p[k] = EOGS_STEP_RETIRED_LOGIT;
  }
  if (full) {
    *reinterpret_cast<float4*>(param + i0) = make_float4(p[0], p[1], p[2], p[3]);
    *reinterpret_cast<float4*>(exp_avg + i0) = make_float4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<float4*>(exp_avg_sq + i0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < ADAM_VEC; k++)
      if (i0 + k < numel) {
        param[i0 + k] = p[k]; exp_avg[i0 + k] = m[k]; exp_avg_sq[i0 + k] = v[k];
      }
  }
}

__global__ __launch_bounds__(BLK) void adam_kernel(AdamTable tab, float w1, float beta2, float w2, float eps, float inv_bc1,
                                                   float sqrt_bc2) {
  // which tensor does this workgroup belong to (n <= 16: linear search on kernel arguments, wave-uniform)
  int ti = 0;
  while (ti + 1 < tab.n && blockIdx.x >= tab.first_block[ti + 1]) ti++;
  const eogs_adam_tensor T = tab.t[ti];
  const int64_t i0 = ((int64_t)(blockIdx.x - tab.first_block[ti]) * BLK + threadIdx.x) * ADAM_VEC;
  if (i0 >= T.numel) return;
  adam_elements<false>(T.param, T.grad, T.exp_avg, T.exp_avg_sq, T.numel, i0, T.lr, w1, beta2, w2, eps, inv_bc1, sqrt_bc2, 0.f);
}

// ---- the step inside a recorded graph (include/eogs_step.h): t and lr are device scalars ----
struct StepPrologueTable {
  const float* lr[EOGS_STEP_MAX_TENSORS];
  float* step[EOGS_STEP_MAX_TENSORS];
  int n;
};

// One workgroup of one wave, lane i = descriptor i. The only launch that writes the step counts, and nothing else reads them
// while it runs: the many workgroups of the element kernel read the table this one leaves in `ws`.
__global__ __launch_bounds__(64) void step_adam_prologue_kernel(StepPrologueTable tab, double beta1, double beta2,
                                                                const uint32_t* __restrict__ gate,
                                                                eogs_step_adam_scalars* __restrict__ ws) {
  const int i = threadIdx.x;
  if (i >= tab.n) return;
  eogs_step_adam_scalars sc;
  sc.lr = *tab.lr[i];
  if (!gate || gate[0] != 0u) {
    float* step = tab.step[i];
    const float t = *step + 1.0f;
    *step = t;
    // bias corrections in double, the expressions of launch_adam
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    sc.inv_bc1 = (float)(1.0 / bc1);
    sc.sqrt_bc2 = (float)sqrt(bc2);
    sc.skip = 0.f;
  } else {
    sc.inv_bc1 = 0.f;
    sc.sqrt_bc2 = 1.f;
    sc.skip = 1.f;
  }
  ws[i] = sc;
}

struct StepAdamTable {
  eogs_step_adam_tensor t[EOGS_STEP_MAX_TENSORS];
  uint32_t first_block[EOGS_STEP_MAX_TENSORS + 1];  // workgroup range of each tensor
  uint8_t slot[EOGS_STEP_MAX_TENSORS];              // which entry of ws is this tensor's (empty tensors have one too)
  int n;
};

__global__ __launch_bounds__(BLK) void step_adam_kernel(StepAdamTable tab, const eogs_step_adam_scalars* __restrict__ ws, float w1,
                                                        float beta2, float w2, float eps) {
  int ti = 0;
  while (ti + 1 < tab.n && blockIdx.x >= tab.first_block[ti + 1]) ti++;
  const eogs_step_adam_scalars sc = ws[tab.slot[ti]];  // (wave-uniform: written by the prologue launch before this one)
  if (sc.skip != 0.f) return;                          // gate closed: no load, no store
  const eogs_step_adam_tensor T = tab.t[ti];
  const int64_t i0 = ((int64_t)(blockIdx.x - tab.first_block[ti]) * BLK + threadIdx.x) * ADAM_VEC;
  if (i0 >= T.numel) return;
  adam_elements<true>(T.param, T.grad, T.exp_avg, T.exp_avg_sq, T.numel, i0, sc.lr, w1, beta2, w2, eps, sc.inv_bc1, sc.sqrt_bc2,
                      T.retire_below);
}

struct GateTable {
  const uint32_t* misc[EOGS_STEP_MAX_FORWARDS];
  uint32_t cap_slots[EOGS_STEP_MAX_FORWARDS], cap_entries[EOGS_STEP_MAX_FORWARDS];
  int n;
};

// One wave, lane i = forward i: reads the count words its forward_prepare wrote, one lane stores the two result words.
__global__ __launch_bounds__(64) void step_gate_kernel(GateTable tab, int accumulate, uint32_t* __restrict__ gate) {
  const int i = threadIdx.x;
  bool bad = false;
  if (i < tab.n) {
    const uint32_t* m = tab.misc[i];
    const uint64_t slots = (uint64_t)m[MISC_TOTAL_LO] | ((uint64_t)m[MISC_TOTAL_HI] << 32);
    const uint64_t entries = (uint64_t)m[MISC_MACRO_LO] | ((uint64_t)m[MISC_MACRO_HI] << 32);
    bad = !capacity_fits(slots, entries, tab.cap_slots[i], tab.cap_entries[i]) || (m[MISC_ERR] & 1u) != 0u;
  }
  const unsigned long long b = __ballot(bad);
  if (threadIdx.x == 0) {
    uint32_t open = b == 0ull ? 1u : 0u, mask = (uint32_t)b;
    if (accumulate) {
      open &= gate[0] != 0u ? 1u : 0u;
      mask |= gate[1];
    }
    gate[0] = open;
    gate[1] = mask;
  }
}

// ---- dst += src0 (+ src1 ...) for several tensors in one launch (include/eogs_optim.h eogs_sum_into) ----
struct SumTable {
  eogs_sum_tensor t[EOGS_SUM_MAX_TENSORS];
  uint32_t first_block[EOGS_SUM_MAX_TENSORS + 1];
  int n, nsrc;
};

__global__ __launch_bounds__(BLK) void sum_into_kernel(SumTable tab) {
  int ti = 0;
  while (ti + 1 < tab.n && blockIdx.x >= tab.first_block[ti + 1]) ti++;
  const eogs_sum_tensor T = tab.t[ti];
  const int64_t i0 = ((int64_t)(blockIdx.x - tab.first_block[ti]) * BLK + threadIdx.x) * ADAM_VEC;
  if (i0 >= T.numel) return;
  uintptr_t al = (uintptr_t)T.dst;
  for (int s = 0; s < tab.nsrc; s++) al |= (uintptr_t)T.src[s];
  if (i0 + ADAM_VEC <= T.numel && (al & 15u) == 0) {
    float4 a = *reinterpret_cast<const float4*>(T.dst + i0);
    for (int s = 0; s < tab.nsrc; s++) {  // (in order: the sum autograd would have made source by source)
      const float4 b = *reinterpret_cast<const float4*>(T.src[s] + i0);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    *reinterpret_cast<float4*>(T.dst + i0) = a;
  } else {
    for (int k = 0; k < ADAM_VEC; k++)
      if (i0 + k < T.numel) {
        float a = T.dst[i0 + k];
        for (int s = 0; s < tab.nsrc; s++) a += T.src[s][i0 + k];
        T.dst[i0 + k] = a;
      }
  }
}

// ---- compaction ----
constexpr int COMPACT_ROWS = BLK;  // rows per workgroup

__global__ __launch_bounds__(BLK) void compact_count_kernel(const uint8_t* __restrict__ keep, int64_t n,
                                                            uint32_t* __restrict__ blk) {
  __shared__ uint32_t s_w[BLK / 64];
  const int64_t i = (int64_t)blockIdx.x * COMPACT_ROWS + threadIdx.x;
  const bool k = i < n && keep[i] != 0;
  const unsigned long long b = __ballot(k);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// single workgroup: exclusive scan of the per-workgroup counts in place, total appended at blk[nblk]
__global__ __launch_bounds__(BLK) void compact_scan_kernel(uint32_t* __restrict__ blk, uint32_t nblk) {
  __shared__ uint32_t s_w[BLK / 64];
  __shared__ uint32_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t b0 = 0; b0 < nblk; b0 += BLK) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nblk ? blk[i] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t nb = __shfl_up(inc, o, 64);
      if (lane >= o) inc += nb;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    const uint32_t pre = (w > 0 ? s_w[0] : 0u) + (w > 1 ? s_w[1] : 0u) + (w > 2 ? s_w[2] : 0u);
    const uint32_t carry = s_carry;
    if (i < nblk) blk[i] = carry + pre + inc - v;
    __syncthreads();
    if (threadIdx.x == BLK - 1) s_carry = carry + pre + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) blk[nblk] = s_carry;
}

struct CompactTable {
  const char* src[EOGS_COMPACT_MAX_TENSORS];
  char* dst[EOGS_COMPACT_MAX_TENSORS];
  int row_words[EOGS_COMPACT_MAX_TENSORS];
  int n;
};

// One workgroup = 256 consecutive rows. The kept rows of the workgroup are consecutive in every destination, so each
// tensor's kept rows are staged in LDS in output order and written as one contiguous run.
__global__ __launch_bounds__(BLK) void compact_apply_kernel(CompactTable tab, const uint8_t* __restrict__ keep, int64_t n,
                                                            const uint32_t* __restrict__ blk) {
  __shared__ uint32_t s_w[BLK / 64];
  __shared__ uint16_t s_srcrow[BLK];  // kept-row rank -> local source row
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * COMPACT_ROWS;
  const int64_t i = row0 + threadIdx.x;
  const bool k = i < n && keep[i] != 0;
  const unsigned long long b = __ballot(k);
  if (lane == 0) s_w[w] = (uint32_t)__popcll(b);
  __syncthreads();
  const uint32_t pre = (w > 0 ? s_w[0] : 0u) + (w > 1 ? s_w[1] : 0u) + (w > 2 ? s_w[2] : 0u);
  const uint32_t kept = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  const uint32_t rank = pre + (uint32_t)__popcll(b & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
  if (k) s_srcrow[rank] = (uint16_t)threadIdx.x;
  __syncthreads();
  if (kept == 0) return;
  const size_t out0 = blk[blockIdx.x];
  for (int t = 0; t < tab.n; t++) {
    const int rw = tab.row_words[t];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tab.src[t]) + (size_t)row0 * rw;
    uint32_t* dst = reinterpret_cast<uint32_t*>(tab.dst[t]) + out0 * rw;
    const uint32_t words = kept * (uint32_t)rw;
    for (uint32_t e = threadIdx.x; e < words; e += BLK) {  // consecutive lanes -> consecutive output words
      const uint32_t r = e / (uint32_t)rw, c = e - r * (uint32_t)rw;
      dst[e] = src[(size_t)s_srcrow[r] * rw + c];
    }
  }
}

struct PackTable {
  eogs_pack_tensor t[EOGS_PACK_MAX_TENSORS];
  int n;
};

// One workgroup = 256 consecutive rows. A tensor's 256 x width block and the bucket's 256 x K block are both contiguous in
// memory, so every global access is a contiguous run (lane = consecutive word); the column shuffle happens in LDS.
// (One lane per row - 14 scalar stores 56 bytes apart per lane - ran at 0.093 ms for 1 M rows, slower than torch.cat.)
#define PACK_MAX_COLS 16
template <bool UNPACK>
__global__ __launch_bounds__(BLK) void pack_columns_kernel(PackTable tab, int64_t rows, float* __restrict__ packed, int K) {
  __shared__ float s_pk[BLK * PACK_MAX_COLS];
  const int64_t row0 = (int64_t)blockIdx.x * BLK;
  const int nrows = (int)((rows - row0) < (int64_t)BLK ? (rows - row0) : (int64_t)BLK);
  float* pblk = packed + (size_t)row0 * K;
  if (UNPACK) {
    for (int e = threadIdx.x; e < nrows * K; e += BLK) s_pk[e] = pblk[e];
    __syncthreads();
  }
  int o = 0;
  for (int t = 0; t < tab.n; t++) {
    const int wd = tab.t[t].width, c0 = tab.t[t].col0, nc = tab.t[t].ncols;
    float* blk = tab.t[t].data + (size_t)row0 * wd;
    for (int e = threadIdx.x; e < nrows * wd; e += BLK) {
      const int r = e / wd, c = e - r * wd - c0;
      if (c >= 0 && c < nc) {
        if (UNPACK) blk[e] = s_pk[r * K + o + c];
        else s_pk[r * K + o + c] = blk[e];
      }
    }
    o += nc;
  }
  if (!UNPACK) {
    __syncthreads();
    for (int e = threadIdx.x; e < nrows * K; e += BLK) pblk[e] = s_pk[e];
  }
}

}  // namespace

// the three table builders: 0, or -1 when the chunks of all tensors exceed one launch's grid
static int launch_adam(int n, const eogs_adam_tensor* tensors, double beta1, double beta2, double eps, int64_t step, hipStream_t s) {
  AdamTable tab;
  tab.n = 0;
  uint64_t blocks = 0;
  for (int i = 0; i < n; i++) {
    if (tensors[i].numel <= 0) continue;
    tab.t[tab.n] = tensors[i];
    tab.first_block[tab.n] = (uint32_t)blocks;
    blocks += (uint64_t)((tensors[i].numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
    tab.n++;
  }
  tab.first_block[tab.n] = (uint32_t)blocks;
  if (tab.n == 0) return 0;
  if (blocks > 0x7FFFFFFFull) return -1;
  // bias corrections in double, like Python floats in torch.optim.adam._single_tensor_adam
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  hipLaunchKernelGGL(adam_kernel, dim3((uint32_t)blocks), dim3(BLK), 0, s, tab, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps, (float)(1.0 / bc1), (float)sqrt(bc2));
  return 0;
}

static int launch_step_adam(int n, const eogs_step_adam_tensor* tensors, double beta1, double beta2, double eps,
                            const uint32_t* gate, eogs_step_adam_scalars* ws, hipStream_t s) {
  StepPrologueTable pro;
  StepAdamTable tab;
  pro.n = n;
  tab.n = 0;
  uint64_t blocks = 0;
  for (int i = 0; i < EOGS_STEP_MAX_TENSORS; i++) {
    pro.lr[i] = i < n ? tensors[i].lr : nullptr;
    pro.step[i] = i < n ? tensors[i].step : nullptr;
    if (i >= n || tensors[i].numel <= 0) continue;
    tab.t[tab.n] = tensors[i];
    tab.slot[tab.n] = (uint8_t)i;
    tab.first_block[tab.n] = (uint32_t)blocks;
    blocks += (uint64_t)((tensors[i].numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
    tab.n++;
  }
  tab.first_block[tab.n] = (uint32_t)blocks;
  if (blocks > 0x7FFFFFFFull) return -1;
  hipLaunchKernelGGL(step_adam_prologue_kernel, dim3(1), dim3(64), 0, s, pro, beta1, beta2, gate, ws);
  if (tab.n == 0) return 0;
  hipLaunchKernelGGL(step_adam_kernel, dim3((uint32_t)blocks), dim3(BLK), 0, s, tab, (const eogs_step_adam_scalars*)ws,
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
  return 0;
}

static int launch_sum_into(int n, const eogs_sum_tensor* tensors, int nsrc, hipStream_t s) {
  SumTable tab;
  tab.n = 0;
  tab.nsrc = nsrc;
  uint64_t blocks = 0;
  for (int i = 0; i < n; i++) {
    if (tensors[i].numel <= 0) continue;
    tab.t[tab.n] = tensors[i];
    tab.first_block[tab.n] = (uint32_t)blocks;
    blocks += (uint64_t)((tensors[i].numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
    tab.n++;
  }
  tab.first_block[tab.n] = (uint32_t)blocks;
  if (tab.n == 0 || nsrc == 0) return 0;
  if (blocks > 0x7FFFFFFFull) return -1;
  hipLaunchKernelGGL(sum_into_kernel, dim3((uint32_t)blocks), dim3(BLK), 0, s, tab);
  return 0;
}

struct CompactWS {
  uint32_t* blk;  // [nblk + 1] kept rows per 256-row workgroup -> exclusive prefix, total at [nblk]
  uint32_t nblk;
  size_t bytes;
};
static CompactWS compact_layout(char* base, int64_t n_rows) {
  CompactWS w;
  w.nblk = (uint32_t)((n_rows + COMPACT_ROWS - 1) / COMPACT_ROWS);
  w.blk = reinterpret_cast<uint32_t*>(base);
  w.bytes = (((size_t)w.nblk + 1) * sizeof(uint32_t) + 255) / 256 * 256 + 256;
  return w;
}

static int compact_check(const char* who, int64_t n_rows, const void* keep, const void* ws, size_t ws_bytes, CompactWS* w) {
  if (n_rows < 0 || n_rows > (int64_t)0x7FFFFFFF * 128) return fail(EOGS_ERR_INVALID_ARG, "%s: bad row count", who);
  if ((n_rows > 0 && !keep) || !ws) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  char* base = ws_base(const_cast<void*>(ws));
  *w = compact_layout(base, n_rows);
  if ((size_t)(base - (const char*)ws) + w->bytes - 256 > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  return EOGS_OK;
}

extern "C" {

// ---- include/eogs_optim.h ----
int eogs_adam_step(int n, const eogs_adam_tensor* tensors, double beta1, double beta2, double eps, int64_t step, void* stream) {
  clear_error();
  if (n < 0 || n > EOGS_ADAM_MAX_TENSORS || (n > 0 && !tensors) || step < 1)
    return fail(EOGS_ERR_INVALID_ARG, "adam_step: bad argument (at most 16 tensors, step >= 1)");
  for (int i = 0; i < n; i++)
    if (tensors[i].numel < 0 || (tensors[i].numel > 0 && (!tensors[i].param || !tensors[i].grad || !tensors[i].exp_avg ||
                                                          !tensors[i].exp_avg_sq)))
      return fail(EOGS_ERR_INVALID_ARG, "adam_step: NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  { ProfScope ps(PS_ADAM, s); rc = launch_adam(n, tensors, beta1, beta2, eps, step, s); }
  if (rc) return fail(EOGS_ERR_OVERFLOW, "adam_step: too many elements for one launch");
  LAUNCH_TRY(s, false, "adam");
  return EOGS_OK;
}

int eogs_sum_into(int n, const eogs_sum_tensor* tensors, int nsrc, void* stream) {
  clear_error();
  if (n < 0 || n > EOGS_SUM_MAX_TENSORS || nsrc < 0 || nsrc > EOGS_SUM_MAX_SOURCES || (n > 0 && !tensors))
    return fail(EOGS_ERR_INVALID_ARG, "sum_into: bad argument (at most 8 tensors with at most 4 sources each)");
  for (int i = 0; i < n; i++) {
    if (tensors[i].numel < 0 || (tensors[i].numel > 0 && !tensors[i].dst)) return fail(EOGS_ERR_INVALID_ARG, "sum_into: NULL tensor");
    for (int k = 0; k < nsrc; k++)
      if (tensors[i].numel > 0 && !tensors[i].src[k]) return fail(EOGS_ERR_INVALID_ARG, "sum_into: NULL source");
  }
  hipStream_t s = (hipStream_t)stream;
  if (launch_sum_into(n, tensors, nsrc, s)) return fail(EOGS_ERR_OVERFLOW, "sum_into: too many elements for one launch");
  LAUNCH_TRY(s, false, "sum_into");
  return EOGS_OK;
}

int eogs_pack_columns(int64_t rows, int n, const eogs_pack_tensor* tensors, float* packed, int packed_cols, int unpack,
                      void* stream) {
  clear_error();
  if (rows < 0 || n < 0 || n > EOGS_PACK_MAX_TENSORS || packed_cols < 0 || packed_cols > 16)
    return fail(EOGS_ERR_INVALID_ARG, "pack_columns: bad sizes");
  if (rows == 0 || n == 0) return EOGS_OK;
  if (!tensors || !packed) return fail(EOGS_ERR_INVALID_ARG, "pack_columns: NULL argument");
  int total = 0;
  PackTable tab;
  tab.n = n;
  for (int i = 0; i < n; i++) {
    const eogs_pack_tensor& t = tensors[i];
    if (!t.data || t.width <= 0 || t.col0 < 0 || t.ncols <= 0 || t.col0 + t.ncols > t.width)
      return fail(EOGS_ERR_INVALID_ARG, "pack_columns: bad tensor descriptor");
    total += t.ncols;
    tab.t[i] = t;
  }
  if (total != packed_cols) return fail(EOGS_ERR_INVALID_ARG, "pack_columns: packed_cols is not the sum of the column counts");
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((rows + BLK - 1) / BLK);
  if (unpack) hipLaunchKernelGGL(pack_columns_kernel<true>, dim3(blocks), dim3(BLK), 0, s, tab, rows, packed, packed_cols);
  else hipLaunchKernelGGL(pack_columns_kernel<false>, dim3(blocks), dim3(BLK), 0, s, tab, rows, packed, packed_cols);
  LAUNCH_TRY(s, false, "pack_columns");
  return EOGS_OK;
}

int eogs_compact_bytes(int64_t n_rows, size_t* bytes) {
  if (n_rows < 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "compact_bytes: bad argument");
  *bytes = compact_layout(nullptr, n_rows).bytes;
  return EOGS_OK;
}

int eogs_compact_plan(int64_t n_rows, const uint8_t* keep, void* ws, size_t ws_bytes, int64_t* n_keep, void* stream) {
  clear_error();
  CompactWS w;
  const int rc = compact_check("compact_plan", n_rows, keep, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (!n_keep) return fail(EOGS_ERR_INVALID_ARG, "compact_plan: NULL n_keep");
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(PS_COMPACT, s);
    if (w.nblk) hipLaunchKernelGGL(compact_count_kernel, dim3(w.nblk), dim3(BLK), 0, s, keep, n_rows, w.blk);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(BLK), 0, s, w.blk, w.nblk);
  }
  LAUNCH_TRY(s, false, "compact_plan");
  uint32_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, w.blk + w.nblk, sizeof total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_keep = (int64_t)total;
  return EOGS_OK;
}

int eogs_compact_apply(int64_t n_rows, const uint8_t* keep, int n_tensors, const void* const* src, void* const* dst,
                       const int* row_bytes, const void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  CompactWS w;
  const int rc = compact_check("compact_apply", n_rows, keep, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (n_tensors < 0 || (n_tensors > 0 && (!src || !dst || !row_bytes))) return fail(EOGS_ERR_INVALID_ARG, "compact_apply: bad tensor list");
  for (int t = 0; t < n_tensors; t++)
    if (row_bytes[t] < 0 || row_bytes[t] > 256 || (row_bytes[t] & 3) || (row_bytes[t] > 0 && n_rows > 0 && (!src[t] || !dst[t])))
      return fail(EOGS_ERR_INVALID_ARG, "compact_apply: row sizes must be multiples of 4 up to 256 bytes, pointers non-NULL");
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(PS_COMPACT, s);
    for (int t0 = 0; t0 < n_tensors; t0 += EOGS_COMPACT_MAX_TENSORS) {
      CompactTable tab;
      tab.n = 0;
      for (int t = t0; t < n_tensors && tab.n < EOGS_COMPACT_MAX_TENSORS; t++) {
        if (row_bytes[t] == 0) continue;
        tab.src[tab.n] = (const char*)src[t];
        tab.dst[tab.n] = (char*)dst[t];
        tab.row_words[tab.n] = row_bytes[t] / 4;
        tab.n++;
      }
      if (tab.n && w.nblk) hipLaunchKernelGGL(compact_apply_kernel, dim3(w.nblk), dim3(BLK), 0, s, tab, keep, n_rows, w.blk);
    }
  }
  LAUNCH_TRY(s, false, "compact_apply");
  return EOGS_OK;
}

// ---- include/eogs_step.h ----
int eogs_step_gate(int n, const eogs_step_forward* fw, int accumulate, uint32_t* gate, void* stream) {
  clear_error();
  if (n < 0 || n > EOGS_STEP_MAX_FORWARDS || (n > 0 && !fw) || !gate)
    return fail(EOGS_ERR_INVALID_ARG, "step_gate: bad argument (at most 16 forwards, a gate)");
  GateTable tab;
  tab.n = n;
  for (int i = 0; i < EOGS_STEP_MAX_FORWARDS; i++) {
    tab.misc[i] = nullptr;
    tab.cap_slots[i] = tab.cap_entries[i] = 0u;
  }
  for (int i = 0; i < n; i++) {
    if (fw[i].P <= 0 || !fw[i].geom || fw[i].capacity < 0) return fail(EOGS_ERR_INVALID_ARG, "step_gate: bad forward descriptor");
    char* base = ws_base(const_cast<void*>(fw[i].geom));
    const GeomWS g = geom_layout(base, fw[i].P);
    if ((size_t)(base - (const char*)fw[i].geom) + g.bytes - 256 > fw[i].geom_bytes)
      return fail(EOGS_ERR_WORKSPACE, "step_gate: geom workspace too small");
    tab.misc[i] = g.misc;  // each forward's count words
    tab.cap_slots[i] = nr_slots(fw[i].capacity);
    tab.cap_entries[i] = nr_entries(fw[i].capacity);
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(step_gate_kernel, dim3(1), dim3(64), 0, s, tab, accumulate, gate);
  LAUNCH_TRY(s, false, "step_gate");
  return EOGS_OK;
}

int eogs_step_adam_bytes(int n, size_t* bytes) {
  if (n < 0 || n > EOGS_STEP_MAX_TENSORS || !bytes) return fail(EOGS_ERR_INVALID_ARG, "step_adam_bytes: bad argument (at most 16 tensors)");
  *bytes = (size_t)n * sizeof(eogs_step_adam_scalars);
  return EOGS_OK;
}

int eogs_step_adam(int n, const eogs_step_adam_tensor* tensors, double beta1, double beta2, double eps, const uint32_t* gate,
                   void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (n < 0 || n > EOGS_STEP_MAX_TENSORS) return fail(EOGS_ERR_INVALID_ARG, "step_adam: bad argument (at most 16 tensors)");
  if (n == 0) return EOGS_OK;
  if (!tensors) return fail(EOGS_ERR_INVALID_ARG, "step_adam: NULL tensors");
  for (int i = 0; i < n; i++) {
    const eogs_step_adam_tensor& t = tensors[i];
    if (t.numel < 0 || !t.lr || !t.step || (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)))
      return fail(EOGS_ERR_INVALID_ARG, "step_adam: NULL tensor member");
  }
  if (!ws || ws_bytes < (size_t)n * sizeof(eogs_step_adam_scalars)) return fail(EOGS_ERR_WORKSPACE, "step_adam: workspace too small");
  if ((uintptr_t)ws & 15u) return fail(EOGS_ERR_INVALID_ARG, "step_adam: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  { ProfScope ps(PS_ADAM, s); rc = launch_step_adam(n, tensors, beta1, beta2, eps, gate, (eogs_step_adam_scalars*)ws, s); }
  if (rc) return fail(EOGS_ERR_OVERFLOW, "step_adam: too many elements for one launch");
  LAUNCH_TRY(s, false, "step_adam");
  return EOGS_OK;
}

}  // extern "C"
