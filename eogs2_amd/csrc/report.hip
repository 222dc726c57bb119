// report.hip — the end of a run and the inference side (include/eogs_report.h): the colour alignment before the final save
// (utils/save_utils.py:10-33), the train -> test colour-correction converters (utils/convert_color_correction.py), the L1 / PSNR
// sums of training_report (train_pan.py:942-943) and the packing of a view's products into file layout (render_pan.py,
// render_video.py:138-164).
//
// normalize_rows streams P x 3 floats once, in place: HBM-bound, four rows (three 16-byte accesses) per lane. recompose and
// cc_to_test are one wave over a few hundred bytes: latency-bound by construction; their point is that nothing on the host
// waits and no tensor is replaced. The metrics read two images once: HBM-bound, a lane per pixel in a grid-stride loop, double
// sums per workgroup and then by one workgroup in index order. pack reads planes and writes pixels, a lane per pixel:
// the reads are coalesced per plane, the writes of a wave cover one contiguous range.
#include "api_util.h"
#include "reduce.h"
#include "report_cc.h"
#include "eogs_report.h"

namespace {

constexpr int RT = 256;         // threads per workgroup
constexpr int RMAXBLK = 1024;   // workgroups of the metrics' first launch
constexpr int RK = 8;           // doubles per workgroup partial: sum |d| and sum d^2 for up to four channels
constexpr int PACK_PER_WG = 4;  // pixels per lane of pack
constexpr float SH_C0 = 0.28209479177387814f;

// ---- colour alignment: rows ---------------------------------------------------------------------------------------------
struct CC {
  float A[9], b[3];
};

__device__ __forceinline__ void normalize_row(const CC& m, float& f0, float& f1, float& f2) {
  const float c0 = f0 * SH_C0 + 0.5f, c1 = f1 * SH_C0 + 0.5f, c2 = f2 * SH_C0 + 0.5f;  // SH2RGB
  const float r0 = ((m.A[0] * c0 + m.A[1] * c1) + m.A[2] * c2) + m.b[0];
  const float r1 = ((m.A[3] * c0 + m.A[4] * c1) + m.A[5] * c2) + m.b[1];
  const float r2 = ((m.A[6] * c0 + m.A[7] * c1) + m.A[8] * c2) + m.b[2];
  f0 = (r0 - 0.5f) / SH_C0;  // RGB2SH
  f1 = (r1 - 0.5f) / SH_C0;
  f2 = (r2 - 0.5f) / SH_C0;
}

// grid: ceil(ceil(P / 4) / RT). A lane takes rows 4 q .. 4 q + 3: 12 floats, three 16-byte accesses when `vec` (f_dc 16-byte
// aligned), all loaded before the first store; the last lane's missing rows and the unaligned case go float by float.
__global__ __launch_bounds__(RT) void report_rows_kernel(int64_t P, float* f, const float* __restrict__ A1, const float* __restrict__ b1, int vec) {
  CC m;
#pragma unroll
  for (int i = 0; i < 9; i++) m.A[i] = A1[i];  // (wave-uniform addresses: scalar loads)
#pragma unroll
  for (int i = 0; i < 3; i++) m.b[i] = b1[i];
  const int64_t q = (int64_t)blockIdx.x * RT + threadIdx.x;
  const int64_t row0 = q * 4;
  if (row0 >= P) return;
  if (vec && row0 + 4 <= P) {
    float4* p = reinterpret_cast<float4*>(f + row0 * 3);
    float4 a = p[0], b = p[1], c = p[2];
    normalize_row(m, a.x, a.y, a.z);
    normalize_row(m, a.w, b.x, b.y);
    normalize_row(m, b.z, b.w, c.x);
    normalize_row(m, c.y, c.z, c.w);
    p[0] = a;
    p[1] = b;
    p[2] = c;
    return;
  }
  const int64_t row1 = row0 + 4 < P ? row0 + 4 : P;
  for (int64_t r = row0; r < row1; r++) {
    float x = f[r * 3], y = f[r * 3 + 1], z = f[r * 3 + 2];
    normalize_row(m, x, y, z);
    f[r * 3] = x;
    f[r * 3 + 1] = y;
    f[r * 3 + 2] = z;
  }
}

// ---- colour alignment: cameras --------------------------------------------------------------------------------------------
struct CameraTable {
  eogs_report_camera cam[EOGS_REPORT_MAX_CAMERAS];
};

// One wave, lane i camera i. ref_w / ref_b usually ARE one camera's tensors, so nothing here is __restrict__. Every lane's
// stores take values computed from its loads of A1 and b1, and the wave's lanes run one instruction at a time: the wave waits
// for ALL lanes' loads before the first store is issued, so every camera sees the original A1 and b1.
__global__ __launch_bounds__(64) void report_recompose_kernel(int n, CameraTable T, const float* ref_w, const float* ref_b) {
  if (blockIdx.x != 0) return;
  const int t = (int)threadIdx.x;
  float A1[9], b1[3];
#pragma unroll
  for (int i = 0; i < 9; i++) A1[i] = ref_w[i];
#pragma unroll
  for (int i = 0; i < 3; i++) b1[i] = ref_b[i];
  if (t >= n) return;
  float* w = T.cam[t].weight;
  float* b = T.cam[t].bias;
  float Ai[9], bi[3], oA[9], ob[3];
#pragma unroll
  for (int i = 0; i < 9; i++) Ai[i] = w[i];
#pragma unroll
  for (int i = 0; i < 3; i++) bi[i] = b[i];
  report_recompose(Ai, bi, A1, b1, oA, ob);
#pragma unroll
  for (int i = 0; i < 9; i++) w[i] = oA[i];
#pragma unroll
  for (int i = 0; i < 3; i++) b[i] = ob[i];
}

// ---- train -> test colour correction ---------------------------------------------------------------------------------------
// One wave, lane e element e of (weight, bias). AVERAGE: torch.zeros_like, += per camera in order, /= len (fp32, a division).
__global__ __launch_bounds__(64) void report_cc_to_test_kernel(int mode, int n_train, CameraTable train, int n_test, CameraTable test,
                                                               int w_elems, int b_elems) {
  if (blockIdx.x != 0) return;
  const int e = (int)threadIdx.x;
  if (e >= w_elems + b_elems) return;
  const bool is_w = e < w_elems;
  const int k = is_w ? e : e - w_elems;
  float v;
  if (mode == EOGS_REPORT_CC_REF) {
    v = is_w ? train.cam[0].weight[k] : train.cam[0].bias[k];
  } else {
    v = 0.f;
    for (int c = 0; c < n_train; c++) v += is_w ? train.cam[c].weight[k] : train.cam[c].bias[k];
    v = v / (float)n_train;
  }
  for (int c = 0; c < n_test; c++) {
    if (is_w) test.cam[c].weight[k] = v;
    else test.cam[c].bias[k] = v;
  }
}

// ---- report metrics -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float clamp01_keep_nan(float g) { return g < 0.f ? 0.f : (g > 1.f ? 1.f : g); }  // torch.clamp

template <int C>
__global__ __launch_bounds__(RT) void report_metrics_partial_kernel(int64_t n, const float* __restrict__ image, const float* __restrict__ gt,
                                                                    double* __restrict__ partial) {
  double a[2 * C];  // sum |d| and sum d^2, channel by channel
#pragma unroll
  for (int k = 0; k < 2 * C; k++) a[k] = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * RT + threadIdx.x; p < n; p += (int64_t)gridDim.x * RT) {
#pragma unroll
    for (int k = 0; k < C; k++) {
      const double d = (double)image[k * n + p] - (double)clamp01_keep_nan(gt[k * n + p]);  // exact in double
      a[2 * k] += fabs(d);
      a[2 * k + 1] += d * d;
    }
  }
  wg_partials<RT>(a, partial + (size_t)blockIdx.x * RK);
}

// one workgroup: the partials column by column in index order, then the view's two figures and the table
__global__ __launch_bounds__(RT) void report_metrics_final_kernel(int C, int64_t n, const double* __restrict__ partial, int nblk, int kind,
                                                                  eogs_report_table* __restrict__ table, const uint32_t* __restrict__ gate) {
  __shared__ double s_red[4];
  if (blockIdx.x != 0) return;
  if (gate != nullptr && gate[0] == 0u) return;  // (uniform over the workgroup)
  double tot[RK];
#pragma unroll
  for (int k = 0; k < RK; k++) {
    tot[k] = 0.0;
    if (k < 2 * C) tot[k] = column_sum<RT>(partial + k, nblk, RK, s_red);  // (uniform)
  }
  if (threadIdx.x != 0) return;
  double sum_abs = 0.0, sum_psnr = 0.0;
#pragma unroll
  for (int k = 0; k < EOGS_REPORT_MAX_CHANNELS; k++) {
    if (k < C) {
      sum_abs += tot[2 * k];
      const double mse = tot[2 * k + 1] / (double)n;
      sum_psnr += 20.0 * log10(1.0 / sqrt(mse));  // mse 0: +inf
    }
  }
  const float l1 = (float)(sum_abs / ((double)C * (double)n));
  const float psnr = (float)(sum_psnr / (double)C);
  table->l1[kind] += (double)l1;
  table->psnr[kind] += (double)psnr;
  table->views[kind] += 1;
  table->last_l1 = l1;
  table->last_psnr = psnr;
}

__global__ __launch_bounds__(64) void report_metrics_reset_kernel(eogs_report_table* table) {
  if (blockIdx.x != 0) return;
  uint64_t* w = reinterpret_cast<uint64_t*>(table);
  if (threadIdx.x < sizeof(eogs_report_table) / 8) w[threadIdx.x] = 0ull;
}

// ---- product packing -----------------------------------------------------------------------------------------------------
struct PackPlan {
  eogs_report_item item[EOGS_REPORT_MAX_ITEMS];
  uint32_t first[EOGS_REPORT_MAX_ITEMS + 1];  // the first workgroup of every item; first[n] = the grid
  int n;
};
constexpr uint32_t PACK_WG_PIXELS = RT * PACK_PER_WG;

__device__ __forceinline__ uint8_t to_u8(float x, int mode) {
  float t;
  if (mode == EOGS_REPORT_U8_ROUND) {
    t = x * 255.f + 0.5f;
    t = t > 0.f ? (t < 255.f ? t : 255.f) : 0.f;  // a NaN fails the first comparison: 0
  } else {
    const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;
    t = c * 255.f;
  }
  return (uint8_t)(int)t;  // 0 <= t <= 255: the cast truncates
}

__global__ __launch_bounds__(RT) void report_pack_kernel(PackPlan plan, char* __restrict__ dst) {
  int s = 0;
  for (int i = 1; i < plan.n; i++) s = (blockIdx.x >= plan.first[i]) ? i : s;  // (wave-uniform; empty items share a start)
  const eogs_report_item& it = plan.item[s];
  const int C = it.C, W = it.W;
  const int64_t n = (int64_t)it.H * W;
  const bool replicate = (it.flags & EOGS_REPORT_REPLICATE) != 0u, reverse = (it.flags & EOGS_REPORT_REVERSE) != 0u,
             premap = (it.flags & EOGS_REPORT_PREMAP) != 0u;
  const int Co = replicate ? 3 : C;
  const int64_t p0 = (int64_t)(blockIdx.x - plan.first[s]) * PACK_WG_PIXELS + threadIdx.x;
#pragma unroll
  for (int j = 0; j < PACK_PER_WG; j++) {
    const int64_t p = p0 + (int64_t)j * RT;
    if (p >= n) break;
    const int64_t r = p / W, c = p - r * W;
    float v[EOGS_REPORT_PACK_MAX_CHANNELS];
#pragma unroll
    for (int k = 0; k < EOGS_REPORT_PACK_MAX_CHANNELS; k++) {
      if (k < Co) {
        const int sc = replicate ? 0 : (reverse ? C - 1 - k : k);
        float x = it.src[(int64_t)sc * n + p];
        if (premap) x = (x - it.lo) / it.d;
        v[k] = x;
      }
    }
    char* px = dst + it.dst_offset + (uint64_t)r * it.dst_pitch;
    if (it.mode == EOGS_REPORT_FLOAT_HWC) {
      float* o = reinterpret_cast<float*>(px) + c * Co;
#pragma unroll
      for (int k = 0; k < EOGS_REPORT_PACK_MAX_CHANNELS; k++)
        if (k < Co) o[k] = v[k];
    } else {
      uint8_t* o = reinterpret_cast<uint8_t*>(px) + c * Co;
#pragma unroll
      for (int k = 0; k < EOGS_REPORT_PACK_MAX_CHANNELS; k++)
        if (k < Co) o[k] = to_u8(v[k], it.mode);
    }
  }
}

// ---- host checks ---------------------------------------------------------------------------------------------------------
bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}
size_t metrics_ws_bytes() { return (size_t)RMAXBLK * RK * sizeof(double) + 256; }

int check_cameras(int n, const eogs_report_camera* cams, size_t wb, size_t bb, const char* who) {
  if (n < 0 || n > EOGS_REPORT_MAX_CAMERAS) return fail(EOGS_ERR_INVALID_ARG, "%s: at most 64 cameras in one call", who);
  if (n > 0 && !cams) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL camera table", who);
  for (int i = 0; i < n; i++) {
    if (!cams[i].weight || !cams[i].bias) return fail(EOGS_ERR_INVALID_ARG, "%s: a camera without its weight or bias", who);
    if (misaligned(cams[i].weight, 4) || misaligned(cams[i].bias, 4)) return fail(EOGS_ERR_INVALID_ARG, "%s: a pointer is not 4-byte aligned", who);
    if (overlaps(cams[i].weight, wb, cams[i].bias, bb)) return fail(EOGS_ERR_INVALID_ARG, "%s: a camera's weight overlaps its bias", who);
    for (int j = 0; j < i; j++)
      if (overlaps(cams[i].weight, wb, cams[j].weight, wb) || overlaps(cams[i].weight, wb, cams[j].bias, bb) ||
          overlaps(cams[i].bias, bb, cams[j].weight, wb) || overlaps(cams[i].bias, bb, cams[j].bias, bb))
        return fail(EOGS_ERR_INVALID_ARG, "%s: two cameras written by one call overlap", who);
  }
  return EOGS_OK;
}

}  // namespace

extern "C" {

int eogs_report_normalize_rows(int64_t P, float* f_dc, const float* A1, const float* b1, void* stream) {
  clear_error();
  if (P < 0) return fail(EOGS_ERR_INVALID_ARG, "report_normalize_rows: negative row count");
  if (P > ((int64_t)1 << 40)) return fail(EOGS_ERR_OVERFLOW, "report_normalize_rows: too many rows for one launch");
  if (!A1 || !b1) return fail(EOGS_ERR_INVALID_ARG, "report_normalize_rows: NULL A1 or b1");
  if (misaligned(A1, 4) || misaligned(b1, 4) || misaligned(f_dc, 4)) return fail(EOGS_ERR_INVALID_ARG, "report_normalize_rows: a pointer is not 4-byte aligned");
  if (P == 0) return EOGS_OK;
  if (!f_dc) return fail(EOGS_ERR_INVALID_ARG, "report_normalize_rows: NULL f_dc");
  const size_t fb = (size_t)P * 3 * sizeof(float);
  if (overlaps(f_dc, fb, A1, 36) || overlaps(f_dc, fb, b1, 12)) return fail(EOGS_ERR_INVALID_ARG, "report_normalize_rows: f_dc overlaps A1 or b1");
  const int64_t lanes = (P + 3) / 4, blocks = (lanes + RT - 1) / RT;
  if (blocks > 0x7fffffffLL) return fail(EOGS_ERR_OVERFLOW, "report_normalize_rows: too many rows for one launch");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(report_rows_kernel, dim3((unsigned)blocks), dim3(RT), 0, s, P, f_dc, A1, b1, misaligned(f_dc, 16) ? 0 : 1);
  LAUNCH_TRY(s, false, "report_normalize_rows");
  return EOGS_OK;
}

int eogs_report_recompose(int n, const eogs_report_camera* cameras, const float* ref_weight, const float* ref_bias, void* stream) {
  clear_error();
  int rc = check_cameras(n, cameras, 36, 12, "report_recompose");
  if (rc) return rc;
  if (!ref_weight || !ref_bias) return fail(EOGS_ERR_INVALID_ARG, "report_recompose: NULL reference weight or bias");
  if (misaligned(ref_weight, 4) || misaligned(ref_bias, 4)) return fail(EOGS_ERR_INVALID_ARG, "report_recompose: a pointer is not 4-byte aligned");
  // the reference tensors may BE a camera's own; any other overlap with one is refused
  for (int i = 0; i < n; i++) {
    const bool w_same = cameras[i].weight == ref_weight, b_same = cameras[i].bias == ref_bias;
    if ((!w_same && overlaps(cameras[i].weight, 36, ref_weight, 36)) || overlaps(cameras[i].weight, 36, ref_bias, 12) ||
        overlaps(cameras[i].bias, 12, ref_weight, 36) || (!b_same && overlaps(cameras[i].bias, 12, ref_bias, 12)))
      return fail(EOGS_ERR_INVALID_ARG, "report_recompose: the reference correction partly overlaps a camera's");
  }
  if (n == 0) return EOGS_OK;
  CameraTable T;
  for (int i = 0; i < EOGS_REPORT_MAX_CAMERAS; i++) T.cam[i] = i < n ? cameras[i] : eogs_report_camera{nullptr, nullptr};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(report_recompose_kernel, dim3(1), dim3(64), 0, s, n, T, ref_weight, ref_bias);
  LAUNCH_TRY(s, false, "report_recompose");
  return EOGS_OK;
}

int eogs_report_cc_to_test(int mode, int n_train, const eogs_report_camera* train, int n_test, const eogs_report_camera* test,
                           int w_elems, int b_elems, void* stream) {
  clear_error();
  if (mode != EOGS_REPORT_CC_REF && mode != EOGS_REPORT_CC_AVERAGE) return fail(EOGS_ERR_INVALID_ARG, "report_cc_to_test: unknown mode");
  if (w_elems < 1 || b_elems < 1 || w_elems + b_elems > EOGS_REPORT_MAX_CC_ELEMS) return fail(EOGS_ERR_INVALID_ARG, "report_cc_to_test: bad element counts");
  if (n_train < 1) return fail(EOGS_ERR_INVALID_ARG, "report_cc_to_test: no train camera");
  const size_t wb = (size_t)w_elems * 4, bb = (size_t)b_elems * 4;
  // (train cameras are only read: they may repeat)
  if (n_train > EOGS_REPORT_MAX_CAMERAS) return fail(EOGS_ERR_INVALID_ARG, "report_cc_to_test: at most 64 cameras in one call");
  if (!train) return fail(EOGS_ERR_INVALID_ARG, "report_cc_to_test: NULL camera table");
  for (int i = 0; i < n_train; i++) {
    if (!train[i].weight || !train[i].bias) return fail(EOGS_ERR_INVALID_ARG, "report_cc_to_test: a camera without its weight or bias");
    if (misaligned(train[i].weight, 4) || misaligned(train[i].bias, 4)) return fail(EOGS_ERR_INVALID_ARG, "report_cc_to_test: a pointer is not 4-byte aligned");
  }
  int rc = check_cameras(n_test, test, wb, bb, "report_cc_to_test");
  if (rc) return rc;
  for (int i = 0; i < n_test; i++)
    for (int j = 0; j < n_train; j++)
      if (overlaps(test[i].weight, wb, train[j].weight, wb) || overlaps(test[i].weight, wb, train[j].bias, bb) ||
          overlaps(test[i].bias, bb, train[j].weight, wb) || overlaps(test[i].bias, bb, train[j].bias, bb))
        return fail(EOGS_ERR_INVALID_ARG, "report_cc_to_test: a test camera overlaps a train camera");
  if (n_test == 0) return EOGS_OK;
  CameraTable A, B;
  for (int i = 0; i < EOGS_REPORT_MAX_CAMERAS; i++) {
    A.cam[i] = i < n_train ? train[i] : eogs_report_camera{nullptr, nullptr};
    B.cam[i] = i < n_test ? test[i] : eogs_report_camera{nullptr, nullptr};
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(report_cc_to_test_kernel, dim3(1), dim3(64), 0, s, mode, n_train, A, n_test, B, w_elems, b_elems);
  LAUNCH_TRY(s, false, "report_cc_to_test");
  return EOGS_OK;
}

int eogs_report_metrics_bytes(size_t* bytes) {
  clear_error();
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "report_metrics_bytes: NULL argument");
  *bytes = metrics_ws_bytes();
  return EOGS_OK;
}

int eogs_report_metrics_reset(eogs_report_table* table, void* stream) {
  clear_error();
  if (!table || misaligned(table, 8)) return fail(EOGS_ERR_INVALID_ARG, "report_metrics_reset: table NULL or not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(report_metrics_reset_kernel, dim3(1), dim3(64), 0, s, table);
  LAUNCH_TRY(s, false, "report_metrics_reset");
  return EOGS_OK;
}

int eogs_report_metrics_accumulate(int C, int H, int W, const float* image, const float* gt, int kind, eogs_report_table* table,
                                   const uint32_t* gate, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "report_metrics_accumulate: bad sizes");
  if (C < 1 || C > EOGS_REPORT_MAX_CHANNELS) return fail(EOGS_ERR_INVALID_ARG, "report_metrics_accumulate: 1 to 4 channels");
  if (kind != EOGS_REPORT_KIND_PAN && kind != EOGS_REPORT_KIND_MSI) return fail(EOGS_ERR_INVALID_ARG, "report_metrics_accumulate: unknown kind");
  if (!image || !gt || !table || !ws) return fail(EOGS_ERR_INVALID_ARG, "report_metrics_accumulate: NULL argument");
  if (misaligned(image, 4) || misaligned(gt, 4) || misaligned(gate, 4) || misaligned(table, 8))
    return fail(EOGS_ERR_INVALID_ARG, "report_metrics_accumulate: a pointer is not aligned");
  if (ws_bytes < metrics_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "report_metrics_accumulate: workspace too small");
  const int64_t n = (int64_t)H * W;
  const size_t ib = (size_t)n * C * sizeof(float);
  if (overlaps(table, sizeof(eogs_report_table), image, ib) || overlaps(table, sizeof(eogs_report_table), gt, ib) ||
      overlaps(ws, ws_bytes, image, ib) || overlaps(ws, ws_bytes, gt, ib) || overlaps(ws, ws_bytes, table, sizeof(eogs_report_table)))
    return fail(EOGS_ERR_INVALID_ARG, "report_metrics_accumulate: the table or the workspace overlaps an input");
  hipStream_t s = (hipStream_t)stream;
  const int nb = capped_blocks(n, RT, RMAXBLK);
  double* partial = reinterpret_cast<double*>(ws_base(ws));
  switch (C) {
    case 1: hipLaunchKernelGGL(report_metrics_partial_kernel<1>, dim3(nb), dim3(RT), 0, s, n, image, gt, partial); break;
    case 2: hipLaunchKernelGGL(report_metrics_partial_kernel<2>, dim3(nb), dim3(RT), 0, s, n, image, gt, partial); break;
    case 3: hipLaunchKernelGGL(report_metrics_partial_kernel<3>, dim3(nb), dim3(RT), 0, s, n, image, gt, partial); break;
    default: hipLaunchKernelGGL(report_metrics_partial_kernel<4>, dim3(nb), dim3(RT), 0, s, n, image, gt, partial); break;
  }
  hipLaunchKernelGGL(report_metrics_final_kernel, dim3(1), dim3(RT), 0, s, C, n, partial, nb, kind, table, gate);
  LAUNCH_TRY(s, false, "report_metrics_accumulate");
  return EOGS_OK;
}

int eogs_report_pack(int n, const eogs_report_item* items, void* dst, size_t dst_bytes, void* stream) {
  clear_error();
  if (n < 0 || n > EOGS_REPORT_MAX_ITEMS) return fail(EOGS_ERR_INVALID_ARG, "report_pack: bad item count (at most 16 items in one call)");
  if (n == 0) return EOGS_OK;
  if (!items || !dst) return fail(EOGS_ERR_INVALID_ARG, "report_pack: NULL items or dst");
  PackPlan plan;
  plan.n = n;
  uint64_t wg = 0;
  for (int i = 0; i < EOGS_REPORT_MAX_ITEMS; i++) {
    plan.first[i] = (uint32_t)wg;
    if (i >= n) {
      plan.item[i] = eogs_report_item{nullptr, 1, 0, 0, 0, 0, 0, 0u, 0.f, 1.f};
      continue;
    }
    const eogs_report_item& t = items[i];
    if (!t.src || misaligned(t.src, 4)) return fail(EOGS_ERR_INVALID_ARG, "report_pack: an item's source is NULL or not 4-byte aligned");
    if (t.C < 1 || t.C > EOGS_REPORT_PACK_MAX_CHANNELS || t.H < 1 || t.W < 1) return fail(EOGS_ERR_INVALID_ARG, "report_pack: an item needs 1 to 5 channels and positive sizes");
    if (t.mode != EOGS_REPORT_FLOAT_HWC && t.mode != EOGS_REPORT_U8_ROUND && t.mode != EOGS_REPORT_U8_TRUNC) return fail(EOGS_ERR_INVALID_ARG, "report_pack: unknown mode");
    if (t.flags & ~(EOGS_REPORT_REVERSE | EOGS_REPORT_REPLICATE | EOGS_REPORT_PREMAP)) return fail(EOGS_ERR_INVALID_ARG, "report_pack: unknown flag");
    if ((t.flags & EOGS_REPORT_REPLICATE) && t.C != 1) return fail(EOGS_ERR_INVALID_ARG, "report_pack: REPLICATE takes a one-channel source");
    const uint64_t eb = t.mode == EOGS_REPORT_FLOAT_HWC ? 4 : 1, Co = (t.flags & EOGS_REPORT_REPLICATE) ? 3 : (uint64_t)t.C;
    const uint64_t row = (uint64_t)t.W * Co * eb;
    if (t.dst_pitch < row) return fail(EOGS_ERR_INVALID_ARG, "report_pack: an item's pitch is shorter than its row");
    if (t.dst_pitch > ((uint64_t)1 << 40) || t.dst_offset > ((uint64_t)1 << 48)) return fail(EOGS_ERR_OVERFLOW, "report_pack: offset or pitch out of range");
    if (eb == 4 && ((t.dst_offset | t.dst_pitch) & 3u || misaligned(dst, 4))) return fail(EOGS_ERR_INVALID_ARG, "report_pack: a FLOAT_HWC item's offset and pitch must be multiples of 4");
    const uint64_t extent = (uint64_t)(t.H - 1) * t.dst_pitch + row;
    if (t.dst_offset + extent > (uint64_t)dst_bytes) return fail(EOGS_ERR_INVALID_ARG, "report_pack: an item's rectangle leaves dst");
    if (overlaps(t.src, (size_t)t.C * t.H * t.W * 4, dst, dst_bytes)) return fail(EOGS_ERR_INVALID_ARG, "report_pack: a source overlaps dst");
    plan.item[i] = t;
    wg += ((uint64_t)t.H * t.W + PACK_WG_PIXELS - 1) / PACK_WG_PIXELS;
    if (wg > 0x7fffffffULL) return fail(EOGS_ERR_OVERFLOW, "report_pack: too many pixels for one launch");
  }
  plan.first[EOGS_REPORT_MAX_ITEMS] = (uint32_t)wg;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(report_pack_kernel, dim3((unsigned)wg), dim3(RT), 0, s, plan, reinterpret_cast<char*>(dst));
  LAUNCH_TRY(s, false, "report_pack");
  return EOGS_OK;
}

}  // extern "C"
