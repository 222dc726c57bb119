// model.hip — the per-row passes of scene/gaussian_model.py::GaussianModel (include/eogs_model.h):
//   create_from_pcd   :159-215: seven tensors from points, colours and the 3-NN statistic, one launch
//   save_ply/load_ply :310-346, :354-449: six parameter tensors <-> the row-major block a PLY file's vertex payload is
// All three are streams: nothing is reused, nothing is arithmetic-bound. What matters is that a wave's loads and stores are
// runs of consecutive dwords on both sides, although one side is six arrays of 4- to 180-byte rows and the other one array
// of 68- to 248-byte rows. A workgroup therefore owns a tile of rows, whose slice of every array is one contiguous range,
// and turns the layout round in LDS: the tile is staged in the block's own layout, so the block side moves it as one
// range in 16-byte pieces and the tensor side walks each tensor's range dword by dword, lane after lane.
#include "api_util.h"
#include "eogs_model.h"

namespace {

constexpr int TR = EOGS_MODEL_TILE_ROWS;
constexpr float SH_C0 = 0.28209479177387814f;  // utils/sh_utils.py C0
constexpr float DIST2_MIN = 0.0000001f;        // gaussian_model.py:181

template <int NREST>
struct Cols {  // construct_list_of_attributes, gaussian_model.py:296-308
  static constexpr int XYZ = 0, NORMAL = 3, F_DC = 6, F_REST = 9, OPACITY = 9 + 3 * NREST, SCALE = OPACITY + 1, ROT = OPACITY + 4,
                       C = EOGS_MODEL_ROW_COLS(NREST);
  static_assert(ROT + 4 == C, "the columns fill the row");
  // where element j of a row of f_rest [NREST][3] goes: channel-major, transpose(1, 2).flatten(start_dim=1)
  static __device__ __forceinline__ int rest(int j) { const int k = j / 3, c = j - 3 * k; return F_REST + c * NREST + k; }
};

// one tensor's slice of the tile, W floats per row starting at column COL0 of the staged rows: global <-> LDS
template <int C, int W, int COL0, bool TO_LDS>
__device__ __forceinline__ void move_plain(float* __restrict__ g, float* __restrict__ t, int n) {
  for (int e = threadIdx.x; e < n * W; e += BLK) {
    const int r = e / W, j = e - r * W;
    if (TO_LDS) t[r * C + COL0 + j] = g[e]; else g[e] = t[r * C + COL0 + j];
  }
}

template <int NREST, bool TO_LDS>
__device__ __forceinline__ void move_rest(float* __restrict__ g, float* __restrict__ t, int n) {
  using L = Cols<NREST>;
  constexpr int W = 3 * NREST;
  if (W == 0) return;
  for (int e = threadIdx.x; e < n * W; e += BLK) {
    const int r = e / (W ? W : 1), j = e - r * W;
    if (TO_LDS) t[r * L::C + L::rest(j)] = g[e]; else g[e] = t[r * L::C + L::rest(j)];
  }
}

// the tile as one range of the block: LDS <-> global, 16 bytes per lane where the block's address allows it
template <bool TO_LDS>
__device__ __forceinline__ void move_tile(float* __restrict__ g, float* __restrict__ t, int total) {
  int done = 0;
  if (((uintptr_t)g & 15u) == 0) {
    const int n4 = total >> 2;
    float4* g4 = reinterpret_cast<float4*>(g);
    float4* t4 = reinterpret_cast<float4*>(t);
    for (int v = threadIdx.x; v < n4; v += BLK) {
      if (TO_LDS) t4[v] = g4[v]; else g4[v] = t4[v];
    }
    done = n4 << 2;
  }
  for (int e = done + threadIdx.x; e < total; e += BLK) {
    if (TO_LDS) t[e] = g[e]; else g[e] = t[e];
  }
}

template <int NREST, bool PACK>
__global__ __launch_bounds__(BLK) void rows_kernel(int64_t P, float* __restrict__ xyz, float* __restrict__ f_dc,
                                                   float* __restrict__ f_rest, float* __restrict__ opacity,
                                                   float* __restrict__ scaling, float* __restrict__ rotation,
                                                   float* __restrict__ rows) {
  using L = Cols<NREST>;
  constexpr int C = L::C;
  __shared__ __attribute__((aligned(16))) float t[TR * C];
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int n = (int)(P - row0 < (int64_t)TR ? P - row0 : (int64_t)TR);  // >= 1: the grid covers P rows
  float* block = rows + row0 * C;
  if (!PACK) {
    move_tile<true>(block, t, n * C);
    __syncthreads();
  }
  move_plain<C, 3, L::XYZ, PACK>(xyz + row0 * 3, t, n);
  move_plain<C, 3, L::F_DC, PACK>(f_dc + row0 * 3, t, n);
  move_rest<NREST, PACK>(f_rest + row0 * (3 * NREST), t, n);
  move_plain<C, 1, L::OPACITY, PACK>(opacity + row0, t, n);
  move_plain<C, 3, L::SCALE, PACK>(scaling + row0 * 3, t, n);
  move_plain<C, 4, L::ROT, PACK>(rotation + row0 * 4, t, n);
  if (PACK) {
    for (int e = threadIdx.x; e < n * 3; e += BLK) {
      const int r = e / 3, j = e - r * 3;
      t[r * C + L::NORMAL + j] = 0.0f;
    }
    __syncthreads();
    move_tile<false>(block, t, n * C);
  }
}

__global__ __launch_bounds__(BLK) void init_kernel(int64_t P, int n_rest, const float* __restrict__ points,
                                                   const float* __restrict__ colors, const float* __restrict__ dist2,
                                                   float opacity_logit, float* __restrict__ xyz, float* __restrict__ f_dc,
                                                   float* __restrict__ f_rest, float* __restrict__ scaling,
                                                   float* __restrict__ rotation, float* __restrict__ opacity,
                                                   float* __restrict__ max_radii2D) {
  __shared__ float log_scale[BLK];
  const int64_t row0 = (int64_t)blockIdx.x * BLK;
  const int n = (int)(P - row0 < (int64_t)BLK ? P - row0 : (int64_t)BLK);
  if ((int)threadIdx.x < n) {
    float d = dist2[row0 + threadIdx.x];
    d = d < DIST2_MIN ? DIST2_MIN : d;  // clamp_min: a NaN stays
    log_scale[threadIdx.x] = logf(sqrtf(d));
    opacity[row0 + threadIdx.x] = opacity_logit;
    max_radii2D[row0 + threadIdx.x] = 0.0f;
  }
  __syncthreads();
  const int64_t b3 = row0 * 3;
  for (int e = threadIdx.x; e < n * 3; e += BLK) {
    xyz[b3 + e] = points[b3 + e];
    f_dc[b3 + e] = (colors[b3 + e] - 0.5f) / SH_C0;
    scaling[b3 + e] = log_scale[e / 3];
  }
  for (int e = threadIdx.x; e < n * 4; e += BLK) rotation[row0 * 4 + e] = (e & 3) == 0 ? 1.0f : 0.0f;
  const int w = 3 * n_rest;
  for (int e = threadIdx.x; e < n * w; e += BLK) f_rest[row0 * w + e] = 0.0f;
}

constexpr int64_t MAX_ROWS = 0x7FFFFFFF;  // one workgroup per tile of rows, every in-tile index an int

// [a, a + na) and [b, b + nb) floats share an address (an empty or NULL range shares none)
bool overlap(const float* a, int64_t na, const float* b, int64_t nb) {
  if (!a || !b || na <= 0 || nb <= 0) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * 4u && b0 < a0 + (uintptr_t)na * 4u;
}

bool rest_ok(int n_rest) { return n_rest == 0 || n_rest == 3 || n_rest == 8 || n_rest == 15; }

template <bool PACK>
int launch_rows(const char* who, int64_t P, int n_rest, float* xyz, float* f_dc, float* f_rest, float* opacity, float* scaling,
                float* rotation, float* rows, void* stream) {
  clear_error();
  if (P < 0 || P > MAX_ROWS) return fail(EOGS_ERR_INVALID_ARG, "%s: bad row count", who);
  if (!rest_ok(n_rest)) return fail(EOGS_ERR_INVALID_ARG, "%s: n_rest is 0, 3, 8 or 15 (sh_degree 0 .. 3)", who);
  if (P == 0) return EOGS_OK;
  if (!xyz || !f_dc || !opacity || !scaling || !rotation || !rows || (n_rest > 0 && !f_rest))
    return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (((uintptr_t)xyz | (uintptr_t)f_dc | (uintptr_t)f_rest | (uintptr_t)opacity | (uintptr_t)scaling | (uintptr_t)rotation |
       (uintptr_t)rows) & 3u)
    return fail(EOGS_ERR_INVALID_ARG, "%s: arrays not 4-byte aligned", who);
  const float* tensors[6] = {xyz, f_dc, f_rest, opacity, scaling, rotation};
  const int64_t widths[6] = {3, 3, 3 * (int64_t)n_rest, 1, 3, 4};
  for (int i = 0; i < 6; i++) {
    if (overlap(tensors[i], widths[i] * P, rows, P * EOGS_MODEL_ROW_COLS(n_rest)))
      return fail(EOGS_ERR_INVALID_ARG, "%s: the block needs an array of its own", who);
    for (int j = i + 1; !PACK && j < 6; j++)  // what unpack writes: no two of them share an address
      if (overlap(tensors[i], widths[i] * P, tensors[j], widths[j] * P))
        return fail(EOGS_ERR_INVALID_ARG, "%s: two output tensors overlap", who);
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((uint32_t)((P + TR - 1) / TR)), block(BLK);
  switch (n_rest) {
    case 0: hipLaunchKernelGGL((rows_kernel<0, PACK>), grid, block, 0, s, P, xyz, f_dc, f_rest, opacity, scaling, rotation, rows); break;
    case 3: hipLaunchKernelGGL((rows_kernel<3, PACK>), grid, block, 0, s, P, xyz, f_dc, f_rest, opacity, scaling, rotation, rows); break;
    case 8: hipLaunchKernelGGL((rows_kernel<8, PACK>), grid, block, 0, s, P, xyz, f_dc, f_rest, opacity, scaling, rotation, rows); break;
    default: hipLaunchKernelGGL((rows_kernel<15, PACK>), grid, block, 0, s, P, xyz, f_dc, f_rest, opacity, scaling, rotation, rows); break;
  }
  LAUNCH_TRY(s, false, who);
  return EOGS_OK;
}

}  // namespace

extern "C" {

int eogs_model_init(int64_t P, int n_rest, const float* points, const float* colors, const float* dist2, float opacity_logit,
                    float* xyz, float* f_dc, float* f_rest, float* scaling, float* rotation, float* opacity, float* max_radii2D,
                    void* stream) {
  clear_error();
  if (P < 0 || P > MAX_ROWS) return fail(EOGS_ERR_INVALID_ARG, "model_init: bad row count");
  if (!rest_ok(n_rest)) return fail(EOGS_ERR_INVALID_ARG, "model_init: n_rest is 0, 3, 8 or 15 (sh_degree 0 .. 3)");
  if (P == 0) return EOGS_OK;
  if (!points || !colors || !dist2 || !xyz || !f_dc || !scaling || !rotation || !opacity || !max_radii2D || (n_rest > 0 && !f_rest))
    return fail(EOGS_ERR_INVALID_ARG, "model_init: NULL argument");
  if (((uintptr_t)points | (uintptr_t)colors | (uintptr_t)dist2 | (uintptr_t)xyz | (uintptr_t)f_dc | (uintptr_t)f_rest |
       (uintptr_t)scaling | (uintptr_t)rotation | (uintptr_t)opacity | (uintptr_t)max_radii2D) & 3u)
    return fail(EOGS_ERR_INVALID_ARG, "model_init: arrays not 4-byte aligned");
  const float* in[3] = {points, colors, dist2};
  const int64_t in_w[3] = {3, 3, 1};
  const float* out[7] = {xyz, f_dc, f_rest, scaling, rotation, opacity, max_radii2D};
  const int64_t out_w[7] = {3, 3, 3 * (int64_t)n_rest, 3, 4, 1, 1};
  for (int o = 0; o < 7; o++) {
    for (int i = 0; i < 3; i++)
      if (overlap(out[o], out_w[o] * P, in[i], in_w[i] * P))
        return fail(EOGS_ERR_INVALID_ARG, "model_init: an output needs an array of its own");
    for (int q = o + 1; q < 7; q++)
      if (overlap(out[o], out_w[o] * P, out[q], out_w[q] * P))
        return fail(EOGS_ERR_INVALID_ARG, "model_init: two outputs overlap");
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(init_kernel, dim3((uint32_t)((P + BLK - 1) / BLK)), dim3(BLK), 0, s, P, n_rest, points, colors, dist2,
                     opacity_logit, xyz, f_dc, f_rest, scaling, rotation, opacity, max_radii2D);
  LAUNCH_TRY(s, false, "model_init");
  return EOGS_OK;
}

int eogs_model_rows_pack(int64_t P, int n_rest, const float* xyz, const float* f_dc, const float* f_rest, const float* opacity,
                         const float* scaling, const float* rotation, float* rows, void* stream) {
  // (one kernel template serves both directions: the tensor pointers are only read when PACK)
  return launch_rows<true>("model_rows_pack", P, n_rest, const_cast<float*>(xyz), const_cast<float*>(f_dc), const_cast<float*>(f_rest),
                           const_cast<float*>(opacity), const_cast<float*>(scaling), const_cast<float*>(rotation), rows, stream);
}

int eogs_model_rows_unpack(int64_t P, int n_rest, const float* rows, float* xyz, float* f_dc, float* f_rest, float* opacity,
                           float* scaling, float* rotation, void* stream) {
  return launch_rows<false>("model_rows_unpack", P, n_rest, xyz, f_dc, f_rest, opacity, scaling, rotation, const_cast<float*>(rows),
                            stream);
}

}  // extern "C"
