// flow.hip — the flow-matching warp (include/eogs_resample.h, eogs_resample_flow_*): out[c][y][x] = bilinear sample of
// img[c] at (x + flow_x, y + flow_y), border padding; its adjoint with respect to img; one-pass statistics of a flow.
// Reference: flowmatching/flow_matching.py:225-253 (grid + flow, two normalisations, permute, grid_sample(border,
// align_corners=True)) and autograd's atomic scatter backward. Here the position stays in pixels (flow_taps.h), the
// forward is one kernel, and the backward writes every dL/dimg element exactly once with sums in a fixed order:
//   field flow        the four-tap scatter as the bucketed gather of bucket_gather.h (shared with the resample backward);
//   constant flow     the warp is separable, so input pixel (j, i) gathers the product of two short runs of outputs
//                     (flow_axis_run): at most a few, except on the border rows / columns that collect every output clamped
//                     onto them; runs longer than CST_LONG outputs are summed by the whole workgroup.
// A one-element `gate` on the device switches the warp off (forward and backward become copies) without a host read.
// All kernels are HBM-bound streams with neighbouring lanes on neighbouring addresses.
#include "bucket_gather.h"
#include "api_util.h"
#include "flow_taps.h"
#include "reduce.h"

namespace {

struct FlowField {  // a [2][H][W] flow with element strides; sy == sx == 0: one displacement for the whole image
  const float* __restrict__ f;
  int64_t sc, sy, sx;
  __device__ float2 at(int x, int y) const {
    const int64_t o = (int64_t)y * sy + (int64_t)x * sx;
    return make_float2(f[o], f[sc + o]);
  }
};

__device__ inline bool gate_open(const float* gate) { return !gate || gate[0] != 0.f; }

// ---- forward: one lane per pixel, the flow and the taps once for all planes, planar stores ----
__global__ __launch_bounds__(BLK) void flow_fwd_kernel(int C, int H, int W, const float* __restrict__ img, const FlowField fl,
                                                       const float* __restrict__ gate, float* __restrict__ out) {
  const int HW = H * W;
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= HW) return;
  if (!gate_open(gate)) {
    for (int c = 0; c < C; c++) out[(size_t)c * HW + p] = img[(size_t)c * HW + p];
    return;
  }
  const int y = p / W, x = p - y * W;
  const float2 f = fl.at(x, y);
  const FlowAxisTap tx = flow_axis_tap(x, f.x, W), ty = flow_axis_tap(y, f.y, H);
  const float wx0 = 1.f - tx.w1, wy0 = 1.f - ty.w1;
  const float wnw = wx0 * wy0, wne = tx.w1 * wy0, wsw = wx0 * ty.w1, wse = tx.w1 * ty.w1;
  const int onw = ty.i0 * W + tx.i0, one = ty.i0 * W + tx.i1, osw = ty.i1 * W + tx.i0, ose = ty.i1 * W + tx.i1;
  // the taps of up to four planes are requested together (as resample_fwd_kernel does)
  for (int c0 = 0; c0 < C; c0 += 4) {
    float v[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float* src = img + (size_t)(c0 + k < C ? c0 + k : c0) * HW;
      v[k][0] = src[onw]; v[k][1] = src[one]; v[k][2] = src[osw]; v[k][3] = src[ose];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (c0 + k >= C) break;
      out[(size_t)(c0 + k) * HW + p] = v[k][0] * wnw + v[k][1] * wne + v[k][2] * wsw + v[k][3] * wse;
    }
  }
}

// ---- backward, field flow: bounding boxes of the cells each 16 x 16 output tile touches, then the bucketed gather ----
struct FlowSrc {
  FlowField fl;
  const float* __restrict__ gate;
  struct Raw { float fx, fy; int x, y; };
  __device__ Raw load(size_t, int x, int y) const {
    const float2 f = fl.at(x, y);
    return Raw{f.x, f.y, x, y};
  }
  __device__ void taps(const Raw& r, int Wv, int Hv, int& x0, int& y0, float& wx1, float& wy1, bool& outside) const {
    const FlowAxisTap tx = flow_axis_tap(r.x, r.fx, Wv), ty = flow_axis_tap(r.y, r.fy, Hv);
    x0 = tx.i0; y0 = ty.i0; wx1 = tx.w1; wy1 = ty.w1;  // (the tap east of column W - 1 has no cell and weighs 0)
    outside = false;
  }
  __device__ bool bypass() const { return !gate_open(gate); }
};

__global__ __launch_bounds__(BLK) void flow_bbox_kernel(int H, int W, const FlowField fl, int4* __restrict__ bbox) {
  __shared__ int s_box[4][BLK / 64];
  const int x = blockIdx.x * OT + (threadIdx.x & (OT - 1)), y = blockIdx.y * OT + (threadIdx.x >> 4);
  int bx0 = 0x7FFFFFFF, by0 = 0x7FFFFFFF, bx1 = -0x7FFFFFFF, by1 = -0x7FFFFFFF;
  if (x < W && y < H) {
    const float2 f = fl.at(x, y);
    bx0 = flow_axis_tap(x, f.x, W).i0; bx1 = bx0 + 1;
    by0 = flow_axis_tap(y, f.y, H).i0; by1 = by0 + 1;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    bx0 = min(bx0, __shfl_xor(bx0, o, 64)); by0 = min(by0, __shfl_xor(by0, o, 64));
    bx1 = max(bx1, __shfl_xor(bx1, o, 64)); by1 = max(by1, __shfl_xor(by1, o, 64));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_box[0][w] = bx0; s_box[1][w] = by0; s_box[2][w] = bx1; s_box[3][w] = by1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < BLK / 64; k++) {
      bx0 = min(bx0, s_box[0][k]); by0 = min(by0, s_box[1][k]); bx1 = max(bx1, s_box[2][k]); by1 = max(by1, s_box[3][k]);
    }
    bbox[blockIdx.y * gridDim.x + blockIdx.x] = make_int4(bx0, by0, bx1, by1);
  }
}

// ---- backward, constant displacement: a closed-form gather, no buckets, no workspace ----
constexpr int CTX = 64, CTY = BLK / CTX;  // input tile of a workgroup: one wave per row
constexpr int CST_LONG = 64;              // outputs one lane sums alone; longer runs (border rows / columns) go to the workgroup
constexpr int CCH = 4;                    // planes per pass

__global__ __launch_bounds__(BLK) void flow_bwd_cst_kernel(int C, int H, int W, const float* __restrict__ flow, int64_t sc,
                                                           const float* __restrict__ gate, const float* __restrict__ g,
                                                           float* __restrict__ gimg) {
  __shared__ int4 s_run[BLK];  // {xa, nx, ya, ny} of the lanes whose run is long, nx = 0 otherwise
  __shared__ float s_red[BLK / 64][CCH];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int i = blockIdx.x * CTX + lane, j = blockIdx.y * CTY + wv;
  const bool live = i < W && j < H;
  const size_t HW = (size_t)H * W;
  if (!gate_open(gate)) {
    if (live)
      for (int c = 0; c < C; c++) gimg[c * HW + (size_t)j * W + i] = g[c * HW + (size_t)j * W + i];
    return;
  }
  const float dx = flow[0], dy = flow[sc];
  int xa = 0, xb = -1, ya = 0, yb = -1;
  if (live) {
    flow_axis_run(i, dx, W, &xa, &xb);
    flow_axis_run(j, dy, H, &ya, &yb);
  }
  const int nx = max(xb - xa + 1, 0), ny = max(yb - ya + 1, 0);
  const bool is_long = (int64_t)nx * ny > CST_LONG;
  if (live && !is_long) {  // rows outside, columns inside; the products in that fixed order
    float wxs[5];  // the column weights of the window inside the image, once for all rows (a border column's run may be longer)
#pragma unroll
    for (int k = 0; k < 5; k++) wxs[k] = xa + k <= xb ? flow_axis_weight(xa + k, dx, W, i) : 0.f;
    for (int c0 = 0; c0 < C; c0 += CCH) {
      float acc[CCH] = {0.f, 0.f, 0.f, 0.f};
      for (int y = ya; y <= yb; y++) {
        const float wy = flow_axis_weight(y, dy, H, j);
        if (wy == 0.f) continue;
        for (int x = xa; x <= xb; x++) {
          const int kx = x - xa;
          const float wx = kx < 5 ? (kx == 0 ? wxs[0] : kx == 1 ? wxs[1] : kx == 2 ? wxs[2] : kx == 3 ? wxs[3] : wxs[4])
                                  : flow_axis_weight(x, dx, W, i);
          if (wx == 0.f) continue;
          const float w = wx * wy;
          const size_t o = (size_t)y * W + x;
#pragma unroll
          for (int k = 0; k < CCH; k++)
            if (c0 + k < C) acc[k] += g[(c0 + k) * HW + o] * w;
        }
      }
#pragma unroll
      for (int k = 0; k < CCH; k++)
        if (c0 + k < C) gimg[(c0 + k) * HW + (size_t)j * W + i] = acc[k];
    }
  }
  if (!__syncthreads_or(is_long ? 1 : 0)) return;
  // long runs, one pixel after the other in lane order: element e of the run belongs to thread e mod BLK, the partial sums
  // meet in a butterfly and then wave by wave: the order depends on the shape and the displacement alone
  s_run[t] = is_long ? make_int4(xa, nx, ya, ny) : make_int4(0, 0, 0, 0);
  __syncthreads();
  for (int q = 0; q < BLK; q++) {
    const int4 r = s_run[q];
    if (r.y == 0) continue;  // (uniform: every thread reads the same entry)
    const int qi = blockIdx.x * CTX + (q & 63), qj = blockIdx.y * CTY + (q >> 6);
    const int n = r.y * r.w;
    for (int c0 = 0; c0 < C; c0 += CCH) {
      float acc[CCH] = {0.f, 0.f, 0.f, 0.f};
      for (int e = t; e < n; e += BLK) {
        const int ey = e / r.y, y = r.z + ey, x = r.x + (e - ey * r.y);
        const float w = flow_axis_weight(x, dx, W, qi) * flow_axis_weight(y, dy, H, qj);
        if (w == 0.f) continue;
        const size_t o = (size_t)y * W + x;
#pragma unroll
        for (int k = 0; k < CCH; k++)
          if (c0 + k < C) acc[k] += g[(c0 + k) * HW + o] * w;
      }
#pragma unroll
      for (int k = 0; k < CCH; k++) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
        if (lane == 0) s_red[wv][k] = acc[k];
      }
      __syncthreads();
      if (t == q) {
#pragma unroll
        for (int k = 0; k < CCH; k++) {
          float v = s_red[0][k];
          for (int w2 = 1; w2 < BLK / 64; w2++) v += s_red[w2][k];
          if (c0 + k < C) gimg[(c0 + k) * HW + (size_t)qj * W + qi] = v;
        }
      }
      __syncthreads();
    }
  }
}

// ---- statistics: sums in double around a pivot (the flow's first element of each plane), a grid that depends on the
// shape alone, partials combined in index order by one workgroup ----
constexpr int ST_MAX_GRID = 256;
constexpr int ST_N = 5;  // sum x', sum y', sum |x| + |y|, sum x'^2, sum y'^2

__global__ __launch_bounds__(BLK) void flow_stats_partial_kernel(int H, int W, const FlowField fl, double* __restrict__ part) {
  const float2 piv = fl.at(0, 0);
  const int HW = H * W;
  double a[ST_N] = {0., 0., 0., 0., 0.};
  for (int p = blockIdx.x * BLK + threadIdx.x; p < HW; p += gridDim.x * BLK) {
    const int y = p / W, x = p - y * W;
    const float2 f = fl.at(x, y);
    const double ux = (double)f.x - (double)piv.x, uy = (double)f.y - (double)piv.y;
    a[0] += ux; a[1] += uy; a[2] += (double)fabsf(f.x) + (double)fabsf(f.y); a[3] += ux * ux; a[4] += uy * uy;
  }
  wg_partials<BLK>(a, part + (size_t)blockIdx.x * ST_N);
}

__global__ __launch_bounds__(64) void flow_stats_final_kernel(int H, int W, const FlowField fl, const double* __restrict__ part,
                                                              int nblk, float* __restrict__ stats) {
  if (threadIdx.x != 0) return;
  double a[ST_N] = {0., 0., 0., 0., 0.};
  for (int b = 0; b < nblk; b++)
    for (int k = 0; k < ST_N; k++) a[k] += part[(size_t)b * ST_N + k];
  const float2 piv = fl.at(0, 0);
  const double n = (double)H * (double)W;
  const double mx = a[0] / n, my = a[1] / n;  // means of the shifted values
  const double vx = fmax(a[3] - n * mx * mx, 0.) / (n - 1.), vy = fmax(a[4] - n * my * my, 0.) / (n - 1.);  // unbiased, as torch.std
  stats[0] = (float)((double)piv.x + mx);
  stats[1] = (float)((double)piv.y + my);
  stats[2] = (float)(a[2] / (2. * n));
  stats[3] = (float)sqrt(vx);
  stats[4] = (float)sqrt(vy);
}

}  // namespace

static size_t flow_stats_ws_bytes(int H, int W) { return (size_t)capped_blocks((int64_t)H * W, BLK, ST_MAX_GRID) * ST_N * sizeof(double) + 256; }

// the field backward's workspace: one box per 16 x 16 output tile (a constant displacement needs none)
static size_t flow_bwd_ws_bytes(int H, int W) {
  const size_t nt = (size_t)((W + OT - 1) / OT) * ((H + OT - 1) / OT);
  return (nt * sizeof(int4) + 255) / 256 * 256 + 256;
}

static void launch_flow_bwd(int C, int H, int W, const float* flow, int64_t sc, int64_t sy, int64_t sx, const float* gate,
                     const float* g, float* gimg, void* ws, hipStream_t s) {
  if (sy == 0 && sx == 0) {
    hipLaunchKernelGGL(flow_bwd_cst_kernel, dim3((W + CTX - 1) / CTX, (H + CTY - 1) / CTY), dim3(BLK), 0, s, C, H, W, flow, sc,
                       gate, g, gimg);
    return;
  }
  const FlowSrc src{FlowField{flow, sc, sy, sx}, gate};
  const int ntx = (W + OT - 1) / OT, nty = (H + OT - 1) / OT;
  int4* bbox = reinterpret_cast<int4*>(ws_base(ws));
  hipLaunchKernelGGL(flow_bbox_kernel, dim3(ntx, nty), dim3(BLK), 0, s, H, W, src.fl, bbox);
  const bool big = (size_t)H * W > 1500000;  // the tile choice of the resample backward
  const int vx = big ? 64 : 32, vy = 32;
  const size_t HW = (size_t)H * W;
  for (int c0 = 0; c0 < C; c0 += 4) {  // the gather holds up to four planes in registers
    const int n = C - c0 < 4 ? C - c0 : 4;
    auto* kern = n == 1 ? (big ? resample_bwd_gather_kernel<1, 64, 32, FlowSrc> : resample_bwd_gather_kernel<1, 32, 32, FlowSrc>)
                        : (big ? resample_bwd_gather_kernel<4, 64, 32, FlowSrc> : resample_bwd_gather_kernel<4, 32, 32, FlowSrc>);
    hipLaunchKernelGGL(kern, dim3((W + vx - 1) / vx, (H + vy - 1) / vy), dim3(BLK), 0, s, n, H, W, H, W, n, src, -1,
                       g + c0 * HW, (const int4*)bbox, ntx, nty, gimg + c0 * HW);
  }
}

static int flow_check(const char* who, int C, int H, int W) {
  if (C < 1 || H < 2 || W < 2 || (int64_t)H * W > 0x7FFFFFFF) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (C >= 1, H >= 2, W >= 2)", who);
  return EOGS_OK;
}

extern "C" {

int eogs_resample_flow_forward(int C, int H, int W, const float* img, const float* flow, int64_t plane_stride,
                               int64_t row_stride, int64_t col_stride, const float* gate, float* out, void* stream) {
  clear_error();
  const int rc = flow_check("resample_flow_forward", C, H, W);
  if (rc != EOGS_OK) return rc;
  if (!img || !flow || !out) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_forward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  {
    ProfScope ps(PS_FLOW_FWD, s);
    hipLaunchKernelGGL(flow_fwd_kernel, dim3((HW + BLK - 1) / BLK), dim3(BLK), 0, s, C, H, W, img,
                       FlowField{flow, plane_stride, row_stride, col_stride}, gate, out);
  }
  LAUNCH_TRY(s, false, "flow_fwd");
  return EOGS_OK;
}

int eogs_resample_flow_bytes(int H, int W, size_t* bytes) {
  clear_error();
  if (H < 2 || W < 2 || (int64_t)H * W > 0x7FFFFFFF || !bytes) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_bytes: bad argument");
  *bytes = flow_bwd_ws_bytes(H, W);
  return EOGS_OK;
}

int eogs_resample_flow_backward(int C, int H, int W, const float* flow, int64_t plane_stride, int64_t row_stride,
                                int64_t col_stride, const float* gate, const float* dL_dout, float* dL_dimg, void* ws,
                                size_t ws_bytes, void* stream) {
  clear_error();
  const int rc = flow_check("resample_flow_backward", C, H, W);
  if (rc != EOGS_OK) return rc;
  if (!flow || !dL_dout || !dL_dimg) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_backward: NULL argument");
  const bool field = row_stride != 0 || col_stride != 0;
  if (field && (!ws || ws_bytes < flow_bwd_ws_bytes(H, W)))
    return fail(EOGS_ERR_WORKSPACE, "resample_flow_backward: workspace too small (a flow field needs eogs_resample_flow_bytes)");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_FLOW_BWD, s); launch_flow_bwd(C, H, W, flow, plane_stride, row_stride, col_stride, gate, dL_dout, dL_dimg, ws, s); }
  LAUNCH_TRY(s, false, "flow_bwd");
  return EOGS_OK;
}

int eogs_resample_flow_stats_bytes(int H, int W, size_t* bytes) {
  clear_error();
  if (H < 2 || W < 2 || (int64_t)H * W > 0x7FFFFFFF || !bytes) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_stats_bytes: bad argument");
  *bytes = flow_stats_ws_bytes(H, W);
  return EOGS_OK;
}

int eogs_resample_flow_stats(int H, int W, const float* flow, int64_t plane_stride, int64_t row_stride, int64_t col_stride,
                             float* stats, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const int rc = flow_check("resample_flow_stats", 1, H, W);
  if (rc != EOGS_OK) return rc;
  if (!flow || !stats || !ws) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_stats: NULL argument");
  if (ws_bytes < flow_stats_ws_bytes(H, W)) return fail(EOGS_ERR_WORKSPACE, "resample_flow_stats: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const FlowField fl{flow, plane_stride, row_stride, col_stride};
  double* part = reinterpret_cast<double*>(ws_base(ws));
  const int nb = capped_blocks((int64_t)H * W, BLK, ST_MAX_GRID);
  {
    ProfScope ps(PS_FLOW_STATS, s);
    hipLaunchKernelGGL(flow_stats_partial_kernel, dim3(nb), dim3(BLK), 0, s, H, W, fl, part);
    hipLaunchKernelGGL(flow_stats_final_kernel, dim3(1), dim3(64), 0, s, H, W, fl, (const double*)part, nb, stats);
  }
  LAUNCH_TRY(s, false, "flow_stats");
  return EOGS_OK;
}

}  // extern "C"
