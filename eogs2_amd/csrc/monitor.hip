// monitor.hip — the training monitor (include/eogs_monitor.h): what train_pan.py:423-429, 471-495, 512-597 and
// utils/callback_utils.py:15-44 keep on the host, kept in one device buffer. The only pass over images is the per-plane
// sum of squared differences of the PSNR (L1 and SSIM come from the loss the iteration has already run); everything else
// is a few scalars.
//
// Latency-bound work: what counts is the number of launches and the order of the sums. reduce.h's two-stage reductions:
// a grid that depends on the shape alone leaves float64 per-workgroup partials with plain stores, one workgroup adds them
// in a fixed order and updates the state in the same launch. No atomics: the same bits on every run and stream. An element
// is assigned to a lane by its INDEX in the plane (groups of four consecutive elements), so a base that is not 16-byte
// aligned changes the loads (four scalar ones instead of one 16-byte load), not the order of the sums.
//
// Every launch that writes the state starts with the gate: gate[0] == 0 leaves every byte of the state as it was.
#include <math.h>

#include "api_util.h"
#include "reduce.h"

namespace {

constexpr int MT = 256;        // threads per workgroup
constexpr int MSQ_MAXBLK = 256;   // workgroups per plane of the squared-difference pass
constexpr int MMODEL_MAXBLK = 1024;  // workgroups of the model pass

__device__ inline bool gate_closed(const uint32_t* gate) { return gate != nullptr && gate[0] == 0u; }

// ---- per-plane sum of (x - y)^2 ------------------------------------------------------------------------------------
// grid (blocks per plane, planes). A lane walks groups of four consecutive elements, d and d*d in fp32 as the reference
// forms them (image_utils.py:20), added into one fp32 accumulator in element order; wave and workgroup sums in double.
__global__ __launch_bounds__(MT) void monitor_sq_kernel(int64_t n, const float* __restrict__ img, const float* __restrict__ gt,
                                                        double* __restrict__ partial) {
  const float* __restrict__ x = img + (size_t)blockIdx.y * n;
  const float* __restrict__ y = gt + (size_t)blockIdx.y * n;
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;  // uniform over the workgroup
  const int64_t full = n >> 2, groups = (n + 3) >> 2;
  float acc = 0.f;
  for (int64_t g = (int64_t)blockIdx.x * MT + threadIdx.x; g < groups; g += (int64_t)gridDim.x * MT) {
    if (g < full) {
      float4 a, b;
      if (vec) {
        a = *reinterpret_cast<const float4*>(x + 4 * g);
        b = *reinterpret_cast<const float4*>(y + 4 * g);
      } else {
        a = make_float4(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]);
        b = make_float4(y[4 * g], y[4 * g + 1], y[4 * g + 2], y[4 * g + 3]);
      }
      const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
      acc += d0 * d0;
      acc += d1 * d1;
      acc += d2 * d2;
      acc += d3 * d3;
    } else {  // the plane's last one to three elements
      for (int64_t i = 4 * g; i < n; i++) {
        const float d = x[i] - y[i];
        acc += d * d;
      }
    }
  }
  double s[1] = {(double)acc};
  wg_partials<MT>(s, partial + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// One workgroup: per plane the partials in a fixed order, the plane's PSNR in fp32 (image_utils.py:20-21), their mean;
// then thread 0 performs the accumulation of observe (train_pan.py:423-429, 471-485).
__global__ __launch_bounds__(MT) void monitor_observe_kernel(int planes, int nblk, int64_t n, const double* __restrict__ partial,
                                                             const float* __restrict__ loss_out, float one_minus_lambda,
                                                             float lambda, int kind, int photometric_on,
                                                             const uint32_t* __restrict__ gate,
                                                             eogs_monitor_state* __restrict__ st) {
  __shared__ double s_red[MT / 64];
  if (gate_closed(gate)) return;  // uniform: before any barrier
  double psnr_sum = 0.;  // thread 0's
  for (int p = 0; p < planes; p++) {
    const double tot = column_sum<MT>(partial + (size_t)p * nblk, nblk, 1, s_red);
    if (threadIdx.x == 0) {
      const float mse = (float)(tot / (double)n);
      psnr_sum += (double)(20.f * log10f(1.f / sqrtf(mse)));  // mse 0: +inf, as the reference's
    }
  }
  if (threadIdx.x != 0) return;
  const float psnr = (float)(psnr_sum / (double)planes);
  const float l1 = loss_out[1], ssim = loss_out[2];
  const float photometric = one_minus_lambda * l1 + lambda * (1.f - ssim);  // image_utils.py:28
  st->sums[EOGS_MONITOR_L1] += (double)l1;
  if (photometric_on) {
    st->sums[EOGS_MONITOR_PHOTOMETRIC] += (double)photometric;
    st->n_photo += 1;
  }
  if (kind == EOGS_MONITOR_KIND_PAN) {
    st->sums[EOGS_MONITOR_PAN_PSNR] += (double)psnr;
    st->sums[EOGS_MONITOR_PAN_SSIM] += (double)ssim;
    st->n_pan += 1;
  } else {
    st->sums[EOGS_MONITOR_MSI_PSNR] += (double)psnr;
    st->sums[EOGS_MONITOR_MSI_SSIM] += (double)ssim;
    st->n_msi += 1;
  }
  st->last[0] = l1;
  st->last[1] = ssim;
  st->last[2] = photometric_on ? photometric : 0.f;  // (train_pan.py:301: Lphotometric = 0 without the term)
  st->last[3] = psnr;
}

// ---- the model: mean opacity over the rows that are not retired, and their number ----------------------------------
__global__ __launch_bounds__(MT) void monitor_model_kernel(int64_t P, const float* __restrict__ opacity,
                                                           double* __restrict__ partial) {
  const bool vec = (reinterpret_cast<uintptr_t>(opacity) & 15u) == 0;
  const int64_t full = P >> 2, groups = (P + 3) >> 2;
  double a[2] = {0., 0.};  // sum of sigmoid(opacity), rows
  for (int64_t g = (int64_t)blockIdx.x * MT + threadIdx.x; g < groups; g += (int64_t)gridDim.x * MT) {
    float o[4];
    int k = 4;
    if (g < full && vec) {
      const float4 v = *reinterpret_cast<const float4*>(opacity + 4 * g);
      o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    } else {
      k = (int)((P - 4 * g) < 4 ? (P - 4 * g) : 4);
#pragma unroll
      for (int j = 0; j < 4; j++) o[j] = j < k ? opacity[4 * g + j] : EOGS_REG_RETIRED_BELOW;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (o[j] <= EOGS_REG_RETIRED_BELOW) continue;  // eogs_reg.h's rule (a NaN logit is a row, as there)
      a[0] += (double)sigmoidf_(o[j]);
      a[1] += 1.;
    }
  }
  wg_partials<MT>(a, partial + 2 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(MT) void monitor_model_final_kernel(int nblk, const double* __restrict__ partial,
                                                                 const uint32_t* __restrict__ gate,
                                                                 eogs_monitor_state* __restrict__ st) {
  __shared__ double s_red[MT / 64];
  if (gate_closed(gate)) return;
  double tot[2];
  column_sums<MT>(partial, nblk, 2, tot, s_red);
  const double sum = tot[0], rows = tot[1];
  if (threadIdx.x != 0) return;
  st->mean_opacity = rows > 0. ? (float)(sum / rows) : 0.f;
  st->rows = (int64_t)rows;
}

// ---- the scalar steps ----------------------------------------------------------------------------------------------
__global__ void monitor_reset_kernel(eogs_monitor_state* __restrict__ st, int op) {
  uint64_t* w = reinterpret_cast<uint64_t*>(st);
  for (unsigned i = threadIdx.x; i < sizeof(eogs_monitor_state) / 8; i += blockDim.x) w[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) st->best = op == EOGS_MONITOR_MIN ? (double)INFINITY : -(double)INFINITY;  // callback_utils.py:6-9
}

__global__ void monitor_end_iteration_kernel(const float* __restrict__ loss, const uint32_t* __restrict__ gate,
                                             eogs_monitor_state* __restrict__ st) {
  if (threadIdx.x != 0 || gate_closed(gate)) return;
  st->ema_loss = 0.4 * (double)loss[0] + 0.6 * st->ema_loss;  // train_pan.py:492-495
  st->ema_photometric = 0.4 * (double)st->last[2] + 0.6 * st->ema_photometric;
  st->iteration += 1;
}

__global__ void monitor_close_kernel(int metric, int op, int64_t patience, const uint32_t* __restrict__ gate,
                                     eogs_monitor_state* __restrict__ st) {
  if (threadIdx.x != 0 || gate_closed(gate)) return;
  eogs_monitor_record& r = st->latest;  // (filled in place: `metric` indexes memory, not registers)
  const double d_photo = (double)(st->n_photo > 1 ? st->n_photo : 1), d_pan = (double)(st->n_pan > 1 ? st->n_pan : 1),
               d_msi = (double)(st->n_msi > 1 ? st->n_msi : 1);
  r.means[EOGS_MONITOR_PHOTOMETRIC] = st->sums[EOGS_MONITOR_PHOTOMETRIC] / d_photo;  // train_pan.py:512-519
  r.means[EOGS_MONITOR_L1] = st->sums[EOGS_MONITOR_L1] / d_photo;
  r.means[EOGS_MONITOR_PAN_PSNR] = st->sums[EOGS_MONITOR_PAN_PSNR] / d_pan;
  r.means[EOGS_MONITOR_PAN_SSIM] = st->sums[EOGS_MONITOR_PAN_SSIM] / d_pan;
  r.means[EOGS_MONITOR_MSI_PSNR] = st->sums[EOGS_MONITOR_MSI_PSNR] / d_msi;
  r.means[EOGS_MONITOR_MSI_SSIM] = st->sums[EOGS_MONITOR_MSI_SSIM] / d_msi;
  if (patience >= 0) {  // callback_utils.py:15-44
    const double m = r.means[metric];
    if (!(m == 0.)) {
      if (op == EOGS_MONITOR_MIN ? m < st->best : m > st->best) {
        st->best = m;
        st->counter = 0;
      } else {
        st->counter += 1;
        if (st->counter >= patience) st->early_stop = 1;
      }
    }
  }
  st->intervals += 1;
  r.interval = st->intervals;
  r.iteration = st->iteration;
  r.ema_loss = st->ema_loss;
  r.ema_photometric = st->ema_photometric;
  r.mean_opacity = (double)st->mean_opacity;
  r.rows = st->rows;
  r.best = st->best;
  r.counter = st->counter;
  r.early_stop = st->early_stop;
  r.reserved = 0;
  st->ring[(st->intervals - 1) % EOGS_MONITOR_RING] = r;
  for (int k = 0; k < EOGS_MONITOR_METRICS; k++) st->sums[k] = 0.;  // train_pan.py:580-597
  st->n_photo = st->n_pan = st->n_msi = 0;
}

}  // namespace

static size_t monitor_sq_bytes(int planes, int H, int W) {  // the per-plane partials of observe, a multiple of 256
  return (((size_t)planes * capped_blocks(((int64_t)H * W + 3) / 4, MT, MSQ_MAXBLK) * sizeof(double)) + 255) & ~(size_t)255;
}

static size_t monitor_model_ws_bytes(int64_t P) { return (size_t)capped_blocks((P + 3) / 4, MT, MMODEL_MAXBLK) * 2 * sizeof(double) + 256; }

static int monitor_state_check(const char* who, const void* state) {
  if (!state) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL state", who);
  if ((uintptr_t)state & 15u) return fail(EOGS_ERR_INVALID_ARG, "%s: state not 16-byte aligned", who);
  return EOGS_OK;
}

static int monitor_image_check(const char* who, int planes, int H, int W) {
  if (planes <= 0 || H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes", who);
  if (!loss_grid_fits(planes, H)) return fail(EOGS_ERR_INVALID_ARG, "%s: too many planes / rows for one launch", who);
  return EOGS_OK;
}

extern "C" {

int eogs_monitor_state_bytes(size_t* bytes) {
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "monitor_state_bytes: NULL argument");
  *bytes = sizeof(eogs_monitor_state);
  return EOGS_OK;
}

int eogs_monitor_reset(void* state, size_t state_bytes, int op, void* stream) {
  clear_error();
  const int rc = monitor_state_check("monitor_reset", state);
  if (rc != EOGS_OK) return rc;
  if (state_bytes < sizeof(eogs_monitor_state)) return fail(EOGS_ERR_WORKSPACE, "monitor_reset: state buffer too small");
  if (op != EOGS_MONITOR_MIN && op != EOGS_MONITOR_MAX) return fail(EOGS_ERR_INVALID_ARG, "monitor_reset: operator is min or max");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(monitor_reset_kernel, dim3(1), dim3(MT), 0, s, (eogs_monitor_state*)state, op);
  LAUNCH_TRY(s, false, "monitor_reset");
  return EOGS_OK;
}

int eogs_monitor_observe_bytes(int planes, int H, int W, int standalone, size_t* bytes) {
  const int rc = monitor_image_check("monitor_observe_bytes", planes, H, W);
  if (rc != EOGS_OK) return rc;
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe_bytes: NULL argument");
  size_t n = 256 + monitor_sq_bytes(planes, H, W);
  if (standalone) n += 256 + loss_layout(nullptr, planes, H, W, EOGS_LOSS_L1 | EOGS_LOSS_SSIM).bytes;
  *bytes = n;
  return EOGS_OK;
}

int eogs_monitor_observe(int planes, int H, int W, const float* image, const float* gt, const float* loss_out,
                         double lambda_dssim, int kind, int photometric_on, const uint32_t* gate, void* state, void* ws,
                         size_t ws_bytes, void* stream) {
  clear_error();
  int rc = monitor_image_check("monitor_observe", planes, H, W);
  if (rc != EOGS_OK) return rc;
  if (kind != EOGS_MONITOR_KIND_PAN && kind != EOGS_MONITOR_KIND_MSI)
    return fail(EOGS_ERR_INVALID_ARG, "monitor_observe: kind is pan or msi");
  if (!image || !gt || !ws) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe: NULL argument");
  if (!(lambda_dssim == lambda_dssim)) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe: lambda_dssim is NaN");
  rc = monitor_state_check("monitor_observe", state);
  if (rc != EOGS_OK) return rc;
  char* base = ws_base(ws);
  const size_t sq = monitor_sq_bytes(planes, H, W);
  size_t need = (size_t)(base - (char*)ws) + sq;
  LossWS w;
  const unsigned mode = EOGS_LOSS_L1 | EOGS_LOSS_SSIM;
  if (!loss_out) {
    w = loss_layout(base + sq + 256, planes, H, W, mode);
    need += 256 + w.bytes - 256;
  }
  if (need > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "monitor_observe: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const float lam = (float)lambda_dssim, oml = (float)(1.0 - lambda_dssim);  // torch rounds the Python scalars once each
  if (!loss_out) {
    float* out = reinterpret_cast<float*>(base + sq);
    { ProfScope ps(PS_LOSS_FWD, s); launch_loss_fwd(w, planes, H, W, image, gt, mode, oml, -lam, lam, out, nullptr, s); }
    loss_out = out;
  }
  const int64_t n = (int64_t)H * W;
  const int nb = capped_blocks((n + 3) / 4, MT, MSQ_MAXBLK);
  double* partial = reinterpret_cast<double*>(base);
  hipLaunchKernelGGL(monitor_sq_kernel, dim3(nb, planes), dim3(MT), 0, s, n, image, gt, partial);
  hipLaunchKernelGGL(monitor_observe_kernel, dim3(1), dim3(MT), 0, s, planes, nb, n, (const double*)partial, loss_out, oml, lam, kind,
                     photometric_on != 0, gate, (eogs_monitor_state*)state);
  LAUNCH_TRY(s, false, "monitor_observe");
  return EOGS_OK;
}

int eogs_monitor_model_bytes(int64_t P, size_t* bytes) {
  if (P <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "monitor_model_bytes: bad argument");
  *bytes = monitor_model_ws_bytes(P);
  return EOGS_OK;
}

int eogs_monitor_observe_model(int64_t P, const float* opacity, const uint32_t* gate, void* state, void* ws, size_t ws_bytes,
                               void* stream) {
  clear_error();
  if (P <= 0) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe_model: bad size");
  if (!opacity || !ws) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe_model: NULL argument");
  const int rc = monitor_state_check("monitor_observe_model", state);
  if (rc != EOGS_OK) return rc;
  if (ws_bytes < monitor_model_ws_bytes(P)) return fail(EOGS_ERR_WORKSPACE, "monitor_observe_model: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(ws_base(ws));
  const int nb = capped_blocks((P + 3) / 4, MT, MMODEL_MAXBLK);
  hipLaunchKernelGGL(monitor_model_kernel, dim3(nb), dim3(MT), 0, s, P, opacity, partial);
  hipLaunchKernelGGL(monitor_model_final_kernel, dim3(1), dim3(MT), 0, s, nb, (const double*)partial, gate,
                     (eogs_monitor_state*)state);
  LAUNCH_TRY(s, false, "monitor_observe_model");
  return EOGS_OK;
}

int eogs_monitor_end_iteration(const float* loss, const uint32_t* gate, void* state, void* stream) {
  clear_error();
  if (!loss) return fail(EOGS_ERR_INVALID_ARG, "monitor_end_iteration: NULL loss");
  const int rc = monitor_state_check("monitor_end_iteration", state);
  if (rc != EOGS_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(monitor_end_iteration_kernel, dim3(1), dim3(64), 0, s, loss, gate, (eogs_monitor_state*)state);
  LAUNCH_TRY(s, false, "monitor_end_iteration");
  return EOGS_OK;
}

int eogs_monitor_close_interval(int metric, int op, int64_t patience, const uint32_t* gate, void* state, void* stream) {
  clear_error();
  if (metric < 0 || metric >= EOGS_MONITOR_METRICS) return fail(EOGS_ERR_INVALID_ARG, "monitor_close_interval: unknown metric");
  if (op != EOGS_MONITOR_MIN && op != EOGS_MONITOR_MAX)
    return fail(EOGS_ERR_INVALID_ARG, "monitor_close_interval: operator is min or max");
  const int rc = monitor_state_check("monitor_close_interval", state);
  if (rc != EOGS_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(monitor_close_kernel, dim3(1), dim3(64), 0, s, metric, op, patience, gate, (eogs_monitor_state*)state);
  LAUNCH_TRY(s, false, "monitor_close_interval");
  return EOGS_OK;
}

}  // extern "C"
