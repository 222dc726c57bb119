// reg.hip — the regularisers of the training loss that read the model or a render directly (include/eogs_reg.h):
// opacity, visible-opacity and effective-rank terms over the raw Gaussian parameters; total variation of the altitude
// render and the accumulated-opacity term over render planes. Reference semantics: loss/opacity.py:14-17,30-35,44-45 and
// loss/main_loss.py:26-34,46-50 (under src/gaussiansplatting/).
//
// Elementwise work plus a handful of sums: HBM-bound by construction. One lane per Gaussian / per pixel in a grid-stride
// loop, nothing is saved between forward and backward (backward recomputes from the inputs), gradients are written once
// per element with plain stores. Sums: float64 per lane, per wave, per workgroup, then one workgroup combines the
// partials in a fixed order — no atomics, a grid that depends on the shape alone, bitwise reproducible. Weights and
// upstream gradients are read from device memory, so a recorded graph follows a caller that rewrites them.
#include "api_util.h"
#include "reduce.h"

namespace {

constexpr int RT = 256;         // threads per workgroup
constexpr int RMAXBLK = 1024;   // workgroups per launch (4 per CU); partial sums live in the caller's workspace
constexpr int RK = 4;           // doubles per workgroup partial

// ---- Gaussian-space terms ------------------------------------------------------------------------------------------
// main_loss.py:27-32 for one row; everything backward needs again
struct ErankRow {
  float s[3], s2[3], S, q[3], lq[3], e, t, m;
};

__device__ inline ErankRow erank_row(const float* __restrict__ l) {
  ErankRow r;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    r.s[k] = expf(l[k]);
    r.s2[k] = r.s[k] * r.s[k] + 1e-5f;
  }
  r.S = (r.s2[0] + r.s2[1]) + r.s2[2];
  float h = 0.f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    r.q[k] = r.s2[k] / r.S;
    r.lq[k] = logf(r.q[k] + 1e-6f);
    h += r.q[k] * r.lq[k];
  }
  r.e = expm1f(-h);
  r.t = -logf(r.e + 1e-5f);
  r.m = fminf(fminf(r.s2[0], r.s2[1]), r.s2[2]);
  return r;
}

__global__ __launch_bounds__(RT) void reg_gauss_fwd_kernel(int64_t P, unsigned want, const float* __restrict__ opacity,
                                                           const float* __restrict__ log_scales,
                                                           const int32_t* __restrict__ radii, double* __restrict__ partial) {
  double a[4] = {0., 0., 0., 0.};  // sum sigmoid, sum visible sigmoid, sum erank rows, rows that are not retired
  for (int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x; i < P; i += (int64_t)gridDim.x * RT) {
    const float o = opacity[i];
    if (o <= EOGS_REG_RETIRED_BELOW) continue;
    a[3] += 1.;
    if (want & (EOGS_REG_OPACITY | EOGS_REG_OPACITY_RADII)) {
      const float sg = sigmoidf_(o);
      a[0] += (double)sg;
      if ((want & EOGS_REG_OPACITY_RADII) && radii[i] > 0) a[1] += (double)sg;
    }
    if (want & EOGS_REG_ERANK) {
      const float l[3] = {log_scales[3 * i], log_scales[3 * i + 1], log_scales[3 * i + 2]};
      const ErankRow r = erank_row(l);
      a[2] += (double)(fmaxf(r.t, 0.f) + sqrtf(r.m));
    }
  }
  wg_partials<RT>(a, partial + (size_t)blockIdx.x * RK);
}

__global__ __launch_bounds__(RT) void reg_gauss_final_kernel(const double* __restrict__ partial, int nblk, unsigned want,
                                                             float n_init, const float* __restrict__ weights,
                                                             float* __restrict__ out) {
  __shared__ double s_red[RT / 64];
  double tot[4];
  for (int k = 0; k < 4; k++) tot[k] = column_sum<RT>(partial + k, nblk, RK, s_red);
  if (threadIdx.x != 0) return;
  const float t0 = (want & EOGS_REG_OPACITY) ? (float)(tot[0] / (double)n_init) : 0.f;
  const float t1 = (want & EOGS_REG_OPACITY_RADII) ? (float)(tot[1] / (double)n_init) : 0.f;
  const float t2 = ((want & EOGS_REG_ERANK) && tot[3] > 0.) ? (float)(tot[2] / tot[3]) : 0.f;
  float total = 0.f;
  if (want & EOGS_REG_OPACITY) total += weights[0] * t0;
  if (want & EOGS_REG_OPACITY_RADII) total += weights[1] * t1;
  if (want & EOGS_REG_ERANK) total += weights[2] * t2;
  out[0] = t0;
  out[1] = t1;
  out[2] = t2;
  out[3] = total;
  out[4] = (float)tot[3];
}

// Per row, in autograd's order:
//   opacity:  d/do = (c0 + [radii > 0] c1) / n_init * (1 - sg) sg
//   erank:    row = max(t, 0) + sqrt(m), t = -log(e + 1e-5), e = expm1(H), H = -sum_k q_k log(q_k + 1e-6), q = s2 / S
//             d/dt = c [t >= 0];  d/de = -d/dt / (e + 1e-5);  d/dH = d/de (e + 1);  d/dq_k = -d/dH (lq_k + q_k / (q_k + 1e-6))
//             d/ds2_k = d/dq_k / S - sum_j d/dq_j s2_j / S^2 + [s2_k == m] c / (2 sqrt(m) #minima);  d/dl_k = d/ds2_k 2 s_k s_k
//             with c = c2 / rows that are not retired
__global__ __launch_bounds__(RT) void reg_gauss_bwd_kernel(int64_t P, unsigned want, const float* __restrict__ opacity,
                                                           const float* __restrict__ log_scales,
                                                           const int32_t* __restrict__ radii, float n_init,
                                                           const float* __restrict__ weights, const float* __restrict__ out,
                                                           const float* __restrict__ g_total, const float* __restrict__ g_terms,
                                                           float* __restrict__ g_opacity, float* __restrict__ g_scaling) {
  const float gt = g_total ? g_total[0] : 0.f;
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c[k] = 0.f;
    if ((want >> k) & 1u) c[k] = (g_total ? gt * weights[k] : 0.f) + (g_terms ? g_terms[k] : 0.f);
  }
  const float c0 = c[0] / n_init, c1 = c[1] / n_init;
  const float rows = out[4];
  const float ce = rows > 0.f ? c[2] / rows : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x; i < P; i += (int64_t)gridDim.x * RT) {
    const float o = opacity[i];
    const bool alive = !(o <= EOGS_REG_RETIRED_BELOW);
    float go = 0.f;
    if (alive && (want & (EOGS_REG_OPACITY | EOGS_REG_OPACITY_RADII))) {
      const float sg = sigmoidf_(o);
      float up = c0;
      if ((want & EOGS_REG_OPACITY_RADII) && radii[i] > 0) up += c1;
      go = up * ((1.f - sg) * sg);
    }
    g_opacity[i] = go;
    if (!(want & EOGS_REG_ERANK)) continue;
    float gl[3] = {0.f, 0.f, 0.f};
    if (alive) {
      const float l[3] = {log_scales[3 * i], log_scales[3 * i + 1], log_scales[3 * i + 2]};
      const ErankRow r = erank_row(l);
      float gs2[3] = {0.f, 0.f, 0.f};
      if (r.t >= 0.f) {  // clip(min=0) passes the gradient at equality
        const float ge = ce / (r.e + 1e-5f);  // -d/de
        const float gh = ge * (r.e + 1.f);    // -d/dH (expm1' = result + 1)
        float gq[3], gS = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          gq[k] = gh * (r.lq[k] + r.q[k] / (r.q[k] + 1e-6f));  // d/dq_k: the sign of H = -sum cancels the one above
          gS += gq[k] * r.s2[k];
        }
        gS = -gS / (r.S * r.S);
#pragma unroll
        for (int k = 0; k < 3; k++) gs2[k] = gq[k] / r.S + gS;
      }
      const int ties = (r.s2[0] == r.m) + (r.s2[1] == r.m) + (r.s2[2] == r.m);  // amin: an even split among exact ties
      const float gm = ce * 0.5f / sqrtf(r.m) / (float)ties;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (r.s2[k] == r.m) gs2[k] += gm;
        gl[k] = gs2[k] * (2.f * r.s[k]) * r.s[k];
      }
    }
    g_scaling[3 * i] = gl[0];
    g_scaling[3 * i + 1] = gl[1];
    g_scaling[3 * i + 2] = gl[2];
  }
}

// ---- render-space terms --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) void reg_image_fwd_kernel(int H, int W, const float* __restrict__ alt,
                                                           const float* __restrict__ acc, double* __restrict__ partial) {
  const int64_t n = (int64_t)H * W;
  double a[3] = {0., 0., 0.};  // sum of |vertical differences|, of |horizontal differences|, of 1 - acc
  for (int64_t p = (int64_t)blockIdx.x * RT + threadIdx.x; p < n; p += (int64_t)gridDim.x * RT) {
    if (alt) {
      const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
      const float v = alt[p];
      if (y + 1 < H) a[0] += (double)fabsf(alt[p + W] - v);
      if (x + 1 < W) a[1] += (double)fabsf(alt[p + 1] - v);
    }
    if (acc) a[2] += (double)(1.f - acc[p]);
  }
  wg_partials<RT>(a, partial + (size_t)blockIdx.x * RK);
}

__global__ __launch_bounds__(RT) void reg_image_final_kernel(const double* __restrict__ partial, int nblk, int H, int W,
                                                             bool has_alt, bool has_acc, const float* __restrict__ weights,
                                                             float* __restrict__ out) {
  __shared__ double s_red[RT / 64];
  double tot[3];
  for (int k = 0; k < 3; k++) tot[k] = column_sum<RT>(partial + k, nblk, RK, s_red);
  if (threadIdx.x != 0) return;
  const double nv = (double)(H - 1) * (double)W, nh = (double)H * (double)(W - 1), n = (double)H * (double)W;
  const float t0 = has_alt ? (float)(0.5 * (tot[0] / nv + tot[1] / nh)) : 0.f;
  const float t1 = has_acc ? (float)(tot[2] / n) : 0.f;
  float total = 0.f;
  if (has_alt) total += weights[0] * t0;
  if (has_acc) total += weights[1] * t1;
  out[0] = t0;
  out[1] = t1;
  out[2] = total;
}

__global__ __launch_bounds__(RT) void reg_image_bwd_kernel(int H, int W, const float* __restrict__ alt, bool has_acc,
                                                           const float* __restrict__ weights, const float* __restrict__ g_total,
                                                           const float* __restrict__ g_terms, float* __restrict__ g_alt,
                                                           float* __restrict__ g_acc) {
  const int64_t n = (int64_t)H * W;
  const float gt = g_total ? g_total[0] : 0.f;
  const float c0 = (g_total ? gt * weights[0] : 0.f) + (g_terms ? g_terms[0] : 0.f);
  const float c1 = (g_total ? gt * weights[1] : 0.f) + (g_terms ? g_terms[1] : 0.f);
  const float cv = (0.5f * c0) / (float)((int64_t)(H - 1) * W), ch = (0.5f * c0) / (float)((int64_t)H * (W - 1));
  const float ca = -(c1 / (float)n);
  for (int64_t p = (int64_t)blockIdx.x * RT + threadIdx.x; p < n; p += (int64_t)gridDim.x * RT) {
    if (alt) {
      const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
      const float v = alt[p];
      float dv = 0.f, dh = 0.f;  // sign(v - above) - sign(below - v), sign(v - left) - sign(right - v)
      if (y > 0) dv += sgn(v - alt[p - W]);
      if (y + 1 < H) dv -= sgn(alt[p + W] - v);
      if (x > 0) dh += sgn(v - alt[p - 1]);
      if (x + 1 < W) dh -= sgn(alt[p + 1] - v);
      g_alt[p] = cv * dv + ch * dh;
    }
    if (has_acc) g_acc[p] = ca;
  }
}

}  // namespace

static size_t reg_ws_bytes() { return (size_t)RMAXBLK * RK * sizeof(double) + 256; }

static int reg_gauss_check(const char* who, int64_t P, unsigned want, const float* opacity, const float* log_scales,
                           const int32_t* radii, float n_init, const float* weights) {
  if (P <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad size", who);
  if (want == 0u || (want & ~(EOGS_REG_OPACITY | EOGS_REG_OPACITY_RADII | EOGS_REG_ERANK)))
    return fail(EOGS_ERR_INVALID_ARG, "%s: `want` selects at least one of the three terms and nothing else", who);
  if (!opacity || !weights) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if ((want & EOGS_REG_ERANK) && !log_scales) return fail(EOGS_ERR_INVALID_ARG, "%s: the erank term needs log_scales (NULL argument)", who);
  if ((want & EOGS_REG_OPACITY_RADII) && !radii) return fail(EOGS_ERR_INVALID_ARG, "%s: the visible-opacity term needs radii (NULL argument)", who);
  if ((want & (EOGS_REG_OPACITY | EOGS_REG_OPACITY_RADII)) && !(n_init > 0.f))
    return fail(EOGS_ERR_INVALID_ARG, "%s: n_init must be positive", who);
  return EOGS_OK;
}

extern "C" {

int eogs_reg_gauss_bytes(int64_t P, size_t* bytes) {
  clear_error();
  if (P <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "reg_gauss_bytes: bad argument");
  *bytes = reg_ws_bytes();
  return EOGS_OK;
}

int eogs_reg_gauss_forward(int64_t P, unsigned want, const float* opacity, const float* log_scales, const int32_t* radii,
                           float n_init, const float* weights, float* out, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const int rc = reg_gauss_check("reg_gauss_forward", P, want, opacity, log_scales, radii, n_init, weights);
  if (rc != EOGS_OK) return rc;
  if (!out || !ws) return fail(EOGS_ERR_INVALID_ARG, "reg_gauss_forward: NULL argument");
  if (ws_bytes < reg_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "reg_gauss_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(ws_base(ws));
  const int nb = capped_blocks(P, RT, RMAXBLK);
  {
    ProfScope ps(PS_REG_FWD, s);
    hipLaunchKernelGGL(reg_gauss_fwd_kernel, dim3(nb), dim3(RT), 0, s, P, want, opacity, log_scales, radii, partial);
    hipLaunchKernelGGL(reg_gauss_final_kernel, dim3(1), dim3(RT), 0, s, (const double*)partial, nb, want, n_init, weights, out);
  }
  LAUNCH_TRY(s, false, "reg_gauss_fwd");
  return EOGS_OK;
}

int eogs_reg_gauss_backward(int64_t P, unsigned want, const float* opacity, const float* log_scales, const int32_t* radii,
                            float n_init, const float* weights, const float* out, const float* g_total,
                            const float* g_terms, float* g_opacity, float* g_scaling, void* stream) {
  clear_error();
  const int rc = reg_gauss_check("reg_gauss_backward", P, want, opacity, log_scales, radii, n_init, weights);
  if (rc != EOGS_OK) return rc;
  if (!out || !g_opacity) return fail(EOGS_ERR_INVALID_ARG, "reg_gauss_backward: NULL argument");
  if (((want & EOGS_REG_ERANK) != 0u) != (g_scaling != nullptr))
    return fail(EOGS_ERR_INVALID_ARG, "reg_gauss_backward: g_scaling goes with the erank term");
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(PS_REG_BWD, s);
    hipLaunchKernelGGL(reg_gauss_bwd_kernel, dim3(capped_blocks(P, RT, RMAXBLK)), dim3(RT), 0, s, P, want, opacity, log_scales, radii, n_init,
                       weights, out, g_total, g_terms, g_opacity, g_scaling);
  }
  LAUNCH_TRY(s, false, "reg_gauss_bwd");
  return EOGS_OK;
}

int eogs_reg_image_bytes(int H, int W, size_t* bytes) {
  clear_error();
  if (H < 2 || W < 2 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "reg_image_bytes: bad argument");
  *bytes = reg_ws_bytes();
  return EOGS_OK;
}

int eogs_reg_image_forward(int H, int W, const float* altitude, const float* accumulated_opacity, const float* weights,
                           float* out, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (H < 2 || W < 2) return fail(EOGS_ERR_INVALID_ARG, "reg_image_forward: bad sizes (H and W must be at least 2)");
  if ((!altitude && !accumulated_opacity) || !weights || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "reg_image_forward: NULL argument");
  if (ws_bytes < reg_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "reg_image_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(ws_base(ws));
  const int nb = capped_blocks((int64_t)H * W, RT, RMAXBLK);
  {
    ProfScope ps(PS_REG_FWD, s);
    hipLaunchKernelGGL(reg_image_fwd_kernel, dim3(nb), dim3(RT), 0, s, H, W, altitude, accumulated_opacity, partial);
    hipLaunchKernelGGL(reg_image_final_kernel, dim3(1), dim3(RT), 0, s, (const double*)partial, nb, H, W, altitude != nullptr,
                       accumulated_opacity != nullptr, weights, out);
  }
  LAUNCH_TRY(s, false, "reg_image_fwd");
  return EOGS_OK;
}

int eogs_reg_image_backward(int H, int W, const float* altitude, const float* accumulated_opacity, const float* weights,
                            const float* g_total, const float* g_terms, float* g_altitude, float* g_accumulated_opacity,
                            void* stream) {
  clear_error();
  if (H < 2 || W < 2) return fail(EOGS_ERR_INVALID_ARG, "reg_image_backward: bad sizes (H and W must be at least 2)");
  if ((!altitude && !accumulated_opacity) || !weights) return fail(EOGS_ERR_INVALID_ARG, "reg_image_backward: NULL argument");
  if ((altitude != nullptr) != (g_altitude != nullptr) || (accumulated_opacity != nullptr) != (g_accumulated_opacity != nullptr))
    return fail(EOGS_ERR_INVALID_ARG, "reg_image_backward: a gradient plane goes with its input, NULL with NULL");
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(PS_REG_BWD, s);
    hipLaunchKernelGGL(reg_image_bwd_kernel, dim3(capped_blocks((int64_t)H * W, RT, RMAXBLK)), dim3(RT), 0, s, H, W, altitude,
                       accumulated_opacity != nullptr, weights, g_total, g_terms, g_altitude, g_accumulated_opacity);
  }
  LAUNCH_TRY(s, false, "reg_image_bwd");
  return EOGS_OK;
}

}  // extern "C"
