// pan.hip — the panchromatic camera's render pipeline (include/eogs_pan.h): colour correction, shadow and the MSI->PAN
// map fused into one kernel each way. Reference semantics: scene/cameras/PAN_affine_cameras.py:83-176,
// scene/cameras/affine_cameras.py:33-40, scene/msi_to_pan/transf_msi_to_pan.py (all under src/gaussiansplatting/).
//
// Pure streaming work, HBM-bound like shade.hip: every input plane is read once and every output written once, V = 4
// pixels (one 16-byte access per plane) per lane and trip where H*W and the pointers allow it, V = 1 otherwise. The
// order of the pipeline, the map and the presence of the shadow term are launch-uniform and therefore template
// parameters: the pixel loop carries no branch on them. Nothing is saved between forward and backward. The parameter
// sums go through reduce.h's two stages (one workgroup of the second kernel per column) — no atomics, bitwise reproducible.
#include "api_util.h"
#include "reduce.h"

namespace {

constexpr int PT = 256;               // threads per workgroup
constexpr int PMAXBLK = 1024;         // workgroups per launch (4 per CU); partial sums live in the caller's workspace
constexpr int PK = EOGS_PAN_NPARAMS;  // floats per workgroup partial: dM[12], dinshadow[3], dmap_params[5]
constexpr int A_INS = 12, A_MAP = 15;

__host__ __device__ constexpr int map_nparams(int kind) {
  return kind == EOGS_PAN_FIXED ? 5
         : (kind == EOGS_PAN_BASE || kind == EOGS_PAN_BASE_SIGMOID || kind == EOGS_PAN_TRANSLATE_FROZEN) ? 4
         : kind == EOGS_PAN_TRANSLATE ? 8
                                      : 0;
}

template <int V>
__device__ inline void ldv(const float* __restrict__ p, float (&o)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
  } else {
    o[0] = *p;
  }
}

template <int V>
__device__ inline void stv(float* __restrict__ p, const float (&o)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
    *p = o[0];
  }
}

template <int KIND>
__device__ inline float map_fwd(const float (&mp)[8], float x0, float x1, float x2) {
  if constexpr (KIND == EOGS_PAN_ONE_CHANNEL) return x0;
  if constexpr (KIND == EOGS_PAN_AVERAGE) return (x0 + x1 + x2) / 3.f;
  if constexpr (KIND == EOGS_PAN_FIXED) return mp[3] * (mp[0] * x0 + mp[1] * x1 + mp[2] * x2 + mp[4]);
  if constexpr (KIND == EOGS_PAN_BASE) return mp[0] * x0 + mp[1] * x1 + mp[2] * x2 + mp[3];
  if constexpr (KIND == EOGS_PAN_BASE_SIGMOID) return 1.f / (1.f + expf(-(mp[0] * x0 + mp[1] * x1 + mp[2] * x2 + mp[3])));
  if constexpr (KIND == EOGS_PAN_TRANSLATE)
    return (mp[4] * x0 + mp[5] * x1 + mp[6] * x2 + mp[7]) + (mp[0] * x0 + mp[1] * x1 + mp[2] * x2 + mp[3]);
  if constexpr (KIND == EOGS_PAN_TRANSLATE_FROZEN) return mp[0] * x0 + mp[1] * x1 + mp[2] * x2 + mp[3];
  return 0.f;
}

// dx[k] = g dmap/dx[k]; am[] += g dmap/dmap_params[] in the layout of g_params[15..19]
template <int KIND>
__device__ inline void map_bwd(const float (&mp)[8], const float (&x)[3], float g, float (&dx)[3], float* __restrict__ am) {
  if constexpr (KIND == EOGS_PAN_ONE_CHANNEL) {
    dx[0] = g, dx[1] = 0.f, dx[2] = 0.f;
  } else if constexpr (KIND == EOGS_PAN_AVERAGE) {
    dx[0] = dx[1] = dx[2] = g / 3.f;
  } else if constexpr (KIND == EOGS_PAN_FIXED) {
    const float inner = mp[0] * x[0] + mp[1] * x[1] + mp[2] * x[2] + mp[4];
    const float gi = g * mp[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      dx[k] = gi * mp[k];
      am[k] += gi * x[k];
    }
    am[3] += g * inner;
    am[4] += gi;
  } else if constexpr (KIND == EOGS_PAN_BASE || KIND == EOGS_PAN_BASE_SIGMOID) {
    float gz = g;
    if constexpr (KIND == EOGS_PAN_BASE_SIGMOID) {
      const float y = 1.f / (1.f + expf(-(mp[0] * x[0] + mp[1] * x[1] + mp[2] * x[2] + mp[3])));
      gz = g * (y * (1.f - y));
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      dx[k] = gz * mp[k];
      am[k] += gz * x[k];
    }
    am[3] += gz;
  } else if constexpr (KIND == EOGS_PAN_TRANSLATE) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      dx[k] = g * mp[4 + k];
      am[k] += g * x[k];
    }
    am[3] += g;
  } else {
    dx[0] = dx[1] = dx[2] = 0.f;
  }
}

template <int ORDER, int KIND>
__device__ inline void load_params(const float* __restrict__ Mp, const float* __restrict__ insp, const float* __restrict__ mpp,
                                   bool shadow, float (&M)[12], float (&ins)[3], float (&mp)[8]) {
  constexpr int NM = ORDER == EOGS_PAN_ORDER_CC_FIRST ? 12 : 2, NI = ORDER == EOGS_PAN_ORDER_CC_FIRST ? 3 : 1;
#pragma unroll
  for (int i = 0; i < 12; i++) M[i] = i < NM ? Mp[i] : 0.f;
#pragma unroll
  for (int i = 0; i < 3; i++) ins[i] = (shadow && i < NI) ? insp[i] : 0.f;
#pragma unroll
  for (int i = 0; i < 8; i++) mp[i] = i < map_nparams(KIND) ? mpp[i] : 0.f;
}

template <int ORDER, int KIND, bool SH, int V>
__global__ __launch_bounds__(PT) void pan_fwd_kernel(int64_t n, const float* __restrict__ raw, const float* __restrict__ alt_diff,
                                                     const float* __restrict__ Mp, const float* __restrict__ insp,
                                                     const float* __restrict__ mpp, float* __restrict__ cc,
                                                     float* __restrict__ shaded, float* __restrict__ shadow) {
  constexpr bool A = ORDER == EOGS_PAN_ORDER_CC_FIRST;
  float M[12], ins[3], mp[8];
  load_params<ORDER, KIND>(Mp, insp, mpp, SH, M, ins, mp);
  const int64_t nv = n / V;  // V == 4 only when n is a multiple of 4
  for (int64_t i = (int64_t)blockIdx.x * PT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * PT) {
    const int64_t p = i * V;
    float r[3][V], d[V], oc[3][V], os[V], ow[V];
#pragma unroll
    for (int k = 0; k < 3; k++) ldv<V>(raw + k * n + p, r[k]);
    if constexpr (SH) ldv<V>(alt_diff + p, d);
#pragma unroll
    for (int v = 0; v < V; v++) {
      float s = 1.f;
      if constexpr (SH) ow[v] = s = expf(0.4f * shadow_clip(d[v]));
      if constexpr (A) {
        float c[3], x[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          oc[k][v] = c[k] = M[4 * k] * r[0][v] + M[4 * k + 1] * r[1][v] + M[4 * k + 2] * r[2][v] + M[4 * k + 3];
          x[k] = SH ? s * c[k] + ((1.f - s) * ins[k]) * c[k] : c[k];
        }
        os[v] = map_fwd<KIND>(mp, x[0], x[1], x[2]);
      } else {
        const float p0 = map_fwd<KIND>(mp, r[0][v], r[1][v], r[2][v]);
        const float c = M[0] * p0 + M[1];
        oc[0][v] = c;
        os[v] = SH ? s * c + ((1.f - s) * ins[0]) * c : p0;
      }
    }
    if constexpr (A) {
      if (cc) {
#pragma unroll
        for (int k = 0; k < 3; k++) stv<V>(cc + k * n + p, oc[k]);
      }
    } else {
      stv<V>(cc + p, oc[0]);
    }
    stv<V>(shaded + p, os);
    if constexpr (SH) stv<V>(shadow + p, ow);
  }
}

// CC_FIRST, with x_c = cc_c f_c, f_c = s + (1 - s) ins_c and g3_c = g_shaded dmap/dx_c:
//   d/dcc_c = f_c g3_c (+ g_cc_c);  d/ds = sum_c g3_c cc_c (1 - ins_c) (+ g_shadow);  d/dins_c = sum_p g3_c (1 - s) cc_c
//   d/draw_k = sum_c M[c][k] d/dcc_c;  d/dM[c][k] = sum_p d/dcc_c raw_k;  d/dM[c][3] = sum_p d/dcc_c
// MAP_FIRST, with p0 = map(raw), cc = w p0 + b, f = s + (1 - s) ins:
//   shadow:    d/dcc = f g_shaded (+ g_cc);  d/ds = g_shaded cc (1 - ins) (+ g_shadow);  d/dp0 = w d/dcc
//   no shadow: d/dcc = g_cc;  d/dp0 = g_shaded + w d/dcc          (shaded is p0 there, eogs_pan.h)
//   d/dw = sum_p d/dcc p0;  d/db = sum_p d/dcc;  d/draw_k = d/dp0 dmap/draw_k
// Both: d/dalt_diff = d/ds * 0.4 s [alt_diff <= 0]   (torch.clamp(max=0) passes the gradient at equality)
template <int ORDER, int KIND, bool SH, int V>
__global__ __launch_bounds__(PT) void pan_bwd_kernel(int64_t n, const float* __restrict__ raw, const float* __restrict__ alt_diff,
                                                     const float* __restrict__ Mp, const float* __restrict__ insp,
                                                     const float* __restrict__ mpp, const float* __restrict__ g_shaded,
                                                     const float* __restrict__ g_cc, const float* __restrict__ g_shadow,
                                                     float* __restrict__ g_raw, float* __restrict__ g_alt,
                                                     float* __restrict__ partial) {
  constexpr bool A = ORDER == EOGS_PAN_ORDER_CC_FIRST;
  constexpr int NCC = A ? 3 : 1;
  float M[12], ins[3], mp[8];
  load_params<ORDER, KIND>(Mp, insp, mpp, SH, M, ins, mp);
  float acc[PK];
#pragma unroll
  for (int i = 0; i < PK; i++) acc[i] = 0.f;
  const int64_t nv = n / V;
  for (int64_t i = (int64_t)blockIdx.x * PT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * PT) {
    const int64_t p = i * V;
    float r[3][V], d[V], gsd[V], gc[NCC][V], gsw[V], og[3][V], oa[V];
#pragma unroll
    for (int k = 0; k < 3; k++) ldv<V>(raw + k * n + p, r[k]);
    if constexpr (SH) ldv<V>(alt_diff + p, d);
    if (g_shaded) {
      ldv<V>(g_shaded + p, gsd);
    } else {
#pragma unroll
      for (int v = 0; v < V; v++) gsd[v] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < NCC; k++) {
      if (g_cc) {
        ldv<V>(g_cc + k * n + p, gc[k]);
      } else {
#pragma unroll
        for (int v = 0; v < V; v++) gc[k][v] = 0.f;
      }
    }
    if (SH && g_shadow) {
      ldv<V>(g_shadow + p, gsw);
    } else {
#pragma unroll
      for (int v = 0; v < V; v++) gsw[v] = 0.f;
    }
#pragma unroll
    for (int v = 0; v < V; v++) {
      const float rv[3] = {r[0][v], r[1][v], r[2][v]};
      float s = 1.f;
      if constexpr (SH) s = expf(0.4f * shadow_clip(d[v]));
      float gs = gsw[v];
      if constexpr (A) {
        float c[3], x[3], g3[3], gcc[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          c[k] = M[4 * k] * rv[0] + M[4 * k + 1] * rv[1] + M[4 * k + 2] * rv[2] + M[4 * k + 3];
          x[k] = SH ? s * c[k] + ((1.f - s) * ins[k]) * c[k] : c[k];
        }
        map_bwd<KIND>(mp, x, gsd[v], g3, acc + A_MAP);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          if constexpr (SH) {
            gcc[k] = g3[k] * (s + (1.f - s) * ins[k]) + gc[k][v];
            gs += g3[k] * c[k] * (1.f - ins[k]);
            acc[A_INS + k] += g3[k] * (1.f - s) * c[k];
          } else {
            gcc[k] = g3[k] + gc[k][v];
          }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
          og[k][v] = M[k] * gcc[0] + M[4 + k] * gcc[1] + M[8 + k] * gcc[2];
          acc[4 * k] += gcc[k] * rv[0];
          acc[4 * k + 1] += gcc[k] * rv[1];
          acc[4 * k + 2] += gcc[k] * rv[2];
          acc[4 * k + 3] += gcc[k];
        }
      } else {
        const float p0 = map_fwd<KIND>(mp, rv[0], rv[1], rv[2]);
        const float c = M[0] * p0 + M[1];
        float gcc, gp0, dx[3];
        if constexpr (SH) {
          gcc = gsd[v] * (s + (1.f - s) * ins[0]) + gc[0][v];
          gs += gsd[v] * c * (1.f - ins[0]);
          acc[A_INS] += gsd[v] * (1.f - s) * c;
          gp0 = M[0] * gcc;
        } else {
          gcc = gc[0][v];
          gp0 = gsd[v] + M[0] * gcc;
        }
        acc[0] += gcc * p0;
        acc[1] += gcc;
        map_bwd<KIND>(mp, rv, gp0, dx, acc + A_MAP);
#pragma unroll
        for (int k = 0; k < 3; k++) og[k][v] = dx[k];
      }
      if constexpr (SH) oa[v] = d[v] <= 0.f ? gs * 0.4f * s : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) stv<V>(g_raw + k * n + p, og[k]);
    if constexpr (SH) stv<V>(g_alt + p, oa);
  }
  wg_partials<PT>(acc, partial + (size_t)blockIdx.x * PK);
}

// out[k] = sum_b partial[b][k]: workgroup k sums column k of the [nblk][PK] partials in a fixed order
__global__ __launch_bounds__(PT) void pan_reduce_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ out) {
  __shared__ float s_red[PT / 64];
  const float tot = column_sum<PT>(partial + blockIdx.x, nblk, PK, s_red);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

struct PanArgs {
  int64_t n;
  const float *raw, *alt_diff, *M, *ins, *mp, *g_shaded, *g_cc, *g_shadow;
  float *cc, *shaded, *shadow, *g_raw, *g_alt, *partial;
  bool bwd, vec;
  int nb;
  hipStream_t s;
};

template <int ORDER, int KIND, bool SH, int V>
void pan_launch(const PanArgs& a) {
  if (a.bwd)
    hipLaunchKernelGGL((pan_bwd_kernel<ORDER, KIND, SH, V>), dim3(a.nb), dim3(PT), 0, a.s, a.n, a.raw, a.alt_diff, a.M, a.ins, a.mp,
                       a.g_shaded, a.g_cc, a.g_shadow, a.g_raw, a.g_alt, a.partial);
  else
    hipLaunchKernelGGL((pan_fwd_kernel<ORDER, KIND, SH, V>), dim3(a.nb), dim3(PT), 0, a.s, a.n, a.raw, a.alt_diff, a.M, a.ins, a.mp,
                       a.cc, a.shaded, a.shadow);
}

template <int ORDER, int KIND>
void pan_launch_kind(const PanArgs& a) {
  if (a.alt_diff) {
    if (a.vec) pan_launch<ORDER, KIND, true, 4>(a);
    else pan_launch<ORDER, KIND, true, 1>(a);
  } else {
    if (a.vec) pan_launch<ORDER, KIND, false, 4>(a);
    else pan_launch<ORDER, KIND, false, 1>(a);
  }
}

template <int ORDER>
void pan_launch_order(int kind, const PanArgs& a) {
  switch (kind) {
    case EOGS_PAN_ONE_CHANNEL: return pan_launch_kind<ORDER, EOGS_PAN_ONE_CHANNEL>(a);
    case EOGS_PAN_AVERAGE: return pan_launch_kind<ORDER, EOGS_PAN_AVERAGE>(a);
    case EOGS_PAN_FIXED: return pan_launch_kind<ORDER, EOGS_PAN_FIXED>(a);
    case EOGS_PAN_BASE: return pan_launch_kind<ORDER, EOGS_PAN_BASE>(a);
    case EOGS_PAN_BASE_SIGMOID: return pan_launch_kind<ORDER, EOGS_PAN_BASE_SIGMOID>(a);
    case EOGS_PAN_TRANSLATE: return pan_launch_kind<ORDER, EOGS_PAN_TRANSLATE>(a);
    default: return pan_launch_kind<ORDER, EOGS_PAN_TRANSLATE_FROZEN>(a);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

void pan_dispatch(int order, int kind, PanArgs& a) {
  // 16-byte accesses need every plane of every image to start on a 16-byte boundary: base pointers aligned, H*W % 4 == 0
  a.vec = (a.n % 4 == 0) && aligned16(a.raw) && aligned16(a.alt_diff) && aligned16(a.g_shaded) && aligned16(a.g_cc) &&
          aligned16(a.g_shadow) && aligned16(a.cc) && aligned16(a.shaded) && aligned16(a.shadow) && aligned16(a.g_raw) &&
          aligned16(a.g_alt);
  a.nb = capped_blocks(a.vec ? a.n / 4 : a.n, PT, PMAXBLK);
  if (order == EOGS_PAN_ORDER_CC_FIRST) pan_launch_order<EOGS_PAN_ORDER_CC_FIRST>(kind, a);
  else pan_launch_order<EOGS_PAN_ORDER_MAP_FIRST>(kind, a);
}

}  // namespace

static size_t pan_ws_bytes() { return (size_t)PMAXBLK * PK * sizeof(float) + 256; }

static int pan_check(const char* who, int H, int W, int order, int kind, const float* raw, const float* alt_diff, const float* M,
                     const float* inshadow, const float* map_params) {
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes", who);
  if (order != EOGS_PAN_ORDER_CC_FIRST && order != EOGS_PAN_ORDER_MAP_FIRST) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown order", who);
  if (kind < EOGS_PAN_ONE_CHANNEL || kind > EOGS_PAN_TRANSLATE_FROZEN) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown map kind", who);
  if (!raw || !M) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (alt_diff && !inshadow) return fail(EOGS_ERR_INVALID_ARG, "%s: alt_diff needs inshadow (NULL argument)", who);
  if (map_nparams(kind) > 0 && !map_params) return fail(EOGS_ERR_INVALID_ARG, "%s: this map kind needs map_params (NULL argument)", who);
  return EOGS_OK;
}

extern "C" {

int eogs_pan_bytes(int H, int W, size_t* bytes) {
  clear_error();
  if (H <= 0 || W <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "pan_bytes: bad argument");
  *bytes = pan_ws_bytes();
  return EOGS_OK;
}

int eogs_pan_forward(int H, int W, int order, int kind, const float* raw, const float* alt_diff, const float* M,
                     const float* inshadow, const float* map_params, float* cc, float* shaded, float* shadow,
                     void* stream) {
  clear_error();
  const int rc = pan_check("pan_forward", H, W, order, kind, raw, alt_diff, M, inshadow, map_params);
  if (rc != EOGS_OK) return rc;
  if (!shaded || (order == EOGS_PAN_ORDER_MAP_FIRST && !cc)) return fail(EOGS_ERR_INVALID_ARG, "pan_forward: NULL argument");
  if ((alt_diff != nullptr) != (shadow != nullptr)) return fail(EOGS_ERR_INVALID_ARG, "pan_forward: alt_diff and shadow go together");
  hipStream_t s = (hipStream_t)stream;
  PanArgs a{};
  a.n = (int64_t)H * W;
  a.raw = raw, a.alt_diff = alt_diff, a.M = M, a.ins = inshadow, a.mp = map_params;
  a.cc = cc, a.shaded = shaded, a.shadow = shadow;
  a.bwd = false, a.s = s;
  pan_dispatch(order, kind, a);
  LAUNCH_TRY(s, false, "pan_fwd");
  return EOGS_OK;
}

int eogs_pan_backward(int H, int W, int order, int kind, const float* raw, const float* alt_diff, const float* M,
                      const float* inshadow, const float* map_params, const float* g_shaded, const float* g_cc,
                      const float* g_shadow, float* g_raw, float* g_alt_diff, float* g_params, void* ws, size_t ws_bytes,
                      void* stream) {
  clear_error();
  const int rc = pan_check("pan_backward", H, W, order, kind, raw, alt_diff, M, inshadow, map_params);
  if (rc != EOGS_OK) return rc;
  if (!g_raw || !g_params || !ws) return fail(EOGS_ERR_INVALID_ARG, "pan_backward: NULL argument");
  if ((alt_diff != nullptr) != (g_alt_diff != nullptr) || (!alt_diff && g_shadow))
    return fail(EOGS_ERR_INVALID_ARG, "pan_backward: alt_diff, g_shadow and g_alt_diff go together");
  if (ws_bytes < pan_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "pan_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  PanArgs a{};
  a.n = (int64_t)H * W;
  a.raw = raw, a.alt_diff = alt_diff, a.M = M, a.ins = inshadow, a.mp = map_params;
  a.g_shaded = g_shaded, a.g_cc = g_cc, a.g_shadow = g_shadow, a.g_raw = g_raw, a.g_alt = g_alt_diff;
  a.partial = reinterpret_cast<float*>(ws_base(ws));
  a.bwd = true, a.s = s;
  pan_dispatch(order, kind, a);
  hipLaunchKernelGGL(pan_reduce_kernel, dim3(PK), dim3(PT), 0, s, (const float*)a.partial, a.nb, g_params);
  LAUNCH_TRY(s, false, "pan_bwd");
  return EOGS_OK;
}

}  // extern "C"
