// randomcam_compose.h — the two matrices of the shadow-mapped virtual view (include/eogs_randomcam.h): one text for the
// kernel of csrc/randomcam.hip and for the host program that checks it against numpy (tests/randomcam_compose_host.cpp).
// Plain C++ over float and double: no HIP header, no library call. The library is built with -ffp-contract=off, and so is
// the host program: every product and sum below is rounded on its own.
//
//   virt_to_sun = C^-1 . S     (renderer_cc_shadow.py:93-95: torch.inverse(cam2virt), torch.matmul(cam2virt_inv, camera_to_sun))
//   K           = virt_to_sun . C
//
// all in double over the fp32 inputs; C^-1 = adj(C) / det(C). Each of the 18 results is rounded to fp32 once.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RANDOMCAM_HD __host__ __device__
#else
#define RANDOMCAM_HD
#endif

// c, s: row-major 3 x 3. out[0..9) = virt_to_sun, out[9..18) = K. det(c) zero or not finite: NaN in all 18.
RANDOMCAM_HD inline void randomcam_compose(const float c[9], const float s[9], float out[18]) {
  double C[9], S[9];
  for (int i = 0; i < 9; i++) {
    C[i] = (double)c[i];
    S[i] = (double)s[i];
  }
  // cofactors of the first row's expansion first: det = C[0] adj[0] + C[1] adj[3] + C[2] adj[6]
  double adj[9];
  adj[0] = C[4] * C[8] - C[5] * C[7];
  adj[1] = C[2] * C[7] - C[1] * C[8];
  adj[2] = C[1] * C[5] - C[2] * C[4];
  adj[3] = C[5] * C[6] - C[3] * C[8];
  adj[4] = C[0] * C[8] - C[2] * C[6];
  adj[5] = C[2] * C[3] - C[0] * C[5];
  adj[6] = C[3] * C[7] - C[4] * C[6];
  adj[7] = C[1] * C[6] - C[0] * C[7];
  adj[8] = C[0] * C[4] - C[1] * C[3];
  const double det = (C[0] * adj[0] + C[1] * adj[3]) + C[2] * adj[6];
  // (a NaN fails both comparisons; an infinity is caught by det - det)
  const bool ok = (det > 0.0 || det < 0.0) && (det - det == 0.0);
  if (!ok) {
    const float nan = __builtin_nanf("");
    for (int i = 0; i < 18; i++) out[i] = nan;
    return;
  }
  double inv[9], V[9];
  for (int i = 0; i < 9; i++) inv[i] = adj[i] / det;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) V[3 * i + j] = (inv[3 * i] * S[j] + inv[3 * i + 1] * S[3 + j]) + inv[3 * i + 2] * S[6 + j];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double k = (V[3 * i] * C[j] + V[3 * i + 1] * C[3 + j]) + V[3 * i + 2] * C[6 + j];
      out[3 * i + j] = (float)V[3 * i + j];
      out[9 + 3 * i + j] = (float)k;
    }
}
