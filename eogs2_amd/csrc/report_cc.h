// report_cc.h — a camera's colour correction recomposed against the reference camera's (include/eogs_report.h): one text
// for the kernel of csrc/report.hip and for the host program that checks it against numpy (tests/report_cc_host.cpp).
// Plain C++ over float and double: no HIP header, no library call. The library is built with -ffp-contract=off, and so is
// the host program: every product and sum below is rounded on its own.
//
//   Ai' = Ai . A1^-1        bi' = bi - Ai' . b1        (utils/save_utils.py:26-33: Ai @ A1inv, -(Ai @ A1inv @ b1) + bi)
//
// all in double over the fp32 inputs; A1^-1 = adj(A1) / det(A1). Each of the 12 results is rounded to fp32 once.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define REPORT_CC_HD __host__ __device__
#else
#define REPORT_CC_HD
#endif

// Ai, A1: row-major 3 x 3. det(A1) zero or not finite: NaN in all 12.
REPORT_CC_HD inline void report_recompose(const float Ai[9], const float bi[3], const float A1[9], const float b1[3], float outA[9],
                                          float outb[3]) {
  double A[9], C[9];
  for (int i = 0; i < 9; i++) {
    A[i] = (double)Ai[i];
    C[i] = (double)A1[i];
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
    for (int i = 0; i < 9; i++) outA[i] = nan;
    for (int i = 0; i < 3; i++) outb[i] = nan;
    return;
  }
  double inv[9], R[9];
  for (int i = 0; i < 9; i++) inv[i] = adj[i] / det;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = (A[3 * i] * inv[j] + A[3 * i + 1] * inv[3 + j]) + A[3 * i + 2] * inv[6 + j];
  for (int i = 0; i < 3; i++) {
    const double t = (R[3 * i] * (double)b1[0] + R[3 * i + 1] * (double)b1[1]) + R[3 * i + 2] * (double)b1[2];
    outb[i] = (float)((double)bi[i] - t);
    for (int j = 0; j < 3; j++) outA[3 * i + j] = (float)R[3 * i + j];
  }
}
