// flow_taps.h — where a pixel of the flow warp samples, one axis at a time (flow.hip; tests/flow_taps_host.cpp builds it
// with a host compiler). Reference: flowmatching/flow_matching.py:225-253, grid + flow through
// grid_sample(bilinear, padding_mode="border", align_corners=True): the sample position p + f in PIXELS is clamped to
// [0, n - 1], its floor is the first tap, the next pixel the second (weight = the fractional part).
// The indices are in [0, n - 1] for EVERY bit pattern of f: the clamp runs in float with NaN-dropping min / max (fmaxf and
// fminf return the operand that is a number, so NaN becomes 0), the conversion sees a value in [0, n - 1], and the integers
// are clamped once more. At the far border both taps name pixel n - 1 and the second one weighs 0.
#ifndef EOGS_FLOW_TAPS_H_INCLUDED
#define EOGS_FLOW_TAPS_H_INCLUDED

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EOGS_FLOW_HD __host__ __device__
#else
#define EOGS_FLOW_HD
#endif

struct FlowAxisTap {
  int i0, i1;  // first and second tap, both in [0, n - 1]
  float w1;    // weight of the second tap, in [0, 1); the first weighs 1 - w1
};

EOGS_FLOW_HD inline FlowAxisTap flow_axis_tap(int p, float f, int n) {
  float s = (float)p + f;
  s = fminf(fmaxf(s, 0.f), (float)(n - 1));
  const float fl = floorf(s);
  FlowAxisTap t;
  t.w1 = s - fl;
  int i = (int)fl;
  i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  t.i0 = i;
  t.i1 = i + 1 < n ? i + 1 : n - 1;
  return t;
}

// Weight with which output pixel p of an axis reads input pixel i (the adjoint's view of the same taps).
EOGS_FLOW_HD inline float flow_axis_weight(int p, float f, int n, int i) {
  const FlowAxisTap t = flow_axis_tap(p, f, n);
  return (t.i0 == i ? 1.f - t.w1 : 0.f) + (t.i1 == i ? t.w1 : 0.f);
}

// Constant displacement d: the outputs p whose taps can name input pixel i form one run [a, b] (p + d is monotone in p).
// Inside the image |p + d - i| < 1, a window of five around i - d that absorbs every rounding of the two float sums; pixel 0
// also takes every output clamped onto it from the left (p + d <= 0), pixel n - 1 those from the right. The run may hold
// outputs that weigh 0: the caller asks flow_axis_weight for each. An empty run has b < a.
EOGS_FLOW_HD inline void flow_axis_run(int i, float d, int n, int* a, int* b) {
  if (d != d) {  // NaN: every position clamps to 0 (flow_axis_tap), so pixel 0 takes all outputs and the others none
    *a = 0;
    *b = i == 0 ? n - 1 : -1;
    return;
  }
  float c = (float)i - d;
  c = fminf(fmaxf(c, -2.f), (float)n + 1.f);
  const int m = (int)floorf(c);
  int lo = m - 2, hi = m + 2;
  if (i == 0) lo = 0;
  if (i == n - 1) hi = n - 1;
  *a = lo < 0 ? 0 : lo;
  *b = hi > n - 1 ? n - 1 : hi;
}

#endif /* EOGS_FLOW_TAPS_H_INCLUDED */
