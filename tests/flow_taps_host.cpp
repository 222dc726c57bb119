// Host harness of eogs2_amd/csrc/flow_taps.h (built with g++ by tests/test_flow_taps_host.py): the tap indices stay inside
// the image and the weights finite for every kind of flow value, the taps agree with the float64 statement for finite flows,
// and the runs of the constant-displacement adjoint cover every output that weighs on a pixel.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "flow_taps.h"

static int g_fail = 0;
#define CHECK(c, ...)                                      \
  do {                                                     \
    if (!(c)) {                                            \
      if (g_fail++ < 20) { printf("FAILED: " __VA_ARGS__); printf("\n"); } \
    }                                                      \
  } while (0)

static float from_bits(unsigned b) { float f; memcpy(&f, &b, 4); return f; }

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> odd = {nan, -nan, from_bits(0x7FA00001u), from_bits(0xFFFFFFFFu), inf, -inf, 1e30f, -1e30f, 3e38f, -3e38f,
                            from_bits(1u), -from_bits(1u), from_bits(0x007FFFFFu), 1e-40f, -1e-40f, 0.f, -0.f, 2147483648.f,
                            -2147483648.f, 4294967296.f, 1e9f, -1e9f, 16777216.f, 0.5f, -0.5f, 1.f, -1.f};
  const int sizes[] = {2, 3, 17, 1024, 65536, 1 << 24};
  long n_odd = 0;
  for (int n : sizes)
    for (float f : odd)
      for (int p : {0, 1, n / 2, n - 2, n - 1}) {
        const FlowAxisTap t = flow_axis_tap(p, f, n);
        CHECK(t.i0 >= 0 && t.i0 < n && t.i1 >= 0 && t.i1 < n, "index out of range: n %d p %d f %g -> %d %d", n, p, f, t.i0, t.i1);
        CHECK(std::isfinite(t.w1) && t.w1 >= 0.f && t.w1 < 1.f, "weight: n %d p %d f %g -> %g", n, p, f, t.w1);
        CHECK(t.i1 == t.i0 + 1 || (t.i1 == t.i0 && t.i0 == n - 1), "second tap: n %d p %d f %g -> %d %d", n, p, f, t.i0, t.i1);
        const float w = flow_axis_weight(p, f, n, t.i0);
        CHECK(std::isfinite(w), "adjoint weight: n %d p %d f %g", n, p, f);
        int a, b;
        flow_axis_run(p, f, n, &a, &b);
        CHECK(a >= 0 && b < n && b - a < n && b >= -1, "run out of range: n %d i %d d %g -> [%d, %d]", n, p, f, a, b);
        n_odd++;
      }
  // finite flows against the float64 statement: clip(p + f, 0, n - 1), floor, fraction
  long n_fin = 0;
  unsigned r = 12345u;
  for (int n : {2, 33, 47, 1024, 4096})
    for (int k = 0; k < 20000; k++) {
      r = r * 1664525u + 1013904223u;
      const int p = (int)((r >> 8) % (unsigned)n);
      r = r * 1664525u + 1013904223u;
      const float scale = (k % 4 == 0) ? 2.f * n : (k % 4 == 1 ? 40.f : 3.f);
      float f = ((float)(r >> 8) / 16777216.f - 0.5f) * scale;
      if (k % 7 == 0) f = roundf(f);
      const FlowAxisTap t = flow_axis_tap(p, f, n);
      const double su = (double)p + (double)f;
      const double s = su < 0 ? 0 : (su > n - 1 ? n - 1 : su);
      // the value the two taps interpolate to for the ramp img[i] = i is the position itself
      const double got = (1.0 - (double)t.w1) * t.i0 + (double)t.w1 * t.i1;
      // one rounding of the float sum p + f: half an ulp, 2^-24 relative
      CHECK(std::fabs(got - s) <= 6e-8 * std::fabs(su), "position: n %d p %d f %.9g -> %.9g, statement %.9g", n, p, f, got, s);
      n_fin++;
    }
  // the runs of the adjoint: every output with a non-zero weight on input i lies inside [a, b]
  long n_run = 0;
  for (int n : {2, 5, 33, 128})
    for (float d : {0.f, 0.37f, -1.62f, 3.f, -4.f, 7.999999f, -70.25f, 200.f, -200.f, 1e30f, -1e30f, nan, inf, -inf, 1e-40f, 127.f, -127.5f})
      for (int i = 0; i < n; i++) {
        int a, b;
        flow_axis_run(i, d, n, &a, &b);
        float inside = 0.f, all = 0.f;
        for (int p = 0; p < n; p++) {
          const float w = flow_axis_weight(p, d, n, i);
          all += w;
          if (p >= a && p <= b) inside += w;
          else CHECK(w == 0.f, "run misses an output: n %d d %g i %d p %d w %g run [%d, %d]", n, d, i, p, w, a, b);
        }
        CHECK(inside == all, "run sum: n %d d %g i %d", n, d, i);
        CHECK((i == 0 || i == n - 1) || b - a <= 4, "interior run longer than five: n %d d %g i %d [%d, %d]", n, d, i, a, b);
        n_run++;
      }
  printf("checked %ld odd, %ld finite, %ld runs\n", n_odd, n_fin, n_run);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL CHECKS PASSED\n");
  return 0;
}
