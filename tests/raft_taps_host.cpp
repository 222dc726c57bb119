// Host harness of eogs2_amd/csrc/raft_taps.h (built with g++ by tests/test_raft_taps_host.py): for every kind of coordinate
// the clamped floor stays inside the range the window arithmetic is safe in, the weight is finite and in [0, 1], and every
// tap is either inside the level or has the verdict "outside"; what is not a finite in-range coordinate has ALL taps outside
// and weight 0 (the kernel then writes exact zeros); finite coordinates agree with the float64 statement.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "raft_taps.h"

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
  const int sizes[] = {1, 2, 3, 17, 128, 256, 65536, 1 << 24};
  long n_odd = 0;
  for (int n : sizes)
    for (int r = 1; r <= EOGS_RAFT_TAPS_MAX_RADIUS; r++)
      for (int l = 0; l < EOGS_RAFT_TAPS_MAX_LEVELS; l++)
        for (float c : odd) {
          const RaftAxisTap t = raft_axis_tap(c, l, n, r);
          CHECK(t.f >= -(r + 2) && t.f <= n + r + 1, "floor out of range: n %d r %d l %d c %g -> %d", n, r, l, c, t.f);
          CHECK(std::isfinite(t.w) && t.w >= 0.f && t.w <= 1.f, "weight: n %d r %d l %d c %g -> %g", n, r, l, c, t.w);
          int inside = 0;
          for (int k = 0; k <= 2 * r + 1; k++) {
            const int p = raft_tap_pos(t.f, r, k);
            const bool in = raft_tap_inside(p, n);
            CHECK(in == (p >= 0 && p < n), "verdict: n %d pos %d", n, p);
            inside += in;
          }
          const double s = (double)c * std::ldexp(1.0, -l);
          const bool tame = std::isfinite(c) && std::floor(s) >= -(double)(r + 2) && std::floor(s) <= (double)(n + r + 1);
          if (!tame) {
            CHECK(inside == 0, "a wild coordinate reads the level: n %d r %d l %d c %g -> floor %d", n, r, l, c, t.f);
            CHECK(t.w == 0.f, "a wild coordinate has a weight: n %d r %d l %d c %g -> %g", n, r, l, c, t.w);
          }
          if (t.f == -(r + 2) || t.f == n + r + 1) CHECK(inside == 0, "the ends of the range must lie outside: n %d r %d f %d", n, r, t.f);
          n_odd++;
        }
  // finite coordinates against the float64 statement: s = c 2^-l exact, f = floor(s), w = s - f
  long n_fin = 0;
  unsigned rnd = 12345u;
  for (int n : {2, 16, 19, 128, 256})
    for (int l = 0; l < EOGS_RAFT_TAPS_MAX_LEVELS; l++)
      for (int k = 0; k < 20000; k++) {
        rnd = rnd * 1664525u + 1013904223u;
        const float scale = (k % 4 == 0) ? 3.f * n * (1 << l) : (k % 4 == 1 ? 40.f : 3.f);
        float c = ((float)(rnd >> 8) / 16777216.f - 0.3f) * scale;
        if (k % 7 == 0) c = roundf(c);
        if (k % 11 == 0) c = roundf(c * 8.f) / 8.f;
        const int r = 1 + (k % 4);
        const RaftAxisTap t = raft_axis_tap(c, l, n, r);
        const double s = (double)c * std::ldexp(1.0, -l), f = std::floor(s);
        if (f >= -(double)(r + 2) && f <= (double)(n + r + 1)) {
          CHECK((double)t.f == f, "floor: n %d l %d c %.9g -> %d, statement %.17g", n, l, c, t.f, f);
          // s - f is exact in float wherever |s| >= 2^-24 |f|-ish; a tiny negative s rounds to weight 1: half an ulp of 1
          CHECK(std::fabs((double)t.w - (s - f)) <= 6e-8, "weight: n %d l %d c %.9g -> %.9g, statement %.17g", n, l, c, t.w, s - f);
        } else {
          CHECK(t.w == 0.f && (t.f == -(r + 2) || t.f == n + r + 1), "clamp: n %d l %d c %.9g -> %d %g", n, l, c, t.f, t.w);
        }
        n_fin++;
      }
  // the channel order: the x offset is the slow index
  CHECK(raft_tap_channel(0, 1, 7) == 1 && raft_tap_channel(1, 0, 7) == 7 && raft_tap_channel(6, 6, 7) == 48, "channel order");
  CHECK(EOGS_RAFT_X_OFFSET_IS_SLOW == 1, "channel order constant");
  printf("checked %ld odd, %ld finite\n", n_odd, n_fin);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL CHECKS PASSED\n");
  return 0;
}
