// raft_taps.h — where a pixel of the correlation lookup samples a pyramid level, one axis at a time (raft.hip;
// tests/raft_taps_host.cpp builds it with a host compiler). Semantics (include/eogs_resample.h, eogs_raft_lookup): s = coord * 2^-level,
// f = floor(s), w = s - f; the window of radius r reads positions f - r ... f + r + 1 and a position outside [0, n) gives 0.
//
// The floor is clamped IN FLOAT to [-(r + 2), n + r + 1] before the conversion to int, so every bit pattern of a
// coordinate yields an int the window arithmetic cannot overflow, and at either end of that range every position of the
// window lies outside: the verdict "all taps outside" stands for everything beyond it. A coordinate that is not inside the
// range (NaN, +-inf, +-1e30) gets the weight 0, so no NaN reaches the blend: such a pixel's output is exactly 0. NaN takes
// the low end (the comparisons are false for it).
#ifndef EOGS_RAFT_TAPS_H_INCLUDED
#define EOGS_RAFT_TAPS_H_INCLUDED

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EOGS_RAFT_HD __host__ __device__
#else
#define EOGS_RAFT_HD
#endif

#define EOGS_RAFT_TAPS_MAX_RADIUS 4
#define EOGS_RAFT_TAPS_MAX_LEVELS 4

// The order of a level's (2r+1)^2 output channels: channel = a * (2r+1) + b with a the x offset and b the y offset, the x
// offset the SLOW index (RAFT stacks meshgrid(d, d, indexing="ij") onto (x, y)). The one place that decides it.
#define EOGS_RAFT_X_OFFSET_IS_SLOW 1

struct RaftAxisTap {
  int f;    // clamped floor, in [-(r + 2), n + r + 1]
  float w;  // weight of the upper neighbour, in [0, 1]; 0 where the floor was clamped
};

// 2^-level, level in [0, 3]: the product with it is exact in float (short of the denormal range)
EOGS_RAFT_HD inline float raft_level_scale(int level) {
  return level <= 0 ? 1.f : (level == 1 ? 0.5f : (level == 2 ? 0.25f : 0.125f));
}

EOGS_RAFT_HD inline RaftAxisTap raft_axis_tap(float coord, int level, int n, int r) {
  const float s = coord * raft_level_scale(level);
  const float fl = floorf(s);
  const float lo = -(float)(r + 2), hi = (float)(n + r + 1);
  const bool in = fl >= lo && fl <= hi;  // false for NaN
  RaftAxisTap t;
  t.w = in ? s - fl : 0.f;
  t.f = (int)(in ? fl : (fl > hi ? hi : lo));
  if (t.f > n + r + 1) t.f = n + r + 1;  // (float)(n + r + 1) may round up where n is near 2^24; there s is an integer, w is 0
  return t;
}

// position of tap k (0 ... 2r + 1) of the window around floor f
EOGS_RAFT_HD inline int raft_tap_pos(int f, int r, int k) { return f - r + k; }

EOGS_RAFT_HD inline bool raft_tap_inside(int pos, int n) { return pos >= 0 && pos < n; }

// output channel of (x offset a, y offset b) inside a level, K = 2r + 1
EOGS_RAFT_HD inline int raft_tap_channel(int a, int b, int K) {
#if EOGS_RAFT_X_OFFSET_IS_SLOW
  return a * K + b;
#else
  return b * K + a;
#endif
}

#endif /* EOGS_RAFT_TAPS_H_INCLUDED */
