// draw_rng.h — the stream behind the per-iteration random draws (include/eogs_draw.h): Philox4x32-10 as a pure function of
// (seed, iteration, camera slot, purpose), and the two maps from its words to the numbers an iteration uses. One text for
// the kernel, for the host program that checks the known answers (tests/draw_rng_host.cpp) and, restated in Python
// integers, for eogs2_amd.draw.draws_for. Plain C++ over uint32_t / uint64_t: no signed arithmetic, no HIP header.
//
//   key     = (seed low word, seed high word)
//   counter = (iteration low word, iteration high word, camera slot, purpose)
//
// so seed 0, iteration 0, slot 0, purpose 0 is the all-zero known-answer vector of Random123.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRAW_HD __host__ __device__
#else
#define DRAW_HD
#endif

constexpr uint32_t DRAW_PURPOSE_BG = 0u;     // words 0, 1, 2: the background's three uniforms
constexpr uint32_t DRAW_PURPOSE_SHEAR = 1u;  // words 0, 1: one Box-Muller pair, the virtual camera's shear

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;  // the round's multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;  // the key's Weyl increments

struct DrawBlock {
  uint32_t w[4];
};

DRAW_HD inline DrawBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; round++) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += PHILOX_W0;  // (unsigned: wraps)
    k1 += PHILOX_W1;
  }
  DrawBlock b;
  b.w[0] = c0; b.w[1] = c1; b.w[2] = c2; b.w[3] = c3;
  return b;
}

DRAW_HD inline DrawBlock draw_block(uint64_t seed, uint64_t iteration, uint32_t slot, uint32_t purpose) {
  return philox4x32_10((uint32_t)iteration, (uint32_t)(iteration >> 32), slot, purpose, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// (w >> 8) * 2^-24: 24 bits, exact in fp32, in [0, 1), the same bits wherever it is computed
DRAW_HD inline float draw_uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }

// One Box-Muller pair in double from two words, each rounded to float and clamped to [-1, 1]: `randn(2).clip(-1, 1)`.
// u1 = (w0 + 0.5) * 2^-32 lies in (0, 1): the logarithm is finite.
DRAW_HD inline void draw_normals(uint32_t w0, uint32_t w1, float z[2]) {
  const double u1 = ((double)w0 + 0.5) * 2.3283064365386962890625e-10;
  const double u2 = ((double)w1 + 0.5) * 2.3283064365386962890625e-10;
  const double r = sqrt(-2.0 * log(u1));
  const double a = 6.283185307179586476925286766559 * u2;
  const float z0 = (float)(r * cos(a)), z1 = (float)(r * sin(a));
  z[0] = fminf(fmaxf(z0, -1.0f), 1.0f);
  z[1] = fminf(fmaxf(z1, -1.0f), 1.0f);
}
