// Host program over eogs2_amd/csrc/draw_rng.h (the text the kernel of csrc/draw.hip compiles): the Random123 known-answer
// vectors of philox4x32-10, the two maps from words to numbers at their edges, the statistics of the clipped normals over
// 65 536 consecutive iterations of one seed, and a printed sample that tests/test_draw_rng_host.py and tests/test_draw_api.py
// compare with the Python restatement. Built with the host compiler alone (and its sanitizers): no HIP header.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "draw_rng.h"

static int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      failures++;                             \
      std::printf("FAILED %s: ", #cond);      \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
    }                                         \
  } while (0)

static uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

static void known_answers() {
  struct Kat { uint32_t c[4], k[2], out[4]; };
  const Kat kats[3] = {
      {{0u, 0u, 0u, 0u}, {0u, 0u}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
      {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
      {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
  };
  for (int i = 0; i < 3; i++) {
    const Kat& t = kats[i];
    const DrawBlock b = philox4x32_10(t.c[0], t.c[1], t.c[2], t.c[3], t.k[0], t.k[1]);
    for (int j = 0; j < 4; j++) CHECK(b.w[j] == t.out[j], "vector %d word %d: %08x, expected %08x", i, j, b.w[j], t.out[j]);
  }
  // the counter's layout: seed 0, iteration 0, slot 0, purpose 0 is the all-zero vector; each field lands in its own word
  const DrawBlock z = draw_block(0u, 0u, 0u, DRAW_PURPOSE_BG);
  CHECK(z.w[0] == 0x6627e8d5u && z.w[3] == 0x9b00dbd8u, "draw_block(0, 0, 0, 0) is not the all-zero vector");
  const DrawBlock f = draw_block(~0ull, ~0ull, ~0u, ~0u);
  CHECK(f.w[0] == 0x408f276du && f.w[3] == 0x6d5451fdu, "draw_block of all ones is not the all-ones vector");
  const DrawBlock p = draw_block(0x299f31d0a4093822ull, 0x85a308d3243f6a88ull, 0x13198a2eu, 0x03707344u);
  CHECK(p.w[0] == 0xd16cfe09u && p.w[1] == 0x94fdccebu && p.w[2] == 0x5001e420u && p.w[3] == 0x24126ea1u, "draw_block's field order");
}

static void edges() {
  CHECK(draw_uniform(0u) == 0.0f, "uniform(0) = %g", draw_uniform(0u));
  CHECK(draw_uniform(0xffu) == 0.0f, "the low 8 bits take no part");
  const float top = draw_uniform(0xffffffffu);
  CHECK(top < 1.0f && top == 1.0f - 5.9604644775390625e-8f, "uniform(0xffffffff) = %.9g", top);
  CHECK(draw_uniform(0x80000000u) == 0.5f, "uniform(0x80000000) = %g", draw_uniform(0x80000000u));
  const uint32_t words[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu, 0x3fffffffu, 0x40000000u, 0xc0000000u};
  for (uint32_t w0 : words) {
    const double u1 = ((double)w0 + 0.5) * 2.3283064365386962890625e-10;
    CHECK(u1 > 0.0 && u1 < 1.0, "u1 of %08x is %g", w0, u1);
    for (uint32_t w1 : words) {
      float z[2];
      draw_normals(w0, w1, z);
      CHECK(std::isfinite(z[0]) && std::isfinite(z[1]), "normals of %08x %08x are not finite", w0, w1);
      CHECK(std::fabs(z[0]) <= 1.0f && std::fabs(z[1]) <= 1.0f, "|z| > 1 at %08x %08x", w0, w1);
    }
  }
  float z[2];
  draw_normals(0u, 0u, z);  // the largest radius there is: clamped
  CHECK(z[0] == 1.0f, "z0 at u1 -> 0 is %g", z[0]);
}

// Over N = 65 536 consecutive iterations of one seed, per component: the share at +-1 is P(|z| >= 1) = 0.3173 within
// 5 sigma, sigma = sqrt(p (1 - p) / N) = 0.0018; the share of positive values is 0.5 within 5 sigma = 0.0098.
static void statistics(uint64_t seed) {
  const int N = 65536;
  for (int comp = 0; comp < 2; comp++) {
    int clipped = 0, positive = 0;
    for (int it = 0; it < N; it++) {
      const DrawBlock b = draw_block(seed, (uint64_t)it, 0u, DRAW_PURPOSE_SHEAR);
      float z[2];
      draw_normals(b.w[0], b.w[1], z);
      CHECK(std::fabs(z[comp]) <= 1.0f, "|z| > 1 at iteration %d", it);
      clipped += std::fabs(z[comp]) == 1.0f;
      positive += z[comp] > 0.0f;
    }
    const double share = (double)clipped / N, pos = (double)positive / N;
    std::printf("STAT seed %" PRIu64 " component %d clipped %.6f positive %.6f\n", seed, comp, share, pos);
    CHECK(std::fabs(share - 0.3173) <= 0.0091, "share at +-1 of component %d: %.6f", comp, share);
    CHECK(std::fabs(pos - 0.5) <= 0.0098, "share of positive values of component %d: %.6f", comp, pos);
  }
  double mean = 0.0;  // the background's uniforms over the same iterations: mean 1/2 within 5 sigma, sigma = 1 / sqrt(12 N)
  for (int it = 0; it < N; it++) {
    const DrawBlock b = draw_block(seed, (uint64_t)it, 0u, DRAW_PURPOSE_BG);
    for (int k = 0; k < 3; k++) {
      const float u = draw_uniform(b.w[k]);
      CHECK(u >= 0.0f && u < 1.0f, "a uniform outside [0, 1) at iteration %d", it);
      mean += u;
    }
  }
  mean /= 3.0 * N;
  CHECK(std::fabs(mean - 0.5) <= 5.0 / std::sqrt(12.0 * 3.0 * N), "mean of the uniforms: %.6f", mean);
}

// SAMPLE seed iteration slot | the background block's words | the uniforms' bits | the shear block's w0 w1 | the normals' bits
static void sample() {
  const uint64_t seeds[] = {0ull, 1ull, 0x0123456789abcdefull, ~0ull};
  const uint64_t iterations[] = {0ull, 1ull, 0xffffffffull, 0x100000000ull, 0x7fffffffffffffffull, 12345ull};
  const uint32_t slots[] = {0u, 1u, 7u};
  for (uint64_t s : seeds)
    for (uint64_t it : iterations)
      for (uint32_t slot : slots) {
        const DrawBlock b = draw_block(s, it, slot, DRAW_PURPOSE_BG), c = draw_block(s, it, slot, DRAW_PURPOSE_SHEAR);
        float z[2];
        draw_normals(c.w[0], c.w[1], z);
        std::printf("SAMPLE %" PRIu64 " %" PRIu64 " %u %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", s, it, slot, b.w[0], b.w[1],
                    b.w[2], b.w[3], bits(draw_uniform(b.w[0])), bits(draw_uniform(b.w[1])), bits(draw_uniform(b.w[2])), c.w[0], c.w[1],
                    bits(z[0]), bits(z[1]));
      }
}

int main() {
  known_answers();
  edges();
  statistics(2024ull);
  sample();
  if (failures) {
    std::printf("%d CHECKS FAILED\n", failures);
    return 1;
  }
  std::printf("ALL CHECKS PASSED\n");
  return 0;
}
