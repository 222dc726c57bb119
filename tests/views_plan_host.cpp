// The slot plan of the view bank (eogs2_amd/csrc/views_plan.h) walked on the host: for every payload around the workgroup
// boundaries and for random sets of 1, 2, 31 and 32 slots (a zero-byte slot among them) the chunks partition every slot
// exactly once and in order, no chunk crosses a slot, and the 16-byte path is chosen only when table row, working base and
// offset are all 16-byte aligned. The function is the one the kernels call.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "views_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (failures < 20) {               \
        std::printf("FAILED: %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
      failures++;                        \
    }                                    \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// walks every chunk of the plan; the slots' pointers are never dereferenced
static void walk(ViewsPlan& plan, const char* what) {
  CHECK(views_plan_prefix(plan), "%s", what);
  const uint32_t chunks = plan.first[plan.n];
  std::vector<size_t> covered(plan.n, 0);  // bytes of each slot seen so far: chunks must arrive in order and abut
  int last_slot = -1;
  for (uint32_t c = 0; c < chunks; c++) {
    const ViewsChunk k = views_plan_chunk(plan, c);
    CHECK(k.slot >= 0 && k.slot < plan.n, "%s: chunk %u names slot %d", what, c, k.slot);
    if (k.slot < 0 || k.slot >= plan.n) return;
    const eogs_views_slot& S = plan.slot[k.slot];
    CHECK(k.slot >= last_slot, "%s: chunk %u goes back to slot %d", what, c, k.slot);
    last_slot = k.slot;
    CHECK(k.offset == covered[k.slot], "%s: chunk %u of slot %d starts at %zu, expected %zu", what, c, k.slot, k.offset, covered[k.slot]);
    CHECK(k.bytes >= 4 && k.bytes <= VIEWS_WG_BYTES && k.bytes % 4 == 0, "%s: chunk %u has %u bytes", what, c, k.bytes);
    CHECK(k.offset + k.bytes <= S.row_bytes, "%s: chunk %u crosses the end of slot %d", what, c, k.slot);
    CHECK(k.bytes == VIEWS_WG_BYTES || k.offset + k.bytes == S.row_bytes, "%s: a short chunk %u inside slot %d", what, c, k.slot);
    const bool aligned = ((uintptr_t)S.table % 16 == 0) && (S.row_stride % 16 == 0) && ((uintptr_t)S.working % 16 == 0) && (k.offset % 16 == 0);
    CHECK((k.vec != 0) == aligned, "%s: chunk %u of slot %d: vec %d, aligned %d", what, c, k.slot, k.vec, (int)aligned);
    covered[k.slot] += k.bytes;
  }
  for (int i = 0; i < plan.n; i++)
    CHECK(covered[i] == plan.slot[i].row_bytes, "%s: slot %d: %zu of %zu bytes covered", what, i, covered[i], plan.slot[i].row_bytes);
  // past the end there is no chunk
  CHECK(views_plan_chunk(plan, chunks).slot == -1, "%s: a chunk past the end", what);
  CHECK(views_plan_chunk(plan, 0xFFFFFFFFu).slot == -1, "%s: a chunk at 2^32 - 1", what);
}

static eogs_views_slot slot_of(size_t row_bytes, unsigned table_mis, unsigned working_mis) {
  eogs_views_slot s;
  s.table = (void*)(uintptr_t)(0x10000000u + 4u * table_mis);
  s.working = (void*)(uintptr_t)(0x20000000u + 4u * working_mis);
  s.row_bytes = row_bytes;
  s.row_stride = (row_bytes + 15) / 16 * 16;
  if (s.row_stride == 0) s.row_stride = 16;
  s.flags = EOGS_VIEWS_LOAD;
  return s;
}

int main() {
  // every payload from 4 bytes to 4 (wg/4 + 5) bytes, alone in its plan, with every pair of misalignments
  for (size_t bytes = 4; bytes <= 4 * ((size_t)VIEWS_WG_BYTES / 4 + 5); bytes += 4)
    for (unsigned mis = 0; mis < 16; mis++) {
      ViewsPlan plan;
      plan.n = 1;
      plan.slot[0] = slot_of(bytes, mis & 3, mis >> 2);
      walk(plan, "single payload");
      const uint32_t want = (uint32_t)((bytes + VIEWS_WG_BYTES - 1) / VIEWS_WG_BYTES);
      CHECK(plan.first[1] == want, "single payload of %zu bytes: %u chunks, expected %u", bytes, plan.first[1], want);
    }
  // random sets of slots, one of them empty (not in the one-slot sets, which have their own empty case below)
  const int counts[] = {1, 2, 31, 32};
  for (int rep = 0; rep < 200; rep++)
    for (int n : counts) {
      ViewsPlan plan;
      plan.n = n;
      const int empty = n > 1 ? (int)(rnd() % n) : -1;
      for (int i = 0; i < n; i++) {
        size_t bytes;
        switch (rnd() % 4) {
          case 0: bytes = 4 * (1 + rnd() % 16); break;                                      // a camera's parameters
          case 1: bytes = 4 * (1 + rnd() % (3 * VIEWS_WG_BYTES / 4)); break;                // a few workgroups
          case 2: bytes = VIEWS_WG_BYTES * (1 + rnd() % 4) + 4 * (rnd() % 3) - 4 * (rnd() % 2); break;  // on a boundary
          default: bytes = 4 * (size_t)(3 * 1024 * 1024 / 4 + rnd() % 1000); break;         // an image
        }
        if (i == empty) bytes = 0;
        plan.slot[i] = slot_of(bytes, (rnd() % 2) ? (unsigned)(rnd() % 4) : 0, (rnd() % 2) ? (unsigned)(rnd() % 4) : 0);
      }
      walk(plan, "random set");
    }
  {  // a plan of one empty slot has no chunk; an empty plan neither
    ViewsPlan plan;
    plan.n = 1;
    plan.slot[0] = slot_of(0, 0, 0);
    walk(plan, "one empty slot");
    CHECK(plan.first[1] == 0, "one empty slot: %u chunks", plan.first[1]);
    plan.n = 0;
    CHECK(views_plan_prefix(plan) && plan.first[0] == 0, "empty plan");
    CHECK(views_plan_chunk(plan, 0).slot == -1, "empty plan: chunk 0");
  }
  {  // more chunks than a launch has workgroups: refused
    ViewsPlan plan;
    plan.n = 2;
    plan.slot[0] = slot_of((size_t)0x7FFFFFFFull * VIEWS_WG_BYTES, 0, 0);
    plan.slot[1] = slot_of(4, 0, 0);
    CHECK(!views_plan_prefix(plan), "2^31 chunks accepted");
  }
  if (failures) {
    std::printf("%d CHECKS FAILED\n", failures);
    return 1;
  }
  std::printf("ALL CHECKS PASSED\n");
  return 0;
}
