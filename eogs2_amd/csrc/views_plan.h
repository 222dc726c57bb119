// views_plan.h — the slot plan of the view bank (include/eogs_views.h): which bytes of which slot a workgroup of
// eogs_views_load / eogs_views_store moves, and whether as 16-byte accesses or as dwords. One function for the kernels and
// for the host program that walks every chunk of every plan (tests/views_plan_host.cpp): plain C++, no device code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "eogs_views.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIEWS_HD __host__ __device__
#else
#define VIEWS_HD
#endif

// Bytes one workgroup moves: 256 threads x 4 accesses of 16 bytes, every load issued before the first store, so a
// workgroup has 16 KiB in flight and a 12 MB ground truth is 768 workgroups.
constexpr uint32_t VIEWS_WG_BYTES = 16384;

// What the kernel gets by value: the slots of one launch and, per slot, the index of its first chunk. first[n] is the
// number of chunks, i.e. of workgroups. A slot of zero bytes has no chunk: first[i + 1] == first[i].
struct ViewsPlan {
  eogs_views_slot slot[EOGS_VIEWS_MAX_SLOTS];
  uint32_t first[EOGS_VIEWS_MAX_SLOTS + 1];
  int n;
};

struct ViewsChunk {
  int slot;         // index into plan.slot, -1: no such chunk
  size_t offset;    // byte offset inside the row and inside the working tensor
  uint32_t bytes;   // 4 .. VIEWS_WG_BYTES, a multiple of 4
  int vec;          // 1: 16-byte accesses (a tail of 4, 8 or 12 bytes goes as dwords), 0: dwords
};

// Fills plan.first from plan.slot[0 .. n): false when the chunks do not fit a launch's 2^31 - 1 workgroups.
inline bool views_plan_prefix(ViewsPlan& plan) {
  uint64_t total = 0;
  plan.first[0] = 0;
  for (int i = 0; i < EOGS_VIEWS_MAX_SLOTS; i++) {
    if (i < plan.n) total += ((uint64_t)plan.slot[i].row_bytes + VIEWS_WG_BYTES - 1) / VIEWS_WG_BYTES;
    if (total > 0x7FFFFFFFull) return false;
    plan.first[i + 1] = (uint32_t)total;
  }
  return true;
}

// Chunk `chunk` of the plan. Chunks of a slot are consecutive, in byte order, all VIEWS_WG_BYTES long but the last.
VIEWS_HD inline ViewsChunk views_plan_chunk(const ViewsPlan& plan, uint32_t chunk) {
  ViewsChunk c;
  c.slot = -1; c.offset = 0; c.bytes = 0; c.vec = 0;
  if (plan.n < 1 || plan.n > EOGS_VIEWS_MAX_SLOTS || chunk >= plan.first[plan.n]) return c;
  // first[] never decreases, so the slot is the number of later slots that start at or before the chunk (empty slots are
  // stepped over). Unrolled over fixed offsets on purpose: the table sits in the kernel arguments, and a search whose every
  // step waits for the previous step's load pays the argument memory's latency once per step.
  int s = 0;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
  for (int i = 1; i < EOGS_VIEWS_MAX_SLOTS; i++) s += (i < plan.n && plan.first[i] <= chunk) ? 1 : 0;
  const eogs_views_slot& S = plan.slot[s];
  c.slot = s;
  c.offset = (size_t)(chunk - plan.first[s]) * VIEWS_WG_BYTES;
  const size_t left = S.row_bytes - c.offset;
  c.bytes = left < VIEWS_WG_BYTES ? (uint32_t)left : VIEWS_WG_BYTES;
  // every row starts 16-byte aligned when the table does and the stride is a multiple of 16
  c.vec = (((uintptr_t)S.table | (uintptr_t)S.working | (uintptr_t)S.row_stride | (uintptr_t)c.offset) & 15u) == 0;
  return c;
}
