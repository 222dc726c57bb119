// views.hip — the device-side view bank (include/eogs_views.h): the current view's rows into the working tensors of a
// recorded step, the updated working tensors back into its rows, the cursor on. Copies and nothing else: no arithmetic,
// every word moves as an integer, so a NaN keeps its payload. A workgroup finds its slot and its bytes from the plan in the
// kernel arguments (views_plan.h); the ground truth — 12 MB at 3 x 1024^2 — moves as 16-byte accesses, four per thread
// and all loaded before the first is stored; the handful of 3..12-element camera tensors take the dword path of the same launch.
#include "api_util.h"
#include "eogs_views.h"
#include "views_plan.h"

namespace {

constexpr int VEC_PER_THREAD = VIEWS_WG_BYTES / (BLK * 16);  // 4
constexpr int DW_PER_THREAD = VIEWS_WG_BYTES / (BLK * 4);    // 16
static_assert(VEC_PER_THREAD * BLK * 16 == (int)VIEWS_WG_BYTES && DW_PER_THREAD % 4 == 0, "a chunk is whole passes of the workgroup");

// order[cursor mod order_len] when it names a view, else -1 (never an index)
__device__ __forceinline__ int scheduled_view(const eogs_views_schedule& S) {
  const int64_t c = *S.cursor;
  int64_t k;
  if ((((uint64_t)c | (uint64_t)S.order_len) >> 32) == 0) {
    // (wave-uniform) every cursor of a real run: a 32-bit remainder. The 64-bit one is a 64-trip loop of 64-bit VALU work,
    // and every wave of the launch runs it before its first load: it cost the load of a 12 MB image twice the copy itself
    k = (int64_t)((uint32_t)c % (uint32_t)S.order_len);
  } else {
    k = c % S.order_len;
    if (k < 0) k += S.order_len;
  }
  const int32_t v = S.order[k];
  return (v >= 0 && v < S.n_views) ? v : -1;
}

// Keeps the scheduler from sinking a pass's loads between its stores (it otherwise pairs each load with its store and
// waits for every one: one access in flight per thread instead of four). Emits no instruction. It holds only for pointers
// the compiler may think aliased: copy_chunk's are deliberately not __restrict__.
#define LOADS_BEFORE_STORES() asm volatile("" ::: "memory")

// `bytes` (> 0, a multiple of 4) of src -> dst, both at least 4-byte aligned; vec: both 16-byte aligned. Every load of a pass
// is issued before its first store: a load past the chunk's end reads the chunk's last element instead (a branch per access
// would have the compiler wait for each load before the next), and only the stores are guarded.
__device__ __forceinline__ void copy_chunk(const char* src, char* dst, uint32_t bytes, bool vec) {
  if (vec && bytes >= 16u) {
    const uint32_t nvec = bytes >> 4;
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
    uint4 r[VEC_PER_THREAD];
    if (bytes == VIEWS_WG_BYTES) {  // (wave-uniform) every chunk of an image but its last
#pragma unroll
      for (int k = 0; k < VEC_PER_THREAD; k++) r[k] = s[(uint32_t)k * BLK + threadIdx.x];
      LOADS_BEFORE_STORES();
#pragma unroll
      for (int k = 0; k < VEC_PER_THREAD; k++) d[(uint32_t)k * BLK + threadIdx.x] = r[k];
      return;
    }
#pragma unroll
    for (int k = 0; k < VEC_PER_THREAD; k++) r[k] = s[min((uint32_t)k * BLK + threadIdx.x, nvec - 1u)];
    LOADS_BEFORE_STORES();
#pragma unroll
    for (int k = 0; k < VEC_PER_THREAD; k++) {
      const uint32_t i = (uint32_t)k * BLK + threadIdx.x;
      if (i < nvec) d[i] = r[k];
    }
    const uint32_t tail = (bytes >> 2) - (nvec << 2);  // 0 .. 3 dwords behind the last whole 16 bytes
    if (threadIdx.x < tail) {
      const uint32_t i = (nvec << 2) + threadIdx.x;
      reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(src)[i];
    }
  } else {
    const uint32_t ndw = bytes >> 2;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int k0 = 0; k0 < DW_PER_THREAD; k0 += 4) {
      if ((uint32_t)k0 * BLK >= ndw) break;
      uint32_t r[4];
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] = s[min((uint32_t)(k0 + k) * BLK + threadIdx.x, ndw - 1u)];
      LOADS_BEFORE_STORES();
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t i = (uint32_t)(k0 + k) * BLK + threadIdx.x;
        if (i < ndw) d[i] = r[k];
      }
    }
  }
}

// grid: max(1, chunks). Every workgroup reads the cursor, none writes it; workgroup 0 leaves `current`, nobody reads it here.
__global__ __launch_bounds__(BLK) void views_load_kernel(ViewsPlan plan, eogs_views_schedule S) {
  const int v = scheduled_view(S);
  if (blockIdx.x == 0 && threadIdx.x == 0) *S.current = v;
  if (v < 0) return;
  const ViewsChunk c = views_plan_chunk(plan, blockIdx.x);
  if (c.slot < 0) return;
  const eogs_views_slot T = plan.slot[c.slot];
  copy_chunk((const char*)T.table + (size_t)v * T.row_stride + c.offset, (char*)T.working + c.offset, c.bytes, c.vec != 0);
}

// grid: chunks (>= 1). Reads `current` as the load left it; writes rows only.
__global__ __launch_bounds__(BLK) void views_store_kernel(ViewsPlan plan, eogs_views_schedule S, const uint32_t* __restrict__ gate) {
  if (gate != nullptr && gate[0] == 0u) return;
  const int32_t v = *S.current;
  if (v < 0 || v >= S.n_views) return;
  const ViewsChunk c = views_plan_chunk(plan, blockIdx.x);
  if (c.slot < 0) return;
  const eogs_views_slot T = plan.slot[c.slot];
  copy_chunk((const char*)T.working + c.offset, (char*)T.table + (size_t)v * T.row_stride + c.offset, c.bytes, c.vec != 0);
}

__global__ void views_advance_kernel(eogs_views_schedule S, const uint32_t* __restrict__ gate) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (gate != nullptr && gate[0] == 0u) return;
  if (scheduled_view(S) < 0) return;
  *S.cursor = *S.cursor + 1;
}

int check_schedule(const eogs_views_schedule* sch, const char* who) {
  if (!sch) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL schedule", who);
  if (!sch->order || !sch->cursor || !sch->current) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL schedule member", who);
  if (sch->order_len < 1 || sch->n_views < 1) return fail(EOGS_ERR_INVALID_ARG, "%s: order_len and n_views must be positive", who);
  if (((uintptr_t)sch->order | (uintptr_t)sch->current) & 3u || ((uintptr_t)sch->cursor & 7u))
    return fail(EOGS_ERR_INVALID_ARG, "%s: schedule members not aligned", who);
  return EOGS_OK;
}

// the slots of `slots` that carry `flag` and have bytes to move, as the plan of one launch
int make_plan(int n, const eogs_views_slot* slots, const eogs_views_schedule* sch, uint32_t flag, ViewsPlan& plan, const char* who) {
  if (n < 0 || n > EOGS_VIEWS_MAX_SLOTS) return fail(EOGS_ERR_INVALID_ARG, "%s: bad slot count (at most 32 slots in one call)", who);
  int rc = check_schedule(sch, who);
  if (rc) return rc;
  if (n > 0 && !slots) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL slots", who);
  plan.n = 0;
  for (int i = 0; i < EOGS_VIEWS_MAX_SLOTS; i++) plan.slot[i] = eogs_views_slot{nullptr, nullptr, 0, 0, 0u};
  for (int i = 0; i < n; i++) {
    const eogs_views_slot& t = slots[i];
    if (t.flags == 0u || (t.flags & ~(EOGS_VIEWS_LOAD | EOGS_VIEWS_STORE))) return fail(EOGS_ERR_INVALID_ARG, "%s: a slot's flags must be LOAD, STORE or both", who);
    if (t.row_bytes & 3u) return fail(EOGS_ERR_INVALID_ARG, "%s: row_bytes must be a multiple of 4", who);
    if ((t.row_stride & 15u) || t.row_stride < t.row_bytes) return fail(EOGS_ERR_INVALID_ARG, "%s: row_stride must be a multiple of 16 and at least row_bytes", who);
    if (t.row_bytes == 0) continue;
    if (!t.table || !t.working) return fail(EOGS_ERR_INVALID_ARG, "%s: a slot without its table or its working tensor", who);
    if (((uintptr_t)t.table | (uintptr_t)t.working) & 3u) return fail(EOGS_ERR_INVALID_ARG, "%s: table or working tensor not 4-byte aligned", who);
    if (t.flags & flag) plan.slot[plan.n++] = t;
  }
  if (!views_plan_prefix(plan)) return fail(EOGS_ERR_OVERFLOW, "%s: too many bytes for one launch", who);
  return EOGS_OK;
}

}  // namespace

extern "C" {

int eogs_views_wg_bytes(size_t* bytes) {
  clear_error();
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "views_wg_bytes: NULL argument");
  *bytes = VIEWS_WG_BYTES;
  return EOGS_OK;
}

int eogs_views_load(int n, const eogs_views_slot* slots, const eogs_views_schedule* schedule, void* stream) {
  clear_error();
  ViewsPlan plan;
  int rc = make_plan(n, slots, schedule, EOGS_VIEWS_LOAD, plan, "views_load");
  if (rc) return rc;
  if (n == 0) return EOGS_OK;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t chunks = plan.first[plan.n];
  hipLaunchKernelGGL(views_load_kernel, dim3(chunks ? chunks : 1u), dim3(BLK), 0, s, plan, *schedule);
  LAUNCH_TRY(s, false, "views_load");
  return EOGS_OK;
}

int eogs_views_store(int n, const eogs_views_slot* slots, const eogs_views_schedule* schedule, const uint32_t* gate, void* stream) {
  clear_error();
  ViewsPlan plan;
  int rc = make_plan(n, slots, schedule, EOGS_VIEWS_STORE, plan, "views_store");
  if (rc) return rc;
  if ((uintptr_t)gate & 3u) return fail(EOGS_ERR_INVALID_ARG, "views_store: gate not 4-byte aligned");
  const uint32_t chunks = plan.first[plan.n];
  if (n == 0 || chunks == 0) return EOGS_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(views_store_kernel, dim3(chunks), dim3(BLK), 0, s, plan, *schedule, gate);
  LAUNCH_TRY(s, false, "views_store");
  return EOGS_OK;
}

int eogs_views_advance(const eogs_views_schedule* schedule, const uint32_t* gate, void* stream) {
  clear_error();
  int rc = check_schedule(schedule, "views_advance");
  if (rc) return rc;
  if ((uintptr_t)gate & 3u) return fail(EOGS_ERR_INVALID_ARG, "views_advance: gate not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(views_advance_kernel, dim3(1), dim3(64), 0, s, *schedule, gate);
  LAUNCH_TRY(s, false, "views_advance");
  return EOGS_OK;
}

}  // extern "C"
