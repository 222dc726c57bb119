// api_util.h — what every extern "C" entry needs on the host: the thread's error message, launch checks and the profile
// brackets. The state behind them (the thread_local message, the profile mutex, sums and event pool) is defined once, in
// api.hip; the entries themselves live beside their kernels (api.hip: eogs_rast_*, a side module's in its own .hip).
#pragma once
#include "common.h"

#pragma GCC visibility push(hidden)  // shared inside the library, no part of its surface

// formats the calling thread's message (eogs_rast_last_error) and returns `code`
int fail(int code, const char* fmt, const char* detail = "");
void clear_error();  // an entry that reports through the message empties it first

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) return fail(EOGS_ERR_DEVICE, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

// after a group of launches: always catch launch errors; in debug mode also synchronise (auxiliary.h:178-185)
int check_launch(hipStream_t s, bool debug, const char* what);

#define LAUNCH_TRY(s, dbg, what)              \
  do {                                        \
    int rc_ = check_launch((s), (dbg), what); \
    if (rc_ != EOGS_OK) return rc_;           \
  } while (0)

// the grid of a grid-stride launch: one thread per item (an element, or a unit of four where the kernel counts in those),
// at least one workgroup and at most `cap`
inline int capped_blocks(int64_t items, int threads, int cap) {
  const int64_t b = (items + threads - 1) / threads;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- optional per-kernel-group timing with hipEvents on the launch stream ----
// (the order is the ABI of eogs_rast_profile_get: slots are read by index; their names are api.hip's kSlotNames)
enum { PS_PREPROCESS, PS_DEPTH_SORT, PS_BINNING, PS_RENDER_FWD, PS_RENDER_BWD, PS_GAUSS_BWD, PS_LOSS_FWD, PS_LOSS_BWD, PS_ADAM,
       PS_COMPACT, PS_RESAMPLE_FWD, PS_RESAMPLE_BWD, PS_KNN, PS_SHADE_FWD, PS_SHADE_BWD, PS_MLOSS_FWD, PS_MLOSS_BWD, PS_TSDF,
       PS_TSDF_NORMALS, PS_TSDF_PRIOR, PS_TSDF_SURFACE, PS_DSM_DOWNSAMPLE, PS_DSM_PIVOTS, PS_DSM_MOMENTS, PS_DSM_FINALIZE,
       PS_DSM_APPLY, PS_DSM_MAE, PS_FLOW_FWD, PS_FLOW_BWD, PS_FLOW_STATS, PS_REG_FWD, PS_REG_BWD, PS_COUNT };
static_assert(PS_COUNT <= 32, "eogs_rast_profile_select takes a 32-bit slot mask");

// brackets the launches of its scope with two events on `st` when the slot is being profiled
struct ProfScope {
  hipStream_t s; int slot; bool on = false; hipEvent_t a{}, b{};
  ProfScope(int slot_, hipStream_t st);
  ~ProfScope();
};

#pragma GCC visibility pop
