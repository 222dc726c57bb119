// api.hip — the extern "C" boundary declared in include/eogs_rast.h (device pointers + hipStream_t).
// Orchestration only: argument checks, workspace carving, kernel launches. The library never allocates
// device memory; the only host allocation is a small pinned staging buffer for the num_rendered readback.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "common.h"

namespace {

thread_local char g_err[512] = "";
thread_local uint32_t* g_pinned = nullptr;  // MISC_WORDS u32, pinned host memory (one per calling thread)
// the forward_prepare whose count readback is still pending on this thread (EOGS_FLAG_DEFER_COUNTS)
struct PendingCounts { bool valid; int P, H, W; bool have_scratch; uint32_t sort_cap; hipStream_t side; bool alt; };
thread_local PendingCounts g_pending_counts = {false, 0, 0, 0, false, 0u, nullptr};
// the side stream of a count copy into g_pinned that nobody has waited for yet (a deferred forward whose counts were never
// asked for): the next forward_prepare drains it before it arms g_pinned again, or the old copy would land as the new counts
thread_local hipStream_t g_copy_in_flight = nullptr;
#define MIRROR_PENDING 0xFFFFFFFFu  // sentinel of a count word that has not arrived (never a legitimate high word of a count below 2^31)

// per calling thread and device: a non-blocking side stream + event for the num_rendered readback
struct Side { int dev; hipStream_t stream; hipEvent_t ev; };
thread_local Side g_side[16];
thread_local int g_nside = 0;
Side* side_for_current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  for (int i = 0; i < g_nside; i++)
    if (g_side[i].dev == dev) return &g_side[i];
  if (g_nside == 16) return nullptr;
  Side sd;
  sd.dev = dev;
  if (hipStreamCreateWithFlags(&sd.stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
  if (hipEventCreateWithFlags(&sd.ev, hipEventDisableTiming) != hipSuccess) { (void)hipStreamDestroy(sd.stream); return nullptr; }
  g_side[g_nside] = sd;
  return &g_side[g_nside++];
}

int fail(int code, const char* fmt, const char* detail = "") {
  snprintf(g_err, sizeof g_err, fmt, detail);
  return code;
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) return fail(EOGS_ERR_DEVICE, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

// after a group of launches: always catch launch errors; in debug mode also synchronise (auxiliary.h:178-185)
int check_launch(hipStream_t s, bool debug, const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && debug) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return EOGS_ERR_DEVICE;
  }
  return EOGS_OK;
}
// ---- optional per-kernel-group timing with hipEvents on the launch stream ----
enum { PS_PREPROCESS, PS_DEPTH_SORT, PS_BINNING, PS_RENDER_FWD, PS_RENDER_BWD, PS_GAUSS_BWD, PS_LOSS_FWD, PS_LOSS_BWD, PS_ADAM,
       PS_COMPACT, PS_RESAMPLE_FWD, PS_RESAMPLE_BWD, PS_KNN, PS_SHADE_FWD, PS_SHADE_BWD, PS_MLOSS_FWD, PS_MLOSS_BWD, PS_TSDF,
       PS_TSDF_NORMALS, PS_TSDF_PRIOR, PS_TSDF_SURFACE, PS_DSM_DOWNSAMPLE, PS_DSM_PIVOTS, PS_DSM_MOMENTS, PS_DSM_FINALIZE,
       PS_DSM_APPLY, PS_DSM_MAE, PS_FLOW_FWD, PS_FLOW_BWD, PS_FLOW_STATS, PS_REG_FWD, PS_REG_BWD, PS_COUNT };
static_assert(PS_COUNT <= 32, "eogs_rast_profile_select takes a 32-bit slot mask");
const char* const kSlotNames[PS_COUNT] = {"preprocess_fwd", "depth_sort", "binning", "render_fwd", "render_bwd", "gaussian_bwd",
                                          "loss_fwd", "loss_bwd", "adam", "compact", "resample_fwd", "resample_bwd", "knn",
                                          "shade_fwd", "shade_bwd", "mloss_fwd", "mloss_bwd", "tsdf",
                                          "tsdf_normals", "tsdf_prior", "tsdf_surface", "dsm_downsample", "dsm_pivots",
                                          "dsm_moments", "dsm_finalize", "dsm_apply_shift", "dsm_mae", "flow_fwd", "flow_bwd",
                                          "flow_stats",
                                          // the Gaussian-space and the render-space groups of eogs_reg.h share one slot
                                          // each way: these two fill the 32-bit mask
                                          "reg_fwd", "reg_bwd"};
struct Pending { int slot; hipEvent_t a, b; };
// process-wide (autograd runs backward on its own thread), guarded by g_prof_mu
std::mutex g_prof_mu;
std::atomic<bool> g_prof_on{false};
std::atomic<uint32_t> g_prof_mask{0xFFFFFFFFu};  // bit per slot: which kernel groups are bracketed
double g_prof_ms[PS_COUNT];
int64_t g_prof_n[PS_COUNT];
Pending g_pending[4096];
int g_npending = 0;

// events are pooled: creating / destroying a hipEvent per bracket costs several microseconds of host time each
hipEvent_t g_pool[8192];
int g_npool = 0;
bool prof_get_event(hipEvent_t* e) {  // caller holds g_prof_mu
  if (g_npool > 0) { *e = g_pool[--g_npool]; return true; }
  return hipEventCreate(e) == hipSuccess;
}
void prof_put_event(hipEvent_t e) {  // caller holds g_prof_mu
  if (g_npool < 8192) g_pool[g_npool++] = e;
  else (void)hipEventDestroy(e);
}

void prof_drain() {  // caller holds g_prof_mu
  for (int i = 0; i < g_npending; i++) {
    float ms = 0.f;
    if (hipEventSynchronize(g_pending[i].b) == hipSuccess && hipEventElapsedTime(&ms, g_pending[i].a, g_pending[i].b) == hipSuccess) {
      g_prof_ms[g_pending[i].slot] += ms;
      g_prof_n[g_pending[i].slot] += 1;
    }
    prof_put_event(g_pending[i].a);
    prof_put_event(g_pending[i].b);
  }
  g_npending = 0;
}
// The two events live in the scope object and the {slot, a, b} triple is queued only once both are recorded: forward
// and autograd's backward run on different threads, and a drain triggered by another scope must never see (or recycle)
// a half-recorded pair.
struct ProfScope {
  hipStream_t s; int slot; bool on = false; hipEvent_t a{}, b{};
  ProfScope(int slot_, hipStream_t st) : s(st), slot(slot_) {
    if (!g_prof_on.load(std::memory_order_relaxed) || !((g_prof_mask.load(std::memory_order_relaxed) >> slot) & 1u)) return;
    {
      std::lock_guard<std::mutex> lk(g_prof_mu);
      if (!prof_get_event(&a)) return;
      if (!prof_get_event(&b)) { prof_put_event(a); return; }
    }
    on = true;
    (void)hipEventRecord(a, s);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(b, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_npending == 4096) prof_drain();
    g_pending[g_npending++] = Pending{slot, a, b};
  }
};

#define LAUNCH_TRY(s, dbg, what)              \
  do {                                        \
    int rc_ = check_launch((s), (dbg), what); \
    if (rc_ != EOGS_OK) return rc_;           \
  } while (0)

}  // namespace

extern "C" {

const char* eogs_rast_last_error(void) { return g_err; }
int eogs_rast_abi_version(void) { return EOGS_RAST_ABI_VERSION; }
const char* eogs_rast_backend(void) { return "hip-gfx950"; }

int eogs_rast_geom_bytes(int P, size_t* bytes) {
  if (P < 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "geom_bytes: bad argument");
  *bytes = geom_layout(nullptr, P).bytes;
  return EOGS_OK;
}
int eogs_rast_image_bytes(int H, int W, size_t* bytes) {
  if (H < 0 || W < 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "image_bytes: bad argument");
  *bytes = img_layout(nullptr, H, W).bytes;
  return EOGS_OK;
}
int eogs_rast_binning_bytes(int P, int H, int W, int64_t R, size_t* bytes) {
  (void)P;
  if (R < 0 || H < 0 || W < 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "binning_bytes: bad argument");
  *bytes = bin_layout(nullptr, H, W, R).bytes;
  return EOGS_OK;
}
int eogs_rast_scratch_bytes(int P, int H, int W, size_t* bytes) {
  (void)H; (void)W;
  if (P < 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "scratch_bytes: bad argument");
  *bytes = sort_layout(nullptr, ent_cap(P)).bytes;
  return EOGS_OK;
}

int eogs_rast_forward_prepare(int P, int H, int W, const float* means3D, const float* scales, const float* rotations,
                              const float* cov3D_precomp, const float* opacities, const float* colors,
                              float scale_modifier, const float* viewmatrix, const float* projmatrix,
                              const float* alt_affine, unsigned flags, int* radii, void* geom,
                              size_t geom_bytes, void* scratch, size_t scratch_bytes, int64_t* num_rendered, void* stream) {
  (void)projmatrix;
  g_err[0] = 0;
  g_pending_counts.valid = false;
  if (P < 0 || H <= 0 || W <= 0 || !num_rendered) return fail(EOGS_ERR_INVALID_ARG, "forward_prepare: bad sizes");
  *num_rendered = 0;
  if (P == 0) return EOGS_OK;
  if (((W + TILE - 1) / TILE) > 32767 || ((H + TILE - 1) / TILE) > 32767)
    return fail(EOGS_ERR_INVALID_ARG, "forward_prepare: image too large for 16-bit internal tile coordinates");
  if ((uint64_t)macro_grid_x(W, BLOCK_BIG) * macro_grid_y(H, BLOCK_BIG) > MAX_BLOCKS)
    return fail(EOGS_ERR_INVALID_ARG, "forward_prepare: image too large (more than 65536 blocks of 32 x 32 pixels)");
  if (!means3D || !opacities || !viewmatrix || !radii || !geom) return fail(EOGS_ERR_INVALID_ARG, "forward_prepare: NULL input");
  if (!colors) return fail(EOGS_ERR_NO_COLORS, "For non-RGB, provide precomputed Gaussian colors!");
  const bool have_sr = scales && rotations, have_cov = cov3D_precomp != nullptr;
  if (have_sr == have_cov || (!!scales != !!rotations))
    return fail(EOGS_ERR_INVALID_ARG,
                "forward_prepare: provide exactly one of either scale/rotation pair or precomputed 3D covariance");
  const bool raw = (flags & EOGS_FLAG_RAW_PARAMS) != 0;
  if (raw && (!have_sr || !alt_affine))
    return fail(EOGS_ERR_INVALID_ARG, "forward_prepare: EOGS_FLAG_RAW_PARAMS needs scales, rotations and alt_affine");
  char* base = ws_base(geom);
  const GeomWS g = geom_layout(base, P);
  if ((size_t)(base - (char*)geom) + g.bytes - 256 > geom_bytes)
    return fail(EOGS_ERR_WORKSPACE, "forward_prepare: geom workspace too small");
  // The entry sort runs here, before the host knows how many entries there are, when the caller hands over a scratch
  // buffer of the size eogs_rast_scratch_bytes() names; otherwise (or when the entries exceed its capacity) it runs in
  // forward_render inside the binning workspace.
  SortWS sw = sort_layout(nullptr, 0);
  bool have_scratch = false;
  if (scratch) {
    char* sb = ws_base(scratch);
    sw = sort_layout(sb, ent_cap(P));
    have_scratch = (size_t)(sb - (char*)scratch) + sw.bytes - 256 <= scratch_bytes;
    if (!have_scratch) return fail(EOGS_ERR_WORKSPACE, "forward_prepare: scratch smaller than eogs_rast_scratch_bytes()");
  }
  hipStream_t s = (hipStream_t)stream;
  const bool debug = flags & EOGS_FLAG_DEBUG;
  const bool readback = !(flags & EOGS_FLAG_NO_READBACK);
  if (!readback && !(flags & EOGS_FLAG_DEFER_COUNTS))
    return fail(EOGS_ERR_INVALID_ARG, "forward_prepare: EOGS_FLAG_NO_READBACK needs EOGS_FLAG_DEFER_COUNTS");
  if (!readback && debug) return fail(EOGS_ERR_INVALID_ARG, "forward_prepare: EOGS_FLAG_DEBUG waits for the stream: not with EOGS_FLAG_NO_READBACK");
  if (readback && !g_pinned) HIP_TRY(hipHostMalloc((void**)&g_pinned, MISC_WORDS * sizeof(uint32_t), hipHostMallocDefault));

  // (g.misc needs no clearing: the scan writes every word the host reads, the error flag included)
  FwdPrepArgs a{P, H, W, means3D, scales, rotations, cov3D_precomp, opacities, colors, viewmatrix, scale_modifier,
                (flags & EOGS_FLAG_ANTIALIASING) != 0, radii, raw, alt_affine};
  { ProfScope ps(PS_PREPROCESS, s); launch_preprocess_fwd(a, g, s); }
  LAUNCH_TRY(s, debug, "preprocess_fwd");
  { ProfScope ps(PS_BINNING, s); launch_pblock_scan(g, P, s); }
  LAUNCH_TRY(s, debug, "pblock_scan");
  // The counts are read back on a side stream that waits only for the two kernels above, so the host wakes up while the
  // caller's stream is busy with the entry sort (which reads the entry count on the device) and has the rest of the
  // forward queued before the GPU runs dry.
  Side* sd = nullptr;
  if (readback) {
    sd = side_for_current_device();
    if (!sd) return fail(EOGS_ERR_DEVICE, "forward_prepare: cannot create the readback stream");
    // The host does not sleep on this copy (hipStreamSynchronize parks the thread after a short spin, and the wake-up — an
    // interrupt plus the scheduler — is on the critical path of every eager forward: a late host is an idle GPU). It arms the
    // pinned words with a sentinel here and polls them in eogs_rast_forward_counts, as a graph's host does with its mirror.
    if (g_copy_in_flight) { HIP_TRY(hipStreamSynchronize(g_copy_in_flight)); g_copy_in_flight = nullptr; }
    for (int i = 0; i < MISC_READBACK; i++) reinterpret_cast<volatile uint32_t*>(g_pinned)[i] = MIRROR_PENDING;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    HIP_TRY(hipEventRecord(sd->ev, s));
    HIP_TRY(hipStreamWaitEvent(sd->stream, sd->ev, 0));
    HIP_TRY(hipMemcpyAsync(g_pinned, g.misc, MISC_READBACK * sizeof(uint32_t), hipMemcpyDeviceToHost, sd->stream));
    g_copy_in_flight = sd->stream;
  }
  if (have_scratch) {
    ProfScope ps(PS_BINNING, s);
    launch_entry_sort(g, sw, P, H, W, s);
  }
  LAUNCH_TRY(s, debug, "entry_sort");
  if (!readback) return EOGS_OK;  // (the caller reads the counts itself: eogs_rast_read_counts)
  g_pending_counts = PendingCounts{true, P, H, W, have_scratch, sw.cap, sd->stream, (flags & EOGS_FLAG_ALT_ONLY) != 0};
  if (flags & EOGS_FLAG_DEFER_COUNTS) return EOGS_OK;  // the caller asks for the token later (eogs_rast_forward_counts)
  return eogs_rast_forward_counts(num_rendered);
}

}  // extern "C"
namespace {
// exact token of a forward from its count words (host copy of GeomWS::misc)
int token_from_counts(const uint32_t* m, int P, int H, int W, bool have_scratch, uint32_t sort_cap, int64_t* num_rendered, bool alt) {
  const uint64_t total = (uint64_t)m[MISC_TOTAL_LO] | ((uint64_t)m[MISC_TOTAL_HI] << 32);
  const uint64_t entries = (uint64_t)m[MISC_MACRO_LO] | ((uint64_t)m[MISC_MACRO_HI] << 32);
  // List granularity the render kernels read (common.h "blocks"). Per-tile lists while footprints are small: every entry a
  // wave reads is one it uses. Lists per 32 x 32-pixel block once a Gaussian is listed in many tiles: the lists are then
  // 4-7x shorter to write and re-read, which can outweigh the block-list scan in the render waves. Since the lists are built
  // per block and split locally (round 3) per-tile lists with the quad kernels win up to at least 13.8 listed tiles per
  // Gaussian (1024^2 trained 0.694 against 0.704 ms, 300 k / 1600^2 0.679 against 0.722); block lists still win at 31
  // (2048^2 trained: 1.536 against 1.596): the switch sits between — profiles/r03_regime_scan.txt.
  static const double block_switch = [] {  // tuning aid: EOGS_BLOCK_SWITCH=<tiles per Gaussian> overrides the default
    const char* e = getenv("EOGS_BLOCK_SWITCH");
    return e ? atof(e) : (double)EOGS_BLOCK_SWITCH;
  }();
  // Second criterion: termination. With opaque Gaussians a pixel stops after ~ln(1e4) / (mean alpha) list entries, so a
  // tile's list (length L = pairs / tiles) is only rendered to a depth ~1 / opacity while binning still writes all of it.
  // While per-tile binning SORTED every pair (rounds 1-2) block lists won when L * (mean pair opacity) exceeded ~115; now a
  // pair costs one 8-byte list item and the criterion loses or ties everywhere it used to fire (2 M Gaussians at opacity
  // 0.3: 1.24 ms per-tile against 1.29; 2 M / 4 M trained: equal), so it is off by default.
  static const double depth_switch = [] {  // EOGS_DEPTH_SWITCH=<L * mean opacity> overrides; 0 disables the criterion
    const char* e = getenv("EOGS_DEPTH_SWITCH");
    return e ? atof(e) : (double)EOGS_DEPTH_SWITCH;
  }();
  const uint64_t opw = (uint64_t)m[MISC_OPW_LO] | ((uint64_t)m[MISC_OPW_HI] << 32);
  const double ntiles8 = (double)macro_grid_x(W, 1) * (double)macro_grid_y(H, 1);
  const double list_depth = (double)opw / 64.0 / ntiles8;  // = L * mean pair opacity
  const bool by_footprint = (double)total > block_switch * (double)P;
  const bool by_depth = depth_switch > 0.0 && list_depth > depth_switch && total >= 2 * entries;  // blocks must merge entries
  // (an altitude-only forward — EOGS_FLAG_ALT_ONLY — runs the quad kernels' one-channel variants: per-tile lists)
  const int block = alt ? 1 : ((by_footprint || by_depth) ? BLOCK_BIG : 1);
  if (m[MISC_ERR] & 1u) return fail(EOGS_ERR_ALTITUDE, "Point is too high: altitude > 200");
  if (total >= ((uint64_t)1 << 31) || entries >= ((uint64_t)1 << 27)) return fail(EOGS_ERR_OVERFLOW, "the forward lists more than the token holds: 2^31 record slots (tile, Gaussian) or 2^27 list "
                                                                                                   "entries (32-px block, Gaussian)");
  // block_lists_kernel's 8-item build pays when the average block holds 2800 ... 6000 entries (csrc/binning.hip)
  const double per_block = (double)entries / ((double)macro_grid_x(W, BLOCK_BIG) * (double)macro_grid_y(H, BLOCK_BIG));
  // (nothing listed: the token is 0, as include/eogs_rast.h says — callers test it whole, every R > 0 shortcut applies)
  // (... except for an altitude-only forward, whose token must still say so: the render launches pick their variant by it)
  *num_rendered = (total == 0 && entries == 0 && !alt) ? 0 : nr_pack((uint32_t)total, (uint32_t)entries, block, have_scratch && entries <= (uint64_t)sort_cap,
                          per_block > 2800.0 && per_block <= 6000.0, list_depth <= (double)GB_WIDE_DEPTH, alt);
  return EOGS_OK;
}


}  // namespace
extern "C" {

int eogs_rast_forward_counts(int64_t* num_rendered) {
  g_err[0] = 0;
  if (!num_rendered) return fail(EOGS_ERR_INVALID_ARG, "forward_counts: NULL argument");
  *num_rendered = 0;
  if (!g_pending_counts.valid) return fail(EOGS_ERR_INVALID_ARG, "forward_counts: no forward_prepare pending on this thread");
  const PendingCounts pc = g_pending_counts;
  g_pending_counts.valid = false;
  const int P = pc.P, H = pc.H, W = pc.W;
  // Poll the armed words (forward_prepare); every 256 looks ask the stream, so a failed copy or a faulted kernel ends the wait
  // with its error instead of spinning for ever. Arrived = every word replaced (eogs_rast_mirror_token's rule) and the tag.
  const volatile uint32_t* v = g_pinned;
  for (uint32_t spin = 1;; spin++) {
    bool arrived = true;
    for (int i = 0; i < MISC_READBACK; i++)
      if (i != MISC_KEY_NMIN && v[i] == MIRROR_PENDING) { arrived = false; break; }
    if (arrived) break;
    if ((spin & 255u) == 0u) {
      const hipError_t q = hipStreamQuery(pc.side);
      if (q == hipSuccess) {  // the copy is done: its words are in memory
        HIP_TRY(hipStreamSynchronize(pc.side));
        break;
      }
      if (q != hipErrorNotReady) HIP_TRY(q);
    }
    __builtin_ia32_pause();
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  g_copy_in_flight = nullptr;
  uint32_t m[MISC_READBACK];
  for (int i = 0; i < MISC_READBACK; i++) m[i] = v[i];
  if (m[MISC_TAG] != MISC_TAG_VALUE) return fail(EOGS_ERR_DEVICE, "forward_counts: the count words did not arrive");
  return token_from_counts(m, P, H, W, pc.have_scratch, pc.sort_cap, num_rendered, pc.alt);
}

int eogs_rast_read_counts(int P, int H, int W, const void* geom, size_t geom_bytes, int have_scratch, void* stream,
                          int64_t* num_rendered) {
  g_err[0] = 0;
  if (P <= 0 || H <= 0 || W <= 0 || !geom || !num_rendered) return fail(EOGS_ERR_INVALID_ARG, "read_counts: bad argument");
  *num_rendered = 0;
  char* base = ws_base(const_cast<void*>(geom));
  const GeomWS g = geom_layout(base, P);
  if ((size_t)(base - (const char*)geom) + g.bytes - 256 > geom_bytes) return fail(EOGS_ERR_WORKSPACE, "read_counts: geom workspace too small");
  uint32_t m[MISC_WORDS];
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(m, g.misc, MISC_READBACK * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return token_from_counts(m, P, H, W, (have_scratch & 1) != 0, ent_cap(P), num_rendered, (have_scratch & 2) != 0);
}

static_assert(MISC_READBACK * sizeof(uint32_t) <= EOGS_MIRROR_BYTES, "mirror buffer");

int eogs_rast_mirror_arm(void* host) {
  if (!host || ((uintptr_t)host & 63u)) return fail(EOGS_ERR_INVALID_ARG, "mirror_arm: NULL or unaligned host buffer");
  volatile uint32_t* m = (volatile uint32_t*)host;
  for (int i = 0; i < MISC_READBACK; i++) m[i] = MIRROR_PENDING;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  return EOGS_OK;
}

int eogs_rast_mirror_counts(int P, const void* geom, size_t geom_bytes, void* host, void* stream) {
  g_err[0] = 0;
  if (P <= 0 || !geom || !host || ((uintptr_t)host & 63u)) return fail(EOGS_ERR_INVALID_ARG, "mirror_counts: bad argument");
  char* base = ws_base(const_cast<void*>(geom));
  const GeomWS g = geom_layout(base, P);
  if ((size_t)(base - (const char*)geom) + g.bytes - 256 > geom_bytes) return fail(EOGS_ERR_WORKSPACE, "mirror_counts: geom workspace too small");
  HIP_TRY(hipMemcpyAsync(host, g.misc, MISC_READBACK * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  return EOGS_OK;
}

int eogs_rast_mirror_token(int P, int H, int W, const void* host, int have_scratch, int64_t* num_rendered, int* arrived) {
  g_err[0] = 0;
  if (P <= 0 || H <= 0 || W <= 0 || !host || !num_rendered || !arrived) return fail(EOGS_ERR_INVALID_ARG, "mirror_token: bad argument");
  *arrived = 0;
  const volatile uint32_t* v = (const volatile uint32_t*)host;
  // Arrived = EVERY word of the 40-byte copy has replaced its sentinel, so nothing rests on the copy landing as one
  // transaction. None of them can legitimately hold the sentinel — the high words of counts below 2^31, low words
  // of counts that would otherwise be refused as overflow, a few error bits, MISC_TAG_VALUE, a positive float's bits — except
  // MISC_KEY_NMIN (~min depth key = ~0 for a depth of exactly 0.0f), which sits between two checked words of its 16 bytes.
  for (int i = 0; i < MISC_READBACK; i++)
    if (i != MISC_KEY_NMIN && v[i] == MIRROR_PENDING) return EOGS_OK;
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  uint32_t m[MISC_READBACK];
  for (int i = 0; i < MISC_READBACK; i++) m[i] = v[i];
  if (m[MISC_TAG] != MISC_TAG_VALUE) return fail(EOGS_ERR_INVALID_ARG, "mirror_token: the mirrored words are not a forward's counts");
  *arrived = 1;
  return token_from_counts(m, P, H, W, (have_scratch & 1) != 0, ent_cap(P), num_rendered, (have_scratch & 2) != 0);
}

int eogs_rast_capacity_token(int P, int64_t num_rendered, double slack, int have_scratch, int64_t exact, int64_t* capacity,
                             int* fits) {
  if (P < 0 || num_rendered < 0 || !(slack >= 0.0) || !capacity) return fail(EOGS_ERR_INVALID_ARG, "capacity_token: bad argument");
  uint64_t slots = (uint64_t)((double)nr_slots(num_rendered) * (1.0 + slack)) + 4096u;
  uint64_t ents = (uint64_t)((double)nr_entries(num_rendered) * (1.0 + slack)) + 1024u;
  if (slots > 0x7FFFFFFFull) slots = 0x7FFFFFFFull;
  if (ents > 0x07FFFFFFull) ents = 0x07FFFFFFull;
  // "sorted in scratch" only if every forward that fits this capacity also fits the scratch (then forward_prepare did sort)
  const int sorted = (have_scratch & 1) && ents <= (uint64_t)ent_cap(P);
  const int alt = (have_scratch & 2) != 0 || nr_alt(num_rendered);  // (an altitude-only forward: per-tile lists)
  *capacity = nr_pack((uint32_t)slots, (uint32_t)ents, alt ? 1 : nr_block(num_rendered), sorted, nr_wide(num_rendered),
                      nr_shallow(num_rendered), alt);
  // A capacity token carries the list granularity and the 8-item build of the EARLIER forward: speed only, every choice computes
  // the same values (ABI 3-7 also carried a choice of backward formulation that did matter for parity; gone with ABI 8).
  if (fits) *fits = exact >= 0 && capacity_fits(nr_slots(exact), nr_entries(exact), slots, ents);
  return EOGS_OK;
}

int eogs_rast_forward_render(int P, int H, int W, int64_t R, const float* bg, unsigned flags,
                             void* geom, size_t geom_bytes, void* binning, size_t binning_bytes, void* image,
                             size_t image_bytes, void* scratch, size_t scratch_bytes, float* out_color, float* out_invdepth,
                             void* stream) {
  g_err[0] = 0;
  if (P < 0 || H <= 0 || W <= 0 || R < 0 || !out_color || !bg || !image)
    return fail(EOGS_ERR_INVALID_ARG, "forward_render: bad argument");
  if (R > 0 && (P == 0 || !geom || !binning)) return fail(EOGS_ERR_INVALID_ARG, "forward_render: NULL workspace");
  if (((flags & EOGS_FLAG_ALT_ONLY) != 0) != (nr_alt(R) != 0))
    return fail(EOGS_ERR_INVALID_ARG, "forward_render: EOGS_FLAG_ALT_ONLY and the token disagree (the flag goes to forward_prepare too; "
                                      "tokens built without flags take it as have_scratch | 2)");
  if (nr_alt(R) && nr_block(R) > 1) return fail(EOGS_ERR_INVALID_ARG, "forward_render: malformed altitude-only token");
  hipStream_t s = (hipStream_t)stream;
  const bool debug = flags & EOGS_FLAG_DEBUG;
  char* ibase = ws_base(image);
  const ImgWS im = img_layout(ibase, H, W);
  if ((size_t)(ibase - (char*)image) + im.bytes - 256 > image_bytes)
    return fail(EOGS_ERR_WORKSPACE, "forward_render: image workspace too small");
  GeomWS g = geom_layout(nullptr, 0);
  BinWS b = bin_layout(nullptr, H, W, 0);
  if (P > 0) {
    char* gb = ws_base(geom);
    g = geom_layout(gb, P);
    if ((size_t)(gb - (char*)geom) + g.bytes - 256 > geom_bytes)
      return fail(EOGS_ERR_WORKSPACE, "forward_render: geom workspace too small");
  }
  if (R > 0) {
    char* bb = ws_base(binning);
    b = bin_layout(bb, H, W, R);
    if ((size_t)(bb - (char*)binning) + b.bytes - 256 > binning_bytes)
      return fail(EOGS_ERR_WORKSPACE, "forward_render: binning workspace too small");
  }
  SortWS sw = b.sort;
  if (R > 0 && nr_sorted(R)) {  // forward_prepare sorted the entries in the caller's scratch: the same buffer, untouched since
    if (!scratch) return fail(EOGS_ERR_INVALID_ARG, "forward_render: the scratch buffer handed to forward_prepare is required");
    char* sb = ws_base(scratch);
    sw = sort_layout(sb, ent_cap(P));
    if ((size_t)(sb - (char*)scratch) + sw.bytes - 256 > scratch_bytes)
      return fail(EOGS_ERR_WORKSPACE, "forward_render: scratch smaller than eogs_rast_scratch_bytes()");
  } else if (R > 0 && nr_entries(R)) {
    ProfScope ps(PS_BINNING, s);
    launch_entry_sort(g, sw, P, H, W, s);
  }
  LAUNCH_TRY(s, debug, "entry_sort");
  { ProfScope ps(PS_DEPTH_SORT, s); launch_block_lists(g, sw, b, im, P, H, W, R, s); }
  LAUNCH_TRY(s, debug, "block_lists");
  { ProfScope ps(PS_RENDER_FWD, s); launch_render_fwd(g, b, im, P, H, W, R, bg, out_color, out_invdepth, s); }
  LAUNCH_TRY(s, debug, "render_fwd");
  return EOGS_OK;
}

int eogs_rast_backward_range(int P, int H, int W, int64_t R, const float* bg, const float* means3D, const int* radii,
                             const float* colors, const float* opacities, const float* scales, const float* rotations,
                             float scale_modifier, const float* cov3D_precomp, const float* viewmatrix,
                             const float* projmatrix, const float* alt_affine, unsigned flags, const float* out_color,
                             const float* out_invdepth,
                             const float* dL_dout_color, const float* dL_dout_invdepth, const void* geom, size_t geom_bytes,
                             const void* binning, size_t binning_bytes, const void* image, size_t image_bytes,
                             float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D,
                             float* dL_dscales, float* dL_drotations, float* dL_dT_sum, float* dL_dvm_mean,
                             float* dL_dcolors_lead, int lead_cols, int p_begin, int p_end, void* stream) {
  g_err[0] = 0;
  if (P < 0 || H <= 0 || W <= 0 || R < 0) return fail(EOGS_ERR_INVALID_ARG, "backward: bad sizes");
  if (p_begin < 0 || p_end < p_begin || p_end > P || (p_begin % BLK) != 0 || (p_end != P && (p_end % BLK) != 0))
    return fail(EOGS_ERR_INVALID_ARG, "backward: the Gaussian range must lie in [0, P] with multiples of 256 as inner bounds");
  hipStream_t s = (hipStream_t)stream;
  const bool debug = flags & EOGS_FLAG_DEBUG;
  if (P == 0) {
    if (dL_dT_sum) HIP_TRY(hipMemsetAsync(dL_dT_sum, 0, 6 * sizeof(float), s));
    if (dL_dvm_mean) HIP_TRY(hipMemsetAsync(dL_dvm_mean, 0, 12 * sizeof(float), s));
    return EOGS_OK;
  }
  const bool raw = (flags & EOGS_FLAG_RAW_PARAMS) != 0;
  if (!means3D || !radii || !opacities || !viewmatrix || !projmatrix || !dL_dout_color || !geom ||
      !image || !dL_dmeans2D || !dL_dcolors || !dL_dopacity || !dL_dmeans3D || (!raw && !colors) ||
      (cov3D_precomp && !dL_dcov3D))
    return fail(EOGS_ERR_INVALID_ARG, "backward: NULL argument");
  (void)out_color; (void)out_invdepth;  // (ABI <= 7 read the rendered images back; the back-to-front walk starts from final_T in the image workspace)
  const bool have_sr = scales && rotations;
  if (have_sr == (cov3D_precomp != nullptr)) return fail(EOGS_ERR_INVALID_ARG, "backward: scale/rotation xor cov3D_precomp");
  if (have_sr && (!dL_dscales || !dL_drotations)) return fail(EOGS_ERR_INVALID_ARG, "backward: NULL scale/rotation gradient");
  if (raw && (!have_sr || !alt_affine))
    return fail(EOGS_ERR_INVALID_ARG, "backward: EOGS_FLAG_RAW_PARAMS needs scales, rotations and alt_affine");
  if (R > 0 && !binning) return fail(EOGS_ERR_INVALID_ARG, "backward: NULL binning workspace");
  if (R > 0 && !bg) return fail(EOGS_ERR_INVALID_ARG, "backward: bg is required");
  if (R > 0 && nr_alt(R) && dL_dout_invdepth)
    return fail(EOGS_ERR_INVALID_ARG, "backward: an altitude-only render (EOGS_FLAG_ALT_ONLY) has no inverse-depth output");
  if (R > 0 && nr_alt(R) && nr_block(R) > 1)
    return fail(EOGS_ERR_INVALID_ARG, "backward: malformed altitude-only token");
  if (dL_dcolors_lead && (lead_cols <= 0 || lead_cols > (raw ? 3 : NCH))) return fail(EOGS_ERR_INVALID_ARG, "backward: bad lead_cols");

  char* gb = ws_base(geom);
  const GeomWS g = geom_layout(gb, P);
  char* ib = ws_base(image);
  const ImgWS im = img_layout(ib, H, W);
  BinWS b = bin_layout(nullptr, H, W, 0);
  if (R > 0) {
    char* bb = ws_base(binning);
    b = bin_layout(bb, H, W, R);
    if ((size_t)(bb - (char*)binning) + b.bytes - 256 > binning_bytes)
      return fail(EOGS_ERR_WORKSPACE, "backward: binning workspace too small");
  }
  if ((size_t)(gb - (char*)geom) + g.bytes - 256 > geom_bytes || (size_t)(ib - (char*)image) + im.bytes - 256 > image_bytes)
    return fail(EOGS_ERR_WORKSPACE, "backward: workspace too small");

  if (R > 0 && p_begin == 0) {  // the per-pixel pass covers the whole image: once, with the first range
    { ProfScope ps(PS_RENDER_BWD, s); launch_render_bwd(g, b, im, P, H, W, R, dL_dout_color, dL_dout_invdepth, bg, raw, s); }
    LAUNCH_TRY(s, debug, "render_bwd");
  }
  GaussBwdArgs a{P, H, W, means3D, have_sr ? scales : nullptr, have_sr ? rotations : nullptr, cov3D_precomp, opacities,
                 viewmatrix, projmatrix, radii, scale_modifier, (flags & EOGS_FLAG_ANTIALIASING) != 0,
                 dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, have_sr ? dL_dscales : nullptr,
                 have_sr ? dL_drotations : nullptr, dL_dT_sum, dL_dvm_mean, raw, alt_affine, dL_dcolors_lead,
                 dL_dcolors_lead ? lead_cols : 0, nr_alt(R) != 0, R > 0 ? render_bwd_noflag_ok(b.block, R, P) : 0,
                 R > 0 ? gaussian_bwd_wide(R, P) : 0};
  { ProfScope ps(PS_GAUSS_BWD, s); launch_gaussian_bwd(a, g, b, p_begin, p_end, s); }
  LAUNCH_TRY(s, debug, "gaussian_bwd");
  return EOGS_OK;
}

int eogs_rast_backward(int P, int H, int W, int64_t R, const float* bg, const float* means3D, const int* radii,
                       const float* colors, const float* opacities, const float* scales, const float* rotations,
                       float scale_modifier, const float* cov3D_precomp, const float* viewmatrix,
                       const float* projmatrix, const float* alt_affine, unsigned flags, const float* out_color,
                       const float* out_invdepth,
                       const float* dL_dout_color, const float* dL_dout_invdepth, const void* geom, size_t geom_bytes,
                       const void* binning, size_t binning_bytes, const void* image, size_t image_bytes,
                       float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D,
                       float* dL_dscales, float* dL_drotations, float* dL_dT_sum, float* dL_dvm_mean,
                       float* dL_dcolors_lead, int lead_cols, void* stream) {
  return eogs_rast_backward_range(P, H, W, R, bg, means3D, radii, colors, opacities, scales, rotations, scale_modifier,
                                  cov3D_precomp, viewmatrix, projmatrix, alt_affine, flags, out_color, out_invdepth,
                                  dL_dout_color, dL_dout_invdepth, geom, geom_bytes, binning, binning_bytes, image,
                                  image_bytes, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dscales,
                                  dL_drotations, dL_dT_sum, dL_dvm_mean, dL_dcolors_lead, lead_cols, 0, P < 0 ? 0 : P, stream);
}

int eogs_rast_path_info(int P, int64_t R, int* list_block_px, int* fwd_kernel, int* bwd_kernel) {
  if (P < 0 || R < 0 || !list_block_px || !fwd_kernel || !bwd_kernel) return fail(EOGS_ERR_INVALID_ARG, "path_info: bad argument");
  const int block = nr_block(R);
  *list_block_px = block * SUBX;
  *fwd_kernel = render_fwd_variant(block, R, P);
  *bwd_kernel = render_bwd_variant(block, R, P);
  return EOGS_OK;
}

int eogs_rast_backward_info(int P, int64_t R, int* gaussian_bwd_wide_out) {
  if (P < 0 || R < 0 || !gaussian_bwd_wide_out) return fail(EOGS_ERR_INVALID_ARG, "backward_info: bad argument");
  *gaussian_bwd_wide_out = R > 0 ? gaussian_bwd_wide(R, P) : 0;
  return EOGS_OK;
}

// checkFrustum's predicate has its culling commented out (DGR/cuda_rasterizer/auxiliary.h:151-176): all visible.
int eogs_rast_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                           uint8_t* present, void* stream) {
  (void)means3D; (void)viewmatrix; (void)projmatrix;
  g_err[0] = 0;
  if (P < 0 || (P > 0 && !present)) return fail(EOGS_ERR_INVALID_ARG, "mark_visible: bad argument");
  if (P > 0) HIP_TRY(hipMemsetAsync(present, 1, (size_t)P, (hipStream_t)stream));
  return EOGS_OK;
}

int eogs_rast_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!on) prof_drain();
  g_prof_on = on != 0;
  return EOGS_OK;
}
int eogs_rast_profile_select(unsigned slot_mask) {
  g_prof_mask = slot_mask;
  return EOGS_OK;
}
int eogs_rast_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  prof_drain();
  for (int i = 0; i < PS_COUNT; i++) { g_prof_ms[i] = 0.0; g_prof_n[i] = 0; }
  return EOGS_OK;
}
int eogs_rast_profile_slots(void) { return PS_COUNT; }
int eogs_rast_profile_get(int slot, double* total_ms, int64_t* launches, const char** name) {
  if (slot < 0 || slot >= PS_COUNT || !total_ms || !launches || !name) return fail(EOGS_ERR_INVALID_ARG, "profile_get: bad argument");
  std::lock_guard<std::mutex> lk(g_prof_mu);
  prof_drain();
  *total_ms = g_prof_ms[slot];
  *launches = g_prof_n[slot];
  *name = kSlotNames[slot];
  return EOGS_OK;
}

int eogs_rast_selftest(void* scratch, unsigned* failed, void* stream) {
  g_err[0] = 0;
  if (!scratch || !failed) return fail(EOGS_ERR_INVALID_ARG, "selftest: bad argument");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(scratch, 0, 4, s));
  launch_selftest((uint32_t*)scratch, s);
  LAUNCH_TRY(s, true, "selftest");
  HIP_TRY(hipMemcpy(failed, scratch, 4, hipMemcpyDeviceToHost));
  return EOGS_OK;
}

// ---- include/eogs_loss.h ----
int eogs_loss_bytes(int planes, int H, int W, unsigned mode, size_t* bytes) {
  if (planes < 0 || H < 0 || W < 0 || !bytes || !(mode & (EOGS_LOSS_L1 | EOGS_LOSS_SSIM)))
    return fail(EOGS_ERR_INVALID_ARG, "loss_bytes: bad argument");
  *bytes = loss_layout(nullptr, planes, H, W, mode).bytes;
  return EOGS_OK;
}

int eogs_loss_tile_shape(int* tile_h, int* tile_w) {
  if (!tile_h || !tile_w) return fail(EOGS_ERR_INVALID_ARG, "loss_tile_shape: NULL argument");
  loss_tile_shape(tile_h, tile_w);
  return EOGS_OK;
}

int eogs_loss_window(float* taps) {
  if (!taps) return fail(EOGS_ERR_INVALID_ARG, "loss_window: NULL argument");
  const LossWindow win = loss_window();
  for (int i = 0; i < LOSS_WIN; i++) taps[i] = win.w[i];
  return EOGS_OK;
}

// launch_loss_fwd / launch_loss_bwd put the rows of tiles in gridDim.y and the planes in gridDim.z: 65535 each. The tile height
// is loss.hip's own (the monitor's standalone path launches the same forward and asks the same question).
static bool loss_grid_fits(int planes, int H) {
  int tile_h, tile_w;
  loss_tile_shape(&tile_h, &tile_w);
  return planes <= 65535 && (H - 1) / tile_h + 1 <= 65535;
}

static int loss_check(const char* who, int planes, int H, int W, const void* img, const void* gt, unsigned mode,
                      const void* ws, size_t ws_bytes, LossWS* out) {
  if (planes <= 0 || H <= 0 || W <= 0 || !(mode & (EOGS_LOSS_L1 | EOGS_LOSS_SSIM)) ||
      (mode & ~(EOGS_LOSS_L1 | EOGS_LOSS_SSIM)))
    return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes or mode", who);
  if (!loss_grid_fits(planes, H)) return fail(EOGS_ERR_INVALID_ARG, "%s: too many planes / rows for one launch", who);
  if (!img || !gt || !ws) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  char* base = ws_base(const_cast<void*>(ws));
  *out = loss_layout(base, planes, H, W, mode);
  if ((size_t)(base - (const char*)ws) + out->bytes - 256 > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  return EOGS_OK;
}

int eogs_loss_forward(int planes, int H, int W, const float* img, const float* gt, unsigned mode, float w_l1,
                      float w_ssim, float bias, float* out, float* plane_sums, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  LossWS w;
  const int rc = loss_check("loss_forward", planes, H, W, img, gt, mode, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (!out) return fail(EOGS_ERR_INVALID_ARG, "loss_forward: NULL out");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_LOSS_FWD, s); launch_loss_fwd(w, planes, H, W, img, gt, mode, w_l1, w_ssim, bias, out, plane_sums, s); }
  LAUNCH_TRY(s, false, "loss_fwd");
  return EOGS_OK;
}

int eogs_loss_backward(int planes, int H, int W, const float* img, const float* gt, unsigned mode, float w_l1,
                       float w_ssim, const float* upstream, const float* plane_grad, const void* ws, size_t ws_bytes,
                       float* dL_dimg, void* stream) {
  g_err[0] = 0;
  LossWS w;
  const int rc = loss_check("loss_backward", planes, H, W, img, gt, mode, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (!dL_dimg) return fail(EOGS_ERR_INVALID_ARG, "loss_backward: NULL dL_dimg");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_LOSS_BWD, s); launch_loss_bwd(w, planes, H, W, img, gt, mode, w_l1, w_ssim, upstream, plane_grad, dL_dimg, s); }
  LAUNCH_TRY(s, false, "loss_bwd");
  return EOGS_OK;
}

// ---- include/eogs_optim.h ----
int eogs_adam_step(int n, const eogs_adam_tensor* tensors, double beta1, double beta2, double eps, int64_t step, void* stream) {
  g_err[0] = 0;
  if (n < 0 || n > EOGS_ADAM_MAX_TENSORS || (n > 0 && !tensors) || step < 1)
    return fail(EOGS_ERR_INVALID_ARG, "adam_step: bad argument (at most 16 tensors, step >= 1)");
  for (int i = 0; i < n; i++)
    if (tensors[i].numel < 0 || (tensors[i].numel > 0 && (!tensors[i].param || !tensors[i].grad || !tensors[i].exp_avg ||
                                                          !tensors[i].exp_avg_sq)))
      return fail(EOGS_ERR_INVALID_ARG, "adam_step: NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  { ProfScope ps(PS_ADAM, s); rc = launch_adam(n, tensors, beta1, beta2, eps, step, s); }
  if (rc) return fail(EOGS_ERR_OVERFLOW, "adam_step: too many elements for one launch");
  LAUNCH_TRY(s, false, "adam");
  return EOGS_OK;
}

// ---- include/eogs_step.h ----
int eogs_step_gate(int n, const eogs_step_forward* fw, int accumulate, uint32_t* gate, void* stream) {
  g_err[0] = 0;
  if (n < 0 || n > EOGS_STEP_MAX_FORWARDS || (n > 0 && !fw) || !gate)
    return fail(EOGS_ERR_INVALID_ARG, "step_gate: bad argument (at most 16 forwards, a gate)");
  const uint32_t* misc[EOGS_STEP_MAX_FORWARDS];
  uint32_t cap_slots[EOGS_STEP_MAX_FORWARDS], cap_entries[EOGS_STEP_MAX_FORWARDS];
  for (int i = 0; i < n; i++) {
    if (fw[i].P <= 0 || !fw[i].geom || fw[i].capacity < 0) return fail(EOGS_ERR_INVALID_ARG, "step_gate: bad forward descriptor");
    char* base = ws_base(const_cast<void*>(fw[i].geom));
    const GeomWS g = geom_layout(base, fw[i].P);
    if ((size_t)(base - (const char*)fw[i].geom) + g.bytes - 256 > fw[i].geom_bytes)
      return fail(EOGS_ERR_WORKSPACE, "step_gate: geom workspace too small");
    misc[i] = g.misc;
    cap_slots[i] = nr_slots(fw[i].capacity);
    cap_entries[i] = nr_entries(fw[i].capacity);
  }
  hipStream_t s = (hipStream_t)stream;
  launch_step_gate(n, misc, cap_slots, cap_entries, accumulate, gate, s);
  LAUNCH_TRY(s, false, "step_gate");
  return EOGS_OK;
}

int eogs_step_adam_bytes(int n, size_t* bytes) {
  if (n < 0 || n > EOGS_STEP_MAX_TENSORS || !bytes) return fail(EOGS_ERR_INVALID_ARG, "step_adam_bytes: bad argument (at most 16 tensors)");
  *bytes = (size_t)n * sizeof(eogs_step_adam_scalars);
  return EOGS_OK;
}

int eogs_step_adam(int n, const eogs_step_adam_tensor* tensors, double beta1, double beta2, double eps, const uint32_t* gate,
                   void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (n < 0 || n > EOGS_STEP_MAX_TENSORS) return fail(EOGS_ERR_INVALID_ARG, "step_adam: bad argument (at most 16 tensors)");
  if (n == 0) return EOGS_OK;
  if (!tensors) return fail(EOGS_ERR_INVALID_ARG, "step_adam: NULL tensors");
  for (int i = 0; i < n; i++) {
    const eogs_step_adam_tensor& t = tensors[i];
    if (t.numel < 0 || !t.lr || !t.step || (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)))
      return fail(EOGS_ERR_INVALID_ARG, "step_adam: NULL tensor member");
  }
  if (!ws || ws_bytes < (size_t)n * sizeof(eogs_step_adam_scalars)) return fail(EOGS_ERR_WORKSPACE, "step_adam: workspace too small");
  if ((uintptr_t)ws & 15u) return fail(EOGS_ERR_INVALID_ARG, "step_adam: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  { ProfScope ps(PS_ADAM, s); rc = launch_step_adam(n, tensors, beta1, beta2, eps, gate, (eogs_step_adam_scalars*)ws, s); }
  if (rc) return fail(EOGS_ERR_OVERFLOW, "step_adam: too many elements for one launch");
  LAUNCH_TRY(s, false, "step_adam");
  return EOGS_OK;
}

int eogs_sum_into(int n, const eogs_sum_tensor* tensors, int nsrc, void* stream) {
  g_err[0] = 0;
  if (n < 0 || n > EOGS_SUM_MAX_TENSORS || nsrc < 0 || nsrc > EOGS_SUM_MAX_SOURCES || (n > 0 && !tensors))
    return fail(EOGS_ERR_INVALID_ARG, "sum_into: bad argument (at most 8 tensors with at most 4 sources each)");
  for (int i = 0; i < n; i++) {
    if (tensors[i].numel < 0 || (tensors[i].numel > 0 && !tensors[i].dst)) return fail(EOGS_ERR_INVALID_ARG, "sum_into: NULL tensor");
    for (int k = 0; k < nsrc; k++)
      if (tensors[i].numel > 0 && !tensors[i].src[k]) return fail(EOGS_ERR_INVALID_ARG, "sum_into: NULL source");
  }
  hipStream_t s = (hipStream_t)stream;
  if (launch_sum_into(n, tensors, nsrc, s)) return fail(EOGS_ERR_OVERFLOW, "sum_into: too many elements for one launch");
  LAUNCH_TRY(s, false, "sum_into");
  return EOGS_OK;
}

int eogs_pack_columns(int64_t rows, int n, const eogs_pack_tensor* tensors, float* packed, int packed_cols, int unpack,
                      void* stream) {
  g_err[0] = 0;
  if (rows < 0 || n < 0 || n > EOGS_PACK_MAX_TENSORS || packed_cols < 0 || packed_cols > 16)
    return fail(EOGS_ERR_INVALID_ARG, "pack_columns: bad sizes");
  if (rows == 0 || n == 0) return EOGS_OK;
  if (!tensors || !packed) return fail(EOGS_ERR_INVALID_ARG, "pack_columns: NULL argument");
  int total = 0;
  for (int i = 0; i < n; i++) {
    const eogs_pack_tensor& t = tensors[i];
    if (!t.data || t.width <= 0 || t.col0 < 0 || t.ncols <= 0 || t.col0 + t.ncols > t.width)
      return fail(EOGS_ERR_INVALID_ARG, "pack_columns: bad tensor descriptor");
    total += t.ncols;
  }
  if (total != packed_cols) return fail(EOGS_ERR_INVALID_ARG, "pack_columns: packed_cols is not the sum of the column counts");
  hipStream_t s = (hipStream_t)stream;
  launch_pack_columns(rows, n, tensors, packed, packed_cols, unpack, s);
  LAUNCH_TRY(s, false, "pack_columns");
  return EOGS_OK;
}

int eogs_compact_bytes(int64_t n_rows, size_t* bytes) {
  if (n_rows < 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "compact_bytes: bad argument");
  *bytes = compact_layout(nullptr, n_rows).bytes;
  return EOGS_OK;
}

static int compact_check(const char* who, int64_t n_rows, const void* keep, const void* ws, size_t ws_bytes, CompactWS* w) {
  if (n_rows < 0 || n_rows > (int64_t)0x7FFFFFFF * 128) return fail(EOGS_ERR_INVALID_ARG, "%s: bad row count", who);
  if ((n_rows > 0 && !keep) || !ws) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  char* base = ws_base(const_cast<void*>(ws));
  *w = compact_layout(base, n_rows);
  if ((size_t)(base - (const char*)ws) + w->bytes - 256 > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  return EOGS_OK;
}

int eogs_compact_plan(int64_t n_rows, const uint8_t* keep, void* ws, size_t ws_bytes, int64_t* n_keep, void* stream) {
  g_err[0] = 0;
  CompactWS w;
  const int rc = compact_check("compact_plan", n_rows, keep, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (!n_keep) return fail(EOGS_ERR_INVALID_ARG, "compact_plan: NULL n_keep");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_COMPACT, s); launch_compact_plan(w, n_rows, keep, s); }
  LAUNCH_TRY(s, false, "compact_plan");
  uint32_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, w.blk + w.nblk, sizeof total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_keep = (int64_t)total;
  return EOGS_OK;
}

int eogs_compact_apply(int64_t n_rows, const uint8_t* keep, int n_tensors, const void* const* src, void* const* dst,
                       const int* row_bytes, const void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  CompactWS w;
  const int rc = compact_check("compact_apply", n_rows, keep, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (n_tensors < 0 || (n_tensors > 0 && (!src || !dst || !row_bytes))) return fail(EOGS_ERR_INVALID_ARG, "compact_apply: bad tensor list");
  for (int t = 0; t < n_tensors; t++)
    if (row_bytes[t] < 0 || row_bytes[t] > 256 || (row_bytes[t] & 3) || (row_bytes[t] > 0 && n_rows > 0 && (!src[t] || !dst[t])))
      return fail(EOGS_ERR_INVALID_ARG, "compact_apply: row sizes must be multiples of 4 up to 256 bytes, pointers non-NULL");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_COMPACT, s); launch_compact_apply(w, n_rows, keep, n_tensors, src, dst, row_bytes, s); }
  LAUNCH_TRY(s, false, "compact_apply");
  return EOGS_OK;
}

// ---- include/eogs_resample.h ----
static int resample_check(const char* who, int C, int Hv, int Wv, int H, int W, int n_out, int fill_channel) {
  if (C <= 0 || Hv <= 0 || Wv <= 0 || H <= 0 || W <= 0 || n_out <= 0 || n_out > C || fill_channel >= n_out ||
      (int64_t)H * W > 0x7FFFFFFF || (int64_t)Hv * Wv > 0x7FFFFFFF)
    return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes", who);
  return EOGS_OK;
}

int eogs_resample_forward(int C, int Hv, int Wv, int H, int W, int n_out, const float* virtual_render, const float* uva,
                          const float* cam2virt, int fill_channel, float fill_value, float* sample, float* uv,
                          void* stream) {
  g_err[0] = 0;
  const int rc = resample_check("resample_forward", C, Hv, Wv, H, W, n_out, fill_channel);
  if (rc != EOGS_OK) return rc;
  if (!virtual_render || !uva || !cam2virt || !sample || !uv) return fail(EOGS_ERR_INVALID_ARG, "resample_forward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_RESAMPLE_FWD, s); launch_resample_fwd(C, Hv, Wv, H, W, n_out, virtual_render, uva, cam2virt, fill_channel, fill_value, sample, uv, s); }
  LAUNCH_TRY(s, false, "resample_fwd");
  return EOGS_OK;
}

int eogs_resample_bytes(int H, int W, size_t* bytes) {
  if (H <= 0 || W <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "resample_bytes: bad argument");
  *bytes = resample_bwd_ws_bytes(H, W);
  return EOGS_OK;
}

int eogs_resample_backward(int C, int Hv, int Wv, int H, int W, int n_out, const float* virtual_render, const float* uva,
                           const float* cam2virt, int fill_channel, const float* dL_dsample, const float* dL_duv,
                           float* dL_dvirtual, float* dL_duva, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  const int rc = resample_check("resample_backward", C, Hv, Wv, H, W, n_out, fill_channel);
  if (rc != EOGS_OK) return rc;
  if (!virtual_render || !uva || !cam2virt || !dL_dsample || !dL_dvirtual || !dL_duva)
    return fail(EOGS_ERR_INVALID_ARG, "resample_backward: NULL argument");
  if (ws && ws_bytes < resample_bwd_ws_bytes(H, W)) return fail(EOGS_ERR_WORKSPACE, "resample_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_RESAMPLE_BWD, s); launch_resample_bwd(C, Hv, Wv, H, W, n_out, virtual_render, uva, cam2virt, fill_channel, dL_dsample, dL_duv, dL_dvirtual, dL_duva, ws, s); }
  LAUNCH_TRY(s, false, "resample_bwd");
  return EOGS_OK;
}

// ---- include/eogs_resample.h: flow-matching warp ----
static int flow_check(const char* who, int C, int H, int W) {
  if (C < 1 || H < 2 || W < 2 || (int64_t)H * W > 0x7FFFFFFF) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes (C >= 1, H >= 2, W >= 2)", who);
  return EOGS_OK;
}

int eogs_resample_flow_forward(int C, int H, int W, const float* img, const float* flow, int64_t plane_stride,
                               int64_t row_stride, int64_t col_stride, const float* gate, float* out, void* stream) {
  g_err[0] = 0;
  const int rc = flow_check("resample_flow_forward", C, H, W);
  if (rc != EOGS_OK) return rc;
  if (!img || !flow || !out) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_forward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_FLOW_FWD, s); launch_flow_fwd(C, H, W, img, flow, plane_stride, row_stride, col_stride, gate, out, s); }
  LAUNCH_TRY(s, false, "flow_fwd");
  return EOGS_OK;
}

int eogs_resample_flow_bytes(int H, int W, size_t* bytes) {
  g_err[0] = 0;
  if (H < 2 || W < 2 || (int64_t)H * W > 0x7FFFFFFF || !bytes) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_bytes: bad argument");
  *bytes = flow_bwd_ws_bytes(H, W);
  return EOGS_OK;
}

int eogs_resample_flow_backward(int C, int H, int W, const float* flow, int64_t plane_stride, int64_t row_stride,
                                int64_t col_stride, const float* gate, const float* dL_dout, float* dL_dimg, void* ws,
                                size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  const int rc = flow_check("resample_flow_backward", C, H, W);
  if (rc != EOGS_OK) return rc;
  if (!flow || !dL_dout || !dL_dimg) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_backward: NULL argument");
  const bool field = row_stride != 0 || col_stride != 0;
  if (field && (!ws || ws_bytes < flow_bwd_ws_bytes(H, W)))
    return fail(EOGS_ERR_WORKSPACE, "resample_flow_backward: workspace too small (a flow field needs eogs_resample_flow_bytes)");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_FLOW_BWD, s); launch_flow_bwd(C, H, W, flow, plane_stride, row_stride, col_stride, gate, dL_dout, dL_dimg, ws, s); }
  LAUNCH_TRY(s, false, "flow_bwd");
  return EOGS_OK;
}

int eogs_resample_flow_stats_bytes(int H, int W, size_t* bytes) {
  g_err[0] = 0;
  if (H < 2 || W < 2 || (int64_t)H * W > 0x7FFFFFFF || !bytes) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_stats_bytes: bad argument");
  *bytes = flow_stats_ws_bytes(H, W);
  return EOGS_OK;
}

int eogs_resample_flow_stats(int H, int W, const float* flow, int64_t plane_stride, int64_t row_stride, int64_t col_stride,
                             float* stats, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  const int rc = flow_check("resample_flow_stats", 1, H, W);
  if (rc != EOGS_OK) return rc;
  if (!flow || !stats || !ws) return fail(EOGS_ERR_INVALID_ARG, "resample_flow_stats: NULL argument");
  if (ws_bytes < flow_stats_ws_bytes(H, W)) return fail(EOGS_ERR_WORKSPACE, "resample_flow_stats: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_FLOW_STATS, s); launch_flow_stats(H, W, flow, plane_stride, row_stride, col_stride, stats, ws, s); }
  LAUNCH_TRY(s, false, "flow_stats");
  return EOGS_OK;
}

// ---- include/eogs_knn.h ----
int eogs_knn_bytes(int P, size_t* bytes) {
  if (P < 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "knn_bytes: bad argument");
  *bytes = knn_layout(nullptr, P).bytes;
  return EOGS_OK;
}

int eogs_knn_mean_dist2(int P, const float* points, float* mean_dist2, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (P < 0) return fail(EOGS_ERR_INVALID_ARG, "knn_mean_dist2: bad size");
  if (P == 0) return EOGS_OK;
  if (!points || !mean_dist2 || !ws) return fail(EOGS_ERR_INVALID_ARG, "knn_mean_dist2: NULL argument");
  char* base = ws_base(ws);
  const KnnWS w = knn_layout(base, P);
  if ((size_t)(base - (char*)ws) + w.bytes - 256 > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "knn_mean_dist2: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_KNN, s); launch_knn(w, P, points, mean_dist2, s); }
  LAUNCH_TRY(s, false, "knn");
  return EOGS_OK;
}

// ---- include/eogs_shade.h ----
int eogs_shade_bytes(int H, int W, size_t* bytes) {
  g_err[0] = 0;
  if (H <= 0 || W <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "shade_bytes: bad argument");
  *bytes = shade_ws_bytes();
  return EOGS_OK;
}

int eogs_shade_forward(int H, int W, const float* raw, const float* alt_diff, const float* M, const float* inshadow,
                       float* cc, float* shaded, float* shadow, void* stream) {
  g_err[0] = 0;
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "shade_forward: bad sizes");
  if (!raw || !M || !shaded) return fail(EOGS_ERR_INVALID_ARG, "shade_forward: NULL argument");
  if ((alt_diff != nullptr) != (shadow != nullptr) || (alt_diff && !inshadow))
    return fail(EOGS_ERR_INVALID_ARG, "shade_forward: alt_diff, inshadow and shadow go together");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_SHADE_FWD, s); launch_shade_fwd(H, W, raw, alt_diff, M, inshadow, cc, shaded, shadow, s); }
  LAUNCH_TRY(s, false, "shade_fwd");
  return EOGS_OK;
}

int eogs_shade_backward(int H, int W, const float* raw, const float* alt_diff, const float* M, const float* inshadow,
                        const float* g_shaded, const float* g_cc, const float* g_shadow, float* g_raw,
                        float* g_alt_diff, float* g_params, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "shade_backward: bad sizes");
  if (!raw || !M || !g_shaded || !g_raw || !g_params || !ws) return fail(EOGS_ERR_INVALID_ARG, "shade_backward: NULL argument");
  if ((alt_diff != nullptr) != (g_alt_diff != nullptr) || (alt_diff && !inshadow) || (!alt_diff && g_shadow))
    return fail(EOGS_ERR_INVALID_ARG, "shade_backward: alt_diff, inshadow and g_alt_diff go together");
  if (ws_bytes < shade_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "shade_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_SHADE_BWD, s);
    launch_shade_bwd(H, W, raw, alt_diff, M, inshadow, g_shaded, g_cc, g_shadow, g_raw, g_alt_diff, g_params, ws, s); }
  LAUNCH_TRY(s, false, "shade_bwd");
  return EOGS_OK;
}

int eogs_mloss_forward(int H, int W, int mode, const float* alt_diff, const float* rgb_a, const float* rgb_b,
                       const float* uv, float* out, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (H <= 0 || W <= 0 || (mode != EOGS_MLOSS_SUN && mode != EOGS_MLOSS_RANDOM))
    return fail(EOGS_ERR_INVALID_ARG, "mloss_forward: bad sizes or mode");
  if (!alt_diff || !rgb_a || !rgb_b || !uv || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "mloss_forward: NULL argument");
  if (ws_bytes < shade_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "mloss_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_MLOSS_FWD, s); launch_mloss_fwd(H, W, mode, alt_diff, rgb_a, rgb_b, uv, out, ws, s); }
  LAUNCH_TRY(s, false, "mloss_fwd");
  return EOGS_OK;
}

int eogs_mloss_backward(int H, int W, int mode, const float* alt_diff, const float* rgb_a, const float* rgb_b,
                        const float* uv, const float* out, const float* upstream, float* g_alt_diff, float* g_rgb_a,
                        float* g_rgb_b, void* stream) {
  g_err[0] = 0;
  if (H <= 0 || W <= 0 || (mode != EOGS_MLOSS_SUN && mode != EOGS_MLOSS_RANDOM))
    return fail(EOGS_ERR_INVALID_ARG, "mloss_backward: bad sizes or mode");
  if (!alt_diff || !rgb_a || !rgb_b || !uv || !out || !upstream || !g_alt_diff || !g_rgb_a)
    return fail(EOGS_ERR_INVALID_ARG, "mloss_backward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_MLOSS_BWD, s);
    launch_mloss_bwd(H, W, mode, alt_diff, rgb_a, rgb_b, uv, out, upstream, g_alt_diff, g_rgb_a, g_rgb_b, s); }
  LAUNCH_TRY(s, false, "mloss_bwd");
  return EOGS_OK;
}

int eogs_tshadow_forward(int64_t n, const float* a, float* out, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (n <= 0) return fail(EOGS_ERR_INVALID_ARG, "tshadow_forward: bad size");
  if (!a || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "tshadow_forward: NULL argument");
  if (ws_bytes < shade_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "tshadow_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  launch_tshadow_fwd(n, a, out, ws, s);
  LAUNCH_TRY(s, false, "tshadow_fwd");
  return EOGS_OK;
}

int eogs_tshadow_backward(int64_t n, const float* a, const float* upstream, float* g_a, void* stream) {
  g_err[0] = 0;
  if (n <= 0) return fail(EOGS_ERR_INVALID_ARG, "tshadow_backward: bad size");
  if (!a || !upstream || !g_a) return fail(EOGS_ERR_INVALID_ARG, "tshadow_backward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  launch_tshadow_bwd(n, a, upstream, g_a, s);
  LAUNCH_TRY(s, false, "tshadow_bwd");
  return EOGS_OK;
}

// ---- include/eogs_reg.h ----
int eogs_reg_gauss_bytes(int64_t P, size_t* bytes) {
  g_err[0] = 0;
  if (P <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "reg_gauss_bytes: bad argument");
  *bytes = reg_ws_bytes();
  return EOGS_OK;
}

static int reg_gauss_check(const char* who, int64_t P, unsigned want, const float* opacity, const float* log_scales,
                           const int32_t* radii, float n_init, const float* weights) {
  if (P <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad size", who);
  if (want == 0u || (want & ~(EOGS_REG_OPACITY | EOGS_REG_OPACITY_RADII | EOGS_REG_ERANK)))
    return fail(EOGS_ERR_INVALID_ARG, "%s: `want` selects at least one of the three terms and nothing else", who);
  if (!opacity || !weights) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if ((want & EOGS_REG_ERANK) && !log_scales) return fail(EOGS_ERR_INVALID_ARG, "%s: the erank term needs log_scales (NULL argument)", who);
  if ((want & EOGS_REG_OPACITY_RADII) && !radii) return fail(EOGS_ERR_INVALID_ARG, "%s: the visible-opacity term needs radii (NULL argument)", who);
  if ((want & (EOGS_REG_OPACITY | EOGS_REG_OPACITY_RADII)) && !(n_init > 0.f))
    return fail(EOGS_ERR_INVALID_ARG, "%s: n_init must be positive", who);
  return EOGS_OK;
}

int eogs_reg_gauss_forward(int64_t P, unsigned want, const float* opacity, const float* log_scales, const int32_t* radii,
                           float n_init, const float* weights, float* out, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  const int rc = reg_gauss_check("reg_gauss_forward", P, want, opacity, log_scales, radii, n_init, weights);
  if (rc != EOGS_OK) return rc;
  if (!out || !ws) return fail(EOGS_ERR_INVALID_ARG, "reg_gauss_forward: NULL argument");
  if (ws_bytes < reg_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "reg_gauss_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_REG_FWD, s); launch_reg_gauss_fwd(P, want, opacity, log_scales, radii, n_init, weights, out, ws, s); }
  LAUNCH_TRY(s, false, "reg_gauss_fwd");
  return EOGS_OK;
}

int eogs_reg_gauss_backward(int64_t P, unsigned want, const float* opacity, const float* log_scales, const int32_t* radii,
                            float n_init, const float* weights, const float* out, const float* g_total,
                            const float* g_terms, float* g_opacity, float* g_scaling, void* stream) {
  g_err[0] = 0;
  const int rc = reg_gauss_check("reg_gauss_backward", P, want, opacity, log_scales, radii, n_init, weights);
  if (rc != EOGS_OK) return rc;
  if (!out || !g_opacity) return fail(EOGS_ERR_INVALID_ARG, "reg_gauss_backward: NULL argument");
  if (((want & EOGS_REG_ERANK) != 0u) != (g_scaling != nullptr))
    return fail(EOGS_ERR_INVALID_ARG, "reg_gauss_backward: g_scaling goes with the erank term");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_REG_BWD, s);
    launch_reg_gauss_bwd(P, want, opacity, log_scales, radii, n_init, weights, out, g_total, g_terms, g_opacity, g_scaling, s); }
  LAUNCH_TRY(s, false, "reg_gauss_bwd");
  return EOGS_OK;
}

int eogs_reg_image_bytes(int H, int W, size_t* bytes) {
  g_err[0] = 0;
  if (H < 2 || W < 2 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "reg_image_bytes: bad argument");
  *bytes = reg_ws_bytes();
  return EOGS_OK;
}

int eogs_reg_image_forward(int H, int W, const float* altitude, const float* accumulated_opacity, const float* weights,
                           float* out, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (H < 2 || W < 2) return fail(EOGS_ERR_INVALID_ARG, "reg_image_forward: bad sizes (H and W must be at least 2)");
  if ((!altitude && !accumulated_opacity) || !weights || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "reg_image_forward: NULL argument");
  if (ws_bytes < reg_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "reg_image_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_REG_FWD, s); launch_reg_image_fwd(H, W, altitude, accumulated_opacity, weights, out, ws, s); }
  LAUNCH_TRY(s, false, "reg_image_fwd");
  return EOGS_OK;
}

int eogs_reg_image_backward(int H, int W, const float* altitude, const float* accumulated_opacity, const float* weights,
                            const float* g_total, const float* g_terms, float* g_altitude, float* g_accumulated_opacity,
                            void* stream) {
  g_err[0] = 0;
  if (H < 2 || W < 2) return fail(EOGS_ERR_INVALID_ARG, "reg_image_backward: bad sizes (H and W must be at least 2)");
  if ((!altitude && !accumulated_opacity) || !weights) return fail(EOGS_ERR_INVALID_ARG, "reg_image_backward: NULL argument");
  if ((altitude != nullptr) != (g_altitude != nullptr) || (accumulated_opacity != nullptr) != (g_accumulated_opacity != nullptr))
    return fail(EOGS_ERR_INVALID_ARG, "reg_image_backward: a gradient plane goes with its input, NULL with NULL");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_REG_BWD, s);
    launch_reg_image_bwd(H, W, altitude, accumulated_opacity, weights, g_total, g_terms, g_altitude, g_accumulated_opacity, s); }
  LAUNCH_TRY(s, false, "reg_image_bwd");
  return EOGS_OK;
}

// ---- include/eogs_pan.h ----
int eogs_pan_bytes(int H, int W, size_t* bytes) {
  g_err[0] = 0;
  if (H <= 0 || W <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "pan_bytes: bad argument");
  *bytes = pan_ws_bytes();
  return EOGS_OK;
}

static int pan_check(const char* who, int H, int W, int order, int kind, const float* raw, const float* alt_diff, const float* M,
                     const float* inshadow, const float* map_params) {
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes", who);
  if (order != EOGS_PAN_ORDER_CC_FIRST && order != EOGS_PAN_ORDER_MAP_FIRST) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown order", who);
  if (kind < EOGS_PAN_ONE_CHANNEL || kind > EOGS_PAN_TRANSLATE_FROZEN) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown map kind", who);
  if (!raw || !M) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  if (alt_diff && !inshadow) return fail(EOGS_ERR_INVALID_ARG, "%s: alt_diff needs inshadow (NULL argument)", who);
  if (pan_map_params(kind) > 0 && !map_params) return fail(EOGS_ERR_INVALID_ARG, "%s: this map kind needs map_params (NULL argument)", who);
  return EOGS_OK;
}

int eogs_pan_forward(int H, int W, int order, int kind, const float* raw, const float* alt_diff, const float* M,
                     const float* inshadow, const float* map_params, float* cc, float* shaded, float* shadow,
                     void* stream) {
  g_err[0] = 0;
  const int rc = pan_check("pan_forward", H, W, order, kind, raw, alt_diff, M, inshadow, map_params);
  if (rc != EOGS_OK) return rc;
  if (!shaded || (order == EOGS_PAN_ORDER_MAP_FIRST && !cc)) return fail(EOGS_ERR_INVALID_ARG, "pan_forward: NULL argument");
  if ((alt_diff != nullptr) != (shadow != nullptr)) return fail(EOGS_ERR_INVALID_ARG, "pan_forward: alt_diff and shadow go together");
  hipStream_t s = (hipStream_t)stream;
  launch_pan_fwd(H, W, order, kind, raw, alt_diff, M, inshadow, map_params, cc, shaded, shadow, s);
  LAUNCH_TRY(s, false, "pan_fwd");
  return EOGS_OK;
}

int eogs_pan_backward(int H, int W, int order, int kind, const float* raw, const float* alt_diff, const float* M,
                      const float* inshadow, const float* map_params, const float* g_shaded, const float* g_cc,
                      const float* g_shadow, float* g_raw, float* g_alt_diff, float* g_params, void* ws, size_t ws_bytes,
                      void* stream) {
  g_err[0] = 0;
  const int rc = pan_check("pan_backward", H, W, order, kind, raw, alt_diff, M, inshadow, map_params);
  if (rc != EOGS_OK) return rc;
  if (!g_raw || !g_params || !ws) return fail(EOGS_ERR_INVALID_ARG, "pan_backward: NULL argument");
  if ((alt_diff != nullptr) != (g_alt_diff != nullptr) || (!alt_diff && g_shadow))
    return fail(EOGS_ERR_INVALID_ARG, "pan_backward: alt_diff, g_shadow and g_alt_diff go together");
  if (ws_bytes < pan_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "pan_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  launch_pan_bwd(H, W, order, kind, raw, alt_diff, M, inshadow, map_params, g_shaded, g_cc, g_shadow, g_raw, g_alt_diff, g_params,
                 ws, s);
  LAUNCH_TRY(s, false, "pan_bwd");
  return EOGS_OK;
}

// ---- include/eogs_density.h ----
int eogs_density_stats_update(int64_t P, const float* viewspace_grad, const void* radii, int radii_is_float,
                              float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream) {
  g_err[0] = 0;
  if (P < 0 || P > EOGS_DENSITY_MAX_ROWS) return fail(EOGS_ERR_INVALID_ARG, "density_stats_update: bad row count");
  if (P > 0 && (!viewspace_grad || !radii || !xyz_gradient_accum || !denom || !max_radii2D))
    return fail(EOGS_ERR_INVALID_ARG, "density_stats_update: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  launch_density_stats(P, viewspace_grad, radii, radii_is_float, xyz_gradient_accum, denom, max_radii2D, s);
  LAUNCH_TRY(s, false, "density_stats_update");
  return EOGS_OK;
}

int eogs_density_bytes(int64_t P, size_t* bytes) {
  g_err[0] = 0;
  if (P < 0 || P > EOGS_DENSITY_MAX_ROWS || !bytes) return fail(EOGS_ERR_INVALID_ARG, "density_bytes: bad argument");
  *bytes = density_layout(nullptr, P).bytes;
  return EOGS_OK;
}

static int density_check(const char* who, int64_t P, const void* flags, const void* ws, size_t ws_bytes, DensityWS* w) {
  if (P < 0 || P > EOGS_DENSITY_MAX_ROWS) return fail(EOGS_ERR_INVALID_ARG, "%s: bad row count", who);
  if ((P > 0 && !flags) || !ws) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", who);
  char* base = ws_base(const_cast<void*>(ws));
  *w = density_layout(base, P);
  if ((size_t)(base - (const char*)ws) + w->bytes - 256 > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "%s: workspace too small", who);
  return EOGS_OK;
}

int eogs_density_decide(int64_t P, const float* xyz_gradient_accum, const float* denom, const float* opacity,
                        const float* scaling, float grad_threshold, float dense_threshold, float min_opacity, int use_screen,
                        float big_threshold, float split_div, uint8_t* flags, void* ws, size_t ws_bytes, int64_t* counts,
                        void* stream) {
  g_err[0] = 0;
  DensityWS w;
  const int rc = density_check("density_decide", P, flags, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (!counts) return fail(EOGS_ERR_INVALID_ARG, "density_decide: NULL counts");
  if (P > 0 && (!xyz_gradient_accum || !denom || !opacity || !scaling)) return fail(EOGS_ERR_INVALID_ARG, "density_decide: NULL argument");
  if (!(split_div > 0.f)) return fail(EOGS_ERR_INVALID_ARG, "density_decide: split_div must be positive");
  hipStream_t s = (hipStream_t)stream;
  launch_density_decide(w, P, xyz_gradient_accum, denom, opacity, scaling, grad_threshold, dense_threshold, min_opacity, use_screen,
                        big_threshold, split_div, flags, s);
  LAUNCH_TRY(s, false, "density_decide");
  uint32_t total[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(total, w.cnt + 4 * (size_t)w.nblk, sizeof total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 4; k++) counts[k] = (int64_t)total[k];
  return EOGS_OK;
}

int eogs_density_split_rows(int64_t P, const uint8_t* flags, const void* src, void* dst, int row_bytes, const void* ws,
                            size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  DensityWS w;
  const int rc = density_check("density_split_rows", P, flags, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (row_bytes < 0 || row_bytes > 256 || (row_bytes & 3))
    return fail(EOGS_ERR_INVALID_ARG, "density_split_rows: row sizes must be multiples of 4 up to 256 bytes");
  if (row_bytes > 0 && P > 0 && (!src || !dst)) return fail(EOGS_ERR_INVALID_ARG, "density_split_rows: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  launch_density_split_rows(w, P, flags, src, dst, row_bytes, s);
  LAUNCH_TRY(s, false, "density_split_rows");
  return EOGS_OK;
}

int eogs_density_build(int64_t P, int N, const uint8_t* flags, const int64_t* counts, int n_tensors,
                       const eogs_density_tensor* tensors, const float* rotation, const float* samples, float split_div,
                       const void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  DensityWS w;
  const int rc = density_check("density_build", P, flags, ws, ws_bytes, &w);
  if (rc != EOGS_OK) return rc;
  if (N < 1 || N > EOGS_DENSITY_MAX_N) return fail(EOGS_ERR_INVALID_ARG, "density_build: N out of range");
  if (!counts) return fail(EOGS_ERR_INVALID_ARG, "density_build: NULL counts");
  for (int k = 0; k < 4; k++)
    if (counts[k] < 0 || counts[k] > P) return fail(EOGS_ERR_INVALID_ARG, "density_build: counts are not those of density_decide on these rows");
  if (counts[EOGS_DENSITY_N_KEPT_SPLIT] > counts[EOGS_DENSITY_N_SPLIT] || counts[EOGS_DENSITY_N_KEPT] + counts[EOGS_DENSITY_N_SPLIT] > P)
    return fail(EOGS_ERR_INVALID_ARG, "density_build: counts are not those of density_decide on these rows");
  if (n_tensors < 0 || (n_tensors > 0 && !tensors)) return fail(EOGS_ERR_INVALID_ARG, "density_build: bad tensor list");
  if (!(split_div > 0.f)) return fail(EOGS_ERR_INVALID_ARG, "density_build: split_div must be positive");
  const int64_t n_out = counts[0] + counts[1] + (int64_t)N * counts[3];
  bool computed = false;
  for (int t = 0; t < n_tensors; t++) {
    const eogs_density_tensor& T = tensors[t];
    if (T.row_bytes < 0 || T.row_bytes > 256 || (T.row_bytes & 3))
      return fail(EOGS_ERR_INVALID_ARG, "density_build: row sizes must be multiples of 4 up to 256 bytes");
    if (T.kind < EOGS_DENSITY_COPY || T.kind > EOGS_DENSITY_SCALING) return fail(EOGS_ERR_INVALID_ARG, "density_build: unknown tensor kind");
    if ((T.kind == EOGS_DENSITY_XYZ || T.kind == EOGS_DENSITY_SCALING) && T.row_bytes != 12)
      return fail(EOGS_ERR_INVALID_ARG, "density_build: xyz and scaling rows hold three floats");
    if (T.row_bytes > 0 && ((P > 0 && !T.src) || (n_out > 0 && !T.dst))) return fail(EOGS_ERR_INVALID_ARG, "density_build: NULL tensor pointer");
    computed = computed || T.kind == EOGS_DENSITY_XYZ;
  }
  if (computed && counts[EOGS_DENSITY_N_KEPT_SPLIT] > 0 && (!rotation || !samples))
    return fail(EOGS_ERR_INVALID_ARG, "density_build: split rows need rotation and samples (NULL argument)");
  hipStream_t s = (hipStream_t)stream;
  launch_density_build(w, P, N, flags, counts, n_tensors, tensors, rotation, samples, split_div, s);
  LAUNCH_TRY(s, false, "density_build");
  return EOGS_OK;
}

// ---- include/eogs_tsdf.h ----
int eogs_tsdf_integrate(int nx, int ny, int nz, const float* ax, const float* ay, const float* az, const float* affine,
                        float model_scale, float trunc_margin, int H, int W, const float* altitude, const float* weight,
                        float* tsdf_vol, float* weight_vol, void* stream) {
  g_err[0] = 0;
  if (nx < 0 || ny < 0 || nz < 0 || H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "tsdf_integrate: bad sizes");
  if ((size_t)nx * ny * nz == 0) return EOGS_OK;
  if ((uint64_t)nx * ny * nz > ((uint64_t)1 << 40)) return fail(EOGS_ERR_OVERFLOW, "tsdf_integrate: volume too large");
  if (!ax || !ay || !az || !affine || !altitude || !weight || !tsdf_vol || !weight_vol)
    return fail(EOGS_ERR_INVALID_ARG, "tsdf_integrate: NULL argument");
  if (!(model_scale != 0.f) || !(trunc_margin > 0.f)) return fail(EOGS_ERR_INVALID_ARG, "tsdf_integrate: bad scale or truncation");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_TSDF, s);
    launch_tsdf_integrate(nx, ny, nz, ax, ay, az, affine, model_scale, trunc_margin, H, W, altitude, weight, tsdf_vol, weight_vol, s); }
  LAUNCH_TRY(s, false, "tsdf_integrate");
  return EOGS_OK;
}

int eogs_tsdf_normals(int H, int W, const float* altitude, const float* affine, const float* view_dir, float* normals, float* angle,
                      float* weights, void* stream) {
  g_err[0] = 0;
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "tsdf_normals: bad sizes");
  if (!altitude || !affine || !view_dir || !angle) return fail(EOGS_ERR_INVALID_ARG, "tsdf_normals: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_TSDF_NORMALS, s); launch_tsdf_normals(H, W, altitude, affine, view_dir, normals, angle, weights, s); }
  LAUNCH_TRY(s, false, "tsdf_normals");
  return EOGS_OK;
}

int eogs_tsdf_prior_bytes(int nx, int ny, int nz, size_t* bytes) {
  g_err[0] = 0;
  if (nx < 0 || ny < 0 || nz < 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "tsdf_prior_bytes: bad argument");
  if ((uint64_t)nx * ny * nz > ((uint64_t)1 << 40)) return fail(EOGS_ERR_OVERFLOW, "tsdf_prior_bytes: volume too large");
  *bytes = tsdf_prior_ws_bytes(nx, ny, nz);
  return EOGS_OK;
}

int eogs_tsdf_prior(int nx, int ny, int nz, float* tsdf_vol, float* weight_vol, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (nx < 0 || ny < 0 || nz < 0) return fail(EOGS_ERR_INVALID_ARG, "tsdf_prior: bad sizes");
  if ((size_t)nx * ny * nz == 0) return EOGS_OK;
  if ((uint64_t)nx * ny * nz > ((uint64_t)1 << 40)) return fail(EOGS_ERR_OVERFLOW, "tsdf_prior: volume too large");
  if (!tsdf_vol || !weight_vol || !ws) return fail(EOGS_ERR_INVALID_ARG, "tsdf_prior: NULL argument");
  if (ws_bytes < tsdf_prior_ws_bytes(nx, ny, nz)) return fail(EOGS_ERR_WORKSPACE, "tsdf_prior: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_TSDF_PRIOR, s); launch_tsdf_prior(nx, ny, nz, tsdf_vol, weight_vol, ws, s); }
  LAUNCH_TRY(s, false, "tsdf_prior");
  return EOGS_OK;
}

int eogs_tsdf_surface(int nx, int ny, int nz, const float* tsdf_vol, const float* az, int64_t* index, float* height, void* stream) {
  g_err[0] = 0;
  if (nx < 0 || ny < 0 || nz <= 0) return fail(EOGS_ERR_INVALID_ARG, "tsdf_surface: bad sizes");
  if ((size_t)nx * ny == 0) return EOGS_OK;
  if ((uint64_t)nx * ny * nz > ((uint64_t)1 << 40)) return fail(EOGS_ERR_OVERFLOW, "tsdf_surface: volume too large");
  if (!tsdf_vol || !az || !index) return fail(EOGS_ERR_INVALID_ARG, "tsdf_surface: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_TSDF_SURFACE, s); launch_tsdf_surface(nx, ny, nz, tsdf_vol, az, index, height, s); }
  LAUNCH_TRY(s, false, "tsdf_surface");
  return EOGS_OK;
}

}  // extern "C"

// ---- include/eogs_tsdf.h: DSM evaluation (dsm_eval.hip) ----
namespace {

int dsm_check_pair(const char* what, int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int irange) {
  if (Hu <= 0 || Wu <= 0 || Hv <= 0 || Wv <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes", what);
  if (Hv < Hu || Wv < Wu) return fail(EOGS_ERR_INVALID_ARG, "%s: the image to register is smaller than the reference image", what);
  if ((uint64_t)Hv * Wv > ((uint64_t)1 << 31)) return fail(EOGS_ERR_OVERFLOW, "%s: image too large", what);
  if (irange < 0 || irange > EOGS_TSDF_DSM_MAX_IRANGE) return fail(EOGS_ERR_INVALID_ARG, "%s: irange outside 0 .. 8", what);
  if (!u || !v) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL argument", what);
  return EOGS_OK;
}

// one level: pivots, the moments of every shift, their sum, the NCC table and its winner
void dsm_search(int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int f64, int irange, const int32_t* centre,
                int centre_scale, double* table, eogs_tsdf_dsm_result* result, const DsmNccWS& w, hipStream_t s) {
  { ProfScope ps(PS_DSM_PIVOTS, s); launch_dsm_pivots((int64_t)Hu * Wu, u, (int64_t)Hv * Wv, v, f64, w.pivots, s); }
  { ProfScope ps(PS_DSM_MOMENTS, s); launch_dsm_moments(Hu, Wu, u, Wv, v, f64, irange, centre, centre_scale, w, s); }
  { ProfScope ps(PS_DSM_FINALIZE, s); launch_dsm_finalize(irange, centre, centre_scale, w, table, result, s); }
}

struct DsmShiftWS {
  int levels;
  int hu[DSM_MAX_LEVELS], wu[DSM_MAX_LEVELS], hv[DSM_MAX_LEVELS], wv[DSM_MAX_LEVELS];
  double *pu[DSM_MAX_LEVELS], *pv[DSM_MAX_LEVELS];  // float64 pyramid levels 1 .. levels-1 ([0] is the caller's image)
  char* ncc;
  size_t bytes;
};
DsmShiftWS dsm_shift_layout(char* base, int Hu, int Wu, int Hv, int Wv, int irange) {
  DsmShiftWS w;
  w.levels = 1;
  w.hu[0] = Hu; w.wu[0] = Wu; w.hv[0] = Hv; w.wv[0] = Wv;
  w.pu[0] = w.pv[0] = nullptr;
  size_t off = 0;
  while ((Hu < Wu ? Hu : Wu) > 100 && w.levels < DSM_MAX_LEVELS) {  // dsmr.py:168
    Hu = (Hu + 1) / 2; Wu = (Wu + 1) / 2; Hv = (Hv + 1) / 2; Wv = (Wv + 1) / 2;
    const int k = w.levels++;
    w.hu[k] = Hu; w.wu[k] = Wu; w.hv[k] = Hv; w.wv[k] = Wv;
    off = ws_carve(base, off, w.pu[k], (size_t)Hu * Wu);
    off = ws_carve(base, off, w.pv[k], (size_t)Hv * Wv);
  }
  off = ws_align(off);
  w.ncc = base ? base + off : nullptr;
  w.bytes = off + dsm_ncc_layout(nullptr, w.hu[0], w.wu[0], irange).bytes + 256;
  return w;
}

}  // namespace

extern "C" {

int eogs_tsdf_dsm_downsample(int H, int W, const void* in, int f64, double* out, void* stream) {
  g_err[0] = 0;
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "dsm_downsample: bad sizes");
  if ((uint64_t)H * W > ((uint64_t)1 << 31)) return fail(EOGS_ERR_OVERFLOW, "dsm_downsample: image too large");
  if (!in || !out) return fail(EOGS_ERR_INVALID_ARG, "dsm_downsample: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_DSM_DOWNSAMPLE, s); launch_dsm_downsample(H, W, in, f64, out, s); }
  LAUNCH_TRY(s, false, "dsm_downsample");
  return EOGS_OK;
}

int eogs_tsdf_dsm_ncc_bytes(int Hu, int Wu, int irange, size_t* bytes) {
  g_err[0] = 0;
  if (Hu <= 0 || Wu <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_ncc_bytes: bad argument");
  if (irange < 0 || irange > EOGS_TSDF_DSM_MAX_IRANGE) return fail(EOGS_ERR_INVALID_ARG, "dsm_ncc_bytes: irange outside 0 .. 8");
  *bytes = dsm_ncc_layout(nullptr, Hu, Wu, irange).bytes;
  return EOGS_OK;
}

int eogs_tsdf_dsm_ncc(int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int f64, int irange, const int32_t* centre,
                      int centre_scale, double* table, eogs_tsdf_dsm_result* result, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  const int rc = dsm_check_pair("dsm_ncc", Hu, Wu, u, Hv, Wv, v, irange);
  if (rc != EOGS_OK) return rc;
  if (!result || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_ncc: NULL argument");
  if (ws_bytes < dsm_ncc_layout(nullptr, Hu, Wu, irange).bytes) return fail(EOGS_ERR_WORKSPACE, "dsm_ncc: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  dsm_search(Hu, Wu, u, Hv, Wv, v, f64, irange, centre, centre_scale, table, result, dsm_ncc_layout(ws_base(ws), Hu, Wu, irange), s);
  LAUNCH_TRY(s, false, "dsm_ncc");
  return EOGS_OK;
}

int eogs_tsdf_dsm_shift_bytes(int Hu, int Wu, int Hv, int Wv, int irange, size_t* bytes, int* levels) {
  g_err[0] = 0;
  if (Hu <= 0 || Wu <= 0 || Hv < Hu || Wv < Wu || !bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_shift_bytes: bad argument");
  if (irange < 0 || irange > EOGS_TSDF_DSM_MAX_IRANGE) return fail(EOGS_ERR_INVALID_ARG, "dsm_shift_bytes: irange outside 0 .. 8");
  const DsmShiftWS w = dsm_shift_layout(nullptr, Hu, Wu, Hv, Wv, irange);
  *bytes = w.bytes;
  if (levels) *levels = w.levels;
  return EOGS_OK;
}

int eogs_tsdf_dsm_shift(int Hu, int Wu, const void* u, int Hv, int Wv, const void* v, int f64, int irange, double* tables,
                        eogs_tsdf_dsm_result* results, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  const int rc = dsm_check_pair("dsm_shift", Hu, Wu, u, Hv, Wv, v, irange);
  if (rc != EOGS_OK) return rc;
  if (!results || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_shift: NULL argument");
  const DsmShiftWS w = dsm_shift_layout(ws_base(ws), Hu, Wu, Hv, Wv, irange);
  if (ws_bytes < w.bytes) return fail(EOGS_ERR_WORKSPACE, "dsm_shift: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int n = 2 * irange + 1;
  {
    ProfScope ps(PS_DSM_DOWNSAMPLE, s);
    for (int k = 1; k < w.levels; k++) {
      const int src64 = k == 1 ? f64 : 1;
      launch_dsm_downsample(w.hu[k - 1], w.wu[k - 1], k == 1 ? u : (const void*)w.pu[k - 1], src64, w.pu[k], s);
      launch_dsm_downsample(w.hv[k - 1], w.wv[k - 1], k == 1 ? v : (const void*)w.pv[k - 1], src64, w.pv[k], s);
    }
  }
  for (int k = w.levels - 1; k >= 0; k--) {
    // recursive_ncc halves (0, 0) on its way down (dx // 2, dsmr.py:171-172): the coarsest level searches around (0, 0)
    const int32_t* centre = k == w.levels - 1 ? nullptr : &results[k + 1].dx;
    dsm_search(w.hu[k], w.wu[k], k == 0 ? u : (const void*)w.pu[k], w.hv[k], w.wv[k], k == 0 ? v : (const void*)w.pv[k],
               k == 0 ? f64 : 1, irange, centre, 2, tables ? tables + (size_t)k * n * n : nullptr, results + k,
               dsm_ncc_layout(w.ncc, w.hu[k], w.wu[k], irange), s);
  }
  LAUNCH_TRY(s, false, "dsm_shift");
  return EOGS_OK;
}

int eogs_tsdf_dsm_apply_shift(int H, int W, const void* in, int f64, int dx, int dy, double a, double b, double c, double d,
                              void* out, void* stream) {
  g_err[0] = 0;
  if (H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "dsm_apply_shift: bad sizes");
  if ((uint64_t)H * W > ((uint64_t)1 << 31)) return fail(EOGS_ERR_OVERFLOW, "dsm_apply_shift: image too large");
  if (!in || !out || in == out) return fail(EOGS_ERR_INVALID_ARG, "dsm_apply_shift: NULL or aliased argument");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_DSM_APPLY, s); launch_dsm_apply_shift(H, W, in, f64, dx, dy, a, b, c, d, out, s); }
  LAUNCH_TRY(s, false, "dsm_apply_shift");
  return EOGS_OK;
}

int eogs_tsdf_dsm_mae_bytes(size_t* bytes) {
  g_err[0] = 0;
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_mae_bytes: NULL argument");
  *bytes = dsm_mae_ws_bytes();
  return EOGS_OK;
}

int eogs_tsdf_dsm_mae(int Hp, int Wp, void* pred, int Hg, int Wg, const void* gt, int f64, int clip_finite, void* diff, double* out,
                      void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (Hp <= 0 || Wp <= 0 || Hg <= 0 || Wg <= 0) return fail(EOGS_ERR_INVALID_ARG, "dsm_mae: bad sizes");
  if ((uint64_t)Hp * Wp > ((uint64_t)1 << 31) || (uint64_t)Hg * Wg > ((uint64_t)1 << 31))
    return fail(EOGS_ERR_OVERFLOW, "dsm_mae: image too large");
  if (!pred || !gt || !diff || !out || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_mae: NULL argument");
  if (ws_bytes < dsm_mae_ws_bytes()) return fail(EOGS_ERR_WORKSPACE, "dsm_mae: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  { ProfScope ps(PS_DSM_MAE, s); launch_dsm_mae(Hp, Wp, pred, Hg, Wg, gt, f64, clip_finite, diff, out, ws, s); }
  LAUNCH_TRY(s, false, "dsm_mae");
  return EOGS_OK;
}

// ---- include/eogs_monitor.h ----
int eogs_monitor_state_bytes(size_t* bytes) {
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "monitor_state_bytes: NULL argument");
  *bytes = sizeof(eogs_monitor_state);
  return EOGS_OK;
}

static int monitor_state_check(const char* who, const void* state) {
  if (!state) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL state", who);
  if ((uintptr_t)state & 15u) return fail(EOGS_ERR_INVALID_ARG, "%s: state not 16-byte aligned", who);
  return EOGS_OK;
}

int eogs_monitor_reset(void* state, size_t state_bytes, int op, void* stream) {
  g_err[0] = 0;
  const int rc = monitor_state_check("monitor_reset", state);
  if (rc != EOGS_OK) return rc;
  if (state_bytes < sizeof(eogs_monitor_state)) return fail(EOGS_ERR_WORKSPACE, "monitor_reset: state buffer too small");
  if (op != EOGS_MONITOR_MIN && op != EOGS_MONITOR_MAX) return fail(EOGS_ERR_INVALID_ARG, "monitor_reset: operator is min or max");
  hipStream_t s = (hipStream_t)stream;
  launch_monitor_reset(state, op, s);
  LAUNCH_TRY(s, false, "monitor_reset");
  return EOGS_OK;
}

static int monitor_image_check(const char* who, int planes, int H, int W) {
  if (planes <= 0 || H <= 0 || W <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad sizes", who);
  if (!loss_grid_fits(planes, H)) return fail(EOGS_ERR_INVALID_ARG, "%s: too many planes / rows for one launch", who);
  return EOGS_OK;
}

int eogs_monitor_observe_bytes(int planes, int H, int W, int standalone, size_t* bytes) {
  const int rc = monitor_image_check("monitor_observe_bytes", planes, H, W);
  if (rc != EOGS_OK) return rc;
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe_bytes: NULL argument");
  size_t n = 256 + monitor_sq_bytes(planes, H, W);
  if (standalone) n += 256 + loss_layout(nullptr, planes, H, W, EOGS_LOSS_L1 | EOGS_LOSS_SSIM).bytes;
  *bytes = n;
  return EOGS_OK;
}

int eogs_monitor_observe(int planes, int H, int W, const float* image, const float* gt, const float* loss_out,
                         double lambda_dssim, int kind, int photometric_on, const uint32_t* gate, void* state, void* ws,
                         size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  int rc = monitor_image_check("monitor_observe", planes, H, W);
  if (rc != EOGS_OK) return rc;
  if (kind != EOGS_MONITOR_KIND_PAN && kind != EOGS_MONITOR_KIND_MSI)
    return fail(EOGS_ERR_INVALID_ARG, "monitor_observe: kind is pan or msi");
  if (!image || !gt || !ws) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe: NULL argument");
  if (!(lambda_dssim == lambda_dssim)) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe: lambda_dssim is NaN");
  rc = monitor_state_check("monitor_observe", state);
  if (rc != EOGS_OK) return rc;
  char* base = ws_base(ws);
  const size_t sq = monitor_sq_bytes(planes, H, W);
  size_t need = (size_t)(base - (char*)ws) + sq;
  LossWS w;
  const unsigned mode = EOGS_LOSS_L1 | EOGS_LOSS_SSIM;
  if (!loss_out) {
    w = loss_layout(base + sq + 256, planes, H, W, mode);
    need += 256 + w.bytes - 256;
  }
  if (need > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "monitor_observe: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const float lam = (float)lambda_dssim, oml = (float)(1.0 - lambda_dssim);  // torch rounds the Python scalars once each
  if (!loss_out) {
    float* out = reinterpret_cast<float*>(base + sq);
    { ProfScope ps(PS_LOSS_FWD, s); launch_loss_fwd(w, planes, H, W, image, gt, mode, oml, -lam, lam, out, nullptr, s); }
    loss_out = out;
  }
  launch_monitor_observe(planes, H, W, image, gt, loss_out, oml, lam, kind, photometric_on != 0, gate, state,
                         reinterpret_cast<double*>(base), s);
  LAUNCH_TRY(s, false, "monitor_observe");
  return EOGS_OK;
}

int eogs_monitor_model_bytes(int64_t P, size_t* bytes) {
  if (P <= 0 || !bytes) return fail(EOGS_ERR_INVALID_ARG, "monitor_model_bytes: bad argument");
  *bytes = monitor_model_ws_bytes(P);
  return EOGS_OK;
}

int eogs_monitor_observe_model(int64_t P, const float* opacity, const uint32_t* gate, void* state, void* ws, size_t ws_bytes,
                               void* stream) {
  g_err[0] = 0;
  if (P <= 0) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe_model: bad size");
  if (!opacity || !ws) return fail(EOGS_ERR_INVALID_ARG, "monitor_observe_model: NULL argument");
  const int rc = monitor_state_check("monitor_observe_model", state);
  if (rc != EOGS_OK) return rc;
  if (ws_bytes < monitor_model_ws_bytes(P)) return fail(EOGS_ERR_WORKSPACE, "monitor_observe_model: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  launch_monitor_model(P, opacity, gate, state, ws, s);
  LAUNCH_TRY(s, false, "monitor_observe_model");
  return EOGS_OK;
}

int eogs_monitor_end_iteration(const float* loss, const uint32_t* gate, void* state, void* stream) {
  g_err[0] = 0;
  if (!loss) return fail(EOGS_ERR_INVALID_ARG, "monitor_end_iteration: NULL loss");
  const int rc = monitor_state_check("monitor_end_iteration", state);
  if (rc != EOGS_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  launch_monitor_end_iteration(loss, gate, state, s);
  LAUNCH_TRY(s, false, "monitor_end_iteration");
  return EOGS_OK;
}

int eogs_monitor_close_interval(int metric, int op, int64_t patience, const uint32_t* gate, void* state, void* stream) {
  g_err[0] = 0;
  if (metric < 0 || metric >= EOGS_MONITOR_METRICS) return fail(EOGS_ERR_INVALID_ARG, "monitor_close_interval: unknown metric");
  if (op != EOGS_MONITOR_MIN && op != EOGS_MONITOR_MAX)
    return fail(EOGS_ERR_INVALID_ARG, "monitor_close_interval: operator is min or max");
  const int rc = monitor_state_check("monitor_close_interval", state);
  if (rc != EOGS_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  launch_monitor_close(metric, op, patience, gate, state, s);
  LAUNCH_TRY(s, false, "monitor_close_interval");
  return EOGS_OK;
}

// ---- include/eogs_dsm.h ----
static int dsm_source_check(const char* who, const eogs_dsm_source* src) {
  if (!src) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL source", who);
  if (src->kind == EOGS_DSM_SRC_CLOUD) {
    if (src->N < 0) return fail(EOGS_ERR_INVALID_ARG, "%s: negative point count", who);
    if (src->N > 0 && !src->cloud) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL cloud", who);
    if ((uintptr_t)src->cloud & 7u) return fail(EOGS_ERR_INVALID_ARG, "%s: cloud not 8-byte aligned", who);
    return EOGS_OK;
  }
  if (src->kind != EOGS_DSM_SRC_VIEW && src->kind != EOGS_DSM_SRC_GRID) return fail(EOGS_ERR_INVALID_ARG, "%s: unknown source kind", who);
  if (src->H <= 0 || src->W <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: bad image size", who);
  if (!src->altitude || !src->u_axis || !src->v_axis) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL image or axis", who);
  if (src->kind == EOGS_DSM_SRC_VIEW) {
    if (!src->affine) return fail(EOGS_ERR_INVALID_ARG, "%s: NULL affine", who);
    if (!(src->scale == src->scale)) return fail(EOGS_ERR_INVALID_ARG, "%s: scale is NaN", who);
  }
  return EOGS_OK;
}

int eogs_dsm_bounds_bytes(size_t* bytes) {
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_bounds_bytes: NULL argument");
  *bytes = 256 + dsm_bounds_ws_bytes();
  return EOGS_OK;
}

int eogs_dsm_bounds(const eogs_dsm_source* src, eogs_dsm_bounds_result* result, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  const int rc = dsm_source_check("dsm_bounds", src);
  if (rc != EOGS_OK) return rc;
  if (!result || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_bounds: NULL argument");
  if ((uintptr_t)result & 7u) return fail(EOGS_ERR_INVALID_ARG, "dsm_bounds: result not 8-byte aligned");
  char* base = ws_base(ws);
  if ((size_t)(base - (char*)ws) + dsm_bounds_ws_bytes() > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "dsm_bounds: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  launch_dsm_bounds(*src, result, base, s);
  LAUNCH_TRY(s, false, "dsm_bounds");
  return EOGS_OK;
}

static int dsm_grid_check(const char* who, int xsize, int ysize, int radius) {
  if (radius < 0 || radius > EOGS_DSM_MAX_RADIUS) return fail(EOGS_ERR_INVALID_ARG, "%s: radius out of range", who);
  if (xsize <= 0 || ysize <= 0) return fail(EOGS_ERR_INVALID_ARG, "%s: xsize and ysize must be positive", who);
  if (((int64_t)xsize + 2 * radius) * ((int64_t)ysize + 2 * radius) >= ((int64_t)1 << 31))
    return fail(EOGS_ERR_INVALID_ARG, "%s: raster too large", who);
  return EOGS_OK;
}

int eogs_dsm_raster_bytes(int xsize, int ysize, int radius, size_t* bytes) {
  const int rc = dsm_grid_check("dsm_raster_bytes", xsize, ysize, radius);
  if (rc != EOGS_OK) return rc;
  if (!bytes) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster_bytes: NULL argument");
  *bytes = 256 + dsm_raster_layout(nullptr, xsize, ysize, radius).bytes;
  return EOGS_OK;
}

int eogs_dsm_raster(const eogs_dsm_source* src, double xoff, double yoff, double res, int xsize, int ysize, int radius,
                    float* out, int32_t* count, int64_t* skipped, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  int rc = dsm_source_check("dsm_raster", src);
  if (rc != EOGS_OK) return rc;
  rc = dsm_grid_check("dsm_raster", xsize, ysize, radius);
  if (rc != EOGS_OK) return rc;
  const double big = 1.7976931348623157e308;
  if (!(res > 0. && res <= big)) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster: resolution must be positive and finite");
  if (!(xoff >= -big && xoff <= big && yoff >= -big && yoff <= big)) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster: xoff, yoff must be finite");
  if (!out || !ws) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster: NULL argument");
  if ((uintptr_t)skipped & 7u) return fail(EOGS_ERR_INVALID_ARG, "dsm_raster: skipped not 8-byte aligned");
  char* base = ws_base(ws);
  const DsmRasterWS w = dsm_raster_layout(base, xsize, ysize, radius);
  if ((size_t)(base - (char*)ws) + w.bytes > ws_bytes) return fail(EOGS_ERR_WORKSPACE, "dsm_raster: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  launch_dsm_raster(*src, xoff, yoff, res, xsize, ysize, radius, w, out, count, skipped, s);
  LAUNCH_TRY(s, false, "dsm_raster");
  return EOGS_OK;
}

}  // extern "C"
