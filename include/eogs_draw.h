/*
 * eogs_draw.h — C-ABI of the per-iteration random draws: what the reference draws on the host in every training iteration
 * beside the view, computed on the device from a counter-based generator, so that a recorded step
 * (eogs2_amd.graph.GraphedStep) renders against another background and another virtual camera on every replay:
 *
 *   the background      train_pan.py:272-277: bg = torch.rand(5), bg[3] = cam.altitude_bounds[0], bg[4] = 0
 *   the virtual camera  scene/cameras/affine_cameras.py:403-430 sample_random_camera (called at train_pan.py:375-378):
 *                       the view's affine sheared by randn(2).clip(-1, 1) * extent; and :372-401 get_nadir_camera, the same
 *                       formula with a deterministic shear
 *
 *   eogs_draw_iteration  one launch of one wave: lane t draws for camera t of the iteration
 *   eogs_draw_advance    one gated single-thread launch: a stream's own counter moves on
 *
 * Every draw is a pure function of (seed, iteration, camera slot, purpose): Philox4x32-10 with key = the seed's two words and
 * counter = (iteration low, iteration high, slot, purpose), purpose 0 = background, 1 = camera shear (csrc/draw_rng.h). The
 * iteration is read from a device int64 — typically the cursor of an eogs_views_schedule, which eogs_views_advance moves
 * under the step's gate — so there is no generator state to save, gate or record again.
 *
 * Same conventions as eogs_views.h: DEVICE pointers, `void* stream` is a hipStream_t, int status (0 ok, <0 error, message via
 * eogs_rast_last_error()), no device allocation inside the library, arguments are checked before anything is queued.
 * Everything is asynchronous on `stream` and consists of kernel launches alone: a stream capture records it. Nothing here
 * reads the rasterizer's state.
 */
#ifndef EOGS_DRAW_H_INCLUDED
#define EOGS_DRAW_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOGS_DRAW_MAX_CAMERAS 8
#define EOGS_DRAW_BG 1u            /* bg[0..2] = three uniforms of [0, 1), bg[3] = *alt_floor if given, bg[4] = 0 */
#define EOGS_DRAW_BG_COPY_FIRST 2u /* with BG: bg[1] = bg[2] = bg[0] (the reference's copy_background_firschan) */
#define EOGS_DRAW_CAMERA 4u        /* the random shear: d_i = clamp(normal_i, -1, 1) * extent */
#define EOGS_DRAW_NADIR 8u         /* the deterministic shear d_i = -A[i][2] / A[2][2]; reads no generator; not with CAMERA */

/* Where the iteration's index comes from. `counter` is a device int64 (8-byte aligned), read as unsigned. */
typedef struct {
  uint64_t seed;
  const int64_t* counter;
} eogs_draw_stream;

/* One camera of the iteration; its index in the array is its slot in the generator's counter.
 *
 * `affine` is the view's 4 x 4 affine stored transposed, as the reference stores it: A = affine[:3,:3]^T, i.e.
 * A[i][j] = affine[4 j + i], and b[i] = affine[12 + i]. With CAMERA or NADIR, for i in {0, 1}:
 *
 *   new_A[i][j] = fmaf(d_i, A[2][j], A[i][j])
 *   s           = A[2][:] . center, as the fma chain fmaf(A[2][2], c2, fmaf(A[2][1], c1, A[2][0] * c0))
 *   new_b[i]    = fmaf(-d_i, s, b[i])
 *
 * row 2 of A and b[2] are copied bit for bit, the last column is 0, 0, 0, 1 (the reference's eye(4)), and `virt_affine` is
 * written transposed like `affine`. `cam2virt` is the row-major 3 x 3 identity with [0][2] = d_0 * cam2virt_scale and
 * [1][2] = d_1 * cam2virt_scale: scale 1 gives the reference's myM. `shear` receives d_0, d_1. No clamp but the stated one:
 * NaN and infinities propagate as the arithmetic has them, A[2][2] == 0 under NADIR gives what the float division gives.
 *
 * A camera flag needs `affine` and at least one of virt_affine, cam2virt, shear; virt_affine needs `center`. BG needs `bg`.
 * Pointers the flags do not ask for may be NULL and are not touched. Every pointer is 4-byte aligned. An output must not
 * overlap any input of the same call: lanes run side by side. */
typedef struct {
  const float* affine;    /* [16] */
  const float* center;    /* [3]  */
  const float* alt_floor; /* [1], may be NULL: bg[3] is then left alone */
  float* bg;              /* [5]  */
  float* virt_affine;     /* [16] */
  float* cam2virt;        /* [9]  */
  float* shear;           /* [2], optional */
  float extent;           /* CAMERA: finite, >= 0 */
  float cam2virt_scale;   /* finite, >= 0 */
  uint32_t flags;         /* EOGS_DRAW_*: at least one of BG, CAMERA, NADIR */
} eogs_draw_camera;

/* `cams` is a HOST array of n <= EOGS_DRAW_MAX_CAMERAS descriptors (copied into the kernel arguments). One launch, one
 * wave: lane t < n draws for camera t at iteration *stream_desc->counter. n == 0 queues nothing. */
int eogs_draw_iteration(int n, const eogs_draw_camera* cams, const eogs_draw_stream* stream_desc, void* stream);

/* One single-thread launch: *counter += 1, unless gate != NULL and gate[0] == 0 (`gate`: the uint32[2] of eogs_step_gate,
 * eogs_step.h). For a stream that owns its counter; a counter that is a schedule's cursor is moved by eogs_views_advance. */
int eogs_draw_advance(int64_t* counter, const uint32_t* gate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_DRAW_H_INCLUDED */
