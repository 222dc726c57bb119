/*
 * eogs_monitor.h — C-ABI of the training monitor: the part of the reference's loop that WATCHES the training
 * (src/gaussiansplatting/train_pan.py:423-429, 471-495, 512-597 and utils/callback_utils.py:15-44), kept in one device
 * buffer and advanced by kernel launches alone. Per camera and iteration the reference reads five or more scalars back
 * with `.item()` and evaluates SSIM a second time; here nothing waits for the device until the caller copies one record.
 *
 *   eogs_monitor_reset           fill a state buffer: zero sums, best = +inf (min) or -inf (max)
 *   eogs_monitor_observe         one camera of one iteration: L1, SSIM, photometric, PSNR into the interval's sums
 *   eogs_monitor_observe_model   mean opacity and number of rows of the model, retired rows left out
 *   eogs_monitor_end_iteration   the two exponential moving averages of the progress bar, the iteration count
 *   eogs_monitor_close_interval  means of the interval, the early stopper, one record into the ring, sums cleared
 *
 * Same conventions as eogs_rast.h: plain DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status (0 ok,
 * <0 error, message via eogs_rast_last_error()), the library never allocates device memory, arguments are checked before
 * anything touches a device. Everything is asynchronous on `stream` and consists of kernel launches alone: a stream
 * capture records it. Sums are reduced in a fixed order without atomics: the same bits on every run and stream.
 *
 * `gate` (NULL = open) is the uint32[2] of eogs_step_gate (eogs_step.h): with gate[0] == 0 a call leaves every byte of the
 * state as it was, the rule eogs_step_adam follows for parameters and step counts. A replay that outgrew its workspaces and
 * is recorded again is then not counted twice.
 *
 * Sums and moving averages are float64. The reference adds fp32 `.item()` values into Python floats; a double accumulator
 * fed the same fp32 values in the same order holds the same bits.
 */
#ifndef EOGS_MONITOR_H_INCLUDED
#define EOGS_MONITOR_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOGS_MONITOR_RING 16 /* records kept; record k (1-based count of closed intervals) lives in ring[(k - 1) % 16] */

/* the six metrics held on the device, in the order of sums[] and means[]; `metric` of close_interval is one of them */
#define EOGS_MONITOR_PHOTOMETRIC 0
#define EOGS_MONITOR_L1 1
#define EOGS_MONITOR_PAN_PSNR 2
#define EOGS_MONITOR_PAN_SSIM 3
#define EOGS_MONITOR_MSI_PSNR 4
#define EOGS_MONITOR_MSI_SSIM 5
#define EOGS_MONITOR_METRICS 6

#define EOGS_MONITOR_KIND_PAN 0 /* cam.image_type == "pan" */
#define EOGS_MONITOR_KIND_MSI 1 /* "msi"                   */

#define EOGS_MONITOR_MIN 0 /* early_stopping(operator="min"): strict <  */
#define EOGS_MONITOR_MAX 1 /* "max": strict >                           */

/* What close_interval writes: 16 x 8 bytes. */
typedef struct {
  int64_t interval;     /* 1-based number of this record: intervals closed so far, this one included            */
  int64_t iteration;    /* iterations ended (eogs_monitor_end_iteration) when the interval was closed            */
  double means[EOGS_MONITOR_METRICS]; /* train_pan.py:512-519: sums over max(1, n_photo | n_pan | n_msi)         */
  double ema_loss;        /* train_pan.py:492 */
  double ema_photometric; /* train_pan.py:493-495 */
  double mean_opacity;  /* of the last observe_model (an fp32 value), 0 before the first                        */
  int64_t rows;         /* rows that are not retired at the last observe_model                                  */
  double best;          /* the stopper's best_loss after this interval                                          */
  int64_t counter;      /* its counter                                                                          */
  int64_t early_stop;   /* its flag, 0 or 1                                                                     */
  int64_t reserved;
} eogs_monitor_record;

/* The state buffer. The caller allocates eogs_monitor_state_bytes() bytes, 16-byte aligned, and resets them once. */
typedef struct {
  double sums[EOGS_MONITOR_METRICS]; /* of the open interval                                                     */
  int64_t n_photo, n_pan, n_msi;
  double ema_loss, ema_photometric;
  int64_t iteration;
  double best;
  int64_t counter, early_stop;
  int64_t intervals;    /* closed so far                                                                         */
  float last[4];        /* of the last observation: {l1, ssim, photometric, psnr}                                */
  float mean_opacity;   /* of the last observe_model                                                             */
  float reserved0;
  int64_t rows;
  int64_t reserved1;
  eogs_monitor_record latest;                 /* the newest record: what a reader copies                         */
  eogs_monitor_record ring[EOGS_MONITOR_RING];
} eogs_monitor_state;

int eogs_monitor_state_bytes(size_t* bytes);

/* One launch: every byte of the state is written. `op` is EOGS_MONITOR_MIN or _MAX (callback_utils.py:6-9). */
int eogs_monitor_reset(void* state, size_t state_bytes, int op, void* stream);

/* Workspace of observe. standalone != 0: the call evaluates the loss itself (loss_out == NULL) and the workspace holds
 * that of eogs_loss_forward as well. */
int eogs_monitor_observe_bytes(int planes, int H, int W, int standalone, size_t* bytes);

/* One observation. image, gt: `planes` contiguous H x W fp32 planes. In fp32, on the device:
 *     l1          = mean |x - y|,   ssim = mean SSIM (window 11)
 *     photometric = (1 - lambda) l1 + lambda (1 - ssim)                       utils/image_utils.py:27-28
 *     psnr        = mean over planes of 20 log10(1 / sqrt(mse_plane))         utils/image_utils.py:19-21
 * (a plane with mse 0 gives +inf, as the reference's does). Then, unless the gate is closed:
 *     sums[L1] += l1                                                          train_pan.py:424
 *     photometric_on: sums[PHOTOMETRIC] += photometric, n_photo += 1          train_pan.py:426-429
 *     sums[<kind>_PSNR] += psnr, sums[<kind>_SSIM] += ssim, n_<kind> += 1     train_pan.py:471-485
 *     last = {l1, ssim, photometric_on ? photometric : 0, psnr}
 * loss_out != NULL: the f32[3] that eogs_loss_forward wrote for these images (mode L1 | SSIM): l1 = loss_out[1] and
 * ssim = loss_out[2] are read on the device and the only pass over the images is the per-plane sum of (x - y)^2 — the
 * reference's second SSIM is not evaluated. loss_out == NULL: eogs_loss_forward (mode L1 | SSIM) runs first, into the
 * workspace. Two launches after that: the per-plane partial sums, and one workgroup that adds them in a fixed order, forms
 * the PSNR and updates the state. */
int eogs_monitor_observe(int planes, int H, int W, const float* image, const float* gt, const float* loss_out,
                         double lambda_dssim, int kind, int photometric_on, const uint32_t* gate, void* state, void* ws,
                         size_t ws_bytes, void* stream);

/* The reference's `meanopacity` and `number of gaussians` (train_pan.py:331,521,534), which it takes after a physical
 * prune: the mean of sigmoid(o) over the rows that are not retired and their number. A row whose logit is
 * <= EOGS_REG_RETIRED_BELOW (eogs_reg.h) is retired. No row left: the mean is 0. opacity f32[P]. Two launches. */
int eogs_monitor_model_bytes(int64_t P, size_t* bytes);
int eogs_monitor_observe_model(int64_t P, const float* opacity, const uint32_t* gate, void* state, void* ws, size_t ws_bytes,
                               void* stream);

/* `loss` is a device f32 scalar. ema_loss = 0.4 loss + 0.6 ema_loss in double, the same for ema_photometric with
 * last[2]; iteration += 1 (train_pan.py:492-495). One launch. */
int eogs_monitor_end_iteration(const float* loss, const uint32_t* gate, void* state, void* stream);

/* train_pan.py:512-519, 572-597 in one launch: the means; the stopper of callback_utils.py:15-44 on means[metric]
 * (0 skips the update; min improves on strict <, max on strict >; otherwise counter += 1 and counter >= patience sets the
 * flag, so a NaN metric counts as no improvement); one record into `latest` and the ring; sums and counts cleared.
 * patience < 0 switches the stopper off (use_early_stopping: False). */
int eogs_monitor_close_interval(int metric, int op, int64_t patience, const uint32_t* gate, void* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_MONITOR_H_INCLUDED */
