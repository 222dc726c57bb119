/*
 * eogs_report.h — C-ABI of the end of a training run and of the inference side: the global colour alignment before the
 * final save (utils/save_utils.py:10-33), the train -> test colour-correction converters (utils/convert_color_correction.py),
 * the per-kind L1 / PSNR sums of training_report (train_pan.py:838-1025) and the packing of a view's products into file layout
 * (render_pan.py:94-476, render_video.py:138-164).
 *
 *   eogs_report_normalize_rows   every Gaussian's colour through the reference camera's correction, in place
 *   eogs_report_recompose        every camera's correction recomposed against it, in place, in one wave
 *   eogs_report_cc_to_test       the reference camera's or the averaged correction into the test cameras
 *   eogs_report_metrics_*        per-view L1 and PSNR into a device table of float64 sums per camera kind
 *   eogs_report_pack             up to 16 images into one buffer: HWC float, or 8-bit by one of two rounding rules
 *
 * Same conventions as eogs_views.h: plain DEVICE pointers + sizes, descriptor arrays on the HOST (copied into the kernel
 * arguments), `void* stream` is a hipStream_t, int status (0 ok, <0 error, message via eogs_rast_last_error()), the library
 * never allocates device memory, arguments are checked before anything is queued. Everything is kernel launches on `stream`
 * alone: a stream capture records it. Every sum is reduced per workgroup and then in a fixed order (no atomics): results
 * are bitwise reproducible. The library is built with -ffp-contract=off: every product and sum below is rounded on its own.
 */
#ifndef EOGS_REPORT_H_INCLUDED
#define EOGS_REPORT_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOGS_REPORT_MAX_CAMERAS 64 /* per call of recompose / cc_to_test: one lane of one wave each */
#define EOGS_REPORT_MAX_CC_ELEMS 16 /* elements of a camera's weight plus its bias (3 x 3 + 3, or 1 + 1) */
#define EOGS_REPORT_MAX_ITEMS 16
#define EOGS_REPORT_MAX_CHANNELS 4      /* metrics */
#define EOGS_REPORT_PACK_MAX_CHANNELS 5 /* pack */

/* a camera's colour correction: weight f32[w_elems] (Conv2d(3,3,1): row-major 3 x 3), bias f32[b_elems] */
typedef struct {
  float* weight;
  float* bias;
} eogs_report_camera;

/* In place over f_dc f32[P][3] (the [P, 1, 3] of _features_dc), per element in fp32:
 *   f' = ((A1 . (f C0 + 0.5) + b1) - 0.5) / C0         C0 = 0.28209479177387814 as fp32 (utils/sh_utils.py)
 * the dot product as (A_i0 c_0 + A_i1 c_1) + A_i2 c_2. A1 f32[9] row-major and b1 f32[3] are read from device memory: nothing
 * waits. One pass, 16-byte accesses where f_dc is 16-byte aligned. A1 and b1 must not overlap f_dc. */
int eogs_report_normalize_rows(int64_t P, float* f_dc, const float* A1, const float* b1, void* stream);

/* One launch of one wave for n <= EOGS_REPORT_MAX_CAMERAS cameras with 3 x 3 weights and 3-element biases, lane i camera i:
 *   Ai' = Ai . A1^-1        bi' = bi - Ai' . b1                                  (save_utils.py:26-33)
 * in double over the fp32 inputs, A1^-1 = adj(A1) / det(A1) in closed form, each of the 12 results rounded to fp32 once
 * (csrc/report_cc.h). det(A1) zero or not finite: NaN in all 12 (the reference's torch.linalg.inv raises; a launch cannot).
 * Written into the cameras' own storage. ref_weight / ref_bias may be (and usually are) one of the cameras' own tensors:
 * every lane reads them before any lane writes, so every camera, the reference camera included, is recomposed against the
 * ORIGINAL A1 and b1, as in the reference. Apart from that no two tensors may overlap. */
int eogs_report_recompose(int n, const eogs_report_camera* cameras, const float* ref_weight, const float* ref_bias, void* stream);

#define EOGS_REPORT_CC_REF 0     /* copy train[0] (the reference camera, found by the caller) bit for bit */
#define EOGS_REPORT_CC_AVERAGE 1 /* fp32: a zero, += every train camera in order, / (float)n_train */
/* One launch: the result into every test camera's own weight f32[w_elems] and bias f32[b_elems];
 * w_elems + b_elems <= EOGS_REPORT_MAX_CC_ELEMS, both counts at most EOGS_REPORT_MAX_CAMERAS. No test tensor may overlap a
 * train tensor. n_test == 0: nothing is queued. */
int eogs_report_cc_to_test(int mode, int n_train, const eogs_report_camera* train, int n_test, const eogs_report_camera* test,
                           int w_elems, int b_elems, void* stream);

#define EOGS_REPORT_KIND_PAN 0
#define EOGS_REPORT_KIND_MSI 1
/* The device table of an accumulator, 64 bytes, 8-byte aligned. */
typedef struct {
  double l1[2];     /* per kind: the sum over the views of the per-view L1, each rounded to fp32 before it is added */
  double psnr[2];   /* ... of the per-view mean PSNR */
  int64_t views[2]; /* ... the number of views added */
  float last_l1;    /* the per-view values of the last view that was added */
  float last_psnr;
  int64_t reserved;
} eogs_report_table;

/* Workspace of eogs_report_metrics_accumulate (the per-workgroup partial sums), the same for every shape. */
int eogs_report_metrics_bytes(size_t* bytes);
/* table <- zeros: one launch. */
int eogs_report_metrics_reset(eogs_report_table* table, void* stream);
/* What training_report does per camera (train_pan.py:917,942-943) for image, gt f32[C][H][W], 1 <= C <= 4:
 *   g    = clamp(gt, 0, 1)                                  (a NaN stays a NaN)
 *   L1   = mean over all elements of |image - g|
 *   PSNR = mean over the channels of 20 log10(1 / sqrt(mean over the plane of (image - g)^2))
 * Differences, squares and sums in double over the fp32 inputs; L1 and PSNR are each rounded to fp32 once, then
 * table.l1[kind] += L1, table.psnr[kind] += PSNR in double, table.views[kind] += 1. A plane whose error is 0 gives +inf, a NaN
 * pixel NaN. gate: NULL, or u32[2] as eogs_step_gate writes it; gate[0] == 0 leaves every word of the table as it was.
 * Two launches: partial sums per workgroup, then one workgroup that adds them in index order. */
int eogs_report_metrics_accumulate(int C, int H, int W, const float* image, const float* gt, int kind, eogs_report_table* table,
                                   const uint32_t* gate, void* ws, size_t ws_bytes, void* stream);

#define EOGS_REPORT_FLOAT_HWC 0 /* f32: the bytes of permute(1, 2, 0).contiguous() */
#define EOGS_REPORT_U8_ROUND 1  /* u8: trunc(clamp(x 255 + 0.5, 0, 255)) — torchvision's save_image */
#define EOGS_REPORT_U8_TRUNC 2  /* u8: trunc(clamp(x, 0, 1) 255) — clip(0, 1).mul(255.0) and the cast (render_video.py:162) */
#define EOGS_REPORT_REVERSE 1u   /* flags: output channel k is source channel C - 1 - k (RGB -> BGR) */
#define EOGS_REPORT_REPLICATE 2u /* a one-channel source written three times */
#define EOGS_REPORT_PREMAP 4u    /* x <- (x - lo) / d first, in fp32 */
typedef struct {
  const float* src;    /* f32[C][H][W] ([H][W]: C = 1) */
  int32_t C, H, W;     /* 1 <= C <= EOGS_REPORT_PACK_MAX_CHANNELS */
  int32_t mode;        /* EOGS_REPORT_FLOAT_HWC, _U8_ROUND, _U8_TRUNC */
  uint64_t dst_offset; /* bytes from dst to the item's first pixel */
  uint64_t dst_pitch;  /* bytes from one row of the item to the next: at least W x channels written x element size */
  uint32_t flags;
  float lo, d;
} eogs_report_item;

/* One launch for n <= EOGS_REPORT_MAX_ITEMS items, a lane per pixel. Pixel (r, c) of an item goes to
 * dst + dst_offset + r dst_pitch + c (channels x element size), its channels side by side; the offset and the pitch let two
 * items write side by side into one frame. In both 8-bit modes a NaN gives 0, -0 gives 0, +inf 255 and -inf 0. FLOAT_HWC without
 * PREMAP moves bits. A FLOAT_HWC item's offset and pitch are multiples of 4 and dst is 4-byte aligned. Every item's
 * rectangle must lie inside dst_bytes, and no source may overlap dst; bytes outside the rectangles are not touched. That
 * two items' rectangles do not overlap each other is the caller's. */
int eogs_report_pack(int n, const eogs_report_item* items, void* dst, size_t dst_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_REPORT_H_INCLUDED */
