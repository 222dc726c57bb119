/*
 * eogs_views.h — C-ABI of the device-side view bank: the per-view data of a training run (ground truth, matrices, the
 * camera's parameters, their Adam moments and step counts) sit in device tables of one row per view, an order table and a
 * cursor on the device say which view is current, and
 *
 *   eogs_views_load     one launch: the current view's rows go into the fixed working tensors a recorded step points at
 *   eogs_views_store    one gated launch: the working tensors the step updated go back into the current view's rows
 *   eogs_views_advance  one gated single-thread launch: the cursor moves on
 *
 * so that a recorded step (eogs2_amd.graph.GraphedStep) trains another view on every replay with no host work in between:
 * train_pan.py:252-257 pops a view per iteration, :135-138 keeps one optimizer group per camera. The kernels only move
 * bits: 4-byte words, no arithmetic, NaN payloads included.
 *
 * Same conventions as eogs_step.h: DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status (0 ok, <0 error,
 * message via eogs_rast_last_error()), no device allocation inside the library, arguments are checked before anything is
 * queued. Everything is asynchronous on `stream` and consists of kernel launches alone: a stream capture records it.
 * Nothing here reads the rasterizer's state.
 */
#ifndef EOGS_VIEWS_H_INCLUDED
#define EOGS_VIEWS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOGS_VIEWS_MAX_SLOTS 32
#define EOGS_VIEWS_LOAD 1u  /* row -> working, by eogs_views_load  */
#define EOGS_VIEWS_STORE 2u /* working -> row, by eogs_views_store */

/* One per-view tensor. `table` holds n_views rows, row v at table + v * row_stride; the first row_bytes bytes of a row are
 * the payload. row_stride is a multiple of 16 and >= row_bytes, row_bytes a multiple of 4; table and working are 4-byte
 * aligned. A chunk of a slot moves as 16-byte accesses when table, working and the chunk's offset are all 16-byte
 * aligned, else as dwords. row_bytes == 0: the slot takes no part (its pointers may be NULL). */
typedef struct {
  void* table;
  void* working;
  size_t row_stride;
  size_t row_bytes;
  uint32_t flags; /* EOGS_VIEWS_LOAD | EOGS_VIEWS_STORE, at least one */
} eogs_views_slot;

/* Which view is current: order[cursor mod order_len] (cursor >= 0). `current` is where eogs_views_load leaves that entry
 * and where eogs_views_store reads it. An entry < 0 or >= n_views is never turned into an address: load writes
 * current = -1 and touches no slot, store and advance do nothing. */
typedef struct {
  const int32_t* order;
  int64_t order_len;
  int64_t* cursor;
  int32_t* current;
  int32_t n_views;
} eogs_views_schedule;

/* The bytes of a slot one workgroup moves: a slot of row_bytes takes ceil(row_bytes / *bytes) workgroups. */
int eogs_views_wg_bytes(size_t* bytes);

/* `slots` is a HOST array of n <= EOGS_VIEWS_MAX_SLOTS descriptors (copied into the kernel arguments; more slots are the
 * caller's loop). One launch: current = order[cursor mod order_len] (or -1), and row `current` of every slot with
 * EOGS_VIEWS_LOAD goes into its working tensor. n == 0 queues nothing. */
int eogs_views_load(int n, const eogs_views_slot* slots, const eogs_views_schedule* schedule, void* stream);

/* One launch: with gate == NULL or gate[0] != 0 the working tensor of every slot with EOGS_VIEWS_STORE goes into row
 * `current` (as the last eogs_views_load over this schedule left it); with the gate closed nothing is written. `gate` is
 * the uint32[2] of eogs_step_gate (eogs_step.h). n == 0 queues nothing. */
int eogs_views_store(int n, const eogs_views_slot* slots, const eogs_views_schedule* schedule, const uint32_t* gate, void* stream);

/* One single-thread launch: cursor += 1 under the same gate rule; nothing when the current order entry is out of range.
 * A launch of its own, so no launch has one workgroup write the cursor while others read it. */
int eogs_views_advance(const eogs_views_schedule* schedule, const uint32_t* gate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_VIEWS_H_INCLUDED */
