/*
 * eogs_step.h — C-ABI of the optimizer step INSIDE a recorded graph: an Adam step whose step counts and learning rates
 * live on the device, and the gate that keeps a replay whose forwards outgrew their list workspaces from updating
 * anything.
 *
 *   eogs_step_gate    one single-wave launch over the count words of up to 16 deferred-count forwards: did every one of them
 *                     fit the capacity it was rendered with? (what eogs_rast_mirror_counts + eogs_rast_capacity_token tell
 *                     the host after the replay, decided on the device inside it)
 *   eogs_step_adam    eogs_adam_step (eogs_optim.h) with t and lr read from device scalars: a one-workgroup prologue forms the
 *                     bias corrections in double, the element kernel — the arithmetic of eogs_adam_step, bit for bit given
 *                     equal fp32 scalars — reads them from a small table
 *
 * Same conventions as eogs_optim.h: DEVICE pointers + sizes, `void* stream` is a hipStream_t, int status (0 ok, <0 error,
 * message via eogs_rast_last_error()), no device allocation inside the library, arguments are checked before anything is
 * queued. Everything is asynchronous on `stream` and consists of kernel launches alone: a stream capture records it.
 */
#ifndef EOGS_STEP_H_INCLUDED
#define EOGS_STEP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOGS_STEP_MAX_FORWARDS 16
#define EOGS_STEP_MAX_TENSORS 16

/* ---- gate ----------------------------------------------------------------------------------------------------------
 * One forward queued with EOGS_FLAG_DEFER_COUNTS: its geometry workspace (as given to eogs_rast_forward_prepare), its
 * Gaussian count and the capacity token its eogs_rast_forward_render was called with. */
typedef struct {
  const void* geom;
  size_t geom_bytes;
  int P;
  int64_t capacity;
} eogs_step_forward;

/* `fw` is a HOST array of n <= EOGS_STEP_MAX_FORWARDS descriptors (copied into the kernel arguments). The launch reads each
 * forward's count words from its geometry workspace — the words eogs_rast_mirror_counts copies — and writes
 *     gate[0] = 1 when every forward fits its capacity and has no error bit (altitude > 200) set, else 0
 *     gate[1] = bit i set when forward i of this call did not
 * A forward fits when its record slots (tile, Gaussian) are <= the token's and its list entries (32-px block, Gaussian)
 * are <= the token's: the rule of eogs_rast_capacity_token's `*fits`, and of the device when it decides whether to build
 * the forward's lists. A forward with nothing listed always fits. n == 0 opens the gate.
 * accumulate != 0: gate[0] &= ..., gate[1] |= ... on what `gate` already holds (more than 16 forwards in a step: the mask
 * then ORs the calls position by position).
 * Queue it after the eogs_rast_forward_prepare of every forward it names, on a stream ordered after them. */
int eogs_step_gate(int n, const eogs_step_forward* fw, int accumulate, uint32_t* gate, void* stream);

/* ---- Adam ----------------------------------------------------------------------------------------------------------
 * One parameter tensor of a step. `lr` and `step` are DEVICE fp32 scalars; `step` is what
 * torch.optim.Adam(capturable=True) keeps in state["step"]: the number of updates taken so far, incremented by the step
 * itself. Two descriptors of one call must not share a `step`.
 * After the update an element < retire_below is stored as EOGS_STEP_RETIRED_LOGIT: the per-iteration transparent prune
 * in its deferred form (eogs2_amd.optim.retire_rows after optimizer.step(); train_pan.py:664-677). -INFINITY switches it
 * off; a NaN element is never retired. */
#define EOGS_STEP_RETIRED_LOGIT (-1.0e30f)
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  const float* lr;
  float* step;
  float retire_below;
} eogs_step_adam_tensor;

/* What the prologue leaves in `ws` for descriptor i of the call (numel == 0 included): ws is an array of n of these. */
typedef struct {
  float lr;       /* *tensor.lr                                                        */
  float inv_bc1;  /* (float)(1 / (1 - beta1^t)),    formed in double, t = *step + 1    */
  float sqrt_bc2; /* (float)sqrt(1 - beta2^t),      formed in double                   */
  float skip;     /* 1 when the gate is closed: the element kernel leaves the tensor alone, else 0 */
} eogs_step_adam_scalars;

/* bytes = n * sizeof(eogs_step_adam_scalars). */
int eogs_step_adam_bytes(int n, size_t* bytes);

/* `tensors` is a HOST array of n <= EOGS_STEP_MAX_TENSORS descriptors (copied into the kernel arguments). Two launches:
 *   1. one workgroup; per tensor, one lane: when `gate` is NULL or gate[0] != 0, t = *step + 1 is stored back to *step and
 *      {lr, 1 / (1 - beta1^t), sqrt(1 - beta2^t), 0} go to ws[i] — the bias corrections in double from the double betas, as
 *      eogs_adam_step forms them on the host, rounded to fp32 once. With the gate closed ws[i].skip = 1 and *step keeps
 *      its bits.
 *   2. the element kernel of eogs_adam_step with its four scalars read from ws; a tensor marked skip is not touched: no
 *      parameter, no moment, no store.
 * `ws` (ws_bytes >= eogs_step_adam_bytes(n), 16-byte aligned) belongs to this call until the work has run; a recorded
 * graph keeps pointing into it. A tensor with numel == 0 takes part in the prologue only (its step advances, as
 * torch's does; its four array pointers may be NULL); `lr` and `step` are never NULL. */
int eogs_step_adam(int n, const eogs_step_adam_tensor* tensors, double beta1, double beta2, double eps, const uint32_t* gate,
                   void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOGS_STEP_H_INCLUDED */
