/* afldm_hip_slots.h - the slot sampler's update for mixed solvers (libafldm_slots.so).
 *
 * An extension of the slot sampler of afldm_hip.h (afldm_slot_select / afldm_slot_step / afldm_slot_exchange), in a library of
 * its own that links against libafldm_hip.so: the product header and library stay exactly as they are, and only an engine
 * built with kinds other than ("ddim",) loads this one (afldm_amd/_slots.py).  Same conventions as afldm_hip.h: device
 * pointers, stream-ordered, capturable, int status + afldm_last_error() of libafldm_hip.so.
 */
#ifndef AFLDM_HIP_SLOTS_H
#define AFLDM_HIP_SLOTS_H

#include "afldm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* afldm_slot_step_kinds - afldm_slot_step for a row table that holds "ddim" AND "dpm" rows: row_coef [R][8], row_kind [R] int32
 * (0: the "ddim" row in the first four floats, 1: the "dpm" row (p, q, a, b0, b1, b2, 0, 0)); hist fp32 [2][B][C][H][W], h1 then
 * h2, slot b's planes at b C H W inside each half.  For every element of a slot with active[b] != 0 and row r = pos[b]:
 *   kind 0:  afldm_slot_step's update; the slot's history planes are neither read nor written
 *   kind 1:  m0 = p x + q eps;  x = a x + b0 m0 + b1 h1 + b2 h2;  h2 <- h1, h1 <- m0  in afldm_dpm_step's float operations and
 *            order (a slot gives afldm_dpm_step's bits for the same row, in x and in both planes).  A plane whose coefficient
 *            is exactly 0 does not enter the sum - zeros do, so NaN left in it by an earlier occupant reaches no result - and
 *            h2 is then not read at all; h1 is still read for the shift.
 * An inactive slot, a pos outside [0, R) and any other kind code leave the slot's x and history untouched.
 * x: NCHW fp32 [B,C,H,W], in place; eps: NHWC dtype. */
int afldm_slot_step_kinds(float* x, const void* eps, float* hist, const float* row_coef, const int* row_kind, const int* pos,
                          const int* active, int B, int R, int C, int H, int W, int dtype, afldm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AFLDM_HIP_SLOTS_H */
