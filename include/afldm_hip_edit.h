/* afldm_hip_edit.h - the slot sampler's update for image-conditioned requests: img2img and RePaint inpainting in slots, on the
 * counter-based noise (libafldm_edit.so).
 *
 * A library of its own that links against libafldm_hip.so, like afldm_hip_noise.h's: the product header and library and the
 * other extensions stay exactly as they are, and only an EditSlotEngine loads this one (afldm_amd/_edit.py).  Same conventions
 * as afldm_hip.h: device pointers, stream-ordered, capturable, no allocation, int status + afldm_last_error() of libafldm_hip.so.
 *
 * The noise of a request is the stream of afldm_hip_noise.h - Philox-4x32-10, counter (g, ordinal, slot, 0), key from the
 * request's seed, Box-Muller - and the stream slot j is the kind's noise slot j, in the order Schedule.draws uses:
 *   "seeded_repaint"  z_k = slot 0, z_u = slot 1, z_b = slot 2, all at the row's ordinal (its place in the request's own schedule)
 *   "seeded_sdedit"   z_u = slot 0 at the row's ordinal; the run's ONE fixed noise z = slot 1 at ordinal 0
 * A noise whose coefficient is exactly 0 is not generated (z = 0): k1, c, u1 for "seeded_repaint"; c, k1 for "seeded_sdedit".
 *
 * The updates, in exactly these float operations - every product rounded, the sums left to right, no fused multiply-add;
 * clamp keeps a NaN a NaN:
 *   kind 3, "seeded_sdedit", row (p, q, lo, hi, a, b, c, k0, k1, thr, 0, 0); o = cond, m = cmask (the change map):
 *     t = rn(p x) + rn(q eps);  x0 = clamp(t, lo, hi);  xp = (rn(a x0) + rn(b eps)) + rn(c z_u);  held = rn(k0 o) + rn(k1 z)
 *     x_out = (m <= thr) ? held : xp    - a select: nothing of x, eps or z_u reaches a held element; a NaN in m compares false
 *   kind 4, "seeded_repaint", row (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0); kn = cond, m = cmask (the keep mask):
 *     x0 as above;  unknown = (rn(a x0) + rn(b eps)) + rn(c z_u);  knownp = rn(k0 kn) + rn(k1 z_k)
 *     y = rn(m knownp) + rn(rn(1 - m) unknown);  x_out = rn(u0 y) + rn(u1 z_b)
 */
#ifndef AFLDM_HIP_EDIT_H
#define AFLDM_HIP_EDIT_H

#include "afldm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* afldm_slot_step_edit - afldm_slot_step_seeded (afldm_hip_noise.h) on rows of 12 floats (row_coef fp32 [R][12]), plus the kind
 * codes 3 and 4 above.  x: NCHW fp32 [B][C][H][W], updated in place; eps: NHWC dtype; hist: fp32 [2][B][C][H][W]; cond: fp32
 * [B][C][H][W], slot b's original latents (kind 3) or known latents (kind 4); cmask: fp32 [B][1][H][W], its change map or keep
 * mask; row_kind, row_ord: int32 [R]; pos, active: int32 [B]; seeds: int64 [B].  Kinds 0, 1 and 2 read the first 8 floats of the
 * row and give afldm_slot_step_seeded's bits, in x and in both history planes.  Kinds 3 and 4 neither read nor write hist.  An
 * inactive slot, a pos outside [0, R) and any other kind code leave the slot's x and history untouched.  16-byte accesses when
 * H W % 4 == 0 and x, hist, cond and cmask are 16-byte aligned, scalar ones otherwise; the values are the same. */
int afldm_slot_step_edit(float* x, const void* eps, float* hist, const float* cond, const float* cmask, const float* row_coef,
                         const int* row_kind, const int* row_ord, const int* pos, const int* active, const long long* seeds, int B,
                         int R, int C, int H, int W, int dtype, afldm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AFLDM_HIP_EDIT_H */
