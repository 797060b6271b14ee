/* afldm_hip_noise.h - counter-based device noise and the sampler updates that use it (libafldm_noise.so).
 *
 * A library of its own that links against libafldm_hip.so, like afldm_hip_slots.h's: the product header and library stay exactly
 * as they are, and only the seeded samplers load this one (afldm_amd/_noise.py).  Same conventions as afldm_hip.h: device
 * pointers, stream-ordered, capturable, int status + afldm_last_error() of libafldm_hip.so.
 *
 * The noise stream.  Philox-4x32-10 as in Random123 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85, ten rounds), then Box-Muller:
 *   key      (seed & 0xffffffff, seed >> 32) of the sample's seed, 0 <= seed < 2^63
 *   counter  (g, ordinal, slot, 0): g = i >> 2 of element i in the sample's own flat [C][H][W] order, ordinal the step within
 *            the sample's own schedule (0 for its first evaluation), slot the noise slot (0 here; afldm_hip_edit.h uses 1 and 2)
 *   uniforms u_j = ((r_j >> 9) + 0.5) 2^-23, exact in fp32 and in [2^-24, 1 - 2^-24]
 *   normals  (z0, z1) = sqrt(-2 ln u0) (cos 2 pi u1, sin 2 pi u1), (z2, z3) likewise from (u2, u3); element 4 g + k gets z_k;
 *            |z| <= 5.77
 * A value depends on nothing else: not on the batch position, the neighbours, the vector width or the grouping into launches.
 *
 * The update ("seeded" rows: the "sde" row (p, q, lo, hi, a, b, d, c) of afldm_sde_step), in exactly these float operations -
 * every product rounded, the sums left to right, no fused multiply-add:
 *   t = rn(p x) + rn(q eps);  x0 = clamp(t, lo, hi) (a NaN stays a NaN);  x_out = ((rn(a x) + rn(b x0)) + rn(d eps)) + rn(c z)
 * A row whose c is 0 generates nothing: z = 0.
 */
#ifndef AFLDM_HIP_NOISE_H
#define AFLDM_HIP_NOISE_H

#include "afldm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* afldm_philox_bits - the raw Philox words: out uint32 [B][groups][4] = Philox-4x32-10 of the counter (g0 + g, ordinal, slot, c3)
 * - the low 32 bits of each long long - under the key of seeds[b] (int64 [B]).  For known-answer tests. */
int afldm_philox_bits(unsigned int* out, const long long* seeds, long long g0, long long ordinal, long long slot, long long c3,
                      int B, long long groups, afldm_stream_t stream);

/* afldm_counter_noise - the stream above, materialised: out fp32 NCHW [B][C][H][W], sample b from seeds[b] (int64 [B]) at the
 * ordinal ordinals[b] (int32 [B]) and noise slot `slot`.  16-byte stores when C H W % 4 == 0 and out is 16-byte aligned, scalar
 * ones otherwise; the values are the same. */
int afldm_counter_noise(float* out, const long long* seeds, const int* ordinals, int slot, int B, int C, int H, int W,
                        afldm_stream_t stream);

/* afldm_seeded_step - afldm_sde_step with the noise made in registers: row *step_idx of coef [steps][8], the ordinal *step_idx,
 * noise slot 0, sample b from seeds[b] (int64 [B]).  x, x_out: NCHW fp32 (may alias); eps: NHWC dtype.  A negative *step_idx
 * writes nothing.  advance != 0: *step_idx += 1 afterwards. */
int afldm_seeded_step(const float* x, const void* eps, const long long* seeds, float* x_out, const float* coef, int* step_idx,
                      int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream);

/* afldm_slot_step_seeded - afldm_slot_step_kinds (afldm_hip_slots.h) plus kind code 2, the "seeded" row: the update above with
 * the ordinal row_ord[pos[b]] (int32 [R]: the row's place in its own schedule) and the seed seeds[b] (int64 [B]).  Kinds 0 and 1
 * give afldm_slot_step_kinds' bits, in x and in both history planes.  A kind-2 slot neither reads nor writes its history
 * planes.  An inactive slot, a pos outside [0, R) and any other kind code leave the slot's x and history untouched. */
int afldm_slot_step_seeded(float* x, const void* eps, float* hist, const float* row_coef, const int* row_kind, const int* row_ord,
                           const int* pos, const int* active, const long long* seeds, int B, int R, int C, int H, int W, int dtype,
                           afldm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AFLDM_HIP_NOISE_H */
