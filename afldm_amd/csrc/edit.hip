// edit.hip — the slot sampler's update for image-conditioned requests (libafldm_edit.so, include/afldm_hip_edit.h):
//   afldm_slot_step_edit  afldm_slot_step_seeded (noise.hip) on 12-wide rows, plus kind code 3, "seeded_sdedit" - img2img with a
//                         change map, afldm_sdedit_step's select - and kind code 4, "seeded_repaint" - RePaint's blend and jump,
//                         afldm_repaint_step's.  A slot's conditioning image and mask are its own planes of cond / cmask, and all
//                         of its noise is the counter stream of philox.hpp at the ordinal row_ord[pos[b]]: for kind 4 z_k, z_u, z_b
//                         are the noise slots 0, 1, 2; for kind 3 z_u is slot 0 and the run's one fixed noise z is slot 1 at
//                         ordinal 0.  A noise whose coefficient is exactly 0 is not generated: z = 0.
// Kinds 0, 1 and 2 run the code of k_slot_step_seeded on the first 8 floats of the row (slot_update, slot_dpm_*, seeded_update of
// slot_common.hpp / seeded_common.hpp) and give its bits.  The two new updates are edit_sdedit / edit_repaint below, written once
// with contraction off and no fma, so a float32 restatement in the stated order gives their bits (tests/edit_oracle.py).
// Layout as noise.hip: one grid row per slot; a thread owns 4 consecutive elements of one plane (one Philox call per noise,
// 16-byte loads of x / cond / cmask and stores of x) or, in the scalar form, one element - the values do not depend on the form;
// grid-stride over the slot's elements.  Each thread reads and writes its own indices only; every table index read from device
// memory is range-checked before use.  Per thread at most three Philox calls (thirty rounds, six log / sqrt, six sincospi)
// against one 16-byte store and three 16-byte loads: HBM-bound.
// Resources (gfx950, -O3, the compiler's resource report; no scratch, no LDS, no AGPRs in any of them):
//   k_slot_step_edit 54 VGPRs in the 16-byte form (fp32 and bf16 eps), 28 in the scalar form;  8 waves per SIMD in all four
#include "seeded_common.hpp"

#include "../../include/afldm_hip_edit.h"

namespace afldm {

namespace {

constexpr int KIND_SDEDIT = 3, KIND_REPAINT = 4;      // row_kind codes (EditSlotTable.KIND_CODES in afldm_amd/engine.py)
constexpr int EDIT_ROW = 12;                          // floats per row

struct sdedit_row {
  float p, q, lo, hi, a, b, c, k0, k1, thr;
};

struct repaint_row {
  float p, q, lo, hi, a, b, c, k0, k1, u0, u1;
};

// The "seeded_sdedit" update, the "sdedit" row (p, q, lo, hi, a, b, c, k0, k1, thr, 0, 0) - every product rounded, sums left to
// right, no fma:
//   t = rn(p x) + rn(q e);  x0 = clamp_nan(t, lo, hi);  xp = (rn(a x0) + rn(b e)) + rn(c z_u);  held = rn(k0 o) + rn(k1 z)
//   out = (m <= thr) ? held : xp      a SELECT: nothing of x, e or z_u reaches a held element; a NaN in m compares false
__device__ __forceinline__ float edit_sdedit(float x, float e, float o, float m, float z, float zu, const sdedit_row& r) {
#pragma clang fp contract(off)
  const float px = r.p * x, qe = r.q * e;
  const float t = px + qe;
  const float x0 = clamp_nan(t, r.lo, r.hi);
  const float ax0 = r.a * x0, be = r.b * e, cz = r.c * zu;
  const float xp = (ax0 + be) + cz;
  const float k0o = r.k0 * o, k1z = r.k1 * z;
  const float held = k0o + k1z;
  return m <= r.thr ? held : xp;
}

// The "seeded_repaint" update, the "repaint" row (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0), likewise:
//   x0 as above;  unknown = (rn(a x0) + rn(b e)) + rn(c z_u);  knownp = rn(k0 kn) + rn(k1 z_k)
//   y = rn(m knownp) + rn(rn(1 - m) unknown);  out = rn(u0 y) + rn(u1 z_b)
__device__ __forceinline__ float edit_repaint(float x, float e, float kn, float m, float zk, float zu, float zb,
                                              const repaint_row& r) {
#pragma clang fp contract(off)
  const float px = r.p * x, qe = r.q * e;
  const float t = px + qe;
  const float x0 = clamp_nan(t, r.lo, r.hi);
  const float ax0 = r.a * x0, be = r.b * e, cz = r.c * zu;
  const float unknown = (ax0 + be) + cz;
  const float k0k = r.k0 * kn, k1z = r.k1 * zk;
  const float knownp = k0k + k1z;
  const float om = 1.0f - m;
  const float mk = m * knownp, ou = om * unknown;
  const float y = mk + ou;
  const float u0y = r.u0 * y, u1z = r.u1 * zb;
  return u0y + u1z;
}

}  // namespace

// k_slot_step_seeded (noise.hip) on 12-wide rows, with kinds 3 and 4.  x NCHW fp32 [B, C, HW], in place; eps NHWC T; hist fp32
// [2, B, C, HW]; cond fp32 [B, C, HW]; cmask fp32 [B, 1, HW].  V = 4 needs HW % 4 == 0 and 16-byte aligned x, hist, cond, cmask.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_slot_step_edit(float* x, const T* __restrict__ eps, float* hist,
                                                        const float* __restrict__ cond, const float* __restrict__ cmask,
                                                        const float* __restrict__ row_coef, const int* __restrict__ row_kind,
                                                        const int* __restrict__ row_ord, const int* __restrict__ pos,
                                                        const int* __restrict__ active, const long long* __restrict__ seeds,
                                                        int B, int R, int C, int HW) {
  const int b = blockIdx.y;
  if (!active[b]) return;
  const int s = pos[b];
  if (s < 0 || s >= R) return;
  const int kind = row_kind[s];
  if (kind < KIND_DDIM || kind > KIND_REPAINT) return;
  const float* r = row_coef + EDIT_ROW * (size_t)s;
  const int n = C * HW;                  // one slot
  float* xb = x + (size_t)b * n;
  const T* eb = eps + (size_t)b * n;
  if (kind == KIND_DDIM) {
    const float sa_t = r[0], sb_t = r[1], sa_p = r[2], sb_p = r[3];
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n / V; g += gridDim.x * blockDim.x) {
      const int i = g * V;
      const int pix = i % HW, ch = i / HW;
      const T* ep = eb + (size_t)pix * C + ch;
      vecf<V> xv = ld<V>(xb + i);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        xv.v[k] = slot_update(xv.v[k], to_f32(ep[(size_t)k * C]), sa_t, sb_t, sa_p, sb_p);
      }
      st<V>(xb + i, xv);
    }
    return;
  }
  if (kind == KIND_SEEDED) {
    const sde_row row{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
    const bool gen = row.c != 0.0f;
    const long long seed = gen ? seeds[b] : 0;
    const uint32_t ordinal = (uint32_t)row_ord[s];
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n / V; g += gridDim.x * blockDim.x) {
      const int i = g * V;
      const int pix = i % HW, ch = i / HW;
      const T* ep = eb + (size_t)pix * C + ch;
      vecf<V> xv = ld<V>(xb + i);
      const vecf<V> z = seeded_z<V>(gen, seed, (uint32_t)i, ordinal, 0u);
#pragma unroll
      for (int k = 0; k < V; ++k) xv.v[k] = seeded_update(xv.v[k], to_f32(ep[(size_t)k * C]), z.v[k], row);
      st<V>(xb + i, xv);
    }
    return;
  }
  if (kind == KIND_SDEDIT) {
    const sdedit_row row{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9]};
    const bool has_u = row.c != 0.0f, has_z = row.k1 != 0.0f;
    const long long seed = (has_u || has_z) ? seeds[b] : 0;
    const uint32_t ordinal = (uint32_t)row_ord[s];
    const float* ob = cond + (size_t)b * n;
    const float* mb = cmask + (size_t)b * HW;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n / V; g += gridDim.x * blockDim.x) {
      const int i = g * V;
      const int pix = i % HW, ch = i / HW;
      const T* ep = eb + (size_t)pix * C + ch;
      vecf<V> xv = ld<V>(xb + i);
      const vecf<V> ov = ld<V>(ob + i), mv = ld<V>(mb + pix);
      const vecf<V> zu = seeded_z<V>(has_u, seed, (uint32_t)i, ordinal, 0u);
      const vecf<V> z = seeded_z<V>(has_z, seed, (uint32_t)i, 0u, 1u);      // the run's one noise: ordinal 0, slot 1
#pragma unroll
      for (int k = 0; k < V; ++k)
        xv.v[k] = edit_sdedit(xv.v[k], to_f32(ep[(size_t)k * C]), ov.v[k], mv.v[k], z.v[k], zu.v[k], row);
      st<V>(xb + i, xv);
    }
    return;
  }
  if (kind == KIND_REPAINT) {
    const repaint_row row{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10]};
    const bool has_k = row.k1 != 0.0f, has_u = row.c != 0.0f, has_b = row.u1 != 0.0f;
    const long long seed = (has_k || has_u || has_b) ? seeds[b] : 0;
    const uint32_t ordinal = (uint32_t)row_ord[s];
    const float* kb = cond + (size_t)b * n;
    const float* mb = cmask + (size_t)b * HW;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n / V; g += gridDim.x * blockDim.x) {
      const int i = g * V;
      const int pix = i % HW, ch = i / HW;
      const T* ep = eb + (size_t)pix * C + ch;
      vecf<V> xv = ld<V>(xb + i);
      const vecf<V> kv = ld<V>(kb + i), mv = ld<V>(mb + pix);
      const vecf<V> zk = seeded_z<V>(has_k, seed, (uint32_t)i, ordinal, 0u);
      const vecf<V> zu = seeded_z<V>(has_u, seed, (uint32_t)i, ordinal, 1u);
      const vecf<V> zb = seeded_z<V>(has_b, seed, (uint32_t)i, ordinal, 2u);
#pragma unroll
      for (int k = 0; k < V; ++k)
        xv.v[k] = edit_repaint(xv.v[k], to_f32(ep[(size_t)k * C]), kv.v[k], mv.v[k], zk.v[k], zu.v[k], zb.v[k], row);
      st<V>(xb + i, xv);
    }
    return;
  }
  const dpm_coef c{r[0], r[1], r[2], r[3], r[4], r[5]};
  const bool use1 = c.b1 != 0.0f, use2 = c.b2 != 0.0f;
  float* h1 = hist + (size_t)b * n;
  float* h2 = h1 + (size_t)B * n;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n / V; g += gridDim.x * blockDim.x) {
    const int i = g * V;
    const int pix = i % HW, ch = i / HW;
    const T* ep = eb + (size_t)pix * C + ch;
    const vecf<V> xv = ld<V>(xb + i), a1 = ld<V>(h1 + i), a2 = ld_if<V>(use2, h2 + i);
    vecf<V> out, m;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      m.v[k] = slot_dpm_m0<V>(k, xv.v[k], to_f32(ep[(size_t)k * C]), c);
      out.v[k] = slot_dpm_out<V>(xv.v[k], m.v[k], use1 ? a1.v[k] : 0.0f, a2.v[k], c);
    }
    st<V>(xb + i, out);
    st<V>(h2 + i, a1);
    st<V>(h1 + i, m);
  }
}

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_slot_step_edit(float* x, const void* eps, float* hist, const float* cond, const float* cmask,
                                    const float* row_coef, const int* row_kind, const int* row_ord, const int* pos,
                                    const int* active, const long long* seeds, int B, int R, int C, int H, int W, int dtype,
                                    afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && hist && cond && cmask && row_coef && row_kind && row_ord && pos && active && seeds, AFLDM_ENULL,
                "afldm_slot_step_edit: NULL pointer");
  AFLDM_REQUIRE(B > 0 && B <= 65535 && R > 0 && C > 0 && H > 0 && W > 0 && (size_t)C * H * W <= SLOT_ELEMS_MAX, AFLDM_ESHAPE,
                "afldm_slot_step_edit: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, n = C * HW;
  // (HW % 4 == 0: every slot's planes, its mask plane and the second half of hist start a whole number of 16-byte groups in)
  const bool v4 = HW % 4 == 0 && aligned16(x) && aligned16(hist) && aligned16(cond) && aligned16(cmask);
#define LAUNCH(T, V)                                                                                                            \
  (k_slot_step_edit<T, V><<<dim3(step_grid(n / V), B), 256, 0, st>>>(x, (const T*)eps, hist, cond, cmask, row_coef, row_kind, \
                                                                     row_ord, pos, active, seeds, B, R, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_slot_step_edit");
#undef LAUNCH
  return check_launch("afldm_slot_step_edit");
}
