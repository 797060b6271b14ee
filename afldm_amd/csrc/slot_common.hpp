// slot_common.hpp — what the slot sampler's translation units share (slots.hip in libafldm_hip.so, slot_kinds.hip in
// libafldm_slots.so, noise.hip in libafldm_noise.so).  Internal linkage, as step_common.hpp: each gets its own copy.
#pragma once
#include "step_common.hpp"

namespace afldm {

namespace {

constexpr size_t SLOT_ELEMS_MAX = (size_t)1 << 30;      // elements of one slot: the kernels index a slot with int, grid stride included

// k_ddim_step's update as the compiler builds it there: x - c1 e is ONE fma, the last line two rounded products and a sum.
// Spelled out, with contraction off, because left to itself the compiler fuses the last line in the 4-wide form of k_slot_step
// and not in k_ddim_step, and a slot must give afldm_ddim_step's bits (tests/test_gpu_slots.py compares them).
__device__ __forceinline__ float slot_update(float x, float e, float sa_t, float sb_t, float sa_p, float sb_p) {
#pragma clang fp contract(off)
  const float x0 = __builtin_fmaf(-sb_t, e, x) / sa_t;
  const float a = sa_p * x0, b = sb_p * e;
  return a + b;
}

// k_dpm_step's update as the compiler builds it there (gfx950 disassembly of its four instantiations; fp32 and bf16 eps agree,
// the 16-byte and the scalar form do not).  V = 4: the packed fma pairs element 2j's p x with element 2j + 1's q e, so
//   even elements  m = fma(p, x, rn(q e)),   odd elements  m = fma(q, e, rn(p x)),
//   x' = fma(b2, h2, fma(b1, h1, fma(a, x, rn(b0 m))))
// V = 1:  m = fma(p, x, rn(q e)),   x' = ((rn(a x) + rn(b0 m)) + rn(b1 h1)) + rn(b2 h2): four rounded products, three sums.
// Spelled out with contraction off, as slot_update (slot_common.hpp): a slot must give afldm_dpm_step's bits (tests/test_gpu_slots_dpm.py).
struct dpm_coef {
  float p, q, a, b0, b1, b2;
};

template <int V>
__device__ __forceinline__ float slot_dpm_m0(int k, float x, float e, const dpm_coef& c) {
#pragma clang fp contract(off)
  if (V == 4 && (k & 1)) {
    const float t = c.p * x;
    return __builtin_fmaf(c.q, e, t);
  }
  const float t = c.q * e;
  return __builtin_fmaf(c.p, x, t);
}

template <int V>
__device__ __forceinline__ float slot_dpm_out(float x, float m, float h1, float h2, const dpm_coef& c) {
#pragma clang fp contract(off)
  if (V == 4) {
    const float t = c.b0 * m;
    return __builtin_fmaf(c.b2, h2, __builtin_fmaf(c.b1, h1, __builtin_fmaf(c.a, x, t)));
  }
  const float ax = c.a * x, bm = c.b0 * m, t1 = c.b1 * h1, t2 = c.b2 * h2;
  return ((ax + bm) + t1) + t2;
}

constexpr int KIND_DDIM = 0, KIND_DPM = 1;      // row_kind codes (SlotTable.KIND_CODES in afldm_amd/engine.py)

}  // namespace

}  // namespace afldm
