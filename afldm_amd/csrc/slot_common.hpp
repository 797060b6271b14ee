// slot_common.hpp — what the slot sampler's two translation units share (slots.hip in libafldm_hip.so, slot_kinds.hip in
// libafldm_slots.so).  Internal linkage, as step_common.hpp: each gets its own copy.
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

}  // namespace

}  // namespace afldm
