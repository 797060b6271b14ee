// seeded_common.hpp — what the translation units with a seeded update share (noise.hip in libafldm_noise.so, edit.hip in
// libafldm_edit.so): the "seeded" row, its update and the normals of a thread's elements.  Internal linkage, as slot_common.hpp:
// each gets its own copy.
#pragma once
#include "philox.hpp"
#include "slot_common.hpp"

namespace afldm {

namespace {

struct sde_row {
  float p, q, lo, hi, a, b, d, c;
};

// The "seeded" update, the "sde" row (p, q, lo, hi, a, b, d, c) in this order of float operations - products rounded one by one,
// sums left to right, no fma:
//   t = rn(p x) + rn(q e);  x0 = clamp_nan(t, lo, hi);  out = ((rn(a x) + rn(b x0)) + rn(d e)) + rn(c z)
__device__ __forceinline__ float seeded_update(float x, float e, float z, const sde_row& r) {
#pragma clang fp contract(off)
  const float px = r.p * x, qe = r.q * e;
  const float t = px + qe;
  const float x0 = clamp_nan(t, r.lo, r.hi);
  const float ax = r.a * x, bx = r.b * x0, de = r.d * e, cz = r.c * z;
  return ((ax + bx) + de) + cz;
}

// V elements of one sample from element i (i % V == 0) of its flat [C, H, W] order; zeros when the row generates nothing
template <int V>
__device__ __forceinline__ vecf<V> seeded_z(bool on, long long seed, uint32_t i, uint32_t ordinal, uint32_t slot) {
  vecf<V> z;
  if (!on) {
#pragma unroll
    for (int k = 0; k < V; ++k) z.v[k] = 0.0f;
  } else if constexpr (V == 4) {
    const philox_normals n = philox_normal4(seed, i >> 2, ordinal, slot);
#pragma unroll
    for (int k = 0; k < 4; ++k) z.v[k] = n.z[k];
  } else {
    z.v[0] = philox_normal1(seed, i, ordinal, slot);
  }
  return z;
}

constexpr int KIND_SEEDED = 2;                 // row_kind code (SeededSlotTable.KIND_CODES in afldm_amd/engine.py)

}  // namespace

}  // namespace afldm
