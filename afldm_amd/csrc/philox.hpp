// philox.hpp — the counter-based noise stream of the seeded samplers (noise.hip, edit.hip).
// Philox-4x32-10 as in Random123 (Salmon et al., SC'11), then Box-Muller.  The noise of a request is a pure function of
//   key      (seed & 0xffffffff, seed >> 32)                                  the request's seed, 0 <= seed < 2^63
//   counter  (g, ordinal, slot, 0)    g = i >> 2 of element i in the sample's own flat [C, H, W] order, ordinal = the step
//                                     within the request's own schedule, slot = the noise slot (0; 1, 2: edit.hip)
//   uniforms u_j = ((r_j >> 9) + 0.5) 2^-23: exact in fp32, in [2^-24, 1 - 2^-24]
//   normals  (z0, z1) = sqrt(-2 ln u0) (cos 2 pi u1, sin 2 pi u1), (z2, z3) likewise from (u2, u3); element 4 g + k gets z_k
// so it needs no buffer and no host draw, and does not depend on the batch position, the neighbours or the vector width.
// philox4x32_10 is plain C++ (host and device): tools/philox_check.cpp compiles it alone, under the host sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AFLDM_PHILOX_FN __host__ __device__ inline
#else
#define AFLDM_PHILOX_FN inline
#endif

namespace afldm {

struct philox_words {
  uint32_t w[4];
};

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // the multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // the key increments

// ten rounds of (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped after each
AFLDM_PHILOX_FN philox_words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return {{c0, c1, c2, c3}};
}

AFLDM_PHILOX_FN philox_words philox_seeded(long long seed, uint32_t group, uint32_t ordinal, uint32_t slot) {
  const uint64_t s = (uint64_t)seed;
  return philox4x32_10(group, ordinal, slot, 0u, (uint32_t)s, (uint32_t)(s >> 32));
}

#if defined(__HIPCC__)

struct philox_normals {
  float z[4];
};

__device__ __forceinline__ float philox_uniform(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 0x1p-23f; }

// The four normals of one group.  sincospif(2 u) takes the angle in half turns, where 2 u is exact: no 2 pi u rounding and no
// large-argument reduction (which would cost scratch).
__device__ __forceinline__ philox_normals philox_normal4(long long seed, uint32_t group, uint32_t ordinal, uint32_t slot) {
  const philox_words r = philox_seeded(seed, group, ordinal, slot);
  philox_normals n;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float rad = sqrtf(-2.0f * logf(philox_uniform(r.w[2 * h])));
    float sn, cs;
    sincospif(2.0f * philox_uniform(r.w[2 * h + 1]), &sn, &cs);
    n.z[2 * h] = rad * cs;
    n.z[2 * h + 1] = rad * sn;
  }
  return n;
}

// one element's normal: the call of its group, lane i & 3 (the scalar forms)
__device__ __forceinline__ float philox_normal1(long long seed, uint32_t elem, uint32_t ordinal, uint32_t slot) {
  const philox_words r = philox_seeded(seed, elem >> 2, ordinal, slot);
  const int h = (elem >> 1) & 1;
  const float u0 = philox_uniform(h ? r.w[2] : r.w[0]), u1 = philox_uniform(h ? r.w[3] : r.w[1]);
  const float rad = sqrtf(-2.0f * logf(u0));
  float sn, cs;
  sincospif(2.0f * u1, &sn, &cs);
  return rad * ((elem & 1) ? sn : cs);
}

#endif  // __HIPCC__

}  // namespace afldm
