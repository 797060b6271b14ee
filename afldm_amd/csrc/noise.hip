// noise.hip — counter-based device noise and the samplers' updates that use it (libafldm_noise.so, include/afldm_hip_noise.h).
// The noise is the stream of philox.hpp: a pure function of (request seed, step ordinal, noise slot, element) computed in
// registers, so the stochastic update needs no noise buffer, no host draw and - in the slot sampler - no feed per slot.
//   afldm_philox_bits       the raw Philox words of given counters (the known-answer tests)
//   afldm_counter_noise     the stream materialised, fp32 NCHW (the eager path and the tests)
//   afldm_seeded_step       afldm_sde_step with z made in registers: ordinal *step_idx, one seed per sample
//   afldm_slot_step_seeded  afldm_slot_step_kinds plus kind code 2: that update with ordinal row_ord[pos[b]] and seed seeds[b]
// The update is seeded_update (seeded_common.hpp, shared with edit.hip), written once with contraction off and no fma, so a
// float32 restatement in the stated order gives its bits (tests/noise_oracle.py).  A row whose c is 0 generates nothing: z = 0.
// Layout as sde.hip / slot_kinds.hip: a thread owns 4 consecutive elements of one (b, c) plane (one Philox call, 16-byte loads
// and stores) or, in the scalar form, one element (the call of its group, lane i & 3: the values do not depend on the form);
// grid capped at 2048 blocks and grid-stride beyond.  Each thread reads and writes its own indices only, so x and x_out may
// alias; every table index read from device memory is range-checked before use.  Per thread ten Philox rounds, two log / sqrt and
// two sincospi against one 16-byte store: HBM-bound.
// Resources (gfx950, -O3, the compiler's resource report; no scratch, no LDS, no AGPRs in any of them):
//   k_philox_bits 20 VGPRs;  k_counter_noise 32 in the 16-byte form, 22 in the scalar form;  k_seeded_step 45 (fp32 eps) / 49 (bf16
//   eps) and 30;  k_slot_step_seeded 40 / 44 and 24;  8 waves per SIMD everywhere
#include "seeded_common.hpp"

#include "../../include/afldm_hip_noise.h"

namespace afldm {

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

}  // namespace

// out uint32 [B][groups][4]; wide: 16-byte stores (out 16-byte aligned)
template <bool WIDE>
__global__ void __launch_bounds__(256) k_philox_bits(unsigned int* __restrict__ out, const long long* __restrict__ seeds, uint32_t g0,
                                                     uint32_t ordinal, uint32_t slot, uint32_t c3, int B, size_t groups) {
  const size_t total = (size_t)B * groups;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const size_t b = t / groups, g = t % groups;
    const uint64_t s = (uint64_t)seeds[b];
    const philox_words r = philox4x32_10(g0 + (uint32_t)g, ordinal, slot, c3, (uint32_t)s, (uint32_t)(s >> 32));
    if constexpr (WIDE) {
      const u32x4 q = {r.w[0], r.w[1], r.w[2], r.w[3]};
      *reinterpret_cast<u32x4*>(out + 4 * t) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) out[4 * t + k] = r.w[k];
    }
  }
}

// out fp32 [B][n], n = C H W of one sample.  V = 4 needs n % 4 == 0 and out 16-byte aligned.
template <int V>
__global__ void __launch_bounds__(256) k_counter_noise(float* __restrict__ out, const long long* __restrict__ seeds,
                                                       const int* __restrict__ ordinals, uint32_t slot, int B, size_t n) {
  const size_t groups = (size_t)B * n / V;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i = g * V, b = i / n;
    st<V>(out + i, seeded_z<V>(true, seeds[b], (uint32_t)(i - b * n), (uint32_t)ordinals[b], slot));
  }
}

// x, x_out NCHW fp32; eps NHWC T.  V = 4 needs HW % 4 == 0 and 16-byte aligned x / x_out.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_seeded_step(const float* x, const T* __restrict__ eps, const long long* __restrict__ seeds,
                                                     float* x_out, const float* __restrict__ coef, const int* __restrict__ step_idx,
                                                     int B, int C, int HW) {
  const int s = *step_idx;
  if (s < 0) return;                     // (a counter that was never advanced: nothing to read)
  const float* rp = coef + 8 * (size_t)s;
  const sde_row r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7]};
  const bool gen = r.c != 0.0f;
  const size_t per = (size_t)C * HW, n = (size_t)B * per;
  const size_t groups = n / V;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i = g * V;
    const nchw_pos at = nchw_at(i, C, HW);
    const T* ep = eps_at(eps, at, C, HW);
    const vecf<V> xv = ld<V>(x + i);
    const vecf<V> z = seeded_z<V>(gen, gen ? seeds[at.b] : 0, (uint32_t)(i - at.b * per), (uint32_t)s, 0u);
    vecf<V> o;
#pragma unroll
    for (int k = 0; k < V; ++k) o.v[k] = seeded_update(xv.v[k], to_f32(ep[(size_t)k * C]), z.v[k], r);
    st<V>(x_out + i, o);
  }
}

// k_slot_step_kinds (slot_kinds.hip) with a third kind.  x NCHW fp32 [B, C, HW], in place; eps NHWC T; hist fp32 [2, B, C, HW];
// row_coef [R, 8]: the "ddim" row's first four floats, the "dpm" row, or the "seeded" row (p, q, lo, hi, a, b, d, c).
// V = 4 needs HW % 4 == 0 and 16-byte aligned x and hist.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_slot_step_seeded(float* x, const T* __restrict__ eps, float* hist,
                                                          const float* __restrict__ row_coef, const int* __restrict__ row_kind,
                                                          const int* __restrict__ row_ord, const int* __restrict__ pos,
                                                          const int* __restrict__ active, const long long* __restrict__ seeds,
                                                          int B, int R, int C, int HW) {
  const int b = blockIdx.y;
  if (!active[b]) return;
  const int s = pos[b];
  if (s < 0 || s >= R) return;
  const int kind = row_kind[s];
  if (kind != KIND_DDIM && kind != KIND_DPM && kind != KIND_SEEDED) return;
  const float* r = row_coef + 8 * (size_t)s;
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

extern "C" int afldm_philox_bits(unsigned int* out, const long long* seeds, long long g0, long long ordinal, long long slot,
                                 long long c3, int B, long long groups, afldm_stream_t stream) {
  AFLDM_REQUIRE(out && seeds, AFLDM_ENULL, "afldm_philox_bits: NULL pointer");
  AFLDM_REQUIRE(B > 0 && groups > 0 && groups <= ((long long)1 << 32), AFLDM_ESHAPE, "afldm_philox_bits: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)B * (size_t)groups;
  if (aligned16(out))
    k_philox_bits<true><<<step_grid(total), 256, 0, st>>>(out, seeds, (uint32_t)g0, (uint32_t)ordinal, (uint32_t)slot, (uint32_t)c3,
                                                           B, (size_t)groups);
  else
    k_philox_bits<false><<<step_grid(total), 256, 0, st>>>(out, seeds, (uint32_t)g0, (uint32_t)ordinal, (uint32_t)slot,
                                                            (uint32_t)c3, B, (size_t)groups);
  return check_launch("afldm_philox_bits");
}

extern "C" int afldm_counter_noise(float* out, const long long* seeds, const int* ordinals, int slot, int B, int C, int H, int W,
                                   afldm_stream_t stream) {
  AFLDM_REQUIRE(out && seeds && ordinals, AFLDM_ENULL, "afldm_counter_noise: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && slot >= 0 && (size_t)C * H * W <= SLOT_ELEMS_MAX, AFLDM_ESHAPE,
                "afldm_counter_noise: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)C * H * W, total = (size_t)B * n;
  if (n % 4 == 0 && aligned16(out))
    k_counter_noise<4><<<step_grid(total / 4), 256, 0, st>>>(out, seeds, ordinals, (uint32_t)slot, B, n);
  else
    k_counter_noise<1><<<step_grid(total), 256, 0, st>>>(out, seeds, ordinals, (uint32_t)slot, B, n);
  return check_launch("afldm_counter_noise");
}

extern "C" int afldm_seeded_step(const float* x, const void* eps, const long long* seeds, float* x_out, const float* coef,
                                 int* step_idx, int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && seeds && x_out && coef && step_idx, AFLDM_ENULL, "afldm_seeded_step: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (size_t)C * H * W <= SLOT_ELEMS_MAX, AFLDM_ESHAPE,
                "afldm_seeded_step: bad shape");
  const int HW = H * W;
  const size_t n = (size_t)B * C * HW;
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = HW % 4 == 0 && aligned16(x) && aligned16(x_out);
#define LAUNCH(T, V) (k_seeded_step<T, V><<<step_grid(n / V), 256, 0, st>>>(x, (const T*)eps, seeds, x_out, coef, step_idx, B, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_seeded_step");
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_seeded_step");
}

extern "C" int afldm_slot_step_seeded(float* x, const void* eps, float* hist, const float* row_coef, const int* row_kind,
                                      const int* row_ord, const int* pos, const int* active, const long long* seeds, int B, int R,
                                      int C, int H, int W, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && hist && row_coef && row_kind && row_ord && pos && active && seeds, AFLDM_ENULL,
                "afldm_slot_step_seeded: NULL pointer");
  AFLDM_REQUIRE(B > 0 && B <= 65535 && R > 0 && C > 0 && H > 0 && W > 0 && (size_t)C * H * W <= SLOT_ELEMS_MAX, AFLDM_ESHAPE,
                "afldm_slot_step_seeded: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, n = C * HW;
  // (HW % 4 == 0: every slot's planes, and the second half of hist, start a whole number of 16-byte groups in)
  const bool v4 = HW % 4 == 0 && aligned16(x) && aligned16(hist);
#define LAUNCH(T, V)                                                                                                            \
  (k_slot_step_seeded<T, V><<<dim3(step_grid(n / V), B), 256, 0, st>>>(x, (const T*)eps, hist, row_coef, row_kind, row_ord, pos, \
                                                                       active, seeds, B, R, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_slot_step_seeded");
#undef LAUNCH
  return check_launch("afldm_slot_step_seeded");
}
