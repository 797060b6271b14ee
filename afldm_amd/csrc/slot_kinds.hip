// slot_kinds.hip — afldm_slot_step_kinds (libafldm_slots.so, include/afldm_hip_slots.h): the slot sampler's update for a row table
// that holds "ddim" AND "dpm" rows (row_coef [R, 8], row_kind [R]).  It is afldm_slot_step's launch (slots.hip): a "dpm" slot takes
// k_dpm_step's update on its own planes of a per-slot history [2, B, C, HW], a "ddim" slot slot_update and its history planes stay
// untouched.  A history plane whose coefficient is exactly 0 never enters the arithmetic (zeros do: what a cleared history
// gives), so a refilled slot needs no history clear: its first row has b1 = b2 = 0, its second b2 = 0, and what the previous
// occupant left - NaN included - reaches no result.  h2 is not loaded then (ld_if); h1 is still read when b1 = 0, for the shift
// h2 <- h1 alone, so that both planes keep afldm_dpm_step's bits on every row.
// A block serves one slot (blockIdx.y): what it needs of the slot's state is uniform over the block.  HBM-bound; each thread
// reads and writes its own indices only; every table index read from device memory is range-checked before use.
// Resources (gfx950, -O3, the compiler's resource report): 36 VGPRs in the 16-byte form and 20 in the scalar form, for fp32 and
// for bf16 eps alike; no scratch, no LDS, no AGPRs; 8 waves per SIMD.
#include "slot_common.hpp"

#include "../../include/afldm_hip_slots.h"

namespace afldm {

// x NCHW fp32 [B, C, HW], in place; eps NHWC T; hist fp32 [2, B, C, HW] (h1, then h2; slot b's planes at b C HW in each half); row_coef [R, 8]: a "ddim" row's first
// four floats, or the "dpm" row (p, q, a, b0, b1, b2, 0, 0).  V = 4 needs HW % 4 == 0 and 16-byte aligned x and hist.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_slot_step_kinds(float* x, const T* __restrict__ eps, float* hist,
                                                         const float* __restrict__ row_coef, const int* __restrict__ row_kind,
                                                         const int* __restrict__ pos, const int* __restrict__ active, int B, int R,
                                                         int C, int HW) {
  const int b = blockIdx.y;
  if (!active[b]) return;
  const int s = pos[b];
  if (s < 0 || s >= R) return;
  const int kind = row_kind[s];
  if (kind != KIND_DDIM && kind != KIND_DPM) return;
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

extern "C" int afldm_slot_step_kinds(float* x, const void* eps, float* hist, const float* row_coef, const int* row_kind,
                                     const int* pos, const int* active, int B, int R, int C, int H, int W, int dtype,
                                     afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && hist && row_coef && row_kind && pos && active, AFLDM_ENULL, "afldm_slot_step_kinds: NULL pointer");
  AFLDM_REQUIRE(B > 0 && B <= 65535 && R > 0 && C > 0 && H > 0 && W > 0 && (size_t)C * H * W <= SLOT_ELEMS_MAX, AFLDM_ESHAPE,
                "afldm_slot_step_kinds: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, n = C * HW;
  // (HW % 4 == 0: every slot's planes, and the second half of hist, start a whole number of 16-byte groups in)
  const bool v4 = HW % 4 == 0 && aligned16(x) && aligned16(hist);
#define LAUNCH(T, V)                                                                                                          \
  (k_slot_step_kinds<T, V><<<dim3(step_grid(n / V), B), 256, 0, st>>>(x, (const T*)eps, hist, row_coef, row_kind, pos, active, B, \
                                                                      R, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_slot_step_kinds");
#undef LAUNCH
  return check_launch("afldm_slot_step_kinds");
}
