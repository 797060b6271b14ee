// sdedit.hip — image-to-image sampling on the graph-replayed engine: SDEdit (Meng et al., ICLR 2022) with a per-element change
// map (Differential Diffusion, Levin & Fried 2023).  Each UNet evaluation is one coefficient row
// (p, q, lo, hi, a, b, c, k0, k1, thr, 0, 0), the run's ONE fixed noise z and one pre-drawn fp32 noise slot z_u:
//   x0    = clamp(p x + q eps, lo, hi)
//   xp    = a x0 + b eps + c z_u                   the reverse step of a released element
//   held  = k0 orig + k1 z                         the original, noised to the next level
//   x_out = (cmap <= thr) ? held : xp              cmap = change map [b, 0, h, w]; a SELECT: nothing of xp reaches a held element
// The comparison is false for a NaN in cmap, so such an element is generated.  z is loaded only where k1 != 0 and z_u only where
// c != 0 (uniform branches: the row is the same for every thread), so whatever an unused buffer holds - zeros, stale memory,
// NaN - cannot reach the output; and because the last line selects, neither can a NaN or Inf of x or eps at a held element
// (RePaint's blend m knownp + (1 - m) unknown would leak 0 * NaN there).  HBM-bound elementwise, laid out as repaint.hip: every
// thread owns 4 consecutive pixels of one (b, c) plane (16-byte loads of x / orig / cmap / z / z_u, stores of x_out), grid capped
// at 2048 blocks and grid-stride beyond (guide G11).  Each thread reads and writes its own indices only, so x and x_out may alias.
#include "step_common.hpp"

namespace afldm {

namespace {

struct sdedit_row {
  float p, q, lo, hi, a, b, c, k0, k1, thr;
};

// z / zu: 0 where the buffer is not loaded (its coefficient is 0 then, and the product an exact 0).  The roundings are spelled
// out - one product, then fused multiply-adds in this order, nothing left to the compiler's contraction - so that the four engine
// kernels and the two flat ones give the same bits for the same operands.
__device__ __forceinline__ float sdedit_update(float x, float e, float og, float m, float z, float zu, const sdedit_row& r) {
#pragma clang fp contract(off)
  const float qe = r.q * e;
  const float x0 = clamp_nan(__builtin_fmaf(r.p, x, qe), r.lo, r.hi);
  const float ax0 = r.a * x0;
  const float xp = __builtin_fmaf(r.c, zu, __builtin_fmaf(r.b, e, ax0));
  const float k0o = r.k0 * og;
  const float held = __builtin_fmaf(r.k1, z, k0o);
  return m <= r.thr ? held : xp;
}

}  // namespace

// x, orig, z, x_out, noise NCHW fp32; cmap [B][1][HW] fp32; eps NHWC T.  V = 4 needs HW % 4 == 0, the noise stride % 4 == 0 and
// 16-byte aligned x / orig / cmap / z / x_out / noise.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_sdedit_step(const float* x, const T* __restrict__ eps, const float* __restrict__ orig,
                                                     const float* __restrict__ cmap, const float* __restrict__ z,
                                                     const float* __restrict__ noise, size_t noise_step_stride, float* x_out,
                                                     const float* __restrict__ coef, const int* __restrict__ step_idx, int B,
                                                     int C, int HW) {
  const int s = *step_idx;
  const float* rp = coef + 12 * (size_t)s;
  const sdedit_row r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8], rp[9]};
  const bool has_z = r.k1 != 0.0f, has_u = r.c != 0.0f && noise != nullptr;      // (noise is NULL where no step of the schedule draws)
  const float* zu = has_u ? noise + (size_t)s * noise_step_stride : nullptr;
  const size_t n = (size_t)B * C * HW;
  const size_t groups = n / V;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i = g * V;
    const nchw_pos at = nchw_at(i, C, HW);
    const T* ep = eps_at(eps, at, C, HW);
    const vecf<V> xv = ld<V>(x + i), ov = ld<V>(orig + i), mv = ld<V>(cmap + at.b * HW + at.pix);
    const vecf<V> zv = ld_if<V>(has_z, z + i), zuv = ld_if<V>(has_u, zu + i);
    vecf<V> o;
#pragma unroll
    for (int k = 0; k < V; ++k) o.v[k] = sdedit_update(xv.v[k], to_f32(ep[(size_t)k * C]), ov.v[k], mv.v[k], zv.v[k], zuv.v[k], r);
    st<V>(x_out + i, o);
  }
}

// flat same-layout fp32 tensors (the change map too), the row by value; z / z_u are only read where k1 / c is not 0.  16-byte
// groups, then a scalar tail.
template <int V>
__global__ void __launch_bounds__(256) k_sdedit_step_flat(const float* x, const float* __restrict__ eps,
                                                          const float* __restrict__ orig, const float* __restrict__ cmap,
                                                          const float* __restrict__ z, const float* __restrict__ zu, float* x_out,
                                                          sdedit_row r, size_t n) {
  const bool has_z = r.k1 != 0.0f, has_u = r.c != 0.0f;
  const size_t groups = n / V;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t g = tid; g < groups; g += stride) {
    const size_t i = g * V;
    const vecf<V> xv = ld<V>(x + i), ev = ld<V>(eps + i), ov = ld<V>(orig + i), mv = ld<V>(cmap + i);
    const vecf<V> zv = ld_if<V>(has_z, z + i), zuv = ld_if<V>(has_u, zu + i);
    vecf<V> o;
#pragma unroll
    for (int k = 0; k < V; ++k) o.v[k] = sdedit_update(xv.v[k], ev.v[k], ov.v[k], mv.v[k], zv.v[k], zuv.v[k], r);
    st<V>(x_out + i, o);
  }
  for (size_t i = groups * V + tid; i < n; i += stride)
    x_out[i] = sdedit_update(x[i], eps[i], orig[i], cmap[i], has_z ? z[i] : 0.0f, has_u ? zu[i] : 0.0f, r);
}

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_sdedit_step(const float* x, const void* eps, const float* orig, const float* cmap, const float* z,
                                 const float* noise, size_t noise_step_stride, float* x_out, const float* coef, int* step_idx,
                                 int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream) {
  // (noise is NULL for a schedule none of whose steps draws: every row has c = 0 then, and the kernel never reads through it)
  AFLDM_REQUIRE(x && eps && orig && cmap && z && x_out && coef && step_idx, AFLDM_ENULL, "afldm_sdedit_step: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, AFLDM_ESHAPE, "afldm_sdedit_step: bad shape");
  const int HW = H * W;
  const size_t n = (size_t)B * C * HW;
  AFLDM_REQUIRE(!noise || noise_step_stride >= n, AFLDM_ESHAPE, "afldm_sdedit_step: noise_step_stride smaller than B*C*H*W");
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = HW % 4 == 0 && noise_step_stride % 4 == 0 && aligned16(x) && aligned16(orig) && aligned16(cmap) && aligned16(z) &&
                  aligned16(x_out) && aligned16(noise);
#define LAUNCH(T, V)                                                                                                      \
  (k_sdedit_step<T, V><<<step_grid(n / V), 256, 0, st>>>(x, (const T*)eps, orig, cmap, z, noise, noise_step_stride, x_out, coef, \
                                                         step_idx, B, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_sdedit_step");
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_sdedit_step");
}

extern "C" int afldm_sdedit_step_flat(const float* x, const float* eps, const float* orig, const float* cmap, const float* z,
                                      const float* z_u, float* x_out, float p, float q, float lo, float hi, float a, float b,
                                      float c, float k0, float k1, float thr, size_t n, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && orig && cmap && x_out, AFLDM_ENULL, "afldm_sdedit_step_flat: NULL pointer");
  AFLDM_REQUIRE((k1 == 0.0f || z) && (c == 0.0f || z_u), AFLDM_ENULL,
                "afldm_sdedit_step_flat: a noise tensor with a non-zero coefficient is NULL");
  if (n == 0) return AFLDM_OK;
  hipStream_t st = (hipStream_t)stream;
  const sdedit_row r{p, q, lo, hi, a, b, c, k0, k1, thr};
  const bool v4 = aligned16(x) && aligned16(eps) && aligned16(orig) && aligned16(cmap) && aligned16(x_out) &&
                  (k1 == 0.0f || aligned16(z)) && (c == 0.0f || aligned16(z_u));
  if (v4)
    k_sdedit_step_flat<4><<<step_grid(n / 4), 256, 0, st>>>(x, eps, orig, cmap, z, z_u, x_out, r, n);
  else
    k_sdedit_step_flat<1><<<step_grid(n), 256, 0, st>>>(x, eps, orig, cmap, z, z_u, x_out, r, n);
  return check_launch("afldm_sdedit_step_flat");
}
