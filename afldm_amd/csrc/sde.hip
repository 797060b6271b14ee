// sde.hip — the stochastic sampler update on the graph-replayed engine: DDIM with eta != 0 (diffusers DDIMScheduler.step)
// and the I2SB bridge in every (is_ode, clip_sample) form (I2SBScheduler.step).  Each step is one coefficient row
// (p, q, lo, hi, a, b, d, c) and one pre-drawn fp32 noise plane z:
//   x0 = clamp(p x + q eps, lo, hi);  x_out = a x + b x0 + d eps + c z
// The noise is drawn by the caller's generator outside the graph (the same randn calls the eager loop makes), so the
// sample is the eager loop's to fp32 rounding.  HBM-bound elementwise, laid out as dpm.hip: every thread owns 4
// consecutive pixels of one (b, c) plane (16-byte loads of x / z, stores of x_out), grid capped at 2048 blocks and
// grid-stride beyond (guide G11).  Each thread reads and writes its own indices only, so x and x_out may alias.
#include "step_common.hpp"

namespace afldm {

namespace {

struct sde_row {
  float p, q, lo, hi, a, b, d, c;
};

__device__ __forceinline__ float sde_update(float x, float e, float z, const sde_row& r) {
  const float x0 = clamp_nan(r.p * x + r.q * e, r.lo, r.hi);
  return r.a * x + r.b * x0 + r.d * e + r.c * z;
}

}  // namespace

// x, x_out, noise rows NCHW fp32; eps NHWC T.  V = 4 needs HW % 4 == 0 and 16-byte aligned x / x_out / noise row.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_sde_step(const float* x, const T* __restrict__ eps, const float* __restrict__ noise,
                                                  size_t noise_step_stride, float* x_out, const float* __restrict__ coef,
                                                  const int* __restrict__ step_idx, int B, int C, int HW) {
  const int s = *step_idx;
  const float* rp = coef + 8 * (size_t)s;
  const sde_row r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7]};
  const float* z = noise + (size_t)s * noise_step_stride;
  const size_t n = (size_t)B * C * HW;
  const size_t groups = n / V;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i = g * V;
    const T* ep = eps_at(eps, nchw_at(i, C, HW), C, HW);
    if constexpr (V == 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
      const f32x4 zv = *reinterpret_cast<const f32x4*>(z + i);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = sde_update(xv[k], to_f32(ep[(size_t)k * C]), zv[k], r);
      *reinterpret_cast<f32x4*>(x_out + i) = o;
    } else {
      x_out[i] = sde_update(x[i], to_f32(ep[0]), z[i], r);
    }
  }
}

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_sde_step(const float* x, const void* eps, const float* noise, size_t noise_step_stride, float* x_out,
                              const float* coef, int* step_idx, int advance, int B, int C, int H, int W, int dtype,
                              afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && noise && x_out && coef && step_idx, AFLDM_ENULL, "afldm_sde_step: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, AFLDM_ESHAPE, "afldm_sde_step: bad shape");
  const int HW = H * W;
  const size_t n = (size_t)B * C * HW;
  AFLDM_REQUIRE(noise_step_stride >= n, AFLDM_ESHAPE, "afldm_sde_step: noise_step_stride smaller than one step's B*C*H*W");
  hipStream_t st = (hipStream_t)stream;
  // every noise row starts noise_step_stride floats after the previous one: 16-byte groups need that stride % 4 == 0 too
  const bool v4 = HW % 4 == 0 && noise_step_stride % 4 == 0 && aligned16(x) && aligned16(x_out) && aligned16(noise);
#define LAUNCH(T, V) \
  (k_sde_step<T, V><<<step_grid(n / V), 256, 0, st>>>(x, (const T*)eps, noise, noise_step_stride, x_out, coef, step_idx, B, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_sde_step");
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_sde_step");
}
