// dpm.hip — DPM-Solver(++) multistep update (DPMSolverMultistepScheduler, afldm_amd/schedulers/dpmsolver.py).
// For epsilon / v / sample prediction every step of order 1..3 is a linear combination of the latent, the model
// output and at most two earlier converted outputs, so a step is one coefficient row (p, q, a, b0, b1, b2, 0, 0):
//   m0 = p x + q eps;  x_out = a x + b0 m0 + b1 h1 + b2 h2;  h2 <- h1, h1 <- m0
// HBM-bound elementwise: every thread owns 4 consecutive pixels of one (b, c) plane (16-byte loads of x / h1 / h2 /
// x_out), grid capped at 2048 blocks and grid-stride beyond (guide G11).  Each thread reads and writes its own
// indices only, so x and x_out may alias and the history shifts in place.
#include "step_common.hpp"

namespace afldm {

namespace {

struct dpm_row {
  float p, q, a, b0, b1, b2;
};

// one group of V elements: x, h1, h2 at `i` (same layout), eps values already in registers
template <int V>
__device__ __forceinline__ void dpm_update(const float* x, float* x_out, float* h1, float* h2, size_t i,
                                           const float (&e)[V], const dpm_row& c) {
  vecf<V> xv = ld<V>(x + i), a1 = ld<V>(h1 + i), a2 = ld<V>(h2 + i), out, m;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    m.v[k] = c.p * xv.v[k] + c.q * e[k];
    out.v[k] = c.a * xv.v[k] + c.b0 * m.v[k] + c.b1 * a1.v[k] + c.b2 * a2.v[k];
  }
  st<V>(x_out + i, out);
  st<V>(h2 + i, a1);
  st<V>(h1 + i, m);
}

}  // namespace

// x, x_out NCHW fp32; eps NHWC T; hist [2][B][C][HW].  V = 4 needs HW % 4 == 0 and 16-byte aligned fp32 tensors.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_dpm_step(const float* x, const T* __restrict__ eps, float* x_out, float* hist,
                                                  const float* __restrict__ coef, const int* __restrict__ step_idx, int B,
                                                  int C, int HW) {
  const int s = *step_idx;
  const float* r = coef + 8 * (size_t)s;
  const dpm_row c{r[0], r[1], r[2], r[3], r[4], r[5]};
  const size_t n = (size_t)B * C * HW;
  float* h1 = hist;
  float* h2 = hist + n;
  const size_t groups = n / V;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i = g * V;
    const T* ep = eps_at(eps, nchw_at(i, C, HW), C, HW);
    float e[V];
#pragma unroll
    for (int k = 0; k < V; ++k) e[k] = to_f32(ep[(size_t)k * C]);
    dpm_update<V>(x, x_out, h1, h2, i, e, c);
  }
}

// flat same-layout fp32 tensors, coefficients by value; hist [2][n].  16-byte groups, then a scalar tail.
template <int V>
__global__ void __launch_bounds__(256) k_dpm_step_flat(const float* x, const float* __restrict__ eps, float* x_out,
                                                       float* hist, dpm_row c, size_t n) {
  float* h1 = hist;
  float* h2 = hist + n;
  const size_t groups = n / V;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t g = tid; g < groups; g += stride) {
    const size_t i = g * V;
    vecf<V> ev = ld<V>(eps + i);
    float e[V];
#pragma unroll
    for (int k = 0; k < V; ++k) e[k] = ev.v[k];
    dpm_update<V>(x, x_out, h1, h2, i, e, c);
  }
  for (size_t i = groups * V + tid; i < n; i += stride) {
    const float e[1] = {eps[i]};
    dpm_update<1>(x, x_out, h1, h2, i, e, c);
  }
}

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_dpm_step(const float* x, const void* eps, float* x_out, float* hist, const float* coef, int* step_idx,
                              int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && x_out && hist && coef && step_idx, AFLDM_ENULL, "afldm_dpm_step: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, AFLDM_ESHAPE, "afldm_dpm_step: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  const size_t n = (size_t)B * C * HW;
  const bool v4 = HW % 4 == 0 && aligned16(x) && aligned16(x_out) && aligned16(hist);
#define LAUNCH(T, V) (k_dpm_step<T, V><<<step_grid(n / V), 256, 0, st>>>(x, (const T*)eps, x_out, hist, coef, step_idx, B, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_dpm_step");
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_dpm_step");
}

extern "C" int afldm_dpm_step_flat(const float* x, const float* eps, float* x_out, float* hist, float p, float q, float a,
                                   float b0, float b1, float b2, size_t n, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && x_out && hist, AFLDM_ENULL, "afldm_dpm_step_flat: NULL pointer");
  if (n == 0) return AFLDM_OK;
  hipStream_t st = (hipStream_t)stream;
  const dpm_row c{p, q, a, b0, b1, b2};
  // the second history plane starts n floats in: 16-byte groups need n % 4 == 0 as well as aligned bases
  if (n % 4 == 0 && aligned16(x) && aligned16(eps) && aligned16(x_out) && aligned16(hist))
    k_dpm_step_flat<4><<<step_grid(n / 4), 256, 0, st>>>(x, eps, x_out, hist, c, n);
  else
    k_dpm_step_flat<1><<<step_grid(n), 256, 0, st>>>(x, eps, x_out, hist, c, n);
  return check_launch("afldm_dpm_step_flat");
}
