// rev.hip — the bit-reversible sampler's update: a two-step (leapfrog) DDIM, after BDIA (Zhang et al., ECCV 2024) at gamma = 1,
// on latents carried as 64-bit fixed point (grid 2^-32, Q31.32), the way bit-reversible molecular-dynamics integrators carry
// positions (Levesque & Verlet 1993).  Each UNet evaluation is one coefficient row (cx, ce, sign, boot) on a pair (far, near):
//   f = boot ? near : far;  n = near;  x = rn_f32(n) 2^-32;  d = fl32(fl32(cx x) + fl32(ce e));  q = rn_i64(d 2^32)
//   new = f + sign q;  far <- n;  near <- new;  lat <- rn_f32(new) 2^-32
// q is a function of `near` and eps(near) alone, so the same row with the opposite sign, fed the rotated pair, subtracts the very
// integer that was added: the step is undone bit for bit.  The float operations are spelled out - two products, one sum, no fma,
// contraction off - so that a numpy fp32 restatement has the same bits; both scales are powers of two and exact.  Trouble (a
// non-finite d, |d 2^32| >= 2^63, signed overflow of the add) makes q = 0 for that element and stores 1 into bad[sample]: a plain
// store, every writer writes the same value.  HBM-bound elementwise: every thread owns two consecutive elements (16-byte loads
// and stores of far / near, 8-byte stores of lat) where the count is even and the pointers are aligned, else one; grid capped at
// 2048 blocks and grid-stride beyond (guide G11).  Each thread reads and writes its own indices only.
#include "step_common.hpp"

namespace afldm {

namespace {

typedef long long i64;
typedef __attribute__((ext_vector_type(2))) long long i64x2;

struct rev_row {
  float cx, ce;
  int sign, boot;          // sign: +1 / -1; boot: the first step from a single state reads `near` in far's place
};

__device__ __forceinline__ float rev_decode(i64 X) { return (float)X * 0x1p-32f; }          // one RNE rounding, then exact

// (far, near, e) -> the new near; *trouble is set where q was forced to 0
__device__ __forceinline__ i64 rev_update(i64 f, i64 n, float e, const rev_row& r, bool* trouble) {
#pragma clang fp contract(off)
  const float x = rev_decode(n);
  const float a = r.cx * x;
  const float b = r.ce * e;
  const float d = a + b;
  const float v = d * 0x1p32f;                                     // exact, or +-inf
  const bool ok = __builtin_isfinite(d) && __builtin_fabsf(v) < 0x1p63f;
  const i64 q = ok ? (i64)__builtin_rintf(v) : 0;                  // |q| < 2^63: the negation below cannot overflow
  i64 nw;
  const bool over = __builtin_add_overflow(f, r.sign < 0 ? -q : q, &nw);
  *trouble = !ok || over;
  return over ? f : nw;
}

template <int V>
__device__ __forceinline__ void ld_i64(const i64* p, i64* out) {
  if constexpr (V == 2) {
    const i64x2 t = *reinterpret_cast<const i64x2*>(p);
    out[0] = t[0]; out[1] = t[1];
  } else {
    out[0] = p[0];
  }
}

template <int V>
__device__ __forceinline__ void st_i64(i64* p, const i64* v) {
  if constexpr (V == 2) {
    const i64x2 t = {v[0], v[1]};
    *reinterpret_cast<i64x2*>(p) = t;
  } else {
    p[0] = v[0];
  }
}

template <int V>
__device__ __forceinline__ void st_lat(float* p, const float* v) {
  if constexpr (V == 2) {
    const f32x2 t = {v[0], v[1]};
    *reinterpret_cast<f32x2*>(p) = t;
  } else {
    p[0] = v[0];
  }
}

// the part of the update both kernels share, once the V eps values are in registers; bit k of the result: element k had trouble
template <int V>
__device__ __forceinline__ unsigned rev_group(i64* far, i64* near, float* lat, size_t i, const float* e, const rev_row& r) {
  i64 f[V], n[V], nw[V];
  float l[V];
  ld_i64<V>(near + i, n);
  if (r.boot) {
#pragma unroll
    for (int k = 0; k < V; ++k) f[k] = n[k];
  } else {
    ld_i64<V>(far + i, f);
  }
  unsigned any = 0;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    bool t;
    nw[k] = rev_update(f[k], n[k], e[k], r, &t);
    l[k] = rev_decode(nw[k]);
    any |= (unsigned)t << k;
  }
  st_i64<V>(far + i, n);          // (far first: where the flat boot step passes one buffer for both, `new` is what stays)
  st_i64<V>(near + i, nw);
  st_lat<V>(lat + i, l);
  return any;
}

}  // namespace

// far, near int64 NCHW [B,C,HW]; lat fp32 NCHW; eps NHWC T; bad int32 [B].  V = 2 needs C*HW even (a pair then lies in one sample)
// and far / near 16-byte, lat 8-byte aligned.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_rev_step(i64* far, i64* near, const T* __restrict__ eps, float* lat, int* bad,
                                                  const float* __restrict__ coef, const int* __restrict__ step_idx, int B, int C,
                                                  int HW) {
  const float* rp = coef + 4 * (size_t)*step_idx;
  const rev_row r{rp[0], rp[1], rp[2] < 0.0f ? -1 : 1, rp[3] != 0.0f};
  const size_t n = (size_t)B * C * HW;
  const size_t groups = n / V;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i = g * V;
    const nchw_pos at = nchw_at(i, C, HW);
    float e[V];
    e[0] = to_f32(*eps_at(eps, at, C, HW));
    if constexpr (V == 2)          // the next element: the next pixel of the plane, or (HW odd) the first of the next plane
      e[1] = to_f32(at.pix + 1 < HW ? eps_at(eps, at, C, HW)[C] : *eps_at(eps, nchw_at(i + 1, C, HW), C, HW));
    if (rev_group<V>(far, near, lat, i, e, r)) bad[at.b] = 1;
  }
}

// flat same-layout tensors, the row by value: 16-byte groups, then a scalar tail
template <int V>
__global__ void __launch_bounds__(256) k_rev_step_flat(i64* far, i64* near, const float* __restrict__ eps, float* lat, int* bad,
                                                       rev_row r, size_t n, size_t per) {
  const size_t groups = n / V;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t g = tid; g < groups; g += stride) {
    const size_t i = g * V;
    float e[V];
#pragma unroll
    for (int k = 0; k < V; ++k) e[k] = eps[i + k];
    const unsigned t = rev_group<V>(far, near, lat, i, e, r);
#pragma unroll
    for (int k = 0; k < V; ++k)          // (a pair may straddle two samples where `per` is odd)
      if (t >> k & 1) bad[(i + k) / per] = 1;
  }
  for (size_t i = groups * V + tid; i < n; i += stride) {
    const float e = eps[i];
    if (rev_group<1>(far, near, lat, i, &e, r)) bad[i / per] = 1;
  }
}

// X = rn_i64(x 2^32): the product is exact; a non-finite x or |x| >= 2^31 gives X = 0 and bad[i / per] = 1
__global__ void __launch_bounds__(256) k_rev_encode(const float* __restrict__ x, i64* X, int* bad, size_t n, size_t per) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    const bool ok = __builtin_isfinite(v) && __builtin_fabsf(v) < 0x1p31f;
    X[i] = ok ? (i64)__builtin_rintf(v * 0x1p32f) : 0;
    if (!ok) bad[i / per] = 1;
  }
}

static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_rev_step(long long* far, long long* near, const void* eps, float* lat_out, int* bad, const float* coef,
                              int* step_idx, int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(far && near && eps && lat_out && bad && coef && step_idx, AFLDM_ENULL, "afldm_rev_step: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, AFLDM_ESHAPE, "afldm_rev_step: bad shape");
  AFLDM_REQUIRE(aligned8(far) && aligned8(near), AFLDM_EALIGN, "afldm_rev_step: far / near must be 8-byte aligned");
  AFLDM_REQUIRE(far != near, AFLDM_ESHAPE, "afldm_rev_step: far and near are one buffer (only afldm_rev_step_flat with boot takes that)");
  const int HW = H * W;
  const size_t n = (size_t)B * C * HW;
  hipStream_t st = (hipStream_t)stream;
  const bool v2 = ((size_t)C * HW) % 2 == 0 && aligned16(far) && aligned16(near) && aligned8(lat_out);
#define LAUNCH(T, V) (k_rev_step<T, V><<<step_grid(n / V), 256, 0, st>>>(far, near, (const T*)eps, lat_out, bad, coef, step_idx, B, C, HW))
  if (v2) {          // (STEP_DISPATCH with the wide form two int64, not four floats: 16 bytes either way)
    DISPATCH_T(dtype, LAUNCH(float, 2), LAUNCH(bf16, 2), "afldm_rev_step");
  } else {
    DISPATCH_T(dtype, LAUNCH(float, 1), LAUNCH(bf16, 1), "afldm_rev_step");
  }
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_rev_step");
}

extern "C" int afldm_rev_step_flat(long long* far, long long* near, const float* eps, float* lat_out, int* bad, float cx, float ce,
                                   int sign, int boot, size_t n, size_t rows_per_sample, afldm_stream_t stream) {
  AFLDM_REQUIRE(far && near && eps && lat_out && bad, AFLDM_ENULL, "afldm_rev_step_flat: NULL pointer");
  AFLDM_REQUIRE(sign == 1 || sign == -1, AFLDM_ESHAPE, "afldm_rev_step_flat: sign must be +1 or -1");
  AFLDM_REQUIRE(rows_per_sample > 0, AFLDM_ESHAPE, "afldm_rev_step_flat: rows_per_sample must be positive");
  AFLDM_REQUIRE(aligned8(far) && aligned8(near), AFLDM_EALIGN, "afldm_rev_step_flat: far / near must be 8-byte aligned");
  AFLDM_REQUIRE(far != near || boot, AFLDM_ESHAPE, "afldm_rev_step_flat: far and near are one buffer, which only a boot step takes");
  if (n == 0) return AFLDM_OK;
  hipStream_t st = (hipStream_t)stream;
  const rev_row r{cx, ce, sign, boot != 0};
  if (aligned16(far) && aligned16(near) && aligned8(lat_out))
    k_rev_step_flat<2><<<step_grid(n / 2), 256, 0, st>>>(far, near, eps, lat_out, bad, r, n, rows_per_sample);
  else
    k_rev_step_flat<1><<<step_grid(n), 256, 0, st>>>(far, near, eps, lat_out, bad, r, n, rows_per_sample);
  return check_launch("afldm_rev_step_flat");
}

extern "C" int afldm_rev_encode(const float* x, long long* X, int* bad, size_t n, size_t per_sample, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && X && bad, AFLDM_ENULL, "afldm_rev_encode: NULL pointer");
  AFLDM_REQUIRE(per_sample > 0, AFLDM_ESHAPE, "afldm_rev_encode: per_sample must be positive");
  AFLDM_REQUIRE(aligned8(X), AFLDM_EALIGN, "afldm_rev_encode: X must be 8-byte aligned");
  if (n == 0) return AFLDM_OK;
  k_rev_encode<<<step_grid(n), 256, 0, (hipStream_t)stream>>>(x, X, bad, n, per_sample);
  return check_launch("afldm_rev_encode");
}
