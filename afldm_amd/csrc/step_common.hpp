// step_common.hpp — what the sampler-update kernels (dpm, sde, repaint, sdedit, ilvr, pag, pano, hires .hip) share.  Everything here has internal
// linkage: every .hip file is its own translation unit and there is no relocatable device code, so each gets its own copy.
#pragma once
#include "common.hpp"

namespace afldm {

namespace {

// clamp that keeps a NaN a NaN (as torch.clamp does); fmaxf / fminf would turn it into a bound.  lo = -inf, hi = +inf: no clip.
__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// V consecutive floats: V = 4 as one 16-byte access (the pointer 16-byte aligned), V = 1 scalar
template <int V>
struct vecf {
  float v[V];
};

template <int V>
__device__ __forceinline__ vecf<V> ld(const float* p) {
  vecf<V> r;
  if constexpr (V == 4) {
    f32x4 q = *reinterpret_cast<const f32x4*>(p);
    r.v[0] = q[0]; r.v[1] = q[1]; r.v[2] = q[2]; r.v[3] = q[3];
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = p[k];
  }
  return r;
}

// zeros where `on` is false (uniform: a noise slot whose coefficient is 0 is not loaded)
template <int V>
__device__ __forceinline__ vecf<V> ld_if(bool on, const float* p) {
  if (on) return ld<V>(p);
  vecf<V> r;
#pragma unroll
  for (int k = 0; k < V; ++k) r.v[k] = 0.0f;
  return r;
}

template <int V>
__device__ __forceinline__ void st(float* p, const vecf<V>& r) {
  if constexpr (V == 4) {
    f32x4 q = {r.v[0], r.v[1], r.v[2], r.v[3]};
    *reinterpret_cast<f32x4*>(p) = q;
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) p[k] = r.v[k];
  }
}

// Element i of an NCHW [B, C, HW] tensor as (b, ch, pix), and the same element of NHWC eps; the next pixel lies C further on.
struct nchw_pos {
  size_t b;
  int ch, pix;
};

__device__ __forceinline__ nchw_pos nchw_at(size_t i, int C, int HW) {
  const int pix = (int)(i % HW);
  const size_t plane = i / HW;
  const int ch = (int)(plane % C);
  const size_t b = plane / C;
  return {b, ch, pix};
}

template <typename T>
__device__ __forceinline__ const T* eps_at(const T* eps, const nchw_pos& at, int C, int HW) {
  return eps + ((size_t)at.b * HW + at.pix) * C + at.ch;
}

// blocks of 256 threads for `work` items, capped at 2048 (grid-stride beyond: guide G11)
inline int step_grid(size_t work) {
  size_t g = (work + 255) / 256;
  return (int)(g < 2048 ? (g ? g : 1) : 2048);
}

// the step counter's increment for an update launched with advance != 0 (the engine's steps advance in select_step_row instead)
__global__ void k_step_advance(int* step_idx) { *step_idx += 1; }

inline void step_advance(int advance, int* step_idx, hipStream_t st) {
  if (advance) k_step_advance<<<1, 1, 0, st>>>(step_idx);
}

}  // namespace

}  // namespace afldm

// The {fp32, bf16} x {V = 4, V = 1} launch of a step kernel: LAUNCH(T, V) is the call site's launch expression for eps of type T.
#define STEP_DISPATCH(dtype, wide, LAUNCH, name)                             \
  do {                                                                       \
    if (wide)                                                                \
      DISPATCH_T(dtype, LAUNCH(float, 4), LAUNCH(bf16, 4), name);            \
    else                                                                     \
      DISPATCH_T(dtype, LAUNCH(float, 1), LAUNCH(bf16, 1), name);            \
  } while (0)
