// ilvr.hip — ILVR reference-guided sampling (Choi et al., ICCV 2021, Algorithm 1) on the graph-replayed engine, with a linear
// low-pass phi given as two dense [S][S] matrices (the ideal low-pass LPF_RFFT(cutoff = 1 / N) as its circulant, or any other).
// Each UNet evaluation is one coefficient row (p, q, lo, hi, a, b, c, k0, k1, w, 0, 0) and two pre-drawn fp32 noise slots z_k, z_u:
//   x0    = clamp(p x + q eps, lo, hi)
//   xp    = a x0 + b eps + c z_u                 the unconditional proposal x'_{t-1}
//   yk    = k0 ref + k1 z_k                      the reference noised to the same level
//   x_out = xp + w (Lh (yk - xp) Lw^T)           per (b, c) plane; w = 0: x_out = xp
// This is the one sampler update that is not elementwise.  One 256-thread workgroup owns a (b, c) plane, S = H = W <= 64: it forms
// xp (kept in registers) and d = yk - xp (to LDS) for the whole plane, runs the row pass t = d Lw^T and the column pass Lh t out
// of LDS, and adds the result to xp.  Three S x P fp32 tiles (d / result, t, the matrix), P = S | 1: an odd row pitch puts the S
// rows a wave reads at one k (Lw[j][k], j = lane) on S different banks.  Every sum runs k = 0 .. S - 1 ascending in one fmaf
// chain per output: no atomics, no split reduction, so a plane's bits do not depend on B, on the grid or on the batch slice it
// arrived in.  All of a plane's global reads of x come before the first barrier and all stores after the last: x_out may alias x.
// Uniform branches (the row is the same for every thread): a slot whose coefficient (k1, c) is exactly 0 is not loaded, and with
// w = 0 neither are ref, z_k, Lh and Lw, and the two passes are skipped - the launch is then the plain stochastic step.
#include "plane_pass.hpp"

namespace afldm {

namespace {

struct ilvr_row {
  float p, q, lo, hi, a, b, c, k0, k1, w;
};

constexpr int ILVR_SMAX = PLANE_SMAX;
constexpr int ILVR_THREADS = PLANE_THREADS;

// One plane.  xpl / rpl / zk / zu / opl: the plane's S * S floats of x / ref / the two noise slots / x_out; ep: the plane's first
// eps element, es floats between pixels (NHWC: C; same layout as x: 1).  V = 4: S * S % 4 == 0 and 16-byte aligned planes.
template <typename T, int V>
__device__ __forceinline__ void ilvr_plane(const float* xpl, const T* __restrict__ ep, int es, const float* __restrict__ rpl,
                                           const float* __restrict__ zk, const float* __restrict__ zu,
                                           const float* __restrict__ Lh, const float* __restrict__ Lw, float* opl,
                                           const ilvr_row& r, int S, float* lds) {
  constexpr int MAXG = (ILVR_SMAX * ILVR_SMAX / V + ILVR_THREADS - 1) / ILVR_THREADS;
  const int tid = threadIdx.x;
  const int P = S | 1;
  const int groups = S * S / V;
  const bool has_k = r.k1 != 0.0f, has_u = r.c != 0.0f, guided = r.w != 0.0f;
  float* td = lds;                   // d, then the result of the column pass
  float* tt = lds + S * P;           // the row pass's output
  float* tm = lds + 2 * S * P;       // Lw, then Lh
  vecf<V> xp[MAXG];
#pragma unroll
  for (int u = 0; u < MAXG; ++u) {
    const int g = tid + u * ILVR_THREADS;
    if (g < groups) {
      const int i = g * V;
      const vecf<V> xv = ld<V>(xpl + i), zuv = ld_if<V>(has_u, zu + i);
      const vecf<V> rv = ld_if<V>(guided, rpl + i), zkv = ld_if<V>(guided && has_k, zk + i);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float e = to_f32(ep[(size_t)(i + k) * es]);
        const float x0 = clamp_nan(r.p * xv.v[k] + r.q * e, r.lo, r.hi);
        xp[u].v[k] = r.a * x0 + r.b * e + r.c * zuv.v[k];
        if (guided) {
          const float yk = r.k0 * rv.v[k] + r.k1 * zkv.v[k];
          const int row = (i + k) / S;
          td[row * P + (i + k - row * S)] = yk - xp[u].v[k];
        }
      }
    }
  }
  if (guided) {
    plane_load_matrix(Lw, tm, S, P, tid);
    __syncthreads();                                   // every read of x is behind us
    plane_pass(td, tm, P, 1, tt, S, P, tid);           // t[i][j] = sum_k d[i][k] Lw[j][k]
    __syncthreads();
    if (Lh != Lw) {                                    // (uniform; the same matrix twice is already there)
      plane_load_matrix(Lh, tm, S, P, tid);
      __syncthreads();
    }
    plane_pass(tm, tt, 1, P, td, S, P, tid);           // res[i][j] = sum_k Lh[i][k] t[k][j]
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < MAXG; ++u) {
    const int g = tid + u * ILVR_THREADS;
    if (g < groups) {
      const int i = g * V;
      if (guided) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const int row = (i + k) / S;
          xp[u].v[k] += r.w * td[row * P + (i + k - row * S)];
        }
      }
      st<V>(opl + i, xp[u]);
    }
  }
}

}  // namespace

// x, ref, x_out, noise slots NCHW fp32; eps NHWC T; one workgroup per (b, c) plane, blockIdx.x = b * C + c.
template <typename T, int V>
__global__ void __launch_bounds__(ILVR_THREADS) k_ilvr_step(const float* x, const T* __restrict__ eps, const float* __restrict__ ref,
                                                            const float* __restrict__ noise, size_t noise_step_stride,
                                                            size_t noise_slot_stride, const float* __restrict__ Lh,
                                                            const float* __restrict__ Lw, float* x_out,
                                                            const float* __restrict__ coef, const int* __restrict__ step_idx, int C,
                                                            int S) {
  extern __shared__ float ilvr_lds[];
  const int s = *step_idx;
  const float* rp = coef + 12 * (size_t)s;
  const ilvr_row r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8], rp[9]};
  const size_t plane = blockIdx.x, HW = (size_t)S * S;
  const size_t b = plane / C;
  const int ch = (int)(plane - b * C);
  const float* zk = noise + (size_t)s * noise_step_stride + plane * HW;
  ilvr_plane<T, V>(x + plane * HW, eps + b * HW * C + ch, C, ref + plane * HW, zk, zk + noise_slot_stride, Lh, Lw,
                   x_out + plane * HW, r, S, ilvr_lds);
}

// same-layout fp32 tensors, the row by value; a noise pointer is only read where its coefficient is not 0
template <int V>
__global__ void __launch_bounds__(ILVR_THREADS) k_ilvr_step_flat(const float* x, const float* __restrict__ eps,
                                                                 const float* __restrict__ ref, const float* __restrict__ zk,
                                                                 const float* __restrict__ zu, const float* __restrict__ Lh,
                                                                 const float* __restrict__ Lw, float* x_out, ilvr_row r, int S) {
  extern __shared__ float ilvr_lds[];
  const size_t o = (size_t)blockIdx.x * S * S;
  ilvr_plane<float, V>(x + o, eps + o, 1, ref + o, zk + o, zu + o, Lh, Lw, x_out + o, r, S, ilvr_lds);
}

static inline size_t ilvr_lds_bytes(int S) { return (size_t)3 * S * (S | 1) * sizeof(float); }

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_ilvr_step(const float* x, const void* eps, const float* ref, const float* noise, size_t noise_step_stride,
                               size_t noise_slot_stride, const float* Lh, const float* Lw, float* x_out, const float* coef,
                               int* step_idx, int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && ref && noise && Lh && Lw && x_out && coef && step_idx, AFLDM_ENULL, "afldm_ilvr_step: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, AFLDM_ESHAPE, "afldm_ilvr_step: bad shape");
  AFLDM_REQUIRE(H == W && H >= 2 && H <= ILVR_SMAX, AFLDM_ESHAPE,
                "afldm_ilvr_step: plane %d x %d (square planes of 2 .. %d only: one workgroup holds a plane in LDS)", H, W, ILVR_SMAX);
  AFLDM_REQUIRE((long long)B * C <= 0x7fffffffLL, AFLDM_ESHAPE, "afldm_ilvr_step: B * C = %lld planes exceed the grid",
                (long long)B * C);
  const int S = H;
  const size_t n = (size_t)B * C * S * S;
  AFLDM_REQUIRE(noise_slot_stride >= n, AFLDM_ESHAPE, "afldm_ilvr_step: noise_slot_stride smaller than one slot's B*C*H*W");
  AFLDM_REQUIRE(noise_step_stride >= noise_slot_stride + n, AFLDM_ESHAPE,
                "afldm_ilvr_step: noise_step_stride smaller than one step's two slots");
  hipStream_t st = (hipStream_t)stream;
  const int grid = B * C;
  const size_t lds = ilvr_lds_bytes(S);
  // every slot starts a multiple of the two strides after the base: 16-byte groups need both % 4 == 0 too
  const bool v4 = (S * S) % 4 == 0 && noise_step_stride % 4 == 0 && noise_slot_stride % 4 == 0 && aligned16(x) && aligned16(ref) &&
                  aligned16(x_out) && aligned16(noise);
#define LAUNCH(T, V)                                                                                                     \
  (k_ilvr_step<T, V><<<grid, ILVR_THREADS, lds, st>>>(x, (const T*)eps, ref, noise, noise_step_stride, noise_slot_stride, Lh, Lw, \
                                                      x_out, coef, step_idx, C, S))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_ilvr_step");
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_ilvr_step");
}

extern "C" int afldm_ilvr_step_flat(const float* x, const float* eps, const float* ref, const float* z_k, const float* z_u,
                                    const float* Lh, const float* Lw, float* x_out, float p, float q, float lo, float hi, float a,
                                    float b, float c, float k0, float k1, float w, size_t planes, int H, int W,
                                    afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && x_out, AFLDM_ENULL, "afldm_ilvr_step_flat: NULL pointer");
  AFLDM_REQUIRE(w == 0.0f || (ref && Lh && Lw), AFLDM_ENULL, "afldm_ilvr_step_flat: ref / Lh / Lw is NULL but w is not 0");
  AFLDM_REQUIRE((w == 0.0f || k1 == 0.0f || z_k) && (c == 0.0f || z_u), AFLDM_ENULL,
                "afldm_ilvr_step_flat: a noise slot with a non-zero coefficient is NULL");
  AFLDM_REQUIRE(H == W && H >= 2 && H <= ILVR_SMAX, AFLDM_ESHAPE,
                "afldm_ilvr_step_flat: plane %d x %d (square planes of 2 .. %d only: one workgroup holds a plane in LDS)", H, W,
                ILVR_SMAX);
  AFLDM_REQUIRE(planes <= 0x7fffffffULL, AFLDM_ESHAPE, "afldm_ilvr_step_flat: %zu planes exceed the grid", planes);
  if (planes == 0) return AFLDM_OK;
  hipStream_t st = (hipStream_t)stream;
  const int S = H;
  const ilvr_row r{p, q, lo, hi, a, b, c, k0, k1, w};
  const bool guided = w != 0.0f;
  const bool v4 = (S * S) % 4 == 0 && aligned16(x) && aligned16(x_out) && (!guided || aligned16(ref)) &&     // (eps: scalar reads)
                  (!guided || k1 == 0.0f || aligned16(z_k)) && (c == 0.0f || aligned16(z_u));
  if (v4)
    k_ilvr_step_flat<4><<<(int)planes, ILVR_THREADS, ilvr_lds_bytes(S), st>>>(x, eps, ref, z_k, z_u, Lh, Lw, x_out, r, S);
  else
    k_ilvr_step_flat<1><<<(int)planes, ILVR_THREADS, ilvr_lds_bytes(S), st>>>(x, eps, ref, z_k, z_u, Lh, Lw, x_out, r, S);
  return check_launch("afldm_ilvr_step_flat");
}
