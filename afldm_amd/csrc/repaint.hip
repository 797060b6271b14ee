// repaint.hip — RePaint inpainting (Lugmayr et al., CVPR 2022, Algorithm 1) on the graph-replayed engine, and the mask pooling
// that takes a pixel mask to the latent grid.  Each UNet evaluation is one coefficient row
// (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0) and three pre-drawn fp32 noise slots z_k, z_u, z_b:
//   x0      = clamp(p x + q eps, lo, hi)
//   unknown = a x0 + b eps + c z_u                 the reverse step of the generated part
//   knownp  = k0 known + k1 z_k                    the kept part, noised to the same level
//   y       = m knownp + (1 - m) unknown           m = mask[b, 0, h, w], 1 = keep
//   x_out   = u0 y + u1 z_b                        the jump back up the schedule (u1 = 0: none)
// A slot whose coefficient (k1, c, u1) is exactly 0 is not loaded (a uniform branch: the row is the same for every thread), so
// whatever an unused slot holds - zeros, stale memory, NaN - cannot reach the output.  The noise is drawn by the caller's
// generator outside the graph, as for sde.hip.  HBM-bound elementwise, laid out as sde.hip: every thread owns 4 consecutive
// pixels of one (b, c) plane (16-byte loads of x / known / mask / z, stores of x_out), grid capped at 2048 blocks and grid-stride
// beyond (guide G11).  Each thread reads and writes its own indices only, so x and x_out may alias.
#include "step_common.hpp"

namespace afldm {

namespace {

struct repaint_row {
  float p, q, lo, hi, a, b, c, k0, k1, u0, u1;
};

// zk / zu / zb: 0 where the slot is not loaded (its coefficient is 0 then, and the product an exact 0)
__device__ __forceinline__ float repaint_update(float x, float e, float kn, float m, float zk, float zu, float zb,
                                                const repaint_row& r) {
  const float x0 = clamp_nan(r.p * x + r.q * e, r.lo, r.hi);
  const float unknown = r.a * x0 + r.b * e + r.c * zu;
  const float knownp = r.k0 * kn + r.k1 * zk;
  const float y = m * knownp + (1.0f - m) * unknown;
  return r.u0 * y + r.u1 * zb;
}

}  // namespace

// x, known, x_out, noise slots NCHW fp32; mask [B][1][HW] fp32; eps NHWC T.  V = 4 needs HW % 4 == 0, both noise strides % 4 == 0
// and 16-byte aligned x / known / mask / x_out / noise.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_repaint_step(const float* x, const T* __restrict__ eps, const float* __restrict__ known,
                                                      const float* __restrict__ mask, const float* __restrict__ noise,
                                                      size_t noise_step_stride, size_t noise_slot_stride, float* x_out,
                                                      const float* __restrict__ coef, const int* __restrict__ step_idx, int B,
                                                      int C, int HW) {
  const int s = *step_idx;
  const float* rp = coef + 12 * (size_t)s;
  const repaint_row r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8], rp[9], rp[10]};
  const bool has_k = r.k1 != 0.0f, has_u = r.c != 0.0f, has_b = r.u1 != 0.0f;
  const float* zk = noise + (size_t)s * noise_step_stride;
  const float* zu = zk + noise_slot_stride;
  const float* zb = zu + noise_slot_stride;
  const size_t n = (size_t)B * C * HW;
  const size_t groups = n / V;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i = g * V;
    const nchw_pos at = nchw_at(i, C, HW);
    const T* ep = eps_at(eps, at, C, HW);
    const vecf<V> xv = ld<V>(x + i), kv = ld<V>(known + i), mv = ld<V>(mask + at.b * HW + at.pix);
    const vecf<V> zkv = ld_if<V>(has_k, zk + i), zuv = ld_if<V>(has_u, zu + i), zbv = ld_if<V>(has_b, zb + i);
    vecf<V> o;
#pragma unroll
    for (int k = 0; k < V; ++k)
      o.v[k] = repaint_update(xv.v[k], to_f32(ep[(size_t)k * C]), kv.v[k], mv.v[k], zkv.v[k], zuv.v[k], zbv.v[k], r);
    st<V>(x_out + i, o);
  }
}

// flat same-layout fp32 tensors (the mask too), the row by value; a noise pointer is only read where its coefficient is not 0.
// 16-byte groups, then a scalar tail.
template <int V>
__global__ void __launch_bounds__(256) k_repaint_step_flat(const float* x, const float* __restrict__ eps,
                                                           const float* __restrict__ known, const float* __restrict__ mask,
                                                           const float* __restrict__ zk, const float* __restrict__ zu,
                                                           const float* __restrict__ zb, float* x_out, repaint_row r, size_t n) {
  const bool has_k = r.k1 != 0.0f, has_u = r.c != 0.0f, has_b = r.u1 != 0.0f;
  const size_t groups = n / V;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t g = tid; g < groups; g += stride) {
    const size_t i = g * V;
    const vecf<V> xv = ld<V>(x + i), ev = ld<V>(eps + i), kv = ld<V>(known + i), mv = ld<V>(mask + i);
    const vecf<V> zkv = ld_if<V>(has_k, zk + i), zuv = ld_if<V>(has_u, zu + i), zbv = ld_if<V>(has_b, zb + i);
    vecf<V> o;
#pragma unroll
    for (int k = 0; k < V; ++k) o.v[k] = repaint_update(xv.v[k], ev.v[k], kv.v[k], mv.v[k], zkv.v[k], zuv.v[k], zbv.v[k], r);
    st<V>(x_out + i, o);
  }
  for (size_t i = groups * V + tid; i < n; i += stride)
    x_out[i] = repaint_update(x[i], eps[i], known[i], mask[i], has_k ? zk[i] : 0.0f, has_u ? zu[i] : 0.0f, has_b ? zb[i] : 0.0f, r);
}

// mask [B][1][H][W] -> out [B][1][H / r][W / r]: one thread per output, the r x r block under it.  MEAN = false: the minimum
// (a latent is kept only if every pixel under it is); MEAN = true: the mean, summed in fp64 (correctly rounded for any r a mask
// has) and rounded once.  A NaN in the block comes out as NaN in both modes.
template <bool MEAN>
__global__ void __launch_bounds__(256) k_mask_pool(const float* __restrict__ mask, float* __restrict__ out, size_t total, int Ho,
                                                   int Wo, int W, int r) {
  for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
    const int wo = (int)(o % Wo);
    const size_t t = o / Wo;
    const int ho = (int)(t % Ho);
    const size_t b = t / Ho;
    const float* src = mask + ((b * Ho + ho) * (size_t)r) * W + (size_t)wo * r;
    if constexpr (MEAN) {
      double acc = 0.0;
      for (int i = 0; i < r; ++i)
        for (int j = 0; j < r; ++j) acc += (double)src[(size_t)i * W + j];
      out[o] = (float)(acc / ((double)r * (double)r));
    } else {
      float acc = src[0];
      for (int i = 0; i < r; ++i)
        for (int j = 0; j < r; ++j) {
          const float v = src[(size_t)i * W + j];
          acc = (v < acc || v != v) ? v : acc;
        }
      out[o] = acc;
    }
  }
}

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_repaint_step(const float* x, const void* eps, const float* known, const float* mask, const float* noise,
                                  size_t noise_step_stride, size_t noise_slot_stride, float* x_out, const float* coef,
                                  int* step_idx, int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && known && mask && noise && x_out && coef && step_idx, AFLDM_ENULL, "afldm_repaint_step: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, AFLDM_ESHAPE, "afldm_repaint_step: bad shape");
  const int HW = H * W;
  const size_t n = (size_t)B * C * HW;
  AFLDM_REQUIRE(noise_slot_stride >= n, AFLDM_ESHAPE, "afldm_repaint_step: noise_slot_stride smaller than one slot's B*C*H*W");
  AFLDM_REQUIRE(noise_step_stride >= 2 * noise_slot_stride + n, AFLDM_ESHAPE,
                "afldm_repaint_step: noise_step_stride smaller than one step's three slots");
  hipStream_t st = (hipStream_t)stream;
  // every slot starts a multiple of the two strides after the base: 16-byte groups need both % 4 == 0 too
  const bool v4 = HW % 4 == 0 && noise_step_stride % 4 == 0 && noise_slot_stride % 4 == 0 && aligned16(x) && aligned16(known) &&
                  aligned16(mask) && aligned16(x_out) && aligned16(noise);
#define LAUNCH(T, V)                                                                                                \
  (k_repaint_step<T, V><<<step_grid(n / V), 256, 0, st>>>(x, (const T*)eps, known, mask, noise, noise_step_stride, \
                                                          noise_slot_stride, x_out, coef, step_idx, B, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_repaint_step");
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_repaint_step");
}

extern "C" int afldm_repaint_step_flat(const float* x, const float* eps, const float* known, const float* mask, const float* z_k,
                                       const float* z_u, const float* z_b, float* x_out, float p, float q, float lo, float hi,
                                       float a, float b, float c, float k0, float k1, float u0, float u1, size_t n,
                                       afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && known && mask && x_out, AFLDM_ENULL, "afldm_repaint_step_flat: NULL pointer");
  AFLDM_REQUIRE((k1 == 0.0f || z_k) && (c == 0.0f || z_u) && (u1 == 0.0f || z_b), AFLDM_ENULL,
                "afldm_repaint_step_flat: a noise slot with a non-zero coefficient is NULL");
  if (n == 0) return AFLDM_OK;
  hipStream_t st = (hipStream_t)stream;
  const repaint_row r{p, q, lo, hi, a, b, c, k0, k1, u0, u1};
  const bool v4 = aligned16(x) && aligned16(eps) && aligned16(known) && aligned16(mask) && aligned16(x_out) &&
                  (k1 == 0.0f || aligned16(z_k)) && (c == 0.0f || aligned16(z_u)) && (u1 == 0.0f || aligned16(z_b));
  if (v4)
    k_repaint_step_flat<4><<<step_grid(n / 4), 256, 0, st>>>(x, eps, known, mask, z_k, z_u, z_b, x_out, r, n);
  else
    k_repaint_step_flat<1><<<step_grid(n), 256, 0, st>>>(x, eps, known, mask, z_k, z_u, z_b, x_out, r, n);
  return check_launch("afldm_repaint_step_flat");
}

extern "C" int afldm_mask_pool(const float* mask, float* out, int B, int H, int W, int r, int mode, afldm_stream_t stream) {
  AFLDM_REQUIRE(mask && out, AFLDM_ENULL, "afldm_mask_pool: NULL pointer");
  AFLDM_REQUIRE(B > 0 && H > 0 && W > 0, AFLDM_ESHAPE, "afldm_mask_pool: bad shape");
  AFLDM_REQUIRE(r >= 1 && H % r == 0 && W % r == 0, AFLDM_ESHAPE, "afldm_mask_pool: r = %d must be >= 1 and divide H = %d and W = %d",
                r, H, W);
  AFLDM_REQUIRE(mode == AFLDM_MASK_MIN || mode == AFLDM_MASK_MEAN, AFLDM_ESHAPE, "afldm_mask_pool: mode %d (0 = min, 1 = mean)", mode);
  hipStream_t st = (hipStream_t)stream;
  const int Ho = H / r, Wo = W / r;
  const size_t total = (size_t)B * Ho * Wo;
  if (mode == AFLDM_MASK_MEAN)
    k_mask_pool<true><<<step_grid(total), 256, 0, st>>>(mask, out, total, Ho, Wo, W, r);
  else
    k_mask_pool<false><<<step_grid(total), 256, 0, st>>>(mask, out, total, Ho, Wo, W, r);
  return check_launch("afldm_mask_pool");
}
