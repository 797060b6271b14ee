// sag.hip — self-attention guidance (Hong et al., ICCV 2023; diffusers StableDiffusionSAGPipeline) on the graph-replayed engine.
// SAG reads the attention map of one self-attention site and blurs the predicted x0 where the map says "salient".  Two things
// the library had no entry point for:
//
// 1. afldm_attn_key_mass — the attention mass each KEY receives,
//      mass[b, j] = (1 / heads) sum_h sum_i softmax_j(scale q_bhi . k_bhj),
//    a column reduction of the T x T probabilities, which never exist in memory.  Two launches:
//      k_km_stats  a wave owns 16 * QTW query rows of one (b, h): S = Q K^T on MFMA (fp32 accumulation), a first sweep over the key
//                  tiles for the row maximum, a second for the row sum of exp(scale s - max), evaluated as 2^(c2 s - c2 max)
//                  with c2 = scale log2(e): one fma and one v_exp_f32 per score; (c2 max, 1 / sum) per query go to the
//                  workspace.  Two sweeps instead of a running rescale: one exponential per score, and no rescale rounding.
//      k_km_mass   a workgroup owns 16 * KTW keys of one sample and walks every (head, query tile) on the TRANSPOSED product
//                  K Q^T, so that a lane holds 4 keys x 1 query and the column sums of P are lane-local running sums.  Per head
//                  the four waves take the query tiles round-robin; their partial sums meet in LDS in a fixed order.
//    Operands: bf16 goes to v_mfma_f32_16x16x32_bf16 with the head's d columns zero-padded to 32 (bf16 products are exact in
//    fp32), fp32 to d / 4 v_mfma_f32_16x16x4_f32.  Behind the operand reads everything is fp32; probabilities are neither
//    rounded to bf16 nor stored.  No atomics, every sum in a fixed order, a workgroup never spans two samples: a sample's bits
//    depend neither on B nor on its place in the batch.
//
// 2. afldm_sag_degrade / afldm_sag_degrade_flat — the whole degradation in one launch, one workgroup per (b, c) plane:
//      x0 = p x + q e  -> LDS;  G x0 by a horizontal and a vertical pass out of LDS ("reflect" or circular boundary);
//      M = mass > 1 read through the integer ratio r = H / hm;   x_d = M ? x + (G x0 - x0) / p : x.
//    The engine form reads x NCHW fp32 and e NHWC in the model dtype, takes (p, q) from the device coefficient table and writes
//    x_d NHWC in the model dtype (the UNet's next input); the flat form is all NCHW fp32 with (p, q) by value.  One device
//    function, one arithmetic order: with fp32 everywhere the two agree bit for bit.  The taps travel by value (a captured
//    graph keeps them) and are copied to LDS first, so that the tap loops index LDS and not the argument block.
#include "common.hpp"

namespace afldm {

namespace {

// ------------------------------------------------------------------------------------------------ key mass
// One lane's share of a 16-row operand tile for one head: lane (li = lane & 15, g = lane >> 4) holds row li, and of the head's D
// columns the set its k-slot g covers.  Any split of the columns over the k-slots is legal as long as both operands use the same.
template <typename T, int D>
struct KmFrag;

template <int D>
struct KmFrag<float, D> {
  static constexpr int N = D / 4;      // columns per lane: [N g, N g + N)
  float f[N];
  __device__ __forceinline__ void load(const float* __restrict__ row, int g, bool ok) {
#pragma unroll
    for (int e = 0; e < N; e += 2) {
      f32x2 v = {0.f, 0.f};
      if (ok) v = *reinterpret_cast<const f32x2*>(row + N * g + e);      // (8-byte aligned: ld, D and N are even)
      f[e] = v[0];
      f[e + 1] = v[1];
    }
  }
  static __device__ __forceinline__ void mma(f32x4& acc, const KmFrag& a, const KmFrag& b) {
#pragma unroll
    for (int e = 0; e < N; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.f[e], b.f[e], acc, 0, 0, 0);
  }
};

template <int D>
struct KmFrag<bf16, D> {
  bf16x8 c;      // columns [8 g, 8 g + 8), zero past D
  __device__ __forceinline__ void load(const bf16* __restrict__ row, int g, bool ok) {
    c = Mma<bf16>::zero();
    if (ok && 8 * g < D) c = ld16<bf16x8>(row + 8 * g);      // (16-byte aligned: ld and D are multiples of 8)
  }
  static __device__ __forceinline__ void mma(f32x4& acc, const KmFrag& a, const KmFrag& b) { Mma<bf16>::mma(acc, a.c, b.c); }
};

// (max, 1 / sum) of every softmax row.  st: [B, heads, T] pairs.
template <typename T, int D, int QTW>
__global__ void __launch_bounds__(256) k_km_stats(const T* __restrict__ q, int ldq, const T* __restrict__ k, int ldk,
                                                  float* __restrict__ st, int B, int heads, int Tn, float c2) {
  typedef KmFrag<T, D> Frag;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int nQB = (Tn + 16 * QTW - 1) / (16 * QTW);
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)B * heads * nQB) return;      // (no barrier in this kernel)
  const int qb = (int)(item % nQB);
  const int bh = (int)(item / nQB);
  const int h = bh % heads, b = bh / heads;
  const int q0 = qb * 16 * QTW;
  const T* qbase = q + (size_t)b * Tn * ldq + h * D;
  const T* kbase = k + (size_t)b * Tn * ldk + h * D;
  Frag qf[QTW];
#pragma unroll
  for (int u = 0; u < QTW; ++u) {
    const int row = q0 + 16 * u + li;
    qf[u].load(qbase + (size_t)(row < Tn ? row : 0) * ldq, g, row < Tn);
  }
  const int nKT = (Tn + 15) / 16;
  float m[QTW][4], l[QTW][4];
#pragma unroll
  for (int u = 0; u < QTW; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[u][r] = -INFINITY;
      l[u][r] = 0.f;
    }
  // sweep 1: the row maxima of the raw products (c2 > 0: the maximum commutes with the scaling).  D on lane (li, g):
  // S[query 4 g + r][key li]
#pragma unroll 2
  for (int kt = 0; kt < nKT; ++kt) {
    const int row = kt * 16 + li;
    const bool ok = row < Tn;
    Frag kf;
    kf.load(kbase + (size_t)(ok ? row : 0) * ldk, g, ok);
#pragma unroll
    for (int u = 0; u < QTW; ++u) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      Frag::mma(acc, qf[u], kf);
      if (ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) m[u][r] = fmaxf(m[u][r], acc[r]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < QTW; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) m[u][r] = fmaxf(m[u][r], __shfl_xor(m[u][r], o, 64));      // (xor < 16: the lanes of one g)
      m[u][r] *= c2;      // the maximum in the exponent's units: scale log2(e) max_j q.k
    }
  // sweep 2: the row sums of 2^(c2 q.k - max): one fma and one v_exp_f32 per score
#pragma unroll 2
  for (int kt = 0; kt < nKT; ++kt) {
    const int row = kt * 16 + li;
    const bool ok = row < Tn;
    Frag kf;
    kf.load(kbase + (size_t)(ok ? row : 0) * ldk, g, ok);
#pragma unroll
    for (int u = 0; u < QTW; ++u) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      Frag::mma(acc, qf[u], kf);
      if (ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) l[u][r] += __builtin_amdgcn_exp2f(fmaf(acc[r], c2, -m[u][r]));
      }
    }
  }
#pragma unroll
  for (int u = 0; u < QTW; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) l[u][r] += __shfl_xor(l[u][r], o, 64);
      const int row = q0 + 16 * u + 4 * g + r;
      if (li == 0 && row < Tn)
        *reinterpret_cast<f32x2*>(st + (((size_t)b * heads + h) * Tn + row) * 2) = f32x2{m[u][r], 1.0f / l[u][r]};
    }
}

template <typename T, int D, int KTW>
__global__ void __launch_bounds__(256) k_km_mass(const T* __restrict__ q, int ldq, const T* __restrict__ k, int ldk,
                                                 const float* __restrict__ st, float* __restrict__ mass, int heads, int Tn,
                                                 float c2) {
  typedef KmFrag<T, D> Frag;
  __shared__ float red[4][KTW * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int nKB = (Tn + 16 * KTW - 1) / (16 * KTW);
  const int b = blockIdx.x / nKB, kb = blockIdx.x - b * nKB;
  const int k0 = kb * 16 * KTW;
  const int nQT = (Tn + 15) / 16;
  const T* qbase = q + (size_t)b * Tn * ldq;
  const T* kbase = k + (size_t)b * Tn * ldk;
  float acc[KTW][4];
#pragma unroll
  for (int u = 0; u < KTW; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[u][r] = 0.f;
#pragma unroll 2
  for (int h = 0; h < heads; ++h) {      // ascending (head, query tile): a fixed order per wave
    Frag kf[KTW];
#pragma unroll
    for (int u = 0; u < KTW; ++u) {
      const int row = k0 + 16 * u + li;
      kf[u].load(kbase + (size_t)(row < Tn ? row : 0) * ldk + h * D, g, row < Tn);
    }
    const float* sth = st + ((size_t)b * heads + h) * Tn * 2;
#pragma unroll 2
    for (int qt = wave; qt < nQT; qt += 4) {
      const int qrow = qt * 16 + li;
      const bool qok = qrow < Tn;
      Frag qf;
      qf.load(qbase + (size_t)(qok ? qrow : 0) * ldq + h * D, g, qok);
      f32x2 ms = {0.f, 0.f};      // an absent query: 2^(0 - 0) * 0
      if (qok) ms = *reinterpret_cast<const f32x2*>(sth + (size_t)qrow * 2);
#pragma unroll
      for (int u = 0; u < KTW; ++u) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        Frag::mma(s, kf[u], qf);      // D on lane (li, g): S^T[key 4 g + r][query li]
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[u][r] = fmaf(__builtin_amdgcn_exp2f(fmaf(s[r], c2, -ms[0])), ms[1], acc[u][r]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < KTW; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) acc[u][r] += __shfl_xor(acc[u][r], o, 64);
      if (li == 0) red[wave][16 * u + 4 * g + r] = acc[u][r];
    }
  __syncthreads();
  if (tid < KTW * 16) {
    const int key = k0 + tid;
    if (key < Tn) mass[(size_t)b * Tn + key] = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) / (float)heads;
  }
}

static bool key_mass_shape_ok(int B, int heads, int T, int d, int dtype) {
  if ((dtype != AFLDM_BF16 && dtype != AFLDM_F32) || B <= 0 || heads <= 0) return false;
  if (T != 4 && T != 16 && T != 64 && T != 256 && T != 1024) return false;
  if (d != 8 && d != 16 && d != 24 && d != 32) return false;
  return (long long)B * heads * T < (1ll << 28);
}

template <typename T, int D>
static int launch_key_mass(const T* q, int ldq, const T* k, int ldk, float* mass, float* st, int B, int heads, int Tn, float scale,
                           hipStream_t stream) {
  const float c2 = scale * 1.4426950408889634f;      // exp(scale s) = 2^(c2 s)
  if (Tn >= 64) {
    k_km_stats<T, D, 2><<<cdiv((long long)B * heads * (Tn / 32), 4), 256, 0, stream>>>(q, ldq, k, ldk, st, B, heads, Tn, c2);
    k_km_mass<T, D, 4><<<B * (Tn / 64), 256, 0, stream>>>(q, ldq, k, ldk, st, mass, heads, Tn, c2);
  } else {
    k_km_stats<T, D, 1><<<cdiv((long long)B * heads, 4), 256, 0, stream>>>(q, ldq, k, ldk, st, B, heads, Tn, c2);
    k_km_mass<T, D, 1><<<B, 256, 0, stream>>>(q, ldq, k, ldk, st, mass, heads, Tn, c2);
  }
  return check_launch("afldm_attn_key_mass");
}

template <typename T>
static int dispatch_key_mass(const T* q, int ldq, const T* k, int ldk, float* mass, float* st, int B, int heads, int Tn, int d,
                             float scale, hipStream_t stream) {
  switch (d) {
    case 8: return launch_key_mass<T, 8>(q, ldq, k, ldk, mass, st, B, heads, Tn, scale, stream);
    case 16: return launch_key_mass<T, 16>(q, ldq, k, ldk, mass, st, B, heads, Tn, scale, stream);
    case 24: return launch_key_mass<T, 24>(q, ldq, k, ldk, mass, st, B, heads, Tn, scale, stream);
    default: return launch_key_mass<T, 32>(q, ldq, k, ldk, mass, st, B, heads, Tn, scale, stream);
  }
}

// ------------------------------------------------------------------------------------------------ degradation
constexpr int SAG_MAX_TAPS = 15;
constexpr int SAG_MAX_SIDE = 64;

struct SagTaps {
  float w[SAG_MAX_TAPS];
};

// index i + off of an axis of H elements, |off| < H: "reflect" (no edge repeat, F.pad mode='reflect') or circular
__device__ __forceinline__ int sag_index(int i, int H, int boundary) {
  if (boundary) return i < 0 ? i + H : (i >= H ? i - H : i);
  return i < 0 ? -i : (i >= H ? 2 * (H - 1) - i : i);
}

// One (b, c) plane.  Element pix = y * H + x of x lies at xp[pix], of e at ep[pix * es], of x_d at op[pix * os]; mrow: the
// sample's hm * hm masses.  s0, s1: H * H floats of LDS each, sw: the taps.
template <typename T>
__device__ __forceinline__ void sag_plane(const float* __restrict__ xp, const T* __restrict__ ep, size_t es,
                                          const float* __restrict__ mrow, T* __restrict__ op, size_t os, float p, float q,
                                          const SagTaps& taps, int ntaps, int boundary, int H, int hm, float* s0, float* s1,
                                          float* sw) {
  const int tid = threadIdx.x;
  const int HW = H * H, half = ntaps >> 1, r = H / hm;
#pragma unroll
  for (int t = 0; t < SAG_MAX_TAPS; ++t)
    if (tid == t) sw[t] = t < ntaps ? taps.w[t] : 0.f;      // (constant indices into the argument block)
  for (int i = tid; i < HW; i += blockDim.x) s0[i] = fmaf(p, xp[i], q * to_f32(ep[(size_t)i * es]));
  __syncthreads();
  for (int i = tid; i < HW; i += blockDim.x) {
    const int y = i / H, x = i - y * H;
    float a = 0.f;
    for (int t = 0; t < ntaps; ++t) a = fmaf(sw[t], s0[y * H + sag_index(x + t - half, H, boundary)], a);
    s1[i] = a;
  }
  __syncthreads();
  for (int i = tid; i < HW; i += blockDim.x) {
    const int y = i / H, x = i - y * H;
    float a = 0.f;
    for (int t = 0; t < ntaps; ++t) a = fmaf(sw[t], s1[sag_index(y + t - half, H, boundary) * H + x], a);
    const float xv = xp[i];
    const bool masked = mrow[(y / r) * hm + x / r] > 1.0f;      // strict; a NaN masks nothing
    op[(size_t)i * os] = from_f32<T>(masked ? xv + (a - s0[i]) / p : xv);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) k_sag_degrade(const float* __restrict__ x, const T* __restrict__ e, const float* __restrict__ mass,
                                                     T* __restrict__ xd, const float* __restrict__ coef,
                                                     const int* __restrict__ step_idx, SagTaps taps, int ntaps, int boundary, int C,
                                                     int H, int hm) {
  __shared__ float s0[SAG_MAX_SIDE * SAG_MAX_SIDE], s1[SAG_MAX_SIDE * SAG_MAX_SIDE], sw[16];
  const int s = *step_idx;
  const float p = coef[12 * (size_t)s], q = coef[12 * (size_t)s + 1];
  const int b = blockIdx.x / C, c = blockIdx.x - b * C;
  const size_t HW = (size_t)H * H;
  sag_plane<T>(x + (size_t)blockIdx.x * HW, e + (size_t)b * HW * C + c, (size_t)C, mass + (size_t)b * hm * hm,
               xd + (size_t)b * HW * C + c, (size_t)C, p, q, taps, ntaps, boundary, H, hm, s0, s1, sw);
}

__global__ void __launch_bounds__(256) k_sag_degrade_flat(const float* __restrict__ x, const float* __restrict__ e,
                                                          const float* __restrict__ mass, float* __restrict__ xd, float p, float q,
                                                          SagTaps taps, int ntaps, int boundary, int C, int H, int hm) {
  __shared__ float s0[SAG_MAX_SIDE * SAG_MAX_SIDE], s1[SAG_MAX_SIDE * SAG_MAX_SIDE], sw[16];
  const int b = blockIdx.x / C;
  const size_t o = (size_t)blockIdx.x * H * H;
  sag_plane<float>(x + o, e + o, 1, mass + (size_t)b * hm * hm, xd + o, 1, p, q, taps, ntaps, boundary, H, hm, s0, s1, sw);
}

static int sag_degrade_check(const char* name, const float* taps, int ntaps, int boundary, int B, int C, int H, int W, int hm) {
  AFLDM_REQUIRE(taps, AFLDM_ENULL, "%s: NULL taps", name);
  AFLDM_REQUIRE(ntaps >= 1 && ntaps <= SAG_MAX_TAPS && (ntaps & 1), AFLDM_ESHAPE, "%s: %d taps (odd, 1 .. %d)", name, ntaps,
                SAG_MAX_TAPS);
  AFLDM_REQUIRE(boundary == 0 || boundary == 1, AFLDM_ESHAPE, "%s: boundary %d (0 = reflect, 1 = circular)", name, boundary);
  AFLDM_REQUIRE(B > 0 && C > 0 && H == W && H >= 8 && H <= SAG_MAX_SIDE, AFLDM_ESHAPE,
                "%s: B = %d, C = %d, H = %d, W = %d (square planes of 8 .. %d)", name, B, C, H, W, SAG_MAX_SIDE);
  AFLDM_REQUIRE((long long)C * H * W <= 16384, AFLDM_ESHAPE, "%s: %lld elements per sample (16384 at the most)", name,
                (long long)C * H * W);
  AFLDM_REQUIRE(hm >= 1 && hm <= H && H % hm == 0, AFLDM_ESHAPE, "%s: a %d x %d map on %d x %d latents (hm must divide H)", name,
                hm, hm, H, W);
  AFLDM_REQUIRE((ntaps >> 1) < H, AFLDM_ESHAPE, "%s: half width %d on planes of %d", name, ntaps >> 1, H);
  return AFLDM_OK;
}

}  // namespace

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_attn_key_mass_ok(int B, int heads, int T, int d, int dtype) {
  return key_mass_shape_ok(B, heads, T, d, dtype) ? 1 : 0;
}

extern "C" int afldm_attn_key_mass(const void* q, int ldq, const void* k, int ldk, float* mass, float* stats_ws, int B, int heads,
                                   int T, int d, float scale, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(q && k && mass && stats_ws, AFLDM_ENULL, "afldm_attn_key_mass: NULL pointer");
  AFLDM_REQUIRE(key_mass_shape_ok(B, heads, T, d, dtype), AFLDM_ESHAPE,
                "afldm_attn_key_mass: no kernel for B = %d, heads = %d, T = %d, d = %d, dtype %d (see afldm_attn_key_mass_ok)", B,
                heads, T, d, dtype);
  AFLDM_REQUIRE(scale > 0.0f, AFLDM_ESHAPE, "afldm_attn_key_mass: scale = %g must be positive", (double)scale);
  AFLDM_REQUIRE(ldq >= heads * d && ldk >= heads * d && ldq % 8 == 0 && ldk % 8 == 0, AFLDM_ESHAPE,
                "afldm_attn_key_mass: ldq = %d, ldk = %d (multiples of 8, at least heads * d = %d)", ldq, ldk, heads * d);
  AFLDM_REQUIRE(aligned16(q) && aligned16(k) && (reinterpret_cast<uintptr_t>(stats_ws) & 7) == 0, AFLDM_EALIGN,
                "afldm_attn_key_mass: q, k need 16-byte alignment, stats_ws 8-byte");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == AFLDM_F32)
    return dispatch_key_mass<float>((const float*)q, ldq, (const float*)k, ldk, mass, stats_ws, B, heads, T, d, scale, st);
  return dispatch_key_mass<bf16>((const bf16*)q, ldq, (const bf16*)k, ldk, mass, stats_ws, B, heads, T, d, scale, st);
}

extern "C" int afldm_sag_degrade(const float* x, const void* e, const float* mass, void* x_d, const float* coef,
                                 const int* step_idx, const float* taps, int ntaps, int boundary, int B, int C, int H, int W,
                                 int hm, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && e && mass && x_d && coef && step_idx, AFLDM_ENULL, "afldm_sag_degrade: NULL pointer");
  if (int rc = sag_degrade_check("afldm_sag_degrade", taps, ntaps, boundary, B, C, H, W, hm)) return rc;
  AFLDM_REQUIRE(x_d != e, AFLDM_ESHAPE, "afldm_sag_degrade: x_d must not alias e");
  SagTaps tp;
  for (int t = 0; t < SAG_MAX_TAPS; ++t) tp.w[t] = t < ntaps ? taps[t] : 0.f;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype,
             (k_sag_degrade<float><<<B * C, 256, 0, st>>>(x, (const float*)e, mass, (float*)x_d, coef, step_idx, tp, ntaps, boundary,
                                                         C, H, hm)),
             (k_sag_degrade<bf16><<<B * C, 256, 0, st>>>(x, (const bf16*)e, mass, (bf16*)x_d, coef, step_idx, tp, ntaps, boundary, C,
                                                        H, hm)),
             "afldm_sag_degrade");
  return check_launch("afldm_sag_degrade");
}

extern "C" int afldm_sag_degrade_flat(const float* x, const float* e, const float* mass, float* x_d, float p, float q,
                                      const float* taps, int ntaps, int boundary, int B, int C, int H, int W, int hm,
                                      afldm_stream_t stream) {
  AFLDM_REQUIRE(x && e && mass && x_d, AFLDM_ENULL, "afldm_sag_degrade_flat: NULL pointer");
  if (int rc = sag_degrade_check("afldm_sag_degrade_flat", taps, ntaps, boundary, B, C, H, W, hm)) return rc;
  AFLDM_REQUIRE(x_d != x && x_d != e, AFLDM_ESHAPE, "afldm_sag_degrade_flat: x_d must not alias x or e");
  SagTaps tp;
  for (int t = 0; t < SAG_MAX_TAPS; ++t) tp.w[t] = t < ntaps ? taps[t] : 0.f;
  k_sag_degrade_flat<<<B * C, 256, 0, (hipStream_t)stream>>>(x, e, mass, x_d, p, q, tp, ntaps, boundary, C, H, hm);
  return check_launch("afldm_sag_degrade_flat");
}
