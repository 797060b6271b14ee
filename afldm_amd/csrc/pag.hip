// pag.hip — perturbed-attention guidance (Ahn et al. 2024; diffusers PAGMixin / PAGIdentitySelfAttnProcessor2_0) on the
// graph-replayed engine.  Two launches carry it:
//
// 1. afldm_attn_identity_block — an attention block whose attention map is the identity: softmax(q k^T) v collapses to v, so
//      y = x + to_out(to_v(GN(x))) = x + GN(x) W_vo^T + b_vo,   W_vo = W_o W_v,  b_vo = W_o b_v + b_o  (folded on the host, fp64)
//    as ONE launch: GroupNorm-apply + GEMM + bias + residual.  GroupNorm is APPLIED TO THE A OPERAND (not folded into the weight
//    rows as attnf.hip phase A does: the fold needs a per-sample copy of W in LDS, C x C here against attnf's 3 d x C).  A
//    workgroup (4 waves) owns BM token rows and all C output channels: it finishes mean / rstd of the (sample, group) pairs its
//    rows touch from the producer's per-channel partial sums (a quarter wave per pair, fixed order, fp64 sums - the arithmetic
//    of afldm_gn_apply), writes bf16(GN(x)) of its rows to LDS - THE single operand rounding, the one afldm_gn_apply makes when
//    it stores its output - and runs K complete on MFMA with the weight fragments read straight from L2 (every workgroup reads
//    all of W_vo: BM grows as C shrinks so that this stays below the tile's own traffic).  fp32 accumulation, K ascending in
//    32-wide steps, then + bias + x, one output rounding.  At T < BM a tile's rows span BM / T samples; T and BM are powers of
//    two, so a tile never holds part of a sample next to another one.  Rows past B T are zero in LDS and never stored.
//
// 2. afldm_pag_step / afldm_pag_step_flat — the guided update.  eps2 holds both UNet outputs, e (rows 0 .. B-1) and the
//    perturbed e_p (rows B .. 2B-1); the row is (p, q, lo, hi, a, b, d, c, s, phi, 0, 0):
//      g = e + s (e - e_p);   phi > 0:  g <- g (phi sigma(e) / sigma(g) + 1 - phi)     (diffusers rescale_noise_cfg, per sample)
//      x0 = clamp(p x + q g, lo, hi);   x_out = a x + b x0 + d g + c z                  (the "sde" row applied to g)
//    One 1024-thread workgroup per sample keeps the sample's e and g in registers (up to 16 elements a thread: 16384 elements a
//    sample).  sigma: two passes in fp32, the mean and then the centred squares, every sum a pairwise tree (4 elements, 4 groups,
//    64 lanes by xor-shuffles, 16 waves out of LDS in a fixed tree): depth log2(16384), no atomics, bits independent of B.  The
//    ratio is sqrt(ss_e / ss_g) (the 1 / (n - 1) of the two deviations cancels), 1 where ss_g = 0; with phi = 0 the reduction is
//    skipped.  z is read only where c != 0.  All of a sample's reads of x come before its stores: x_out may alias x.
#include "step_common.hpp"

namespace afldm {

namespace {

// ------------------------------------------------------------------------------------------------ identity attention block
struct IdbP {
  const bf16* x;
  const float* st;
  const float* gamma;
  const float* beta;
  const bf16* w;
  const float* bias;
  bf16* y;
  int B, T, S, G;
  float eps;
};

template <int C, int BM>
struct IdbCfg {
  static constexpr int NT = C / 64;          // 16-cout tiles per wave (a wave owns C / 4 couts)
  static constexpr int MT = BM / 16;         // 16-token tiles
  static constexpr int ROW = C + 8;          // bf16 elements between rows of the normalised tile (16-byte multiple, bank spread)
  static constexpr int KEYS_MAX = (BM / 4) * 32;      // (sample, group) pairs of a tile at T = 4, G = 32
  static constexpr int LDS = BM * ROW * 2 + KEYS_MAX * 8;
  static_assert(C % 64 == 0 && BM % 32 == 0, "tile shape");
};

template <int C, int BM>
__global__ void __launch_bounds__(256) k_attn_identity(IdbP p) {
  typedef IdbCfg<C, BM> CF;
  typedef Mma<bf16> MM;
  typedef MM::Chunk Chunk;
  extern __shared__ __attribute__((aligned(16))) char idb_smem[];
  bf16* sa = reinterpret_cast<bf16*>(idb_smem);
  f32x2* sms = reinterpret_cast<f32x2*>(idb_smem + BM * CF::ROW * 2);      // (mean, rstd) per (sample slot, group)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int M = p.B * p.T;
  const int m0 = blockIdx.x * BM;
  const int T = p.T;
  constexpr int G = 32, cpg = C / G;      // (afldm_attn_identity_block_ok: 32 groups)
  const int nsamp = T >= BM ? 1 : BM / T;      // samples the tile's rows span
  const int b0 = m0 / T;

  // ---- (mean, rstd) of the tile's (sample, group) pairs: a quarter wave per pair, its cpg x S partials strided over 16 lanes
  {
    const int quarter = tid >> 4, ql = tid & 15;
    const int nkeys = nsamp * G;
    const double n = (double)cpg * T;
    for (int key = quarter; key < nkeys; key += 16) {
      const int sl = key / G, g = key - sl * G;
      const int b = b0 + sl;
      double s1 = 0.0, s2 = 0.0;
      if (b < p.B) {
        for (int j = ql; j < cpg * p.S; j += 16) {
          const int c = g * cpg + j / p.S, sp = j - (j / p.S) * p.S;
          const f32x2 v = *reinterpret_cast<const f32x2*>(p.st + (((size_t)b * p.S + sp) * C + c) * 2);
          s1 += (double)v[0];
          s2 += (double)v[1];
        }
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {          // (xor < 16: stays inside the quarter)
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
      }
      if (ql == 0) {
        float mean = 0.f, rstd = 0.f;
        if (b < p.B) gn_mean_rstd(s1, s2, n, p.eps, mean, rstd);
        sms[key] = f32x2{mean, rstd};
      }
    }
  }
  __syncthreads();

  // ---- bf16(GN(x)) of the tile's rows -> LDS, 8 channels (16 bytes) per item
  {
    constexpr int CPR = C / 8;
    for (int i = tid; i < BM * CPR; i += 256) {
      const int row = i / CPR, kc = i - row * CPR;
      const int m = m0 + row;
      Chunk o = MM::zero();
      if (m < M) {
        const int sl = T >= BM ? 0 : row / T;
        const Chunk xv = ld16<Chunk>(p.x + (size_t)m * C + kc * 8);
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(p.gamma + kc * 8), g1 = *reinterpret_cast<const f32x4*>(p.gamma + kc * 8 + 4);
        const f32x4 e0 = *reinterpret_cast<const f32x4*>(p.beta + kc * 8), e1 = *reinterpret_cast<const f32x4*>(p.beta + kc * 8 + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const f32x2 ms = sms[sl * G + (kc * 8 + e) / cpg];
          const float ga = e < 4 ? g0[e & 3] : g1[e & 3], be = e < 4 ? e0[e & 3] : e1[e & 3];
          o[e] = (bf16)(((float)xv[e] - ms[0]) * ms[1] * ga + be);
        }
      }
      st16<Chunk>(sa + row * CF::ROW + kc * 8, o);
    }
  }
  __syncthreads();

  // ---- GEMM: A = W_vo rows (couts), B = the normalised tokens: a lane ends with 4 consecutive couts of one token
  const int n0w = wave * (C / 4);
  f32x4 acc[CF::NT][CF::MT];
#pragma unroll
  for (int tn = 0; tn < CF::NT; ++tn)
#pragma unroll
    for (int tm = 0; tm < CF::MT; ++tm) acc[tn][tm] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int kf = 0; kf < C / 32; ++kf) {
    Chunk xb[CF::MT];
#pragma unroll
    for (int tm = 0; tm < CF::MT; ++tm) xb[tm] = ld16<Chunk>(sa + (16 * tm + li) * CF::ROW + 32 * kf + 8 * lg);
#pragma unroll
    for (int tn = 0; tn < CF::NT; ++tn) {
      const Chunk wf = ld16<Chunk>(p.w + (size_t)(n0w + 16 * tn + li) * C + 32 * kf + 8 * lg);
#pragma unroll
      for (int tm = 0; tm < CF::MT; ++tm) MM::mma(acc[tn][tm], wf, xb[tm]);
    }
  }

  // ---- + bias + x, one rounding; 8-byte pieces of token rows
#pragma unroll
  for (int tn = 0; tn < CF::NT; ++tn) {
    const int n = n0w + 16 * tn + 4 * lg;
    const f32x4 bq = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
    for (int tm = 0; tm < CF::MT; ++tm) {
      const int m = m0 + 16 * tm + li;
      if (m < M) {
        const bf16x4 xr = *reinterpret_cast<const bf16x4*>(p.x + (size_t)m * C + n);
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (bf16)(acc[tn][tm][r] + bq[r] + (float)xr[r]);
        *reinterpret_cast<bf16x4*>(p.y + (size_t)m * C + n) = o;
      }
    }
  }
}

template <int C, int BM>
static int launch_identity(const IdbP& p, hipStream_t st) {
  typedef IdbCfg<C, BM> CF;
  static_assert(CF::LDS <= 64 * 1024, "the tile fits the default LDS limit");
  const long long M = (long long)p.B * p.T;
  k_attn_identity<C, BM><<<cdiv(M, BM), 256, CF::LDS, st>>>(p);
  return check_launch("afldm_attn_identity_block");
}

static bool identity_shape_ok(int B, int T, int C, int G, int dtype) {
  if (dtype != AFLDM_BF16 || B <= 0 || G != 32) return false;
  if (T != 4 && T != 16 && T != 64 && T != 256 && T != 1024) return false;
  if (C != 64 && C != 128 && C != 192 && C != 384 && C != 768) return false;
  return (long long)B * T * C < (1ll << 31);
}

// ------------------------------------------------------------------------------------------------ guided update
struct pag_row {
  float p, q, lo, hi, a, b, d, c, s, phi;
};

constexpr int PAG_THREADS = 1024;
constexpr int PAG_PER_THREAD = 16;
constexpr int PAG_NMAX = PAG_THREADS * PAG_PER_THREAD;      // elements per sample

// Sum of (a, b) over the workgroup, the same bits in every thread: xor-shuffles inside a wave, then the 16 wave sums out of LDS in a
// fixed pairwise tree.  `red` holds 2 x 16 floats; two barriers, so it can be reused by the next call.
__device__ __forceinline__ void pag_block_sum(float& a, float& b, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave] = a;
    red[16 + wave] = b;
  }
  __syncthreads();
  float va[16], vb[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    va[i] = red[i];
    vb[i] = red[16 + i];
  }
#pragma unroll
  for (int w = 8; w > 0; w >>= 1)
#pragma unroll
    for (int i = 0; i < w; ++i) {
      va[i] = va[i] + va[i + w];
      vb[i] = vb[i] + vb[i + w];
    }
  a = va[0];
  b = vb[0];
  __syncthreads();
}

// One sample of n = C * HW elements.  xs / zs / os: the sample's x / noise / x_out (NCHW fp32); es / eps: the sample's first element
// of e / e_p; element i = ch * HW + pix of the sample lies at e[(flat ? i : pix * C + ch)].  V = 4: HW % 4 == 0 (non-flat) or
// n % 4 == 0 (flat), 16-byte aligned x / z / x_out.
template <typename T, int V, bool FLAT>
__device__ __forceinline__ void pag_sample(const float* xs, const T* __restrict__ es, const T* __restrict__ eps, const float* __restrict__ zs,
                                           float* os, const pag_row& r, int C, int HW, int n, float* red) {
  constexpr int GR = PAG_PER_THREAD / V;
  const int tid = threadIdx.x;
  float e[GR][V], g[GR][V];
#pragma unroll
  for (int u = 0; u < GR; ++u) {
    const int i = (tid + u * PAG_THREADS) * V;
#pragma unroll
    for (int k = 0; k < V; ++k) e[u][k] = g[u][k] = 0.0f;
    if (i < n) {
      size_t off, stride;
      if constexpr (FLAT) {
        off = (size_t)i;
        stride = 1;
      } else {
        const int ch = i / HW, pix = i - ch * HW;
        off = (size_t)pix * C + ch;
        stride = (size_t)C;
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float ev = to_f32(es[off + k * stride]), pv = to_f32(eps[off + k * stride]);
        e[u][k] = ev;
        g[u][k] = ev + r.s * (ev - pv);
      }
    }
  }
  if (r.phi != 0.0f) {      // (uniform: the row is the same for every thread)
    // pairwise inside the thread: the V elements of a group, then the groups (absent elements are 0 in both passes)
    auto tree = [&](float (&v)[GR][V]) {
      float s[GR];
#pragma unroll
      for (int u = 0; u < GR; ++u) {
        if constexpr (V == 4) s[u] = (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
        else s[u] = v[u][0];
      }
#pragma unroll
      for (int w = GR / 2; w > 0; w >>= 1)
#pragma unroll
        for (int u = 0; u < w; ++u) s[u] = s[u] + s[u + w];
      return s[0];
    };
    float se = tree(e), sg = tree(g);
    pag_block_sum(se, sg, red);
    const float me = se / (float)n, mg = sg / (float)n;
    float de[GR][V], dg[GR][V];
#pragma unroll
    for (int u = 0; u < GR; ++u) {
      const int i = (tid + u * PAG_THREADS) * V;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const bool on = i < n;      // (V == 4: whole groups; V == 1: one element)
        const float a = e[u][k] - me, b = g[u][k] - mg;
        de[u][k] = on ? a * a : 0.0f;
        dg[u][k] = on ? b * b : 0.0f;
      }
    }
    float qe = tree(de), qg = tree(dg);
    pag_block_sum(qe, qg, red);
    const float ratio = qg > 0.0f ? sqrtf(qe / qg) : 1.0f;
    const float f = r.phi * ratio + (1.0f - r.phi);
#pragma unroll
    for (int u = 0; u < GR; ++u)
#pragma unroll
      for (int k = 0; k < V; ++k) g[u][k] *= f;
  }
  const bool has_z = r.c != 0.0f && zs != nullptr;
  float out[GR][V];
#pragma unroll
  for (int u = 0; u < GR; ++u) {
    const int i = (tid + u * PAG_THREADS) * V;
    if (i < n) {
      float xv[V], zv[V];
      if constexpr (V == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(xs + i);
        xv[0] = q[0]; xv[1] = q[1]; xv[2] = q[2]; xv[3] = q[3];
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (has_z) z = *reinterpret_cast<const f32x4*>(zs + i);
        zv[0] = z[0]; zv[1] = z[1]; zv[2] = z[2]; zv[3] = z[3];
      } else {
        xv[0] = xs[i];
        zv[0] = has_z ? zs[i] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float x0 = clamp_nan(r.p * xv[k] + r.q * g[u][k], r.lo, r.hi);
        out[u][k] = r.a * xv[k] + r.b * x0 + r.d * g[u][k] + r.c * zv[k];
      }
    }
  }
  __syncthreads();      // every read of x in the workgroup is behind us (x_out may alias x)
#pragma unroll
  for (int u = 0; u < GR; ++u) {
    const int i = (tid + u * PAG_THREADS) * V;
    if (i < n) {
      if constexpr (V == 4) *reinterpret_cast<f32x4*>(os + i) = f32x4{out[u][0], out[u][1], out[u][2], out[u][3]};
      else os[i] = out[u][0];
    }
  }
}

template <typename T, int V>
__global__ void __launch_bounds__(PAG_THREADS) k_pag_step(const float* x, const T* __restrict__ eps2, const float* __restrict__ noise,
                                                          size_t noise_step_stride, float* x_out, const float* __restrict__ coef,
                                                          const int* __restrict__ step_idx, int B, int C, int HW) {
  __shared__ float red[32];
  const int s = *step_idx;
  const float* rp = coef + 12 * (size_t)s;
  const pag_row r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8], rp[9]};
  const int n = C * HW;
  const size_t o = (size_t)blockIdx.x * n;
  const float* zs = noise ? noise + (size_t)s * noise_step_stride + o : nullptr;
  pag_sample<T, V, false>(x + o, eps2 + o, eps2 + (size_t)B * n + o, zs, x_out + o, r, C, HW, n, red);
}

template <int V>
__global__ void __launch_bounds__(PAG_THREADS) k_pag_step_flat(const float* x, const float* __restrict__ e, const float* __restrict__ ep,
                                                               const float* __restrict__ z, float* x_out, pag_row r, int n) {
  __shared__ float red[32];
  const size_t o = (size_t)blockIdx.x * n;
  pag_sample<float, V, true>(x + o, e + o, ep + o, z ? z + o : nullptr, x_out + o, r, 1, n, n, red);
}

}  // namespace

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_attn_identity_block_ok(int B, int T, int C, int G, int dtype) {
  return identity_shape_ok(B, T, C, G, dtype) ? 1 : 0;
}

extern "C" int afldm_attn_identity_block(const void* x, const float* stats, int S, const float* gamma, const float* beta, int G,
                                         float eps, const void* w_vo, const float* bias_vo, void* y, int B, int T, int C, int dtype,
                                         afldm_stream_t stream) {
  AFLDM_REQUIRE(x && stats && gamma && beta && w_vo && bias_vo && y, AFLDM_ENULL, "afldm_attn_identity_block: NULL pointer");
  AFLDM_REQUIRE(S > 0 && identity_shape_ok(B, T, C, G, dtype), AFLDM_ESHAPE,
                "afldm_attn_identity_block: no kernel for B = %d, T = %d, C = %d, G = %d, S = %d, dtype %d "
                "(see afldm_attn_identity_block_ok)", B, T, C, G, S, dtype);
  AFLDM_REQUIRE(x != y, AFLDM_ESHAPE, "afldm_attn_identity_block: y must not alias x");
  AFLDM_REQUIRE(aligned16(x) && aligned16(y) && aligned16(w_vo) && aligned16(bias_vo) && aligned16(gamma) && aligned16(beta) &&
                    (reinterpret_cast<uintptr_t>(stats) & 7) == 0,
                AFLDM_EALIGN, "afldm_attn_identity_block: x, y, w_vo, bias_vo, gamma, beta need 16-byte alignment, stats 8-byte");
  const IdbP p{(const bf16*)x, stats, gamma, beta, (const bf16*)w_vo, bias_vo, (bf16*)y, B, T, S, G, eps};
  hipStream_t st = (hipStream_t)stream;
  switch (C) {
    case 64: return launch_identity<64, 128>(p, st);
    case 128: return launch_identity<128, 128>(p, st);
    case 192: return launch_identity<192, 128>(p, st);
    case 384: return launch_identity<384, 64>(p, st);
    default: return launch_identity<768, 32>(p, st);
  }
}

extern "C" int afldm_pag_step(const float* x, const void* eps2, const float* noise, size_t noise_step_stride, float* x_out,
                              const float* coef, int* step_idx, int advance, int B, int C, int H, int W, int dtype,
                              afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps2 && x_out && coef && step_idx, AFLDM_ENULL, "afldm_pag_step: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, AFLDM_ESHAPE, "afldm_pag_step: bad shape");
  const long long n = (long long)C * H * W;
  AFLDM_REQUIRE(n <= PAG_NMAX, AFLDM_ESHAPE,
                "afldm_pag_step: %lld elements per sample (one workgroup holds a sample in registers: %d at the most)", n, PAG_NMAX);
  AFLDM_REQUIRE(!noise || noise_step_stride >= (size_t)B * n, AFLDM_ESHAPE,
                "afldm_pag_step: noise_step_stride smaller than one step's B*C*H*W");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  const bool v4 = HW % 4 == 0 && aligned16(x) && aligned16(x_out) && (!noise || (noise_step_stride % 4 == 0 && aligned16(noise)));
#define LAUNCH(T, V) \
  (k_pag_step<T, V><<<B, PAG_THREADS, 0, st>>>(x, (const T*)eps2, noise, noise_step_stride, x_out, coef, step_idx, B, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_pag_step");
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_pag_step");
}

extern "C" int afldm_pag_step_flat(const float* x, const float* e, const float* e_p, const float* z, float* x_out, float p, float q,
                                   float lo, float hi, float a, float b, float d, float c, float s, float phi, float r10, float r11,
                                   int B, size_t n, afldm_stream_t stream) {
  (void)r10;
  (void)r11;
  AFLDM_REQUIRE(x && e && e_p && x_out, AFLDM_ENULL, "afldm_pag_step_flat: NULL pointer");
  AFLDM_REQUIRE(c == 0.0f || z, AFLDM_ENULL, "afldm_pag_step_flat: z is NULL but c is not 0");
  AFLDM_REQUIRE(B >= 0 && n > 0, AFLDM_ESHAPE, "afldm_pag_step_flat: bad shape");
  AFLDM_REQUIRE(n <= (size_t)PAG_NMAX, AFLDM_ESHAPE,
                "afldm_pag_step_flat: %zu elements per sample (one workgroup holds a sample in registers: %d at the most)", n, PAG_NMAX);
  if (B == 0) return AFLDM_OK;
  hipStream_t st = (hipStream_t)stream;
  const pag_row r{p, q, lo, hi, a, b, d, c, s, phi};
  const float* zz = c != 0.0f ? z : nullptr;
  const bool v4 = n % 4 == 0 && aligned16(x) && aligned16(x_out) && (!zz || aligned16(zz));      // (e, e_p: scalar reads)
  if (v4)
    k_pag_step_flat<4><<<B, PAG_THREADS, 0, st>>>(x, e, e_p, zz, x_out, r, (int)n);
  else
    k_pag_step_flat<1><<<B, PAG_THREADS, 0, st>>>(x, e, e_p, zz, x_out, r, (int)n);
  return check_launch("afldm_pag_step_flat");
}
