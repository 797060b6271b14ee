// resconv.hip — the convolutions of the VANILLA resamplers (diffusers Downsample2D / Upsample2D with use_conv), for the stock
// UNet / AutoencoderKL and for the levels of a partly alias-free VAE that keep them:
//   afldm_conv2d_s2   3x3 convolution at stride 2, zero padding (pad_lo, pad_hi):  UNet Downsample2D (1, 1) and the VAE
//                     encoder's F.pad(x, (0, 1, 0, 1)) + unpadded conv (0, 1)
//   afldm_conv2d_up2  conv3x3(nearest2x(x)), 'same' padding, as four 2x2 convolutions of the LOW-resolution x (one per output
//                     phase) with per-phase folded weights (afldm_pack_weight_up2): 16 instead of 36 MACs per 2x2 output block
//                     per (cin, cout); the x2 plane is never formed.
// Both are one implicit GEMM on MFMA: rows = output pixels (up2: low-resolution pixels), columns = couts (up2: 4 Cout, phase
// major), K = taps x Cin with the tap outer and 128-byte channel blocks inner.  The pixel and weight operands go HBM -> LDS by
// LDS-DMA (buffer_load ... lds) through a double-buffered ring; zero padding, channel / row / column tails are the buffer
// descriptor's bounds check (an out-of-range voffset lands zeros in LDS).  Only the address generation differs from the stride-1
// convolutions of conv.hip: input row = 2 oh + kh - pad_lo (s2), oh + th - 1 + a for phase a (up2).
// Epilogue: + fp32 bias, rounded once to the activation dtype, staged in LDS and written as 16-byte row pieces (up2: scattered
// to the interleaved [B, 2H, 2W, Cout] output), plus the per-channel GroupNorm partial sums of the stored values for the
// ResnetBlock2D norm1 that follows.
#include "conv_common.hpp"

namespace afldm {

namespace {

struct RsP {
  const void* x;
  const void* w;
  const float* bias;
  void* y;
  float* stats;
  int H, W, Cin, Cout;  // input plane, channels
  int Ho, Wo;           // GEMM rows per sample = Ho x Wo (s2: the output plane; up2: the input plane)
  int M, N;             // M = B Ho Wo, N = Cout (s2) / 4 Cout (up2)
  int pad_lo;
  int ksteps;           // taps x channel blocks
  int tiles_n, m_fast;
  int stats_S, stats_Sp;  // splits per sample; per phase (up2)
};

constexpr int kBM = 128;   // rows per tile (2 x 2 waves, 64 rows each)
constexpr int kStages = 2;
constexpr unsigned kOOB = 0x80000000u;

template <typename T, int BN>
constexpr int stage_bytes() {
  return (kBM + BN) * 128;
}
template <typename T, int BN>
constexpr int lds_bytes() {
  constexpr int ring = kStages * stage_bytes<T, BN>();
  constexpr int epi = kBM * (BN + 8) * (int)sizeof(T);
  return ring > epi ? ring : epi;
}

// MODE 0: stride-2 3x3 (9 taps); MODE 1: phase-folded nearest-x2 + 3x3 (4 taps, the tile's phase = n0 / Cout).
template <typename T, int MODE, int BN>
__global__ void __launch_bounds__(256, 2) k_resconv(RsP p) {
  typedef Mma<T> MM;
  typedef typename MM::Chunk Chunk;
  constexpr int EPC = MM::EPC, KSTEP = 8 * EPC;     // one 128-byte LDS row per pixel / weight row and K step
  constexpr int ESZ = (int)sizeof(T);
  constexpr int KS = MODE == 0 ? 3 : 2, TAPS = KS * KS;
  constexpr int WMS = kBM / 2, WNS = BN / 2, TM = WMS / 16, TN = WNS / 16;
  constexpr int XPW = kBM / 8 / 4, WPW = BN / 8 / 4;   // LDS-DMA wave-instructions (8 rows each) per wave and stage
  constexpr int X_STAGE = kBM * 128, STAGE = stage_bytes<T, BN>();

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 15, lg = lane >> 4;

  // consecutive tiles share one XCD (xcd_remap) and, there, their larger operand: the pixel rows (n fastest) unless the
  // weights outweigh them (m fastest)
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int tiles_m = (p.M + kBM - 1) / kBM;
  const int tile_m = p.m_fast ? tile % tiles_m : tile / p.tiles_n;
  const int tile_n = p.m_fast ? tile / tiles_m : tile % p.tiles_n;
  const int m0 = tile_m * kBM, n0 = tile_n * BN;
  const int phase = MODE == 1 ? n0 / p.Cout : 0;    // up2: BN divides Cout, a tile lies in one phase
  const int pa = phase >> 1, pc = phase & 1;
  const int plane = p.Ho * p.Wo;
  const int Cin = p.Cin;

  const long long x_bytes = (long long)(p.M / plane) * p.H * p.W * Cin * ESZ;
  const long long w_bytes = (long long)p.N * TAPS * Cin * ESZ;
  __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)w_bytes, 0x00020000);

  // Instruction j of a stage covers LDS rows 8 j .. 8 j + 7; lane l fills row 8 j + (l >> 3), position l & 7 of that row, with
  // source chunk (l & 7) ^ ((row >> 1) & 7): the read side (ds_read_b128 of 16 rows x 4 chunks) is then conflict-free.
  int xr0[XPW], xc0[XPW], xcin[XPW];
  unsigned xpix[XPW];   // input pixel index of (sample, row xr0, column xc0)
  bool xok[XPW];
#pragma unroll
  for (int i = 0; i < XPW; ++i) {
    const int j = wave + 4 * i;
    const int row = 8 * j + (lane >> 3);
    xcin[i] = ((lane & 7) ^ ((4 * j + (lane >> 4)) & 7)) * EPC;
    const int m = m0 + row;
    xok[i] = m < p.M;
    const int mm = xok[i] ? m : 0;
    const int b = mm / plane, pix = mm - b * plane;
    const int oh = pix / p.Wo, ow = pix - oh * p.Wo;
    xr0[i] = MODE == 0 ? 2 * oh - p.pad_lo : oh - 1 + pa;
    xc0[i] = MODE == 0 ? 2 * ow - p.pad_lo : ow - 1 + pc;
    xpix[i] = (unsigned)(b * p.H * p.W);
  }
  unsigned wrow[WPW];
  int wcin[WPW];
  bool wok[WPW];
#pragma unroll
  for (int i = 0; i < WPW; ++i) {
    const int j = wave + 4 * i;
    const int n = n0 + 8 * j + (lane >> 3);
    wcin[i] = ((lane & 7) ^ ((4 * j + (lane >> 4)) & 7)) * EPC;
    wok[i] = n < p.N;
    wrow[i] = (unsigned)(wok[i] ? n : 0) * (unsigned)(TAPS * Cin);
  }

  // K cursor of the next step to issue: tap outer, channel block inner
  int is_kt = 0, is_tap = 0, is_kh = 0, is_kw = 0, is_ci0 = 0;
  unsigned xtap[XPW];   // byte offset of the lane's pixel for the current tap (channel 0), or kOOB
  auto retap = [&]() {
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
      const int ih = xr0[i] + is_kh, iw = xc0[i] + is_kw;
      const bool ok = xok[i] && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      xtap[i] = ok ? (xpix[i] + (unsigned)(ih * p.W + iw)) * (unsigned)Cin * ESZ : kOOB;
    }
  };
  retap();

  auto issue = [&](int slot) {
    char* sbase = smem + slot * STAGE;
    const bool live = is_kt < p.ksteps;
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
      const int j = wave + 4 * i;
      const int ci = is_ci0 + xcin[i];
      const unsigned off = (live && ci < Cin && xtap[i] != kOOB) ? xtap[i] + (unsigned)(ci * ESZ) : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_ptr_t)(sbase + j * 1024), 16, (int)off, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
      const int j = wave + 4 * i;
      const int ci = is_ci0 + wcin[i];
      const unsigned off = (live && ci < Cin && wok[i]) ? (wrow[i] + (unsigned)(is_tap * Cin + ci)) * ESZ : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr_t)(sbase + X_STAGE + j * 1024), 16, (int)off, 0, 0, 0);
    }
    ++is_kt;
    is_ci0 += KSTEP;
    if (is_ci0 >= Cin) {
      is_ci0 = 0;
      ++is_tap;
      if (++is_kw == KS) {
        is_kw = 0;
        ++is_kh;
      }
      if (is_kt < p.ksteps) retap();
    }
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TM; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int slot) {
    const char* sX = smem + slot * STAGE;
    const char* sW = sX + X_STAGE;
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      Chunk a[TN], b[TM];
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const int row = wn * WNS + t * 16 + li;
        a[t] = ld16<Chunk>(sW + row * 128 + (((kc * 4 + lg) ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const int row = wm * WMS + t * 16 + li;
        b[t] = ld16<Chunk>(sX + row * 128 + (((kc * 4 + lg) ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) MM::mma(acc[tn][tm], a[tn], b[tm]);
    }
  };

  // K step kt: every wave waits for its own LDS-DMA of step kt, one barrier (all waves' loads of kt have landed, all waves are
  // done reading step kt - 1), then the slot of kt - 1 is refilled with step kt + 1 while step kt is multiplied.
  issue(0);
  for (int kt = 0; kt < p.ksteps; ++kt) {
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (kt + 1 < p.ksteps) issue((kt + 1) & 1);
    compute(kt & 1);
  }
  __syncthreads();

  // ---- epilogue: + bias, rounded once, staged as T rows in the idle ring, then 16-byte row pieces out and the statistics
  constexpr int SROW = BN + 8;   // elements; a 16-byte multiple of padding per row
  T* sT = reinterpret_cast<T*>(smem);
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int col = wn * WNS + tn * 16 + 4 * lg;
    const int n = n0 + col;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias && n < p.N) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias + (MODE == 1 ? n - phase * p.Cout : n));
      bv[0] = b4[0]; bv[1] = b4[1]; bv[2] = b4[2]; bv[3] = b4[3];
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int row = wm * WMS + tm * 16 + li;
      store4<T>(sT + row * SROW + col, acc[tn][tm][0] + bv[0], acc[tn][tm][1] + bv[1], acc[tn][tm][2] + bv[2],
                acc[tn][tm][3] + bv[3]);
    }
  }
  __syncthreads();

  constexpr int EO = 16 / ESZ, CPR = BN / EO;
  T* y = (T*)p.y;
  for (int idx = tid; idx < kBM * CPR; idx += 256) {
    const int row = idx / CPR, ch = idx - row * CPR;
    const int m = m0 + row, n = n0 + ch * EO;
    if (m >= p.M || n >= p.N) continue;
    const Chunk v = ld16<Chunk>(sT + row * SROW + ch * EO);
    size_t opix;
    if (MODE == 0) {
      opix = (size_t)m;
    } else {
      const int b = m / plane, pix = m - b * plane;
      const int i = pix / p.Wo, jj = pix - i * p.Wo;
      opix = ((size_t)b * 2 * p.H + 2 * i + pa) * (size_t)(2 * p.W) + 2 * jj + pc;
    }
    st16_out<Chunk>(y + opix * p.Cout + (MODE == 1 ? n - phase * p.Cout : n), v);
  }

  if (p.stats) {
    // per-channel (sum, sum of squares) of the stored values.  A tile lies inside one sample (plane >= BM: split
    // (m0 % plane) / BM of it) or holds BM / plane whole samples (split 0 of each); up2 adds the phase: split = phase Sp + sp.
    const int seg = plane >= kBM ? kBM : plane, nseg = kBM / seg;
    for (int idx = tid; idx < nseg * BN; idx += 256) {
      const int c = idx % BN, s = idx / BN;
      const int n = n0 + c, r0 = s * seg;
      if (n >= p.N || m0 + r0 >= p.M) continue;
      float a1 = 0.f, a2 = 0.f;
      for (int r = r0; r < r0 + seg && m0 + r < p.M; ++r) {
        const float v = to_f32(sT[r * SROW + c]);
        a1 += v;
        a2 = fmaf(v, v, a2);
      }
      const int m = m0 + r0, b = m / plane;
      const int sp = (plane >= kBM ? (m - b * plane) / kBM : 0) + phase * p.stats_Sp;
      const int cout = MODE == 1 ? n - phase * p.Cout : n;
      *reinterpret_cast<f32x2*>(p.stats + (((size_t)b * p.stats_S + sp) * p.Cout + cout) * 2) = f32x2{a1, a2};
    }
  }
}

template <typename T, int MODE, int BN>
void launch(const RsP& p, hipStream_t st) {
  constexpr int LDS = lds_bytes<T, BN>();
  static unsigned long long attr_done = 0;
  if (LDS > 65536 && first_on_device(attr_done))
    (void)hipFuncSetAttribute((const void*)k_resconv<T, MODE, BN>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  const int tiles_m = cdiv(p.M, kBM);
  hipLaunchKernelGGL((k_resconv<T, MODE, BN>), dim3(tiles_m * p.tiles_n), dim3(256), LDS, st, p);
}

int bn_for(int mode, int Cout) {
  if (mode == 1) return Cout % 128 == 0 ? 128 : 64;   // a tile must not straddle two phases
  return Cout % 128 == 0 || Cout > 192 ? 128 : 64;
}

// statistics from the epilogue need tiles that lie in one sample or hold whole samples
bool epilogue_stats(int plane) { return plane % kBM == 0 || kBM % plane == 0; }

int splits(int mode, const afldm_conv_args* a) {
  const int plane = mode == 0 ? (a->H / 2) * (a->W / 2) : a->H * a->W;
  if (!epilogue_stats(plane)) return gn_splits(mode == 0 ? plane : 4 * plane);
  return (plane >= kBM ? plane / kBM : 1) * (mode == 1 ? 4 : 1);
}

int validate(int mode, const afldm_conv_args* a, int pad_lo, int pad_hi, const char* name) {
  AFLDM_REQUIRE(a, AFLDM_ENULL, "%s: NULL args", name);
  AFLDM_REQUIRE(a->x1 && a->w && a->y, AFLDM_ENULL, "%s: x1 / w / y must be non-NULL", name);
  AFLDM_REQUIRE(a->dtype == AFLDM_F32 || a->dtype == AFLDM_BF16, AFLDM_EDTYPE, "%s: unknown dtype %d", name, a->dtype);
  AFLDM_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->C1 > 0 && a->Cout > 0, AFLDM_ESHAPE, "%s: empty shape", name);
  AFLDM_REQUIRE(a->C1 % 8 == 0 && a->Cout % 8 == 0, AFLDM_ESHAPE, "%s: Cin %d / Cout %d must be multiples of 8", name, a->C1,
                a->Cout);
  AFLDM_REQUIRE(aligned16(a->x1) && aligned16(a->w) && aligned16(a->y) && (!a->bias || aligned16(a->bias)) &&
                    (!a->stats_out || ((uintptr_t)a->stats_out & 7) == 0),
                AFLDM_EALIGN, "%s: operands must be 16-byte aligned", name);
  if (mode == 0) {
    AFLDM_REQUIRE(a->H % 2 == 0 && a->W % 2 == 0, AFLDM_ESHAPE, "%s: H %d / W %d must be even", name, a->H, a->W);
    AFLDM_REQUIRE(pad_lo >= 0 && pad_lo <= 1 && pad_hi >= 0 && pad_hi <= 1 && pad_lo + pad_hi >= 1, AFLDM_ESHAPE,
                  "%s: padding (%d, %d) does not give an H/2 x W/2 output", name, pad_lo, pad_hi);
  } else {
    AFLDM_REQUIRE(a->Cout % 64 == 0, AFLDM_ESHAPE, "%s: Cout %d must be a multiple of 64", name, a->Cout);
  }
  const long long per_sample = (long long)a->H * a->W * a->C1 * (a->dtype == AFLDM_F32 ? 4 : 2);
  AFLDM_REQUIRE(per_sample <= 0x7fffffffLL, AFLDM_ESHAPE, "%s: one sample's input exceeds 2 GiB", name);
  const long long rows = (long long)a->B * (mode == 0 ? (a->H / 2) * (a->W / 2) : a->H * a->W);
  AFLDM_REQUIRE(rows <= 0x7fffffffLL, AFLDM_ESHAPE, "%s: too many output rows", name);
  return AFLDM_OK;
}

// Batch chunk: the largest divisor of B whose input operand fits a buffer descriptor (2 GiB), as afldm_conv2d does
int batch_chunk(const afldm_conv_args* a) {
  const long long per_sample = (long long)a->H * a->W * a->C1 * (a->dtype == AFLDM_F32 ? 4 : 2);
  int c = a->B;
  while (c > 1 && (a->B % c != 0 || per_sample * c > 0x7fffffffLL)) --c;
  return c;
}

template <typename T>
int run(int mode, const afldm_conv_args* a, int pad_lo, hipStream_t st) {
  const int ESZ = (int)sizeof(T);
  const int B = a->B, H = a->H, W = a->W, Cin = a->C1, Cout = a->Cout;
  const int Ho = mode == 0 ? H / 2 : H, Wo = mode == 0 ? W / 2 : W;
  const int plane = Ho * Wo, out_plane = mode == 0 ? plane : 4 * plane;
  const int S = splits(mode, a);
  const bool epi_stats = a->stats_out && epilogue_stats(plane);
  const int BN = bn_for(mode, Cout);
  const int N = mode == 0 ? Cout : 4 * Cout;
  const int taps = mode == 0 ? 9 : 4;
  const int kstep = 128 / ESZ;
  const int c = batch_chunk(a);
  for (int b0 = 0; b0 < B; b0 += c) {
    RsP p;
    p.x = (const char*)a->x1 + (size_t)b0 * H * W * Cin * ESZ;
    p.w = a->w;
    p.bias = a->bias;
    p.y = (char*)a->y + (size_t)b0 * out_plane * Cout * ESZ;
    p.stats = epi_stats ? a->stats_out + (size_t)b0 * S * Cout * 2 : nullptr;
    p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.Ho = Ho; p.Wo = Wo;
    p.M = c * plane;
    p.N = N;
    p.pad_lo = pad_lo;
    p.ksteps = taps * ((Cin + kstep - 1) / kstep);
    p.tiles_n = cdiv(N, BN);
    const long long xb = (long long)c * H * W * Cin, wb = (long long)N * taps * Cin;
    p.m_fast = wb > xb;
    p.stats_S = S;
    p.stats_Sp = plane >= kBM ? plane / kBM : 1;
    if (mode == 0) {
      if (BN == 128) launch<T, 0, 128>(p, st);
      else launch<T, 0, 64>(p, st);
    } else {
      if (BN == 128) launch<T, 1, 128>(p, st);
      else launch<T, 1, 64>(p, st);
    }
  }
  int rc = check_launch(mode == 0 ? "afldm_conv2d_s2" : "afldm_conv2d_up2");
  if (rc) return rc;
  if (a->stats_out && !epi_stats) return afldm_gn_stats(a->y, Cout, a->stats_out, B, out_plane, a->dtype, st);
  return AFLDM_OK;
}

int dispatch(int mode, const afldm_conv_args* a, int pad_lo, int pad_hi, afldm_stream_t stream) {
  const char* name = mode == 0 ? "afldm_conv2d_s2" : "afldm_conv2d_up2";
  int rc = validate(mode, a, pad_lo, pad_hi, name);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(a->dtype, return run<float>(mode, a, pad_lo, st), return run<bf16>(mode, a, pad_lo, st), name);
  return AFLDM_OK;
}

// fold of the 3 taps of one axis onto the 2 taps of output phase `ph`: {i-1: w0, i: w1+w2} / {i: w0+w1, i+1: w2}
__device__ __forceinline__ float fold3(const float* w, int stride, int ph, int t) {
  if (ph == 0) return t == 0 ? w[0] : w[stride] + w[2 * stride];
  return t == 0 ? w[0] + w[stride] : w[2 * stride];
}

template <typename T>
__global__ void __launch_bounds__(256) k_pack_up2(const float* __restrict__ src, T* __restrict__ dst, int Cout, int Cin) {
  // dst [4][Cout][2][2][Cin], src OIHW [Cout][Cin][3][3]; rows folded first, then columns, in fp32; one rounding
  const long long total = 16LL * Cout * Cin;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin);
    long long r = i / Cin;
    const int tw = (int)(r & 1), th = (int)((r >> 1) & 1);
    r >>= 2;
    const int co = (int)(r % Cout), ph = (int)(r / Cout);
    const int a = ph >> 1, c = ph & 1;
    const float* w = src + ((size_t)co * Cin + ci) * 9;
    float rows[3];
    for (int kw = 0; kw < 3; ++kw) rows[kw] = fold3(w + kw, 3, a, th);
    dst[i] = from_f32<T>(fold3(rows, 1, c, tw));
  }
}

}  // namespace

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_conv2d_s2(const afldm_conv_args* args, int pad_lo, int pad_hi, afldm_stream_t stream) {
  return dispatch(0, args, pad_lo, pad_hi, stream);
}

extern "C" int afldm_conv2d_up2(const afldm_conv_args* args, afldm_stream_t stream) {
  return dispatch(1, args, 0, 0, stream);
}

extern "C" int afldm_conv2d_s2_stats_splits(const afldm_conv_args* args) {
  if (!args || args->H < 2 || args->W < 2) return 1;
  return splits(0, args);
}

extern "C" int afldm_conv2d_up2_stats_splits(const afldm_conv_args* args) {
  if (!args || args->H < 1 || args->W < 1) return 1;
  return splits(1, args);
}

extern "C" int afldm_pack_weight_up2(const float* src, void* dst, int Cout, int Cin, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(src && dst, AFLDM_ENULL, "afldm_pack_weight_up2: NULL pointer");
  AFLDM_REQUIRE(Cout > 0 && Cin > 0, AFLDM_ESHAPE, "afldm_pack_weight_up2: empty shape");
  hipStream_t st = (hipStream_t)stream;
  const long long total = 16LL * Cout * Cin;
  const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  DISPATCH_T(dtype, hipLaunchKernelGGL(k_pack_up2<float>, dim3(grid), dim3(256), 0, st, src, (float*)dst, Cout, Cin),
             hipLaunchKernelGGL(k_pack_up2<bf16>, dim3(grid), dim3(256), 0, st, src, (bf16*)dst, Cout, Cin),
             "afldm_pack_weight_up2");
  return check_launch("afldm_pack_weight_up2");
}
