// hires.hip — high-resolution sampling (after DemoFusion: Du et al., CVPR 2024) on the graph-replayed engine: a canvas
// [P, C, Hc, Wc] of Hc = Wc = scale * S latents is denoised through the S x S windows of a UNet trained at S.  Per canvas the window
// batch holds the nwin = ny * nx local windows of pano.hip (window k = iy * nx + ix at (oy[iy], ox[ix]), no wrap) and then the
// scale^2 dilated windows: window nwin + i * scale + j covers the canvas elements (i + scale u, j + scale v).  Two launches:
//   afldm_hires_step     the fused update on the "hires" row (p, q, lo, hi, a, b, c, k0, k1, r, g, f), per canvas element x at (Y, X):
//                          x0_k = clamp(p x + q e_k, lo, hi);  A = sum_k w x0_k;  E = sum_k w e_k;  W = sum_k w       (local windows)
//                          e_g  = eps of the dilated window nwin + (Y % scale) scale + X % scale at (Y / scale, X / scale)
//                          x0m  = (1 - g) A / W + g clamp(p x + q e_g, lo, hi);  em = (1 - g) E / W + g e_g
//                          xp   = a x0m + b em + c z_u
//                          out  = r (k0 ref + k1 eps_ref) + (1 - r) xp
//                        canvas_out = out; the local windows of the next UNet input are its crops, the dilated ones the sub-lattices
//                        of  out + f (Lh out Lw^T - out)  per plane: the low-pass is seen by the UNet only, never by the canvas.
//   afldm_hires_windows  that last line alone, for a given canvas and f (the engine's reset, the eager loop).
// One 256-thread workgroup owns a (P, ch) plane, Hc <= 64: a thread gathers up to 16 elements as k_pano_step gathers one (ascending
// k, fp32 fmaf, every other product and sum rounded on its own) and keeps `out` in registers.  Where f != 0 the plane also goes to
// LDS and the two passes of plane_pass.hpp, which ilvr.hip runs too, work out of it - the row pass t = out Lw^T, then the column
// pass Lh t, each output one ascending-k fmaf chain - in three Hc x (Hc | 1) fp32 tiles, under 50 KB.  No atomics, no workspace: a
// plane's bits depend neither on P nor on the grid.  All of a plane's canvas reads come before the first barrier and all stores
// after the last, so canvas_out may alias the canvas.  Uniform branches (the row is the same for every thread): with g = 0 the
// dilated eps is not read, with c = 0 the noise, with r = 0 ref and eps_ref, with f = 0 Lh and Lw, and the passes are skipped.
// The origin lists travel by value in the kernel arguments (at most 16 per axis), so a captured graph holds its geometry.
#include "plane_pass.hpp"

namespace afldm {

namespace {

constexpr int HIRES_MAX_ORIGINS = 16;
constexpr int HIRES_HMAX = PLANE_SMAX;
constexpr int HIRES_THREADS = PLANE_THREADS;
constexpr int HIRES_PER_THREAD = HIRES_HMAX * HIRES_HMAX / HIRES_THREADS;

struct hires_geom {
  int Hc, S, ny, nx, scale;
  int oy[HIRES_MAX_ORIGINS], ox[HIRES_MAX_ORIGINS];
};

struct hires_row {
  float p, q, lo, hi, a, b, c, k0, k1, r, g, f;
};

__device__ __forceinline__ float hires_x0(float x, float e, const hires_row& r) {
#pragma clang fp contract(off)
  return clamp_nan(r.p * x + r.q * e, r.lo, r.hi);
}

// the update from the two local means on: mx0 = A / W, me = E / W; eg, z, rf, er are only looked at where g, c, r are not 0
__device__ __forceinline__ float hires_out(float x, float mx0, float me, float eg, float z, float rf, float er, const hires_row& r) {
#pragma clang fp contract(off)
  float x0m = mx0, em = me;
  if (r.g != 0.0f) {
    const float og = 1.0f - r.g;
    x0m = og * mx0 + r.g * hires_x0(x, eg, r);
    em = og * me + r.g * eg;
  }
  const float xp = r.a * x0m + r.b * em + r.c * z;
  if (r.r == 0.0f) return xp;
  return r.r * (r.k0 * rf + r.k1 * er) + (1.0f - r.r) * xp;
}

__device__ __forceinline__ float hires_blend(float out, float lp, float f) {
#pragma clang fp contract(off)
  return out + f * (lp - out);
}

// The tail both kernels share.  out[u]: the plane's element tid + 256 u (the caller's registers; with f != 0 the caller has also
// written the plane to the LDS tile `lds`, pitch Hc | 1, and not yet synchronised).  Stores the windows of plane (Pi, ch):
// the local crops, and the dilated views of out + f (Lh out Lw^T - out).
__device__ __forceinline__ void hires_tail(const float (&out)[HIRES_PER_THREAD], float f, const float* __restrict__ Lh,
                                           const float* __restrict__ Lw, float* __restrict__ windows_out, size_t Pi, int ch, int C,
                                           const hires_geom& g, float* lds) {
  const int tid = threadIdx.x;
  const int H = g.Hc, Pp = H | 1, HW = H * H;
  const int nwin = g.ny * g.nx, NW = nwin + g.scale * g.scale;
  const size_t SS = (size_t)g.S * g.S;
  float* td = lds;                   // out, then the result of the column pass
  float* tt = lds + H * Pp;          // the row pass's output
  float* tm = lds + 2 * H * Pp;      // Lw, then Lh
  if (f != 0.0f) {
    plane_load_matrix(Lw, tm, H, Pp, tid);
    __syncthreads();                                   // every read of the canvas is behind us
    plane_pass(td, tm, Pp, 1, tt, H, Pp, tid);        // t[i][j] = sum_k out[i][k] Lw[j][k]
    __syncthreads();
    if (Lh != Lw) {                                    // (uniform; the same matrix twice is already there)
      plane_load_matrix(Lh, tm, H, Pp, tid);
      __syncthreads();
    }
    plane_pass(tm, tt, 1, Pp, td, H, Pp, tid);        // lp[i][j] = sum_k Lh[i][k] t[k][j]
    __syncthreads();
  }
  float* wbase = windows_out + (Pi * NW * C + ch) * SS;        // window k of this plane: wbase + k C SS
#pragma unroll
  for (int u = 0; u < HIRES_PER_THREAD; ++u) {
    const int i = tid + u * HIRES_THREADS;
    if (i >= HW) break;
    const int Y = i / H, X = i - Y * H;
    for (int iy = 0; iy < g.ny; ++iy) {
      const int wu = Y - g.oy[iy];
      if (wu < 0 || wu >= g.S) continue;
      for (int ix = 0; ix < g.nx; ++ix) {
        const int wv = X - g.ox[ix];
        if (wv < 0 || wv >= g.S) continue;
        wbase[(size_t)(iy * g.nx + ix) * C * SS + (size_t)wu * g.S + wv] = out[u];
      }
    }
    const int dy = Y / g.scale, dx = X / g.scale;
    const int kd = nwin + (Y - dy * g.scale) * g.scale + (X - dx * g.scale);
    wbase[(size_t)kd * C * SS + (size_t)dy * g.S + dx] = f != 0.0f ? hires_blend(out[u], td[Y * Pp + X], f) : out[u];
  }
}

// The checks both entry points share, before any launch.
int hires_check(const char* name, int Hc, int Wc, int S, const int* oy, int ny, const int* ox, int nx, int scale, hires_geom& g) {
  AFLDM_REQUIRE(oy && ox, AFLDM_ENULL, "%s: NULL origin list", name);
  AFLDM_REQUIRE(scale >= 1, AFLDM_ESHAPE, "%s: scale %d, want >= 1", name, scale);
  AFLDM_REQUIRE(Hc == Wc && Hc >= 2 && Hc <= HIRES_HMAX, AFLDM_ESHAPE,
                "%s: canvas %d x %d (square canvases of 2 .. %d only: one workgroup holds a plane in LDS)", name, Hc, Wc, HIRES_HMAX);
  AFLDM_REQUIRE(S >= 1 && (long long)scale * S == Hc, AFLDM_ESHAPE, "%s: a canvas of %d is not scale %d times the window %d", name, Hc,
                scale, S);
  AFLDM_REQUIRE(ny >= 1 && nx >= 1 && ny <= HIRES_MAX_ORIGINS && nx <= HIRES_MAX_ORIGINS, AFLDM_ESHAPE,
                "%s: %d x %d window origins, want 1 .. %d per axis", name, ny, nx, HIRES_MAX_ORIGINS);
  g.Hc = Hc; g.S = S; g.ny = ny; g.nx = nx; g.scale = scale;
  for (int i = 0; i < HIRES_MAX_ORIGINS; ++i) {
    g.oy[i] = i < ny ? oy[i] : 0;
    g.ox[i] = i < nx ? ox[i] : 0;
  }
  for (int axis = 0; axis < 2; ++axis) {
    const int* o = axis ? g.ox : g.oy;
    const int n = axis ? nx : ny;
    for (int i = 0; i < n; ++i)
      AFLDM_REQUIRE(o[i] >= 0 && o[i] <= Hc - S, AFLDM_ESHAPE, "%s: the window at %c origin %d (size %d) leaves the canvas of %d", name,
                    axis ? 'x' : 'y', o[i], S, Hc);
    for (int Y = 0; Y < Hc; ++Y) {
      bool covered = false;
      for (int i = 0; i < n && !covered; ++i) covered = Y >= o[i] && Y - o[i] < S;
      AFLDM_REQUIRE(covered, AFLDM_ESHAPE, "%s: no window covers %c = %d", name, axis ? 'x' : 'y', Y);
    }
  }
  return AFLDM_OK;
}

inline size_t hires_lds_bytes(int Hc) { return (size_t)3 * Hc * (Hc | 1) * sizeof(float); }

}  // namespace

// canvas, ref, eps_ref, canvas_out, noise rows: NCHW fp32 [P, C, Hc, Hc]; eps: NHWC T [P * NW, S, S, C]; windows_out: NCHW fp32
// [P * NW, C, S, S], NW = nwin + scale^2; wt fp32 [S, S]; Lh, Lw fp32 [Hc, Hc].  blockIdx.x = P * C + ch.
template <typename T>
__global__ void __launch_bounds__(HIRES_THREADS) k_hires_step(const float* canvas, const T* __restrict__ eps,
                                                              const float* __restrict__ ref, const float* __restrict__ eps_ref,
                                                              const float* __restrict__ noise, size_t noise_step_stride,
                                                              const float* __restrict__ wt, const float* __restrict__ Lh,
                                                              const float* __restrict__ Lw, float* canvas_out,
                                                              float* __restrict__ windows_out, const float* __restrict__ coef,
                                                              const int* __restrict__ step_idx, int C, hires_geom g) {
  extern __shared__ float hires_lds[];
  const int s = *step_idx;
  const float* rp = coef + 12 * (size_t)s;
  const hires_row r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8], rp[9], rp[10], rp[11]};
  const int tid = threadIdx.x;
  const int H = g.Hc, Pp = H | 1, HW = H * H;
  const size_t plane = blockIdx.x;
  const size_t Pi = plane / C;
  const int ch = (int)(plane - Pi * C);
  const int nwin = g.ny * g.nx, NW = nwin + g.scale * g.scale;
  const size_t SS = (size_t)g.S * g.S;
  const bool has_z = noise != nullptr && r.c != 0.0f, has_r = r.r != 0.0f, has_g = r.g != 0.0f, has_f = r.f != 0.0f;
  const float* xpl = canvas + plane * HW;
  const float* zpl = has_z ? noise + (size_t)s * noise_step_stride + plane * HW : nullptr;
  const float* rpl = ref + plane * HW;
  const float* epl = eps_ref + plane * HW;
  const T* ebase = eps + Pi * NW * SS * C + ch;                 // window k of this canvas, pixel q: ebase + (k SS + q) C
  float out[HIRES_PER_THREAD];
#pragma unroll
  for (int u = 0; u < HIRES_PER_THREAD; ++u) {
    const int i = tid + u * HIRES_THREADS;
    out[u] = 0.0f;
    if (i >= HW) break;
    const int Y = i / H, X = i - Y * H;
    const float x = xpl[i];
    float A = 0.0f, E = 0.0f, W = 0.0f;
    for (int iy = 0; iy < g.ny; ++iy) {
      const int wu = Y - g.oy[iy];
      if (wu < 0 || wu >= g.S) continue;
      for (int ix = 0; ix < g.nx; ++ix) {
        const int wv = X - g.ox[ix];
        if (wv < 0 || wv >= g.S) continue;
        const size_t q = (size_t)wu * g.S + wv;
        const float e = to_f32(ebase[((size_t)(iy * g.nx + ix) * SS + q) * C]);
        const float w = wt[q];
        A = fmaf(w, hires_x0(x, e, r), A);
        E = fmaf(w, e, E);
        W += w;
      }
    }
    float eg = 0.0f;
    if (has_g) {
      const int dy = Y / g.scale, dx = X / g.scale;
      const int kd = nwin + (Y - dy * g.scale) * g.scale + (X - dx * g.scale);
      eg = to_f32(ebase[((size_t)kd * SS + (size_t)dy * g.S + dx) * C]);
    }
    out[u] = hires_out(x, A / W, E / W, eg, has_z ? zpl[i] : 0.0f, has_r ? rpl[i] : 0.0f, has_r ? epl[i] : 0.0f, r);
    if (has_f) hires_lds[Y * Pp + X] = out[u];
  }
  hires_tail(out, r.f, Lh, Lw, windows_out, Pi, ch, C, g, hires_lds);
  float* opl = canvas_out + plane * HW;
#pragma unroll
  for (int u = 0; u < HIRES_PER_THREAD; ++u) {
    const int i = tid + u * HIRES_THREADS;
    if (i >= HW) break;
    opl[i] = out[u];
  }
}

__global__ void __launch_bounds__(HIRES_THREADS) k_hires_windows(const float* __restrict__ canvas, const float* __restrict__ Lh,
                                                                 const float* __restrict__ Lw, float f,
                                                                 float* __restrict__ windows_out, int C, hires_geom g) {
  extern __shared__ float hires_lds[];
  const int tid = threadIdx.x;
  const int H = g.Hc, Pp = H | 1, HW = H * H;
  const size_t plane = blockIdx.x;
  const size_t Pi = plane / C;
  const int ch = (int)(plane - Pi * C);
  const float* xpl = canvas + plane * HW;
  float out[HIRES_PER_THREAD];
#pragma unroll
  for (int u = 0; u < HIRES_PER_THREAD; ++u) {
    const int i = tid + u * HIRES_THREADS;
    out[u] = 0.0f;
    if (i >= HW) break;
    out[u] = xpl[i];
    if (f != 0.0f) {
      const int Y = i / H;
      hires_lds[Y * Pp + (i - Y * H)] = out[u];
    }
  }
  hires_tail(out, f, Lh, Lw, windows_out, Pi, ch, C, g, hires_lds);
}

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_hires_step(const float* canvas, const void* eps, const float* ref, const float* eps_ref, const float* noise,
                                size_t noise_step_stride, const float* wt, const float* Lh, const float* Lw, float* canvas_out,
                                float* windows_out, const float* coef, int* step_idx, int advance, int P, int C, int Hc, int Wc, int S,
                                const int* oy, int ny, const int* ox, int nx, int scale, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(canvas && eps && ref && eps_ref && wt && Lh && Lw && canvas_out && windows_out && coef && step_idx, AFLDM_ENULL,
                "afldm_hires_step: NULL pointer");
  AFLDM_REQUIRE(P > 0 && C > 0, AFLDM_ESHAPE, "afldm_hires_step: bad shape");
  AFLDM_REQUIRE(dtype == AFLDM_F32 || dtype == AFLDM_BF16, AFLDM_EDTYPE, "afldm_hires_step: unknown dtype %d", dtype);
  hires_geom g;
  const int rc = hires_check("afldm_hires_step", Hc, Wc, S, oy, ny, ox, nx, scale, g);
  if (rc != AFLDM_OK) return rc;
  AFLDM_REQUIRE((long long)P * C <= 0x7fffffffLL, AFLDM_ESHAPE, "afldm_hires_step: P * C = %lld planes exceed the grid",
                (long long)P * C);
  const size_t n = (size_t)P * C * Hc * Wc;
  AFLDM_REQUIRE(noise == nullptr || noise_step_stride >= n, AFLDM_ESHAPE,
                "afldm_hires_step: noise_step_stride smaller than one step's P*C*Hc*Wc");
  hipStream_t st = (hipStream_t)stream;
  const int grid = P * C;
  const size_t lds = hires_lds_bytes(Hc);
  DISPATCH_T(dtype,
             (k_hires_step<float><<<grid, HIRES_THREADS, lds, st>>>(canvas, (const float*)eps, ref, eps_ref, noise, noise_step_stride,
                                                                    wt, Lh, Lw, canvas_out, windows_out, coef, step_idx, C, g)),
             (k_hires_step<bf16><<<grid, HIRES_THREADS, lds, st>>>(canvas, (const bf16*)eps, ref, eps_ref, noise, noise_step_stride, wt,
                                                                   Lh, Lw, canvas_out, windows_out, coef, step_idx, C, g)),
             "afldm_hires_step");
  step_advance(advance, step_idx, st);
  return check_launch("afldm_hires_step");
}

extern "C" int afldm_hires_windows(const float* canvas, const float* Lh, const float* Lw, float f, float* windows_out, int P, int C,
                                   int Hc, int Wc, int S, const int* oy, int ny, const int* ox, int nx, int scale,
                                   afldm_stream_t stream) {
  AFLDM_REQUIRE(canvas && windows_out, AFLDM_ENULL, "afldm_hires_windows: NULL pointer");
  AFLDM_REQUIRE(f == 0.0f || (Lh && Lw), AFLDM_ENULL, "afldm_hires_windows: Lh / Lw is NULL but f is not 0");
  AFLDM_REQUIRE(P > 0 && C > 0, AFLDM_ESHAPE, "afldm_hires_windows: bad shape");
  hires_geom g;
  const int rc = hires_check("afldm_hires_windows", Hc, Wc, S, oy, ny, ox, nx, scale, g);
  if (rc != AFLDM_OK) return rc;
  AFLDM_REQUIRE((long long)P * C <= 0x7fffffffLL, AFLDM_ESHAPE, "afldm_hires_windows: P * C = %lld planes exceed the grid",
                (long long)P * C);
  k_hires_windows<<<P * C, HIRES_THREADS, hires_lds_bytes(Hc), (hipStream_t)stream>>>(canvas, Lh, Lw, f, windows_out, C, g);
  return check_launch("afldm_hires_windows");
}
