// pano.hip — MultiDiffusion (Bar-Tal et al., ICML 2023) on the graph-replayed engine: one large fp32 canvas [P, C, Hc, Wc] is
// sampled through overlapping S x S windows, the only planes the UNet ever sees.  A canvas with nwin = ny * nx windows is one
// engine batch of P * nwin; window k = iy * nx + ix has its corner at (oy[iy], ox[ix]) and covers (o + u) mod extent on an axis
// that wraps.  Three launches:
//   afldm_pano_step    the fused update: every window's reverse step, the overlap-weighted mean of the steps, and the next
//                      UNet input (the canvas cropped back into the windows) - the "sde" row (p, q, lo, hi, a, b, d, c):
//                        x0_k = clamp(p x + q e_k, lo, hi);  A = sum_k w x0_k;  E = sum_k w e_k;  W = sum_k w
//                        out  = a x + b A / W + d E / W + c z
//   afldm_window_fuse  canvas = sum_k w win_k / sum_k w   (the pixel-space blend of the per-window decodes)
//   afldm_window_crop  windows = crops of the canvas      (the engine's reset)
// and a fourth for outpainting, RePaint (repaint.hip) on the canvas:
//   afldm_pano_repaint_step  the same gather under the "repaint" row (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0), with the known
//                      canvas, the canvas mask m (1 = keep) and three canvas-shaped noise slots z_k, z_u, z_b:
//                        unknown = a A / W + b E / W + c z_u;  knownp = k0 known + k1 z_k
//                        out     = u0 (m knownp + (1 - m) unknown) + u1 z_b
// All of them are gathers: a thread owns canvas elements (or window elements, for the crop), walks the windows that cover them in
// ascending k with fp32 fmaf and writes what it owns - no atomics, no workspace, so a canvas's bits depend neither on P nor on its
// place in the batch, and canvas_out may alias the canvas.  Neighbouring threads are neighbours along X: canvas loads and stores,
// window stores and the weight plane are read and written along rows; with C = 4 a thread keeps the four channels of its pixel and
// the NHWC eps pixel of a window is one 16-byte (fp32) or 8-byte (bf16) load.  At FFHQ size the update moves a few hundred KB:
// latency-bound, like sde.hip.  The origin lists travel by value in the kernel arguments (at most 16 per axis), so a captured
// graph holds its geometry.
#include "step_common.hpp"

namespace afldm {

namespace {

constexpr int PANO_MAX_ORIGINS = 16;

struct pano_geom {
  int Hc, Wc, S, ny, nx, wrap_y, wrap_x;
  int oy[PANO_MAX_ORIGINS], ox[PANO_MAX_ORIGINS];
};

struct pano_row {
  float p, q, lo, hi, a, b, d, c;
};

// The two expressions of sde.hip's sde_update with every product and sum rounded on its own (no contraction into fma), left to
// right: what afldm_sde_step's one-element-per-thread form computes, so that one window of weight 1 gives its bits.  (That
// kernel's 16-byte form contracts some of them; the two differ in the last bit.)
__device__ __forceinline__ float pano_x0(float x, float e, const pano_row& r) {
#pragma clang fp contract(off)
  return clamp_nan(r.p * x + r.q * e, r.lo, r.hi);
}
__device__ __forceinline__ float pano_out(float x, float x0, float e, float z, const pano_row& r) {
#pragma clang fp contract(off)
  return r.a * x + r.b * x0 + r.d * e + r.c * z;
}

// The "repaint" row (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0) of afldm_pano_repaint_step.  x0 is pano_x0 under (p, q, lo, hi);
// outpaint_out takes the two window means and is repaint.hip's update from `unknown` on, every product and sum rounded on its
// own.  Where 1 - m is exactly 0 the model's side is left out of the sum instead of being added as 0 * unknown: the same bits
// for a finite `unknown`, and a NaN or inf of the model cannot reach a kept element.
struct outpaint_row {
  float p, q, lo, hi, a, b, c, k0, k1, u0, u1;
};

__device__ __forceinline__ float outpaint_out(float x0, float e, float kn, float m, float zk, float zu, float zb,
                                              const outpaint_row& r) {
#pragma clang fp contract(off)
  const float unknown = r.a * x0 + r.b * e + r.c * zu;
  const float knownp = r.k0 * kn + r.k1 * zk;
  const float om = 1.0f - m;
  const float y = om == 0.0f ? m * knownp : m * knownp + om * unknown;
  return r.u0 * y + r.u1 * zb;
}

// position of canvas coordinate Y inside the window at origin o; the window covers Y iff the result is in [0, S)
__device__ __forceinline__ int pano_pos(int Y, int o, int extent, int wrap) {
  int u = Y - o;
  if (wrap && u < 0) u += extent;
  return u;
}

// The checks the three entry points share, before any launch: at most 16 origins per axis, S <= extent, every window inside a
// non-wrapping axis (inside [0, extent) origins on a wrapping one), every coordinate covered.
int pano_check(const char* name, int Hc, int Wc, int S, const int* oy, int ny, const int* ox, int nx, int wrap_y, int wrap_x,
               pano_geom& g) {
  AFLDM_REQUIRE(oy && ox, AFLDM_ENULL, "%s: NULL origin list", name);
  AFLDM_REQUIRE(ny >= 1 && nx >= 1 && ny <= PANO_MAX_ORIGINS && nx <= PANO_MAX_ORIGINS, AFLDM_ESHAPE,
                "%s: %d x %d window origins, want 1 .. %d per axis", name, ny, nx, PANO_MAX_ORIGINS);
  AFLDM_REQUIRE(S >= 1 && Hc >= 1 && Wc >= 1 && S <= Hc && S <= Wc, AFLDM_ESHAPE, "%s: window %d on a %d x %d canvas", name, S, Hc,
                Wc);
  g.Hc = Hc; g.Wc = Wc; g.S = S; g.ny = ny; g.nx = nx; g.wrap_y = wrap_y != 0; g.wrap_x = wrap_x != 0;
  for (int i = 0; i < PANO_MAX_ORIGINS; ++i) {
    g.oy[i] = i < ny ? oy[i] : 0;
    g.ox[i] = i < nx ? ox[i] : 0;
  }
  for (int axis = 0; axis < 2; ++axis) {
    const int* o = axis ? g.ox : g.oy;
    const int n = axis ? nx : ny, extent = axis ? Wc : Hc, wrap = axis ? g.wrap_x : g.wrap_y;
    for (int i = 0; i < n; ++i)
      AFLDM_REQUIRE(o[i] >= 0 && (wrap ? o[i] < extent : o[i] <= extent - S), AFLDM_ESHAPE,
                    "%s: the window at %c origin %d (size %d) leaves the %s axis of extent %d", name, axis ? 'x' : 'y', o[i], S,
                    wrap ? "wrapping" : "non-wrapping", extent);
    for (int Y = 0; Y < extent; ++Y) {
      bool covered = false;
      for (int i = 0; i < n && !covered; ++i) {
        int u = Y - o[i];
        if (wrap && u < 0) u += extent;
        covered = u >= 0 && u < S;
      }
      AFLDM_REQUIRE(covered, AFLDM_ESHAPE, "%s: no window covers %c = %d", name, axis ? 'x' : 'y', Y);
    }
  }
  return AFLDM_OK;
}

}  // namespace

// canvas, canvas_out, noise rows: NCHW fp32 [P, C, Hc, Wc]; eps: NHWC T [P * nwin, S, S, C]; windows_out: NCHW fp32
// [P * nwin, C, S, S]; wt fp32 [S, S].  CV = 4: a thread owns the 4 channels of a pixel (C == 4, eps 4 T-aligned);
// CV = 1: one (channel, pixel) element per thread.  Per element the arithmetic is the same in both.
template <typename T, int CV>
__global__ void __launch_bounds__(256) k_pano_step(const float* canvas, const T* __restrict__ eps, const float* __restrict__ noise,
                                                   size_t noise_step_stride, const float* __restrict__ wt, float* canvas_out,
                                                   float* __restrict__ windows_out, const float* __restrict__ coef,
                                                   const int* __restrict__ step_idx, int P, int C, pano_geom g) {
  const int s = *step_idx;
  const float* rp = coef + 8 * (size_t)s;
  const pano_row r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7]};
  const bool read_z = noise != nullptr && r.c != 0.f;          // c = 0: the row may hold anything (0 * NaN is not 0)
  const float* z = read_z ? noise + (size_t)s * noise_step_stride : nullptr;
  const size_t HW = (size_t)g.Hc * g.Wc, SS = (size_t)g.S * g.S;
  const int nwin = g.ny * g.nx;
  const size_t items = (size_t)P * (CV == 4 ? 1 : C) * HW;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = it % HW, plane = it / HW;
    const int c0 = CV == 4 ? 0 : (int)(plane % C);
    const size_t Pi = CV == 4 ? plane : plane / C;
    const int Y = (int)(pix / g.Wc), X = (int)(pix % g.Wc);
    const size_t base = (Pi * C + c0) * HW + pix;               // channel c0 + j: base + j HW
    float x[CV], A[CV], E[CV], W = 0.f;
#pragma unroll
    for (int j = 0; j < CV; ++j) {
      x[j] = canvas[base + j * HW];
      A[j] = 0.f;
      E[j] = 0.f;
    }
    for (int iy = 0; iy < g.ny; ++iy) {
      const int u = pano_pos(Y, g.oy[iy], g.Hc, g.wrap_y);
      if (u < 0 || u >= g.S) continue;
      for (int ix = 0; ix < g.nx; ++ix) {
        const int v = pano_pos(X, g.ox[ix], g.Wc, g.wrap_x);
        if (v < 0 || v >= g.S) continue;
        const size_t win = Pi * nwin + (size_t)(iy * g.nx + ix);
        const T* ep = eps + (win * SS + (size_t)u * g.S + v) * C + c0;
        const float w = wt[(size_t)u * g.S + v];
        float e[CV];
        if constexpr (CV == 4) {
          load4<T>(ep, e[0], e[1], e[2], e[3]);
        } else {
          e[0] = to_f32(ep[0]);
        }
#pragma unroll
        for (int j = 0; j < CV; ++j) {
          A[j] = fmaf(w, pano_x0(x[j], e[j], r), A[j]);
          E[j] = fmaf(w, e[j], E[j]);
        }
        W += w;
      }
    }
    float out[CV];
#pragma unroll
    for (int j = 0; j < CV; ++j) {
      out[j] = pano_out(x[j], A[j] / W, E[j] / W, read_z ? z[base + j * HW] : 0.f, r);
      canvas_out[base + j * HW] = out[j];
    }
    for (int iy = 0; iy < g.ny; ++iy) {
      const int u = pano_pos(Y, g.oy[iy], g.Hc, g.wrap_y);
      if (u < 0 || u >= g.S) continue;
      for (int ix = 0; ix < g.nx; ++ix) {
        const int v = pano_pos(X, g.ox[ix], g.Wc, g.wrap_x);
        if (v < 0 || v >= g.S) continue;
        const size_t win = Pi * nwin + (size_t)(iy * g.nx + ix);
        float* wp = windows_out + (win * C + c0) * SS + (size_t)u * g.S + v;
#pragma unroll
        for (int j = 0; j < CV; ++j) wp[j * SS] = out[j];
      }
    }
  }
}

// k_pano_step's gather with the "repaint" row: canvas, known, canvas_out and the three noise slots NCHW fp32 [P, C, Hc, Wc], mask
// fp32 [P, 1, Hc, Wc] (1 = keep), the rest as above.  A slot whose coefficient (k1, c, u1) is 0 is not loaded (uniform: the row is
// the same for every thread).
template <typename T, int CV>
__global__ void __launch_bounds__(256) k_pano_repaint_step(const float* canvas, const T* __restrict__ eps,
                                                           const float* __restrict__ known, const float* __restrict__ mask,
                                                           const float* __restrict__ noise, size_t noise_step_stride,
                                                           size_t noise_slot_stride, const float* __restrict__ wt,
                                                           float* canvas_out, float* __restrict__ windows_out,
                                                           const float* __restrict__ coef, const int* __restrict__ step_idx, int P,
                                                           int C, pano_geom g) {
  const int s = *step_idx;
  const float* rp = coef + 12 * (size_t)s;
  const outpaint_row r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8], rp[9], rp[10]};
  const pano_row rx{r.p, r.q, r.lo, r.hi, 0.f, 0.f, 0.f, 0.f};
  const bool has_k = r.k1 != 0.f, has_u = r.c != 0.f, has_b = r.u1 != 0.f;
  const float* zk = noise + (size_t)s * noise_step_stride;
  const float* zu = zk + noise_slot_stride;
  const float* zb = zu + noise_slot_stride;
  const size_t HW = (size_t)g.Hc * g.Wc, SS = (size_t)g.S * g.S;
  const int nwin = g.ny * g.nx;
  const size_t items = (size_t)P * (CV == 4 ? 1 : C) * HW;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = it % HW, plane = it / HW;
    const int c0 = CV == 4 ? 0 : (int)(plane % C);
    const size_t Pi = CV == 4 ? plane : plane / C;
    const int Y = (int)(pix / g.Wc), X = (int)(pix % g.Wc);
    const size_t base = (Pi * C + c0) * HW + pix;               // channel c0 + j: base + j HW
    const float m = mask[Pi * HW + pix];
    float x[CV], A[CV], E[CV], W = 0.f;
#pragma unroll
    for (int j = 0; j < CV; ++j) {
      x[j] = canvas[base + j * HW];
      A[j] = 0.f;
      E[j] = 0.f;
    }
    for (int iy = 0; iy < g.ny; ++iy) {
      const int u = pano_pos(Y, g.oy[iy], g.Hc, g.wrap_y);
      if (u < 0 || u >= g.S) continue;
      for (int ix = 0; ix < g.nx; ++ix) {
        const int v = pano_pos(X, g.ox[ix], g.Wc, g.wrap_x);
        if (v < 0 || v >= g.S) continue;
        const size_t win = Pi * nwin + (size_t)(iy * g.nx + ix);
        const T* ep = eps + (win * SS + (size_t)u * g.S + v) * C + c0;
        const float w = wt[(size_t)u * g.S + v];
        float e[CV];
        if constexpr (CV == 4) {
          load4<T>(ep, e[0], e[1], e[2], e[3]);
        } else {
          e[0] = to_f32(ep[0]);
        }
#pragma unroll
        for (int j = 0; j < CV; ++j) {
          A[j] = fmaf(w, pano_x0(x[j], e[j], rx), A[j]);
          E[j] = fmaf(w, e[j], E[j]);
        }
        W += w;
      }
    }
    float out[CV];
#pragma unroll
    for (int j = 0; j < CV; ++j) {
      const size_t i = base + j * HW;
      out[j] = outpaint_out(A[j] / W, E[j] / W, known[i], m, has_k ? zk[i] : 0.f, has_u ? zu[i] : 0.f, has_b ? zb[i] : 0.f, r);
      canvas_out[i] = out[j];
    }
    for (int iy = 0; iy < g.ny; ++iy) {
      const int u = pano_pos(Y, g.oy[iy], g.Hc, g.wrap_y);
      if (u < 0 || u >= g.S) continue;
      for (int ix = 0; ix < g.nx; ++ix) {
        const int v = pano_pos(X, g.ox[ix], g.Wc, g.wrap_x);
        if (v < 0 || v >= g.S) continue;
        const size_t win = Pi * nwin + (size_t)(iy * g.nx + ix);
        float* wp = windows_out + (win * C + c0) * SS + (size_t)u * g.S + v;
#pragma unroll
        for (int j = 0; j < CV; ++j) wp[j * SS] = out[j];
      }
    }
  }
}

// win: NCHW T [P * nwin, C, S, S]; canvas fp32 [P, C, Hc, Wc]; one canvas element per thread
template <typename T>
__global__ void __launch_bounds__(256) k_window_fuse(const T* __restrict__ win, const float* __restrict__ wt,
                                                     float* __restrict__ canvas, int P, int C, pano_geom g) {
  const size_t HW = (size_t)g.Hc * g.Wc, SS = (size_t)g.S * g.S;
  const int nwin = g.ny * g.nx;
  const size_t items = (size_t)P * C * HW;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = it % HW, plane = it / HW;
    const int c = (int)(plane % C);
    const size_t Pi = plane / C;
    const int Y = (int)(pix / g.Wc), X = (int)(pix % g.Wc);
    float A = 0.f, W = 0.f;
    for (int iy = 0; iy < g.ny; ++iy) {
      const int u = pano_pos(Y, g.oy[iy], g.Hc, g.wrap_y);
      if (u < 0 || u >= g.S) continue;
      for (int ix = 0; ix < g.nx; ++ix) {
        const int v = pano_pos(X, g.ox[ix], g.Wc, g.wrap_x);
        if (v < 0 || v >= g.S) continue;
        const size_t k = Pi * nwin + (size_t)(iy * g.nx + ix);
        const float w = wt[(size_t)u * g.S + v];
        A = fmaf(w, to_f32(win[(k * C + c) * SS + (size_t)u * g.S + v]), A);
        W += w;
      }
    }
    canvas[it] = A / W;
  }
}

// canvas fp32 [P, C, Hc, Wc] -> win fp32 [P * nwin, C, S, S]; one window element per thread
__global__ void __launch_bounds__(256) k_window_crop(const float* __restrict__ canvas, float* __restrict__ win, int P, int C,
                                                     pano_geom g) {
  const size_t HW = (size_t)g.Hc * g.Wc, SS = (size_t)g.S * g.S;
  const int nwin = g.ny * g.nx;
  const size_t items = (size_t)P * nwin * C * SS;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
    const size_t pos = it % SS, plane = it / SS;
    const int c = (int)(plane % C);
    const size_t k = plane / C;
    const int kk = (int)(k % nwin);
    const size_t Pi = k / nwin;
    int Y = g.oy[kk / g.nx] + (int)(pos / g.S), X = g.ox[kk % g.nx] + (int)(pos % g.S);
    if (Y >= g.Hc) Y -= g.Hc;                                   // (only on an axis that wraps: pano_check)
    if (X >= g.Wc) X -= g.Wc;
    win[it] = canvas[(Pi * C + c) * HW + (size_t)Y * g.Wc + X];
  }
}

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_pano_step(const float* canvas, const void* eps, const float* noise, size_t noise_step_stride, const float* wt,
                               float* canvas_out, float* windows_out, const float* coef, int* step_idx, int advance, int P, int C,
                               int Hc, int Wc, int S, const int* oy, int ny, const int* ox, int nx, int wrap_y, int wrap_x, int dtype,
                               afldm_stream_t stream) {
  AFLDM_REQUIRE(canvas && eps && wt && canvas_out && windows_out && coef && step_idx, AFLDM_ENULL, "afldm_pano_step: NULL pointer");
  AFLDM_REQUIRE(P > 0 && C > 0, AFLDM_ESHAPE, "afldm_pano_step: bad shape");
  AFLDM_REQUIRE(dtype == AFLDM_F32 || dtype == AFLDM_BF16, AFLDM_EDTYPE, "afldm_pano_step: unknown dtype %d", dtype);
  pano_geom g;
  const int rc = pano_check("afldm_pano_step", Hc, Wc, S, oy, ny, ox, nx, wrap_y, wrap_x, g);
  if (rc != AFLDM_OK) return rc;
  const size_t n = (size_t)P * C * Hc * Wc;
  AFLDM_REQUIRE(noise == nullptr || noise_step_stride >= n, AFLDM_ESHAPE,
                "afldm_pano_step: noise_step_stride smaller than one step's P*C*Hc*Wc");
  hipStream_t st = (hipStream_t)stream;
  // the four channels of a pixel as one load: 16 bytes of fp32, 8 of bf16
  const bool c4 = C == 4 && (reinterpret_cast<uintptr_t>(eps) & (dtype == AFLDM_F32 ? 15 : 7)) == 0;
#define LAUNCH(T, CV)                                                                                               \
  (k_pano_step<T, CV><<<step_grid(n / CV), 256, 0, st>>>(canvas, (const T*)eps, noise, noise_step_stride, wt, canvas_out, \
                                                         windows_out, coef, step_idx, P, C, g))
  STEP_DISPATCH(dtype, c4, LAUNCH, "afldm_pano_step");
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_pano_step");
}

extern "C" int afldm_pano_repaint_step(const float* canvas, const void* eps, const float* known, const float* mask,
                                       const float* noise, size_t noise_step_stride, size_t noise_slot_stride, const float* wt,
                                       float* canvas_out, float* windows_out, const float* coef, int* step_idx, int advance, int P,
                                       int C, int Hc, int Wc, int S, const int* oy, int ny, const int* ox, int nx, int wrap_y,
                                       int wrap_x, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(canvas && eps && known && mask && noise && wt && canvas_out && windows_out && coef && step_idx, AFLDM_ENULL,
                "afldm_pano_repaint_step: NULL pointer");
  AFLDM_REQUIRE(P > 0 && C > 0, AFLDM_ESHAPE, "afldm_pano_repaint_step: bad shape");
  AFLDM_REQUIRE(dtype == AFLDM_F32 || dtype == AFLDM_BF16, AFLDM_EDTYPE, "afldm_pano_repaint_step: unknown dtype %d", dtype);
  pano_geom g;
  const int rc = pano_check("afldm_pano_repaint_step", Hc, Wc, S, oy, ny, ox, nx, wrap_y, wrap_x, g);
  if (rc != AFLDM_OK) return rc;
  const size_t n = (size_t)P * C * Hc * Wc;
  AFLDM_REQUIRE(noise_slot_stride >= n, AFLDM_ESHAPE, "afldm_pano_repaint_step: noise_slot_stride smaller than one slot's P*C*Hc*Wc");
  AFLDM_REQUIRE(noise_step_stride >= 2 * noise_slot_stride + n, AFLDM_ESHAPE,
                "afldm_pano_repaint_step: noise_step_stride smaller than one step's three slots");
  hipStream_t st = (hipStream_t)stream;
  const bool c4 = C == 4 && (reinterpret_cast<uintptr_t>(eps) & (dtype == AFLDM_F32 ? 15 : 7)) == 0;
#define LAUNCH(T, CV)                                                                                                     \
  (k_pano_repaint_step<T, CV><<<step_grid(n / CV), 256, 0, st>>>(canvas, (const T*)eps, known, mask, noise, noise_step_stride, \
                                                                 noise_slot_stride, wt, canvas_out, windows_out, coef, step_idx, \
                                                                 P, C, g))
  STEP_DISPATCH(dtype, c4, LAUNCH, "afldm_pano_repaint_step");
#undef LAUNCH
  step_advance(advance, step_idx, st);
  return check_launch("afldm_pano_repaint_step");
}

extern "C" int afldm_window_fuse(const void* windows, const float* wt, float* canvas, int P, int C, int Hc, int Wc, int S,
                                 const int* oy, int ny, const int* ox, int nx, int wrap_y, int wrap_x, int dtype,
                                 afldm_stream_t stream) {
  AFLDM_REQUIRE(windows && wt && canvas, AFLDM_ENULL, "afldm_window_fuse: NULL pointer");
  AFLDM_REQUIRE(P > 0 && C > 0, AFLDM_ESHAPE, "afldm_window_fuse: bad shape");
  AFLDM_REQUIRE(dtype == AFLDM_F32 || dtype == AFLDM_BF16, AFLDM_EDTYPE, "afldm_window_fuse: unknown dtype %d", dtype);
  pano_geom g;
  const int rc = pano_check("afldm_window_fuse", Hc, Wc, S, oy, ny, ox, nx, wrap_y, wrap_x, g);
  if (rc != AFLDM_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)P * C * Hc * Wc;
  DISPATCH_T(dtype, (k_window_fuse<float><<<step_grid(n), 256, 0, st>>>((const float*)windows, wt, canvas, P, C, g)),
             (k_window_fuse<bf16><<<step_grid(n), 256, 0, st>>>((const bf16*)windows, wt, canvas, P, C, g)), "afldm_window_fuse");
  return check_launch("afldm_window_fuse");
}

extern "C" int afldm_window_crop(const float* canvas, float* windows, int P, int C, int Hc, int Wc, int S, const int* oy, int ny,
                                 const int* ox, int nx, int wrap_y, int wrap_x, afldm_stream_t stream) {
  AFLDM_REQUIRE(canvas && windows, AFLDM_ENULL, "afldm_window_crop: NULL pointer");
  AFLDM_REQUIRE(P > 0 && C > 0, AFLDM_ESHAPE, "afldm_window_crop: bad shape");
  pano_geom g;
  const int rc = pano_check("afldm_window_crop", Hc, Wc, S, oy, ny, ox, nx, wrap_y, wrap_x, g);
  if (rc != AFLDM_OK) return rc;
  const size_t n = (size_t)P * ny * nx * C * S * S;
  k_window_crop<<<step_grid(n), 256, 0, (hipStream_t)stream>>>(canvas, windows, P, C, g);
  return check_launch("afldm_window_crop");
}
