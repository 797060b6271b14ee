// plane_pass.hpp — a dense [S][S] matrix applied to one side of a whole S x S fp32 plane held in LDS by one 256-thread workgroup,
// S <= 64: the two passes of L d L^T in ilvr.hip (the low band of ILVR's guidance) and hires.hip (the low-pass of the dilated
// views).  Tiles have the row pitch P = S | 1: an odd pitch puts the S rows a wave reads at one k (Lw[j][k], j = lane) on S
// different banks.  Every output is one fmaf chain over k = 0 .. S - 1 ascending: no atomics, no split reduction, so a plane's
// bits do not depend on the batch or the grid.  Internal linkage, like step_common.hpp.
#pragma once
#include "step_common.hpp"

namespace afldm {

namespace {

constexpr int PLANE_SMAX = 64;
constexpr int PLANE_THREADS = 256;

// global row-major [S][S] -> LDS tile of pitch P
__device__ __forceinline__ void plane_load_matrix(const float* __restrict__ L, float* tile, int S, int P, int tid) {
  for (int i = tid; i < S * S; i += PLANE_THREADS) {
    const int r = i / S;
    tile[r * P + (i - r * S)] = L[i];
  }
}

// out[i][j] = sum_k m[i][k] * v(j, k), v(j, k) = vt[j * vsj + k * vsk], k ascending.  Thread (g = tid / S, j = tid % S) owns column
// j of the rows g, g + G, g + 2 G, ... (G = 256 / S >= 4 row groups; the last 256 % S threads idle) and takes them R at a
// time: one read of v and R broadcast reads of m per R fmaf.  Each output is one chain whatever R is.
template <int R>
__device__ __forceinline__ void plane_pass_rows(const float* m, const float* vt, int vsj, int vsk, float* out, int S, int P, int tid) {
  const int G = PLANE_THREADS / S;
  const int g = tid / S, j = tid - g * S;
  if (g >= G) return;
  const float* vp = vt + j * vsj;
  for (int i0 = g; i0 < S; i0 += R * G) {
    int row[R];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = i0 + r * G;
      row[r] = (i < S ? i : S - 1) * P;          // (clamped: read in bounds, not stored)
      acc[r] = 0.0f;
    }
    for (int k = 0; k < S; ++k) {
      const float v = vp[k * vsk];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = fmaf(m[row[r] + k], v, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = i0 + r * G;
      if (i < S) out[i * P + j] = acc[r];
    }
  }
}

// R = the rows a thread owns, ceil(S / G), up to 4: one for S <= 16 (a thread per output), two for S <= 22, four from there on
__device__ __forceinline__ void plane_pass(const float* m, const float* vt, int vsj, int vsk, float* out, int S, int P, int tid) {
  const int G = PLANE_THREADS / S;
  const int rows = (S + G - 1) / G;
  if (rows <= 1)
    plane_pass_rows<1>(m, vt, vsj, vsk, out, S, P, tid);
  else if (rows == 2)
    plane_pass_rows<2>(m, vt, vsj, vsk, out, S, P, tid);
  else
    plane_pass_rows<4>(m, vt, vsj, vsk, out, S, P, tid);
}

}  // namespace

}  // namespace afldm
