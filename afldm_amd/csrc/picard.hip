// picard.hip — parallel-in-time sampling (ParaDiGMS: Shih et al., NeurIPS 2023): a window of Wn consecutive "ddim" rows of an
// image is evaluated as ONE UNet batch and iterated to its fixed point (Picard iteration on the sampler's recurrence).
//   state per image p:  base[p]  the row of the schedule X[0] stands at (0 .. n; n = finished),  iter[p]  iterations seen
//   states   x [Wn + 1][P][C][HW] fp32: X[j] estimates x_{base + j}; X[0] is exact.  State-major, so rows 0 .. Wn - 1 are the
//            contiguous NCHW batch [Wn P] the UNet evaluates (UNet row j P + p).
//   row table [n]:  row_coef[r] = (c0, c1, c2, c3), row_t[r] the timestep, row_temb[r] the row of the time-embedding table
//            [T, row_bytes] - the slot sampler's layout (slots.hip).
// One iteration behind the UNet is three launches:
//   afldm_picard_sweep   Y[0] = X[0]; Y[j + 1] = U_{base + j}(Y[j], e_j) for the rows that exist (base + j < n), a copy for
//                        the others; per (image, row, block) one partial sum of (Y[j] - X[j])^2.  Reads base, writes none.
//   afldm_picard_stride  ONE workgroup per image: adds the partials in ascending block order, decides the stride s, and is the
//                        ONLY place base[p] moves.  The thread that moves it tells the rest of its workgroup through LDS, and
//                        no other workgroup of the launch reads base[p] - the hazard k_advance in misc.hip is a separate
//                        launch for.  Then the per-row gather for the next evaluation (timestep, activity flag,
//                        time-embedding row), as afldm_slot_select gathers.
//   afldm_picard_slide   X[j] = Y[min(j + s, Wn)] with the s the launch before left in stride[p]; does not read base.
// A finished image (base == n) is skipped by all three: nothing of it is read or written but its iteration counter.  Every
// index read from device memory is range-checked before use.  HBM-bound; no atomics; an image's arithmetic depends neither on P
// nor on p.
#include "step_common.hpp"

namespace afldm {

namespace {

constexpr int PICARD_THREADS = 256;
constexpr int PICARD_WAVES = PICARD_THREADS / 64;
constexpr int PICARD_WINDOW_MAX = 256;      // rows of a window: the sweep keeps one partial per row and wave in LDS
constexpr int PICARD_BLOCKS_MAX = 2048;     // blocks of a sweep per image (no grid stride: a thread owns ONE group of V elements)
constexpr int STRIDE_THREADS = 1024;        // chunks of 16 bytes per pass of the gather (x 4 in flight per thread)

// k_ddim_step's update, operation for operation, as slot_update in slot_common.hpp spells it: x - c1 e is ONE fma, the division is
// correctly rounded, the last line two rounded products and a sum; contraction off, so that a swept row has afldm_ddim_step's bits.
__device__ __forceinline__ float picard_update(float x, float e, float sa_t, float sb_t, float sa_p, float sb_p) {
#pragma clang fp contract(off)
  const float x0 = __builtin_fmaf(-sb_t, e, x) / sa_t;
  const float a = sa_p * x0, b = sb_p * e;
  return a + b;
}

// elements per thread of the sweep and the slide: the 16-byte form wherever a plane is whole groups of four
inline int picard_vec(int H, int W) { return (H * W) % 4 == 0 ? 4 : 1; }

inline int picard_blocks(size_t elems, int V) { return (int)((elems / V + PICARD_THREADS - 1) / PICARD_THREADS); }

}  // namespace

// x [Wn + 1][P][n_el] NCHW fp32, y [Wn][P][n_el] (y row j holds Y[j + 1]), eps [Wn P] NHWC T, partial [P][Wn][gridDim.x].
// A thread owns V consecutive elements and carries them down the window in registers.  Reduction: the thread's V squares
// in element order, a butterfly over the wave, the waves' sums as (w0 + w1) + (w2 + w3).
template <typename T, int V>
__global__ void __launch_bounds__(PICARD_THREADS) k_picard_sweep(const float* __restrict__ x, const T* __restrict__ eps,
                                                                 float* __restrict__ y, float* __restrict__ partial,
                                                                 const float* __restrict__ row_coef, const int* __restrict__ base,
                                                                 int P, int Wn, int n, int C, int HW) {
  __shared__ float s_part[PICARD_WINDOW_MAX][PICARD_WAVES];
  const int p = blockIdx.y;
  const int b0 = base[p];
  if (b0 < 0 || b0 >= n) return;                                     // finished (or not a cursor): not read, not written
  const int n_el = C * HW;
  const size_t row = (size_t)P * n_el;                               // one state of every image
  const int i = (blockIdx.x * PICARD_THREADS + threadIdx.x) * V;
  const bool live = i < n_el;
  const int pix = live ? i % HW : 0, ch = live ? i / HW : 0;
  const size_t at = (size_t)p * n_el + (live ? i : 0);
  vecf<V> run;
#pragma unroll
  for (int k = 0; k < V; ++k) run.v[k] = 0.0f;
  if (live) run = ld<V>(x + at);                                     // Y[0] = X[0]
  for (int j = 0; j < Wn; ++j) {
    const int r = b0 + j;
    float sq = 0.0f;
    if (live) {
      if (r < n) {
        const float sa_t = row_coef[4 * r + 0], sb_t = row_coef[4 * r + 1], sa_p = row_coef[4 * r + 2], sb_p = row_coef[4 * r + 3];
        const T* ep = eps + ((size_t)(j * P + p) * HW + pix) * C + ch;
#pragma unroll
        for (int k = 0; k < V; ++k) run.v[k] = picard_update(run.v[k], to_f32(ep[(size_t)k * C]), sa_t, sb_t, sa_p, sb_p);
        const vecf<V> old = ld<V>(x + (size_t)(j + 1) * row + at);
#pragma unroll
        for (int k = 0; k < V; ++k) {
#pragma clang fp contract(off)
          const float d = run.v[k] - old.v[k];
          const float d2 = d * d;
          sq = sq + d2;
        }
      }
      st<V>(y + (size_t)j * row + at, run);                          // an inactive row: the copy of its predecessor, err 0
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if ((threadIdx.x & 63) == 0) s_part[j][threadIdx.x >> 6] = sq;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < Wn; j += PICARD_THREADS) {
    const float lo = s_part[j][0] + s_part[j][1], hi = s_part[j][2] + s_part[j][3];
    partial[((size_t)p * Wn + j) * gridDim.x + blockIdx.x] = lo + hi;
  }
}

// cur = {base [P], iter [P]}.  err [P][Wn], log [log_cap][P]: the stride of every iteration, for the host's statistics.
// gather_only: no decision, no advance (s = 0) - the gather for the cursors as they stand, before the first evaluation of a run.
__global__ void __launch_bounds__(STRIDE_THREADS) k_picard_stride(const float* __restrict__ partial, int* base, int* iter,
                                                                  int* stride, float* err, int* log, int log_cap,
                                                                  const float* __restrict__ row_t, const int* __restrict__ row_temb,
                                                                  float* t_out, int* active, const uint4* __restrict__ table,
                                                                  uint4* rows_out, float tol2, int gather_only, int P, int Wn, int n,
                                                                  int nblk, int n_el, int T, int row_chunks) {
  __shared__ float s_err[PICARD_WINDOW_MAX];
  __shared__ int s_base, s_go;
  const int p = blockIdx.x;
  const int b0 = base[p];                                            // every thread reads it BEFORE the barrier thread 0 writes behind
  const bool running = b0 >= 0 && b0 < n;
  if (!gather_only && running) {
    for (int j = threadIdx.x; j < Wn; j += STRIDE_THREADS) {
      float sum = 0.0f;
      if (b0 + j < n) {
        const float* pp = partial + ((size_t)p * Wn + j) * nblk;
        for (int k = 0; k < nblk; ++k) sum += pp[k];                 // ascending block order
      }
      const float e = sum / (float)n_el;
      s_err[j] = e;
      err[(size_t)p * Wn + j] = e;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    if (!gather_only && running) {
      s = Wn;
      for (int j = 0; j < Wn; ++j) {
        if (s_err[j] > tol2) {                                       // err_{j + 1}: Y[j + 1] against X[j + 1]
          s = j + 1;
          break;
        }
      }
      if (s > n - b0) s = n - b0;
      base[p] = b0 + s;                                              // the ONLY place a cursor moves
    }
    if (!gather_only) {
      const int it = iter[p];
      if (it >= 0 && it < log_cap) log[(size_t)it * P + p] = s;
      iter[p] = it + 1;
      stride[p] = s;
    }
    s_base = b0 + s;
    s_go = gather_only ? (b0 >= 0 && b0 <= n) : s > 0;
  }
  __syncthreads();
  if (!s_go) return;                                                 // a finished image keeps its timesteps and its rows
  const int b1 = s_base;
  for (int j = 0; j < Wn; ++j) {
    const int r = b1 + j;
    int src = -1;
    if (r >= 0 && r < n) {
      const int ti = row_temb[r];
      if (ti >= 0 && ti < T) src = ti;
    }
    const int u = j * P + p;                                         // the UNet's batch row
    if (threadIdx.x == 0) {
      active[u] = src >= 0;
      if (src >= 0) t_out[u] = row_t[r];
    }
    if (src < 0) continue;                                           // past the end: evaluated with what it last held, finite
    const uint4* from = table + (size_t)src * row_chunks;
    uint4* to = rows_out + (size_t)u * row_chunks;
    int c = threadIdx.x;
    for (; c + 3 * STRIDE_THREADS < row_chunks; c += 4 * STRIDE_THREADS) {
      const uint4 a0 = from[c], a1 = from[c + STRIDE_THREADS], a2 = from[c + 2 * STRIDE_THREADS], a3 = from[c + 3 * STRIDE_THREADS];
      to[c] = a0; to[c + STRIDE_THREADS] = a1; to[c + 2 * STRIDE_THREADS] = a2; to[c + 3 * STRIDE_THREADS] = a3;
    }
    for (; c < row_chunks; c += STRIDE_THREADS) to[c] = from[c];
  }
}

// X[j] = Y[min(j + s, Wn)], j = 0 .. Wn; y row k holds Y[k + 1] and s >= 1, so Y[0] is never asked for.
template <int V>
__global__ void __launch_bounds__(PICARD_THREADS) k_picard_slide(float* __restrict__ x, const float* __restrict__ y,
                                                                 const int* __restrict__ stride, int P, int Wn, int n_el) {
  const int p = blockIdx.y;
  const int s = stride[p];
  if (s < 1 || s > Wn) return;
  const int i = (blockIdx.x * PICARD_THREADS + threadIdx.x) * V;
  if (i >= n_el) return;
  const size_t row = (size_t)P * n_el, at = (size_t)p * n_el + i;
  for (int j = 0; j <= Wn; ++j) {
    const int k = (j + s < Wn ? j + s : Wn) - 1;
    st<V>(x + (size_t)j * row + at, ld<V>(y + (size_t)k * row + at));
  }
}

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_picard_blocks(int C, int H, int W) {
  if (C <= 0 || H <= 0 || W <= 0) return 0;
  return picard_blocks((size_t)C * H * W, picard_vec(H, W));
}

extern "C" int afldm_picard_sweep(const float* x, const void* eps, float* y, float* partial, const float* row_coef, const int* base,
                                  int P, int Wn, int n, int C, int H, int W, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && y && partial && row_coef && base, AFLDM_ENULL, "afldm_picard_sweep: NULL pointer");
  AFLDM_REQUIRE(P > 0 && P <= 65535 && Wn > 0 && Wn <= PICARD_WINDOW_MAX && n > 0 && C > 0 && H > 0 && W > 0 &&
                    (size_t)C * H * W <= (size_t)PICARD_BLOCKS_MAX * PICARD_THREADS,
                AFLDM_ESHAPE, "afldm_picard_sweep: bad shape");
  const int HW = H * W, V = picard_vec(H, W);
  AFLDM_REQUIRE(V == 1 || (aligned16(x) && aligned16(y)), AFLDM_EALIGN,
                "afldm_picard_sweep: states of whole 16-byte groups (H W % 4 == 0) must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(picard_blocks((size_t)C * HW, V), P);
#define LAUNCH(T, V) \
  (k_picard_sweep<T, V><<<grid, PICARD_THREADS, 0, st>>>(x, (const T*)eps, y, partial, row_coef, base, P, Wn, n, C, HW))
  STEP_DISPATCH(dtype, V == 4, LAUNCH, "afldm_picard_sweep");
#undef LAUNCH
  return check_launch("afldm_picard_sweep");
}

extern "C" int afldm_picard_stride(const float* partial, int* base, int* iter, int* stride, float* err, int* log, int log_cap,
                                   const float* row_t, const int* row_temb, float* t_out, int* active, const void* temb_table,
                                   void* temb_rows, float tol2, int gather_only, int P, int Wn, int n, int C, int H, int W, int T,
                                   size_t row_bytes, afldm_stream_t stream) {
  AFLDM_REQUIRE(partial && base && iter && stride && err && log && row_t && row_temb && t_out && active && temb_table && temb_rows,
                AFLDM_ENULL, "afldm_picard_stride: NULL pointer");
  AFLDM_REQUIRE(P > 0 && P <= 65535 && Wn > 0 && Wn <= PICARD_WINDOW_MAX && n > 0 && T > 0 && log_cap >= 0 && C > 0 && H > 0 && W > 0 &&
                    (size_t)C * H * W <= (size_t)PICARD_BLOCKS_MAX * PICARD_THREADS && tol2 >= 0.0f,
                AFLDM_ESHAPE, "afldm_picard_stride: bad shape");
  AFLDM_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0 && row_bytes / 16 <= 0x7fffffff && aligned16(temb_table) && aligned16(temb_rows),
                AFLDM_EALIGN, "afldm_picard_stride: rows must be whole 16-byte chunks");
  const int n_el = C * H * W;
  k_picard_stride<<<P, STRIDE_THREADS, 0, (hipStream_t)stream>>>(partial, base, iter, stride, err, log, log_cap, row_t, row_temb, t_out,
                                                                 active, (const uint4*)temb_table, (uint4*)temb_rows, tol2,
                                                                 gather_only, P, Wn, n, picard_blocks((size_t)n_el, picard_vec(H, W)),
                                                                 n_el, T, (int)(row_bytes / 16));
  return check_launch("afldm_picard_stride");
}

extern "C" int afldm_picard_slide(float* x, const float* y, const int* stride, int P, int Wn, int C, int H, int W,
                                  afldm_stream_t stream) {
  AFLDM_REQUIRE(x && y && stride, AFLDM_ENULL, "afldm_picard_slide: NULL pointer");
  AFLDM_REQUIRE(P > 0 && P <= 65535 && Wn > 0 && Wn <= PICARD_WINDOW_MAX && C > 0 && H > 0 && W > 0 &&
                    (size_t)C * H * W <= (size_t)PICARD_BLOCKS_MAX * PICARD_THREADS,
                AFLDM_ESHAPE, "afldm_picard_slide: bad shape");
  const int n_el = C * H * W, V = picard_vec(H, W);
  AFLDM_REQUIRE(V == 1 || (aligned16(x) && aligned16(y)), AFLDM_EALIGN,
                "afldm_picard_slide: states of whole 16-byte groups (H W % 4 == 0) must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(picard_blocks((size_t)n_el, V), P);
  if (V == 4)
    k_picard_slide<4><<<grid, PICARD_THREADS, 0, st>>>(x, y, stride, P, Wn, n_el);
  else
    k_picard_slide<1><<<grid, PICARD_THREADS, 0, st>>>(x, y, stride, P, Wn, n_el);
  return check_launch("afldm_picard_slide");
}
