// slots.hip — the slot sampler's step bookkeeping: every batch row ("slot") of the captured step has a cursor of its own into
// one shared row table, so requests of different lengths share a batch and a finished slot waits, frozen, until the host
// refills it between replays.
//   state per slot b:  pos[b]  the row of the slot's last evaluation (begin - 1 before the first),  end[b]  one past its last row;
//                      the slot is active in a step iff pos[b] + 1 < end[b]
//   row table [R]:     row_coef[r] = (c0, c1, c2, c3) (the "ddim" row), row_t[r] the timestep, row_temb[r] the row of the
//                      time-embedding table [T, row_bytes] that holds that timestep's 27 time_emb_proj outputs
// afldm_slot_select   the step prologue: the ONLY place a cursor moves.  One workgroup per slot, so the thread that advances
//                     pos[b] is the one every other thread of that slot's copy hears the row from (LDS), and every block of the
//                     update below reads the advanced value - the hazard k_advance in misc.hip is a separate launch for.
// afldm_slot_step     the "ddim" update with the slot's own row, k_ddim_step's float operations in k_ddim_step's order; an
//                     inactive slot's elements are neither read nor written.
// afldm_slot_exchange between replays: harvest a finished slot's latents and / or refill it, as a device command buffer says.
// A block serves one slot (select: blockIdx.x, the other two: blockIdx.y): what it needs of the slot's state is uniform over the block.  HBM-bound; each
// thread reads and writes its own indices only.  Every table index read from device memory is range-checked before use.
// (slot_update, the "ddim" update both translation units of the slot sampler apply, is in slot_common.hpp; the update for a table
// of "ddim" AND "dpm" rows, afldm_slot_step_kinds, is slot_kinds.hip in libafldm_slots.so.)
#include "slot_common.hpp"

namespace afldm {

namespace {

constexpr int SELECT_THREADS = 256;      // chunks of 16 bytes per pass of a slot's row copy

}  // namespace

__global__ void __launch_bounds__(SELECT_THREADS) k_slot_select(const float* __restrict__ row_t, const int* __restrict__ row_temb,
                                                                int* pos, const int* __restrict__ end, float* t_out, int* active,
                                                                const uint4* __restrict__ table, uint4* rows_out, int R, int T,
                                                                int row_chunks) {
  __shared__ int s_src;                  // the time-embedding row to copy, or -1: the slot is frozen
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    const int p = pos[b] + 1;
    int src = -1;
    if (p >= 0 && p < end[b] && p < R) {
      const int ti = row_temb[p];
      if (ti >= 0 && ti < T) src = ti;
    }
    if (src >= 0) {
      pos[b] = p;
      t_out[b] = row_t[p];
    }
    active[b] = src >= 0;
    s_src = src;
  }
  __syncthreads();
  if (s_src < 0) return;
  const uint4* src = table + (size_t)s_src * row_chunks;
  uint4* dst = rows_out + (size_t)b * row_chunks;
  for (int i = threadIdx.x; i < row_chunks; i += SELECT_THREADS) dst[i] = src[i];
}

// x NCHW fp32 [B, C, HW], in place; eps NHWC T.  V = 4 needs HW % 4 == 0 and a 16-byte aligned x.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_slot_step(float* x, const T* __restrict__ eps, const float* __restrict__ row_coef,
                                                   const int* __restrict__ pos, const int* __restrict__ active, int R, int C,
                                                   int HW) {
  const int b = blockIdx.y;
  if (!active[b]) return;
  const int s = pos[b];
  if (s < 0 || s >= R) return;
  const float sa_t = row_coef[4 * s + 0], sb_t = row_coef[4 * s + 1], sa_p = row_coef[4 * s + 2], sb_p = row_coef[4 * s + 3];
  const int n = C * HW;                  // one slot
  float* xb = x + (size_t)b * n;
  const T* eb = eps + (size_t)b * n;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n / V; g += gridDim.x * blockDim.x) {
    const int i = g * V;
    const int pix = i % HW, ch = i / HW;
    const T* ep = eb + (size_t)pix * C + ch;
    vecf<V> xv = ld<V>(xb + i);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      xv.v[k] = slot_update(xv.v[k], to_f32(ep[(size_t)k * C]), sa_t, sb_t, sa_p, sb_p);
    }
    st<V>(xb + i, xv);
  }
}

// cmd[b] = {harvest, refill, begin, end}: out[harvest] <- lat[b] (harvest >= 0), then lat[b] <- fresh[refill] and the slot's
// counters (refill >= 0); the harvest and the refill of an element are the same thread's, in that order.
template <int V>
__global__ void __launch_bounds__(256) k_slot_exchange(const int* __restrict__ cmd, float* lat, float* out,
                                                       const float* __restrict__ fresh, int* pos, int* end, int n, int out_rows,
                                                       int fresh_rows) {
  const int b = blockIdx.y;
  const int harvest = cmd[4 * b + 0], refill = cmd[4 * b + 1];
  const bool h = harvest >= 0 && harvest < out_rows, r = refill >= 0 && refill < fresh_rows;
  if (!h && !r) return;
  float* xb = lat + (size_t)b * n;
  float* ob = out + (size_t)(h ? harvest : 0) * n;
  const float* fb = fresh + (size_t)(r ? refill : 0) * n;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n / V; g += gridDim.x * blockDim.x) {
    const int i = g * V;
    if (h) st<V>(ob + i, ld<V>(xb + i));
    if (r) st<V>(xb + i, ld<V>(fb + i));
  }
  if (r && blockIdx.x == 0 && threadIdx.x == 0) {
    pos[b] = cmd[4 * b + 2] - 1;
    end[b] = cmd[4 * b + 3];
  }
}

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_slot_select(const float* row_t, const int* row_temb, int* pos, const int* end, float* t_out, int* active,
                                 const void* temb_table, void* temb_rows, int B, int R, int T, size_t row_bytes,
                                 afldm_stream_t stream) {
  AFLDM_REQUIRE(row_t && row_temb && pos && end && t_out && active && temb_table && temb_rows, AFLDM_ENULL,
                "afldm_slot_select: NULL pointer");
  AFLDM_REQUIRE(B > 0 && R > 0 && T > 0, AFLDM_ESHAPE, "afldm_slot_select: bad shape");
  AFLDM_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0 && row_bytes / 16 <= 0x7fffffff && aligned16(temb_table) && aligned16(temb_rows),
                AFLDM_EALIGN, "afldm_slot_select: rows must be whole 16-byte chunks");
  k_slot_select<<<B, SELECT_THREADS, 0, (hipStream_t)stream>>>(row_t, row_temb, pos, end, t_out, active, (const uint4*)temb_table,
                                                               (uint4*)temb_rows, R, T, (int)(row_bytes / 16));
  return check_launch("afldm_slot_select");
}

extern "C" int afldm_slot_step(float* x, const void* eps, const float* row_coef, const int* pos, const int* active, int B, int R,
                               int C, int H, int W, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && eps && row_coef && pos && active, AFLDM_ENULL, "afldm_slot_step: NULL pointer");
  AFLDM_REQUIRE(B > 0 && B <= 65535 && R > 0 && C > 0 && H > 0 && W > 0 && (size_t)C * H * W <= SLOT_ELEMS_MAX, AFLDM_ESHAPE,
                "afldm_slot_step: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, n = C * HW;
  const bool v4 = HW % 4 == 0 && aligned16(x);
#define LAUNCH(T, V) \
  (k_slot_step<T, V><<<dim3(step_grid(n / V), B), 256, 0, st>>>(x, (const T*)eps, row_coef, pos, active, R, C, HW))
  STEP_DISPATCH(dtype, v4, LAUNCH, "afldm_slot_step");
#undef LAUNCH
  return check_launch("afldm_slot_step");
}

extern "C" int afldm_slot_exchange(const int* cmd, float* lat, float* out, const float* fresh, int* pos, int* end, int B,
                                   size_t slot_elems, int out_rows, int fresh_rows, afldm_stream_t stream) {
  AFLDM_REQUIRE(cmd && lat && out && fresh && pos && end, AFLDM_ENULL, "afldm_slot_exchange: NULL pointer");
  AFLDM_REQUIRE(B > 0 && B <= 65535 && slot_elems > 0 && slot_elems <= SLOT_ELEMS_MAX && out_rows > 0 && fresh_rows > 0, AFLDM_ESHAPE,
                "afldm_slot_exchange: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)slot_elems;
  if (n % 4 == 0 && aligned16(lat) && aligned16(out) && aligned16(fresh))
    k_slot_exchange<4><<<dim3(step_grid(n / 4), B), 256, 0, st>>>(cmd, lat, out, fresh, pos, end, n, out_rows, fresh_rows);
  else
    k_slot_exchange<1><<<dim3(step_grid(n), B), 256, 0, st>>>(cmd, lat, out, fresh, pos, end, n, out_rows, fresh_rows);
  return check_launch("afldm_slot_exchange");
}
