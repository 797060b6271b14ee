// cond.hip — class conditioning for classifier-free guidance on the graph-replayed engine.
//
// diffusers' UNet2DModel adds the class embedding to the time embedding BEFORE the SiLU in front of the resnets' time_emb_proj
// layers:  emb = time_embedding(t) + class_embedding(y);  temb = time_emb_proj(silu(emb)).  So a class-conditional step has no
// per-step row to copy (afldm_select_step_row): the projection depends on (step, row).  What still depends on the step only is
// time_embedding(t), tabulated per schedule BEFORE the SiLU; a step then runs
//
//   afldm_cond_embed:  act[r][j] = silu( rnd( emb_table[s][j] + class_rows[r][j] ) ),   s = *step_idx
//
// and the existing GEMM over all time_emb_proj layers on act.  The class rows are data: the captured graphs hold their address.
// An item is 8 consecutive elements of a row (one 16-byte chunk in bf16, two in fp32); one thread per item, rows x D / 8 items.
// The step counter is READ only: many workgroups read it, and the launch in front (afldm_select_timestep) is the one writer.
#include "common.hpp"

namespace afldm {

namespace {

template <typename T>
struct Item8;

template <>
struct Item8<float> {
  f32x4 lo, hi;
  static __device__ __forceinline__ Item8 load(const float* p) {
    return {*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + 4)};
  }
  __device__ __forceinline__ void store(float* p) const {
    *reinterpret_cast<f32x4*>(p) = lo;
    *reinterpret_cast<f32x4*>(p + 4) = hi;
  }
  __device__ __forceinline__ float get(int e) const { return e < 4 ? lo[e & 3] : hi[e & 3]; }
  __device__ __forceinline__ void set(int e, float v) {
    if (e < 4) lo[e & 3] = v;
    else hi[e & 3] = v;
  }
};

template <>
struct Item8<bf16> {
  bf16x8 v;
  static __device__ __forceinline__ Item8 load(const bf16* p) { return {ld16<bf16x8>(p)}; }
  __device__ __forceinline__ void store(bf16* p) const { st16<bf16x8>(p, v); }
  __device__ __forceinline__ float get(int e) const { return (float)v[e]; }
  __device__ __forceinline__ void set(int e, float f) { v[e] = (bf16)f; }
};

// emb: row 0 of the time embeddings (the table form: row s of it is taken, emb_stride = 0; the flat form: step_idx = nullptr and
// emb_stride = 0 for one broadcast row, D for a row per sample).  items = rows * D / 8.
template <typename T>
__global__ void __launch_bounds__(256) k_cond_embed(const T* __restrict__ emb, size_t emb_stride, int n, const int* __restrict__ step_idx,
                                                    const T* __restrict__ cls, T* __restrict__ act, int D, int items) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  if (step_idx) {
    const int s = *step_idx;
    if (s < 0 || s >= n) return;      // (uniform) a counter outside the table: nothing is read or written
    emb += (size_t)s * D;
  }
  const int cpr = D / 8;
  const int r = i / cpr, j = (i - r * cpr) * 8;
  const Item8<T> a = Item8<T>::load(emb + (size_t)r * emb_stride + j);
  const Item8<T> c = Item8<T>::load(cls + (size_t)r * D + j);
  Item8<T> o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float sum = to_f32(from_f32<T>(a.get(e) + c.get(e)));      // rnd: the one rounding of `emb + class_emb` in dtype
    o.set(e, silu_f(sum));                                           // rounded once on the way out, as k_silu does
  }
  o.store(act + (size_t)r * D + j);
}

int launch_cond_embed(const char* name, const void* emb, size_t emb_stride, int n, const int* step_idx, const void* cls, void* act,
                      int rows, int D, int dtype, hipStream_t st) {
  AFLDM_REQUIRE(rows > 0 && D > 0 && D % 8 == 0, AFLDM_ESHAPE, "%s: rows = %d, D = %d (D must be a positive multiple of 8)", name, rows, D);
  AFLDM_REQUIRE((long long)rows * (D / 8) <= 0x7fffffffLL, AFLDM_ESHAPE, "%s: rows * D / 8 exceeds the launch's index range", name);
  AFLDM_REQUIRE(emb && cls && act, AFLDM_ENULL, "%s: NULL pointer", name);
  AFLDM_REQUIRE(aligned16(emb) && aligned16(cls) && aligned16(act), AFLDM_EALIGN, "%s: emb, class_rows and act need 16-byte alignment", name);
  const int items = rows * (D / 8);
  const int grid = cdiv(items, 256);
  DISPATCH_T(dtype,
             (k_cond_embed<float><<<grid, 256, 0, st>>>((const float*)emb, emb_stride, n, step_idx, (const float*)cls, (float*)act, D, items)),
             (k_cond_embed<bf16><<<grid, 256, 0, st>>>((const bf16*)emb, emb_stride, n, step_idx, (const bf16*)cls, (bf16*)act, D, items)),
             name);
  return check_launch(name);
}

}  // namespace

}  // namespace afldm

using namespace afldm;

extern "C" int afldm_cond_embed(const void* emb_table, int n, const int* step_idx, const void* class_rows, void* act, int rows, int D,
                                int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(n > 0, AFLDM_ESHAPE, "afldm_cond_embed: a table of %d rows", n);
  AFLDM_REQUIRE(step_idx, AFLDM_ENULL, "afldm_cond_embed: NULL step_idx");
  return launch_cond_embed("afldm_cond_embed", emb_table, 0, n, step_idx, class_rows, act, rows, D, dtype, (hipStream_t)stream);
}

extern "C" int afldm_cond_embed_flat(const void* emb, int emb_rows, const void* class_rows, void* act, int rows, int D, int dtype,
                                     afldm_stream_t stream) {
  AFLDM_REQUIRE(emb_rows == 1 || emb_rows == rows, AFLDM_ESHAPE, "afldm_cond_embed_flat: %d embedding rows for %d rows (want 1 or %d)",
                emb_rows, rows, rows);
  return launch_cond_embed("afldm_cond_embed_flat", emb, emb_rows == 1 ? 0 : (size_t)D, 1, nullptr, class_rows, act, rows, D, dtype,
                           (hipStream_t)stream);
}
