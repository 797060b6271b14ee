// flow.hip — warping along an optical-flow field (reference afldm/shift_utils/flow_utils.py, flow_utils_np.py).
//
// afldm_flow_splat: the forward bilinear splat of `_forward_flow_warp` (flow_utils_np.py:116-152) for a whole batch of
//   frames: one thread per (sample, source pixel) forms the landing point in fp32 exactly as the reference does
//   (s * flow rounded, then added to the index; int() truncation; coef = (1 - |ci - gi|)(1 - |cj - gj|), which may be
//   negative above / left of the plane) and adds x * coef and coef to its four targets with return-less fp32 vector
//   atomics into a workspace the entry point zeroes.  A finishing kernel forms bwd_occ = !(cnt > 0), applies the
//   optional fill and writes the output dtype.  "pick" keeps only the targets on the ds grid (the reference's
//   [:, :, ::ds, ::ds] behind the warp), "pool" accumulates at full resolution and sums ds x ds blocks
//   (collect_noise_pixel, flow_utils.py:214-221).  Atomic sums depend on arrival order: two runs agree to fp32
//   summation-order error, not bit for bit.
// afldm_flow_warp: the backward sampler of `bilinear_sample` / `flow_warp` (flow_utils.py:53-86): grid_sample with
//   align_corners=True and zero padding, bilinear or nearest.
#include "common.hpp"

// The coordinates, coefficients and fill expressions below are the reference's fp32 operations one by one: a product fused
// into the following add (the compiler's default for HIP) moves a landing
// point by an ulp of the coordinate and a coefficient by ~1e-6.  No contraction anywhere in this file; the rounded operations
// are spelled as functions defined BELOW the pragma (the header's __fmul_rn / __fadd_rn bodies were compiled above it, keep their
// `contract` flag through inlining and fuse: seen as v_pk_fma_f32 on the landing point).
#pragma clang fp contract(off)

namespace afldm {

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }

// Targets of neighbouring sources are neighbours: with ds = 1 a wave's adds to one plane mostly fall into one or two
// rows of <= 256 contiguous bytes, the shape the memory-side atomic units take at full rate.
__device__ __forceinline__ void add_f32(float* p, float v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The workspace is zeroed by a kernel of this file: a captured call is kernel nodes only (zero -> splat -> finish).
__global__ void __launch_bounds__(256) k_flow_zero(float* ws, size_t n) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) ws[e] = 0.f;
}

// ws [B][C + 1][Hw][Ww] fp32 (plane C = cnt), Hw = H / ds in pick mode (ds > 1 keeps targets on the ds grid), H otherwise.
template <typename T>
__global__ void __launch_bounds__(256) k_flow_splat(const T* __restrict__ x, const float* __restrict__ flow,
                                                    const float* __restrict__ scale, float* ws, int group, int C, int H, int W,
                                                    int ds) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= H * W) return;
  const int b = blockIdx.y, bs = b / group;
  const int i = pix / W, j = pix - i * W;
  const size_t HW = (size_t)H * W;
  const float s = scale[b];
  const float* f = flow + (size_t)bs * 2 * HW;
  // the reference multiplies the flow by the fp32 alpha first, then adds the index: two roundings, no fma
  const float ci = add_rn((float)i, mul_rn(s, f[pix]));
  const float cj = add_rn((float)j, mul_rn(s, f[HW + pix]));
  // outside (-2, H) x (-2, W) none of the four targets is in the plane (and int() below stays in range); NaN ends here too
  if (!(ci > -2.f && ci < (float)H && cj > -2.f && cj < (float)W)) return;
  const int i1 = (int)ci, j1 = (int)cj;          // truncation towards zero, as Python's int()
  const int Hw = H / ds, Ww = W / ds;
  int tgt[4];
  float coef[4];
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                  // reference order: (i1, j1), (i2, j1), (i1, j2), (i2, j2)
    const int gi = i1 + (k & 1), gj = j1 + (k >> 1);
    const bool in = gi >= 0 && gi < H && gj >= 0 && gj < W && gi % ds == 0 && gj % ds == 0;
    tgt[k] = in ? (gi / ds) * Ww + gj / ds : -1;
    coef[k] = mul_rn(sub_rn(1.f, fabsf(sub_rn(ci, (float)gi))), sub_rn(1.f, fabsf(sub_rn(cj, (float)gj))));
    any |= in;
  }
  if (!any) return;
  const size_t plane = (size_t)Hw * Ww;
  float* w = ws + (size_t)b * (C + 1) * plane;
  const T* xs = x + (size_t)bs * C * HW + pix;
  for (int c = 0; c < C; ++c) {
    const float v = to_f32(xs[(size_t)c * HW]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (tgt[k] >= 0) add_f32(w + (size_t)c * plane + tgt[k], mul_rn(v, coef[k]));
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (tgt[k] >= 0) add_f32(w + (size_t)C * plane + tgt[k], coef[k]);
}

// res * (1 - occ) + occ * bg, each operation rounded as the reference's tensor expression (image_interpolation_pipeline.py:574)
__device__ __forceinline__ float fill_expr(float res, float occ, float bg) {
  return add_rn(mul_rn(res, sub_rn(1.f, occ)), mul_rn(occ, bg));
}

// pick mode: out / occ at the workspace's own resolution [B][C][Ho][Wo]; fill is read at pixel stride fps (a plane of
// (Ho fps) x (Wo fps)), sample stride fill_bstride elements (0: one draw shared by every sample)
template <typename T>
__global__ void __launch_bounds__(256) k_flow_finish_pick(const float* __restrict__ ws, const T* __restrict__ fill,
                                                          long long fill_bstride, int fps, T* __restrict__ out, T* __restrict__ occ,
                                                          int B, int C, int Ho, int Wo) {
  const size_t plane = (size_t)Ho * Wo, n = (size_t)B * C * plane;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const size_t p = e % plane, bc = e / plane;
    const int c = (int)(bc % C);
    const size_t b = bc / C;
    const float* w = ws + b * (C + 1) * plane;
    const float o = w[(size_t)C * plane + p] > 0.f ? 0.f : 1.f;
    float r = w[(size_t)c * plane + p];
    if (fill) {
      const size_t ho = p / Wo, wo = p % Wo;
      const size_t fi = (size_t)b * fill_bstride + (size_t)c * plane * fps * fps + ho * fps * ((size_t)Wo * fps) + wo * fps;
      r = fill_expr(r, o, to_f32(fill[fi]));
    }
    out[e] = from_f32<T>(r);
    if (occ && c == 0) occ[b * plane + p] = from_f32<T>(o);
  }
}

// pool mode: ws at full resolution [B][C + 1][H][W]; out [B][C][H / ds][W / ds] = sum over each ds x ds block of
// (fill * occ + res * (1 - occ)) / ds (collect_noise_pixel); occ (optional) [B][1][H][W]
template <typename T>
__global__ void __launch_bounds__(256) k_flow_finish_pool(const float* __restrict__ ws, const T* __restrict__ fill,
                                                          long long fill_bstride, T* __restrict__ out, T* __restrict__ occ, int B, int C,
                                                          int H, int W, int ds) {
  const int Ho = H / ds, Wo = W / ds;
  const size_t oplane = (size_t)Ho * Wo, plane = (size_t)H * W, n = (size_t)B * C * oplane;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const size_t p = e % oplane, bc = e / oplane;
    const int c = (int)(bc % C);
    const size_t b = bc / C;
    const size_t ho = p / Wo, wo = p % Wo;
    const float* w = ws + b * (C + 1) * plane;
    float acc = 0.f;
    for (int a = 0; a < ds; ++a) {
      const size_t row = (ho * ds + a) * W + wo * ds;
      for (int q = 0; q < ds; ++q) {
        const float o = w[(size_t)C * plane + row + q] > 0.f ? 0.f : 1.f;
        const float r = w[(size_t)c * plane + row + q];
        const float bg = fill ? to_f32(fill[(size_t)b * fill_bstride + (size_t)c * plane + row + q]) : 0.f;
        acc += add_rn(mul_rn(bg, o), mul_rn(r, sub_rn(1.f, o)));
        if (occ && c == 0) occ[b * plane + row + q] = from_f32<T>(o);
      }
    }
    out[e] = from_f32<T>(div_rn(acc, (float)ds));
  }
}

// Backward sampler.  One thread per (sample, output pixel), all channels.  add_grid: flow_warp's coords_grid + flip(flow)
// (flow channel 0 = row displacement: x = j + flow[1], y = i + flow[0]); otherwise `flow` holds bilinear_sample's coordinates
// (channel 0 = x).  The reference normalises to [-1, 1] by the OUTPUT extent and grid_sample un-normalises by the INPUT
// extent ((g + 1) / 2 * (size - 1)); the mask is formed from the normalised fp32 coordinate, as the reference's.
template <typename T>
__global__ void __launch_bounds__(256) k_flow_warp(const T* __restrict__ x, const float* __restrict__ flow, T* __restrict__ y,
                                                   unsigned char* __restrict__ mask, int C, int Hi, int Wi, int Ho, int Wo,
                                                   int add_grid, int nearest) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= Ho * Wo) return;
  const int b = blockIdx.y;
  const int i = pix / Wo, j = pix - i * Wo;
  const size_t oplane = (size_t)Ho * Wo, iplane = (size_t)Hi * Wi;
  const float* f = flow + (size_t)b * 2 * oplane;
  float sx, sy;
  if (add_grid) {
    sx = add_rn((float)j, f[oplane + pix]);
    sy = add_rn((float)i, f[pix]);
  } else {
    sx = f[pix];
    sy = f[oplane + pix];
  }
  const float gx = sub_rn(div_rn(mul_rn(2.f, sx), (float)(Wo - 1)), 1.f);
  const float gy = sub_rn(div_rn(mul_rn(2.f, sy), (float)(Ho - 1)), 1.f);
  if (mask) mask[(size_t)b * oplane + pix] = (gx >= -1.f && gy >= -1.f && gx <= 1.f && gy <= 1.f) ? 1 : 0;
  // same extent in and out: the normalise / un-normalise round trip is the identity up to rounding, so the pixel coordinate
  // itself is used (integer flows then copy bit for bit); another input extent goes through the normalised coordinate
  const float ix = (Wi == Wo) ? sx : mul_rn(div_rn(add_rn(gx, 1.f), 2.f), (float)(Wi - 1));
  const float iy = (Hi == Ho) ? sy : mul_rn(div_rn(add_rn(gy, 1.f), 2.f), (float)(Hi - 1));
  const T* xb = x + (size_t)b * C * iplane;
  T* yb = y + (size_t)b * C * oplane + pix;
  const bool near_plane = ix > -1.f && ix < (float)Wi && iy > -1.f && iy < (float)Hi;   // false for NaN
  if (!near_plane) {
    for (int c = 0; c < C; ++c) yb[(size_t)c * oplane] = from_f32<T>(0.f);
    return;
  }
  if (nearest) {
    const int xn = (int)rintf(ix), yn = (int)rintf(iy);            // round half to even, as std::nearbyint
    const bool in = xn >= 0 && xn < Wi && yn >= 0 && yn < Hi;
    for (int c = 0; c < C; ++c)
      yb[(size_t)c * oplane] = in ? xb[(size_t)c * iplane + (size_t)yn * Wi + xn] : from_f32<T>(0.f);
    return;
  }
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float wx1 = ix - fx0, wx0 = (fx0 + 1.f) - ix, wy1 = iy - fy0, wy0 = (fy0 + 1.f) - iy;
  const bool xin0 = x0 >= 0, xin1 = x0 + 1 < Wi, yin0 = y0 >= 0, yin1 = y0 + 1 < Hi;   // x0 >= -1 and x0 < Wi hold here
  const float w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
  for (int c = 0; c < C; ++c) {
    const T* xp = xb + (size_t)c * iplane;
    float acc = 0.f;
    if (yin0 && xin0) acc += to_f32(xp[(size_t)y0 * Wi + x0]) * w00;
    if (yin0 && xin1) acc += to_f32(xp[(size_t)y0 * Wi + x0 + 1]) * w01;
    if (yin1 && xin0) acc += to_f32(xp[(size_t)(y0 + 1) * Wi + x0]) * w10;
    if (yin1 && xin1) acc += to_f32(xp[(size_t)(y0 + 1) * Wi + x0 + 1]) * w11;
    yb[(size_t)c * oplane] = from_f32<T>(acc);
  }
}

static inline int flat_grid(size_t work) {
  size_t g = (work + 255) / 256;
  return (int)(g < 4096 ? (g ? g : 1) : 4096);
}

}  // namespace

}  // namespace afldm

using namespace afldm;

extern "C" size_t afldm_flow_splat_workspace(int B, int C, int H, int W, int ds, int mode) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || ds <= 0 || H % ds || W % ds || (mode != AFLDM_FLOW_PICK && mode != AFLDM_FLOW_POOL))
    return 0;
  const int k = mode == AFLDM_FLOW_PICK ? ds : 1;
  return (size_t)B * (C + 1) * (H / k) * (W / k) * sizeof(float);
}

extern "C" int afldm_flow_splat(const void* x, const float* flow, const float* scale, const void* fill, long long fill_batch_stride,
                                int fill_pix_stride, void* out, void* occ, float* workspace, size_t workspace_bytes, int B,
                                int Bs, int C, int H, int W, int ds, int mode, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && flow && scale && out && workspace, AFLDM_ENULL, "afldm_flow_splat: NULL pointer");
  AFLDM_REQUIRE(B > 0 && Bs > 0 && B % Bs == 0 && C > 0 && H > 0 && W > 0 && ds > 0 && H % ds == 0 && W % ds == 0, AFLDM_ESHAPE,
                "afldm_flow_splat: bad shape (B %d, Bs %d, C %d, H %d, W %d, ds %d): B must be a multiple of Bs, H and W of ds", B,
                Bs, C, H, W, ds);
  AFLDM_REQUIRE((size_t)H * W < (1u << 30), AFLDM_ESHAPE, "afldm_flow_splat: plane too large");
  AFLDM_REQUIRE(B <= 65535, AFLDM_ESHAPE, "afldm_flow_splat: B = %d exceeds 65535 samples per call (the grid's y extent)", B);
  AFLDM_REQUIRE(mode == AFLDM_FLOW_PICK || mode == AFLDM_FLOW_POOL, AFLDM_ESHAPE, "afldm_flow_splat: unknown mode %d", mode);
  AFLDM_REQUIRE(!fill || (fill_batch_stride >= 0 && (mode == AFLDM_FLOW_POOL || fill_pix_stride >= 1)), AFLDM_ESHAPE,
                "afldm_flow_splat: bad fill strides");
  const size_t need = afldm_flow_splat_workspace(B, C, H, W, ds, mode);
  AFLDM_REQUIRE(workspace_bytes >= need, AFLDM_ESHAPE, "afldm_flow_splat: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  AFLDM_REQUIRE(dtype == AFLDM_F32 || dtype == AFLDM_BF16, AFLDM_EDTYPE, "afldm_flow_splat: unknown dtype %d", dtype);
  hipStream_t st = (hipStream_t)stream;
  k_flow_zero<<<flat_grid(need / sizeof(float)), 256, 0, st>>>(workspace, need / sizeof(float));
  const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), (unsigned)B);
  const int group = B / Bs, kds = mode == AFLDM_FLOW_PICK ? ds : 1;
  const int Ho = H / ds, Wo = W / ds;
  const size_t nout = (size_t)B * C * Ho * Wo;
  if (dtype == AFLDM_F32) {
    k_flow_splat<float><<<grid, 256, 0, st>>>((const float*)x, flow, scale, workspace, group, C, H, W, kds);
    if (mode == AFLDM_FLOW_PICK)
      k_flow_finish_pick<float><<<flat_grid(nout), 256, 0, st>>>(workspace, (const float*)fill, fill_batch_stride, fill_pix_stride,
                                                                  (float*)out, (float*)occ, B, C, Ho, Wo);
    else
      k_flow_finish_pool<float><<<flat_grid(nout), 256, 0, st>>>(workspace, (const float*)fill, fill_batch_stride, (float*)out,
                                                                  (float*)occ, B, C, H, W, ds);
  } else {
    k_flow_splat<bf16><<<grid, 256, 0, st>>>((const bf16*)x, flow, scale, workspace, group, C, H, W, kds);
    if (mode == AFLDM_FLOW_PICK)
      k_flow_finish_pick<bf16><<<flat_grid(nout), 256, 0, st>>>(workspace, (const bf16*)fill, fill_batch_stride, fill_pix_stride,
                                                                 (bf16*)out, (bf16*)occ, B, C, Ho, Wo);
    else
      k_flow_finish_pool<bf16><<<flat_grid(nout), 256, 0, st>>>(workspace, (const bf16*)fill, fill_batch_stride, (bf16*)out,
                                                                 (bf16*)occ, B, C, H, W, ds);
  }
  return check_launch("afldm_flow_splat");
}

extern "C" int afldm_flow_warp(const void* x, const float* flow, void* y, unsigned char* mask, int B, int C, int Hin, int Win,
                               int Hout, int Wout, int add_grid, int nearest, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && flow && y, AFLDM_ENULL, "afldm_flow_warp: NULL pointer");
  AFLDM_REQUIRE(B > 0 && C > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, AFLDM_ESHAPE, "afldm_flow_warp: bad shape");
  AFLDM_REQUIRE((size_t)Hin * Win < (1u << 30) && (size_t)Hout * Wout < (1u << 30), AFLDM_ESHAPE, "afldm_flow_warp: plane too large");
  AFLDM_REQUIRE(B <= 65535, AFLDM_ESHAPE, "afldm_flow_warp: B = %d exceeds 65535 samples per call (the grid's y extent)", B);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(((size_t)Hout * Wout + 255) / 256), (unsigned)B);
  DISPATCH_T(dtype,
             (k_flow_warp<float><<<grid, 256, 0, st>>>((const float*)x, flow, (float*)y, mask, C, Hin, Win, Hout, Wout, add_grid, nearest)),
             (k_flow_warp<bf16><<<grid, 256, 0, st>>>((const bf16*)x, flow, (bf16*)y, mask, C, Hin, Win, Hout, Wout, add_grid, nearest)),
             "afldm_flow_warp");
  return check_launch("afldm_flow_warp");
}
