// flowest.hip — the built-in optical-flow estimator: dense pyramidal Lucas-Kanade with Tikhonov damping and iterative
// warping.  It replaces nothing of the reference: the reference estimates flow with GMFlow, a trained
// network whose weights are not available; this is a classical, deterministic estimator the project defines itself, and
// its oracle (tests/flowest_oracle.py) is a float64 restatement of the arithmetic below.
//
// afldm_flowest_pyr_down: [1, 3, 3, 1] / 8 along each axis, decimated by 2 (factor 2), or the conversion to fp32 (factor 1).
// afldm_flowest_up2:      u <- 2 * bilinear_up2(u), half-pixel centres.
// afldm_flowest_lk_step:  one damped Lucas-Kanade update in one launch: warp, gradients, the five channel-summed products,
//                         their (2r+1)^2 window means, the closed 2 x 2 solve, the step clamp.
// afldm_flowest_smooth:   [1, 4, 6, 4, 1] / 16 along each axis.
// Every border is a replicate border (indices clamped into the plane), every sampling coordinate is clamped, there is no
// validity mask and no atomic: the result is a continuous function of the inputs and two runs agree bit for bit.
// Flows are [B][2][H][W] fp32 with channel 0 = ROW displacement, as in flow.hip.
#include "common.hpp"

// The oracle rounds every product and every add on its own, in a fixed order; a product fused into the following add would
// move a bilinear coordinate or a window sum by an ulp.  No contraction anywhere in this file (see flow.hip).
#pragma clang fp contract(off)

namespace afldm {

namespace {

constexpr int FE_RMAX = 4;          // largest window radius of afldm_flowest_lk_step (sizes its LDS)

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// sum_k w[k] v[k], left to right
__device__ __forceinline__ float taps4(float a, float b, float c, float d) {
  return ((a * 0.125f + b * 0.375f) + c * 0.375f) + d * 0.125f;
}
__device__ __forceinline__ float taps5(float a, float b, float c, float d, float e) {
  return (((a * 0.0625f + b * 0.25f) + c * 0.375f) + d * 0.25f) + e * 0.0625f;
}

// (1 - fy) ((1 - fx) v00 + fx v01) + fy ((1 - fx) v10 + fx v11) of plane p [h][w] at the clamped coordinate (sy, sx)
__device__ __forceinline__ float bilinear(const float* __restrict__ p, int h, int w, float sy, float sx) {
  const float y0f = floorf(sy), x0f = floorf(sx);
  const float fy = sy - y0f, fx = sx - x0f;
  // sy in [0, h - 1] here, so 0 <= y0 <= h - 1; the clamps below also keep a NaN coordinate inside the plane
  const int y0 = clampi((int)y0f, h - 1), x0 = clampi((int)x0f, w - 1);
  const int y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1, x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1;
  const float gx = 1.f - fx, gy = 1.f - fy;
  const float top = gx * p[(size_t)y0 * w + x0] + fx * p[(size_t)y0 * w + x1];
  const float bot = gx * p[(size_t)y1 * w + x0] + fx * p[(size_t)y1 * w + x1];
  return gy * top + fy * bot;
}

__device__ __forceinline__ float clampf(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }   // NaN -> 0

template <typename T>
__global__ void __launch_bounds__(256) k_flowest_convert(const T* __restrict__ x, float* __restrict__ y, size_t n) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) y[e] = to_f32(x[e]);
}

// one thread per output pixel: four horizontal sums, then the vertical one
template <typename T>
__global__ void __launch_bounds__(256) k_flowest_pyr_down(const T* __restrict__ x, float* __restrict__ y, int H, int W) {
  const int Ho = H / 2, Wo = W / 2;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= Ho * Wo) return;
  const int oy = pix / Wo, ox = pix - oy * Wo;
  const T* xp = x + (size_t)blockIdx.y * H * W;
  int cx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) cx[k] = clampi(2 * ox - 1 + k, W - 1);
  float h[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const T* row = xp + (size_t)clampi(2 * oy - 1 + k, H - 1) * W;
    h[k] = taps4(to_f32(row[cx[0]]), to_f32(row[cx[1]]), to_f32(row[cx[2]]), to_f32(row[cx[3]]));
  }
  y[(size_t)blockIdx.y * Ho * Wo + pix] = taps4(h[0], h[1], h[2], h[3]);
}

__global__ void __launch_bounds__(256) k_flowest_smooth(const float* __restrict__ u, float* __restrict__ y, int H, int W) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= H * W) return;
  const int py = pix / W, px = pix - py * W;
  const float* up = u + (size_t)blockIdx.y * H * W;
  int cx[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) cx[k] = clampi(px - 2 + k, W - 1);
  float h[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float* row = up + (size_t)clampi(py - 2 + k, H - 1) * W;
    h[k] = taps5(row[cx[0]], row[cx[1]], row[cx[2]], row[cx[3]], row[cx[4]]);
  }
  y[(size_t)blockIdx.y * H * W + pix] = taps5(h[0], h[1], h[2], h[3], h[4]);
}

// u [n][h][w] -> y [n][2h][2w]
__global__ void __launch_bounds__(256) k_flowest_up2(const float* __restrict__ u, float* __restrict__ y, int h, int w) {
  const int H = 2 * h, W = 2 * w;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= H * W) return;
  const int py = pix / W, px = pix - py * W;
  const float sy = clampf(((float)py + 0.5f) / 2.f - 0.5f, (float)(h - 1));
  const float sx = clampf(((float)px + 0.5f) / 2.f - 0.5f, (float)(w - 1));
  y[(size_t)blockIdx.y * H * W + pix] = bilinear(u + (size_t)blockIdx.y * h * w, h, w, sy, sx) * 2.f;
}

// One workgroup per T x T output tile of one sample.  With r the window radius, E = T + 2r the product extent and
// S = E + 2 the staged extent:
//   per channel: I1 and I2w at the S x S positions (tile + halo r + 1, clamped into the plane) -> LDS; then the five
//     products at the E x E positions (tile + halo r), added onto the LDS product planes.  A position outside the plane
//     takes the product of its clamped position (the replicate padding of the product plane), whose own neighbours are
//     clamped again (the replicate padding of the image planes): both are in-plane positions inside the staged block.
//   row sums in place: a thread owns one (plane, row) and walks it left to right (column x reads x .. x + 2r);
//   column sums, the solve and the store: a thread owns output pixels.
// LDS: 2 S^2 + 5 E (E + 1) floats; T = 32, r = 4: 46 KB.
template <int T>
__global__ void __launch_bounds__(256) k_flowest_lk_step(const float* __restrict__ I1, const float* __restrict__ I2,
                                                         const float* __restrict__ uin, float* __restrict__ uout, int C, int H,
                                                         int W, int r, float lam) {
  constexpr int SMAX = T + 2 * FE_RMAX + 2, EMAX = T + 2 * FE_RMAX;
  __shared__ float s_i1[SMAX * SMAX];
  __shared__ float s_iw[SMAX * SMAX];
  __shared__ float s_p[5 * EMAX * (EMAX + 1)];
  const int E = T + 2 * r, S = E + 2, EP = E + 1;          // EP: odd row pitch of the product planes
  const int tid = threadIdx.x, b = blockIdx.z;
  const int ty0 = blockIdx.y * T, tx0 = blockIdx.x * T;
  const size_t HW = (size_t)H * W;
  const float* u0 = uin + (size_t)b * 2 * HW;
  const float* u1 = u0 + HW;
  const int plane = E * EP;

  for (int c = 0; c < C; ++c) {
    const float* p1 = I1 + ((size_t)b * C + c) * HW;
    const float* p2 = I2 + ((size_t)b * C + c) * HW;
    if (c) __syncthreads();                                 // the products of channel c - 1 have read the staged block
    for (int e = tid; e < S * S; e += 256) {
      const int ly = e / S, lx = e - ly * S;
      const int gy = clampi(ty0 - r - 1 + ly, H - 1), gx = clampi(tx0 - r - 1 + lx, W - 1);
      const size_t g = (size_t)gy * W + gx;
      s_i1[e] = p1[g];
      s_iw[e] = bilinear(p2, H, W, clampf((float)gy + u0[g], (float)(H - 1)), clampf((float)gx + u1[g], (float)(W - 1)));
    }
    __syncthreads();
    for (int e = tid; e < E * E; e += 256) {
      const int py = e / E, px = e - py * E;
      // the clamped plane position of this product, and of its four neighbours, in staged coordinates
      const int qy = clampi(ty0 - r + py, H - 1), qx = clampi(tx0 - r + px, W - 1);
      const int oy = r + 1 - ty0, ox = r + 1 - tx0;
      const int ly = qy + oy, lx = qx + ox;
      const int lyp = clampi(qy + 1, H - 1) + oy, lym = clampi(qy - 1, H - 1) + oy;
      const int lxp = clampi(qx + 1, W - 1) + ox, lxm = clampi(qx - 1, W - 1) + ox;
      const float d1y = (s_i1[lyp * S + lx] - s_i1[lym * S + lx]) * 0.5f;
      const float d1x = (s_i1[ly * S + lxp] - s_i1[ly * S + lxm]) * 0.5f;
      const float d2y = (s_iw[lyp * S + lx] - s_iw[lym * S + lx]) * 0.5f;
      const float d2x = (s_iw[ly * S + lxp] - s_iw[ly * S + lxm]) * 0.5f;
      const float gy = (d1y + d2y) * 0.5f, gx = (d1x + d2x) * 0.5f;
      const float it = s_iw[ly * S + lx] - s_i1[ly * S + lx];
      float* pp = s_p + py * EP + px;
      const float v0 = gy * gy, v1 = gy * gx, v2 = gx * gx, v3 = gy * it, v4 = gx * it;
      if (c == 0) {
        pp[0] = v0; pp[plane] = v1; pp[2 * plane] = v2; pp[3 * plane] = v3; pp[4 * plane] = v4;
      } else {                                              // the same thread owns the element for every channel
        pp[0] += v0; pp[plane] += v1; pp[2 * plane] += v2; pp[3 * plane] += v3; pp[4 * plane] += v4;
      }
    }
  }
  __syncthreads();
  // row sums, in place: output column x of a row reads columns x .. x + 2r (left to right) and lands in column x
  for (int row = tid; row < 5 * E; row += 256) {
    float* pr = s_p + (row / E) * plane + (row % E) * EP;
    for (int x = 0; x < T; ++x) {
      float acc = pr[x];
      for (int d = 1; d <= 2 * r; ++d) acc = acc + pr[x + d];
      pr[x] = acc;
    }
  }
  __syncthreads();
  const float n = (float)((2 * r + 1) * (2 * r + 1));
  for (int e = tid; e < T * T; e += 256) {
    const int y = e / T, x = e - y * T;
    const int gy = ty0 + y, gx = tx0 + x;
    if (gy >= H || gx >= W) continue;                       // an overhanging tile masks its stores
    float m[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float* pc = s_p + k * plane + y * EP + x;
      float acc = pc[0];
      for (int d = 1; d <= 2 * r; ++d) acc = acc + pc[d * EP];
      m[k] = acc / n;
    }
    const float a = m[0] + lam, bb = m[1], cc = m[2] + lam, p = m[3], q = m[4];
    const float det = a * cc - bb * bb;
    const float du0 = -((cc * p - bb * q) / det);
    const float du1 = -((a * q - bb * p) / det);
    const float s = fminf(1.f / sqrtf(du0 * du0 + du1 * du1), 1.f);     // 1 / 0 = inf -> 1
    const size_t g = (size_t)gy * W + gx;
    uout[(size_t)b * 2 * HW + g] = u0[g] + du0 * s;
    uout[(size_t)b * 2 * HW + HW + g] = u1[g] + du1 * s;
  }
}

}  // namespace

}  // namespace afldm

using namespace afldm;

static int flowest_plane_ok(const char* what, int n, int H, int W) {
  AFLDM_REQUIRE(n > 0 && H > 0 && W > 0, AFLDM_ESHAPE, "%s: bad shape (n %d, H %d, W %d)", what, n, H, W);
  AFLDM_REQUIRE((size_t)H * W < (1u << 28), AFLDM_ESHAPE, "%s: plane too large", what);
  AFLDM_REQUIRE(n <= 65535, AFLDM_ESHAPE, "%s: n = %d exceeds 65535 planes per call (the grid's y extent)", what, n);
  return AFLDM_OK;
}

extern "C" int afldm_flowest_pyr_down(const void* x, float* y, int n, int H, int W, int factor, int dtype, afldm_stream_t stream) {
  AFLDM_REQUIRE(x && y, AFLDM_ENULL, "afldm_flowest_pyr_down: NULL pointer");
  if (int rc = flowest_plane_ok("afldm_flowest_pyr_down", n, H, W)) return rc;
  AFLDM_REQUIRE(factor == 1 || (factor == 2 && H % 2 == 0 && W % 2 == 0), AFLDM_ESHAPE,
                "afldm_flowest_pyr_down: factor must be 1 (convert) or 2 with even H and W, got factor %d, H %d, W %d", factor, H, W);
  hipStream_t st = (hipStream_t)stream;
  if (factor == 1) {
    const size_t total = (size_t)n * H * W;
    const size_t g = (total + 255) / 256;
    const int grid = (int)(g < 4096 ? g : 4096);
    DISPATCH_T(dtype, (k_flowest_convert<float><<<grid, 256, 0, st>>>((const float*)x, y, total)),
               (k_flowest_convert<bf16><<<grid, 256, 0, st>>>((const bf16*)x, y, total)), "afldm_flowest_pyr_down");
  } else {
    const dim3 grid((unsigned)(((size_t)(H / 2) * (W / 2) + 255) / 256), (unsigned)n);
    DISPATCH_T(dtype, (k_flowest_pyr_down<float><<<grid, 256, 0, st>>>((const float*)x, y, H, W)),
               (k_flowest_pyr_down<bf16><<<grid, 256, 0, st>>>((const bf16*)x, y, H, W)), "afldm_flowest_pyr_down");
  }
  return check_launch("afldm_flowest_pyr_down");
}

extern "C" int afldm_flowest_smooth(const float* u, float* y, int n, int H, int W, afldm_stream_t stream) {
  AFLDM_REQUIRE(u && y && u != y, AFLDM_ENULL, "afldm_flowest_smooth: NULL pointer, or u == y (not an in-place pass)");
  if (int rc = flowest_plane_ok("afldm_flowest_smooth", n, H, W)) return rc;
  const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), (unsigned)n);
  k_flowest_smooth<<<grid, 256, 0, (hipStream_t)stream>>>(u, y, H, W);
  return check_launch("afldm_flowest_smooth");
}

extern "C" int afldm_flowest_up2(const float* u, float* y, int n, int h, int w, afldm_stream_t stream) {
  AFLDM_REQUIRE(u && y && u != y, AFLDM_ENULL, "afldm_flowest_up2: NULL pointer, or u == y");
  if (int rc = flowest_plane_ok("afldm_flowest_up2", n, 2 * h, 2 * w)) return rc;
  AFLDM_REQUIRE(h > 0 && w > 0, AFLDM_ESHAPE, "afldm_flowest_up2: bad shape");
  const dim3 grid((unsigned)(((size_t)4 * h * w + 255) / 256), (unsigned)n);
  k_flowest_up2<<<grid, 256, 0, (hipStream_t)stream>>>(u, y, h, w);
  return check_launch("afldm_flowest_up2");
}

extern "C" int afldm_flowest_lk_step(const float* I1, const float* I2, const float* u_in, float* u_out, int B, int C, int H, int W,
                                     int radius, float lam, int tile, afldm_stream_t stream) {
  AFLDM_REQUIRE(I1 && I2 && u_in && u_out && u_in != u_out, AFLDM_ENULL,
                "afldm_flowest_lk_step: NULL pointer, or u_in == u_out (every tile reads its neighbours' u_in)");
  if (int rc = flowest_plane_ok("afldm_flowest_lk_step", B, H, W)) return rc;
  AFLDM_REQUIRE(C >= 1 && C <= 4, AFLDM_ESHAPE, "afldm_flowest_lk_step: C = %d, 1 to 4 channels are supported", C);
  AFLDM_REQUIRE(radius >= 1 && radius <= FE_RMAX, AFLDM_ESHAPE, "afldm_flowest_lk_step: radius = %d, 1 to %d are supported", radius,
                FE_RMAX);
  AFLDM_REQUIRE(lam > 0.f, AFLDM_ESHAPE, "afldm_flowest_lk_step: lam must be positive (it keeps the 2 x 2 system regular)");
  AFLDM_REQUIRE(tile == 0 || tile == 16 || tile == 32, AFLDM_ESHAPE, "afldm_flowest_lk_step: tile must be 0 (chosen here), 16 or 32");
  if (tile == 0)      // 32 x 32 tiles recompute less halo; 16 x 16 tiles fill the chip when the plane gives few workgroups
    tile = (long long)cdiv(H, 32) * cdiv(W, 32) * B >= 512 ? 32 : 16;
  AFLDM_REQUIRE(cdiv(H, tile) <= 65535, AFLDM_ESHAPE, "afldm_flowest_lk_step: plane too tall");
  const dim3 grid((unsigned)cdiv(W, tile), (unsigned)cdiv(H, tile), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (tile == 32)
    k_flowest_lk_step<32><<<grid, 256, 0, st>>>(I1, I2, u_in, u_out, C, H, W, radius, lam);
  else
    k_flowest_lk_step<16><<<grid, 256, 0, st>>>(I1, I2, u_in, u_out, C, H, W, radius, lam);
  return check_launch("afldm_flowest_lk_step");
}
