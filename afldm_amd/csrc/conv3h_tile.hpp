// conv3h_tile.hpp - the halo-patch 3x3 convolution tile (see conv3h.hip for the design notes): the
// swizzled LDS image helpers and the tile body shared by k_conv3h (conv3h.hip) and the merged launches (actconv.hip).
#pragma once
#include "conv_common.hpp"

#include <type_traits>

namespace afldm {

// The consumers run v_mfma_f32_16x16x32_bf16 / 4 x 16x16x4_f32 (Mma<T>, common.hpp): lane (i = l & 15, g = l >> 4) feeds chunk
// kc * 4 + g of row i; accumulator = 4 consecutive couts of one pixel.  (The 32x32x16 flavour was measured and removed:
// DESIGN.md.)  The weight ring is three stages deep.
constexpr int kH3MF = 16, kH3Stages = 3;

// LDS position of chunk c of row q and its inverse (see conv3h.hip): bit 2 is kept for the lane-group parity, two bits are
// swizzled.  The row's swizzle bits sw: (q >> 1) & 3 of the row index for the weight rows and for patches of planes 16+ wide,
// where 16 consecutive tile pixels are 16 consecutive patch pixels.  On the 8x8 / 4x4 planes a fragment's 16 pixels span 2 / 4
// image rows (patch rows are W + 2 pixels apart) and that rule put two of every 8 equal-lane-group rows on the same banks -
// every patch read of those variants took two LDS cycles.  There the bits come from the patch COORDINATES (pr, pc): column
// pair (pc >> 1) & 3 on 8-wide planes (the 8 pixels of one lane group in a read group are columns c .. c+3 of one row and
// c+4 .. c+7 of the next); column pair and row parity on 4-wide planes (rows a, a+3 or a+1, a+2) - conflict free for all nine
// tap shifts (checked by enumeration).
__device__ __forceinline__ int h_sw_rows(int q) { return (q >> 1) & 3; }
template <int W_>
__device__ __forceinline__ int h_sw_patch(int q) {
  if constexpr (W_ <= 8) {
    const int pr = q / (W_ + 2), pc = q - pr * (W_ + 2);
    return W_ == 8 ? (pc >> 1) & 3 : (((pc >> 1) & 1) | ((pr & 1) << 1));
  } else {
    return h_sw_rows(q);
  }
}
__device__ __forceinline__ int h_pos(int c, int sw) { return (((c & 1) << 2) | ((c >> 2) << 1) | ((c >> 1) & 1)) ^ sw; }
__device__ __forceinline__ int h_chunk_at(int pos, int sw) {   // source chunk that lives at position `pos` of a row with swizzle bits sw
  const int x = pos ^ sw;
  return ((x >> 1) & 1) * 4 + (x & 1) * 2 + (x >> 2);
}

// Whether a tile runs the folded 1x1 shortcut (ConvP.sc_*; the kernel's HAS_SC and the variant row's folds_shortcut).
// Not on the sub-tiled planes, and not on the 48-cout tiles (variants 67 / 68): 92 -> 102 / 137 VGPRs with it, and no shortcut
// site runs either - conv2's K is never long enough for them.
constexpr bool h3_has_shortcut(int bn, int tps, bool sub) { return !sub && !(tps == 3 && bn == 48); }

// TPS: filter taps per K step (1, or 3 = one filter row): the small-plane variants (64 x 96 tiles over the 8x8 / 4x4
// levels, one MFMA wave per SIMD) do 3 taps between two barriers so that a step still carries 36 MFMAs per wave.
// Tiles may hold several whole samples (BM >= H * W: NSEG segments of SEG = H rows, each with its own halo rows) and
// the channel blocks may be split over blockIdx.z (fp32 slabs, reduced by k_splitk_reduce*, conv.hip).
// SUB: the plane is LARGER than the tile (the AF-VAE's 64^2 .. 256^2 planes): a tile is a ROWS x W_ block of an
// H x W plane, its patch the (ROWS + 2) x (W_ + 2) block around it - zero only where that leaves the image - and the
// tile's pixels are W_-long runs p.W pixels apart in memory.  (The implicit GEMM re-fetched the pixel tile for every
// tap there too: 0.69 PFLOP/s at 256^2 x 128 channels, profiles/r03.)

}  // namespace afldm
