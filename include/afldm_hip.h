/*
 * afldm_hip.h — C ABI of libafldm_hip.so: the MI355X (gfx950) kernels behind the
 * alias-free latent-diffusion denoising path of SingleZombie/AFLDM.
 *
 * The reference has NO native boundary on this path: its operator API is PyTorch
 * nn.Module surgery (afldm/af_modules/af_api.py:70-83) over diffusers modules whose
 * arithmetic is dispatched to cuDNN / cuBLAS / cuFFT / SDPA.  This header is the native
 * layer a maintainer would bind underneath those modules; each entry point names the
 * reference computation (file:line) it replaces.  See INTEGRATION.md for the ctypes
 * binding that afldm_amd ships and the module-level hook a reference maintainer would add.
 *
 * Conventions
 *   - every pointer except `afldm_filter_matrix`'s output is a DEVICE pointer;
 *   - activations are NHWC ("channels last"), contiguous, dtype AFLDM_F32 or AFLDM_BF16;
 *     [B, H*W, C] token tensors for attention are the same memory;
 *   - conv / linear weights are OHWI ([Cout][KH][KW][Cin]) in the activation dtype
 *     (afldm_pack_weight converts from the reference's OIHW fp32 state-dict layout);
 *     biases, GroupNorm affine parameters and statistics are fp32;
 *   - all launches are stream-ordered on `stream` (a hipStream_t), never block, never
 *     allocate; the caller owns every buffer (graph-capturable);
 *   - return 0 on success, <0 = AFLDM_E*; afldm_last_error() gives the message of the last
 *     failure on the calling thread.  No entry point aborts.
 */
#ifndef AFLDM_HIP_H
#define AFLDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* afldm_stream_t; /* hipStream_t */

enum { AFLDM_F32 = 0, AFLDM_BF16 = 1 };
enum {
  AFLDM_OK = 0,
  AFLDM_ESHAPE = -1,  /* unsupported / inconsistent shape */
  AFLDM_EDTYPE = -2,  /* unknown dtype code */
  AFLDM_EALIGN = -3,  /* pointer or leading dimension not 16-byte aligned */
  AFLDM_ELAUNCH = -4, /* HIP launch error */
  AFLDM_ENULL = -5    /* required pointer is NULL */
};

int afldm_version(void);
const char* afldm_last_error(void);
/* name[] receives gcnArchName; returns CU count (<0 on error). */
int afldm_device_info(char* name, int name_len);

/* ---- filter matrices (host) ------------------------------------------------------------
 * Builds the dense separable form of the reference's FFT-domain ideal filters from the
 * reference's mask rules (create_lpf_rect ideal_lpf.py:12-24, create_recon_rect :38-49):
 *   kind 0: U  [up*N x N], UpsampleRFFT(up)(X) == U X U^T      (ideal_lpf.py:148-158)
 *   kind 1: D  [N/2 x N],  LPF_RFFT(1/2)(Z)[::2,::2] == D Z D^T (ideal_lpf.py:69-93 + af_blocks.py:26)
 *   kind 2: L  [N x N],    LPF_RFFT(1/2)(Z) == L Z L^T           (ideal_lpf.py:69-93)
 * `out` is HOST memory, row-major fp32 (computed in fp64). */
int afldm_filter_matrix(int kind, int N, int up, float* out);

/* ---- layout / dtype plumbing ----------------------------------------------------------- */
/* src NCHW fp32 -> dst NHWC dtype (latent entry, randn_tensor ldm_pipeline.py:82-88) */
int afldm_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int dtype,
                       afldm_stream_t stream);
/* src NHWC dtype -> dst NCHW fp32 */
int afldm_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int dtype,
                       afldm_stream_t stream);
/* OIHW fp32 (state-dict layout) -> OHWI dtype.  KH*KW == 1 covers nn.Linear [O][I]. */
int afldm_pack_weight(const float* src, void* dst, int O, int I, int KH, int KW, int dtype,
                      afldm_stream_t stream);
/* dtype -> fp32 / fp32 -> dtype flat copies */
int afldm_cast(const void* src, int src_dtype, void* dst, int dst_dtype, size_t n,
               afldm_stream_t stream);

/* ---- timestep embedding ----------------------------------------------------------------
 * diffusers Timesteps / get_timestep_embedding as used by UNet2DModel.time_proj
 * (config configs/ldm/model_unet.json:28-29): out[r, :] = [cos(t w_i) | sin(t w_i)] when
 * flip_sin_to_cos, w_i = exp(-ln(10000) i / (dim/2 - freq_shift)).
 * `t` points to `rows` device floats (the timestep values).  out: [rows, dim] dtype. */
int afldm_timestep_embedding(const float* t, void* out, int rows, int dim, int flip_sin_to_cos,
                             float freq_shift, int dtype, afldm_stream_t stream);

/* y = silu(x), flat.  (TimestepEmbedding.act and ResnetBlock2D.nonlinearity on the 2-D temb:
 * af_blocks.py:20-21 keeps plain SiLU for <4-D tensors.) */
int afldm_silu(const void* x, void* y, size_t n, int dtype, afldm_stream_t stream);

/* ---- GroupNorm ----------------------------------------------------------------------------
 * torch.nn.GroupNorm(G, C, eps) over an NHWC tensor that is the virtual channel-concat of
 * x1 [B,HW,C1] and x2 [B,HW,C2] (x2 may be NULL with C2 = 0): the up-block skip
 * torch.cat([h, skip], 1) is never materialised.
 * Statistics are exchanged as PER-CHANNEL PARTIAL SUMS: stats[B][S][C][2] fp32 = (sum, sum of
 * squares) of channel c of ONE tensor over pixel-split s.  Producers: afldm_gn_stats (S =
 * afldm_gn_stats_splits(HW)) and afldm_conv2d, which emits the statistics of its output from the
 * GEMM epilogue (stats_out, S = afldm_conv2d_stats_splits(args)) so that most GroupNorms cost no
 * extra pass over the tensor.  Consumers (afldm_gn_apply, afldm_af_act, afldm_gn_table) take the
 * statistics of x1 and of x2 separately, add the partials of a group's channels in a fixed order
 * and finish mean / rstd in fp64: no finalize launch, no atomics, bit-reproducible; one tensor's
 * statistics serve both the next block and, later, a skip concatenation whose groups straddle
 * the two tensors. */
int afldm_gn_stats_splits(int HW);
int afldm_gn_stats(const void* x, int C, float* stats, int B, int HW, int dtype, afldm_stream_t stream);
/* y = act((x - mean) * rstd * gamma + beta); act: 0 none (Attention.group_norm),
 * 1 SiLU (conv_norm_out + conv_act, which make_af_unet does NOT wrap: af_api.py:70-83). */
int afldm_gn_apply(const void* x1, int C1, const void* x2, int C2, const float* stats1, int S1,
                   const float* stats2, int S2, const float* gamma, const float* beta, void* y, int B,
                   int HW, int G, float eps, int act, int dtype, afldm_stream_t stream);

/* Fold S_in row splits of per-channel partial sums [B][S_in][C][2] into [B][S_out][C][2] (S_in % S_out == 0):
 * the GEMM epilogue emits one split per 128-pixel tile, 512 per sample on the AF-VAE's 256^2 planes. */
int afldm_gn_fold(const float* stats_in, int S_in, float* stats_out, int S_out, int B, int C,
                  afldm_stream_t stream);

/* diagnostic: device buffer [workgroups][4 waves][2 items][10] of 64-bit shader-clock stamps that later afldm_af_act
 * launches on the plane kernel (N = 16 / 32) fill (phase boundaries of a workgroup's first two items; csrc/af.hip),
 * NULL = off (the default). */
int afldm_af_act_trace(void* buf);
/* Which kernel afldm_af_act / afldm_af_act_c8 run for a call, and how (the function the launch itself goes through):
 * route[0] = AFLDM_AF_ROUTE_*, route[1] = channels per item of the plane kernel (8 / 16, else 0), route[2] = grid,
 * route[3] = the most items one workgroup handles (plane: CH channels of a sample; kron / p8: 16 channels, one item per wave;
 * small: planes, one per thread).  cus = compute units to plan for, 0 = the current device's (only N = 16 / 32 ask);
 * has_packed / has_UD = whether the call passes the packed image / U and D.  Needs no GPU when cus > 0. */
#define AFLDM_AF_ROUTE_PLANE 0
#define AFLDM_AF_ROUTE_KRON 1
#define AFLDM_AF_ROUTE_P8 2
#define AFLDM_AF_ROUTE_SMALL 3
int afldm_af_act_route(int dtype, int N, int C1, int C2, int B, int cus, int has_packed, int has_UD, int* route);
/* The same for afldm_af_up2 / afldm_af_lpf_down2 / afldm_af_resample ([B,N,N,C] -> [B,R,R,C]): route[0] = AFLDM_RESAMPLE_ROUTE_*,
 * route[1] = threads per plane of the one-launch kernel (1 / 2 / 4, else 0). */
#define AFLDM_RESAMPLE_ROUTE_SMALL 0
#define AFLDM_RESAMPLE_ROUTE_REG 1
#define AFLDM_RESAMPLE_ROUTE_GENERIC 2
int afldm_af_resample_route(int N, int C, int R, int* route);
/* Tuning state of both planners, one field per call (tests, A/B timing).  Every field starts from its environment variable,
 * read once: AFLDM_AF_CH (0), AFLDM_AF_SMALL_N (4), AFLDM_AF_P8 (1), AFLDM_AF_STAGGER (0), AFLDM_NO_RESAMPLE_SMALL (0),
 * AFLDM_RESAMPLE_SPLIT (4); max_grid (0 = no cap) limits the plane kernel's grid so that a tensor of a few items gives
 * several items per workgroup.  AFLDM_AF_TUNE_RESET puts every field back to those defaults.  Not synchronised with
 * launches on other threads. */
#define AFLDM_AF_TUNE_RESET 0
#define AFLDM_AF_TUNE_CH 1
#define AFLDM_AF_TUNE_SMALL_N 2
#define AFLDM_AF_TUNE_P8 3
#define AFLDM_AF_TUNE_STAGGER 4
#define AFLDM_AF_TUNE_NO_RESAMPLE_SMALL 5
#define AFLDM_AF_TUNE_RESAMPLE_SPLIT 6
#define AFLDM_AF_TUNE_MAX_GRID 7
int afldm_af_tune(int field, int value);
/* ---- alias-free operators -----------------------------------------------------------------
 * afldm_af_act: [GroupNorm-apply ->] WarpedNonlinearity(SiLU) (af_blocks.py:19-28):
 *   y = D silu(U xn U^T) D^T per (b, c) plane,  xn = GN-applied x when stats1 != NULL
 *   (stats1 / stats2 = per-channel partial sums of x1 / x2, S1 / S2 their split counts).
 * x = virtual concat of x1/x2 as above, [B,N,N,C]; y [B,N,N,C].  N in {2,4,8,16,32}.
 * U: [2N x N], D: [N x 2N] device fp32 matrices from afldm_filter_matrix(0,N,2) / (1,2N,.). */
int afldm_af_act(const void* x1, int C1, const void* x2, int C2, const float* stats1, int S1,
                 const float* stats2, int S2, const float* gamma, const float* beta, int G, float eps,
                 const float* U, const float* D, const void* packed, void* y, int B, int N, int dtype,
                 afldm_stream_t stream);
/* The same with x1 and / or y in 8-channel blocks [B][C/8][N][N][8] (x_layout / y_layout = 1; afldm_conv_args.x_layout): N = 16 / 32,
 * bf16.  An item of the kernel - 8 (16) channels of one sample - is then one (two) contiguous 16 KB run instead of N^2 16-byte
 * pieces at a stride of 2 C bytes; the 3x3 convolutions of the block read / write the layout directly (afldm_conv2d_c8_ok). */
int afldm_af_act_c8(const void* x1, int C1, const void* x2, int C2, const float* stats1, int S1, const float* stats2,
                    int S2, const float* gamma, const float* beta, int G, float eps, const float* U, const float* D,
                    const void* packed, void* y, int B, int N, int dtype, int x_layout, int y_layout,
                    afldm_stream_t stream);
/* afldm_af_act on 2 x 2 planes, result stored ONCE per plane: y [B][C1+C2].  The reference's LPF_RFFT mask for the 4 x 4
 * upsampled plane is lpf(4) = [1,0,0,0] (ideal_lpf.py:17-21, M % 4 == 0 zeroes the Nyquist pair), so LPF_RFFT + [::2,::2] of
 * WarpedNonlinearity (af_blocks.py:19-28) leaves mean(silu(up(x))) in all four pixels: the activated 2 x 2 tensor is
 * plane-constant, bit for bit (the four outputs are one fmaf chain over equal operands).  A 3x3 'same' convolution of such
 * a tensor is a dense layer over Cin (not 4 Cin) columns whose weight is the sum of the taps that see each input pixel
 * (host: afldm_amd/models/blocks.py packed_conv_dense2x2_const) - a quarter of the weight bytes of the 2x2 level. */
int afldm_af_act_const2(const void* x1, int C1, const void* x2, int C2, const float* stats1, int S1, const float* stats2,
                        int S2, const float* gamma, const float* beta, int G, float eps, const float* U, const float* D,
                        void* y, int B, int dtype, afldm_stream_t stream);
/* conv1 -> (+ time embedding) -> norm2 -> WarpedNonlinearity of diffusers ResnetBlock2D.forward on 2 x 2 planes as ONE launch, for a
 * plane-constant input (the block's first WarpedNonlinearity, afldm_af_act_const2): a [B][Cin] is that activation, w [4 Cout][Cin] the
 * tap-summed dense form of conv1 with its rows ordered channel-major (row = 4 n + pixel, pixel = 2 oh + ow), bias [Cout], temb the
 * time_emb_proj row(s) (temb_stride elements between samples, 0 = one row for all), gamma / beta / G / eps norm2, U [4x2] / D [2x4]
 * the N = 2 filter matrices; y [B][Cout] = the plane-constant second activation (input of conv2's dense form).  A workgroup owns
 * one GroupNorm group x 16 samples, so statistics, normalisation and activation need no exchange (csrc/dense2.hip).  Rounding points
 * as afldm_conv2d + afldm_af_act_const2: the convolution output is rounded to `dtype` once before it is normalised.
 * _supported: 1 when there is a kernel (Cout / G in {8, 12, 24}, Cin a multiple of 8 MFMA K steps). */
int afldm_conv2x2_const_norm_act_supported(int Cin, int Cout, int G, int dtype);
int afldm_conv2x2_const_norm_act(const void* a, const void* w, const float* bias, const void* temb, int temb_stride,
                                 const float* gamma, const float* beta, int G, float eps, const float* U, const float* D, void* y,
                                 int B, int Cin, int Cout, int dtype, afldm_stream_t stream);
/* A convolution's split-K slabs straight into the GroupNorm that follows it, on the 2x2 / 4x4 planes (diffusers
 * resnet.py / attention_processor.py): the slabs a deferred afldm_conv2d left in its workspace ([nslab][B*N*N][C]
 * fp32) are summed in slab order, + bias[c] + temb[b*temb_stride + c] + residual, rounded to `dtype` (the value the
 * two-launch path stores; written to y_raw when other consumers need it), GroupNorm-ed with statistics formed
 * inside the launch (one workgroup holds whole groups of one sample: C / G channels x N*N pixels each, fp64
 * finish) and, with act = 1, passed through y = D silu(U xn U^T) D^T per plane:
 *   act = 1: conv1(...) + temb -> norm2 -> the WarpedNonlinearity af_api.py:70-83 wraps around `nonlinearity`
 *   act = 0: conv2(...) + shortcut -> Attention.group_norm of the attention block that follows the resnet
 *   act = 2: as act = 1 on 2 x 2 planes with the plane-constant result stored once, y [B][C] (see afldm_af_act_const2)
 * Replaces the reduction launch (and, for act = 1, the stored intermediate and its re-read).  N in {2, 4};
 * bias / temb / residual / y_raw may be NULL; temb_stride 0 = one row for all samples. */
int afldm_af_act_slabs(const float* slabs, int nslab, const float* bias, const void* temb, int temb_stride,
                       const void* residual, void* y_raw, const float* gamma, const float* beta, int G, float eps,
                       int act, const float* U, const float* D, void* y, int B, int C, int N, int dtype,
                       afldm_stream_t stream);
/* The tail of UNet2DModel.forward in one launch (bf16, 32x32 planes, C in {64, 128, 192}, Cout <= 4):
 * conv_norm_out (GroupNorm from the per-channel partial sums stats[B][S][C][2] of x) -> conv_act (plain SiLU:
 * af_api.py:70-83 leaves it unwrapped) -> conv_out (3x3 'same', weights packed OHWI [Cout][3][3][C], fp32 bias).
 * x NHWC [B,N,N,C]; y NHWC [B,N,N,Cout].  The activated tensor is never stored. */
int afldm_conv_out_fused(const void* x, const float* stats, int S, const float* gamma, const float* beta, int G,
                         float eps, const void* w, const float* bias, void* y, int B, int N, int C, int Cout,
                         int dtype, afldm_stream_t stream);
/* y = M x M^T per plane in ONE kernel (MFMA, no fp32 intermediate through HBM) for the two large
 * resampling sites of the UNet: AliasFreeUpsample2D at 16 -> 32 (M = U, af_blocks.py:92-93) and
 * AliasFreeDownsample2D at 32 -> 16 (M = D, af_blocks.py:149-150).  stats_out (optional):
 * per-channel GroupNorm partial sums of y, [B][1][C][2] (S = 1). */
int afldm_af_resample_plane(const void* x, const float* M, void* y, float* stats_out, int B, int N,
                            int C, int R, int dtype, afldm_stream_t stream);
/* One-time packing of U / D into the kernel's LDS image for the MFMA plane sizes (N = 16, 32):
 * `packed` = device buffer of afldm_af_pack_bytes(N, dtype) bytes, passed to afldm_af_act. */
size_t afldm_af_pack_bytes(int N, int dtype);
int afldm_af_pack(const float* U, const float* D, int N, int dtype, void* packed,
                  afldm_stream_t stream);
/* UpsampleRFFT(2) of AliasFreeUpsample2D (af_blocks.py:92-93): [B,N,N,C] -> [B,2N,2N,C].
 * workspace: device fp32 scratch of B*2N*N*C floats (row pass result). */
int afldm_af_up2(const void* x, const float* U, void* y, float* workspace, int B, int N, int C,
                 int dtype, afldm_stream_t stream);
/* LPF_RFFT(1/2) + [::2,::2] of AliasFreeDownsample2D (af_blocks.py:149-150):
 * [B,N,N,C] -> [B,N/2,N/2,C];  D: [N/2 x N];  workspace: B*(N/2)*N*C floats.
 * stats_out (optional, N a power of two <= 32, C % 4 == 0): per-channel GroupNorm partial sums of y with one
 * split per output row, [B][N/2][C][2]. */
int afldm_af_lpf_down2(const void* x, const float* D, void* y, float* workspace, float* stats_out, int B,
                       int N, int C, int dtype, afldm_stream_t stream);

/* Generic separable product y = M x M^T per (b, c) plane: [B,N,N,C] -> [B,R,R,C], M: [R x N]
 * device fp32.  Serves UpsampleRFFT(up) for any `up` (ImageShifter('ideal', 8):
 * shifters.py:163-170) and the same-size LPF_RFFT (kind 2 matrix).  workspace: B*R*N*C floats. */
int afldm_af_resample(const void* x, const float* M, void* y, float* workspace, int B, int N, int C,
                      int R, int dtype, afldm_stream_t stream);

/* y = Mh x Mw^T per plane with different matrices along H and W ([R][N] each): the phase-ramp shift
 * of shifters.py:103-132 (fourier_shift_batch) in dense circulant form.  workspace: B*R*N*C floats. */
int afldm_af_resample_hw(const void* x, const float* Mh, const float* Mw, void* y, float* workspace,
                         int B, int N, int C, int R, int dtype, afldm_stream_t stream);

/* ---- large-plane separable passes (alias-free VAE, planes 64^2 .. 256^2) ----------------------
 * y[line][r] = act(sum_k M[r][k] xn[line][k])            or, with M2 (chained in registers):
 * y[line][r2] = sum_r M2[r2][r] silu(sum_k M[r][k] xn[line][k])
 * A line is a strided vector: element k of line (outer, inner) sits at
 *   x + outer * in_outer_stride + inner + k * in_k_stride      (inner_count lines are contiguous).
 * xn = x * scale[b][c] + shift[b][c] when gn_table != NULL (b = outer / outer_per_sample,
 * c = inner % C; table from afldm_gn_table).  Used for UpsampleRFFT / LPF_RFFT on big planes and,
 * in three launches (up-H; up-W -> SiLU -> down-W chained; down-H), for WarpedNonlinearity when the
 * 2N x 2N plane does not fit LDS (af_blocks.py:19-28 at N = 64, 128 in the AF-VAE). */
typedef struct {
  const void* x;
  void* y;
  const float* M;        /* [R][K] device fp32 */
  const float* M2;       /* [R2][R] device fp32, or NULL */
  const float* gn_table; /* [B][C][2] device fp32, or NULL */
  long long outer_count, inner_count;
  long long in_outer_stride, in_k_stride, out_outer_stride, out_k_stride; /* elements */
  int K, R, R2;
  int C, outer_per_sample;
  int act;   /* 1: SiLU after M (only when R2 == 0) */
  int dtype;
  /* 1 (chained passes, R == 2 K): the caller guarantees M[2 i][k] = delta(i, k) - true of the reference's x2
   * periodic-sinc upsampler (ideal_lpf.py:96-121: the even phase of the zero-stuffed, recon-filtered signal is the
   * signal itself).  The even rows then need no product: M2 silu(M x) = M2[:, 0::2] silu(x) + M2[:, 1::2] silu(M[1::2] x).
   * Used where it pays (K = 128, bf16); 2 = also at K = 32 / 64, where the full product is faster (tests). */
  int up_identity;
} afldm_sep_args;
int afldm_sep_pass(const afldm_sep_args* args, afldm_stream_t stream);
/* table[b][c] = (rstd * gamma[c], beta[c] - mean * rstd * gamma[c]) from per-channel partial sums */
int afldm_gn_table(const float* stats, int S, const float* gamma, const float* beta, float* table, int B,
                   int C, int G, int HW, float eps, afldm_stream_t stream);
/* y[r][:] = softmax(x[r][:] * scale): the single-head d = 512 attention of the VAE mid block is
 * two GEMMs (afldm_conv2d with per-sample "weights") around this kernel. */
int afldm_softmax_rows(const void* x, void* y, long long rows, int cols, float scale, int dtype,
                       afldm_stream_t stream);

/* ---- convolution / linear as implicit GEMM on MFMA --------------------------------------
 * y[b,oh,ow,n] = bias[n] + temb[b*temb_stride + n] + residual[b,oh,ow,n]
 *              + sum_{kh,kw,ci} x[b, oh+kh-KS/2, ow+kw-KS/2, ci] * w[n,kh,kw,ci]
 * stride 1, zero padding KS/2, KS in {1,3}.  Replaces F.conv2d of ResnetBlock2D.conv1/conv2/
 * conv_shortcut, Downsample2D.conv with stride forced to 1 (af_blocks.py:129), Upsample2D.conv,
 * conv_in/conv_out, and nn.Linear (H = W = 1, B = rows) of Attention.to_q/k/v/to_out and the
 * time MLP.  x is the virtual concat of x1/x2.  out_mode 0: y NHWC with leading dim y_ld
 * (>= Cout, lets several GEMMs write column slices of one buffer); out_mode 1: channel-major
 * y[(b*Cout + n)*H*W + pix] (V^T for afldm_attention).
 * A pixel operand of 2 GiB or more (AF-VAE 256^2 levels at batch 128) is processed as B / c launches over c whole
 * samples each, c the largest divisor of B whose operand fits a buffer descriptor; afldm_conv2d_variant /
 * _stats_splits / _workspace answer for such a chunk. */
typedef struct {
  const void* x1;
  const void* x2;
  const void* w;
  const float* bias;
  const void* temb;     /* dtype T, may be NULL */
  const void* residual; /* dtype T, [B*H*W][res_ld], may be NULL */
  void* y;
  void* workspace; /* fp32 split-K slabs, may be NULL (=> no split-K) */
  size_t workspace_bytes;
  int C1, C2;
  int B, H, W, Cout, KS;
  int temb_stride; /* elements between samples in temb (0 = broadcast one row) */
  int res_ld, y_ld;
  int out_mode;
  int dtype;
  /* optional column split (fused Q|K|V projection): couts >= split_n go, channel-major
   * ([B][Cout - split_n][H*W]), to y2 instead of y; y then holds couts [0, split_n) with y_ld. */
  void* y2;
  int split_n;
  /* optional GroupNorm statistics of the OUTPUT (out_mode 0, no y2): per-channel partial sums
   * stats_out[B][S][Cout][2] fp32 with S = afldm_conv2d_stats_splits(args), computed on the stored
   * (rounded) values by the GEMM epilogue / the split-K reduction; NULL = none. */
  float* stats_out;
  /* 0, or the period of the time-embedding column: temb[b*temb_stride + n % temb_mod] (a 3x3
   * convolution on a 2x2 plane executed as ONE dense layer over the flattened plane: cout index =
   * pixel * C + c, every pixel takes the same per-channel time embedding; must divide Cout). */
  int temb_mod;
  /* optional: `sync_bytes` >= 40960 bytes of device memory that is ZERO before the first call and is left zero by
   * every call (one buffer serves all launches of a stream).  With it - and afldm_conv2d_fused_splitk(1) - a split-K
   * convolution whose workgroups all fit on the chip at once reduces its K slices inside the GEMM launch (arrival counter per output tile, slabs
   * written through, each slice finishing 1/splitk of the tile's rows) instead of in a second kernel; results are
   * bit-identical.  NULL = always the two-launch form. */
  unsigned int* sync;
  size_t sync_bytes;
  /* 1: when the call splits K (afldm_conv2d_variant(args) >> 8 & 255 = nslab > 1), leave the fp32 partial sums in
   * `workspace` ([nslab][B*H*W][Cout]: plain sums, no bias / temb / residual) and do NOT launch the reduction - the
   * caller hands them to a consumer that finishes them itself (afldm_af_act_slabs).  y / stats_out are not written.
   * Ignored (the call completes as usual) when K is not split. */
  int defer_reduce;
  /* 0, or the distance IN ELEMENTS between the weight tensors of consecutive samples: sample b is convolved with
   * w + b * w_batch_stride (KS = 1, out_mode 0, no split-K; a tile never spans two samples).  This is the "per-sample weights"
   * GEMM of the AF-VAE's single-head d = 512 attention (af_vae.py / diffusers AttnProcessor2_0): scores = Q_b K_b^T with K_b as
   * the weights, then P_b V_b with V_b^T as the weights - one launch for the batch instead of one per sample. */
  long long w_batch_stride;
  /* optional: the GroupNorm that FOLLOWS this convolution (diffusers Attention.group_norm behind ResnetBlock2D.conv2), applied by the
   * convolution's own epilogue where one tile holds a whole sample and whole groups (8x8 planes, bf16): y_norm [B*H*W][Cout] =
   * (y - mean_g) rstd_g gamma + beta with the statistics of the stored (rounded) y; y itself is written as usual.  Only honoured when
   * afldm_conv2d_norm_ok(args) == 1 (set y_norm = NULL otherwise and run afldm_gn_apply). */
  void* y_norm;
  const float* norm_gamma;
  const float* norm_beta;
  int norm_groups;
  float norm_eps;
  /* Operand layouts: 0 = NHWC (x [B,H,W,C], y [B,H,W,Cout]); 1 = 8-channel blocks [B][C/8][H][W][8] (bf16; 16 bytes per pixel and
   * block: what afldm_af_act writes / reads with y_layout / x_layout = 1).  The activation <-> 3x3 convolution tensors inside a
   * ResnetBlock2D travel in layout 1 where afldm_conv2d_c8_ok(args) == 1: an activation item (8 channels of a sample) is one
   * contiguous run instead of H*W 16-byte pieces.  Same values, same arithmetic. */
  int x_layout;
  int y_layout;
  /* optional: the 1x1 conv_shortcut of diffusers ResnetBlock2D (in_channels != out_channels) folded into its conv2, the call being
   * conv2 itself: y = conv3x3(x1) + conv1x1(sc_x1 | sc_x2, sc_w) + bias, where `bias` is conv2.bias + conv_shortcut.bias and there
   * is no `residual`.  sc_x1 [B*H*W][sc_C1] and sc_x2 [B*H*W][sc_C2] (NHWC, dtype T; sc_x2 NULL when sc_C2 = 0) are the block input
   * (a virtual concat on the up path), sc_w [Cout][sc_C1 + sc_C2] the 1x1 weight in the afldm_pack_weight (OHWI) form.  The
   * shortcut's channels run as extra centre-tap K steps of the halo-patch kernel (one 128-byte channel block per step; where K is
   * split, each slice takes its share of them and the slabs carry conv2 + shortcut partial sums); only honoured where
   * afldm_conv2d_shortcut_ok(args) != 0 (sc_x1 = NULL otherwise, and run the 1x1 convolution as its own call feeding `residual`). */
  const void* sc_x1;
  const void* sc_x2;
  const void* sc_w;
  int sc_C1, sc_C2;
} afldm_conv_args;
int afldm_conv2d(const afldm_conv_args* args, afldm_stream_t stream);
/* 1: afldm_conv2d(args) accepts x_layout = 1 and / or y_layout = 1 (asked with both at 0 or 1: the answer does not depend on them). */
int afldm_conv2d_c8_ok(const afldm_conv_args* args);
/* 1: afldm_conv2d(args) will apply the GroupNorm described by norm_gamma / norm_beta / norm_groups / norm_eps into y_norm itself. */
int afldm_conv2d_norm_ok(const afldm_conv_args* args);
/* != 0: afldm_conv2d(args) accepts the folded shortcut described by sc_x1 / sc_x2 / sc_w / sc_C1 / sc_C2 (one halo-patch launch, no
 * residual).  1: a tile with one filter tap per K step, whole K per workgroup (the 32^2 / 16^2 levels at the larger batches);
 * 2: a tile with three taps per K step (the 8^2 / 4^2 levels, every level at the small batches) - K may be split there, with
 * defer_reduce (the slabs to afldm_af_act_slabs, which then takes bias = b2 + b_sc and no residual) or y_norm. */
int afldm_conv2d_shortcut_ok(const afldm_conv_args* args);
/* Tuning hook (benchmarks only): force tile/pipeline variant `variant` (>= 0) and/or a split-K
 * factor (>= 1) for subsequent afldm_conv2d calls; -1 restores the automatic choice.  Variant ids are sparse: the
 * live ones are 0, 1, 3 (register-staged GEMM), 29 - 33 (LDS-DMA GEMM) and 41, 43, 46, 51, 52, 54, 55, 58, 63,
 * 65 - 68 (halo-patch 3x3); every other id (retired tuning variants) is refused with AFLDM_ESHAPE and
 * leaves the forcing as it was.  A forced variant that cannot run a shape falls back to the automatic choice. */
int afldm_conv2d_tune(int variant, int splitk);
/* Enable (1) / disable (0, the default) the in-kernel split-K reduction for calls that pass `sync` words: measured
 * slower than the two-launch form on MI355X, kept as a tested option. */
int afldm_conv2d_fused_splitk(int enable);
/* How afldm_conv2d will run this problem (tests / tuning tools): GEMM tile variant | split-K slices << 8 | in-kernel
 * reduction << 16; < 0 for the direct (non-GEMM) kernels. */
int afldm_conv2d_variant(const afldm_conv_args* args);
/* bytes of split-K workspace afldm_conv2d may use for this problem (0 if none). */
size_t afldm_conv2d_workspace(const afldm_conv_args* args);
/* split count S of the statistics afldm_conv2d writes to stats_out for this problem (> 0). */
int afldm_conv2d_stats_splits(const afldm_conv_args* args);

/* ---- vanilla resamplers (diffusers Downsample2D / Upsample2D with use_conv; csrc/resconv.hip) ---------------------------
 * Read from afldm_conv_args: x1, w, bias (fp32, may be NULL), y, B, H, W (the INPUT plane), C1 (= Cin), Cout, dtype and
 * stats_out (may be NULL: then [B][S][Cout][2] per-channel partial sums of the stored output, S = the matching _stats_splits);
 * every other field is ignored.  Cin and Cout multiples of 8; inputs of 2 GiB or more run as launches over whole samples.
 * afldm_conv2d_s2: F.conv2d(x, w, bias, stride=2) of the zero-padded x (pad_lo rows / columns in front, pad_hi behind; the
 *   UNet's padding=1 is (1, 1), the VAE encoder's F.pad(x, (0, 1, 0, 1)) + padding=0 is (0, 1)); w OHWI [Cout][3][3][Cin]
 *   (afldm_pack_weight); H, W even; y [B, H/2, W/2, Cout].
 * afldm_conv2d_up2: F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, bias, padding=1) without the x2 tensor:
 *   output pixel (2i + a, 2j + c) is a 2x2 convolution of x around (i, j) with phase-folded weights, w = the
 *   afldm_pack_weight_up2 form; Cout a multiple of 64; y [B, 2H, 2W, Cout]. */
int afldm_conv2d_s2(const afldm_conv_args* args, int pad_lo, int pad_hi, afldm_stream_t stream);
int afldm_conv2d_up2(const afldm_conv_args* args, afldm_stream_t stream);
int afldm_conv2d_s2_stats_splits(const afldm_conv_args* args);
int afldm_conv2d_up2_stats_splits(const afldm_conv_args* args);
/* OIHW fp32 [Cout][Cin][3][3] -> the folded up2 weight [4][Cout][2][2][Cin] in `dtype`, phase = 2 a + c.  Per axis, phase 0
 * takes taps {i-1: w0, i: w1 + w2} and phase 1 {i: w0 + w1, i+1: w2}; rows are folded first, then columns, in fp32, and the
 * sum is rounded once. */
int afldm_pack_weight_up2(const float* src, void* dst, int Cout, int Cin, int dtype, afldm_stream_t stream);

/* ---- attention ---------------------------------------------------------------------------
 * F.scaled_dot_product_attention as called by AttnProcessor2_0 / CrossFrameAttnProcessor
 * (cross_frame_attn.py:125,128): o = softmax(q k^T * scale) v per (batch, head).
 * q [B,Tq,ldq] k [Bk,Tk,ldk] token-major with head h at columns [h*d, (h+1)*d);
 * vt [Bk, heads*d, Tk] channel-major (written by afldm_conv2d out_mode 1); o [B,Tq,ldo].
 * Bk divides B: sample b reads K/V of kv-sample b / (B/Bk)  (the batch repeat of
 * cross_frame_attn.py:91-96). */
int afldm_attention(const void* q, int ldq, const void* k, int ldk, const void* vt, void* o, int ldo,
                    int B, int Bk, int heads, int Tq, int Tk, int d, float scale, int dtype,
                    afldm_stream_t stream);
/* The interpolating cross-frame attention (reference cross_frame_attn.py:100-122, enable_interp) with the two
 * stored passes' K / V^T as two sources, blended per sample: for sample b, kb = b / (B/Bk),
 *   o[b] = (1 - alpha[b]) softmax(q_b k0_kb^T scale) v0_kb + alpha[b] softmax(q_b k1_kb^T scale) v1_kb
 * Each source's softmax is normalised on its own; the blend is fp32 and o is rounded once.  alpha [B] is fp32
 * DEVICE memory read when the kernel runs (a captured graph picks up new values at every replay).  Operand
 * layouts and limits are those of afldm_attention; the two sources share ldk and shape.  One launch replaces two
 * attentions: to_out is affine and the residual common to both terms, so the blend may sit before to_out. */
int afldm_attention_interp(const void* q, int ldq, const void* k0, const void* k1, int ldk, const void* vt0,
                           const void* vt1, const float* alpha, void* o, int ldo, int B, int Bk, int heads, int Tq,
                           int Tk, int d, float scale, int dtype, afldm_stream_t stream);
/* The same blended attention over a BANK of S stored sources, every sample naming its own two: k [S,Tk,ldk] and
 * vt [S,heads*d,Tk] in afldm_attention's layouts (a STORE pass at batch S leaves exactly this), src int32 [B,2] and
 * alpha fp32 [B] in DEVICE memory, both read when the kernel runs (a replayed graph sees the values of its replay).
 * With s0 = clamp(src[b][0]), s1 = clamp(src[b][1]) (clamped into [0, S) in the kernel),
 *   o[b] = (1 - alpha[b]) softmax(q_b k[s0]^T scale) vt[s0] + alpha[b] softmax(q_b k[s1]^T scale) vt[s1]
 * in afldm_attention_interp's arithmetic.  alpha[b] == 0.0f skips source 1 altogether (neither staged nor read): the
 * sample costs, and equals, the single-source attention on k[s0].  Limits are afldm_attention's, S >= 1, src and alpha
 * non-NULL and 4-byte aligned. */
int afldm_attention_bank(const void* q, int ldq, const void* k, int ldk, const void* vt, const int* src,
                         const float* alpha, void* o, int ldo, int B, int S, int heads, int Tq, int Tk, int d,
                         float scale, int dtype, afldm_stream_t stream);

/* ---- attention block front end, fused ------------------------------------------------------
 * group_norm -> to_q | to_k | to_v -> scaled_dot_product_attention of diffusers' AttnProcessor2_0 on the deprecated
 * attention-block configuration (the self-attention path of reference cross_frame_attn.py:66-77 in IDLE / STORE state;
 * diffusers attention_processor.py AttnProcessor2_0.__call__) as ONE launch: a workgroup owns a (sample, head), normalises
 * the raw tokens x [B,T,C] from the producer's per-channel partial sums `stats` [B,S,C,2] (as afldm_gn_apply does),
 * projects its head's q / k / v with w_qkv [3C,C] (to_q | to_k | to_v rows) + bias_qkv [3C] and runs the attention
 * against K / V^T resident in LDS; o [B,T,C] = the input of to_out.  q | k | v never exist in memory.
 * bf16 only; shapes: see afldm_attn_block_fused_supported (1 = there is a kernel for T tokens, C channels, head_dim,
 * G groups).  Rounding points: q, k, v and the softmax weights are rounded to bf16 as in afldm_conv2d + afldm_attention,
 * but the NORMALISED TOKENS ARE NEVER MATERIALISED: GroupNorm is folded into the head's weight rows, W' = bf16(W * rstd *
 * gamma) with the shift in the (fp32) bias, so bf16 rounds W' where the three-launch path rounds the normalised tokens, and
 * the softmax scale is applied to q before its one rounding.  Same error class (2.1e-3 against 1.9e-3 vs the fp32 form on
 * random data), different bits: a sample's bf16 result depends on which path its batch selected (policy: ops.py
 * _FUSED_ATTN_MIN_WGS; tests pin the path). */
int afldm_attn_block_fused_supported(int T, int C, int head_dim, int G);
/* diagnostic: device buffer [workgroups][waves][12] of 64-bit shader-clock stamps that later afldm_attn_block_fused
 * launches fill (phase boundaries per wave; csrc/attnf.hip), NULL = off (the default). */
int afldm_attn_block_fused_trace(void* buf);
int afldm_attn_block_fused(const void* x, const float* stats, int S, const float* gamma, const float* beta, int G,
                           float eps, const void* w_qkv, const float* bias_qkv, void* o, int B, int T, int C,
                           int heads, float scale, int dtype, afldm_stream_t stream);
/* The same launch carrying the rest of the attention block: y = to_out(o) + x (diffusers Attention.to_out[0] + the
 * residual connection of the attention-block configuration) and stats_out [B,heads,C,2] = per-channel partial sums of the
 * rounded y (the next GroupNorm's input; split h covers the token block [h T / heads, (h+1) T / heads)).  The `heads`
 * workgroups of a sample hand their o slices over inside the launch (one counter line per sample in `sync`, int32 words
 * [16384 + 32 b, ...), zero between launches; word 8193 = 1 when a workgroup gave up waiting, 2 when a sample's workgroups
 * were not on one XCD) and workgroup h then runs the to_out GEMM of its token block out of the XCD's L2.  w_out [C,C],
 * bias_out [C] fp32.  Shapes: afldm_attn_block_fused_out_supported (the 32 x 32 level, B a multiple of 8). */
int afldm_attn_block_fused_out_supported(int B, int T, int C, int head_dim, int G);
int afldm_attn_block_fused_out(const void* x, const float* stats, int S, const float* gamma, const float* beta, int G,
                               float eps, const void* w_qkv, const float* bias_qkv, void* o, const void* w_out,
                               const float* bias_out, void* y, float* stats_out, void* sync, long long sync_bytes, int B,
                               int T, int C, int heads, float scale, int dtype, afldm_stream_t stream);

/* ---- DDIM update -------------------------------------------------------------------------
 * DDIMScheduler.step, eta = 0, epsilon prediction, no clipping:
 *   x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t);  x_prev = sqrt(a_prev) x0 + sqrt(1-a_prev) eps
 * coef: device float[4*nsteps] rows (sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev));
 * step_idx: device int, row to use; if advance != 0 the kernel increments it afterwards (so
 * a captured hipGraph of one step can be replayed 50x with no host involvement).
 * x, x_prev: NCHW fp32 latents [B,C,H,W]; eps: NHWC dtype (the UNet output layout). */
int afldm_ddim_step(const float* x, const void* eps, float* x_prev, const float* coef,
                    int* step_idx, int advance, int B, int C, int H, int W, int dtype,
                    afldm_stream_t stream);
/* Same update on flat fp32 tensors with the coefficients by value: the
 * DDIMScheduler.step(model_output, timestep, sample) API (ldm_pipeline.py:108-109). */
int afldm_ddim_step_flat(const float* x, const float* eps, float* x_prev, float sqrt_a_t,
                         float sqrt_1m_a_t, float sqrt_a_prev, float sqrt_1m_a_prev, size_t n,
                         afldm_stream_t stream);
/* ---- DPM-Solver(++) multistep update ---------------------------------------------------------
 * DPMSolverMultistepScheduler.step, orders 1-3, epsilon / v / sample prediction, no thresholding: each step is
 * the coefficient row (p, q, a, b0, b1, b2, 0, 0) applied elementwise,
 *   m0 = p x + q eps;  x_out = a x + b0 m0 + b1 h1 + b2 h2;  then h2 <- h1, h1 <- m0
 * (m0: the converted model output - x0 for dpmsolver++, eps for dpmsolver; h1, h2: the two before it).
 * coef: device float[8*nsteps]; step_idx / advance as afldm_ddim_step (capturable).
 * x, x_out: NCHW fp32 [B,C,H,W], may alias; eps: NHWC dtype; hist: fp32 [2][B][C][H][W], h1 then h2,
 * zeroed before the first step (its coefficients are 0 there, but 0 * NaN is not). */
int afldm_dpm_step(const float* x, const void* eps, float* x_out, float* hist, const float* coef, int* step_idx,
                   int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream);
/* Same update on flat same-layout fp32 tensors of n elements, hist [2][n], the row by value: the
 * DPMSolverMultistepScheduler.step(model_output, timestep, sample) API. */
int afldm_dpm_step_flat(const float* x, const float* eps, float* x_out, float* hist, float p, float q, float a,
                        float b0, float b1, float b2, size_t n, afldm_stream_t stream);
/* ---- Stochastic sampler update (DDIM eta != 0, the I2SB bridge) ---------------------------------------------
 * diffusers DDIMScheduler.step with eta != 0 (epsilon prediction, no clip) and I2SBScheduler.step in every
 * (is_ode, clip_sample) form: step s = *step_idx applies the row coef[8 s .. 8 s + 8) = (p, q, lo, hi, a, b, d, c),
 *   x0 = clamp(p x + q eps, lo, hi);  x_out = a x + b x0 + d eps + c z,  z = noise[s * noise_step_stride + i]
 * lo = -inf, hi = +inf: no clip; the clamp passes a NaN through as torch.clamp does.  The noise rows are drawn by the
 * caller's generator before the step (outside any captured graph): the same randn calls as the eager loop.
 * x, x_out: NCHW fp32 [B,C,H,W], may alias; noise: fp32 rows of [B,C,H,W] NCHW, noise_step_stride floats apart
 * (>= B*C*H*W: a branch passes its batch slice of a larger buffer); eps: NHWC dtype; advance as afldm_ddim_step. */
int afldm_sde_step(const float* x, const void* eps, const float* noise, size_t noise_step_stride, float* x_out,
                   const float* coef, int* step_idx, int advance, int B, int C, int H, int W, int dtype,
                   afldm_stream_t stream);
/* ---- RePaint inpainting update (Lugmayr et al., CVPR 2022, Algorithm 1; diffusers RePaintPipeline) -------------
 * Step s = *step_idx applies the row coef[12 s .. 12 s + 12) = (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0) and the three noise
 * slots z_k, z_u, z_b = noise[s * noise_step_stride + slot * noise_slot_stride + i], slot = 0, 1, 2:
 *   x0      = clamp(p x + q eps, lo, hi)              lo = -inf, hi = +inf: no clip; a NaN passes through
 *   unknown = a x0 + b eps + c z_u                    the DDIM reverse step of the generated part
 *   knownp  = k0 known + k1 z_k                       the kept latents, noised to the same level
 *   y       = m knownp + (1 - m) unknown              m = mask[b, 0, h, w], 1 = keep, soft values allowed
 *   x_out   = u0 y + u1 z_b                           the jump back up the schedule, one Gaussian step
 * A slot whose coefficient (k1, c, u1) is exactly 0 is not read: what an unused slot holds does not reach x_out.
 * x, known, x_out: NCHW fp32 [B,C,H,W], x_out may alias x; mask: fp32 [B,1,H,W]; eps: NHWC dtype; noise: fp32 slots of
 * [B,C,H,W] NCHW (noise_slot_stride >= B*C*H*W, noise_step_stride >= 2 noise_slot_stride + B*C*H*W: a branch passes its
 * batch slice of a [steps,3,B,C,H,W] buffer), drawn by the caller's generator outside any captured graph; step_idx /
 * advance as the DDIM update above. */
int afldm_repaint_step(const float* x, const void* eps, const float* known, const float* mask, const float* noise,
                       size_t noise_step_stride, size_t noise_slot_stride, float* x_out, const float* coef, int* step_idx,
                       int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream);
/* Same update on flat same-layout fp32 tensors of n elements (the mask expanded to that layout too), the row by value, for
 * an eager loop.  z_k / z_u / z_b may be NULL where k1 / c / u1 is 0. */
int afldm_repaint_step_flat(const float* x, const float* eps, const float* known, const float* mask, const float* z_k,
                            const float* z_u, const float* z_b, float* x_out, float p, float q, float lo, float hi, float a,
                            float b, float c, float k0, float k1, float u0, float u1, size_t n, afldm_stream_t stream);
/* Pixel mask -> latent mask: mask fp32 [B,1,H,W] -> out fp32 [B,1,H/r,W/r] over r x r blocks, any r >= 1 dividing H and W.
 * AFLDM_MASK_MIN: the block minimum (a latent is kept only if every pixel under it is kept); AFLDM_MASK_MEAN: the block
 * mean (summed in fp64, rounded once). */
enum { AFLDM_MASK_MIN = 0, AFLDM_MASK_MEAN = 1 };
int afldm_mask_pool(const float* mask, float* out, int B, int H, int W, int r, int mode, afldm_stream_t stream);
/* ---- Image-to-image update: SDEdit (Meng et al., ICLR 2022) with a change map (Differential Diffusion, Levin & Fried 2023)
 * Step s = *step_idx applies the row coef[12 s .. 12 s + 12) = (p, q, lo, hi, a, b, c, k0, k1, thr, 0, 0), the run's one fixed
 * noise z and the step's noise z_u = noise[s * noise_step_stride + i]:
 *   x0    = clamp(p x + q eps, lo, hi)                lo = -inf, hi = +inf: no clip; a NaN passes through
 *   xp    = a x0 + b eps + c z_u                      the DDIM reverse step of a released element
 *   held  = k0 orig + k1 z                            the original, noised to the next level
 *   x_out = (m <= thr) ? held : xp                    m = cmap[b, 0, h, w], the change map: 0 = keep, 1 = regenerate
 * The last line is a select, not a blend: at a held element nothing of x, eps or z_u reaches x_out (not even a NaN or Inf),
 * and a NaN in cmap compares false, so that element is generated.  z is not read where k1 = 0 and z_u not where c = 0: an
 * unused buffer may hold anything.  noise may be NULL for a schedule none of whose rows has c != 0 (no z_u is added then).
 * x, orig, z, x_out: NCHW fp32 [B,C,H,W], x_out may alias x; cmap: fp32 [B,1,H,W]; eps: NHWC dtype; noise: fp32 rows of
 * [B,C,H,W] NCHW, noise_step_stride floats apart (>= B*C*H*W: a branch passes its batch slice of a larger buffer), drawn by
 * the caller's generator outside any captured graph; step_idx / advance as the DDIM update above. */
int afldm_sdedit_step(const float* x, const void* eps, const float* orig, const float* cmap, const float* z, const float* noise,
                      size_t noise_step_stride, float* x_out, const float* coef, int* step_idx, int advance, int B, int C,
                      int H, int W, int dtype, afldm_stream_t stream);
/* Same update on flat same-layout fp32 tensors of n elements (the change map expanded to that layout too), the row by value,
 * for an eager loop - and for the start of a run: the row (0, 0, -inf, inf, 0, 0, 0, k0, k1, +inf) gives k0 orig + k1 z, the
 * formula every held element follows.  z / z_u may be NULL where k1 / c is 0. */
int afldm_sdedit_step_flat(const float* x, const float* eps, const float* orig, const float* cmap, const float* z,
                           const float* z_u, float* x_out, float p, float q, float lo, float hi, float a, float b, float c,
                           float k0, float k1, float thr, size_t n, afldm_stream_t stream);
/* ---- Bit-reversible update: two-step (leapfrog) DDIM after BDIA (Zhang et al., ECCV 2024, gamma = 1) on int64 latents ----
 * Every latent element is an int64 X on the grid 2^-32 (Q31.32).  Step s = *step_idx applies the row
 * coef[4 s .. 4 s + 4) = (cx, ce, sign, boot) - sign +1 or -1, boot 0 or 1, as floats - to the pair (far, near):
 *   f = boot ? near : far;  n = near;  e = (float)eps
 *   x = rn_f32(n) * 2^-32                               one int64 -> fp32 rounding to nearest even, then an exact scale
 *   d = fl32(fl32(cx * x) + fl32(ce * e))               two products and one sum, no fma
 *   q = rn_i64(d * 2^32)                                the product is exact; ties to even
 *   new = f + sign * q;   far <- n;   near <- new;   lat_out <- rn_f32(new) * 2^-32
 * q depends on near and eps alone, so the same row with the opposite sign, applied to the rotated pair, restores both tensors
 * bit for bit.  Trouble - a non-finite d, |d * 2^32| >= 2^63, signed overflow of the add - makes q = 0 for that element and
 * stores 1 into bad[b] (never a 0: the caller zeroes bad before a run and reads it once after).
 * far, near: int64 NCHW [B,C,H,W], 8-byte aligned (AFLDM_EALIGN), two different buffers (AFLDM_ESHAPE); lat_out: fp32 NCHW;
 * bad: int32 [B]; eps: NHWC dtype; step_idx / advance as the DDIM update above.  16-byte accesses where C*H*W is even and
 * far / near are 16-byte, lat_out 8-byte aligned; element by element otherwise. */
int afldm_rev_step(long long* far, long long* near, const void* eps, float* lat_out, int* bad, const float* coef, int* step_idx,
                   int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream);
/* Same update on flat same-layout tensors of n elements (eps fp32), the row by value (sign +1 or -1: AFLDM_ESHAPE otherwise),
 * for an eager loop.  bad has one word per rows_per_sample consecutive elements (> 0).  far == near is accepted with boot != 0
 * only (a boot step does not read far; the buffer then ends up holding new). */
int afldm_rev_step_flat(long long* far, long long* near, const float* eps, float* lat_out, int* bad, float cx, float ce, int sign,
                        int boot, size_t n, size_t rows_per_sample, afldm_stream_t stream);
/* The entry conversion X = rn_i64(x * 2^32) of n fp32 values (the product is exact; ties to even).  A non-finite x or
 * |x| >= 2^31 gives X = 0 and stores 1 into bad[i / per_sample] (per_sample > 0).  X 8-byte aligned. */
int afldm_rev_encode(const float* x, long long* X, int* bad, size_t n, size_t per_sample, afldm_stream_t stream);
/* ---- ILVR reference-guided update (Choi et al., ICCV 2021, Algorithm 1) with a linear low-pass phi -----------------
 * Step s = *step_idx applies the row coef[12 s .. 12 s + 12) = (p, q, lo, hi, a, b, c, k0, k1, w, 0, 0) and the two noise
 * slots z_k, z_u = noise[s * noise_step_stride + slot * noise_slot_stride + i], slot = 0, 1:
 *   x0    = clamp(p x + q eps, lo, hi)              lo = -inf, hi = +inf: no clip; a NaN passes through
 *   xp    = a x0 + b eps + c z_u                    the unconditional proposal (the DDIM reverse step)
 *   yk    = k0 ref + k1 z_k                         the reference, noised to the same level
 *   x_out = xp + w (Lh (yk - xp) Lw^T)              per (b, c) plane: phi(d) = Lh d Lw^T
 * It replaces, per step: the stochastic step, a subtraction, NCHW -> NHWC, afldm_af_resample (which rounds d to the model
 * dtype), NHWC -> NCHW and an addition.  Lh, Lw: fp32 [S][S] row-major, general (no symmetry assumed), may be the same
 * pointer.  Every sum runs k = 0 .. S-1 ascending in fp32 fmaf: a plane's bits do not depend on B or on the batch slice.
 * z_k is not read where k1 = 0 or w = 0, z_u not where c = 0; with w = 0 neither are ref, Lh and Lw, and the launch is the
 * plain stochastic step.  Planes are square, 2 <= H = W <= 64 (AFLDM_ESHAPE otherwise, before any launch).
 * x, ref, x_out: NCHW fp32 [B,C,H,W], x_out may alias x; eps: NHWC dtype; noise: fp32 slots of [B,C,H,W] NCHW
 * (noise_slot_stride >= B*C*H*W, noise_step_stride >= noise_slot_stride + B*C*H*W: a branch passes its batch slice of a
 * [steps,2,B,C,H,W] buffer), drawn by the caller's generator outside any captured graph; step_idx / advance as the DDIM
 * update above. */
int afldm_ilvr_step(const float* x, const void* eps, const float* ref, const float* noise, size_t noise_step_stride,
                    size_t noise_slot_stride, const float* Lh, const float* Lw, float* x_out, const float* coef, int* step_idx,
                    int advance, int B, int C, int H, int W, int dtype, afldm_stream_t stream);
/* Same update on same-layout fp32 tensors of `planes` contiguous H x W planes (eps too), the row by value, for an eager
 * loop.  z_k / z_u may be NULL where they are not read; with w = 0 so may ref, Lh and Lw. */
int afldm_ilvr_step_flat(const float* x, const float* eps, const float* ref, const float* z_k, const float* z_u,
                         const float* Lh, const float* Lw, float* x_out, float p, float q, float lo, float hi, float a, float b,
                         float c, float k0, float k1, float w, size_t planes, int H, int W, afldm_stream_t stream);
/* ---- Perturbed-attention guidance (Ahn et al. 2024; diffusers PAGMixin) ------------------------------------------------
 * The perturbed attention block: the attention map replaced by the identity, so that softmax(q k^T) v is v and the block is
 *   y[b,t,:] = x[b,t,:] + GN(x)[b,t,:] W_vo^T + b_vo,    W_vo = W_o W_v,  b_vo = W_o b_v + b_o   (folded by the caller)
 * in ONE launch.  x, y: [B,T,C] token-major (NHWC), y must not alias x; stats [B,S,C,2], gamma, beta, G, eps exactly as
 * afldm_gn_apply takes them (mean / rstd are finished the same way); w_vo: [C,C] row-major in dtype (what afldm_pack_weight
 * makes of a Linear weight); bias_vo: fp32 [C].  GroupNorm is applied to the token operand and rounded once to bf16 (what
 * afldm_gn_apply stores); fp32 accumulation on MFMA, then + bias + x and one output rounding.
 * afldm_attn_identity_block_ok: 1 where there is a kernel - bf16, G = 32, T in {4, 16, 64, 256, 1024}, C in {64, 128, 192,
 * 384, 768}, any B >= 1 with B*T*C < 2^31; 0 otherwise (the caller then runs afldm_gn_apply + afldm_conv2d with `residual`
 * on the same folded weight), and afldm_attn_identity_block itself returns AFLDM_ESHAPE there. */
int afldm_attn_identity_block_ok(int B, int T, int C, int G, int dtype);
int afldm_attn_identity_block(const void* x, const float* stats, int S, const float* gamma, const float* beta, int G,
                              float eps, const void* w_vo, const float* bias_vo, void* y, int B, int T, int C, int dtype,
                              afldm_stream_t stream);
/* The guided update.  eps2: NHWC dtype [2B,H,W,C], rows 0 .. B-1 the UNet's output e, rows B .. 2B-1 the output e_p of the
 * perturbed UNet on the same input.  Step s = *step_idx applies the row coef[12 s .. 12 s + 12) =
 * (p, q, lo, hi, a, b, d, c, s, phi, 0, 0):
 *   g     = e + s (e - e_p)
 *   g     = g (phi sigma(e) / sigma(g) + 1 - phi)       only where phi != 0; sigma: the standard deviation over one sample's
 *                                                       C*H*W elements (diffusers rescale_noise_cfg); the ratio is 1 where
 *                                                       sigma(g) = 0
 *   x0    = clamp(p x + q g, lo, hi)                    lo = -inf, hi = +inf: no clip; a NaN passes through
 *   x_out = a x + b x0 + d g + c z                      z = noise[s * noise_step_stride + i], read only where c != 0
 * One workgroup per sample holds the sample in registers: C*H*W <= 16384 (AFLDM_ESHAPE above that, before any launch).
 * sigma is computed in fp32 in two passes (the mean, then the centred squares), each sum a fixed pairwise tree: no atomics,
 * a sample's bits do not depend on B.  x, x_out: NCHW fp32 [B,C,H,W], x_out may alias x; noise: fp32 rows of [B,C,H,W],
 * noise_step_stride floats apart, drawn by the caller outside any captured graph, or NULL when no row has c != 0;
 * step_idx / advance as afldm_ddim_step. */
int afldm_pag_step(const float* x, const void* eps2, const float* noise, size_t noise_step_stride, float* x_out,
                   const float* coef, int* step_idx, int advance, int B, int C, int H, int W, int dtype,
                   afldm_stream_t stream);
/* Same update on same-layout fp32 tensors of B samples of n contiguous elements each (e and e_p too), the twelve fields of
 * the row by value (the last two are reserved and ignored), for an eager loop.  z may be NULL where c = 0. */
int afldm_pag_step_flat(const float* x, const float* e, const float* e_p, const float* z, float* x_out, float p, float q,
                        float lo, float hi, float a, float b, float d, float c, float s, float phi, float r10, float r11,
                        int B, size_t n, afldm_stream_t stream);
/* ---- Self-attention guidance (Hong et al., ICCV 2023; diffusers StableDiffusionSAGPipeline) ---------------------------
 * The attention mass every KEY of a self-attention receives (diffusers: attn_map.mean(1).sum(1)):
 *   mass[b,j] = (1 / heads) sum_h sum_i softmax_j(scale q[b,i,h,:] . k[b,j,h,:])                    fp32 [B,T]
 * q, k: [B,T,ld] token-major with head h at columns [h*d, (h+1)*d), exactly afldm_attention's self-attention operands (the
 * two column halves of one [B,T,2C] buffer, or contiguous tensors): 16-byte aligned, ldq and ldk multiples of 8 and at least
 * heads*d; dtype bf16 or fp32.  Behind the operand reads everything is fp32: q k^T on MFMA with fp32 accumulation (bf16
 * products are exact there), the softmax with its row maximum subtracted, probabilities never rounded to bf16 and never
 * stored.  Two launches: (max, 1 / sum) of every softmax row into stats_ws, fp32 [B*heads*T*2], 8-byte aligned, which the
 * caller provides and may reuse afterwards; then the column sums on the transposed product.  No atomics and every sum in a
 * fixed order: a sample's bits depend neither on B nor on its place in the batch.
 * afldm_attn_key_mass_ok: 1 for d in {8, 16, 24, 32}, T in {4, 16, 64, 256, 1024}, heads >= 1, B >= 1 with B*heads*T < 2^28;
 * 0 otherwise, and afldm_attn_key_mass itself returns AFLDM_ESHAPE there, and for a scale that is not positive, before any
 * launch. */
int afldm_attn_key_mass_ok(int B, int heads, int T, int d, int dtype);
int afldm_attn_key_mass(const void* q, int ldq, const void* k, int ldk, float* mass, float* stats_ws, int B, int heads, int T,
                        int d, float scale, int dtype, afldm_stream_t stream);
/* The degradation, one launch.  With (p, q) = (1/sqrt(abar_t), -sqrt(1-abar_t)/sqrt(abar_t)), the first two fields of the
 * 12-float row coef[12 s .. 12 s + 12), s = *step_idx (read, never advanced: it is the row the afldm_pag_step behind the
 * second UNet evaluation applies; indexing as afldm_ddim_step):
 *   x0  = p x + q e                                            (fmaf(p, x, q e))
 *   G   = the separable blur with `taps` (ntaps odd, 1 .. 15; a HOST array read during the call and passed to the kernel by
 *         value - a captured graph keeps it): a horizontal then a vertical pass, each sum in ascending tap order in fmaf from
 *         0; boundary 0 = reflect without edge repeat (F.pad mode="reflect", diffusers gaussian_blur_2d), 1 = circular
 *   M   = mass[b][(Y / r) hm + X / r] > 1.0f,  r = H / hm      (nearest up-sampling of the [hm,hm] map; strict; a NaN is false)
 *   x_d = M ? x + (G x0 - x0) / p : x                          (an unmasked element is x, rounded to the output dtype)
 * which is diffusers' add_noise(x0 + M (G x0 - x0), noise = e, t).  x: NCHW fp32 [B,C,H,W]; e: NHWC dtype [B,H,W,C] (the UNet's
 * output); mass: fp32 [B,hm*hm]; x_d: NHWC dtype [B,H,W,C] (the UNet's next input), not aliasing e.  One workgroup per (b, c)
 * plane, the plane twice in LDS.  Before any launch AFLDM_ESHAPE unless H = W, 8 <= H <= 64, C*H*W <= 16384, hm divides H and
 * the half width ntaps / 2 < H.  Plain vector stores only. */
int afldm_sag_degrade(const float* x, const void* e, const float* mass, void* x_d, const float* coef, const int* step_idx,
                      const float* taps, int ntaps, int boundary, int B, int C, int H, int W, int hm, int dtype,
                      afldm_stream_t stream);
/* The same on NCHW fp32 tensors throughout (e and x_d too) with p and q by value, for an eager loop: the same device function
 * in the same arithmetic order - with dtype fp32 the engine form's x_d is this one's, bit for bit, in the other layout. */
int afldm_sag_degrade_flat(const float* x, const float* e, const float* mass, float* x_d, float p, float q, const float* taps,
                           int ntaps, int boundary, int B, int C, int H, int W, int hm, afldm_stream_t stream);
/* ---- MultiDiffusion: one canvas sampled through overlapping windows (Bar-Tal et al., ICML 2023) -------------------
 * A canvas is fp32 NCHW [P,C,Hc,Wc]; its nwin = ny * nx windows of S x S are the batch entries P * nwin + k, k = iy * nx + ix,
 * with corners (oy[iy], ox[ix]).  An axis with wrap != 0 is circular: the window covers (o + u) mod extent, 0 <= o < extent;
 * on the other axes 0 <= o <= extent - S.  oy / ox are HOST arrays, read during the call and passed to the kernel by value
 * (a captured graph keeps them).  Before any launch AFLDM_ESHAPE refuses: more than 16 origins on an axis, S > extent, a
 * window that leaves a non-wrapping axis, and origin lists that leave a coordinate uncovered.  wt: fp32 [S][S], strictly
 * positive window weights (all ones: MultiDiffusion's count average).  Every sum runs over the covering windows in ascending
 * k in fp32 fmaf, gathered per canvas element: no atomics, no workspace, a canvas's bits depend neither on P nor on its
 * place in the batch.
 *
 * The fused update: step s = *step_idx applies the "sde" row coef[8 s .. 8 s + 8) = (p, q, lo, hi, a, b, d, c).  For the canvas
 * element x at (P, ch, Y, X), with (u, v) its position inside covering window k and w = wt[u][v]:
 *   e_k  = eps[P nwin + k][u][v][ch]                        (NHWC dtype [P nwin,S,S,C], the UNet's output on the windows)
 *   x0_k = clamp(p x + q e_k, lo, hi)                       (a NaN passes through)
 *   out  = a x + b (sum_k w x0_k / sum_k w) + d (sum_k w e_k / sum_k w) + c z
 *   canvas_out[P][ch][Y][X] = out;  windows_out[P nwin + k][ch][u][v] = out for every covering k
 * windows_out (NCHW fp32 [P nwin,C,S,S]) is the next UNet input: the crops of canvas_out.  With one window of weight 1 the
 * result is the stochastic update's above, bit for bit.  z = noise[s * noise_step_stride + i], fp32 rows of the canvas's
 * shape drawn by the caller's generator outside any captured graph; it is not read where c = 0, and noise may be NULL when
 * no row has c != 0 (z is then 0).  canvas_out may alias canvas; step_idx / advance as the DDIM update above. */
int afldm_pano_step(const float* canvas, const void* eps, const float* noise, size_t noise_step_stride, const float* wt,
                    float* canvas_out, float* windows_out, const float* coef, int* step_idx, int advance, int P, int C, int Hc,
                    int Wc, int S, const int* oy, int ny, const int* ox, int nx, int wrap_y, int wrap_x, int dtype,
                    afldm_stream_t stream);
/* Outpainting: RePaint (afldm_repaint_step) on a MultiDiffusion canvas, one launch per UNet evaluation.  Arguments as
 * afldm_pano_step, plus known (NCHW fp32 [P,C,Hc,Wc]: the content to keep), mask (fp32 [P,1,Hc,Wc], 1 = keep) and three
 * canvas-shaped noise slots per step as afldm_repaint_step lays them out (z_k, z_u, z_b at noise + s noise_step_stride +
 * {0, 1, 2} noise_slot_stride).  coef float[12 nsteps], the "repaint" row (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0); per
 * canvas element, over the windows k that cover it, in ascending k, every product and sum rounded on its own:
 *   x0_k = clamp(p x + q e_k, lo, hi);  A = sum_k w x0_k;  E = sum_k w e_k;  W = sum_k w
 *   unknown = a A / W + b E / W + c z_u;  knownp = k0 known + k1 z_k
 *   out = u0 (m knownp + (1 - m) unknown) + u1 z_b          (1 - m == 0: the unknown side is left out, not added as 0)
 * canvas_out and windows_out as afldm_pano_step.  A slot whose coefficient (k1, c, u1) is 0 is not read; noise itself must
 * not be NULL.  canvas_out may alias canvas; step_idx / advance as the DDIM update above. */
int afldm_pano_repaint_step(const float* canvas, const void* eps, const float* known, const float* mask, const float* noise,
                            size_t noise_step_stride, size_t noise_slot_stride, const float* wt, float* canvas_out,
                            float* windows_out, const float* coef, int* step_idx, int advance, int P, int C, int Hc, int Wc,
                            int S, const int* oy, int ny, const int* ox, int nx, int wrap_y, int wrap_x, int dtype,
                            afldm_stream_t stream);
/* canvas[P][ch][Y][X] = sum_k w windows[P nwin + k][ch][u][v] / sum_k w: windows NCHW dtype [P nwin,C,S,S], canvas fp32.  S,
 * the origins and the extents are in the caller's units (the pixel-space blend of per-window decodes passes all of them
 * times the VAE's scale factor). */
int afldm_window_fuse(const void* windows, const float* wt, float* canvas, int P, int C, int Hc, int Wc, int S, const int* oy,
                      int ny, const int* ox, int nx, int wrap_y, int wrap_x, int dtype, afldm_stream_t stream);
/* windows[P nwin + k][ch][u][v] = canvas[P][ch][(oy + u) mod Hc][(ox + v) mod Wc], fp32 to fp32, exact. */
int afldm_window_crop(const float* canvas, float* windows, int P, int C, int Hc, int Wc, int S, const int* oy, int ny,
                      const int* ox, int nx, int wrap_y, int wrap_x, afldm_stream_t stream);
/* High-resolution sampling (after DemoFusion, Du et al., CVPR 2024), one launch per UNet evaluation.  The canvas is square,
 * Hc = Wc = scale * S <= 64.  Per canvas the window batch holds NW = nwin + scale^2 windows: the nwin = ny * nx local windows of
 * afldm_pano_step (no wrap), then the dilated ones - window nwin + i scale + j covers the canvas elements (i + scale u,
 * j + scale v).  eps: NHWC dtype [P NW,S,S,C]; windows_out: NCHW fp32 [P NW,C,S,S]; ref, eps_ref: NCHW fp32 [P,C,Hc,Wc], the
 * upsampled base latents and the run's one noise tensor; Lh, Lw: fp32 [Hc][Hc], the low-pass of the dilated views; wt and
 * noise as afldm_pano_step (noise may be NULL when no row has c != 0).  coef float[12 nsteps], the "hires" row
 * (p, q, lo, hi, a, b, c, k0, k1, r, g, f).  For the canvas element x at (P, ch, Y, X), every product and sum rounded on its
 * own, the sums over the covering local windows k in ascending k:
 *   x0_k = clamp(p x + q e_k, lo, hi);  A = sum_k w x0_k;  E = sum_k w e_k;  W = sum_k w
 *   e_g  = eps[P NW + nwin + (Y mod scale) scale + X mod scale][Y div scale][X div scale][ch];  x0_g = clamp(p x + q e_g, lo, hi)
 *   x0m  = (1 - g) A / W + g x0_g;  em = (1 - g) E / W + g e_g          (g == 0: x0m = A / W, em = E / W, e_g is not read)
 *   xp   = a x0m + b em + c z                                           (c == 0: z is not read)
 *   out  = r (k0 ref + k1 eps_ref) + (1 - r) xp                         (r == 0: out = xp, ref and eps_ref are not read)
 *   canvas_out = out;  windows_out[local k] = the crops of out
 *   windows_out[dilated] = the sub-lattices of out + f (Lh out Lw^T - out) per plane   (f == 0: of out; Lh, Lw are not read)
 * One 256-thread workgroup per (P, ch) plane holds it in LDS (three Hc x (Hc | 1) fp32 tiles, under 50 KB); each output of the
 * two passes (Lw first, then Lh) is one ascending-k fmaf chain: no atomics, a plane's bits depend neither on P nor on the grid.
 * canvas_out may alias canvas; oy / ox are host arrays passed on by value; step_idx / advance as the DDIM update above.
 * Before any launch AFLDM_ESHAPE refuses: Hc != Wc, Hc != scale * S, Hc < 2 or Hc > 64, scale < 1, more than 16 origins on
 * an axis, a window that leaves the canvas, an uncovered coordinate. */
int afldm_hires_step(const float* canvas, const void* eps, const float* ref, const float* eps_ref, const float* noise,
                     size_t noise_step_stride, const float* wt, const float* Lh, const float* Lw, float* canvas_out,
                     float* windows_out, const float* coef, int* step_idx, int advance, int P, int C, int Hc, int Wc, int S,
                     const int* oy, int ny, const int* ox, int nx, int scale, int dtype, afldm_stream_t stream);
/* The last two lines of afldm_hires_step alone, for a given canvas and f: the local crops and the dilated views of
 * canvas + f (Lh canvas Lw^T - canvas).  The same device code, so the same bits.  Lh / Lw may be NULL when f == 0. */
int afldm_hires_windows(const float* canvas, const float* Lh, const float* Lw, float f, float* windows_out, int P, int C, int Hc,
                        int Wc, int S, const int* oy, int ny, const int* ox, int nx, int scale, afldm_stream_t stream);
/* tvals[step] -> t_out[0] (device->device), so the timestep also follows step_idx.  pre_advance != 0:
 * step_idx is incremented first (a sampler loop then starts from step_idx = -1 and needs no `advance`
 * launch behind afldm_ddim_step). */
int afldm_select_timestep(const float* tvals, int* step_idx, float* t_out, int pre_advance,
                          afldm_stream_t stream);
/* The same plus a table row: row_out[0 .. row_bytes) = table[step * row_bytes ..] (row_bytes % 16 == 0), one
 * launch.  A sampler knows its timesteps up front, so everything that depends on the timestep only - time_proj ->
 * TimestepEmbedding -> SiLU -> every ResnetBlock2D.time_emb_proj (diffusers UNet2DModel.forward) - is a table with
 * one row per step; the step then starts with this launch instead of seven. */
int afldm_select_step_row(const float* tvals, int* step_idx, float* t_out, int pre_advance, const void* table,
                          void* row_out, size_t row_bytes, afldm_stream_t stream);
/* ---- class conditioning (classifier-free guidance) ---------------------------------------------------------------------
 * diffusers' UNet2DModel adds the class embedding to the time embedding BEFORE the SiLU in front of the time_emb_proj layers,
 * so a class-conditional step has no per-step row to copy: it tabulates time_embedding's output per step and runs
 *   act[r][j] = silu( rnd( emb_table[s][j] + class_rows[r][j] ) ),  s = *step_idx (read only, never advanced)
 * in front of the GEMM over all time_emb_proj layers (afldm_conv2d on act).
 * emb_table  [n][D] dtype: time_embedding's output per step, BEFORE the SiLU
 * class_rows [rows][D], act [rows][D], in dtype; all three 16-byte aligned (AFLDM_EALIGN)
 * rnd = one rounding to dtype: in bf16 this is diffusers' bf16 `emb + class_emb`
 * silu = x sigmoid(x) as afldm_silu evaluates it, the result rounded once: the bits of afldm_silu on the rounded sum
 * D % 8 == 0 (16-byte chunks in bf16), else AFLDM_ESHAPE before any launch
 * s outside [0, n): nothing is read or written (the rule of the slot calls)
 * The kernel only reads step_idx (many workgroups do): afldm_select_timestep in front of it is the one place the counter moves.
 * stream-ordered, capturable, allocates nothing */
int afldm_cond_embed(const void* emb_table, int n, const int* step_idx, const void* class_rows, void* act, int rows, int D,
                     int dtype, afldm_stream_t stream);
/* the same for an eager forward: emb [emb_rows][D] with emb_rows in {1, rows} (1 = broadcast), no step index */
int afldm_cond_embed_flat(const void* emb, int emb_rows, const void* class_rows, void* act, int rows, int D, int dtype,
                          afldm_stream_t stream);

/* ---- slot sampler: a step counter per batch row (continuous batching) ------------------------------------------------
 * Every batch row b of B (a "slot") walks its own stretch [begin, end) of one shared row table of capacity R:
 *   pos[b], end[b]  device int32: the row of the slot's last evaluation (begin - 1 before the first) and one past its last row;
 *                   the slot is ACTIVE in a step iff pos[b] + 1 < end[b]
 *   row_coef [R][4] the "ddim" row (c0, c1, c2, c3);  row_t [R] the timestep (float);  row_temb [R] int32: the row of the
 *                   time-embedding table [T][row_bytes] of that timestep (schedules that share a timestep share the row)
 * The tables' contents may change between replays of a captured graph; their addresses are what the graph holds.  All three
 * calls are stream-ordered, capturable and allocate nothing.  An index read from device memory that falls outside its table
 * makes the slot inactive (select), skips it (step) or skips the command (exchange): nothing is read or written out of range.
 *
 * afldm_slot_select - the step prologue, ONE launch of B workgroups, and the only place a cursor moves.  Active slot:
 *   pos[b] += 1; t_out[b] = row_t[pos[b]]; active[b] = 1; temb_rows[b] <- temb_table[row_temb[pos[b]]] (row_bytes % 16 == 0,
 *   16-byte chunks).  Inactive slot: active[b] = 0 and nothing else - t_out[b] and its row of temb_rows keep their last
 *   contents, so the evaluation of a frozen slot stays finite. */
int afldm_slot_select(const float* row_t, const int* row_temb, int* pos, const int* end, float* t_out, int* active,
                      const void* temb_table, void* temb_rows, int B, int R, int T, size_t row_bytes, afldm_stream_t stream);
/* afldm_slot_step - the update, in place: for every element of a slot with active[b] != 0
 *   x0 = (x - c1 eps) / c0;  x = c2 x0 + c3 eps,  (c0 .. c3) = row_coef[pos[b]]
 * in afldm_ddim_step's float operations and order (a slot gives afldm_ddim_step's bits for the same row).  Elements of an
 * inactive slot are neither read nor written; pos is only read.  x: NCHW fp32 [B,C,H,W]; eps: NHWC dtype. */
int afldm_slot_step(float* x, const void* eps, const float* row_coef, const int* pos, const int* active, int B, int R, int C,
                    int H, int W, int dtype, afldm_stream_t stream);
/* afldm_slot_exchange - between replays, driven by the device command buffer cmd [B][4] = {harvest, refill, begin, end} (int32):
 *   harvest >= 0: out[harvest] <- lat[b];  then refill >= 0: lat[b] <- fresh[refill], pos[b] = begin - 1, end[b] = end
 * (the harvest of an element precedes its refill, in the same thread); {-1, -1, ., .} leaves the slot alone.  lat [B], out
 * [out_rows], fresh [fresh_rows]: fp32 rows of slot_elems floats. */
int afldm_slot_exchange(const int* cmd, float* lat, float* out, const float* fresh, int* pos, int* end, int B, size_t slot_elems,
                        int out_rows, int fresh_rows, afldm_stream_t stream);

/* ---- parallel-in-time sampling: Picard sweeps over a window of steps (ParaDiGMS, Shih et al., NeurIPS 2023) ------------
 * Every image p of P keeps Wn + 1 states X[0 .. Wn], estimates of x_{base[p]} .. x_{base[p] + Wn} of ONE "ddim" schedule of n
 * rows; X[0] is exact.  x: fp32 [Wn + 1][P][C][H][W] (state-major: rows 0 .. Wn - 1 are the NCHW batch [Wn P] the UNet
 * evaluates, UNet row j P + p); y: fp32 [Wn][P][C][H][W], row j holds Y[j + 1]; eps: NHWC dtype [Wn P][H][W][C].
 *   base[p], iter[p]  device int32: the schedule row X[0] stands at (0 .. n, n = finished) and the iterations seen so far
 *   row_coef [n][4], row_t [n], row_temb [n], temb_table [T][row_bytes]   the slot sampler's row table (above)
 * One iteration is the UNet evaluation and then the three calls below, in this order.  All are stream-ordered, capturable and
 * allocate nothing; they hold no atomics, and what they compute for an image depends neither on P nor on p.  An index read from
 * device memory that falls outside its table skips what it indexes: nothing is read or written out of range.  A finished
 * image is skipped by all three: of its states, errors, timesteps and time-embedding rows nothing is written.
 *
 * afldm_picard_blocks - the blocks B of a sweep per image, from the shape alone: ceil(C H W / (256 V)), V = 4 where
 *   H W % 4 == 0 (then x and y must be 16-byte aligned: AFLDM_EALIGN otherwise), else 1.  partial is fp32 [P][Wn][B].
 * afldm_picard_sweep - Y[0] = X[0]; for j = 0 .. Wn - 1 with r = base[p] + j:
 *     r < n:   Y[j + 1] = c2 x0 + c3 e_j,  x0 = (Y[j] - c1 e_j) / c0,  (c0 .. c3) = row_coef[r], in afldm_ddim_step's float
 *              operations and order (a swept row has afldm_ddim_step's bits for the same operands)
 *     r >= n:  Y[j + 1] = Y[j]
 *   and partial[p][j][b] = block b's sum of (Y[j + 1] - X[j + 1])^2 (0 for r >= n), summed in a fixed order.  Reads base only.
 * afldm_picard_stride - ONE workgroup per image, and the only place base[p] moves:
 *     err[p][j] = (sum_b partial[p][j][b], b ascending) / (C H W);  s = min({j + 1 : err[p][j] > tol2} U {Wn}, n - base[p]);
 *     stride[p] = s;  base[p] += s;  log[iter[p]][p] = s (iter[p] < log_cap);  iter[p] += 1
 *   (a finished image: s = 0), then, where s > 0, the gather for the next evaluation: for j = 0 .. Wn - 1 with r = base[p] + j
 *   < n: t_out[j P + p] = row_t[r], active[j P + p] = 1, temb_rows[j P + p] <- temb_table[row_temb[r]] (row_bytes % 16 == 0);
 *   r >= n: active[j P + p] = 0 and nothing else, so the row is evaluated with what it last held.  gather_only != 0: no
 *   decision and no advance, only the gather for the cursors as they stand (before the first evaluation of a run).
 * afldm_picard_slide - X[j] = Y[min(j + stride[p], Wn)], j = 0 .. Wn; stride[p] outside 1 .. Wn: the image is left alone. */
int afldm_picard_blocks(int C, int H, int W);
int afldm_picard_sweep(const float* x, const void* eps, float* y, float* partial, const float* row_coef, const int* base, int P,
                       int Wn, int n, int C, int H, int W, int dtype, afldm_stream_t stream);
int afldm_picard_stride(const float* partial, int* base, int* iter, int* stride, float* err, int* log, int log_cap,
                        const float* row_t, const int* row_temb, float* t_out, int* active, const void* temb_table,
                        void* temb_rows, float tol2, int gather_only, int P, int Wn, int n, int C, int H, int W, int T,
                        size_t row_bytes, afldm_stream_t stream);
int afldm_picard_slide(float* x, const float* y, const int* stride, int P, int Wn, int C, int H, int W, afldm_stream_t stream);

/* ---- masked equivariance metrics (shift_utils/metrics.py:5-20) ------------------------------
 * One pass over a, b [B][n] (dtype) and mask [B][n] fp32: out[b] = { sum ((a - b) mask)^2, sum mask,
 * max(a mask), min(a mask), max(b mask), min(b mask) } (fp32 [B][6]).  mask_mse = mean_b out[b][0] / out[b][1];
 * mask_psnr = 10 log10(range^2 / mask_mse) with range = max over both - min over both. */
int afldm_masked_metrics(const void* a, const void* b, const float* mask, float* out, int B, size_t n,
                         int dtype, afldm_stream_t stream);

/* ---- warping along an optical-flow field (afldm/shift_utils/flow_utils.py, flow_utils_np.py) ---------------
 * afldm_flow_splat: the forward bilinear splat of `_forward_flow_warp` (flow_utils_np.py:116-152) and what the callers do
 * behind it, for B samples in one call.  x [Bs][C][H][W] dtype and flow [Bs][2][H][W] fp32 (channel 0 = ROW displacement)
 * are shared by groups of B / Bs samples (sample b reads source b / (B / Bs)); scale [B] fp32 on the DEVICE is the factor the
 * reference multiplies the flow by before the warp (`f_flow * alpha`, image_interpolation_pipeline.py:571-577).  Source
 * (i, j) lands at ci = i + scale * flow0, cj = j + scale * flow1 (fp32, product rounded before the add), i1 = int(ci)
 * truncated towards zero, and each of the targets (i1 | i1 + 1, j1 | j1 + 1) inside the plane receives
 * coef = (1 - |ci - gi|)(1 - |cj - gj|) (negative for some targets when ci or cj < 0): res += x * coef, cnt += coef, in fp32
 * (return-less vector atomics: sums agree between runs to summation order, not bit for bit).  bwd_occ = 1 where cnt > 0 is
 * false; no division by cnt.
 *   mode AFLDM_FLOW_PICK: only targets with gi % ds == 0 and gj % ds == 0 are accumulated: out [B][C][H/ds][W/ds], occ
 *     [B][1][H/ds][W/ds] (NULL: not written) are the reference's `[:, :, ::ds, ::ds]` of the warp (flow_utils.py:333-341).
 *     fill != NULL applies `res * (1 - occ) + occ * fill` (image_interpolation_pipeline.py:574); fill is read at
 *     [b * fill_batch_stride + c * (H/ds * W/ds * fps^2) + (ho * fps) * (W/ds * fps) + wo * fps] with fps = fill_pix_stride
 *     (a full-resolution draw is read in place at the kept pixels with fps = ds; fill_batch_stride = 0 shares one draw).
 *   mode AFLDM_FLOW_POOL: accumulated at full resolution, out [B][C][H/ds][W/ds] = sum over each ds x ds block of
 *     (fill * occ + res * (1 - occ)) / ds (`collect_noise_pixel`, flow_utils.py:214-221; fill [.][C][H][W], NULL = 0),
 *     occ [B][1][H][W] (NULL: not written).
 * workspace: afldm_flow_splat_workspace(...) bytes (0 = bad arguments), zeroed by the call itself (a kernel: a
 * captured call replays kernel nodes only).  x, fill, out, occ share `dtype`. */
enum { AFLDM_FLOW_PICK = 0, AFLDM_FLOW_POOL = 1 };
size_t afldm_flow_splat_workspace(int B, int C, int H, int W, int ds, int mode);
int afldm_flow_splat(const void* x, const float* flow, const float* scale, const void* fill, long long fill_batch_stride,
                     int fill_pix_stride, void* out, void* occ, float* workspace, size_t workspace_bytes, int B, int Bs, int C,
                     int H, int W, int ds, int mode, int dtype, afldm_stream_t stream);
/* afldm_flow_warp: `flow_warp` / `bilinear_sample` (flow_utils.py:53-86): F.grid_sample(align_corners=True,
 * padding_mode='zeros'), bilinear (nearest = 0) or nearest (round half to even), of x [B][C][Hin][Win] dtype at
 * add_grid != 0: x = j + flow[1], y = i + flow[0] (coords_grid + flip(flow): flow [B][2][Hout][Wout] fp32, channel 0 = row
 * displacement); add_grid == 0: flow holds the sample coordinates themselves (channel 0 = x).  y [B][C][Hout][Wout];
 * mask (NULL: not written) [B][Hout][Wout] bytes = the reference's in-bounds mask, formed from the coordinate normalised to
 * [-1, 1] with its fp32 operations (2 c / (n - 1) - 1), so exact at the borders.  With Hin == Hout (Win == Wout) the pixel
 * coordinate is used as it is instead of the normalised one un-normalised again (the same to 4 (n - 1) 2^-24 pixels).
 * Coordinates are fp32 for both dtypes. */
int afldm_flow_warp(const void* x, const float* flow, void* y, unsigned char* mask, int B, int C, int Hin, int Win, int Hout,
                    int Wout, int add_grid, int nearest, int dtype, afldm_stream_t stream);

/* ---- optical-flow estimation: dense pyramidal Lucas-Kanade ---------------------------
 * Not a port: the reference estimates flow with GMFlow, a trained network.  This is a classical, deterministic estimator
 * defined by this project (tests/flowest_oracle.py is its float64 statement).  All planes are fp32 except the input of
 * afldm_flowest_pyr_down; flows are [B][2][H][W] with channel 0 = ROW displacement; every border is a replicate border
 * (indices clamped into the plane); no atomics: two runs agree bit for bit.  Every call is stream-ordered, allocates
 * nothing and may be captured.
 * afldm_flowest_pyr_down: x [n][H][W] dtype -> y fp32.  factor 2: y [n][H/2][W/2], [1, 3, 3, 1] / 8 along the columns, then
 *   along the rows, decimated by 2: output (i, j) reads rows 2i-1 .. 2i+2 and columns 2j-1 .. 2j+2 (H, W even).
 *   factor 1: y [n][H][W] = x converted to fp32 (level 0 of the pyramid).
 * afldm_flowest_up2: y [n][2h][2w] = 2 * bilinear(u [n][h][w]) at the source coordinate (i + 0.5) / 2 - 0.5 clamped to
 *   [0, h - 1] (half-pixel centres): a flow carried to the next finer level.
 * afldm_flowest_lk_step: one update of u_in [B][2][H][W] for the pair I1, I2 [B][C][H][W], C <= 4, in one launch:
 *   I2w(p) = bilinear(I2, clamp(p + u_in(p))); g = (grad I1 + grad I2w) / 2 (central differences); It = I2w - I1; the
 *   products gy gy, gy gx, gx gx, gy It, gx It summed over the channels and averaged over the (2 radius + 1)^2 window
 *   (1 <= radius <= 4) to a, b, c, p, q; du = -[[a + lam, b], [b, c + lam]]^-1 [p, q] (closed form, lam > 0);
 *   u_out = u_in + du min(1, 1 / |du|).  u_out must not be u_in.  tile: the side of a workgroup's output tile, 16 or 32,
 *   or 0 to let the call choose (32 when that still gives 512 workgroups, else 16); the result does not depend on it.
 * afldm_flowest_smooth: y = [1, 4, 6, 4, 1] / 16 along the columns, then along the rows, of u [n][H][W]; y must not be u. */
int afldm_flowest_pyr_down(const void* x, float* y, int n, int H, int W, int factor, int dtype, afldm_stream_t stream);
int afldm_flowest_up2(const float* u, float* y, int n, int h, int w, afldm_stream_t stream);
int afldm_flowest_lk_step(const float* I1, const float* I2, const float* u_in, float* u_out, int B, int C, int H, int W,
                          int radius, float lam, int tile, afldm_stream_t stream);
int afldm_flowest_smooth(const float* u, float* y, int n, int H, int W, afldm_stream_t stream);

/* ---- upfirdn2d ---------------------------------------------------------------------------
 * Zero-stuffing up-sample (upx, upy) -> pad (negative = crop) -> 2-D FIR -> decimate (downx, downy) on
 * NCHW planes: torch_utils/ops/upfirdn2d.py:140-194 (`_upfirdn2d_ref`; the reference's fast path is the
 * vendored upfirdn2d.cu plugin).  x [planes][H][W], f [fh][fw] DEVICE fp32 taps, y [planes][outH][outW],
 * outW = (W*upx + padx0 + padx1 - fw) / downx + 1 (same for H).  flip_filter = 0 is a true convolution
 * (the filter is flipped), 1 a correlation; every tap is scaled by `gain` (the reference scales a 2-D
 * filter by gain and each pass of a separable one by sqrt(gain): callers pass the per-call factor).
 * Serves equivariance.py:68-103 (Lanczos fractional translation), shifters.py:158-161, :292-365. */
int afldm_upfirdn2d(const void* x, const float* f, void* y, int planes, int H, int W, int fh, int fw,
                    int upx, int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1,
                    int flip_filter, float gain, int dtype, afldm_stream_t stream);
/* Output extent along one axis for the arguments above, -1 when the plane is smaller than the filter. */
int afldm_upfirdn2d_out_size(int in, int up, int down, int pad0, int pad1, int ftaps);

/* ---- box calibration probes (measurement only: bench.py's `box` record) --------------------------------
 * afldm_probe_mfma: `workgroups` x 4 waves, each issuing iters x 4 independent v_mfma_f32_32x32x16_bf16
 * (flops = workgroups * 4 * iters * 4 * 32768); out [workgroups * 256] fp32 is never written.
 * afldm_probe_copy: 16-byte-per-lane grid-stride copy of `bytes` (a multiple of 16) device -> device.
 * Neither replaces a reference computation: they fingerprint the box (MFMA clock under load, HBM copy rate)
 * so that cross-box numbers can be normalised. */
int afldm_probe_mfma(float* out, int workgroups, int iters, afldm_stream_t stream);
/* the same loop on operands of random bf16 bit patterns rotating through four register sets (iters % 4 == 0): the
 * sustained MFMA rate of the chip is data-dependent (power): ~1.6 PFLOP/s here against ~2.4 on the near-constant
 * operands of afldm_probe_mfma. */
int afldm_probe_mfma_random(float* out, int workgroups, int iters, afldm_stream_t stream);
int afldm_probe_copy(const void* src, void* dst, size_t bytes, afldm_stream_t stream);
/* latency side of the fingerprint (round 4): afldm_probe_chase walks `steps` dependent loads through `buf` (uint32 indices
 * forming one cycle, built by the host with a stride beyond a cache line; nontemporal loads) on one lane and writes
 * out[0] = last index, out[1] = elapsed shader-clock ticks; afldm_probe_empty launches `workgroups` x 64 threads that do
 * nothing (captured N times into a graph: the kernel-to-kernel boundary of this box). */
int afldm_probe_chase(const void* buf, void* out, int steps, afldm_stream_t stream);
int afldm_probe_empty(int workgroups, afldm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AFLDM_HIP_H */
