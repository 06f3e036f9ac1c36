/*
 * villan_hip.h -- C ABI of the MI355X (gfx950) backdoored-diffusion hot path.
 *
 * The reference (IBM/VillanDiffusion) has no FFI: its hot path is Python calling
 * torch/cuDNN through an un-vendored diffusers fork.  This header is therefore the
 * boundary *below* the reference's Python surface (last row): each
 * entry point replaces the torch op sequence named in its comment (reference
 * file:line of the call site that triggers it).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory (fp32 unless
 *     stated), owned by the caller, 16-byte aligned;
 *   - image tensors are NCHW with contiguous CHW and an explicit batch stride
 *     ("bstride", in elements) so channel-slices of a wider buffer can be passed
 *     without a copy (zero-copy skip concatenation);
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*), never
 *     synchronise, allocate nothing; thread-safe w.r.t. distinct streams;
 *   - return 0 on success, otherwise a hipError_t / negative VD_E* code;
 *     vd_last_error() gives a message.  Nothing throws.
 */
#ifndef VILLAN_HIP_H
#define VILLAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VD_ABI_VERSION 12 /* 12: vd_gemm_kernel_name / vd_conv_wgrad_kernel_name / vd_conv_wgrad_group_kernel_name; a refused pool2 problem answers -1 at vd_gemm_tile.  Unchanged by vd_removal_loss / vd_image_set_stats / vd_score_inv_objective / vd_pyramid_dgrad / vd_image_set_merge / vd_adam_ema_step / vd_swap / vd_neuron_scale / vd_neuron_grad / vd_neuron_step / vd_lora_merge / vd_lora_grad / vd_lora_act_grad / vd_lora_act_grad_ws_floats / vd_loss_sample_fwd_bwd / vd_loss_sample_ws_floats / vd_loss_sample_plan: additions only */
#define VD_EINVAL (-22)
#define VD_ETIMEDOUT (-110) /* an EARLIER asynchronous launch reported a bounded-poll timeout (see vd_async_errors) */

int vd_abi_version(void);
const char* vd_last_error(void);
/* 0 when a gfx950-capable device is visible to this process. */
int vd_device_ok(void);
/* Errors that kernels report asynchronously through a word of pinned host memory (today: poll timeouts of the one-launch chunked
 * GroupNorm, whose statistics are then NaN).  Returns the count since the last clear without synchronising; while it is non-zero every
 * vd_groupnorm_* call fails with VD_ETIMEDOUT (sticky).  clear != 0 resets it. */
int vd_async_errors(int clear);

/* ------------------------------------------------------------------------------------------
 * K2/K4/K5/K6/K7 -- implicit-GEMM on the f32-input MFMA (v_mfma_f32_32x32x2_f32, exact f32).
 *   D[b][m][p] = alpha * sum_k A[m][k] * Bop[k][(b,p)]  (+bias +rowadd +residual)
 * Replaces F.conv2d / F.linear / torch.bmm inside UNet2DModel (reached via loss.py:993 and
 * the pipeline call VillanDiffusion.py:579, model.py:519).
 * ------------------------------------------------------------------------------------------ */
enum vd_a_mode { VD_A_ROW = 0,      /* A[m*lda + k]  (k contiguous: conv/linear weights)      */
                 VD_A_COL = 1 };    /* A[k*lda + m]  (m contiguous)                            */
enum vd_b_mode { VD_B_PLAIN = 0,    /* B[b*bs + k*ldb + p]   (1x1 conv, plain matrices)        */
                 VD_B_KCONTIG = 1,  /* B[b*bs + p*ldb + k]                                     */
                 VD_B_CONV3 = 2,    /* 3x3 pad 1 gather, k = c*9 + r*3 + s                     */
                 VD_B_CONV3_T = 3,  /* 3x3 pad 1 with flipped taps (stride-1 dgrad)            */
                 VD_B_CONV3_S2 = 4, /* pad (0,1,0,1) + 3x3 stride 2 (Downsample2D)             */
                 VD_B_CONV3_UP = 5, /* nearest x2 folded into the 3x3 pad 1 gather (Upsample2D) */
                 VD_B_CONV3_DIL = 6,/* dgrad of CONV3_S2 (zero-dilated gather)                 */
                 VD_B_CONVG = 7     /* general kh x kw convolution, stride conv_stride, zero padding (pad_h, pad_w),
                                       k = (c*kh + r)*kw + s: the InceptionV3 convolutions of the FID measure
                                       (1x7 / 7x1 / 5x5 / 3x3 stride 2; reference fid_score.py:91-148 -> pytorch-fid) */ };

typedef struct vd_gemm_desc {
    const float* A;
    const float* B;
    float* D;
    const float* bias;       /* [M] (or [N] when bias_on_n), nullable                           */
    const float* rowadd;     /* rowadd[b*rowadd_bstride + m] broadcast over p (temb), nullable  */
    const float* residual;   /* residual[b*res_bstride + m*ldd + p], nullable                   */
    int32_t M, N, K;         /* N = nb * NP                                                     */
    int32_t a_mode, b_mode;
    int32_t NP;              /* columns per batch item (OH*OW for conv)                         */
    int32_t C, H, W;         /* conv source dims (per batch item)                               */
    int32_t OH, OW;          /* conv output dims                                                */
    int32_t bias_on_n;
    int32_t d_trans;         /* 1: D[n*ldd + m] (n-major store)                                 */
    int32_t accumulate;      /* 1: D += result                                                  */
    int32_t tile;            /* 0 auto, 1: 128x128, 2: 64x128, 3: 64x64                         */
    int32_t debug;           /* MUST be 0: the release library fails with VD_EINVAL otherwise (ABI 11).  Only a diagnostic
                                `make ABLATION=1` build honours timing-only ablation bits here (results invalid): 1 = no
                                global loads after the first K-step, 2 = no epilogue, 4 = no MFMA, 8 = no LDS stores      */
    float alpha;
    int64_t lda, a_bstride;  /* a_bstride != 0: per-batch A (requires tile_n | NP)              */
    int64_t ldb, b_bstride;
    int64_t ldd, d_bstride;
    int64_t res_bstride, rowadd_bstride;
    float* ws;               /* split-K workspace (vd_gemm_ws_floats() floats), nullable when that is 0        */
    int32_t pad;             /* VD_B_CONV3_S2 only: 0 = zero pad (0,1,0,1) (Downsample2D padding=0, the DDPM UNets),
                                1 = symmetric padding 1 (Downsample2D padding=1, the LDM / NCSN++ UNets)        */
    int32_t nb2;             /* > 1: two-level batch, item i = outer*nb2 + inner at outer*X_bstride + inner*X_b2stride
                                (the heads of multi-head attention are channel slices of one q/k/v tensor); needs
                                rowadd == residual == NULL                                                       */
    int64_t a_b2stride, b_b2stride, d_b2stride;
    const float* gn_ss;      /* VD_B_CONV3 only, nullable: per-(batch item, input channel) GroupNorm scale / shift pairs
                                [nb][C][2] from vd_groupnorm_stats; the convolution then reads silu(x*scale + shift) instead
                                of x (GroupNorm + SiLU folded into the patch loader: inference path, nothing is saved).
                                Needs the patch-staged kernel (OW >= 16, C % 8 == 0, C <= 1024, M >= 64)              */
    const void* a_packed;    /* nullable.  3x3 convolutions (VD_B_CONV3 / _T at 4x4 ... 32x32, _UP at 8x8 ... 32x32, any of them on 64-wide or
                                128k-wide outputs; C % 16 == 0,
                                M >= 64) and VD_B_PLAIN products with a shared A (1x1 convolutions: NP % 128 == 0 or 128 % NP == 0, N % 128 == 0, K % 16 == 0,
                                M >= 64) only: the weights pre-split into bf16 (hi, lo) pairs by vd_conv3_pack_weights.  The
                                contraction then runs as three bf16 MFMAs per product term (hi*hi + hi*lo + lo*hi, f32
                                accumulation; ~1e-5 relative to the exact-f32 kernel) instead of on the f32 MFMA.  A is still
                                required (shape checks) but not read.  Problems outside that set fail with VD_EINVAL.   */
    int32_t a_packed_mpad;   /* row count the packed operand was built with (M rounded up to 128)                      */
    int32_t math;            /* 2: a_packed holds f16 operands (vd_conv3_pack_weights_f16_multi): ONE f16 MFMA per product term, f32 accumulation
                                (~2e-4 relative per contraction) -- only problems the persistent 16x16x32 kernels take (vd_gemm_tile() 18 / 19),
                                else VD_EINVAL.
                                3: opt-in bf16 mixed precision: a_packed is the split-precision operand (vd_conv3_pack_weights), and ONE bf16 MFMA
                                per product term multiplies its hi plane with the hi part of B (f32 B rounded to nearest even, a pre-split B's hi
                                units, or the folded GroupNorm loader's bf16(silu(gn(x)))), f32 accumulation: the exact sum of bf16-rounded
                                operands up to summation order.  Only problems of vd_gemm_tile() 18 / 19 / 20 (3x3 forward, flipped-tap input
                                gradient, Upsample2D, gn_ss / act_out / gn_part / b_presplit as for math 0; 1x1 products); else VD_EINVAL.
                                0: exact f32 MFMA (or a_packed).  1: split-precision product of two ACTIVATION matrices (attention
                                scores / values and their gradients): per-batch A (a_bstride != 0), VD_B_PLAIN or VD_B_KCONTIG,
                                NP % 128 == 0, K % 16 == 0, K >= 32, M >= 64, 16-byte aligned operands and strides; both operands
                                are split into bf16 (hi, lo) inside the kernel.  Anything else fails with VD_EINVAL.           */
    int32_t pool2;           /* 1: VD_B_CONV3_T with a_packed at 16x16 / 32x32 outputs only (the input gradient of an Upsample2D convolution):
                                the epilogue adds each 2x2 block of output pixels and writes D at HALF resolution (ldd = (OH/2)*(OW/2)),
                                i.e. conv-transpose followed by the adjoint of the nearest-2x upsample, without the full-resolution tensor.
                                Needs an unsplit grid (ceil(M/128) * ceil(N/128) >= 256 tiles), no bias / rowadd / residual / accumulate; the
                                persistent kernel (vd_gemm_tile() == 18) also takes it on the wider images it walks.  Else vd_gemm_tile()
                                answers -1 and vd_gemm VD_EINVAL */
    int32_t kh, kw;          /* VD_B_CONVG only: kernel height / width (K = C*kh*kw)                                    */
    int32_t conv_stride;     /* VD_B_CONVG only: 1 .. 4 (both directions)                                               */
    int32_t pad_h, pad_w;    /* VD_B_CONVG only: zero padding on each side                                              */
    int32_t act;             /* 0: none; 1: D = max(D, 0) after every other epilogue term (BasicConv2d = conv + folded BatchNorm + ReLU).
                                Honoured by the exact-f32 gather / plain kernels only (a_packed == NULL, math == 0); else VD_EINVAL */
    float* gn_part;          /* optional OUTPUT of the persistent 16x16x32 3x3 convolution (vd_gemm_tile() == 18, else VD_EINVAL):
                                [B][NP / 256][M][2] = (sum, sum of squares) of the FINAL result (after bias / rowadd / residual) of channel m
                                over each 256-pixel tile -- the GroupNorm that follows (ResnetBlock2D: conv1 -> norm2) gets its statistics
                                from vd_groupnorm_stats_from_partials() instead of a read of the whole tensor.  Fixed-order sums.           */
    float* act_out;          /* optional OUTPUT of the persistent 16x16x32 3x3 convolution with gn_ss (vd_gemm_tile() == 18, else VD_EINVAL): the
                                normalised activation silu(x * scale + shift) the loader computes anyway, written once per element
                                ([nb][C][H][W], batch stride act_bstride) by the workgroups of the first channel tile.  The TRAINING forward
                                saves it for the weight gradient instead of running a separate GroupNorm + SiLU pass (round 4).           */
    int64_t act_bstride;
    int32_t b_presplit;      /* ABI 11.  1: B is a PRE-SPLIT image (vd_presplit_* below: bf16 (hi, lo) pairs, 8 channels of a pixel per 16-byte
                                unit) instead of f32 NCHW -- same bytes, same batch stride, same channel-octet offsets.  Only the persistent
                                16x16x32 convolution (vd_gemm_tile() == 18) with a_packed, math 0, VD_B_CONV3 / VD_B_CONV3_T and no gn_ss takes
                                it: the patch loader then moves (hi, lo) units without converting.  Anything else: VD_EINVAL.      */
    int32_t reserved_;
} vd_gemm_desc;

int vd_gemm(const vd_gemm_desc* desc, void* stream);
/* Floats of split-K workspace vd_gemm needs for this problem (0 for most shapes; the patch-staged convolution splits
 * its channel loop over workgroups for the 8x8 / 4x4 layers, partial slabs are reduced in fixed order). */
int64_t vd_gemm_ws_floats(const vd_gemm_desc* desc);
/* Kernel vd_gemm will use for this problem: 1: 128x128, 2: 64x128, 3: 64x64 gather tiles, 4 / 6: patch-staged 3x3
 * convolution kernel with 128x128 / 128x256 tiles, 5: plain GEMM kernel, 7: direct 3x3 convolution for <= 4 output
 * channels (VD_B_CONV3, and VD_B_CONV3_T without a_packed: the input gradient of a convolution with <= 4 INPUT channels, A being the
 * [C_in][C_out * 9] transposed copy of vd_weight_transpose, W % 4 == 0, C >= 16, 16-byte aligned B / D and strides), 8 / 9 / 10: split-precision bf16 3x3 convolution / plain product (a_packed) / activation product (math = 1), 11: the persistent
 * variant of 9 (grids of >= 1024 tiles), 12 / 15 / 16: the 128 x 256 / 128 x 512 / split 128 x 256 tiles of 8, 13: the 128 x 256 tile of 9,
 * 18: the persistent 16x16x32-MFMA 3x3 convolution (32-channel K-steps, 128 x 256 tiles, LDS-DMA weight stages, 8 x 32 pixel
 * segments of images of any size), 19: the persistent 16x16x32 kernel for 9's problems, 20 (round 6): the whole-K 16x16x32 kernel of the 8x8 level
 * (and of 4x4 grids that fill the chip): 64 channels x 2 | 4 whole images per workgroup, no split-K workspace, f32 input, VD_B_CONV3 / VD_B_CONV3_T,
 * bias / rowadd / residual / accumulate; its sums run over all channels in one chain, so it agrees with the split kernels (8 / 16) to the path's
 * tolerance, not bit for bit, -1: a_packed given for an unsupported problem (profiling / tests). */
int vd_gemm_tile(const vd_gemm_desc* desc);
/* Host-only query (launches nothing, makes no HIP call, needs no device and no workspace): returns vd_gemm_tile(desc) and writes the name of the
 * kernel vd_gemm would launch -- the instantiation as the profiler prints it, written by the very branch that launches it ("conv3_bx3_kernel<32, 1,
 * 2, 512, 2>"; the exact-f32 gather kernels as "gemm_kernel<128x128,ROW,CONV3_S2>"; the persistent 3x3 kernel on images wider than 32 pixels with
 * the image width behind it: "conv3_k32p_kernel<32, 0, true, true, false, false>@64").  Where vd_gemm refuses the descriptor: VD_EINVAL, empty name. */
int vd_gemm_kernel_name(const vd_gemm_desc* desc, char* name, int name_len);

/* Weight gradient of a 3x3 / 1x1 convolution (K2/K5/K6/K7 backward, deterministic split-K):
 *   dW[m][c*T + t] (+)= sum_{b,p} dY[b][m][p] * gather(X)[b][c][p (+) t]
 * mode in {VD_B_PLAIN (1x1), VD_B_CONV3, VD_B_CONV3_S2, VD_B_CONV3_UP}.
 * ws must hold splits*M*C*T floats when splits > 1.  Replaces autograd's conv2d weight grad. */
typedef struct vd_wgrad_desc {
    const float* dY;
    const float* X;
    float* dW;
    float* ws;
    int32_t M, C, T;          /* T = 9 or 1                                                     */
    int32_t nb, NP;           /* batch, output pixels per item (OH*OW)                          */
    int32_t H, W, OH, OW;     /* X spatial dims, dY spatial dims                                */
    int32_t mode, splits, accumulate, tile;
    int64_t dy_bstride, x_bstride;
    int32_t pad;              /* VD_B_CONV3_S2 only, as in vd_gemm_desc                         */
    int32_t math;             /* 0: exact f32 MFMA.  1: split-precision bf16 MFMA (hi*hi + hi*lo + lo*hi, f32 accumulation,
                                 ~1e-5 relative): VD_B_CONV3 / VD_B_CONV3_UP with 8x8 / 16x16 / 32x32 outputs, either of them on images whose
                                 width is a multiple of 32 from 64 up, VD_B_CONV3 at 4x4, or VD_B_PLAIN (1x1) with
                                 NP % 8 == 0; M >= 64, C >= 64; otherwise VD_EINVAL.
                                 3: opt-in bf16 mixed precision, GROUPED launches only: one bf16 MFMA (hi(dY) * hi(X)) per product term, f32
                                 accumulation, for the math = 1 problems whose class runs on the pre-split, 16x16x32 or wide 1x1 kernel
                                 (vd_conv_wgrad_group_class() > 10000: a class of its own, never mixed with math = 1 jobs); vd_conv_wgrad: VD_EINVAL */
    int32_t presplit;         /* ABI 11, math == 1 only.  Bit 0: X, bit 1: dY is a PRE-SPLIT image (vd_presplit_* below) instead of f32 NCHW.
                                 3 (both): the kernel fetches both operands by LDS-DMA and reads them through ds_read_b64_tr_b16 -- no
                                 conversion, no staging registers (VD_B_CONV3 / VD_B_CONV3_UP at 8x8 / 16x16 / 32x32 outputs, M % 8 == C % 8 == 0,
                                 grouped launches only).  Any other non-zero value, or a problem outside that set: VD_EINVAL.               */
    int32_t reserved_;
} vd_wgrad_desc;

int vd_conv_wgrad(const vd_wgrad_desc* desc, void* stream);
/* Floats of workspace vd_conv_wgrad will use for this problem (0 = no split-K chosen). */
int64_t vd_conv_wgrad_ws_floats(const vd_wgrad_desc* desc);
/* Tile and split count vd_conv_wgrad will use (profiling / tests). */
int vd_conv_wgrad_plan(const vd_wgrad_desc* desc, int* tile, int* splits);
/* Host-only query as vd_gemm_kernel_name: returns the tile of vd_conv_wgrad_plan and writes the kernel vd_conv_wgrad would launch, with the reduction
 * that follows it in brackets ("wgrad_k32_kernel<16, 2>(+slab_reduce)", "wgrad_small_kernel<true>(+colsum)"); VD_EINVAL and an empty name where
 * vd_conv_wgrad refuses the descriptor. */
int vd_conv_wgrad_kernel_name(const vd_wgrad_desc* desc, char* name, int name_len);

/* ------------------------------------------------------------------------------------------
 * PRE-SPLIT activation images (round 5, ABI 11) -- csrc/vd_presplit.hip.
 * The split-precision kernels contract f32 operands as bf16 (hi, lo) pairs; a pre-split image holds those pairs as its PRODUCER
 * wrote them, so that no consumer converts: unit (o, p, part) = 16 bytes = channels 8o .. 8o+7 of pixel p as bf16 (part 0 = hi =
 * bf16(x), part 1 = lo = bf16(x - hi)) at byte ((o * HW + p) * 2 + part) * 16 of the image.  Same bytes, batch stride and
 * channel-octet offsets as the f32 [C][HW] image it replaces; C % 8 == 0.  Consumers: vd_gemm_desc.b_presplit (3x3 convolution
 * forward / input gradient), vd_wgrad_desc.presplit (grouped 3x3 weight gradient: LDS-DMA + transposed LDS reads).
 * Replaces the F.group_norm + F.silu -> F.conv2d hand-over inside diffusers ResnetBlock2D (reference loss.py:993).
 * ------------------------------------------------------------------------------------------ */
/* f32 NCHW -> pre-split image and back (x = hi + lo: 16 significant bits); strides in floats. */
int vd_presplit_pack(const float* x, void* y, int B, int C, int HW, int64_t x_bstride, int64_t y_bstride, void* stream);
int vd_presplit_unpack(const void* y, float* x, int B, int C, int HW, int64_t y_bstride, int64_t x_bstride, void* stream);
/* GroupNorm (+ SiLU) forward whose output IS the pre-split image (one read of x, one write of the pairs; mean / rstd as
 * vd_groupnorm_fwd).  _ok: 1 when a kernel exists for (C, HW, G) -- the 16x16 / 32x32 levels with 4 .. 16 channels per group. */
int vd_groupnorm_fwd_presplit_ok(int C, int HW, int G);
int vd_groupnorm_fwd_presplit(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int B, int C, int HW, int G,
                              float eps, int apply_silu, int64_t x_bstride, int64_t y_bstride, void* stream);
/* GroupNorm (+ SiLU) backward (same shapes) as vd_groupnorm_bwd_fused -- dgamma_ws / dbeta_ws rows per (image, channel), residual gradients extra /
 * extra2 added into dx, rowsum[b][c] = sum_p dx -- with dx written as f32 (dx), as the pre-split image (dx_ps: the operand of the producing
 * convolution's input AND weight gradient), or both; at least one of the two must be given. */
int vd_groupnorm_bwd_presplit(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                              const float* extra, const float* extra2, float* dx, void* dx_ps, float* dgamma_ws, float* dbeta_ws, float* rowsum,
                              int B, int C, int HW, int G, int apply_silu, int64_t dy_bstride, int64_t x_bstride, int64_t extra_bstride,
                              int64_t extra2_bstride, int64_t dx_bstride, int64_t ps_bstride, int64_t rowsum_ld, void* stream);

/* GROUPED weight gradients: several split-precision (math = 1) or one-product (math = 3) weight gradients of one kernel class in ONE launch pair (compute +
 * fixed-order slab reduction).  A weight gradient has a small output and a huge reduction length (K = batch * pixels), so a launch
 * that must fill 256 CUs alone splits K over ~32 workgroups per tile and moves 32 partial copies of dW through memory; sharing the
 * grid between the convolutions of a whole gradient bucket keeps the chip full with ~3 splits per tile.  (The reference's autograd
 * computes one weight gradient per convolution, VillanDiffusion.py:1161 accelerator.backward; the result is the same sum.)
 *   class  = vd_conv_wgrad_group_class(desc): 0 = not groupable (vd_conv_wgrad), equal values may share a launch;
 *   plan   : writes the host image of the device job table (n * vd_conv_wgrad_group_job_bytes() bytes; slab pointers held as OFFSETS),
 *            the workspace floats, the compute and reduce grid sizes; returns the class (> 0) or VD_EINVAL (< 0 never; 0 = error);
 *   rebase : once per uploaded table: turns the slab offsets into pointers into `ws`;
 *   launch : the two launches.  Deterministic (fixed reduction order); results agree with vd_conv_wgrad to summation order. */
int vd_conv_wgrad_group_class(const vd_wgrad_desc* desc);
int64_t vd_conv_wgrad_group_job_bytes(void);
/* Kernel family a class runs on: 32 = the 16x16x32 one-tap-row kernel (plain / upsample-fused 3x3 at 8x8 .. 32x32), 256 = the wide 1x1 kernel,
 * 3000 = the pre-split kernel, 0 = the three-copy 32x32x16 kernel (4x4, wide images, stride 2).
 * A math = 3 class (10000 + the math = 1 class) runs on the same family as its math = 1 class, one product per term. */
int vd_conv_wgrad_group_variant(int cls);
int vd_conv_wgrad_group_plan(const vd_wgrad_desc* descs, int n, void* table_out, int64_t* ws_floats, int* blocks, int* rblocks);
int vd_conv_wgrad_group_rebase(void* dev_table, int n, float* ws, void* stream);
int vd_conv_wgrad_group_launch(const void* dev_table, int n, int cls, int blocks, int rblocks, void* stream);
/* Host-only query: the kernel vd_conv_wgrad_group_launch runs for a class ("wgrad_ps_group_kernel<16, 2, true>(+group_reduce)"); 0, or VD_EINVAL
 * (empty name) for a class the launch has no case for. */
int vd_conv_wgrad_group_kernel_name(int cls, char* name, int name_len);

/* Split-precision operand for vd_gemm_desc.a_packed.  taps = 9: element (m, c, t) of the logical [M][C][9] matrix of a 3x3
 * convolution is read from W[m*row_stride + c*chan_stride + t] (plain weights: row_stride = C*9, chan_stride = 9; the transposed
 * operand of the stride-1 dgrad, A'[c_in][m_out] = W[m_out][c_in]: row_stride = 9, chan_stride = C_in*9 with M = C_in, C = M_out).
 * taps = 1: element (m, c) of a plain [M][C] matrix (1x1 convolution, attention projection) from W[m*row_stride + c*chan_stride]
 * (row-major: (C, 1); its transpose: (1, M_out-row length)).  Stored as bf16 hi = bf16(w), lo = bf16(w - hi) in the kernel's
 * fragment order.  `packed` holds vd_conv3_packed_bytes(M, C, taps) bytes, 16-byte aligned; C % 16 == 0. */
int64_t vd_conv3_packed_bytes(int M, int C, int taps);
int vd_conv3_pack_weights(const float* W, void* packed, int M, int C, int taps, int64_t row_stride, int64_t chan_stride, void* stream);
/* The same for n_jobs operands in one launch (all convolutions of a network after an optimizer step).  table: DEVICE array of
 * int64 [n_jobs][8] = {W address, packed address, M, C, row_stride, chan_stride, first workgroup of the job, taps}; job j owns
 * ceil(Mpad_j * C_j / 8 / 256) workgroups of 256 threads, first-workgroup numbers ascending from 0; total_blocks = their sum. */
int vd_conv3_pack_weights_multi(const int64_t* table, int n_jobs, int64_t total_blocks, void* stream);
/* The same job table, f16 operands (round 4, opt-in mixed precision -- the reference's GPU arithmetic is fp16 autocast, VillanDiffusion.py:260-264):
 * unit ((cc * taps + t) * 2 + q) * Mpad + m = channels cc*16 + q*8 + j of tap t, row m, rounded to f16; a job's image holds
 * vd_conv3_packed_bytes(M, C, taps) / 2 bytes.  Consumed by vd_gemm with vd_gemm_desc.math = 2. */
int vd_conv3_pack_weights_f16_multi(const int64_t* table, int n_jobs, int64_t total_blocks, void* stream);

/* W[M][C][T] -> Wt[C][M][T]  (operand for the dgrad GEMMs). */
int vd_weight_transpose(const float* W, float* Wt, int M, int C, int T, void* stream);
/* dX[b][c][y][x] (+)= sum_{2x2} dU[b][c][2y+i][2x+j]   (Upsample2D backward). */
int vd_sumpool2x2(const float* dU, float* dX, int B, int C, int H, int W, int64_t du_bstride, int64_t dx_bstride,
                  int accumulate, void* stream);
/* Stride-2 conv dgrad, second half: dX[b][c][y][x] = sum_{r,s: y+pad-r, x+pad-s even}
 * G[b][(c*9+r*3+s)][(y+pad-r)/2][(x+pad-s)/2], where G[b] = W2d^T[C*9, M] . dY[b][M, OH*OW] comes from vd_gemm (VD_A_COL,
 * VD_B_PLAIN) -- the stride-2 Downsample2D conv of the reference UNet (pad as in vd_gemm_desc). */
int vd_col2im_s2(const float* G, float* dX, int B, int C, int H, int W, int OH, int OW, int pad, int64_t g_bstride,
                 int64_t dx_bstride, void* stream);
/* ws[b*ws_ld + m] = sum_p X[b][m][p]  (bias / temb-projection gradients), then vd_colsum over b. */
int vd_rowsum(const float* X, float* ws, int B, int M, int P, int64_t x_bstride, int64_t ws_ld, void* stream);
/* out[c] (+)= sum_b ws[b*ld + c]  -- fixed order, deterministic. */
int vd_colsum(const float* ws, float* out, int B, int C, int64_t ld, int accumulate, void* stream);
/* n_jobs column sums in one launch: job i = table[4i..4i+3] = {address of ws (+ first column), address of out (+ first
 * column), number of columns (<= 64), ld}; out[c] += sum_b ws[b*ld + c], same order as vd_colsum (bit-identical).
 * `table` is a DEVICE array (the job list of a backward pass is the same every step: build once, reuse). */
int vd_colsum_segmented(const int64_t* table, int n_jobs, int B, void* stream);

/* ------------------------------------------------------------------------------------------
 * K1 -- GroupNorm (+SiLU) forward/backward.  Replaces F.group_norm + F.silu of
 * ResnetBlock2D.norm{1,2}, AttentionBlock.group_norm, conv_norm_out.
 * ------------------------------------------------------------------------------------------ */
/* ws: vd_groupnorm_ws_floats() floats of scratch (16-byte aligned), or NULL.  Groups larger than 28 K elements (256x256 images) are cut
 * into chunks handled by separate workgroups when ws is given (fixed-order combination of the chunk statistics).  Outside a HIP-graph
 * capture the chunks of a group exchange their statistics inside ONE launch (bounded polling of (value, launch-epoch) words in ws; a
 * chunk stays in registers between the statistics and the apply step); inside a capture, or with VD_GN_CHUNK1_OFF=1, a statistics
 * launch and an apply launch. */
int64_t vd_groupnorm_ws_floats(int B, int C, int HW, int G);
int vd_groupnorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                     int B, int C, int HW, int G, float eps, int apply_silu, int64_t x_bstride, int64_t y_bstride,
                     float* ws, void* stream);
/* Statistics only: mean / rstd per (b, group) and ss[b][c] = {gamma_c*rstd, beta_c - mean*gamma_c*rstd} for vd_gemm_desc.gn_ss
 * (one read of x, no y).  Groups of at most 12 K elements. */
int vd_groupnorm_stats(const float* x, const float* gamma, const float* beta, float* ss, float* mean, float* rstd,
                       int B, int C, int HW, int G, float eps, int64_t x_bstride, void* stream);
/* vd_groupnorm_stats from the per-tile channel sums a convolution left in vd_gemm_desc.gn_part ([B][tiles][C][2], HW pixels per image in
 * `tiles` tiles): same outputs, no pass over x.  Sums are combined in double precision in a fixed order. */
int vd_groupnorm_stats_from_partials(const float* part, int tiles, const float* gamma, const float* beta, float* ss, float* mean,
                                     float* rstd, int B, int C, int HW, int G, float eps, void* stream);
/* dx = GN'(dy) (+ extra); dgamma_ws/dbeta_ws are [B][C] partials (reduce with vd_colsum). */
int vd_groupnorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, const float* extra, float* dx, float* dgamma_ws, float* dbeta_ws,
                     int B, int C, int HW, int G, int apply_silu, int64_t dy_bstride, int64_t x_bstride,
                     int64_t extra_bstride, int64_t dx_bstride, float* ws, void* stream);
/* The same with a second residual gradient (extra2: the gradient a skip connection carries into x -- replaces the
 * vd_add_strided pass after the block, VillanDiffusion's UNet concatenates skips: SURVEY 3.4) and, when rowsum != NULL,
 * rowsum[b*rowsum_ld + c] = sum_p dx[b][c][p]: the per-image bias-gradient rows of the layer that produced x (autograd's
 * conv2d bias gradient is the sum of its dY = this dx over batch and pixels; the per-image rows also are the
 * time_emb_proj output gradient of a ResnetBlock2D).  NULL extra / extra2 / rowsum are skipped. */
int vd_groupnorm_bwd_fused(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, const float* extra, const float* extra2, float* dx, float* dgamma_ws,
                           float* dbeta_ws, float* rowsum, int B, int C, int HW, int G, int apply_silu,
                           int64_t dy_bstride, int64_t x_bstride, int64_t extra_bstride, int64_t extra2_bstride,
                           int64_t dx_bstride, int64_t rowsum_ld, float* ws, void* stream);
/* Host-only query (launches nothing): the kernel(s) that `which` (0 vd_groupnorm_fwd, 1 vd_groupnorm_bwd_fused, 2 vd_groupnorm_stats) takes
 * for these dimensions, chosen by the very functions the entry points switch on.  aligned: every pointer is 16-byte aligned and every
 * batch stride a multiple of 4 floats; has_ws: ws != NULL; stream: the stream of the call (a capturing stream takes the two-launch chunked
 * form).  Writes the names as `nm -C` shows the kernels, joined by '+' when there are two launches ("gn_fwd_wave_kernel<2>",
 * "gn_chunk_stats_kernel<16>+gn_chunk_apply_kernel"); a chunked backward with rowsum adds gn_chunk_rowsum_kernel, a generic one with
 * extra2 / rowsum the vd_add_strided / vd_rowsum kernels.  Returns the chunks per group S of the chunked kernels, 0 for the others, or
 * VD_EINVAL (empty name) where the entry point refuses the dimensions. */
int vd_groupnorm_plan(int which, int B, int C, int HW, int G, int aligned, int has_ws, void* stream, char* name, int name_len);

/* ------------------------------------------------------------------------------------------
 * K4 -- attention softmax.  S is [nb][N][N] stored key-major: S[b][j][i] = k_j . q_i * scale;
 * softmax runs over j for every column i.  Replaces torch.softmax in AttentionBlock.
 * ------------------------------------------------------------------------------------------ */
int vd_softmax_col_fwd(float* S, int nb, int N, void* stream);                       /* in place */
int vd_softmax_col_bwd(const float* P, float* dP, int nb, int N, float scale, void* stream); /* dP -> dS in place */
/* Whole single-head attention for tiny token counts (N <= 64): qkv is [B][3C][N]. */
int vd_attn_small_fwd(const float* qkv, float* out, float* P, int B, int C, int N, float scale,
                      int64_t qkv_bstride, int64_t out_bstride, void* stream);
int vd_attn_small_bwd(const float* qkv, const float* P, const float* dout, float* dqkv, int B, int C, int N,
                      float scale, int64_t qkv_bstride, int64_t dout_bstride, int64_t dqkv_bstride, void* stream);

/* K4 fused (diffusers AttentionBlock reached from loss.py:993): the whole attention core of N == 256 tokens in one
 * launch, scores / probabilities in registers, split-precision (bf16 hi/lo, f32 accumulation) contractions on the bf16 MFMA.
 *   qkv [B][3C][N] (q | k | v, C = heads * head_dim, a head = a channel slice), out [B][C][N]:
 *   out[b][h d + c][i] = sum_j v[c][j] P[j][i],  P[.][i] = softmax_j(scale * sum_c k[c][j] q[c][i]).
 * P == NULL: nothing but `out` is written (no-grad path).  P != NULL: [B*heads][N][N] (P[j][i]) is written once for the backward pass.
 * head_dim in {32, 64, 128} or a multiple of 256; anything else / N != 256 -> VD_EINVAL (callers keep the 3-launch path).
 * vd_attn_core_bwd: dP = v^T dout, dS = scale P (dP - delta) with delta_i = sum_j P dP = sum_c dout[c][i] out[c][i] (the saved forward
 * output, so P is read once), dS written to [B*heads][N][N], and dq = k dS written into the q slice of dqkv [B][3C][N] -- one launch;
 * dk = q dS^T and dv = dout P^T are plain products of dS / P (vd_gemm). */
int vd_attn_core_fwd(const float* qkv, float* out, float* P, int B, int heads, int head_dim, int N, float scale, void* stream);
int vd_attn_core_bwd(const float* qkv, const float* P, const float* out, const float* dout, float* dS, float* dqkv, int B, int heads,
                     int head_dim, int N, float scale, void* stream);

/* K4 flash (round 4; same reference code as above, multi-head blocks with MORE than 256 tokens -- the 32x32-token level of the
 * `LDM-CELEBA-HQ-256` UNet, reference model.py:706-776): the N x N score matrix never reaches HBM.
 *   head_dim == 32, N a multiple of 256 (N >= 256); qkv [B][3C][N] with batch stride qkv_bstride, out [B][C][N] (out_bstride).
 * vd_attn_flash_fwd: online softmax over 256-key blocks; lse [B*heads][N] = log sum_j exp(scale s_ji) is written when non-NULL
 *   (the backward pass needs it; NULL in the no-grad path).
 * vd_attn_flash_bwd: two launches -- (1) dq and delta_i = sum_c dout[c][i] out[c][i] (delta: [B*heads][N] scratch, written), with
 *   P = exp(scale s - lse_i) recomputed per key block; (2) dk and dv, the transposed walk (a workgroup owns 128 keys).  All three
 *   slices of dqkv [B][3C][N] are written (no accumulation).  Other shapes -> VD_EINVAL. */
int vd_attn_flash_fwd(const float* qkv, float* out, float* lse, int B, int heads, int head_dim, int N, float scale, int64_t qkv_bstride,
                      int64_t out_bstride, void* stream);
int vd_attn_flash_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* delta, float* dqkv, int B, int heads,
                      int head_dim, int N, float scale, int64_t qkv_bstride, int64_t out_bstride, int64_t dout_bstride,
                      int64_t dqkv_bstride, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3 -- timestep embedding + small elementwise helpers.
 * ------------------------------------------------------------------------------------------ */
/* emb[b][0:half]=sin(t_b*freqs_i), [half:2*half]=cos(t_b*freqs_i); flip_sin_to_cos swaps the halves.
 * freqs = exp(-ln(1e4)*i/(half-freq_shift)) is built by the host with the upstream fp32 op sequence. */
int vd_timestep_embedding(const float* t, const float* freqs, float* emb, int B, int half, int flip_sin_to_cos,
                          void* stream);
int vd_silu_fwd(const float* x, float* y, int64_t n, void* stream);
int vd_silu_bwd(const float* dy, const float* x, float* dx, int64_t n, int accumulate, void* stream);
/* dst[b][c][p] (+)= src[b][c][p] over [B][C*P] with batch strides. */
int vd_add_strided(float* dst, const float* src, int B, int64_t inner, int64_t dst_bstride, int64_t src_bstride,
                   int accumulate, void* stream);
/* x[i] *= alpha (alpha==0 stores exact zeros: gradient-buffer clear). */
int vd_scale(float* x, int64_t n, float alpha, void* stream);
/* out = sum_i coef[i] * src[i], n_src <= 6 (multistep sampler updates).  srcs / coefs are HOST arrays. */
int vd_lincomb(float* out, const float* const* srcs, const float* coefs, int n_src, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * K8 -- q-sample + backdoor shift + target + MSE (loss.py:909-939, 978-1006).
 *   x_t = a[t]*x0 + s[t]*eps + step[t]*R ;  y = coef[t]*R + eps     (VP/LDM: a=sqrt(abar), s=sqrt(1-abar);
 *                                                                    VE: a=1, s=sigma)
 * tables are device fp32 arrays indexed by the int64 timestep.
 * ------------------------------------------------------------------------------------------ */
int vd_qsample_backdoor(const float* x0, const float* R, const float* eps, const int64_t* t,
                        const float* tab_a, const float* tab_s, const float* tab_step, const float* tab_coef,
                        float* x_t, float* y, int B, int64_t chw, void* stream);
/* loss = mean((y - pred*pscale[b])^2); dpred = 2*(pred*pscale-y)*pscale/n * gscale.  partial: >= 1024 floats. */
int vd_mse_fwd_bwd(const float* pred, const float* y, const float* pscale, float* dpred, float* loss,
                   float* partial, int B, int64_t chw, float gscale, void* stream);
/* The same with the reference's selectable norm (loss.py:849-858, picked at loss.py:994,1003): kind VD_LOSS_L2 = F.mse_loss,
 * VD_LOSS_L1 = F.l1_loss (gradient sign(d), 0 at d == 0), VD_LOSS_HUBER = F.smooth_l1_loss (beta 1); all reduced by the mean. */
#define VD_LOSS_L2 0
#define VD_LOSS_L1 1
#define VD_LOSS_HUBER 2
int vd_loss_fwd_bwd(const float* pred, const float* y, const float* pscale, float* dpred, float* loss,
                    float* partial, int B, int64_t chw, float gscale, int kind, void* stream);
/* The shaped loss: vd_loss_fwd_bwd with a weight per sample in and the loss of every sample out.  With d = pred[b,i] * ps_b - y[b,i] and norm /
 * norm' those of vd_loss_fwd_bwd:
 *   l[b]  = (1/chw) sum_i norm(d)                                              (sample_loss, UNWEIGHTED)
 *   w[b]  = (weight ? weight[b] : 1) * (wtab ? wtab[clamp(t[b], 0, T-1)] : 1) * (flags && flags[b] ? poison_weight : 1)
 *   *loss = (1/B) sum_b w[b] l[b]                                              (the mean of the weighted sample losses, not divided by sum w)
 *   dpred[b,i] = ((gcoef * w[b]) * norm'(d)) * ps_b,  gcoef = (kind == VD_LOSS_L2 ? 2 : 1) * gscale / (B * chw)
 *   stats = {sum of l[b] over the clean samples, their count, sum of l[b] over the poisoned (flags[b] != 0) ones, their count}
 * With every weight 1 dpred has the bits vd_loss_fwd_bwd writes.  pscale, weight, flags: [B] or NULL; wtab: [T] or NULL (then t may be NULL);
 * dpred NULL: forward only; sample_loss [B] and stats [4] may be NULL; ws: vd_loss_sample_ws_floats(B, chw) floats.  Every sample is cut into
 * `segments` pieces, each summed by one 256-thread workgroup (16-byte loads when chw % 4 == 0 and pred, y, dpred are 16-byte aligned), and one
 * last workgroup adds the pieces in index order: no atomics, the same bits in every run.  vd_loss_sample_plan (host only) answers the segment
 * count and the grid the launcher uses for (B, chw). */
int vd_loss_sample_fwd_bwd(const float* pred, const float* y, const float* pscale, const float* weight, const float* wtab, const int64_t* t,
                           int T, const uint8_t* flags, float poison_weight, float* dpred, float* loss, float* sample_loss, float* stats,
                           float* ws, int B, int64_t chw, float gscale, int kind, void* stream);
int64_t vd_loss_sample_ws_floats(int B, int64_t chw);
int vd_loss_sample_plan(int B, int64_t chw, int* segments, int* blocks);
/* Trigger-inversion objective (distribution shift, Elijah): r = mean_b e[b] - lambda * tau, *loss = L = ||r||_2 over the chw elements,
 * dout[b] = r / (B L) for every b (the gradient of L with respect to e, contiguous [B, chw]) and dtau = -lambda r / L (the direct term of
 * dL/dtau; the term through the network is the sum over b of the network's input gradient).  e: [B, chw] with batch stride e_bstride >= chw;
 * tau, dtau: [chw]; partial: >= 1024 floats.  Two-phase sum in a fixed order (no atomics): bit-reproducible.  L == 0: zero gradients. */
int vd_trigger_inv_objective(const float* e, const float* tau, float lambda, float* loss, float* dout, float* dtau, float* partial,
                             int B, int64_t chw, int64_t e_bstride, void* stream);
/* Data-free backdoor-removal loss (mitigation.py): pred is [2B, chw] with batch stride pred_bstride >= chw -- rows 0..B-1 the model's output on
 * eps, rows B..2B-1 its output on eps + tau; ref is the frozen teacher's output on eps, contiguous [B, chw].
 *   clean = mean over B*chw of (pred[b] - ref[b])^2,  shift = mean over B*chw of (pred[B+b] - ref[b])^2,
 *   terms[0..2] = {w_clean*clean + w_shift*shift, clean, shift},
 *   dpred (contiguous [2B, chw]): dpred[b] = gscale*w_clean*2/(B*chw) * (pred[b] - ref[b]), dpred[B+b] the same with w_shift.
 * One read of pred and ref, one write of dpred; 16-byte accesses where chw, the stride and the pointers allow, with the same sums either way.
 * partial: >= 2048 floats.  Two-phase sum in a fixed order (no atomics): bit-reproducible. */
int vd_removal_loss(const float* pred, const float* ref, float w_clean, float w_shift, float gscale, float* dpred, float* terms,
                    float* partial, int B, int64_t chw, int64_t pred_bstride, void* stream);
/* Statistics of an image set x [N, C, H, W] (batch stride x_bstride) after y = clamp(x*mul + add, lo, hi), every operation rounded on its own
 * (vd_postprocess's values; lo = -inf, hi = +inf: no clamp).  Two passes: mean_img[C, H, W] = mean of y over N (sum in double); then
 *   stats[0] = sum_i ||y_i - mean_img||^2   (the mean pairwise squared distance over i < j is 2/(N-1) * stats[0]),
 *   stats[1] = sum_i TV(y_i),  TV(y) = sum_c ( sum |y[c,h+1,w] - y[c,h,w]| + sum |y[c,h,w+1] - y[c,h,w]| ).
 * partial: >= 2048 floats.  Fixed-order sums (no atomics): bit-reproducible, and a strided view gives the bits of its contiguous copy. */
int vd_image_set_stats(const float* x, int N, int C, int H, int W, int64_t x_bstride, float mul, float add, float lo, float hi,
                       float* mean_img, float* stats, float* partial, void* stream);
/* Trigger-inversion objective of a score network (SDE-VE, defense_ve.py), in noise-prediction units: n[b] = -sigma * s[b],
 * r = mean_b n[b] - lambda * tau, *loss = L = ||r||_2, dout[b] = sigma * dL/ds[b] = -sigma^2 r / (B L) for every b (contiguous [B, chw];
 * pre-multiplied by sigma: the network is fed x = sigma * (eps + tau), so the sum over b of its input gradient for this dout is the chain term
 * of dL/dtau) and dtau = -lambda r / L (the direct term).  s: [B, chw] with batch stride s_bstride >= chw; partial: >= 1024 floats.  The same
 * two-phase fixed-order sum as vd_trigger_inv_objective: bit-reproducible, and a strided s gives the bits of its contiguous copy.  L == 0: zero
 * gradients. */
int vd_score_inv_objective(const float* s, const float* tau, float sigma, float lambda, float* loss, float* dout, float* dtau,
                           float* partial, int B, int64_t chw, int64_t s_bstride, void* stream);
/* Streaming form of vd_image_set_stats (defense_ldm.py): merges the result (mean_b, stats_b) of a chunk of n_b images into the running result
 * (mean_a, stats_a) of n_a images by the pairwise update of Chan et al. -- never the sum / sum-of-squares form.  With delta = mean_b - mean_a and
 * n = n_a + n_b:  mean_a += delta * n_b / n  (in double, rounded once);  stats_a[0] += stats_b[0] + n_a*n_b/n * sum(delta^2);
 * stats_a[1] += stats_b[1].  n_a == 0 copies b into a.  mean_*: [chw] f32, stats_*: [2] f32; a and b must not alias.  sum(delta^2) is added in
 * double in a fixed order (no atomics): bit-reproducible.  One read of both means, one write of mean_a; 16-byte accesses where chw and the
 * pointers allow, with the same sums either way.  partial: >= 2048 floats, 8-byte aligned. */
int vd_image_set_merge(float* mean_a, float* stats_a, int64_t n_a, const float* mean_b, const float* stats_b, int64_t n_b, int64_t chw,
                       float* partial, void* stream);
/* Adversarial Neuron Pruning (anp.py).  All three take a NEURON TABLE: a device array of n_jobs x 6 int64, one job per selected weight tensor of a
 * flat parameter buffer, {weight offset in floats, rows, row length, bias offset in floats or -1, index of the layer's first neuron, first
 * workgroup}; a job owns ceil(rows / 4) workgroups (one 64-lane wave per row), first workgroups ascend from 0 and total_blocks is their sum.  One
 * launch serves the whole network.  A neuron is a row; neuron j of a job is element (first neuron + j) of mask / delta / xi / gmask / gxi.  Rows
 * need not be 16-byte aligned: an aligned row moves as f32x4, any other as scalars, with the same values and the same sums either way.
 *
 * vd_neuron_scale: w[row j] = s_j * w0[row j] with s_j = mask[j] + delta[j] in f32 (delta NULL: s_j = mask[j]); where the job has a bias,
 * w[bias j] = (1 + xi[j]) * w0[bias j] (xi NULL: the bias is copied).  Floats of w outside every job are not written.  w != w0. */
int vd_neuron_scale(const float* w0, float* w, const int64_t* table, int n_jobs, int64_t total_blocks, const float* mask, const float* delta,
                    const float* xi, void* stream);
/* gmask[j] (+)= scale * sum_k g[row j][k] * w0[row j][k] and, where the job has a bias, gxi[j] (+)= scale * (g[bias j] * w0[bias j]) (a job
 * without one leaves its gxi slots untouched; gxi may be NULL).  accumulate != 0 adds to what is there.  With element k of a row in item k / 4,
 * a lane keeps one f32 partial per position k % 4 over its items q = lane, lane + 64, ... in that order, adds them as (a0 + a1) + (a2 + a3), and
 * the 64 lanes are added by a fixed xor tree: bit-reproducible, and the longest chain of additions is ceil(len / 256) + 8. */
int vd_neuron_grad(const float* g, const float* w0, const int64_t* table, int n_jobs, int64_t total_blocks, float* gmask, float* gxi, float scale,
                   int accumulate, void* stream);
/* The projected step of the mask and of the perturbations, n floats, every f32 operation rounded on its own, in this order:
 *   buf given:  d = momentum * buf + g;  buf = d        (torch: buf.mul_(momentum).add_(g))
 *   buf NULL:   d = use_sign ? (g > 0) - (g < 0) : g    (torch.sign: 0 for +-0)
 *   x = min(max(x - lr * d, lo), hi)                    (torch: (x - lr * d).clamp(lo, hi), lr an f32)
 * A negative lr ascends. */
int vd_neuron_step(float* x, const float* g, float* buf, int64_t n, float lr, float momentum, float lo, float hi, int use_sign, void* stream);
/* LoRA fine-tuning (lora.py).  Both take an ADAPTER TABLE: a device array of n_jobs x 7 int64, one job per adapted weight tensor of a flat
 * parameter buffer, {weight offset in floats, rows M, row length L, offset of A in the adapter buffer, offset of B in the adapter buffer, first
 * row workgroup, first column workgroup}.  The weight is viewed as [M, L]; the ADAPTER BUFFER `ab` is one flat f32 buffer that holds, per job,
 * A [r, L] row-major and then B [M, r] row-major, every piece starting at a multiple of 4 floats (the padding is never read and never written);
 * `gab` mirrors it.  A job owns ceil(M / 4) row workgroups (one 64-lane wave per row) and ceil(L / 256) column workgroups (256 columns each);
 * both first-workgroup columns ascend from 0.  One rank 1 <= r <= 32 per launch.  Rows need not be 16-byte aligned: where L is a multiple of 4
 * and the job starts 16-byte aligned in every buffer a row moves as f32x4, otherwise as scalars, with the same values and sums either way.
 *
 * vd_lora_merge: w[row j][k] = w0[row j][k] + s * sum_{q<r} B[j][q] * A[q][k] for every job, the sum over q in ascending order from 0, every
 * operation rounded on its own (B = 0 gives w0 + 0).  Floats of w outside every job are not written.  w != w0.  total_blocks: the row
 * workgroups of the table. */
int vd_lora_merge(const float* w0, float* w, const int64_t* table, int n_jobs, int64_t total_blocks, const float* ab, int r, float s, void* stream);
/* gab.B[j][q] (+)= s * sum_k g[row j][k] * A[q][k];  gab.A[q][k] (+)= s * sum_j B[j][q] * g[row j][k];  accumulate != 0 adds to what is
 * there.  g: the ordinary weight gradient, laid out like w.  One launch: total_blocks = the row workgroups of the table plus its column
 * workgroups; the row workgroups come first.  g is read twice, the padding of gab is never written, no atomics: bit-reproducible.  The sums:
 *   B[j][q]: with element k of a row in item k / 4, a lane keeps one f32 partial over its items lane, lane + 64, ... in that order, the four
 *            elements of an item in index order; the 64 lanes are added by a fixed xor tree; the sum is multiplied by s.
 *   A[q][k]: wave w of the four adds rows j = w, w + 4, w + 8, ... in that order in one f32 chain; the chains are added as
 *            ((c0 + c1) + c2) + c3; the sum is multiplied by s. */
int vd_lora_grad(const float* g, const int64_t* table, int n_jobs, int64_t total_blocks, const float* ab, float* gab, int r, float s,
                 int accumulate, void* stream);
/* The adapter gradient of 1x1 layers y_b = W x_b (W = W0 + s B A) straight from their activations: no [M, L] weight gradient is formed.
 *   gab.A[q][l] (+)= s * sum_{b,p} (sum_m Bm[m][q] dy[b][m][p]) x[b][l][p]      gab.B[m][q] (+)= s * sum_{b,p} dy[b][m][p] (sum_l A[q][l] x[b][l][p])
 * One compute launch plus one reduce launch serve an ACTIVATION JOB TABLE of n_rows x 16 int64, given twice: `host_table` in host memory (every
 * row is checked there before any launch) and `table`, the same bytes in device memory.  A row is
 *   {dy address, dy batch stride in floats, x address, x batch stride, images B, M, L, pixels N, offset of A [r, L] in the adapter buffer,
 *    offset of B [M, r] in the adapter buffer, first workgroup, workgroups n_wg, first accumulator row, accumulator rows, workspace offset in
 *    floats, first reduce workgroup}
 * with dy [B, M, N] and x [B, L, N] f32, channel stride N, pixels contiguous (channel slices of wider tensors: their own batch strides).  The
 * L + M ACCUMULATOR ROWS of a layer are the rows of x (-> A[.][l]) followed by the rows of dy (-> B[m][.]); a table row covers at most 768 of
 * them, a layer with more takes several table rows (each reads x and dy in full).  1 <= n_wg <= B * ceil(N / 32); first workgroups ascend
 * from 0 by n_wg, workspace offsets from 0 by n_wg * rows * r, first reduce workgroups from 0 by ceil(rows * r / 256)
 * (villandiffusion_amd.ops.lora_act_plan lays a table out).  f32 FMA, f32 accumulation, no atomics: bit-reproducible.  The sums:
 *   workgroup w of a row takes the 32-pixel TILES w, w + n_wg, ... of the B * ceil(N / 32) tiles of its layer (tile = image * ceil(N / 32) +
 *   tile of the image).  Per tile, Z[q][p] = sum_l A[q][l] x[l][p]: wave v of the four adds the row pairs j = v, v + 4, ... (rows 2j, 2j + 1) in
 *   that order, one fma chain per row parity; the two parities are added, then the waves as ((w0 + w1) + w2) + w3; T = Bm^T dy likewise.
 *   Each accumulator element is one fma chain over the pixels of its workgroup's tiles in ascending order (tile after tile), written to the
 *   workspace; the reduce launch adds the n_wg partials in workgroup order from 0, multiplies by s and stores (accumulate == 0) or adds in f32.
 * Every pixel is read as a scalar: rows need no alignment, and there is no second path.  ab, x, dy are never written; the padding of gab and
 * every slot of gab outside the table's rows are never written; `ws` (caller-owned, >= vd_lora_act_grad_ws_floats floats) is scratch.
 * VD_EINVAL before any launch: a rank outside [1, 32], a row that breaks the rules above, a workspace that is too small. */
int64_t vd_lora_act_grad_ws_floats(const int64_t* host_table, int n_rows, int r);   /* -1: an invalid table or rank */
int vd_lora_act_grad(const int64_t* host_table, const int64_t* table, int n_rows, const float* ab, float* gab, int r, float s, int accumulate,
                     float* ws, int64_t ws_floats, void* stream);

/* ------------------------------------------------------------------------------------------
 * K9 -- global grad-norm clip + Adam on flat buffers (VillanDiffusion.py:445,1165-1169).
 * ------------------------------------------------------------------------------------------ */
int vd_l2norm_sq(const float* g, int64_t n, float* partial, float* out_sq, void* stream);
/* clip = min(1, max_norm/(sqrt(*norm_sq)*inv_scale + 1e-6)); g' = g*inv_scale*clip; torch.optim.Adam update.  With norm_sq given and
 * *norm_sq not finite the kernel leaves p / m / v untouched (GradScaler.step's overflow skip) and adds 1 to *skipped (device word, may be
 * NULL): the host reads that counter lazily and refuses to go on (default arithmetic) or halves its loss scale (f16 mode). */
int vd_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* norm_sq, float max_norm,
                 float inv_scale, float lr, float beta1, float beta2, float eps, int step, unsigned* skipped, void* stream);
/* vd_adam_step plus, in the same pass, the exponential moving average of the updated parameters (diffusers EMAModel.step):
 * ema += (p_new - ema) * one_minus_decay, each operation rounded on its own.  p / m / v get the bits vd_adam_step gives them.  A skipped step
 * (see above) leaves ema untouched as well.  one_minus_decay in [0, 1]; ema: n floats, 16-byte aligned like the rest.  36 B/parameter. */
int vd_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* norm_sq, float max_norm,
                     float inv_scale, float lr, float beta1, float beta2, float eps, int step, float one_minus_decay, unsigned* skipped,
                     void* stream);
/* a <-> b in place, n floats each, bit for bit (nothing is rounded; NaN payloads survive): 16-byte accesses where both pointers allow, 4-byte
 * otherwise.  The buffers must not overlap. */
int vd_swap(float* a, float* b, int64_t n, void* stream);
/* Sharpness-aware minimisation (trainer.py, Trainer(sam=...)): the perturbation w <- w + e between the two passes of a SAM step, with
 * e_i = rho * T_i^2 g_i / ||T g||_2.  mode 0 (SAM): T_i = 1; mode 1 (ASAM): T_i = |w_i| + eta, in f32.  Plain C++ with vector loads and stores,
 * no atomics, every operation rounded on its own (no FMA contraction), every sum in a fixed order: bit-reproducible.  The flat kernels walk
 * the n floats in items of four from the buffer's start, item q in thread q % (grid * block) of the launch vd_sam_plan reports: one 16-byte
 * access where every pointer is 16-byte aligned, four scalar ones otherwise (and for a last, partial item), with the same values and the
 * same sums either way.  Pointers are 4-byte aligned.  VD_EINVAL before any launch: a mode outside {0, 1}, a negative or non-finite rho or
 * eta, n < 0, a required pointer that is NULL, buffers that overlap.
 *
 * vd_sam_plan (host only): the launch shape of vd_sam_norm_sq's first stage and of vd_sam_perturb for n floats:
 *   block = 256, floats_per_thread = 16, grid = clamp(ceil(n / (block * floats_per_thread)), 1, 1024); past the cap a thread strides on. */
int vd_sam_plan(int64_t n, int* grid, int* block, int* floats_per_thread);
/* *out_sq = sum_i u_i * u_i with u_i = T_i * g_i (mode 0: u_i = g_i; w may be NULL).  partial: >= 1024 floats of scratch.  Two stages:
 *   1. a thread keeps one f32 partial per position k % 4 over its items in ascending order, adds them as (a0 + a1) + (a2 + a3); the 64 lanes
 *      of a wave are added by a fixed xor tree, the four waves as (r0 + r1) + (r2 + r3); partial[workgroup] holds the result;
 *   2. one workgroup: thread t adds partial[t], partial[t + 256], ... in that order, then the same tree.
 * The longest chain of additions is ceil(ceil(n / 4) / (grid * block)) + ceil(grid / 256) + 18. */
int vd_sam_norm_sq(const float* g, const float* w, int64_t n, int mode, float eta, float* partial, float* out_sq, void* stream);
/* One pass: backup[i] = w[i] (bit for bit; backup may be NULL), then w[i] = w[i] + a * g[i] with c = rho / (sqrtf(*norm_sq) + 1e-12f) and a = c
 * (mode 0) or a = (c * T_i) * T_i (mode 1, T_i from the w[i] just read).  *norm_sq is a device word.  If it is not finite or is 0, w is left
 * as it is and backup is still written.  w, g and backup do not overlap.  A raw write of weights: the caller invalidates what it derived
 * from them. */
int vd_sam_perturb(float* w, const float* g, float* backup, int64_t n, int mode, float eta, float rho, const float* norm_sq, void* stream);
/* The neuron-adaptive mode, over a NEURON TABLE (see vd_neuron_scale): T_j = sqrtf(wsq_j / len_j) + eta, the root mean square of weight row j
 * plus eta, with wsq_j = sum_k w_jk^2 and gsq_j = sum_k g_jk^2 from vd_neuron_grad(w, w, ...) and vd_neuron_grad(g, g, ...).  wsq, gsq, coef:
 * n_neurons floats.
 *   *norm_sq = sum_j (T_j * T_j) * gsq_j;   coef[j] = ((rho / (sqrtf(*norm_sq) + 1e-12f)) * T_j) * T_j;   every coef[j] = 0 where *norm_sq
 * is not finite or is 0.  One workgroup of 256 threads: thread t walks the jobs in table order and in each job the rows t, t + 256, ... in that
 * order, all in ONE f32 chain; the 256 chains are added by the xor tree of a wave and the four waves as (r0 + r1) + (r2 + r3).  The longest
 * chain of additions is sum over the jobs of ceil(rows / 256), plus 8. */
int vd_sam_neuron_coef(const float* wsq, const float* gsq, const int64_t* table, int n_jobs, int64_t n_neurons, float rho, float eta, float* coef,
                       float* norm_sq, void* stream);
/* w[row j][k] = w[row j][k] + coef[j] * g[row j][k] for every weight row of the table, in vd_neuron_scale's layout (one wave per row, four rows
 * per workgroup; an aligned row moves as f32x4, any other as scalars, with the same values).  Biases and every float outside the table's rows
 * are not written.  w != g. */
int vd_neuron_axpy(float* w, const float* g, const int64_t* table, int n_jobs, int64_t total_blocks, const float* coef, void* stream);
/* Activation-based channel pruning (actprune.py) -- csrc/vd_actstat.hip.
 *
 * vd_channel_stats: per-channel sums of a hidden activation for a whole network.  A JOB TABLE of n_jobs x 11 int64, one job per tapped tensor,
 * is given twice: `host_table` in host memory (every job is checked there before any launch) and `table`, the same bytes in device memory.  A
 * job is
 *   {address of x, address of mean, address of rstd, address of gamma, address of beta, B, C, HW, G, first channel, first workgroup}
 * with x f32 [B, C, HW] contiguous, mean and rstd [B, G], gamma and beta [C].  First channels ascend and the channel ranges do not overlap;
 * a job owns the workgroups vd_channel_stats_plan reports, first workgroups ascend from 0 by that count (the neuron-table convention).
 *   act = 0:  a = x; the four statistics addresses are not read and may be 0.
 *   act = 1:  a = z * sigmoid(z), z = fma((x - mean[b][g]) * rstd[b][g], gamma[c], beta[c]), g = c / (C / G), every other operation rounded
 *             on its own: the order of vd_groupnorm_fwd's element path and its sigmoid (1 ulp hardware reciprocal of 1 + exp(-z)) with SiLU
 *             on.  (Its register, wave and chunk kernels fold the same map into fma(x, gamma * rstd, beta - mean * gamma * rstd).)
 *   out[2 * (first channel + c) + {0, 1}] = {sum of a, sum of a * a} over b and p, f32, WRITTEN (never accumulated); out holds out_channels
 *   pairs.
 * No atomics; every sum in a fixed order: bit-reproducible.  The channel is walked in items of four consecutive floats of one image's run
 * (I = ceil(HW / 4) items per run, B * I per channel, item q = b * I + i) and cut into S segments of L = ceil(B * I / S) items, S =
 * clamp(ceil(B * I / 1024), 1, 256).  One 64-lane wave sums one (channel, segment): lane l takes the items lo + l, lo + l + 64, ... in that
 * order, one f32 partial per position of an item, added as (a0 + a1) + (a2 + a3), the lanes by a fixed xor tree.  With S > 1 the pairs are
 * parked in `ws` and a second launch adds a channel's S pairs in index order.  The longest chain of additions is
 *   ceil(L / 64) + 8 + (S - 1).
 * An item is one 16-byte load where x is 16-byte aligned and HW % 4 == 0, four scalar loads otherwise, with the same values and sums either
 * way.  x is read once; nothing but out and ws is written.  ws: >= vd_channel_stats_ws_floats floats (0: may be NULL).
 * VD_EINVAL before any launch: n_jobs < 1, act outside {0, 1}, C % G != 0, a null x, a null statistics address with act = 1, first
 * channels or workgroups that break the rules above, an out or ws that is too small.
 * vd_channel_stats_plan (host only): workgroups of a job, segments S per channel, and the chain length above. */
int vd_channel_stats_plan(int B, int C, int64_t HW, int* workgroups, int* segments, int64_t* chain);
int64_t vd_channel_stats_ws_floats(const int64_t* host_table, int n_jobs);      /* -1: an invalid table */
int vd_channel_stats(const int64_t* host_table, const int64_t* table, int n_jobs, int act, float* out, int64_t out_channels, float* ws,
                     int64_t ws_floats, void* stream);
/* buf[row j][k] = +0.0f for every weight row j of a NEURON TABLE (see vd_neuron_scale) with keep[first neuron + j] == 0.0f, in place, in
 * vd_neuron_scale's layout (one wave per row; an aligned row moves as f32x4, any other as scalars).  Every other float of buf -- kept rows,
 * biases, floats outside the table -- is neither read nor written.  One launch for the network. */
int vd_neuron_keep_rows(float* buf, const int64_t* table, int n_jobs, int64_t total_blocks, const float* keep, void* stream);
/* Channel Lipschitzness-based Pruning (clp.py) -- csrc/vd_clp.hip.
 *
 * vd_channel_lipschitz: out[first neuron + j] = sigma_max(W_j) * |scale[first neuron + j]| for every weight row of a network, W_j the row seen
 * as a [Cin, T] matrix, in one launch.  A LIPSCHITZ TABLE of n_jobs x 6 int64 is given twice: `host_table` in host memory (every job is checked
 * there before any launch) and `table`, the same bytes in device memory.  A job is
 *   {weight offset in floats, rows, Cin, T, first neuron, first workgroup}
 * with the weight [rows, Cin, T] contiguous at w + offset; T = 9 (3x3 convolutions) or 1 (1x1 convolutions, linears, attention projections).
 * The neuron-table convention: one 64-lane wave per row, four rows per 256-thread workgroup, a job owns ceil(rows / 4) workgroups; first
 * neurons ascend from 0 by rows, first workgroups from 0 by that count, and total_blocks is their sum.
 *   Gram stage.  G = W_j^T W_j, the T (T + 1) / 2 entries (i, j), i <= j, entry e = i * 9 - i * (i - 1) / 2 + (j - i) (the upper triangle row
 *   by row).  Lane l takes the input channels l, l + 64, ... in ascending order, one f32 partial per entry from +0, p_e = p_e + w[c][i] * w[c][j]
 *   with the product and the sum rounded on their own; the 64 lanes are added by the fixed xor tree (offsets 32, 16, ..., 1).  No atomics:
 *   bit-reproducible.  The longest chain of additions is ceil(Cin / 64) + 6 (vd_channel_lipschitz_plan reports it).
 *   Eigen stage.  T = 1: lambda_max = G_00.  T = 9: G is scaled by a power of two so that its largest diagonal entry lies in [1, 2) and
 *   diagonalised in f32 by cyclic Jacobi, 8 sweeps over the pairs (p, q), p < q, row by row, with Rutishauser's rotation formulas and
 *   correctly rounded division and square root; a pair with |a_pq| <= 2^-30 is left alone, so a diagonal G gives exactly max_i G_ii.
 *   lambda_max is the largest diagonal entry after the last sweep.  Relative error of lambda_max: at most 5760.5 * 2^-24 (each of the at most
 *   288 rotations moves it by at most 20 * 2^-24 lambda_max: 4 roundings per updated entry and the rounding of c, s, tau, over rows and columns
 *   of Frobenius norm at most 2 lambda_max; 2^-25 for the pairs left alone and the off-diagonal rest after the last sweep) -- a worst case
 *   over the operation count; a few 2^-24 is what is measured.
 *   out = sqrtf(lambda_max) * fabsf(scale) (scale NULL: no factor), WRITTEN, never accumulated; a zero row gives +0.0.
 *   gram != NULL: the row's Gram entries are also written at gram[45 * neuron + e]; a T = 1 row writes slot 0 and touches no other.
 * A row is staged through LDS in pieces of 576 floats: f32x4 loads where the job starts 16-byte aligned and Cin * T is a multiple of 4, scalar
 * loads otherwise, with the same values and sums either way.  w is read once; nothing but out and gram is written.  out and scale hold one
 * float per neuron of the table, gram 45.
 * VD_EINVAL before any launch: a null w, host_table, table or out; n_jobs < 1; T outside {1, 9}; rows < 1 or Cin < 1; a negative offset; first
 * neurons, first workgroups or a total_blocks that break the rule above.
 * vd_channel_lipschitz_plan (host only): the chain length of a row of Cin channels and T taps. */
int vd_channel_lipschitz_plan(int Cin, int T, int64_t* chain);
int vd_channel_lipschitz(const float* w, const int64_t* host_table, const int64_t* table, int n_jobs, int64_t total_blocks, const float* scale,
                         float* out, float* gram, void* stream);
/* Anchored fine-tuning (anchor.py, Trainer(anchor=...)) -- csrc/vd_anchor.hip: the penalty lambda / 2 * sum_i F_i (w_i - w0_i)^2 that holds the
 * weights to a starting point w0 (EWC, Kirkpatrick et al. 2017, F the diagonal Fisher information; F = 1: L2-SP, Li et al. 2018).  Plain C++ with
 * vector loads and stores, no atomics, every operation rounded on its own (no FMA contraction), every sum in a fixed order: bit-reproducible.
 * Both kernels walk the n floats as vd_sam_perturb does: items of four from the buffer's start, item q in thread q % (grid * block), one 16-byte
 * access where every pointer is 16-byte aligned, four scalar ones otherwise (and for a last, partial item), with the same values and the same
 * sums either way.  Pointers are 4-byte aligned.  VD_EINVAL before any launch: n < 0, a required pointer that is NULL, buffers that overlap, a
 * non-finite s or coef, a negative s.
 *
 * vd_anchor_plan (host only): the launch shape of both kernels for n floats.  It is vd_sam_plan's rule:
 *   block = 256, floats_per_thread = 16, grid = clamp(ceil(n / (block * floats_per_thread)), 1, 1024); past the cap a thread strides on. */
int vd_anchor_plan(int64_t n, int* grid, int* block, int* floats_per_thread);
/* One step of the Fisher estimate, in this order:  q = g[i] * g[i];  F[i] = F[i] + s * q.   s >= 0 is the 1 / K of a mean over K batches.
 * F and g do not overlap.  12 B/float. */
int vd_fisher_accum(float* F, const float* g, int64_t n, float s, void* stream);
/* The penalty's gradient added to g, in this order:  d = w[i] - w0[i];  t = F[i] * d (F NULL: t = d, L2-SP);  g[i] = g[i] + coef * t.
 * With pen != NULL the same pass forms *pen = sum_i t * d (a device word: the UNSCALED penalty sum F d^2; the caller multiplies by lambda / 2),
 * every product t * d rounded to f32 and added in vd_sam_norm_sq's two stages:
 *   1. a thread keeps one f32 partial per position k % 4 over its items in ascending order, adds them as (a0 + a1) + (a2 + a3); the 64 lanes
 *      of a wave are added by a fixed xor tree, the four waves as (r0 + r1) + (r2 + r3); partial[workgroup] holds the result;
 *   2. one workgroup: thread t adds partial[t], partial[t + 256], ... in that order, then the same tree.
 * The longest chain of additions is ceil(ceil(n / 4) / (grid * block)) + ceil(grid / 256) + 18.
 * partial: >= 1024 floats of scratch, needed with pen only.  pen NULL: no sum is formed, neither partial nor pen is touched.  w, w0 and F are
 * read only; g, w, w0, F do not overlap each other or the scratch.  20 B/float (16 without F). */
int vd_anchor_grad(float* g, const float* w, const float* w0, const float* F, int64_t n, float coef, float* partial, float* pen, void* stream);
/* Mode Connectivity Repair (curve.py: Curve, CurveAdam) -- csrc/vd_curve.hip: a point of a one-bend curve between two checkpoints A and B of
 * one architecture (Garipov et al. 2018; Zhao et al. 2020), phi = ca * A + cm * theta + cb * B over whole flat weight buffers, and the squared
 * sides of the triangle (A, theta, B).  Plain C++ with vector loads and stores, no atomics, every operation rounded on its own (no FMA
 * contraction), every sum in a fixed order: bit-reproducible.  Both kernels walk the n floats as vd_sam_perturb does: items of four from the
 * buffer's start, item q in thread q % (grid * block), one 16-byte access where every pointer of the call is 16-byte aligned, four scalar ones
 * otherwise (and for a last, partial item), with the same values and the same sums either way.  Pointers are 4-byte aligned.
 *
 * vd_curve_plan (host only): the launch shape of both kernels for n floats.  It is vd_sam_plan's rule:
 *   block = 256, floats_per_thread = 16, grid = clamp(ceil(n / (block * floats_per_thread)), 1, 1024); past the cap a thread strides on. */
int vd_curve_plan(int64_t n, int* grid, int* block, int* floats_per_thread);
/* out[i] = (ca * wa[i] + cm * wm[i]) + cb * wb[i]: three products and two sums in that order, each rounded to f32.  The three inputs may be
 * one another (the midpoint of the chord is wm = wa with cm = 0); out overlaps none of them.  n = 0 returns 0 without a launch.  A raw write of
 * weights where out is a network's: the caller invalidates what it derived from them.  16 B/float.
 * VD_EINVAL before any launch: n < 0, a NULL pointer, out overlapping an input, a non-finite coefficient. */
int vd_curve_point(float* out, const float* wa, const float* wm, const float* wb, int64_t n, float ca, float cm, float cb, void* stream);
/* out3 = {sum_i (wm[i] - wa[i])^2, sum_i (wm[i] - wb[i])^2, sum_i (wa[i] - wb[i])^2} (a device array), every difference and every square rounded
 * to f32, each sum added in vd_sam_norm_sq's two stages:
 *   1. a thread keeps one f32 partial per position k % 4 over its items in ascending order, adds them as (a0 + a1) + (a2 + a3); the 64 lanes
 *      of a wave are added by a fixed xor tree, the four waves as (r0 + r1) + (r2 + r3); partial[s * 1024 + workgroup] holds sum s;
 *   2. one workgroup: per sum, thread t adds partial[t], partial[t + 256], ... in that order, then the same tree.
 * The longest chain of additions is ceil(ceil(n / 4) / (grid * block)) + ceil(grid / 256) + 18.
 * partial: >= 3 * 1024 floats of scratch.  The three inputs are read once and may be one another; n = 0 writes three +0.0.  12 B/float.
 * VD_EINVAL before any launch: n < 0, a NULL pointer, the scratch or out3 overlapping an input or each other. */
int vd_curve_geometry(const float* wa, const float* wm, const float* wb, int64_t n, float* partial, float* out3, void* stream);
/* Checkpoint merging (merge.py: merge, merge_scan) -- csrc/vd_merge.hip: task arithmetic (Ilharco et al. 2023) and TIES-Merging (Yadav et al.
 * 2023) of up to 8 checkpoints of one layout over whole flat weight buffers, tau_i = theta_i - theta_base the task vectors.  Plain C++ with
 * vector loads and stores, every operation rounded to f32 on its own (no FMA contraction), no float atomics and no global atomics (LDS integer
 * adds into histogram bins only: integer counts do not depend on order): bit-reproducible.  The kernels walk the n floats as vd_curve_point
 * does: items of four from the buffer's start, item q in thread q % (grid * block), one 16-byte access where every data pointer of the call is
 * 16-byte aligned, four scalar ones otherwise (and for a last, partial item), with the same bits either way.  n >= 2^31 is VD_EINVAL
 * everywhere (the per-workgroup counts are 32-bit).
 * Two deliberate departures from the published TIES code: the k largest magnitudes are kept with ties at the threshold ALL kept (the published
 * code keeps k + 1), and a sign sum of exactly zero elects + (the published code takes the majority sign of the whole vector there).
 *
 * vd_merge_plan (host only): the launch shape of the kernels below for n floats, vd_curve_plan's rule
 *   block = 256, floats_per_thread = 16, grid = clamp(ceil(n / (block * floats_per_thread)), 1, 1024); past the cap a thread strides on,
 * and ws_bytes = 32 + grid * 257 * 4, the scratch vd_merge_select needs for n floats. */
enum { VD_MERGE_LINEAR = 0, VD_MERGE_TIES = 1 };
int vd_merge_plan(int64_t n, int* grid, int* block, int* floats_per_thread, int64_t* ws_bytes);
/* Exact selection: with d[j] = w[j] - base[j] (one f32 subtraction) and key[j] the bits of |d[j]| as uint32 (non-negative floats order like
 * their bits), thr_out[0] (a device f32) = the k-th largest key, 0 <= k <= n, found by radix selection in FOUR PASSES OF 8 BITS, most
 * significant byte first.  Each pass reads w and base once, counts the keys that match the prefix found so far into per-workgroup LDS bins
 * and writes them to ws; a one-workgroup finish adds them in 64 bits, walks the bins from the top and moves the prefix and the remaining rank
 * (kept in ws) on.  A fixed launch sequence on `stream`, no read-back between passes.  8 B/float per pass.
 *   rec[0] = n_gt, keys above the threshold; rec[1] = n_eq, keys equal to it; rec[2] = n_nonfinite, keys >= 0x7F800000 (inf and NaN; counted
 *   in the first pass whatever k is).  INVARIANT for 1 <= k <= n:  n_gt < k <= n_gt + n_eq.
 *   k = 0: thr_out = +inf, n_gt = n_eq = 0 (one pass, for n_nonfinite).  k = n: the minimum.  n = 0: nothing that reads w is launched; +inf
 *   and three zeros are written.
 * w and base are read only and may be one another.  ws: >= ws_bytes of vd_merge_plan(n), 8-byte aligned; rec: 3 int64.
 * VD_EINVAL before any launch: a NULL or misaligned pointer, k outside [0, n], ws, thr_out or rec overlapping an input or each other. */
int vd_merge_select(const float* w, const float* base, int64_t n, int64_t k, void* ws, float* thr_out, int64_t* rec, void* stream);
/* The merge, one pass with no temporary.  tasks: a HOST array of K device pointers, 1 <= K <= 8; lam: a HOST array of K floats (both read at
 * the call; lam is ignored and may be NULL with VD_MERGE_TIES); thr: a DEVICE array of K floats, what vd_merge_select wrote, or zeros for
 * "keep everything".  Per element j, with d_i = tasks[i][j] - base[j] and t_i = (|d_i| >= thr[i]) ? d_i : +0.0f:
 *   VD_MERGE_LINEAR:  acc = 0; for i ascending: acc = acc + lam[i] * t_i;  out[j] = base[j] + acc.
 *   VD_MERGE_TIES:    s = 0; for i ascending: s = s + t_i;  the elected sign is + where s >= 0, else -;
 *                     m = 0, c = 0; for i ascending, if t_i != 0 and its sign is the elected one: m = m + t_i, c += 1;
 *                     tau = c ? m / (float)c : +0.0f (an IEEE division);  out[j] = base[j] + lam_out * tau.
 * stats (2 K + 2 device int64): kept[i] = #(|d_i| >= thr[i]) (= n_gt + n_eq of the matching select); won[i] = the entries of task i that
 * entered m (LINEAR: its non-zero kept entries); support = positions with any non-zero t_i; conflict = positions with non-zero t_i of both
 * signs.  Per-workgroup uint32 counts go to partial (>= (2 K + 2) * 1024 uint32), a one-workgroup finish adds them in 64 bits.
 * out may be exactly base or exactly one tasks[i] (in place: a thread reads an element before it writes it), otherwise it overlaps none of
 * them; the inputs may be one another.  n = 0: no launch over the data, stats all zero.  4 (K + 2) B/float.
 * VD_EINVAL before any launch: K outside [1, 8], an unknown mode, a NULL or misaligned pointer or entry of tasks, out overlapping an input
 * partially, a non-finite lam[i] (LINEAR) or lam_out, partial or stats overlapping anything else. */
int vd_merge_apply(float* out, const float* base, const float* const* tasks, const float* lam, const float* thr, int K, int64_t n, int mode,
                   float lam_out, uint32_t* partial, int64_t* stats, void* stream);
/* vd_merge_apply with a seeded random drop of every task vector: DARE (Yu et al., ICML 2024: drop with probability p, rescale the survivors
 * by 1 / (1 - p); VD_MERGE_LINEAR is DARE-linear, VD_MERGE_TIES DARE-TIES) and, with VD_DROP_COPY, Fine-mixing (Zhang et al., Findings of
 * EMNLP 2022).  tasks, lam, drop_thr, rescale and streams are HOST arrays of K entries read at the call; thr is the DEVICE array of
 * vd_merge_apply.  The walk, the alignment rule, n < 2^31 and n = 0 are vd_merge_apply's, the launch shape vd_merge_plan's.
 * The draw is a pure function of (seed, streams[i], element index j counted from the buffer's start -- never of an address):
 *   q = j >> 2;  r = philox4x32_10(counter = (lo32(q), hi32(q), streams[i], 1), key = (lo32(seed), hi32(seed)))[j & 3];
 *   keep_i = (uint64)r >= drop_thr[i],   0 <= drop_thr[i] <= 2^32:  0 keeps everything, 2^32 nothing; an integer Bernoulli whose keep
 *   probability is exactly (2^32 - drop_thr[i]) / 2^32.
 * Counter word 3 is 1; vd_randn and vd_sched_step use 0 there, so no noise draw of the same seed shares a counter.  One Philox call serves
 * the four floats of an item for one task.
 * Per element j, with d_i = tasks[i][j] - base[j]:
 *   t_i = (|d_i| >= thr[i] && keep_i) ? (VD_DROP_RESCALE ? d_i * rescale[i] : d_i) : +0.0f,
 * then VD_MERGE_LINEAR / VD_MERGE_TIES proceed word for word as stated for vd_merge_apply, every operation rounded to f32 on its own.  With
 * every drop_thr[i] = 0 and no VD_DROP_RESCALE the bits and the counts are vd_merge_apply's; with drop_thr[i] = 2^32 out is base (a -0.0 of
 * base becomes +0.0 as at lam = 0) and drawn = 0.  rescale is the caller's number (DARE: f32(1 / (1 - p)) of the nominal p).
 * VD_DROP_COPY (K = 1 and VD_MERGE_LINEAR; thr, lam, rescale and lam_out are ignored and may be NULL):  out[j] = keep_0 ? tasks[0][j] :
 *   base[j], the bits copied, -0.0, denormals and NaN payloads included.  12 B/float.
 * stats (3 K + 2 device int64): drawn[i] = #keep_i (a function of seed, streams[i], drop_thr[i] and n only); kept[i] = #(|d_i| >= thr[i] &&
 * keep_i); won[i], support and conflict as in vd_merge_apply.  VD_DROP_COPY: kept[0] = won[0] = drawn[0], support = #(keep_0 and tasks[0][j]
 * != base[j] as floats), conflict = 0.  Per-workgroup uint32 counts go to partial (>= (3 K + 2) * 1024 uint32), a one-workgroup finish adds
 * them in 64 bits.  No float atomics and no global atomics.
 * out may be exactly base or exactly one tasks[i], otherwise it overlaps none of them; the inputs may be one another.  4 (K + 2) B/float.
 * VD_EINVAL before any launch: everything vd_merge_apply refuses, a NULL drop_thr or streams, drop_thr[i] > 2^32, VD_DROP_RESCALE with a NULL
 * or non-finite rescale[i], unknown flag bits, VD_DROP_COPY with VD_DROP_RESCALE, with K != 1 or with a mode other than VD_MERGE_LINEAR. */
enum { VD_DROP_RESCALE = 1, VD_DROP_COPY = 2 };
int vd_merge_apply_drop(float* out, const float* base, const float* const* tasks, const float* lam, const float* thr, const uint64_t* drop_thr,
                        const float* rescale, const uint32_t* streams, int K, int64_t n, int mode, float lam_out, uint64_t seed, int flags,
                        uint32_t* partial, int64_t* stats, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10 -- sampler steps (diffusers *Scheduler.step, via pipeline(...) VillanDiffusion.py:579).
 *   x0 = (x - c_eps*eps) / c_div ; clamp(+-clip) when clip > 0 ; out = c_x0*x0 + c_x*x + c_e*eps + c_z*z
 * every product/sum individually rounded (no FMA contraction) so results match the torch op sequence bit for bit.
 * z: noise pointer, or NULL with (seed, offset) for the on-device Philox4x32-10 + Box-Muller stream (c_z != 0).
 * ------------------------------------------------------------------------------------------ */
int vd_sched_step(const float* x, const float* eps, const float* z, float* out, float* x0_out, int64_t n,
                  float c_eps, float c_div, float clip, float c_x0, float c_x, float c_e, float c_z,
                  uint64_t seed, uint64_t offset, void* stream);
/* out[b] = sqrt(sum_i x[b][i]^2): per-sample L2 norms (ScoreSDE-VE corrector step size, diffusers step_correct). */
int vd_batch_l2norm(const float* x, float* out, int B, int64_t inner, void* stream);
/* out = clamp(x*mul + add, lo, hi), optionally NCHW -> NHWC (pipeline post-processing). */
int vd_postprocess(const float* x, float* out, int B, int C, int HW, float mul, float add, float lo, float hi,
                   int to_nhwc, void* stream);
/* out[n] = mean over the SSIM map of image pair n (a, b: [N, C, H, W]; win: the K x K gaussian window, K odd <= 32): torchmetrics'
 * StructuralSimilarityIndexMeasure(data_range) as measure() uses it (reference VillanDiffusion.py:1001-1007): reflect padding whose border is
 * cropped from the map; c1 = (0.01 data_range)^2, c2 = (0.03 data_range)^2. */
int vd_ssim(const float* a, const float* b, const float* win, float* out, int N, int C, int H, int W, int K, float c1, float c2,
            void* stream);
/* VQ-VAE quantiser (diffusers VectorQuantizer.forward, reached through VQModel.decode: reference loss.py:951-962,
 * model.py:713): zq[b][:, p] = codebook[argmin_e |z[b][:, p] - e|^2], idx[b*HW + p] = that e (may be NULL).
 * z / zq: [B, D, HW] with batch strides, codebook [n_e, D], D <= 16. */
int vd_vq_nearest(const float* z, const float* codebook, float* zq, int64_t* idx, int B, int D, int HW, int n_e,
                  int64_t z_bstride, int64_t q_bstride, void* stream);
/* NCSN++ (SDE-VE score network, reference model.py:839-894) helpers.
 * vd_fir_resample2: diffusers upsample_2d / downsample_2d with the (1,3,3,1) FIR kernel, factor 2, on `planes` images of
 *   H x W; out = scale * resample(x) (+ out).  The adjoints are the same kernels: d(up)^T g = 4 down(g), d(down)^T g = up(g)/4.
 * vd_fourier_embedding: GaussianFourierProjection(log=True): emb[b] = [sin(log t_b W 2pi), cos(log t_b W 2pi)].
 * vd_rowscale: out[b][:] = x[b][:] * s[b] (divide=0) or / s[b] (divide=1)  (UNet2DModel's final `sample / timesteps`). */
int vd_fir_resample2(const float* x, float* out, int64_t planes, int H, int W, int up, float scale, int accumulate, void* stream);
/* Gradient of one level of NCSN++'s input-image pyramid with respect to its image (h = skip_conv(image) + ..., image_next = FIRdown(image)):
 *   out[b][c][h][w] = sum_k w[k][c] * g[b][k][h][w]  +  0.25 * FIRup(coarse)[b][c][h][w] (coarse non-NULL)  (+ out, accumulate != 0)
 * g: [B, K, H, W] with batch stride g_bstride >= K*H*W (a channel slice of a wider gradient is fine); w: [K, C], the 1x1 weight, C <= 4;
 * coarse: the next level's gradient [B, C, H/2, W/2] or NULL; out: contiguous [B, C, H, W].  Exact f32, k summed in a fixed order, no
 * atomics: bit-reproducible, and a strided g gives the bits of its contiguous copy.  The FIR taps are vd_fir_resample2's (up = 1). */
int vd_pyramid_dgrad(const float* g, const float* w, const float* coarse, float* out, int B, int K, int C, int H, int W,
                     int64_t g_bstride, int accumulate, void* stream);
int vd_fourier_embedding(const float* t, const float* W, float* emb, int B, int half, void* stream);
int vd_rowscale(const float* x, const float* s, float* out, int B, int64_t inner, int divide, void* stream);
/* z ~ N(0,1) from Philox4x32-10 (throughput mode noise). */
int vd_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);

/* ------------------------------------------------------------------------------------------
 * K11 -- trigger stamping on the GPU (dataset.py:475-545 + util.py:119-147).
 * img: uint8 NHWC dataset resident in HBM; idx[b] (nullable = identity) selects the sample of batch slot b (fused
 * gather); flags: bit0 = poisoned, bit1 = horizontal flip.
 *   x = norm(img) ; clean: pixel_values=0, target=x ; poisoned: pixel_values=mask?x:trigger, target=target
 * ------------------------------------------------------------------------------------------ */
int vd_poison_batch(const uint8_t* img, const int64_t* idx, const uint8_t* flags, const float* trigger, const float* target,
                    float* pixel_values, float* tgt_out, float* image_out, int B, int C, int H, int W, float vmin,
                    float vmax, int R_trigger_only, void* stream);

/* ------------------------------------------------------------------------------------------
 * FID feature extractor (reference fid_score.py:91-148 -> pytorch-fid InceptionV3): the convolutions run
 * through vd_gemm (VD_B_CONVG / VD_B_PLAIN with act = 1 over BatchNorm-folded weights); these are the remaining ops.
 * ------------------------------------------------------------------------------------------ */
/* 3x3 pooling of NCHW planes: mode 0 = F.max_pool2d, 1 = F.avg_pool2d(count_include_pad=False); stride 1 | 2, pad 0 | 1.
 * y has (H + 2 pad - 3) / stride + 1 rows; bstrides in elements (channel slices of wider buffers are allowed). */
int vd_pool3(const float* x, float* y, int B, int C, int H, int W, int stride, int pad, int mode, int64_t x_bstride, int64_t y_bstride,
             void* stream);
/* y = mul * F.interpolate(x, (OH, OW), mode="bilinear", align_corners=False) + add over `planes` contiguous H x W planes. */
int vd_resize_bilinear(const float* x, float* y, int64_t planes, int H, int W, int OH, int OW, float mul, float add, void* stream);

/* ------------------------------------------------------------------------------------------
 * LPIPS (reference VillanDiffusion.py:892 -> lpips.LPIPS(net='alex')): the AlexNet convolutions run through vd_gemm
 * (VD_B_CONVG with act = 1) and vd_pool3; these are the remaining ops.
 * ------------------------------------------------------------------------------------------ */
/* y[b][c][:] = x[b][c][:] * mul[c] + add[c] over contiguous [B][C][HW] tensors (the input ScalingLayer). */
int vd_channel_affine(const float* x, const float* mul, const float* add, float* y, int B, int C, int HW, void* stream);
/* One tap of the metric on contiguous [N][C][HW] feature maps: out[n] (+)= mean_p sum_c w[c] * (unit(f0)[n][c][p] - unit(f1)[n][c][p])^2,
 * unit(f) = f / (sqrt(sum_c f^2) + 1e-10). */
int vd_lpips_layer(const float* f0, const float* f1, const float* w, float* out, int N, int C, int HW, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VILLAN_HIP_H */
