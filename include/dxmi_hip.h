/*
 * dxmi_hip.h — C-ABI of libdxmi_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for
 * the DxMI few-step sampling / training hot path.
 *
 * The reference (swyoon/Diffusion-by-MaxEntIRL) is pure Python on torch.nn and has NO FFI of
 * its own; every entry point below therefore names the reference *Python* call site whose
 * torch ops it replaces (file:line relative to the reference root).  The Python host modules
 * under diffusion-by-maxentirl_amd/models/ bind these symbols through ctypes
 * (diffusion-by-maxentirl_amd/dxmi_hip/_lib.py); INTEGRATION.md shows the stub a maintainer
 * of the reference would add.
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = DXMI_E* ; dxmi_last_error() gives text.
 *   - pointers are raw DEVICE pointers (tensor.data_ptr()); the caller owns all memory.
 *     The library allocates nothing on the device and never synchronises.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every launch is asynchronous on it, so all calls are hipGraph-capturable.
 *   - activations between kernels: NHWC bf16.  Sampler state / network edges: NCHW fp32.
 *   - no exceptions cross the boundary; functions are re-entrant.
 *   - NOT in this header: the gradient exchange of the data-parallel train step (reference: torch DDP wrappers,
 *     train_cifar10.py:298-309).  The host stays PyTorch, so the collectives are issued through torch.distributed with the
 *     "nccl" backend (= RCCL on ROCm) by dxmi_hip/dist.py (FlatGradSync: persistent flat buffer, ~32 MB buckets all-reduced
 *     during the backward); this library only produces the gradients those buckets carry.  Generation needs no collective.
 */
#ifndef DXMI_HIP_H
#define DXMI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DXMI_OK            0
#define DXMI_EINVAL       -1   /* bad shape / unsupported configuration */
#define DXMI_ELAUNCH      -2   /* hipLaunch failed */
#define DXMI_ENODEV       -3   /* no gfx950 device visible */

#define DXMI_ACT_NONE      0
#define DXMI_ACT_LEAKY02   1   /* leaky_relu(x, 0.2)  — models/modules.py:84,101,145 */
#define DXMI_ACT_RELU      2   /* relu               — models/modules.py:150 */
#define DXMI_ACT_SILU      3   /* x*sigmoid(x)       — models/DxMI/unet_small.py:30 */

#define DXMI_IN_NHWC_BF16     0
#define DXMI_IN_NCHW_F32_K27  1  /* 3-channel NCHW fp32 image, 3x3/s1/p1 im2col'd to K=27(+5 zero) */
#define DXMI_IN_ROWS_F32      2  /* internal: fp32 row-major [P,K] (dxmi_linear_fwd) */
#define DXMI_OUT_NHWC_BF16    0
#define DXMI_OUT_NCHW_F32     1
#define DXMI_OUT_ROWS_F32     2  /* internal: fp32 row-major [P,M] (dxmi_linear_fwd) */

const char* dxmi_last_error(void);
int dxmi_version(void);
/* 0 when a gfx950 device is usable; DXMI_ENODEV otherwise (never falls back to CPU). */
int dxmi_device_check(void);
/* Kernel-selection knobs (process-wide; initial value from the environment variable in brackets).  They choose between kernels
 * that compute the same convolution (same operands, fp32 accumulation; the summation order inside a K extent differs between
 * kernels, i.e. results agree to rounding, not bit for bit); unknown names return DXMI_EINVAL.
 *   "conv_ws_min_tiles" [DXMI_CONV_WS_MIN_TILES, 0]: 3x3 convs with fewer (256-pixel, 128-cout) tiles run on the 64-pixel-tile
 *                        kernel instead of the wave-specialised one (small batches leave most CUs without a tile);
 *   "conv_sm_mask"      [DXMI_CONV_SM, 9]: bit 0 4x4 maps, bit 1 every 8x8 map, bit 2 8x8 maps whose 256-pixel-tile grid is
 *                        under-filled, bit 3 8x8 maps with >= 1024 channels in and out (a rule on the layer shape, not on the
 *                        batch), on the feed-tiled small-map kernel.
 *   "gn_bwd_fused"      [DXMI_GN_BWD_FUSED, 1]: dxmi_groupnorm_generic_bwd[_saved] as ONE launch that keeps a workgroup's rows
 *                        in registers across an in-launch per-image hand-off, on maps of <= 256 pixels where it measured faster
 *                        (2: on every shape it fits; 0: the reduce + apply launches of rounds 2-5 everywhere).
 * Defaults: one kernel per layer shape whatever the batch size, so an image's result does not depend on the batch it rides in.
 * The training entry points set 96 / 13 (throughput at small per-GPU batches; +5..8 % on the EDM train step).  The answers of
 * dxmi_conv2d_gn_stats_partials / dxmi_conv2d_gn_fuse_supported depend on the knobs: query again after changing one.
 * No reference counterpart (the reference leaves algorithm choice to cuDNN). */
int dxmi_set_tuning(const char* name, int32_t value);
int dxmi_get_tuning(const char* name, int32_t* value);

/* ------------------------------------------------------------------------------------------
 * Convolution as MFMA implicit GEMM (bf16 operands, fp32 accumulate), fused epilogue.
 * Replaces torch.nn.Conv2d / F.pad+conv / F.interpolate+conv / torch.cat+conv at
 *   models/DxMI/unet_small.py:50-54 (Upsample), :69-76 (Downsample, pad (0,1,0,1) + k3 s2),
 *   :117-136 (ResnetBlock conv1/conv2/nin_shortcut + temb add + residual),
 *   :167-191 (AttnBlock q,k,v,proj_out 1x1), :302, :321-322 (cat(h, skip)), :331 (conv_out);
 *   models/modules.py:71-101 (ResBlockV2 conv1/conv2/skip), :142-145 (IGEBMEncoderV2.conv1).
 * Weights are pre-packed into MFMA A-fragment order by dxmi_pack_conv_weight().
 * ---------------------------------------------------------------------------------------- */
typedef struct dxmi_conv_desc {
    const void*  in0;        /* NHWC bf16 [N,IH,IW,C0]  (or NCHW f32 [N,3,IH,IW] for K27 mode) */
    const void*  in1;        /* second concat source NHWC bf16 [N,IH,IW,C1] or NULL */
    const void*  wpacked;    /* from dxmi_pack_conv_weight */
    const float* bias;       /* [Cout] or NULL */
    const float* addvec;     /* per-(n,co) additive term (temb_proj output) [N,addvec_ld] or NULL */
    const void*  residual;   /* NHWC bf16 [N,OH,OW,Cout] added before activation, or NULL */
    void*        out;        /* NHWC bf16 [N,OH,OW,Cout] or NCHW f32 [N,Cout,OH,OW] */
    int32_t N, IH, IW, C0, C1;
    int32_t OH, OW, Cout;
    int32_t ksize;           /* 1 or 3 */
    int32_t stride;          /* 1 or 2 */
    int32_t pad;             /* top/left zero padding (bottom/right padding is implied by OH/OW) */
    int32_t upsample;        /* 1: input is nearest-upsampled x2 before the conv; 2: zero-stuffed x2 (the
                                data gradient of a stride-2 conv is a stride-1 conv over the stuffed dY) */
    int32_t act;             /* DXMI_ACT_* applied last */
    int32_t addvec_ld;       /* row stride of addvec in floats: >= Cout, or 0 = one row shared by the whole batch */
    int32_t in_mode;         /* DXMI_IN_*  */
    int32_t out_mode;        /* DXMI_OUT_* */
    int32_t variant;         /* 0 = default tiling; >0 selects an alternative (tuning / tests) */
    const void*  mask_src;   /* backward use: NHWC bf16 tensor shaped like out; result *= (mask_src > 0 ? 1 : mask_slope)
                                after bias/residual, i.e. the LeakyReLU/ReLU derivative of a saved activation; or NULL */
    float        mask_slope;
    float*       gn_stats;   /* optional output: GroupNorm block statistics of `out` for the Normalize() that consumes it
                                (unet_small.py:35-36,119-126): fp32 [N][P][Cout/2][2] = (sum, sum of squares) of the STORED bf16
                                values over the pixels of partial p of the image, per PAIR of consecutive channels, summed in a
                                fixed order inside the conv's epilogue (bitwise reproducible).  P = dxmi_conv2d_gn_stats_partials(d);
                                NULL = not wanted.  Setting it for a shape whose kernel cannot produce them is DXMI_EINVAL. */
    /* optional: GroupNorm(+SiLU) of the conv's OUTPUT fused into its epilogue, for shapes whose workgroup tile holds whole
       images and whole groups (the 4x4 maps of the U-Net, and the 8x8 maps when gn_flags bit 1 drops the raw output:
       Normalize()+nonlinearity of the next layer, unet_small.py:119-126):
       gn_out = silu?(group_norm(round_bf16(out))) with statistics in fp32 (two-pass, from registers), bitwise independent of
       the batch.  gn_out NULL = off.  dxmi_conv2d_gn_fuse_supported(d) says whether the selected kernel can; setting it for a
       shape that cannot is DXMI_EINVAL. */
    void*        gn_out;     /* NHWC bf16 [N,OH,OW,Cout] */
    const float* gn_gamma;   /* [Cout] */
    const float* gn_beta;    /* [Cout] */
    float        gn_eps;
    int32_t      gn_groups;  /* Cout / gn_groups must be 8 */
    int32_t      gn_flags;   /* bit 0: SiLU after the affine; bit 1: do not write `out` (the raw tensor has no other reader);
                                bit 2: the caller also takes the wave-specialised 3x3 kernel's fused output (conv_ws_gn_kernel: 16x16
                                maps, Cout % 128 == 0, no residual / mask / upsample, together with bit 1).  There gn_out is
                                bitwise what dxmi_groupnorm_apply gives on the conv's output and gn_stats (block statistics in
                                fp32, a pair's partials in partial order, a group's pairs in channel order).  Without bit 2 the
                                selection and dxmi_conv2d_gn_fuse_supported answer as they did before the bit existed. */
} dxmi_conv_desc;

int dxmi_conv2d_fwd(const dxmi_conv_desc* d, void* stream);
/* 1 when the kernel dxmi_conv2d_fwd would launch for `d` can fuse the GroupNorm of its output (gn_out ...), else 0. */
int dxmi_conv2d_gn_fuse_supported(const dxmi_conv_desc* d);
/* Measurement aid (round 5): (s_memtime, s_memrealtime) at the first and the last instruction of workgroup 0 of the most recent
 * wave-specialised 3x3 conv launch (conv_ws_kernel), copied to host memory: host_out4 = {cycles0, ref0, cycles1, ref1}; the shader
 * clock the chip held during that launch is (cycles1 - cycles0) / (ref1 - ref0) x 100 MHz.  Synchronises (a device-to-host copy). */
int dxmi_conv_ws_last_clock(unsigned long long* host_out4);
/* Partials per image (P above) the kernel dxmi_conv2d_fwd would launch for `d` writes into d->gn_stats; 0 = that kernel
 * does not produce block statistics (use dxmi_gn_block_stats on its output, or the one-pass dxmi_groupnorm_silu_fwd). */
int dxmi_conv2d_gn_stats_partials(const dxmi_conv_desc* d);
/* Template instantiation dxmi_conv2d_fwd would launch (MB*1000+NB*100+PMAX), no launch; <0 on error. */
int dxmi_conv2d_kernel_id(const dxmi_conv_desc* d);

/* Packs an fp32 OIHW weight [Cout,Cin,k,k] (device) into bf16 A-fragment order
 * [tap][Cin/16][ceil(Cout/32)][64 lanes][8].  transpose_flip=1 packs the data-gradient
 * (flipped, Cin<->Cout) operator instead.  k27=1 packs the Cin=3,k=3 im2col form.
 * dst must hold dxmi_packed_conv_weight_bytes(...) bytes. */
int64_t dxmi_packed_conv_weight_bytes(int32_t Cout, int32_t Cin, int32_t ksize, int32_t k27);
int dxmi_pack_conv_weight(const float* w_oihw, void* dst, int32_t Cout, int32_t Cin,
                          int32_t ksize, int32_t transpose_flip, int32_t k27, void* stream);

/* Multi-tensor form of dxmi_pack_conv_weight: `count` weights (a HOST array of descriptors; the library cuts it into launches
 * of DXMI_PACK_MAX items passed by value) — after an optimiser step (trainer.py:264, :325, :389; fp16_util.py:204-223) every
 * packed weight of a net is refreshed by a handful of launches instead of one per layer. */
#define DXMI_PACK_MAX 32
typedef struct dxmi_pack_item {
    const float* w;          /* fp32 OIHW [Cout,Cin,k,k] (transpose_flip: the ORIGINAL tensor [Cin_logical][Cout_logical][k][k]) */
    void*        dst;        /* dxmi_packed_conv_weight_bytes(Cout, Cin, ksize, k27) bytes */
    int32_t Cout, Cin, ksize, transpose_flip, k27;
} dxmi_pack_item;
int dxmi_pack_conv_weights(const dxmi_pack_item* items, int32_t count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the convolutions (training path: models/DxMI/trainer.py:261,322,387 call
 * .backward() through the value network and the U-Net).
 *  - data gradient: dxmi_conv2d_fwd with weights packed by dxmi_pack_conv_weight(transpose_flip=1)
 *    (stride-1 convs; mask_src/mask_slope fuse the activation derivative, residual fuses the
 *    skip-path gradient).
 *  - weight gradient: dxmi_conv2d_wgrad: dW[co][ci][ky][kx] = sum_p dY[p][co] X[p+tap][ci] as an MFMA
 *    GEMM over the pixel index (ds_read_b64_tr_b16 transposed fragments, split-K over pixel tiles,
 *    fixed-order reduction).  x0|x1: forward input (virtual concat), dy: output gradient, both NHWC
 *    bf16; dw_oihw fp32 [Cout,Cin,k,k]; accumulate != 0 adds into dw_oihw.
 *  - bias gradient: dxmi_colsum_bf16 over dy viewed as [P, C].
 * ---------------------------------------------------------------------------------------- */
int64_t dxmi_conv2d_wgrad_workspace_bytes(int32_t N, int32_t OH, int32_t OW, int32_t Cin, int32_t Cout,
                                          int32_t ksize);
int dxmi_conv2d_wgrad(const void* x0, int32_t C0, const void* x1, int32_t C1, const void* dy,
                      float* dw_oihw, void* workspace, int32_t N, int32_t IH, int32_t IW, int32_t OH,
                      int32_t OW, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, int32_t upsample,
                      int32_t accumulate, void* stream);
/* The kernel dxmi_conv2d_wgrad[_bias] launches for a shape (the launch makes its choice through this same function):
 * out4 = {family, S, PT, reduce}.  S: pixel splits (partial sums added by the reduce in split order), PT: pixel tiles (128
 * pixels, zero-padded past the last image; 64 for DXMI_WGRAD_1X1_B128), split s sums tiles s, s + S, ...  Reflects the
 * DXMI_WGRAD_* environment overrides.  DXMI_EINVAL for the shapes the launch rejects. */
#define DXMI_WGRAD_1X1_B128      0   /* conv_wgrad1x1_b128_kernel: 128 co x 128 ci blocks, DMA-staged 64-pixel tiles */
#define DXMI_WGRAD_WS3           1   /* conv_wgrad_ws_kernel<3>: wave-specialised, DMA-staged */
#define DXMI_WGRAD_WS1           2   /* conv_wgrad_ws_kernel<1> */
#define DXMI_WGRAD_REG3_PF       3   /* conv_wgrad_kernel<3, true>: register-staged, next tile prefetched */
#define DXMI_WGRAD_REG3          4   /* conv_wgrad_kernel<3, false> */
#define DXMI_WGRAD_REG1_PF       5   /* conv_wgrad_kernel<1, true> */
#define DXMI_WGRAD_REG1          6   /* conv_wgrad_kernel<1, false> */
#define DXMI_WGRAD_REDUCE_TAPS4  0   /* wgrad_reduce_kernel<4, taps>: all taps per thread, S in 4 slices */
#define DXMI_WGRAD_REDUCE_TAPS16 1   /* wgrad_reduce_kernel<16, taps> */
#define DXMI_WGRAD_REDUCE_FLAT4  2   /* wgrad_reduce_flat_kernel<4> */
#define DXMI_WGRAD_REDUCE_FLAT16 3   /* wgrad_reduce_flat_kernel<16> */
int dxmi_conv2d_wgrad_plan(int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW, int32_t C0, int32_t C1, int32_t Cout,
                           int32_t ksize, int32_t stride, int32_t pad, int32_t upsample, int32_t* out4);
/* Same plus the bias gradient dbias[co] = sum_p dY[p][co] (fp32 [Cout]), summed from the dY tiles the kernel stages
 * anyway (replaces a separate column-sum pass over dY; trainer.py's loss.backward() for nn.Conv2d.bias). */
int dxmi_conv2d_wgrad_bias(const void* x0, int32_t C0, const void* x1, int32_t C1, const void* dy, float* dw_oihw,
                           float* dbias, void* workspace, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW,
                           int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, int32_t upsample,
                           int32_t accumulate, void* stream);
/* workspace: ceil(P/512) * C floats */
int dxmi_colsum_bf16(const void* x, float* out, void* workspace, int64_t P, int32_t C,
                     int32_t accumulate, void* stream);
/* out[b][c] = sum of rows [b*rows_per_block, (b+1)*rows_per_block) of x[P][C] (per-image channel sums). */
int dxmi_colsum_blocks_bf16(const void* x, float* out, int64_t P, int32_t C, int32_t rows_per_block,
                            void* stream);
/* out[b][c] = sum_n in[b][n][c], fp32, fixed order (the [2][N][C] per-image d(gamma) / d(beta) partials of
 * dxmi_groupnorm_silu_bwd -> [2][C]). */
int dxmi_colsum_f32(const float* in, float* out, int32_t B, int32_t N, int32_t C, void* stream);

/* Backward of GroupNorm(+SiLU) (training path).  x = [in0 | in1] and dy (gradient w.r.t. the forward
 * kernel's output, one dense [N,HW,C0+C1] tensor) -> dx0 [N,HW,C0], dx1 [N,HW,C1] (+ add0/add1 fused:
 * skip-connection / residual gradients), and per-image partial sums dgamma_part/dbeta_part [N,C] fp32
 * (sum over dim 0 gives the parameter gradients).  Statistics are recomputed, nothing is saved by the
 * forward.  Replaces autograd through unet_small.py:119-126,169,329-330. */
int dxmi_groupnorm_silu_bwd(const void* in0, int32_t C0, const void* in1, int32_t C1, const void* dy,
                            const void* add0, const void* add1, const float* gamma, const float* beta,
                            void* dx0, void* dx1, float* dgamma_part, float* dbeta_part, int32_t N,
                            int32_t HW, int32_t groups, float eps, int32_t apply_silu, void* stream);
/* 1 when dxmi_groupnorm_silu_bwd can serve the shape (x and dy both stay resident, so its limits are tighter than the
 * forward's), else 0 — use dxmi_groupnorm_generic_bwd then. */
int dxmi_groupnorm_silu_bwd_supported(int32_t C0, int32_t C1, int32_t HW, int32_t groups);

/* Batched bf16 GEMM on MFMA for attention backward: C[b] = alpha * A[b] (MxK) * B[b] (KxN), batch
 * b = (outer, inner) with element strides *_b0 / *_b1.  *_kcontig != 0: element (row,k) of that operand
 * is at row*ld + k; == 0: at k*ld + row (read through transposing LDS loads).  C row-major [M,N] with
 * c_ld, fp32 or bf16.  dxmi_softmax_bwd: per row of length T, P = softmax(S), dS = P o (dP - <dP,P>). */
int dxmi_bgemm_bf16(const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t a_b0,
                    int64_t a_b1, int32_t a_ld, int32_t a_kcontig, int64_t b_b0, int64_t b_b1, int32_t b_ld,
                    int32_t b_kcontig, int64_t c_b0, int64_t c_b1, int32_t c_ld, int32_t c_f32, float alpha,
                    int32_t outer, int32_t inner, void* stream);
int dxmi_softmax_bwd(const float* S, const float* dP, void* P, void* dS, int64_t rows, int32_t T,
                     void* stream);

/* Fused attention backward (round 4) for head dimension 64 (every attention block of the ADM / EDM nets,
 * models/cm/unet.py:413-441): dqkv [N,T,3C] from qkv [N,T,3C], the forward output o [N,T,C] and its gradient dout [N,T,C]
 * (bf16), without any [T,T] tensor in HBM: the probabilities are recomputed from the row log-sum-exp (first kernel, which also
 * forms delta = <dO, O> and dQ), then dK / dV per key block (second kernel).  Fixed summation orders: bitwise reproducible.
 * workspace: dxmi_attention_bwd_workspace_bytes(N, T, heads) bytes.  dxmi_attention_bwd_supported: 1 when C / heads == 64
 * (other head sizes: the dxmi_bgemm_bf16 / dxmi_softmax_bwd sequence above). */
int dxmi_attention_bwd_supported(int32_t T, int32_t C, int32_t heads);
int64_t dxmi_attention_bwd_workspace_bytes(int32_t N, int32_t T, int32_t heads);
int dxmi_attention_bwd(const void* qkv, const void* o, const void* dout, void* dqkv, void* workspace, int32_t N, int32_t T,
                       int32_t C, int32_t heads, float scale, void* stream);

/* The saved softmax statistics of autograd's attention node (round 6): dxmi_attention_fwd_lse is dxmi_attention_fwd that also leaves the
 * row log-sum-exp of the scaled logits (log2 domain: max + log2(sum) of scale * log2(e) * q.k; fp32 [N][heads][T]); dxmi_attention_bwd_lse
 * is dxmi_attention_bwd taking it, one sweep over the keys shorter.  _supported: every shape of dxmi_attention_fwd except the
 * single-head 256-token x 256-channel block.  Replaces models/cm/unet.py:413-441 under autograd. */
int dxmi_attention_fwd_lse_supported(int32_t T, int32_t C, int32_t heads);
int dxmi_attention_fwd_lse(const void* qkv, void* out, float* lse, int32_t N, int32_t T, int32_t C, int32_t heads, float scale, void* stream);
int dxmi_attention_bwd_lse(const void* qkv, const void* o, const void* dout, void* dqkv, const float* lse_fwd, void* workspace, int32_t N,
                           int32_t T, int32_t C, int32_t heads, float scale, void* stream);

/* Backward of dxmi_pool_act: din = (pool ? 0.25 * upsample2(g) : g), g = dout * (act_out > 0 ? 1 : slope);
 * dout/act_out: [N,OH,OW,C], din: [N,H,W,C] (H = 2*OH when pool). */
int dxmi_pool_act_bwd(const void* dout, const void* act_out, void* din, int32_t N, int32_t H, int32_t W,
                      int32_t C, int32_t pool, float slope, void* stream);
/* Backward of the value head w.r.t. its feature map: dfeat[n,p,c] = dy[n] * w[c] * (feat > 0); also
 * returns s[n,c] = sum_p relu(feat[n,p,c]) (fp32) from which the caller forms the tiny parameter
 * gradients. */
int dxmi_value_head_bwd(const void* feat, const float* w, const float* dy, void* dfeat, float* s,
                        int32_t N, int32_t HW, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm (+ optional SiLU) over NHWC bf16, optionally over a virtual concat of two
 * tensors.  One pass over HBM: a workgroup keeps its (image, channel-slice) in registers,
 * two-pass mean/variance in fp32 with wavefront shuffles + LDS.
 * Replaces Normalize()+nonlinearity at models/DxMI/unet_small.py:35-36,119-120,125-126,
 * 169,329-330 (eps 1e-6) and GroupNorm32 at models/cm/nn.py:19-21 (eps 1e-5).
 * ---------------------------------------------------------------------------------------- */
int dxmi_groupnorm_silu_fwd(const void* in0, int32_t C0, const void* in1, int32_t C1,
                            const float* gamma, const float* beta, void* out,
                            int32_t N, int32_t HW, int32_t groups, float eps,
                            int32_t apply_silu, void* stream);

/* GroupNorm(+SiLU) as ONE streaming read + write, given block statistics of the input(s) (the statistics pass of
 * Normalize() / GroupNorm32 is folded into whatever produced the tensor: dxmi_conv_desc.gn_stats, or dxmi_gn_block_stats):
 *   stats0 / stats1: fp32 [N][P0|P1][C0|C1 / 2][2] (sum, sum of squares per channel pair and partial).  Every workgroup
 *   re-reduces its image's partials in a fixed order (pair outer, partial inner), mean = s/cnt, var = max(q/cnt - mean^2, 0),
 *   then streams its rows: y = x*(rstd*gamma) + (beta - mean*rstd*gamma), optional FiLM scale-shift
 *   (y*(1+scale[n,c]) + shift[n,c]: scale_shift fp32 [N, ss_ld], scale at [c], shift at [C + c]; models/cm/unet.py:252-256),
 *   optional SiLU, one rounding to bf16.
 * Channels per group must be even, C0 and C1 multiples of 8.  No residency limit on HW.
 * dxmi_gn_block_stats: the statistics of a tensor that has no producer-side statistics: x [N,HW,C] -> stats
 *   [N][P][C/2][2] with P = dxmi_gn_block_stats_partials(HW) row chunks per image.
 * dxmi_gn_stats_fold: [N][P][C/2][2] -> [N][ceil(P/group)][C/2][2], `group` consecutive partials added in order (large maps:
 *   a conv writes one partial per 128-pixel half tile — 512 per 256x256 image — too many for every apply workgroup to
 *   re-add); C = floats per partial (= channels). */
int dxmi_gn_block_stats_partials(int32_t HW);
int dxmi_gn_block_stats(const void* x, float* stats, int32_t N, int32_t HW, int32_t C, void* stream);
int dxmi_gn_stats_fold(const float* stats, float* out, int32_t N, int32_t P, int32_t C, int32_t group, void* stream);
int dxmi_groupnorm_apply(const void* in0, int32_t C0, const float* stats0, int32_t P0, const void* in1, int32_t C1,
                         const float* stats1, int32_t P1, const float* gamma, const float* beta, const float* scale_shift,
                         int32_t ss_ld, void* out, int32_t N, int32_t HW, int32_t groups, float eps, int32_t apply_silu,
                         void* stream);

/* dxmi_groupnorm_apply as TWO launches (round 6): a one-workgroup-per-image kernel forms the per-(image, channel) scale / offset
 * pairs (statistics partials -> group mean / rstd -> gamma, beta and the FiLM scale-shift folded in) into ab_workspace
 * (N * (C0 + C1) * 2 floats), and the streaming pass reads them instead of running that prologue in every one of its workgroups.
 * Same operations in the same order: bit-identical output.  Pays when the extra launch is cheap (a node of a replayed hipGraph). */
int dxmi_groupnorm_apply_split(const void* in0, int32_t C0, const float* stats0, int32_t P0, const void* in1, int32_t C1,
                               const float* stats1, int32_t P1, const float* gamma, const float* beta,
                               const float* scale_shift, int32_t ss_ld, void* out, float* ab_workspace, int32_t N, int32_t HW,
                               int32_t groups, float eps, int32_t apply_silu, void* stream);

/* GroupNorm(+SiLU) of [in0 | in1] AND the 1x1 convolution `d` of the same input in one pass over it (a ResnetBlock's norm1 and
 * nin_shortcut): d is the shortcut's descriptor as dxmi_conv2d_fwd takes it (in0 / in1 / C0 / C1 the input, out the shortcut
 * output), stats0 / stats1 the input's block statistics as dxmi_groupnorm_apply takes them, y the normalised tensor [N, H, W, C0 + C1],
 * ab_workspace N * (C0 + C1) * 2 floats.  y is bitwise dxmi_groupnorm_apply's output, out bitwise dxmi_conv2d_fwd's.  Returns 1 and
 * launches nothing when the pair is out of scope (dxmi_groupnorm_silu_shortcut_supported returns 0): the caller runs the two ops. */
int dxmi_groupnorm_silu_shortcut_supported(const dxmi_conv_desc* d, int32_t groups);
int dxmi_groupnorm_silu_shortcut(const dxmi_conv_desc* d, const float* stats0, int32_t P0, const float* stats1, int32_t P1,
                                 const float* gamma, const float* beta, int32_t groups, float eps, int32_t apply_silu, void* y,
                                 float* ab_workspace, void* stream);

/* Block statistics ([N][P][C/2][2], as dxmi_conv_desc.gn_stats / dxmi_gn_block_stats write them; st1 for the second part of a virtual
 * concat or NULL) -> the statistics partials of the generic GroupNorm kernels (dxmi_groupnorm_generic_workspace_bytes(N, HW, C) bytes:
 * what dxmi_groupnorm_generic_bwd_saved takes as fwd_stats): a training forward that normalised with dxmi_groupnorm_apply hands the
 * generic backward the same sums without another pass over the input. */
int dxmi_gn_blockstats_to_generic(const float* stats0, int32_t P0, int32_t C0, const float* stats1, int32_t P1, int32_t C1,
                                  float* generic_stats, int32_t N, int32_t HW, int32_t groups, void* stream);

/* Parameter and FiLM gradients of a scale-shift GroupNorm from dxmi_groupnorm_generic_bwd's g_out [2][N][C] in one launch:
 * d_scale_shift [N][2C] = (G1 gamma + G0 beta | G0), dgamma [C] = sum_n G1 (1 + scale), dbeta [C] = sum_n G0 (1 + scale); scale_shift as the
 * backward took it ([N][ss_ld], scale first).  Replaces the reference's autograd of models/cm/unet.py:252-256. */
int dxmi_gn_ss_grads(const float* g, const float* scale_shift, int32_t ss_ld, const float* gamma, const float* beta,
                     float* d_scale_shift, float* dgamma, float* dbeta, int32_t N, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Single-/multi-head self-attention over a fused qkv tensor, MFMA QK^T and PV with an
 * online softmax.  qkv: NHWC bf16 [N,T,3*C] laid out [q | k | v] along channels, heads are
 * contiguous channel blocks of size C/heads.  out: [N,T,C] bf16.  scale multiplies q.k.
 * Replaces models/DxMI/unet_small.py:175-187 (bmm/softmax/bmm, scale C^-0.5) and
 * models/cm/unet.py:413-441 (QKVAttentionLegacy).
 * ---------------------------------------------------------------------------------------- */
int dxmi_attention_fwd(const void* qkv, void* out, int32_t N, int32_t T, int32_t C,
                       int32_t heads, float scale, void* stream);

/* AttnBlock tail fused behind the attention (reference unet_small.py:187-190: h_ = proj_out(h_); return x + h_), for the
 * single-head 256-token x 256-channel block of the CIFAR-10 net (dxmi_attention_proj_supported): the attention output never
 * leaves the CU — it stays in registers as the MFMA operand of the 1x1 projection — and out = x + proj_out(attention) + bias is
 * written once.  Same arithmetic as dxmi_attention_fwd followed by dxmi_conv2d_fwd (attention output rounded to bf16, fp32
 * accumulation, one rounding of the sum).  wproj_packed: 128 KiB from dxmi_pack_attn_proj_weight (fp32 [256][256] OI weight).
 * Inference path only: training keeps the two launches (the projection's weight gradient needs the attention output). */
int dxmi_attention_proj_supported(int32_t T, int32_t C, int32_t heads);
int dxmi_pack_attn_proj_weight(const float* w_oi, void* dst, void* stream);
int dxmi_attention_proj_fwd(const void* qkv, const void* wproj_packed, const float* bias, const void* residual, void* out,
                            float* gn_stats, int32_t N, int32_t T, int32_t C, int32_t heads, float scale, void* stream);
/* gn_stats (optional): GroupNorm block statistics of `out`, fp32 [N][8][C/2][2] — one partial per 32 tokens, the layout
 * dxmi_groupnorm_apply reads (P = 8). */

/* The whole AttnBlock in ONE launch (round 5; reference models/DxMI/unet_small.py:167-191: h_ = norm(x); q, k, v = 1x1 convs of
 * h_; w_ = softmax(q^T k * C^-0.5); h_ = proj_out(v w_^T); return x + h_), for the single-head 256-token x 256-channel blocks of
 * the CIFAR-10 net (dxmi_attn_block_supported), inference path only.  x: NHWC bf16 [N,256,256]; stats: its GroupNorm block
 * statistics fp32 [N][P][128][2], P <= 8 (dxmi_conv_desc.gn_stats / dxmi_gn_block_stats layout; dxmi_gn_stats_fold folds more);
 * gamma / beta: the block's norm.  The
 * normalised input, q, k, v and the attention output never exist in memory: with G = scale Wk^T Wq and W' = Wproj Wv folded once
 * per weight version (dxmi_attn_block_pack: fp32 [256][256] OI weights and [256] biases -> dxmi_attn_block_packed_bytes() bytes)
 * the raw x tile in LDS is K, V and the residual at once (terms constant along the key axis drop out of the softmax; rows of the
 * softmax sum to one).  out: [N,256,256] bf16; out_stats (optional): block statistics of out, fp32 [N][8][128][2].
 * Tolerance against the reference block in fp32: the same as the three-launch form it replaces (dxmi_groupnorm_apply +
 * dxmi_conv2d_fwd + dxmi_attention_proj_fwd), see tests/test_hip_round5_kernels.py. */
int dxmi_attn_block_supported(int32_t T, int32_t C, int32_t heads, int32_t groups);
int64_t dxmi_attn_block_packed_bytes(void);
int dxmi_attn_block_pack(const float* wq, const float* bq, const float* wk, const float* wv, const float* bv,
                         const float* wproj, const float* bproj, float scale, void* dst, void* stream);
int dxmi_attn_block_fwd(const void* x, const float* stats, int32_t P, const float* gamma, const float* beta, float eps,
                        const void* packed, void* out, float* out_stats, int32_t N, int32_t T, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Timestep-embedding path.
 * dxmi_timestep_embedding: out[N,dim] fp32 sinusoid of t; freq_i = exp(-ln(max_period)*i/denom)
 *   order 0 = [sin | cos], denom = dim/2 - 1   (get_timestep_embedding, unet_small.py:9-27)
 *   order 1 = [cos | sin], denom = dim/2       (timestep_embedding, models/cm/nn.py:119-137)
 * dxmi_linear_fwd: out[P,M] = post(pre(x[P,K]) @ W[M,K]^T + b): fp32 rows in/out, bf16 MFMA
 *   operands (same kernel as the convs).  Serves temb.dense.{0,1} (unet_small.py:297-299), the
 *   concatenation of all temb_proj layers in ONE launch (unet_small.py:123; pre = swish) and
 *   the EDM time_embed / emb_layers (models/cm/unet.py:775-779, :249).
 *   wpacked = dxmi_pack_conv_weight(W as [M,K,1,1]).
 * ---------------------------------------------------------------------------------------- */
int dxmi_timestep_embedding(const float* t, float* out, int32_t N, int32_t dim, int32_t order,
                            float max_period, void* stream);
int dxmi_linear_fwd(const float* x, const void* wpacked, const float* bias, float* out,
                    int32_t P, int32_t K, int32_t M, int32_t pre_act, int32_t post_act,
                    void* stream);
/* Split-K form for skinny products with a long K (the data gradient of the ADM nets' concatenated emb_layers, models/cm/unet.py:249:
 * 16 rows x K ~ 30 000 -> 768 columns): partials[s][P][M], s < dxmi_linear_splitk_slices(P, K, M) (0: unsupported shape, 1: no
 * split pays), each slice the product over its K range; the caller sums the slices in order and adds bias / activation. */
int dxmi_linear_splitk_slices(int32_t P, int32_t K, int32_t M);
int dxmi_linear_splitk(const float* x, const void* wpacked, float* partials, int32_t P, int32_t K, int32_t M, int32_t pre_act,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused VAR sampler transition (models/DxMI/var_sampler.py:262-295 and :373-407):
 *   xs = x*xmul[b]; control = cmul[b]*eps; mean = xs+control; x' = mean + sigma[b]*z;
 *   logp[b] = mean_CHW Normal(mean, sigma).log_prob(x').
 * assoc selects the reference's floating-point association of the update: 0 = mean + sigma*z
 * (sample_step, :399), 1 = xs + (control + sigma*z) (VAR_sampling, :285).
 * Per-sample scalars are read from device vectors, so one kernel serves both the T-step
 * loop (all entries equal) and sample_step with per-sample integer t.
 * ---------------------------------------------------------------------------------------- */
int dxmi_var_step_fwd(const float* x, const float* eps, const float* z,
                      const float* xmul, const float* cmul, const float* sigma,
                      float* x_next, float* mean, float* control, float* logp,
                      int32_t N, int32_t CHW, int32_t assoc, void* stream);

/* Backward of the VAR transition for the differentiable `sample_step` of the policy update (reference var_sampler.py:357-408 under
 * torch autograd): with x' = xm x + c eps + sigma z, mean = xm x + c eps, control = c eps and logp as dxmi_var_step_fwd forms it
 * (x' detached inside), given the gradients of the loss w.r.t. x' / mean / control ([N, CHW]) and logp ([N]) — any may be NULL —
 *   d_eps = c (g_next + g_mean + g_control + g_logp z / (sigma CHW))       d_sigma[n] = sum g_next z + g_logp (mean z^2 - 1) / sigma
 * (cmul = theta multiplier x adhoc_scale1, per sample).  The sigma gradient is reduced in-kernel in a fixed order; the caller chains it
 * into log_betas (sigma = exp(log_betas[t])). */
int dxmi_var_step_bwd(const float* g_next, const float* g_mean, const float* g_control, const float* g_logp, const float* z,
                      const float* cmul, const float* sigma, float* d_eps, float* d_sigma, int32_t N, int32_t CHW, void* stream);

/* Backward of the EDM transition (openai_diffusion.py:71-94): d_model_out = -(c_out (sigma_down - sigma) / sigma) (g_sample + g_mean),
 * d_sigma_up[n] = sum g_sample z; g_sample / g_mean may be NULL. */
int dxmi_edm_step_bwd(const float* g_sample, const float* g_mean, const float* z, const float* sigma, const float* sigma_down,
                      float* d_model_out, float* d_sigma_up, int32_t N, int32_t CHW, float sigma_data, void* stream);

/* INT path: per-sample gather of schedule tables by integer timestep
 * (var_sampler.py:363-376,389; models/diffusion.py:18-22).  Writes
 *   tau[b] = continuous_steps[t[b]], xmul[b], cmul[b] (theta multiplier), sigma[b] =
 *   exp(log_betas_all[t[b]]).  Bit-exact w.r.t. the fp32 tables. */
int dxmi_var_gather_sched(const int64_t* t, const float* continuous_steps,
                          const float* xmul_tab, const float* cmul_tab,
                          const float* log_betas_all, float* tau, float* xmul, float* cmul,
                          float* sigma, int32_t N, int32_t T, void* stream);

/* Elementwise helpers of the value network (models/modules.py:96-101): 2x2 average pool
 * (optional) followed by activation, NHWC bf16. */
int dxmi_pool_act(const void* in, void* out, int32_t N, int32_t H, int32_t W, int32_t C,
                  int32_t pool, int32_t act, void* stream);
/* Value head (models/modules.py:150-158): relu -> sum over HxW -> Linear(C,1) -> out_scale
 * (Linear(1,1): y*out_w[0]+out_b[0], both device scalars, or both NULL). */
int dxmi_value_head(const void* in, const float* w, const float* b, const float* out_w,
                    const float* out_b, float* out, int32_t N, int32_t HW, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * EDM / ADM U-Net path (models/cm/unet.py, models/cm/karras_diffusion.py, models/DxMI/openai_diffusion.py).
 * dxmi_groupnorm_generic_fwd: GroupNorm32 (+ scale-shift norm, + SiLU) for any channels-per-group and
 *   map size (two kernels: coalesced partial statistics, then apply); scale_shift: fp32 [N, ss_ld] with
 *   scale at [c] and shift at [C + c] (unet.py:252-256) or NULL.  workspace from
 *   dxmi_groupnorm_generic_workspace_bytes.
 * dxmi_upsample2x: nearest x2 (ResBlock up, x branch; unet.py:197-198).
 * dxmi_edm_precond: x_in = c_in(sigma)*x, t = 250 ln(sigma + 1e-44)   (karras_diffusion.py:64-68,348-349).
 * dxmi_edm_step_fwd: fused Euler-ancestral transition (openai_diffusion.py:71-94): denoised =
 *   c_out F + c_skip x; d = (x - denoised)/sigma; mean = x + d (sigma_down - sigma); sample = mean + z sigma_up.
 * ---------------------------------------------------------------------------------------- */
int dxmi_groupnorm_silu_supported(int32_t C0, int32_t C1, int32_t HW, int32_t groups); /* 1: one-pass kernel serves it */
int64_t dxmi_groupnorm_generic_workspace_bytes(int32_t N, int32_t HW, int32_t C);
int dxmi_groupnorm_generic_fwd(const void* in0, int32_t C0, const void* in1, int32_t C1, const float* gamma,
                               const float* beta, const float* scale_shift, int32_t ss_ld, void* out,
                               void* workspace, int32_t N, int32_t HW, int32_t groups, float eps,
                               int32_t apply_silu, void* stream);
/* Backward of dxmi_groupnorm_generic_fwd: dx0 | dx1 (bf16, optional additive inputs add0 | add1 fused) and
 * g_out fp32 [2][N][C] = per-image sums of dyy and dyy*xhat, from which the caller forms dgamma, dbeta and the FiLM
 * gradients (dscale = G1*gamma + G0*beta, dshift = G0).  Replaces autograd through models/cm/unet.py:228-260. */
int64_t dxmi_groupnorm_generic_bwd_workspace_bytes(int32_t N, int32_t HW, int32_t C);
/* Launch form dxmi_groupnorm_generic_bwd[_saved] takes for the shape under the current "gn_bwd_fused" knob and device:
 * 0 = the reduce + apply launches, 8 or 16 = the one-launch form with that many rows per thread (its residency guard passed). */
int dxmi_groupnorm_generic_bwd_plan(int32_t N, int32_t HW, int32_t C);
int dxmi_groupnorm_generic_bwd(const void* in0, int32_t C0, const void* in1, int32_t C1, const void* dy,
                               const void* add0, const void* add1, const float* gamma, const float* beta,
                               const float* scale_shift, int32_t ss_ld, void* dx0, void* dx1, float* g_out,
                               void* workspace, int32_t N, int32_t HW, int32_t groups, float eps,
                               int32_t apply_silu, void* stream);
/* Same with the forward's statistics kept by the caller: fwd_stats = the first dxmi_groupnorm_generic_workspace_bytes bytes of the
 * workspace dxmi_groupnorm_generic_fwd was given (per-chunk group sums; untouched by the forward's second kernel), which saves the
 * backward its own statistics pass over the input (autograd keeps mean / rstd the same way).  fwd_stats NULL: recomputed. */
int dxmi_groupnorm_generic_bwd_saved(const void* in0, int32_t C0, const void* in1, int32_t C1, const void* dy,
                                     const void* add0, const void* add1, const float* gamma, const float* beta,
                                     const float* scale_shift, int32_t ss_ld, void* dx0, void* dx1, float* g_out,
                                     const float* fwd_stats, void* workspace, int32_t N, int32_t HW, int32_t groups, float eps,
                                     int32_t apply_silu, void* stream);
int dxmi_upsample2x(const void* in, void* out, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int dxmi_edm_precond(const float* x, const float* sigma, float* x_in, float* t_out, int32_t N, int32_t CHW,
                     float sigma_data, void* stream);
int dxmi_edm_step_fwd(const float* x, const float* model_out, const float* z, const float* sigma,
                      const float* sigma_down, const float* sigma_up, float* sample, float* mean, int32_t N,
                      int32_t CHW, float sigma_data, void* stream);

/* im2col of a 3-channel NCHW fp32 image (3x3, stride 1, pad 1): out [N,H,W,64] bf16, channel
 * k = ci*9+ky*3+kx for k < 27, zero above — the activation operand of the stem convs' weight gradient
 * (dxmi_conv2d_wgrad with ksize 1). */
int dxmi_im2col27(const float* x, void* out, int32_t N, int32_t H, int32_t W, void* stream);

/* Output stage of generate_cifar10.py / generate_large.py: NCHW fp32 sampler output -> uint8 pixels (NHWC when out_nhwc,
 * else NCHW), the reference's fp32 operation order, no fused multiply-add between its steps (bit-exact pixel values):
 *   mode 0: v = (x - (-1)) / 2 -> clamp(0,1) -> * 255 -> + 0.5 -> clamp(0,255) -> truncate
 *           (rescale(), generate_cifar10.py:41-42 and :205-209; generate_large.py:36-41; torchvision.utils.save_image)
 *   mode 1: (x + 1) * 127.5 -> clamp(0,255) -> truncate   (the FID / samples_N.npz array, generate_large.py:43)
 * HW must be a multiple of 4. */
int dxmi_quantize_u8(const float* x, void* out, int32_t N, int32_t C, int32_t HW, int32_t mode, int32_t out_nhwc,
                     void* stream);

/* Layout converters at the network edge. */
int dxmi_nchw_f32_to_nhwc_bf16(const float* in, void* out, int32_t N, int32_t C, int32_t HW,
                               void* stream);
int dxmi_nhwc_bf16_to_nchw_f32(const void* in, float* out, int32_t N, int32_t C, int32_t HW,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Train-step tail: multi-tensor optimiser steps, gradient-norm clip, dropout, replay-buffer gathers.
 * Tensor lists are HOST arrays of device pointers / element counts (any length; the library cuts them into
 * launches of DXMI_MT_MAX tensors passed by value in the kernel arguments — no descriptor upload).
 * ---------------------------------------------------------------------------------------- */
#define DXMI_MT_MAX 64

/* Workgroups one multi-tensor launch series uses over `numel[0..count)` (= fp32 partials dxmi_gradnorm_clip needs). */
int64_t dxmi_mt_blocks(const int64_t* numel, int32_t count);

/* torch.optim.Adam.step() over fp32 tensors (models/DxMI/trainer.py:264, :325, :389 with the optimisers of
 * train_cifar10.py:283-296), the arithmetic of torch's _multi_tensor_adam (no amsgrad / weight decay), every
 * intermediate rounded to fp32 where the foreach implementation stores one:
 *   m = m + (1-b1)(g - m);  v = v*b2 + (1-b2) g*g;  p = p + step_size[i] * m / (sqrt(v)/bc2_sqrt + eps)
 * step_size[i] = -(lr_i / (1 - b1^t)) and bc2_sqrt = sqrt(1 - b2^t) are formed by the caller in double, as torch does;
 * scalar hyper-parameters cross the ABI as double and are rounded to fp32 once (ATen's Scalar -> float conversion).
 * grad_scale: optional DEVICE scalar multiplied into every gradient first (the clip coefficient of
 * dxmi_gradnorm_clip: clip-then-step without a host round trip); write_back_grad also stores the scaled gradient. */
int dxmi_adam_step(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                   const int64_t* numel, const float* step_size, int32_t count, double beta1, double beta2,
                   double eps, double bc2_sqrt, const float* grad_scale, int32_t write_back_grad, void* stream);

/* The same update for a step that is REPLAYED from a hipGraph (dxmi_hip/graph.py: kernel arguments are frozen at capture, the
 * step count is not): the step-dependent scalars are read from DEVICE memory, hyper = fp32 [bc2_sqrt, step_size[0..count)],
 * formed by the host exactly as for dxmi_adam_step and uploaded before every replay.  Bit-identical results. */
int dxmi_adam_step_dev(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                       const int64_t* numel, int32_t count, double beta1, double beta2, double eps, const float* hyper,
                       const float* grad_scale, int32_t write_back_grad, void* stream);

/* torch.optim.RAdam.step() (MixedPrecisionTrainer.optimize, models/cm/fp16_util.py:204-223; optimiser built at
 * train_image_large.py:153-160), arithmetic of torch/optim/radam.py _single_tensor_radam:
 *   p -= ((m/bc1) * lr_i) * (bc2_sqrt / (sqrt(v) + eps)) * rect      (rect < 0: p -= (m/bc1) * lr_i, rho_t <= 5)
 * grad_scale: optional DEVICE scalar (1 / 2^lg_loss_scale); found_inf: optional DEVICE flag, non-zero skips the whole
 * step on the device (the overflow test of fp16_util.py:208-212 without a host sync in front of the kernels). */
int dxmi_radam_step(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                    const int64_t* numel, const float* lr, int32_t count, double beta1, double beta2, double eps,
                    double bc1, double bc2_sqrt, double rect, const float* grad_scale, const float* found_inf,
                    void* stream);

/* dxmi_radam_step for a hipGraph-replayed step: hyper = DEVICE fp32 [fp32(1/bc1), bc2_sqrt, rect, lr[0..count)]. */
int dxmi_radam_step_dev(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                        const int64_t* numel, int32_t count, double beta1, double beta2, double eps, const float* hyper,
                        const float* grad_scale, const float* found_inf, void* stream);

/* torch.nn.utils.clip_grad_norm_(params, max_norm) (trainer.py:388, :666-667; also MixedPrecisionTrainer._compute_norms
 * fp16_util.py:232-240 with max_norm <= 0 = "norm only"): out3[0] = global L2 norm, out3[1] = min(1, max_norm/(norm+1e-6)),
 * out3[2] = 1 if the norm is inf/nan.  Fixed-order reductions (reproducible).  partials: >= dxmi_mt_blocks() floats.
 * scale_in_place: multiply the gradients by out3[1] (otherwise hand out3+1 to dxmi_adam_step as grad_scale). */
int dxmi_gradnorm_clip(void* const* grads, const int64_t* numel, int32_t count, float max_norm, float* partials,
                       float* out3, int32_t scale_in_place, void* stream);

/* nn.Dropout(p) of ResnetBlock (models/DxMI/unet_small.py:129), NHWC bf16: y[i] = keep(i) ? bf16(x[i]/(1-p)) : 0 with
 * keep(i) = (mix32(i ^ seed) >> 8) >= p*2^24, mix32 = the 32-bit finaliser x^=x>>16; x*=0x7feb352d; x^=x>>15;
 * x*=0x846ca68b; x^=x>>16.  The backward pass calls it again on the gradient with the same seed (no stored mask). */
int dxmi_dropout_bf16(const void* x, void* y, int64_t n, float p, uint32_t seed, void* stream);
/* ... with the seed read from DEVICE memory (a dropout site of a hipGraph-replayed step: the host uploads a fresh seed
 * before every replay). */
int dxmi_dropout_bf16_dev(const void* x, void* y, int64_t n, float p, const uint32_t* seed, void* stream);

/* Denoising score-matching loss of the EDM teacher (KarrasDenoiser.training_losses, models/cm/karras_diffusion.py:82-106, with
 * get_weightings :18-31 and denoise :337-351), fp32 NCHW [N, CHW] tensors (CHW a multiple of 4 below 2^30, 16-byte aligned), sigma [N]:
 * dxmi_edm_dsm_prep:     x_in = c_in(s) (x_start + noise s), t[n] = 250 ln(s + 1e-44) — the network input; x_t is not stored.
 * dxmi_edm_dsm_loss_fwd: x_t recomputed, denoised = c_out F + c_skip x_t (boundary-condition scalings when distillation != 0),
 *                        xs_mse[n] = mean((denoised - x_start)^2), mse[n] = mean(w(s) (denoised - x_start)^2), w = the weight
 *                        schedule below; per-sample sums in a fixed order (bitwise reproducible).
 * dxmi_edm_dsm_loss_bwd: d_model_out = (((g_mse/D) w) 2e + (g_xs/D) 2e) c_out, e = denoised - x_start: autograd's nodes in its
 *                        order; g_mse / g_xs are DEVICE [N] upstream gradients, either may be NULL (that term not differentiated).
 * Every fp32 operation in the reference's order, one rounding per torch op. */
#define DXMI_DSM_W_SNR        0   /* snrs = sigma^-2 */
#define DXMI_DSM_W_SNR_P1     1   /* snrs + 1 */
#define DXMI_DSM_W_KARRAS     2   /* snrs + 1 / sigma_data^2 */
#define DXMI_DSM_W_TRUNC_SNR  3   /* clamp(snrs, min=1) */
#define DXMI_DSM_W_UNIFORM    4   /* 1 */
#define DXMI_DSM_W_ICT        5   /* 1 / (t - t2), t = t_table[index], t2 = t_table[index + 1] (Song and Dhariwal 2023, "Improved
                                   * Techniques for Training Consistency Models"): dxmi_cd_huber_fwd / _bwd ONLY, which have both
                                   * levels; every other entry point refuses it */
int dxmi_edm_dsm_prep(const float* x_start, const float* noise, const float* sigma, float* x_in, float* t_out, int32_t N,
                      int32_t CHW, float sigma_data, void* stream);
int dxmi_edm_dsm_loss_fwd(const float* model_out, const float* x_start, const float* noise, const float* sigma, float* xs_mse,
                          float* mse, int32_t N, int32_t CHW, float sigma_data, float sigma_min, int32_t distillation,
                          int32_t weight_schedule, void* stream);
int dxmi_edm_dsm_loss_bwd(const float* g_mse, const float* g_xs, const float* model_out, const float* x_start, const float* noise,
                          const float* sigma, float* d_model_out, int32_t N, int32_t CHW, float sigma_data, float sigma_min,
                          int32_t distillation, int32_t weight_schedule, void* stream);

/* Noise-prediction training of the DDPM U-Net (Ho et al. 2020, "Denoising Diffusion Probabilistic Models"), fp32 NCHW [N, CHW]
 * tensors (CHW a multiple of 4 below 2^30, 16-byte aligned).  table: fp32 [2][T] on the DEVICE, row 0 = sqrt(alpha_bar), row 1 =
 * sqrt(1 - alpha_bar) of calc_diffusion_hyperparams (models/DxMI/var_sampler.py); t_idx: int64 [N] on the DEVICE.
 * dxmi_ddpm_prep (eq. 4, q(x_t | x_0)): x_t[n] = table[0][t] x_start[n] + table[1][t] noise[n] (two products, one sum),
 *   t_out[n] = (float)t — the network's input.  An index outside [0, T) gives NaN coefficients for that sample; nothing outside
 *   the table is read.
 * dxmi_ddpm_loss_fwd (eq. 14, L_simple): loss[n] = mean_flat((eps_pred - noise)^2); the sum in a fixed order (bitwise reproducible).
 * dxmi_ddpm_loss_bwd: d_eps[n] = (g_loss[n] / CHW) * (2 (eps_pred[n] - noise[n])): torch autograd's nodes of
 *   ((a - b) ** 2).mean(dim) in its order; g_loss is the DEVICE [N] upstream gradient. */
int dxmi_ddpm_prep(const float* x_start, const float* noise, const int64_t* t_idx, const float* table, int32_t T, float* x_t,
                   float* t_out, int32_t N, int32_t CHW, void* stream);
int dxmi_ddpm_loss_fwd(const float* eps_pred, const float* noise, float* loss, int32_t N, int32_t CHW, void* stream);
int dxmi_ddpm_loss_bwd(const float* g_loss, const float* eps_pred, const float* noise, float* d_eps, int32_t N, int32_t CHW,
                       void* stream);

/* update_ema (models/cm/nn.py:57-67) for up to DXMI_EMA_MAX_RATES rates at once (TrainLoop._update_ema, train_util.py:190-193):
 * ema[k * count + i] = rates[k] ema[k * count + i] + (1 - rates[k]) src[i] over fp32 DEVICE tensors of numel[i] elements, as
 * torch's mul_(rate).add_(src, alpha=1-rate) (rate and 1-rate formed in double, rounded to fp32 once; the add is one fused
 * multiply-add, as ATen's).  A rate of exactly 0 (the target network of improved consistency training) is a copy of src, bit for
 * bit (0 * ema + src would turn a src of -0 into +0 and a non-finite ema into NaN).  The source is read once for all rates.  found_inf: DEVICE fp32 flag or NULL; when it is non-zero the
 * launch leaves every EMA tensor untouched (the step was skipped on overflow), with no host sync. */
#define DXMI_EMA_MAX_RATES 4
int dxmi_ema_update(void* const* ema, const void* const* src, const int64_t* numel, int32_t count, int32_t n_rates,
                    const double* rates, const float* found_inf, void* stream);

/* Consistency distillation / consistency training losses (KarrasDenoiser.consistency_losses, models/cm/karras_diffusion.py:108-241),
 * one launch between two network evaluations.  fp32 NCHW [N, CHW] tensors (CHW a multiple of 4 below 2^30, 16-byte aligned); indices: int64
 * [N] on the DEVICE; t_table: fp32 [num_scales] on the DEVICE, the time ladder of :180-188 built on the host: t = t_table[index],
 * t2 = t_table[index + 1].  An index outside [0, num_scales - 2] gives NaN levels; nothing outside the table is read.  Every fp32
 * operation in the reference's order, one rounding per torch op (true division by t; (d + next_d) * ((t2 - t) / 2)).
 * dxmi_cd_prep (:190, denoise :345-349): x_t = x_start + noise t (kept), x_in = c_in(t) x_t, t_out = 250 ln(t + 1e-44) — the online
 *   net's input; x_in_teacher (NULL: not written) = c_in(t) x_t under teacher_sigma_data, for a teacher diffusion whose sigma_data
 *   differs (its time is t_out: the time does not depend on sigma_data).
 * dxmi_cd_solver (euler_solver :164-174, heun_solver :144-162), the denoiser formed with the SOLVER diffusion's scalings (the
 *   teacher's sigma_data / sigma_min / distillation flag; denoise() does not clamp) and x_in_next scaled by c_in(t2) under
 *   next_sigma_data, t_next = 250 ln(t2 + 1e-44):
 *     EULER_X0   x_t2 = x_t + ((x_t - x_start) / t) (t2 - t); x_in_next = the TARGET net's input (no network between).
 *     HEUN_PRED  model_out = the teacher at (x_t, t): d = (x_t - denoiser) / t and samples = x_t + d (t2 - t) are written;
 *                x_in_next = the teacher's second input c_in(t2) samples.
 *     HEUN_CORR  model_out = the teacher at (samples, t2): next_d = (samples - denoiser) / t2,
 *                x_t2 = x_t + (d + next_d) ((t2 - t) / 2); x_in_next = the TARGET net's input.
 * dxmi_cd_loss_fwd (:193-220): distiller = c_out(t) f_online + c_skip(t) x_t, target = c_out(t2) f_target + c_skip(t2) x_t2
 *   (boundary-condition scalings when distillation != 0), diffs = |.| (L1), (.)^2 (L2), or (.)^2 after both were resized to
 *   32 x 32 by F.interpolate(size=32, mode="bilinear") (L2_32: align_corners False, no antialias, two taps per axis);
 *   loss[n] = mean_flat(diffs) * get_weightings(weight_schedule, t^-2) (DXMI_DSM_W_*).  Sums in a fixed order (bitwise reproducible).
 * dxmi_cd_loss_bwd: d_f_online of loss for the DEVICE [N] upstream gradient g_loss: autograd's nodes in its order; L1 uses
 *   sign with sign(0) = 0 (th.abs), L2_32 the transpose of the resize.
 * dxmi_cd_huber_fwd: the pseudo-Huber metric of improved consistency training on the same difference df = distiller - target
 *   (the scalings of dxmi_cd_loss_fwd): ssq[n] = sum(df^2) over the image (a sum, not mean_flat; the fixed order of the L2 norm,
 *   bitwise reproducible) and loss[n] = w ssq / (sqrt(ssq + c^2) + c), c = huber_c > 0.  That form equals sqrt(ssq + c^2) - c and
 *   keeps its digits at ssq << c^2, where the subtraction loses them.  w: DXMI_DSM_W_* including DXMI_DSM_W_ICT.
 * dxmi_cd_huber_bwd: d_f_online = (g_loss[n] w / sqrt(ssq[n] + c^2)) df c_out(t) for the DEVICE [N] upstream gradient g_loss; ssq
 *   is the forward's (read, not recomputed).  Neither reads anything back. */
#define DXMI_CD_EULER_X0   0
#define DXMI_CD_HEUN_PRED  1
#define DXMI_CD_HEUN_CORR  2
#define DXMI_CD_NORM_L1    0
#define DXMI_CD_NORM_L2    1
#define DXMI_CD_NORM_L2_32 2
int dxmi_cd_prep(const float* x_start, const float* noise, const int64_t* indices, const float* t_table, int32_t num_scales,
                 float* x_t, float* x_in, float* t_out, float* x_in_teacher, int32_t N, int32_t CHW, float sigma_data,
                 float teacher_sigma_data, void* stream);
int dxmi_cd_solver(int32_t mode, const float* x_start, const float* x_t, const float* model_out, float* d, float* samples,
                   const int64_t* indices, const float* t_table, int32_t num_scales, float* x_t2, float* x_in_next, float* t_next,
                   int32_t N, int32_t CHW, float solver_sigma_data, float solver_sigma_min, int32_t solver_distillation,
                   float next_sigma_data, void* stream);
int dxmi_cd_loss_fwd(const float* f_online, const float* f_target, const float* x_t, const float* x_t2, const int64_t* indices,
                     const float* t_table, int32_t num_scales, float* loss, int32_t N, int32_t C, int32_t H, int32_t W,
                     int32_t loss_norm, float sigma_data, float sigma_min, int32_t distillation, int32_t weight_schedule, void* stream);
int dxmi_cd_loss_bwd(const float* g_loss, const float* f_online, const float* f_target, const float* x_t, const float* x_t2,
                     const int64_t* indices, const float* t_table, int32_t num_scales, float* d_f_online, int32_t N, int32_t C,
                     int32_t H, int32_t W, int32_t loss_norm, float sigma_data, float sigma_min, int32_t distillation,
                     int32_t weight_schedule, void* stream);
int dxmi_cd_huber_fwd(const float* f_online, const float* f_target, const float* x_t, const float* x_t2, const int64_t* indices,
                      const float* t_table, int32_t num_scales, float* loss, float* ssq, int32_t N, int32_t CHW, float huber_c,
                      float sigma_data, float sigma_min, int32_t distillation, int32_t weight_schedule, void* stream);
int dxmi_cd_huber_bwd(const float* g_loss, const float* ssq, const float* f_online, const float* f_target, const float* x_t,
                      const float* x_t2, const int64_t* indices, const float* t_table, int32_t num_scales, float* d_f_online,
                      int32_t N, int32_t CHW, float huber_c, float sigma_data, float sigma_min, int32_t distillation,
                      int32_t weight_schedule, void* stream);

/* Progressive distillation loss (KarrasDenoiser.progdist_losses, models/cm/karras_diffusion.py:243-335), the launches between its
 * network evaluations; the first, x_t and the inputs at t (:300, denoise :345-349), is dxmi_cd_prep on the first num_scales + 1
 * entries of the table.  Tensors as for dxmi_cd_*.  t_table: fp32 [2 num_scales + 1] on the DEVICE, built on the host with the
 * reference's expressions (:285-298): entries [0, num_scales] the coarse ladder (t = t_table[index], t3 = t_table[index + 1]),
 * entries [num_scales + 1, 2 num_scales] the half steps (t2 = t_table[num_scales + 1 + index]).  num_scales >= 1.  An index outside
 * [0, num_scales - 1] gives NaN levels; nothing outside the table is read.  Every fp32 operation in the reference's order, one
 * rounding per torch op.
 * dxmi_pd_solver (euler_solver :267-274, euler_to_denoiser :276-281), the denoiser formed with the SOLVER diffusion's scalings
 *   (the teacher's sigma_data / sigma_min / distillation flag; denoise() does not clamp):
 *     MID  model_out = the teacher at (x_t, t): out = x_t2 = x_t + ((x_t - denoiser) / t) (t2 - t); x_in_next = c_in(t2) x_t2
 *          under next_sigma_data and t_next = 250 ln(t2 + 1e-44), the teacher's second input.  x_t2_in is not read.
 *     END  model_out = the teacher at (x_t2_in, t2): x_t3 = x_t2 + ((x_t2 - denoiser) / t2) (t3 - t2) (never stored) and
 *          out = target_x = x_t - (t (x_t3 - x_t)) / (t3 - t) (:278-280).  x_in_next / t_next are not written (may be NULL).
 * dxmi_pd_loss_fwd (:302, :309-316): denoised = c_out(t) f_online + c_skip(t) x_t (boundary-condition scalings when
 *   distillation != 0), diffs = |denoised - target_x| (DXMI_CD_NORM_L1) or (.)^2 (DXMI_CD_NORM_L2; progdist has no l2-32),
 *   loss[n] = mean_flat(diffs) * get_weightings(weight_schedule, t^-2) (DXMI_DSM_W_*).  Sums in a fixed order.
 * dxmi_pd_loss_bwd: d_f_online of that loss for the DEVICE [N] upstream gradient g_loss; L1 uses sign with sign(0) = 0 (th.abs).
 * dxmi_pd_lpips_images (:317-327): x01 fp32 [2 N, CHW] = (denoised + 1) / 2 in rows [0, N) and (target_x + 1) / 2 in rows
 *   [N, 2 N), weights[n] = get_weightings(weight_schedule, t^-2); the backward of the lpips norm is dxmi_cd_lpips_bwd on the coarse
 *   ladder, which needs only c_out(t). */
#define DXMI_PD_MID 0
#define DXMI_PD_END 1
int dxmi_pd_solver(int32_t mode, const float* x_t, const float* x_t2_in, const float* model_out, const int64_t* indices,
                   const float* t_table, int32_t num_scales, float* out, float* x_in_next, float* t_next, int32_t N, int32_t CHW,
                   float solver_sigma_data, float solver_sigma_min, int32_t solver_distillation, float next_sigma_data, void* stream);
int dxmi_pd_loss_fwd(const float* f_online, const float* x_t, const float* target_x, const int64_t* indices, const float* t_table,
                     int32_t num_scales, float* loss, int32_t N, int32_t CHW, int32_t loss_norm, float sigma_data, float sigma_min,
                     int32_t distillation, int32_t weight_schedule, void* stream);
int dxmi_pd_loss_bwd(const float* g_loss, const float* f_online, const float* x_t, const float* target_x, const int64_t* indices,
                     const float* t_table, int32_t num_scales, float* d_f_online, int32_t N, int32_t CHW, int32_t loss_norm,
                     float sigma_data, float sigma_min, int32_t distillation, int32_t weight_schedule, void* stream);
int dxmi_pd_lpips_images(const float* f_online, const float* x_t, const float* target_x, const int64_t* indices,
                         const float* t_table, int32_t num_scales, float* x01, float* weights, int32_t N, int32_t CHW,
                         float sigma_data, float sigma_min, int32_t distillation, int32_t weight_schedule, void* stream);

/* Distribution matching distillation of an EDM teacher into a ONE-step generator G(z) = D_theta(sigma_G z, sigma_G)
 * (KarrasDenoiser.dm_generator_losses; Diff-Instruct, Luo et al. 2023, eq. 8 and Algorithm 1; DMD, Yin et al. 2023, eq. 7-8; DMD2,
 * Yin et al. 2024, eq. 2-3; its GAN term is further down, csrc/gan_head.hip): the launches between the generator and the "real" (teacher) and "fake" (trained
 * online on the generator's samples) denoisers.  Tensors as for dxmi_cd_*: fp32 [N, CHW] contiguous, 16-byte aligned, CHW % 4 == 0.
 * t_table: fp32 [num_scales] on the DEVICE (the ladder of dxmi_cd_*); t = t_table[index], and since no t2 is needed every index
 * in [0, num_scales - 1] is legal.  An index outside gives a NaN level; nothing outside the table is read.  One rounding per written
 * operation, sums in a fixed order (bitwise reproducible), no atomics.  gen_sigma and every sigma_data must be positive and finite.
 * dxmi_dm_gen_in   (the generator's input, EDM preconditioning, Karras et al. 2022 eq. 7): x_in = c_in(sigma_G) (sigma_G z) and
 *   t_out[n] = 250 ln(sigma_G + 1e-44).
 * dxmi_dm_gen_out  (sampling; DMD eq. 1 with the EDM scalings, distillation = False): x = c_skip(sigma_G) (sigma_G z) +
 *   c_out(sigma_G) f_gen, clamped to [-1, 1] when clip != 0.
 * dxmi_dm_gen_prep (training; DMD2 Algorithm 1, the forward diffusion of the generated image): the same unclamped x (kept),
 *   x_t = x + noise t (kept), x_in_real = c_in_real(t) x_t, t_out[n] = 250 ln(t + 1e-44) (the time of both denoisers), and
 *   x_in_fake = c_in_fake(t) x_t where x_in_fake is not NULL (pass it only where fake_sigma_data differs).
 * dxmi_dm_grad_fwd (DMD eq. 7-8): D_r = c_out_r(t) f_real + c_skip_r(t) x_t, D_f likewise with the fake net's scalings
 *   (boundary-condition scalings where that diffusion's distillation != 0), s[n] = mean|x - D_r| (DMD eq. 8's normaliser),
 *   g = (D_f - D_r) / s (DXMI_DM_W_DMD) or D_f - D_r (DXMI_DM_W_NONE, Diff-Instruct eq. 8 with w = 1), loss[n] = 0.5 mean(g^2).
 *   A sample with s == 0 gets g = 0 and loss = 0 under either weighting.  One workgroup per image; D_f - D_r stays in registers up
 *   to CHW = 12288 (3 x 64 x 64), above that the inputs are read a second time.
 * dxmi_dm_gen_bwd  (DMD eq. 7: the gradient reaches the generator through x alone, d loss_n / d x = g_n / CHW):
 *   d_f_gen[n] = ((upstream[n] / CHW) g[n]) c_out(sigma_G) for the DEVICE [N] upstream gradient. */
#define DXMI_DM_W_DMD  0
#define DXMI_DM_W_NONE 1
int dxmi_dm_gen_in(const float* z, float* x_in, float* t_out, int32_t N, int32_t CHW, float gen_sigma, float sigma_data, void* stream);
int dxmi_dm_gen_out(const float* f_gen, const float* z, float* x, int32_t N, int32_t CHW, float gen_sigma, float sigma_data,
                    int32_t clip, void* stream);
int dxmi_dm_gen_prep(const float* f_gen, const float* z, const float* noise, const int64_t* indices, const float* t_table,
                     int32_t num_scales, float* x, float* x_t, float* x_in_real, float* t_out, float* x_in_fake, int32_t N,
                     int32_t CHW, float gen_sigma, float gen_sigma_data, float real_sigma_data, float fake_sigma_data, void* stream);
int dxmi_dm_grad_fwd(const float* f_real, const float* f_fake, const float* x, const float* x_t, const int64_t* indices,
                     const float* t_table, int32_t num_scales, float* g, float* loss, float* s, int32_t N, int32_t CHW,
                     int32_t weighting, float real_sigma_data, float real_sigma_min, int32_t real_distillation,
                     float fake_sigma_data, float fake_sigma_min, int32_t fake_distillation, void* stream);
int dxmi_dm_gen_bwd(const float* upstream, const float* g, float* d_f_gen, int32_t N, int32_t CHW, float gen_sigma, float sigma_data,
                    void* stream);

/* The K-step generator of the same loss, trained by backward simulation (DMD2, Yin et al. 2024, section 4.4-4.5;
 * KarrasDenoiser.dm_generator_losses with gen_sigmas, dm_sample with gen_sigmas; csrc/dm_train.hip).  gen_sigmas: fp32
 * [num_steps] on the DEVICE, sigma_0 > ... > sigma_{K-1} > 0 (K = num_steps >= 1).  Step j of the generator is the EDM denoiser
 * G_j(x) = c_skip(sigma_j) x + c_out(sigma_j) F(c_in(sigma_j) x, 250 ln(sigma_j + 1e-44)); the sampler's states are x_0 = sigma_0 z,
 * x_{j+1} = G_j(x_j) + sigma_{j+1} eps_j, never clamped.  steps: int64 [N] on the DEVICE, image n's graded step k_n; a step outside
 * [0, K - 1] gives NaN for that image, and nothing outside the ladder is read.  Tensors, rounding and alignment as dxmi_dm_*.
 * dxmi_dmms_in:    x = sigma_0 z (kept), x_in = c_in(sigma_0) x, t_out[n] = 250 ln(sigma_0 + 1e-44).
 * dxmi_dmms_stage: ONE launch between generator evaluations `stage` and `stage` + 1 (0 <= stage <= K - 2), in place.  For image n with
 *   steps == NULL or steps[n] > stage: x = (c_skip(sigma_j) x + c_out(sigma_j) f_gen) + eps sigma_{j+1}, x_in = c_in(sigma_{j+1}) x,
 *   t_out[n] = 250 ln(sigma_{j+1} + 1e-44).  An image with steps[n] <= stage is frozen: its x, x_in and t_out rows are neither read
 *   nor written, so after stages 0 .. K - 2 x[n] = x_{k_n} and x_in / t_out hold the operands of the graded evaluation.  eps is given,
 *   or made in the launch where sample_index (int64 [N] on the device) is given instead: the bits of
 *   dxmi_randn_indexed(sample_index, CHW, seed, draw).  Giving both, or neither, is an error.
 * dxmi_dmms_prep:  dxmi_dm_gen_prep with x_k where sigma_G z stood and sigma_{steps[n]} where gen_sigma stood; x may be x_k.
 * dxmi_dmms_out:   x = G_{K-1} = c_skip(sigma_{K-1}) x_k + c_out(sigma_{K-1}) f_gen, clamped to [-1, 1] when clip != 0; x may be x_k.
 * dxmi_dmms_bwd:   d_f_gen[n] = ((upstream[n] / CHW) g[n]) c_out(sigma_{steps[n]}). */
int dxmi_dmms_in(const float* z, const float* gen_sigmas, int32_t num_steps, float* x, float* x_in, float* t_out, int32_t N, int32_t CHW,
                 float sigma_data, void* stream);
int dxmi_dmms_stage(const float* f_gen, const float* eps, const int64_t* sample_index, uint32_t draw, uint64_t seed, const int64_t* steps,
                    const float* gen_sigmas, int32_t num_steps, int32_t stage, float* x, float* x_in, float* t_out, int32_t N,
                    int32_t CHW, float sigma_data, void* stream);
int dxmi_dmms_prep(const float* f_gen, const float* x_k, const float* noise, const int64_t* steps, const float* gen_sigmas,
                   int32_t num_steps, const int64_t* indices, const float* t_table, int32_t num_scales, float* x, float* x_t,
                   float* x_in_real, float* t_out, float* x_in_fake, int32_t N, int32_t CHW, float gen_sigma_data,
                   float real_sigma_data, float fake_sigma_data, void* stream);
int dxmi_dmms_out(const float* f_gen, const float* x_k, const float* gen_sigmas, int32_t num_steps, float* x, int32_t N, int32_t CHW,
                  float sigma_data, int32_t clip, void* stream);
int dxmi_dmms_bwd(const float* upstream, const float* g, const int64_t* steps, const float* gen_sigmas, int32_t num_steps,
                  float* d_f_gen, int32_t N, int32_t CHW, float sigma_data, void* stream);

/* Score identity Distillation of the same one-step generator (KarrasDenoiser.sid_generator_losses; SiD, Zhou et al., ICML 2024, the
 * fused loss L~^(alpha); csrc/sid_train.hip): the loss is differentiated through both denoisers with respect to their
 * input x_t, and these are the two launches around the two input-only backward walks.  Tensors, table, index rule, rounding and
 * sum order as for dxmi_dm_*.  With D_r, D_f as dxmi_dm_grad_fwd forms them, delta = D_r - D_f and e = D_f - x:
 * dxmi_sid_grad_fwd: s[n] = mean|x - D_r|, loss[n] = ((1 - alpha) sum(delta^2) + sum(delta e)) / (CHW s[n]) (0 where s == 0);
 *   a_r = 2 (1 - alpha) delta + e, a_f = (2 alpha - 1) delta - e; v_real = c_out_r a_r and v_fake = c_out_f a_f, the cotangents
 *   on f_real and f_fake, and d_dir = (c_skip_r a_r + c_skip_f a_f) - delta, all three WITHOUT the factor 1 / s.  One workgroup
 *   per image and one pass over the operands at every CHW.  alpha must be finite.
 * dxmi_sid_join: with g_real = J_real^T v_real and g_fake = J_fake^T v_fake, each with respect to its net's own input c_in x_t:
 *   g = ((d_dir + c_in_r g_real) + c_in_f g_fake) / s, 0 where s == 0: d loss_n / d x = g_n / CHW, the operand of dxmi_dm_gen_bwd.
 *   c_in is the same under the EDM and the boundary-condition scalings, so only the two sigma_data are taken.  g may alias d_dir
 *   (and nothing else). */
int dxmi_sid_grad_fwd(const float* f_real, const float* f_fake, const float* x, const float* x_t, const int64_t* indices,
                      const float* t_table, int32_t num_scales, float alpha, float* v_real, float* v_fake, float* d_dir, float* loss,
                      float* s, int32_t N, int32_t CHW, float real_sigma_data, float real_sigma_min, int32_t real_distillation,
                      float fake_sigma_data, float fake_sigma_min, int32_t fake_distillation, void* stream);
int dxmi_sid_join(const float* d_dir, const float* g_real, const float* g_fake, const float* s, const int64_t* indices,
                  const float* t_table, int32_t num_scales, float* g, int32_t N, int32_t CHW, float real_sigma_data,
                  float fake_sigma_data, void* stream);

/* Adversarial Score identity Distillation (SiDA, Zhou, Zheng et al. 2024; KarrasDenoiser.sida_generator_losses and
 * sida_discriminator_losses; csrc/sida_train.hip): a discriminator WITHOUT parameters on the fake denoiser's bottleneck
 * activation h, NHWC bf16 [N, P, Cb] (P positions, Cb channels, Cb % 8 == 0, Cb <= 4096, P <= 2^20, h and d_h 16-byte aligned):
 *   logit[n, p] = (1 / Cb) sum_c h[n, p, c],   a[n] = (1 / P) sum_p softplus(sign[n] logit[n, p]),
 * softplus in the form of dxmi_gan_logit_loss_fwd.  fp32, a fixed sum order that does not depend on N (an image gives the same bits
 * in every batch), no atomics.  sign (int32, -1 or +1 per image) and coef (fp32, finite) are HOST arrays of N values: they are checked
 * in the call (DXMI_EINVAL names the first bad index) and travel as kernel arguments, 64 images to a launch; nothing is copied and
 * nothing waits for the device.
 * dxmi_sida_map_fwd: h -> logit [N, P] and a [N].
 * dxmi_sida_map_bwd: d_h[n, p, c] = bf16((coef[n] upstream[n]) sign[n] sigmoid(sign[n] logit[n, p]) / (P Cb)) for every c: the
 *   cotangent of sum_n coef[n] upstream[n] a[n] with respect to h, rounded once.  upstream: fp32 [N] on the device (the per-image
 *   gradient an autograd backward receives), or NULL for 1. */
int dxmi_sida_map_fwd(const void* h, const int32_t* sign, float* logit, float* a, int32_t N, int32_t P, int32_t Cb, void* stream);
int dxmi_sida_map_bwd(const float* logit, const int32_t* sign, const float* coef, const float* upstream, void* d_h, int32_t N,
                      int32_t P, int32_t Cb, void* stream);

/* TD step of DxMI_Trainer.update_f_v on the replay ring, data side in one launch (reference trainer.py:271-300, :163-169): rows
 * `state_rows[b]` (and `next_rows[b]`, or the dense re-drawn next states of value_resample) of the ring's fp32 [n_src_rows, CHW]
 * trajectory block are gathered into out_state / out_next — the two halves of the batch [next_state | state] the value net
 * evaluates in one forward — and cost[b] = mean_CHW (x' - x)^2 / (2 beta) is reduced on the way.  INT path bit-exact; an index
 * outside [0, n_src_rows) fills the row with NaN.  beta: DEVICE scalar (betas_for_q[T - 1 - t]).  out_next may be NULL. */
int dxmi_td_gather_cost(const float* traj, const int64_t* state_rows, const int64_t* next_rows, const float* next_dense,
                        const float* beta, float* out_next, float* out_state, float* cost, int32_t B, int32_t CHW,
                        int64_t n_src_rows, void* stream);

/* TD loss of one step and its gradient (trainer.py:300-302: F.mse_loss(v(x_t), (v(x_t+1) + extra).detach())): v = the value
 * net's output on [next_state | state] ([2B]); grad[0..B) = 0, grad[B + i] = 2 (v[B + i] - v[i] - extra) / B;
 * logs3 = (loss, mean v(x_t), mean cost).  extra: DEVICE scalar (time-cost terms of the step) or NULL. */
int dxmi_td_loss(const float* v, const float* cost, const float* extra, float* grad, float* logs3, int32_t B, void* stream);

/* Parameter gradients of the value head (models/modules.py:146-163: relu, spatial sum, Linear(C,1), out_scale Linear(1,1)) in one
 * launch: s = the relu-sum features [N, C] dxmi_value_head_bwd returns, dy [N]; out = fp32 [C + 3] = d linear.weight |
 * d linear.bias | d out_scale.weight | d out_scale.bias (zeros when out_w is NULL).  Fixed summation order. */
int dxmi_value_head_pgrad(const float* s, const float* w, const float* b, const float* dy, const float* out_w, float* out,
                          int32_t N, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * InceptionV3 feature extractor of the FID evaluation (reference pytorch_fid/inception.py:16-163 with the FID patches
 * :193-310, called as `model(batch)[0]` by pytorch_fid/fid_score.py:170-221).  Shape-agnostic kernels (the net's maps are 149 ... 8
 * pixels wide, its kernels 1x1 ... 7x1): NHWC bf16 activations whose channel count is a multiple of 16, outputs written at a
 * channel offset of a wider tensor so that the blocks' concatenations are never materialised.
 * ---------------------------------------------------------------------------------------- */

/* bf16 elements of a packed generic-conv weight: [ceil32(Cout)][KH * KW][ceil16(Cin)]. */
int64_t dxmi_gconv_packed_elems(int32_t Cout, int32_t Cin, int32_t KH, int32_t KW);

/* BasicConv2d's weights for dxmi_gconv_fwd (torchvision Inception3: Conv2d(bias=False) + BatchNorm2d(eps) + ReLU): w fp32
 * [Cout, Cin, KH, KW]; the BatchNorm scale gamma / sqrt(var + eps) is folded into the bf16 weights, bias[ceil32(Cout)] = beta -
 * mean * scale.  bn_gamma NULL: plain conv (bias zero). */
int dxmi_gconv_pack(const float* w, const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var,
                    float bn_eps, void* w_packed, float* bias, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW, void* stream);

/* out[n, oy, ox, out_coff + co] = relu?(bias[co] + sum x[n, oy*SH - PH + ky, ox*SW - PW + kx, ci] * w[co][ky, kx][ci]) — implicit
 * GEMM on the bf16 MFMA, fp32 accumulation; x NHWC bf16 with Cin % 16 == 0 channels (the packed weight's padded count), out NHWC
 * bf16 with out_cstride channels per pixel.  OH = (IH + 2 PH - KH) / SH + 1 (likewise OW). */
int dxmi_gconv_fwd(const void* x, const void* w_packed, const float* bias, void* out, int32_t N, int32_t IH, int32_t IW,
                   int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t SH, int32_t SW, int32_t PH, int32_t PW,
                   int32_t out_cstride, int32_t out_coff, int32_t relu, void* stream);

/* 3x3 pooling, NHWC bf16: max (padding = -inf; F.max_pool2d) or, avg_exclude_pad != 0, the average over the window's IN-BOUNDS
 * pixels only (F.avg_pool2d(count_include_pad=False): the FID patch of inception.py:209-212).  pad 0 or 1. */
int dxmi_pool3x3(const void* x, void* out, int32_t N, int32_t IH, int32_t IW, int32_t C, int32_t stride, int32_t pad,
                 int32_t avg_exclude_pad, int32_t out_cstride, int32_t out_coff, void* stream);

/* adaptive_avg_pool2d(x, 1): [N, HW, C] bf16 -> [N, C] fp32 (pixels summed in order). */
int dxmi_global_avgpool(const void* x, float* out, int32_t N, int32_t HW, int32_t C, void* stream);

/* F.interpolate(x, (OH, OW), mode='bilinear', align_corners=False) (+ 2 x - 1 when normalize; inception.py:146-153): NCHW fp32
 * [N, 3, IH, IW] -> NHWC bf16 [N, OH, OW, 16] (channels 3..15 zero). */
int dxmi_resize_bilinear_nhwc16(const float* x, void* out, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW,
                                int32_t normalize, void* stream);

/* The same extractor in fp32 end to end (csrc/inception_f32.hip), as the reference runs it (pytorch_fid/inception.py:129-163 is
 * torch fp32; evaluations/evaluator.py:584-616): NHWC fp32 activations whose channel count is a multiple of 8, weights that are a
 * re-layout of the checkpoint's conv.weight with no arithmetic on them, BatchNorm in the conv epilogue.  Every entry validates its
 * arguments before it touches the device (DXMI_EINVAL + dxmi_last_error). */

/* fp32 elements of a packed weight: [ceil32(Cout)][KH * KW][ceil8(Cin)] (0 for a non-positive size). */
int64_t dxmi_gconv_f32_packed_elems(int32_t Cout, int32_t Cin, int32_t KH, int32_t KW);

/* BasicConv2d's operands for dxmi_gconv_f32_fwd (inception.py:193-310 over torchvision's BasicConv2d): w fp32 [Cout, Cin, KH, KW]
 * -> w_packed[co][ky * KW + kx][ci], copied bit for bit, padded couts / channels zero; scale[ceil32(Cout)] = gamma / sqrt(var + eps),
 * shift = beta - mean * scale (padding zero).  bn_gamma NULL: scale 1, shift = conv_bias (NULL: 0); conv_bias excludes BatchNorm. */
int dxmi_gconv_f32_pack(const float* w, const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var,
                        float bn_eps, const float* conv_bias, float* w_packed, float* scale, float* shift, int32_t Cout,
                        int32_t Cin, int32_t KH, int32_t KW, void* stream);

/* out[n, oy, ox, out_coff + co] = relu?(scale[co] * (sum x[n, oy*SH - PH + ky, ox*SW - PW + kx, ci] * w[co][ky, kx][ci]) + shift[co]):
 * dxmi_gconv_fwd's argument shape on the exact f32-input MFMA, fp32 accumulation over K = Cin * KH * KW in one fixed order per
 * layer shape (a pixel's result does not depend on N); Cin % 8 == 0 (the packed weight's padded count); one fp32 store. */
int dxmi_gconv_f32_fwd(const float* x, const float* w_packed, const float* scale, const float* shift, float* out, int32_t N,
                       int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t SH, int32_t SW,
                       int32_t PH, int32_t PW, int32_t out_cstride, int32_t out_coff, int32_t relu, void* stream);

/* dxmi_pool3x3 on NHWC fp32 (inception.py:209-212, :299-308): C % 8 == 0, out_cstride and out_coff multiples of 4; the maximum is
 * bitwise, the average is the in-order fp32 sum of the in-bounds pixels divided by their count. */
int dxmi_pool3x3_f32(const float* x, float* out, int32_t N, int32_t IH, int32_t IW, int32_t C, int32_t stride, int32_t pad,
                     int32_t avg_exclude_pad, int32_t out_cstride, int32_t out_coff, void* stream);

/* adaptive_avg_pool2d(x, 1) (inception.py:124): [N, HW, C] fp32 -> [N, C] fp32, pixels summed in index order; C % 8 == 0. */
int dxmi_global_avgpool_f32(const float* x, float* out, int32_t N, int32_t HW, int32_t C, void* stream);

/* dxmi_resize_bilinear_nhwc16's expressions (inception.py:146-153) with fp32 stores: NCHW fp32 [N, 3, IH, IW] -> NHWC fp32
 * [N, OH, OW, 8] (channels 3..7 zero). */
int dxmi_resize_bilinear_nhwc_f32(const float* x, float* out, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW,
                                  int32_t normalize, void* stream);

/* NHWC fp32 [N, HW, C] -> NCHW fp32 [N, C, HW] (the feature maps forward() returns, inception.py:155-163). */
int dxmi_nhwc_f32_to_nchw_f32(const float* in, float* out, int32_t N, int32_t C, int32_t HW, void* stream);

/* Replay-buffer row gather (INT path; trainer.py:278-289 `state_dict[key][indices][train_indices]`, :357-359):
 * dst[r] = src[idx[r]], rows of row_bytes (multiple of 4), idx int64 on the device, negative indices wrap; an index
 * outside [-n_src_rows, n_src_rows) fills the row with 0xFF bytes instead of reading out of bounds. */
int dxmi_gather_rows(const void* src, const int64_t* idx, void* dst, int64_t n_rows, int64_t n_src_rows,
                     int64_t row_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * FID activation statistics (the part that needs no Inception weights).
 * Replaces, on the device, the host-side numpy statistics the reference takes of the gathered activations:
 *   m1, s1 = np.mean(act, axis=0), np.cov(act, rowvar=False)
 * at train_image_large.py:62-69 (fid()), train_cifar10.py (fid()), and pytorch_fid/fid_score.py:283-303
 * (calculate_activation_statistics).  act: fp32 [N, D] row-major (D % 4 == 0: pytorch_fid's feature sizes are 64 / 192 /
 * 768 / 2048) -> mu fp64 [D], sigma fp64 [D, D] (unbiased, N - 1, as np.cov).  Column means in fp64; the centred Gram matrix on
 * the f32-input MFMA (exact fp32 products, fp32 accumulation inside a row split), splits folded in fp64 in a fixed order
 * (bitwise reproducible).  workspace: dxmi_fid_stats_workspace_bytes(N, D) bytes.
 * The Frechet distance itself (a 2048 x 2048 matrix square root, fid_score.py:224-281) has two forms in pytorch_fid/fid_score.py of
 * this package: calculate_frechet_distance, the reference's float64 host algorithm (scipy.linalg.sqrtm), and its device sibling
 * calculate_frechet_distance_device on the fp64 kernels below.
 * ---------------------------------------------------------------------------------------- */
int64_t dxmi_fid_stats_workspace_bytes(int64_t N, int32_t D);
int dxmi_fid_stats(const float* act, int64_t N, int32_t D, double* mu, double* sigma, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp64 matrix kernels of the Frechet distance (csrc/frechet.hip): tr sqrt(S1 S2) of symmetric PSD S1, S2 by the
 * coupled Newton-Schulz iteration on symmetric matrices (dxmi_hip/ops.py frechet_trace_sqrt holds the loop).  All matrices are
 * fp64 row-major n x n on the device, n % 16 == 0, 16 <= n <= 4096.  Every reduction runs in a fixed order without atomics: two
 * calls give bitwise the same result.  Inf and NaN flow through as arithmetic.
 *
 * dxmi_gemm_f64: C = alpha * A * B + diag * I on v_mfma_f64_16x16x4_f64.  A, B, C 16-byte aligned; C must not overlap A or B
 * (A may be B).  trace, if not NULL, receives trace(C) as a device double (a second, one-workgroup launch over C's diagonal).
 * dxmi_frob_norm_f64: *out = ||X||_F (device double); workspace: dxmi_frechet_workspace_bytes(n) bytes.
 * dxmi_scale_f64: Y = alpha * X (Y may be X itself).   dxmi_symmetrize_f64: X <- (X + X^T) / 2 in place.
 * ---------------------------------------------------------------------------------------- */
int64_t dxmi_frechet_workspace_bytes(int32_t n);
int dxmi_gemm_f64(const double* A, const double* B, double* C, int32_t n, double alpha, double diag, double* trace, void* stream);
int dxmi_frob_norm_f64(const double* X, int32_t n, double* out, void* workspace, void* stream);
int dxmi_scale_f64(const double* X, double* Y, int32_t n, double alpha, void* stream);
int dxmi_symmetrize_f64(double* X, int32_t n, void* stream);

/* ----------------------------------------------------------------------------------------
 * Sample-quality metrics of the ADM evaluator (reference evaluations/evaluator.py), csrc/eval_metrics.hip.
 * Every pairwise distance is d(u, v) = max((|u|^2 + |v|^2) - 2 u.v, 0) in f32, u.v a K-ordered fmaf chain on the f32-input MFMA
 * and |u|^2 the same chain: a pair's value is bitwise the same in every kernel, tile, column split and argument order.
 *
 * dxmi_knn_radii: ManifoldEstimator.manifold_radii (evaluator.py:243-280, one nhood size, clamp_to_percentile=None).
 * x fp32 [N, D] row-major -> radii fp32 [N]: radii[i] = np.partition(d(x_i, x_*), k)[k] (the self-distance 0 and duplicates
 * count).  1 <= k <= 7, N >= k + 1.  splits: the number of column ranges the N x N work is cut into (0: automatic); the
 * result does not depend on it.  Nothing N x N is allocated: workspace dxmi_knn_radii_workspace_bytes(N, D, k, splits)
 * = N row norms + 2 * splits * N * (k + 1) floats.
 * ---------------------------------------------------------------------------------------- */
int64_t dxmi_knn_radii_workspace_bytes(int64_t N, int32_t D, int32_t k, int32_t splits);
int dxmi_knn_radii(const float* x, int64_t N, int32_t D, int32_t k, int32_t splits, float* radii, void* workspace, void* stream);

/* dxmi_pr_membership: ManifoldEstimator.evaluate_pr / DistanceBlock.less_thans (evaluator.py:328-417).  Reference set A fp32
 * [NA, D] with radii rA [NA], sample set B fp32 [NB, D] with radii rB [NB] ->
 *     a_in_b[i] = any_j d(a_i, b_j) <= rB[j]     (int32 0 / 1 [NA]; mean = recall)
 *     b_in_a[j] = any_i d(a_i, b_j) <= rA[i]     (int32 0 / 1 [NB]; mean = precision)
 * in one launch over 128 x 128 tiles of the NA x NB distances (nothing materialised).  workspace:
 * dxmi_pr_membership_workspace_bytes(NA, NB) (the row norms of both sets). */
int64_t dxmi_pr_membership_workspace_bytes(int64_t NA, int64_t NB);
int dxmi_pr_membership(const float* A, int64_t NA, const float* rA, const float* B, int64_t NB, const float* rB, int32_t D,
                       int32_t* a_in_b, int32_t* b_in_a, void* workspace, void* stream);

/* dxmi_kid_sums: the Gram sums of the Kernel Inception Distance (Binkowski, Sutherland, Arbel, Gretton 2018, "Demystifying MMD
 * GANs", the unbiased MMD^2 estimate with the polynomial kernel).  X fp32 [NX, D], Y fp32 [NY, D]; idx_x int32
 * [S, mx] and idx_y int32 [S, my] name the rows of S subsets, x_i = X[idx_x[s, i]], y_j = Y[idx_y[s, j]] (device).  Both NULL: S = 1
 * and the subset is every row (mx = NX, my = NY).  sums fp64 [S, 3] (device):
 *     sums[s, 0] = Sxx = sum_{i != j} k(x_i, x_j)     sums[s, 1] = Syy = sum_{i != j} k(y_i, y_j)     sums[s, 2] = Sxy = sum_{i, j} k(x_i, y_j)
 *     k(u, v) = t^3,  t = (double)(u . v) * gamma + coef0     (u . v the f32 dot above; t, the cube and every sum in fp64, no fma)
 * The estimate is (Sxx / (mx (mx - 1)) + Syy / (my (my - 1)) - 2 Sxy / (mx my)) (host).  One launch covers all subsets (rows are
 * gathered through the index in the tile loader, no gathered copy), X.X and Y.Y run their upper-triangular tiles only, and a second
 * launch adds each subset's per-tile partials: no atomics, a summation order that depends on (mx, my, D) alone, bitwise reproducible.
 * An index outside [0, NX) / [0, NY) is never dereferenced and makes that subset's three sums NaN.  2 <= mx, my.  workspace:
 * dxmi_kid_sums_workspace_bytes(S, mx, my, D) = one double per tile, S * (Tx (Tx + 1) / 2 + Ty (Ty + 1) / 2 + Tx Ty) with
 * Tx = ceil(mx / 128), Ty = ceil(my / 128); 0 for shapes dxmi_kid_sums refuses. */
int64_t dxmi_kid_sums_workspace_bytes(int64_t S, int64_t mx, int64_t my, int32_t D);
int dxmi_kid_sums(const float* X, int64_t NX, const float* Y, int64_t NY, int32_t D, const int32_t* idx_x, const int32_t* idx_y,
                  int64_t S, int64_t mx, int64_t my, double gamma, double coef0, double* sums, void* workspace, void* stream);

/* dxmi_dc_counts: the ball counts of density and coverage (Naeem, Oh, Uh, Choi, Yoo 2020, "Reliable Fidelity and Diversity
 * Metrics for Generative Models", eq. 4 and 5, as the `prdc` package computes them).  Reference set A fp32 [NA, D]
 * with its k-NN radii rA [NA] (dxmi_knn_radii), sample set B fp32 [NB, D] ->
 *     counts[i] = #{ j : d(a_i, b_j) < rA[i] }     (int32 [NA]; strict, where dxmi_pr_membership uses <=)
 * density = sum_i counts[i] / (k NB), coverage = mean_i (counts[i] > 0) (host).  splits: the number of column ranges B is cut
 * into (0: automatic); the result does not depend on it.  No atomics, nothing NA x NB: workspace
 * dxmi_dc_counts_workspace_bytes(NA, NB, splits) = the row norms of both sets + splits * NA int32. */
int64_t dxmi_dc_counts_workspace_bytes(int64_t NA, int64_t NB, int32_t splits);
int dxmi_dc_counts(const float* A, int64_t NA, const float* rA, const float* B, int64_t NB, int32_t D, int32_t splits, int32_t* counts,
                   void* workspace, void* stream);

/* dxmi_inception_score: Evaluator.compute_inception_score (evaluator.py:179-193) with the classifier weight only
 * (`softmax/logits/MatMul`, evaluator.py:603-616: no bias).  pool fp32 [N, D], w fp32 [C, D] (fc.weight layout) ->
 * kl_mean fp64 [ceil(N / split)] (device): for each split of `split` rows, mean_r sum_c p (log p - log p_bar) with
 * p = softmax(pool . w^T) in f32 and p_bar the split's marginal; the sums in fp64 in a fixed order (bitwise reproducible).
 * The score is mean_s exp(kl_mean[s]) (host).  workspace: dxmi_inception_score_workspace_bytes(N, C, split). */
int64_t dxmi_inception_score_workspace_bytes(int64_t N, int32_t C, int32_t split);
int dxmi_inception_score(const float* pool, int64_t N, int32_t D, const float* w, int32_t C, int32_t split, double* kl_mean,
                         void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Karras samplers of the EDM teacher: karras_sample / sample_heun / sample_dpm / sample_euler / sample_euler_ancestral
 * (models/cm/karras_diffusion.py:354-420, :447-640; scalings :64-68, denoise :337-351, to_d :432-434).
 * dxmi_karras_stage is the ONE launch between two network evaluations.  With F the output of the evaluation just done at
 * the point x_e (x, or x2 for the correctors) and noise level s = tab[row][SIGMA], per element in fp32 and in the reference's
 * operation order (no fused multiply-add):
 *     denoised = c_out F + c_skip x_e, clamped to [-1, 1] if CLIP != 0 (clip_denoised, :408-412) -> denoised (if not NULL)
 *     d        = (x_e - denoised) / s
 *   DXMI_KARRAS_FIRST      x = x * XSCALE                    (x_T = randn * sigma_max; F unused)
 *   DXMI_KARRAS_PRED       d -> d;  x2 = x + d DT            (heun :541-542 with DT = sigma_next - sigma_hat;
 *                                                             dpm :614-617 with DT = sigma_mid - sigma_hat)
 *   DXMI_KARRAS_HEUN_CORR  x' = x + ((d_saved + d) / 2) DT   (:543-546; x_e = x2)
 *   DXMI_KARRAS_DPM_CORR   x' = x + d DT                     (:618-620; x_e = x2, DT = dt_2)
 *   DXMI_KARRAS_EULER      x' = x + d DT                     (:576-577; heun's last step :537-539)
 *   DXMI_KARRAS_ANCESTRAL  x' = x + d DT; x' = x' + z SIGMA_UP (:476-478; DT = sigma_down - sigma; z = noise, NULL = 0)
 * then, except after PRED:  last ? out = clamp(x', -1, 1)  (:420)
 *                                : x = x' + (eps SNOISE) CHURN  (next step's churn :523-527, only when noise = eps is not NULL
 *                                                                and the mode is not ANCESTRAL);
 * and, unless last, the next evaluation's input x_in = CIN x (x2 after PRED) and t[n] = T.  tab: fp32 [rows][DXMI_KT_COLS],
 * device; row: the row of this launch.  x, x2, d, model_out, noise, x_in, out, denoised: fp32 [N, CHW] (x, x2, d read and
 * written in place).  CHW must be a multiple of 4. */
#define DXMI_KARRAS_FIRST      0
#define DXMI_KARRAS_PRED       1
#define DXMI_KARRAS_HEUN_CORR  2
#define DXMI_KARRAS_DPM_CORR   3
#define DXMI_KARRAS_EULER      4
#define DXMI_KARRAS_ANCESTRAL  5
#define DXMI_KT_SIGMA     0   /* noise level of the evaluation the launch follows (the divisor of d) */
#define DXMI_KT_CSKIP     1   /* c_skip(SIGMA) */
#define DXMI_KT_COUT      2   /* c_out(SIGMA) */
#define DXMI_KT_DT        3   /* step of the update */
#define DXMI_KT_SIGMA_UP  4   /* ancestral noise scale */
#define DXMI_KT_CHURN     5   /* (sigma_hat^2 - sigma^2)^0.5 of the next step */
#define DXMI_KT_SNOISE    6   /* s_noise */
#define DXMI_KT_CIN       7   /* c_in of the next evaluation's noise level */
#define DXMI_KT_T         8   /* 250 ln(next noise level + 1e-44) */
#define DXMI_KT_XSCALE    9   /* scale of the initial draw: sigma_max for karras_sample, 1 when x is given (FIRST) */
#define DXMI_KT_CLIP     10   /* 1: clip_denoised */
#define DXMI_KT_COLS      16
int dxmi_karras_stage(int32_t mode, int32_t last, const float* tab, int32_t row, float* x, float* x2, float* d,
                      const float* model_out, const float* noise, float* x_in, float* t_out, float* out, float* denoised,
                      int32_t N, int32_t CHW, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Consistency-model sampling and zero-shot editing: sample_onestep / stochastic_iterative_sampler (the `multistep` sampler) /
 * iterative_colorization / iterative_inpainting / iterative_superres (models/cm/karras_diffusion.py:644-683, :722-951;
 * boundary-condition scalings :70-80, chosen by denoise :336-351; dispatch karras_sample :354-420).
 * dxmi_cm_stage is the ONE launch between two network evaluations.  With F the output of the evaluation just done at the
 * state x, per element in fp32 and in the reference's operation order (no fused multiply-add):
 *   DXMI_CM_FIRST  x = x * XSCALE                           (x_T = randn * sigma_max; F unused, no edit, no noise)
 *   DXMI_CM_STEP   x0 = c_out F + c_skip x, clamped to [-1, 1] if CLIP != 0            -> denoised (if not NULL)
 *                  edit:  NONE    x0
 *                         MASK    ref m + x0 (1 - m)                                   (iterative_inpainting :803-805)
 *                         COLOUR  per pixel y = v^T Q over the 3 channel planes (Q: 3x3), y_0 from ref, y_1..2 from x0,
 *                                 x0 = Q y                                             (iterative_colorization :741-747)
 *                         PATCH   per 8x8 patch of each plane, in-patch index d = 8 row + col, y = v^T Q (Q: 64x64),
 *                                 y_0 from ref, y_1..63 from x0, x0 = Q y              (iterative_superres :858-900)
 *                  x' = x0 + z NOISE                       (z = noise; NULL = 0: the draw is skipped)
 *                  last ? out = x', clamped to [-1, 1] if OUTCLAMP != 0 (karras_sample :420)
 *                       : x = x'
 * and, unless last, the next evaluation's input x_in = CIN x and t[n] = T.  tab: fp32 [rows][DXMI_CT_COLS], device; row: the
 * row of this launch.  Q: fp32 row-major (Q[d][e] at Q + d * dim + e), device.  x, model_out, noise, ref, mask, x_in, out,
 * denoised: fp32 [N, C, H, W] (x read and written in place).  C*H*W must be a multiple of 4 (NONE, MASK); COLOUR needs C = 3
 * and H*W a multiple of 4; PATCH needs H and W multiples of 8.  The Q transforms sum in another order than the reference's
 * einsum: per element |err| <= c u32 sum|Q||v|. */
#define DXMI_CM_FIRST        0
#define DXMI_CM_STEP         1
#define DXMI_CM_EDIT_NONE    0
#define DXMI_CM_EDIT_MASK    1
#define DXMI_CM_EDIT_COLOUR  2
#define DXMI_CM_EDIT_PATCH   3
#define DXMI_CT_CSKIP     0   /* c_skip of the evaluation the launch follows (boundary-condition or plain) */
#define DXMI_CT_COUT      1   /* c_out of that evaluation */
#define DXMI_CT_NOISE     2   /* sqrt(next_t^2 - t_min^2), float64 then rounded once (0 for onestep) */
#define DXMI_CT_CIN       3   /* c_in of the next evaluation's noise level */
#define DXMI_CT_T         4   /* 250 ln(next noise level + 1e-44) */
#define DXMI_CT_XSCALE    5   /* scale of the initial draw: sigma_max for karras_sample, 1 when x is given (FIRST) */
#define DXMI_CT_CLIP      6   /* 1: clamp denoised (clip_denoised, and always in the editing loops) */
#define DXMI_CT_OUTCLAMP  7   /* 1: clamp the final output (karras_sample) */
#define DXMI_CT_COLS      8
int dxmi_cm_stage(int32_t mode, int32_t edit, int32_t last, const float* tab, int32_t row, const float* Q, float* x,
                  const float* model_out, const float* noise, const float* ref, const float* mask, float* x_in, float* t_out,
                  float* out, float* denoised, int32_t N, int32_t C, int32_t H, int32_t W, void* stream);

/* LPIPS (piq's LPIPS(replace_pooling=True, reduction="none") on torchvision's VGG16 features) as a device loss: the launches around
 * the 13 convolutions, which go through dxmi_gconv_fwd forward and, with transposed-and-flipped packed weights, backward.
 * Activations and gradients are NHWC bf16; every sum is fp32 and taken in a fixed order (bitwise reproducible, no atomics).
 * dxmi_lpips_front_fwd: x fp32 [N, 3, IH, IW] in [0, 1] -> F.interpolate(size=(OH, OW), mode="bilinear") (align_corners False; the
 *   identity when the sizes agree) -> (v - mean) / std -> out bf16 [N, OH, OW, 16], channels 3..15 zero.
 * dxmi_lpips_front_bwd: its transpose from g_out bf16 [N, OH, OW, 16] (channels 0..2 read) to d_x fp32 [N, 3, IH, IW], 1 / std included.
 * dxmi_avgpool2x2_fwd: AvgPool2d(2, 2, 0), x [N, IH, IW, C] -> out [N, IH / 2, IW / 2, C] (floor).  dxmi_avgpool2x2_bwd: g_out of that shape
 *   -> g_in [N, IH, IW, C]; a dropped last row / column gets zero.  C % 8 == 0.
 * dxmi_lpips_tap_fwd: fx, fy bf16 [N, HW, C], w fp32 [C]: per pixel f^ = f / (sqrt(sum_c f^2) + 1e-10) of both,
 *   v[n] = (1 / HW) sum_pixels sum_c w_c (fx^ - fy^)^2; out[n] = (accumulate ? out[n] : 0) + v[n], then times scale[n] if scale is not
 *   NULL.  partials: fp32 workspace of N * dxmi_lpips_tap_partials(HW, C) elements.  C % 16 == 0, 16 <= C <= 512.
 * dxmi_lpips_tap_bwd: d_fx bf16 [N, HW, C] of v[n] for the upstream g[n] (NULL: 1), through the normalisation; zero-norm pixels take
 *   the subgradient 0 of the norm.  fy is a constant.
 * dxmi_relu_mask_acc: out = (g_a + g_b) * (act > 0) over numel bf16 values (g_b NULL: g_a alone); numel % 8 == 0. */
int dxmi_lpips_front_fwd(const float* x, void* out, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW, void* stream);
int dxmi_lpips_front_bwd(const void* g_out, float* d_x, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW, void* stream);
int dxmi_avgpool2x2_fwd(const void* x, void* out, int32_t N, int32_t IH, int32_t IW, int32_t C, void* stream);
int dxmi_avgpool2x2_bwd(const void* g_out, void* g_in, int32_t N, int32_t IH, int32_t IW, int32_t C, void* stream);
int64_t dxmi_lpips_tap_partials(int32_t HW, int32_t C);
int dxmi_lpips_tap_fwd(const void* fx, const void* fy, const float* w, const float* scale, float* partials, float* out, int32_t N,
                       int32_t HW, int32_t C, int32_t accumulate, void* stream);
int dxmi_lpips_tap_bwd(const float* g, const void* fx, const void* fy, const float* w, void* d_fx, int32_t N, int32_t HW, int32_t C,
                       void* stream);
int dxmi_relu_mask_acc(const void* g_a, const void* g_b, const void* act, void* out, int64_t numel, void* stream);
/* The lpips norm of the consistency losses (reference :221-234) around that network.  dxmi_cd_lpips_images: with the scalings of
 * dxmi_cd_loss_fwd, x01 fp32 [2 N, CHW] = (distiller + 1) / 2 in rows [0, N) and (target + 1) / 2 in rows [N, 2 N), and
 * weights[n] = get_weightings(weight_schedule, t^-2).  dxmi_cd_lpips_bwd: d_f_online = ((g_loss w) d_x01 / 2) c_out(t) for d_x01
 * fp32 [N, CHW], the gradient of the LPIPS value into the online image at unit upstream. */
int dxmi_cd_lpips_images(const float* f_online, const float* f_target, const float* x_t, const float* x_t2, const int64_t* indices,
                         const float* t_table, int32_t num_scales, float* x01, float* weights, int32_t N, int32_t CHW, float sigma_data,
                         float sigma_min, int32_t distillation, int32_t weight_schedule, void* stream);
int dxmi_cd_lpips_bwd(const float* g_loss, const float* d_x01, const int64_t* indices, const float* t_table, int32_t num_scales,
                      float* d_f_online, int32_t N, int32_t CHW, float sigma_data, float sigma_min, int32_t distillation,
                      int32_t weight_schedule, void* stream);

/* Training batches from a uint8 image array (csrc/image_batch.hip): what the reference's loaders do per image on the
 * host (models/cm/image_datasets.py:115-119 `arr[:, ::-1]`, `arr.astype(np.float32) / 127.5 - 1`, `np.transpose(arr, [2, 0, 1])`;
 * loader/__init__.py:14-15 RandomHorizontalFlip + ToTensor, then train_cifar10.py:170 `2 * images - 1`) as ONE launch per batch.
 * store: uint8 [n_rows, H, W, C] on the device (`arr_0` of the evaluator's .npz batches and of make_npz.py), C = 3 or 1.
 * idx: int64 [B] on the device, the source row of each output image; NULL = rows 0 .. B-1 (B <= n_rows).  An index outside
 * [0, n_rows) fills that image with NaN and reads nothing outside the store (no wrap-around).  flip: uint8 [B] on the device,
 * nonzero mirrors the image along W; NULL = no flips.  out: fp32 [B, C, H, W].  norm, one rounding per operation:
 *   DXMI_IMG_NORM_ADM       v / 127.5f - 1.0f
 *   DXMI_IMG_NORM_TOTENSOR  2.0f * (v / 255.0f) - 1.0f
 * W % 16 == 0 with 16-byte aligned store and out: 16-byte loads of interleaved pixels, f32x4 stores per channel plane, the flip in
 * the store index.  Anything else: one element per lane.  No workspace; bitwise reproducible. */
#define DXMI_IMG_NORM_ADM       0
#define DXMI_IMG_NORM_TOTENSOR  1
int dxmi_image_batch(const void* store, int64_t n_rows, const int64_t* idx, const uint8_t* flip, float* out, int32_t B, int32_t H,
                     int32_t W, int32_t C, int32_t norm, void* stream);

/* Batch- and rank-invariant sampling noise (csrc/randn_indexed.hip): the device form of the reference's
 * DeterministicGenerator / DeterministicIndividualGenerator (models/cm/random_util.py:28-182), whose one property is that image i of
 * a run sees the same noise whatever the batch size and however many ranks share the run.  A counter-based generator: every value is
 * a pure function of (seed, sample_index[n], draw, element), and one launch produces a draw for the whole batch.  The stream is this
 * library's own; it matches neither torch's CPU nor torch's device generator.
 * out: [N, per_sample] contiguous, 16-byte aligned.  sample_index: int64 [N] on the device, the global index of row n (any int64; its
 * 64 bits go into the counter, so indices above 2^32 stay distinct).  A row depends on its own index only: not on n, N or the launch.
 * Generator: Philox-4x32-10 (Salmon et al., SC'11; Random123) with the published constants (multipliers 0xD2511F53, 0xCD9E8D57, key
 *   increments 0x9E3779B9, 0xBB67AE85).  key = (seed & 0xffffffff, seed >> 32); counter = (block, draw, index & 0xffffffff,
 *   index >> 32) with block = e / 4 for element e of the row: the four output words x0..x3 of one call are elements 4 block .. 4 block + 3.
 * dxmi_randn_indexed: uniforms u(x) = ((x >> 9) + 0.5f) * 2^-23, exact in fp32 and inside [2^-24, 1 - 2^-24] (23 bits: with 24 the
 *   half would not fit the significand for x >> 8 >= 2^23, and the sum would round to 1.0 at the top).  Box-Muller on the pairs
 *   (x0, x1) and (x2, x3): r = sqrtf(-2.f * logf(u(x_a))), t = 6.2831855f * u(x_b), z_a = r * cosf(t), z_b = r * sinf(t); so
 *   |z| <= sqrt(48 ln 2) = 5.77.  fp32 throughout, one rounding per operation (no fused multiply-add); logf, sinf and cosf are the device
 *   library's (ROCm OCML, ~1 ulp), sqrtf is correctly rounded: the bits of a normal depend on them, so they may change with the
 *   ROCm release, while the raw words never do.
 * dxmi_randint_indexed: out int64, element e = low + (x_(e % 4) mod (high - low)) from the same words, one 32-bit word per element;
 *   1 <= high - low <= 2^31 (wider ranges: DXMI_EINVAL).  The usual modulo bias, below (high - low) / 2^32.  low = 0, high = 2^31
 *   exposes the low 31 bits of every word.
 * N in [1, 65535], per_sample in [1, 2^31 - 1].  f32x4 stores per lane where the rows are 16-byte aligned (per_sample % 4 == 0), 4-byte
 * aligned vector stores otherwise, the last per_sample % 4 elements one by one.  No workspace, no LDS, no atomics. */
int dxmi_randn_indexed(float* out, const int64_t* sample_index, int32_t N, int64_t per_sample, uint64_t seed, uint32_t draw,
                       void* stream);
int dxmi_randint_indexed(int64_t* out, const int64_t* sample_index, int32_t N, int64_t per_sample, int64_t low, int64_t high,
                         uint64_t seed, uint32_t draw, void* stream);

/* The DxMI samplers' transitions with the noise made in the launch (csrc/step_indexed.hip): dxmi_var_step_fwd and
 * dxmi_edm_step_fwd without their z operand.  The kernel makes
 *   z[n][e] = the value dxmi_randn_indexed gives for (seed, sample_index[n], draw, e)
 * (key = the two halves of the seed, counter = (e / 4, draw, index low word, index high word), the same Philox / Box-Muller
 * functions: the same bits) and then forms what the launch it is named after forms from x, the network output and z.  Every output
 * is BIT FOR BIT that of dxmi_randn_indexed followed by dxmi_var_step_fwd / dxmi_edm_step_fwd on the z it wrote: the fused
 * multiply-adds those two kernels are compiled to are written out here (VAR: mean = fma(xmul, x, control), assoc 1: x' = xmul x +
 * fma(sigma, z, control), assoc 0: x' = fma(sigma, z, mean); EDM: denoised = fma(c_out, F, c_skip x), mean = fma(sigma_down - sigma,
 * d, x), sample = fma(sigma_up, z, mean); everything else one rounding per operation), and logp is reduced in the same order.  The
 * launch saves the pair one launch and one write plus read of z per transition.
 * dxmi_var_step_fwd_indexed: x_next, mean, control ([N, CHW]) and logp ([N]) as dxmi_var_step_fwd writes them, assoc 0 or 1 with its
 *   meaning there; mean, control and logp may be NULL.
 * dxmi_edm_step_fwd_indexed: sample and mean ([N, CHW]) as dxmi_edm_step_fwd writes them; N <= 65535.
 * sample_index: int64 [N] on the device, the global index of row n; a row's noise depends on its own index only.
 * Control: ctl NULL: draw and seed are the by-value arguments.  ctl not NULL: an int32[4] block on the DEVICE laid out as that of
 *   dxmi_ddpm_stage = (unused, draw, seed low word, seed high word), read by the kernel (the by-value two are ignored), so a
 *   captured launch is fed per replay.
 * DXMI_EINVAL with a message and no launch: a null pointer (but the optional ones), N <= 0, CHW not a multiple of 4 in [4, 2^30],
 *   assoc outside {0, 1}, or a misaligned tensor (x, the network output and the [N, CHW] outputs 16-byte; sample_index 8-byte; ctl, the
 *   per-sample vectors and logp 4-byte).  One workgroup per image (VAR) or per 1024 elements up to 64 per image (EDM), f32x4 per
 *   lane; with the generator the launch is VALU-bound.  No workspace, no atomics; LDS: VAR's four partial sums. */
int dxmi_var_step_fwd_indexed(const float* x, const float* eps, const int64_t* sample_index, const int32_t* ctl, uint32_t draw,
                              uint64_t seed, const float* xmul, const float* cmul, const float* sigma, float* x_next, float* mean,
                              float* control, float* logp, int32_t N, int32_t CHW, int32_t assoc, void* stream);
int dxmi_edm_step_fwd_indexed(const float* x, const float* model_out, const int64_t* sample_index, const int32_t* ctl, uint32_t draw,
                              uint64_t seed, const float* sigma, const float* sigma_down, const float* sigma_up, float* sample,
                              float* mean, int32_t N, int32_t CHW, float sigma_data, void* stream);

/* Ancestral / DDIM sampling of the DDPM teacher (csrc/ddpm_sample.hip; models/DxMI/ddpm_sample.py): Ho et al. 2020,
 * "Denoising Diffusion Probabilistic Models", Algorithm 2; Song et al. 2021, "Denoising Diffusion Implicit Models", eq. 12 and 16.
 * dxmi_ddpm_stage is the ONE launch between two network evaluations.  With eps the output of the evaluation just done at the state
 * x and K = tab[row], per element in fp32, one rounding per operation (no fused multiply-add but the linear form's one):
 *     x0 = K[A] x - K[B] eps                                  (the predicted x_0; A = 1 / sqrt(a_t), B = sqrt(1 / a_t - 1))
 *   FLAG_CLIP set (clip_denoised):
 *     x0c = clamp(x0, -1, 1);  eps_hat = (x - K[Q] x0c) K[R]    (Q = sqrt(a_t), R = 1 / sqrt(1 - a_t))
 *     x'  = (K[C0] x0c + K[C1] eps_hat) + K[S] z                (C0 = sqrt(a_p), C1 = sqrt(1 - a_p - sigma^2))
 *     pred_xstart = x0c
 *   FLAG_CLIP clear (the linear form, the association of dxmi_var_step_fwd with assoc = 1):
 *     x'  = K[XM] x + fma(K[S], z, K[C] eps);  pred_xstart = x0    (that launch's one fused multiply-add, so the two agree bit for bit)
 *   a row with K[S] == 0 adds no noise: it reads neither z nor the generator (x' = K[C0] x0c + K[C1] eps_hat, K[XM] x + K[C] eps).
 * then x = x' in place, t_out[n] = K[T_NEXT] (the next evaluation's time) and, on a row with FLAG_LAST, out = clamp(x', -1, 1).
 * pred_xstart is written when not NULL.  A NaN in eps reaches x' (the clamps pass it); images do not mix.
 * DXMI_DDPM_FIRST writes t_out[n] = K[T] only (the first evaluation's time); x, eps, out may be NULL.
 * Control: ctl NULL: row, draw and seed are the by-value arguments, and row outside [0, rows) is DXMI_EINVAL.  ctl not NULL: an
 *   int32[4] block on the DEVICE = (row, draw, seed low word, seed high word) read by the kernel (the by-value three are ignored),
 *   so a captured launch serves every row; a row outside [0, rows) read there gives NaN in x, out and t_out, and nothing outside
 *   the table is read.
 * Noise: z (fp32 [N, CHW]) is given, or z == NULL and sample_index (int64 [N], DEVICE) is: the kernel then makes
 *   z[n][e] = the value dxmi_randn_indexed gives for (seed, sample_index[n], draw, e) (same counter layout, same functions: the
 *   same bits).  Both NULL: no noise is added.  Both given: DXMI_EINVAL.
 * tab: fp32 [rows][DXMI_DT_COLS] on the device.  x, eps, z, out, pred_xstart: fp32 [N, CHW], 16-byte aligned; CHW % 4 != 0 takes
 * 4-byte aligned vector accesses and a scalar tail.  N in [1, 65535].  No workspace, no LDS, no atomics. */
#define DXMI_DDPM_FIRST   0
#define DXMI_DDPM_STEP    1
#define DXMI_DT_T         0   /* time of the evaluation the launch follows: (float)tau_k */
#define DXMI_DT_T_NEXT    1   /* time of the next evaluation (0 on the last row) */
#define DXMI_DT_XM        2   /* linear form: sqrt(a_p / a_t) */
#define DXMI_DT_C         3   /* linear form: sqrt(1 - a_p - sigma^2) - sqrt(1 - a_t) sqrt(a_p / a_t) */
#define DXMI_DT_S         4   /* noise scale s (0 on the last row, and everywhere for eta = 0) */
#define DXMI_DT_A         5   /* 1 / sqrt(a_t) */
#define DXMI_DT_B         6   /* sqrt(1 / a_t - 1) */
#define DXMI_DT_Q         7   /* sqrt(a_t) */
#define DXMI_DT_R         8   /* 1 / sqrt(1 - a_t) */
#define DXMI_DT_C0        9   /* sqrt(a_p) */
#define DXMI_DT_C1       10   /* sqrt(1 - a_p - sigma^2) */
#define DXMI_DT_FLAGS    11   /* DXMI_DT_FLAG_* summed, stored as a float */
#define DXMI_DT_COLS     16
#define DXMI_DT_FLAG_CLIP 1
#define DXMI_DT_FLAG_LAST 2
int dxmi_ddpm_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw, uint64_t seed,
                    float* x, const float* eps, const float* z, const int64_t* sample_index, float* t_out, float* out,
                    float* pred_xstart, int32_t N, int32_t CHW, void* stream);

/* DPM-Solver++ sampling of the DDPM teacher (csrc/dpm_sample.hip; models/DxMI/dpm_sample.py): Lu, Zhou, Bao, Chen,
 * Li and Zhu 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models" (arXiv:2211.01095), the
 * multistep data-prediction solver of Algorithm 2 at orders 1-3 and its SDE variant at orders 1-2 (the reference tree has no such
 * sampler).  dxmi_dpm_stage is the ONE launch between two network evaluations.  With eps the output of evaluation k = row at the
 * state x and K = tab[row], per element in fp32, one rounding per operation (no fused multiply-add), in this order:
 *     D0  = K[A] x - K[B] eps;  FLAG_CLIP: D0 = clamp(D0, -1, 1)        (the data prediction; A = 1 / alpha_t, B = sigma_t / alpha_t)
 *     acc = K[CX] x + K[W0] D0
 *     acc += K[W1] D1     if K[W1] != 0       (D1 = D_{k-1}, the data prediction of the evaluation before)
 *     acc += K[W2] D2     if K[W2] != 0       (D2 = D_{k-2})
 *     acc += K[S] z       if K[S] != 0
 * then x = acc in place, hist[row % 3] = D0, t_out[n] = K[T_NEXT] (the next evaluation's time) and, on a row with FLAG_LAST,
 * out = clamp(acc, -1, 1).  pred_xstart = D0 is written when not NULL.  A NaN in eps reaches x' (the clamps pass it); images do not
 * mix.
 * History: hist is fp32 [3][N][CHW].  D1 and D2 are read from slots (row + 2) % 3 and (row + 1) % 3; the three slots are derived
 *   in the kernel from the row number, so one captured launch serves every row.  A weight that is exactly 0 means its slot is NOT
 *   read: rows 0 and 1 of a run and the rows whose order is lowered never touch history that was never written.
 * DXMI_DPM_FIRST writes t_out[n] = K[T] only (the first evaluation's time); x, eps, hist, out may be NULL.
 * Control: ctl NULL: row, draw and seed are the by-value arguments, and row outside [0, rows) is DXMI_EINVAL.  ctl not NULL: an
 *   int32[4] block on the DEVICE = (row, draw, seed low word, seed high word) read by the kernel (the by-value three are ignored);
 *   a row outside [0, rows) read there gives NaN in x, out, t_out and slot 0 of the history; nothing outside the table and no
 *   history slot is read.
 * Noise: z (fp32 [N, CHW]) is given, or z == NULL and sample_index (int64 [N], DEVICE) is: the kernel then makes
 *   z[n][e] = the value dxmi_randn_indexed gives for (seed, sample_index[n], draw, e) (the same bits).  Both NULL: no noise is
 *   added.  Both given: DXMI_EINVAL.  A row with K[S] == 0 reads neither z nor the generator.
 * tab: fp32 [rows][DXMI_MT_COLS] on the device.  x, eps, z, hist, out, pred_xstart: 16-byte aligned; CHW % 4 != 0 takes 4-byte
 * aligned vector accesses and a scalar tail.  N in [1, 65535].  No workspace, no LDS, no atomics. */
#define DXMI_DPM_FIRST    0
#define DXMI_DPM_STEP     1
#define DXMI_MT_T         0   /* time of the evaluation the launch follows: (float)tau */
#define DXMI_MT_T_NEXT    1   /* time of the next evaluation (0 on the last row) */
#define DXMI_MT_CX        2   /* ODE sigma_p / sigma_t; SDE (sigma_p / sigma_t) exp(-h); 0 on the last row */
#define DXMI_MT_W0        3   /* weight of D_k (1 on the last row) */
#define DXMI_MT_W1        4   /* weight of D_{k-1}; exactly 0: the slot is not read */
#define DXMI_MT_W2        5   /* weight of D_{k-2}; exactly 0: the slot is not read */
#define DXMI_MT_S         6   /* noise scale: SDE sigma_p sqrt(1 - exp(-2h)); 0 for the ODE and on the last row */
#define DXMI_MT_A         7   /* 1 / alpha_t */
#define DXMI_MT_B         8   /* sigma_t / alpha_t */
#define DXMI_MT_FLAGS     9   /* DXMI_MT_FLAG_* summed, stored as a float */
#define DXMI_MT_ORDER    10   /* the order the row was built with (1-3); not read by the kernel */
#define DXMI_MT_COLS     16
#define DXMI_MT_FLAG_CLIP 1
#define DXMI_MT_FLAG_LAST 2
int dxmi_dpm_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw, uint64_t seed,
                   float* x, const float* eps, const float* z, const int64_t* sample_index, float* hist, float* t_out, float* out,
                   float* pred_xstart, int32_t N, int32_t CHW, void* stream);

/* DPM-Solver++ sampling of the EDM nets (csrc/edm_dpm_sample.hip; models/cm/dpm_sample.py): the multistep solver of
 * dxmi_dpm_stage in the EDM parametrisation x = x_0 + sigma e (alpha = 1, lambda = -ln sigma) on a sigma ladder, with the Karras
 * preconditioning inside the launch (the reference tree has no such sampler).  dxmi_edm_dpm_stage is the ONE launch between two
 * network evaluations.  With F = model_out the output of evaluation k = row at c_in(sigma_k) x and K = tab[row], per element in fp32,
 * one rounding per operation (no fused multiply-add), in this order:
 *     D0  = K[COUT] F + K[CSKIP] x;  FLAG_CLIP: D0 = clamp(D0, -1, 1)    (the data prediction; dxmi_karras_stage's order)
 *     acc = K[CX] x + K[W0] D0
 *     acc += K[W1] D1     if K[W1] != 0       (D1 = D_{k-1}, the data prediction of the evaluation before)
 *     acc += K[W2] D2     if K[W2] != 0       (D2 = D_{k-2})
 *     acc += K[S] z       if K[S] != 0
 * then x = acc in place, hist[row % 3] = D0, t_out[n] = K[T_NEXT] (the next evaluation's time 250 ln(sigma_{k+1} + 1e-44)),
 * on a row without FLAG_LAST x_in = K[CIN_NEXT] acc (the next evaluation's input; x_in is not touched on the last row) and, on the
 * row with FLAG_LAST, out = clamp(acc, -1, 1).  pred_xstart = D0 is written when not NULL.  A NaN in F reaches x' (the clamps pass
 * it); images do not mix.
 * History: hist is fp32 [3][N][CHW], addressed from the row number exactly as dxmi_dpm_stage addresses it; a weight that is exactly
 *   0 means its slot is NOT read.
 * DXMI_EDM_DPM_FIRST: x = x K[XSCALE] in place (x_T = randn sigma_max), x_in = K[CIN] x, t_out[n] = K[T]; model_out, hist and out
 *   may be NULL.
 * Control: ctl NULL: row, draw and seed are the by-value arguments, and row outside [0, rows) is DXMI_EINVAL.  ctl not NULL: an
 *   int32[4] block on the DEVICE = (row, draw, seed low word, seed high word) read by the kernel (the by-value three are ignored);
 *   a row outside [0, rows) read there gives NaN in x, x_in, out, t_out and slot 0 of the history; nothing outside the table and no
 *   history slot is read.
 * Noise: as dxmi_dpm_stage: z given, or z == NULL and sample_index (int64 [N], DEVICE): the bits of dxmi_randn_indexed for
 *   (seed, sample_index[n], draw, e).  Both NULL: no noise.  Both given: DXMI_EINVAL.  A row with K[S] == 0 reads neither.
 * x_in may be NULL only on the table's last row (rows - 1, the one the host flags last) given by value: with a control block the
 *   row is not known to the host, so x_in is required.
 * tab: fp32 [rows][DXMI_ET_COLS] on the device.  x, model_out, z, hist, x_in, out, pred_xstart: 16-byte aligned; CHW % 4 != 0
 * takes 4-byte aligned vector accesses and a scalar tail.  N in [1, 65535].  No workspace, no LDS, no atomics.
 * The table: columns 0-10 are those of DXMI_MT_* with the preconditioning's two scalars in the place of A and B. */
#define DXMI_EDM_DPM_FIRST 0
#define DXMI_EDM_DPM_STEP  1
#define DXMI_ET_T         0   /* time of the evaluation the launch follows: 250 ln(sigma_k + 1e-44) */
#define DXMI_ET_T_NEXT    1   /* time of the next evaluation (0 on the last row) */
#define DXMI_ET_CX        2   /* ODE sigma_p / sigma_t; SDE (sigma_p / sigma_t) exp(-h); 0 on the last row */
#define DXMI_ET_W0        3   /* weight of D_k (1 on the last row) */
#define DXMI_ET_W1        4   /* weight of D_{k-1}; exactly 0: the slot is not read */
#define DXMI_ET_W2        5   /* weight of D_{k-2}; exactly 0: the slot is not read */
#define DXMI_ET_S         6   /* noise scale: SDE sigma_p sqrt(1 - exp(-2h)); 0 for the ODE and on the last row */
#define DXMI_ET_CSKIP     7   /* c_skip(sigma_k) */
#define DXMI_ET_COUT      8   /* c_out(sigma_k) */
#define DXMI_ET_FLAGS     9   /* DXMI_ET_FLAG_* summed, stored as a float */
#define DXMI_ET_ORDER    10   /* the order the row was built with (1-3); not read by the kernel */
#define DXMI_ET_CIN      11   /* c_in(sigma_k): FIRST's factor of x_in */
#define DXMI_ET_CIN_NEXT 12   /* c_in(sigma_{k+1}) (0 on the last row, where x_in is not written) */
#define DXMI_ET_XSCALE   13   /* FIRST's factor of x: sigma_max */
#define DXMI_ET_SIGMA    14   /* sigma_k; not read by the kernel */
#define DXMI_ET_COLS     16
#define DXMI_ET_FLAG_CLIP 1
#define DXMI_ET_FLAG_LAST 2
int dxmi_edm_dpm_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw, uint64_t seed,
                       float* x, const float* model_out, const float* z, const int64_t* sample_index, float* hist, float* x_in,
                       float* t_out, float* out, float* pred_xstart, int32_t N, int32_t CHW, void* stream);

/* UniPC sampling of the DDPM teacher (csrc/unipc_sample.hip; models/DxMI/unipc_sample.py): Zhao, Bai, Rao, Zhou and Lu
 * 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models" (arXiv:2302.04867), the multistep
 * data-prediction predictor UniP with the corrector UniC at orders 1-3, ODE only (UniPC has no reference call site: the reference
 * tree has no such sampler).  dxmi_unipc_stage is the ONE launch between two network evaluations.  x is the predicted state the
 * network was evaluated on, xc the corrected state of the evaluation before.  With eps the output of evaluation k = row at x and
 * K = tab[row], per element in fp32, one rounding per operation (no fused multiply-add), in this order:
 *     D0  = K[A] x - K[B] eps;  FLAG_CLIP: D0 = clamp(D0, -1, 1)        (the data prediction)
 *     a row with FLAG_CORR, xc given (the corrector: the step that led here, re-done with D0 as a node at its end):
 *       b = K[CCX] xc;  b += K[CV0] D0;  b += K[CV1] D1;  b += K[CV2] D2 if K[CV2] != 0;  b += K[CV3] D3 if K[CV3] != 0
 *     otherwise b = x
 *     acc = K[CX] b + K[W0] D0;  acc += K[W1] D1 if K[W1] != 0;  acc += K[W2] D2 if K[W2] != 0      (the predictor)
 * then x = acc and xc = b in place (xc when given), hist[row % 4] = D0, t_out[n] = K[T_NEXT] and, on a row with FLAG_LAST,
 * out = clamp(acc, -1, 1).  pred_xstart = D0 is written when not NULL.  A NaN in eps reaches x' (the clamps pass it); images do not
 * mix.  The solver adds no noise: there is no z, no sample_index, no draw and no seed.
 * History: hist is fp32 [4][N][CHW].  D1, D2 and D3 are read from slots (row + 3) % 4, (row + 2) % 4 and (row + 1) % 4, derived in
 *   the kernel from the row number.  Slot j is read only if one of its two weights (K[Wj]; K[CVj] on a corrected row) is not 0.
 * xc: fp32 [N, CHW], read only on a row with FLAG_CORR, written on every row.  xc == NULL means "no corrected state": every row
 *   runs uncorrected, whatever its flags, and reads what its predictor alone reads.  xc == x is DXMI_EINVAL.
 * DXMI_UNIPC_FIRST writes t_out[n] = K[T] only (the first evaluation's time); x, xc, eps, hist, out may be NULL.
 * Control: ctl NULL: row is the by-value argument, and row outside [0, rows) is DXMI_EINVAL.  ctl not NULL: an int32[4] block on
 *   the DEVICE whose first word is the row (the layout of dxmi_dpm_stage's block; the other three words are not read); a row outside
 *   [0, rows) read there gives NaN in x, xc, out, t_out and slot 0 of the history; nothing outside the table, no history slot and
 *   no xc is read.
 * tab: fp32 [rows][DXMI_UT_COLS] on the device.  x, xc, eps, hist, out, pred_xstart: 16-byte aligned; CHW % 4 != 0 takes 4-byte
 * aligned vector accesses and a scalar tail.  N in [1, 65535].  No workspace, no LDS, no atomics.
 * The table: the columns of DXMI_MT_* (the solver has no noise: S's place holds the corrector's order) and the corrector's five. */
#define DXMI_UNIPC_FIRST   0
#define DXMI_UNIPC_STEP    1
#define DXMI_UT_T          0   /* time of the evaluation the launch follows: (float)tau */
#define DXMI_UT_T_NEXT     1   /* time of the next evaluation (0 on the last row) */
#define DXMI_UT_CX         2   /* sigma_{k+1} / sigma_k; 0 on the last row */
#define DXMI_UT_W0         3   /* predictor weight of D_k (1 on the last row) */
#define DXMI_UT_W1         4   /* predictor weight of D_{k-1} */
#define DXMI_UT_W2         5   /* predictor weight of D_{k-2} */
#define DXMI_UT_CORDER     6   /* the corrector's order q (0: the row is not corrected); not read by the kernel */
#define DXMI_UT_A          7   /* 1 / alpha_k */
#define DXMI_UT_B          8   /* sigma_k / alpha_k */
#define DXMI_UT_FLAGS      9   /* DXMI_UT_FLAG_* summed, stored as a float */
#define DXMI_UT_ORDER     10   /* the predictor's order p (1-3); not read by the kernel */
#define DXMI_UT_CCX       11   /* sigma_k / sigma_{k-1}: the corrector's factor of xc */
#define DXMI_UT_CV0       12   /* corrector weight of D_k */
#define DXMI_UT_CV1       13   /* corrector weight of D_{k-1} */
#define DXMI_UT_CV2       14   /* corrector weight of D_{k-2}; 0 below q = 2 */
#define DXMI_UT_CV3       15   /* corrector weight of D_{k-3}; 0 below q = 3 */
#define DXMI_UT_COLS      16
#define DXMI_UT_FLAG_CLIP  1
#define DXMI_UT_FLAG_LAST  2
#define DXMI_UT_FLAG_CORR  4
int dxmi_unipc_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, float* x, float* xc,
                     const float* eps, float* hist, float* t_out, float* out, float* pred_xstart, int32_t N, int32_t CHW,
                     void* stream);

/* UniPC sampling of the EDM nets (csrc/edm_unipc_sample.hip; models/cm/unipc_sample.py): dxmi_unipc_stage's solver in
 * the EDM parametrisation x = x_0 + sigma e (alpha = 1, lambda = -ln sigma) with the Karras preconditioning inside the launch, as
 * dxmi_edm_dpm_stage has it (UniPC has no reference call site: the reference tree has no such sampler).  With F = model_out the
 * output of evaluation k = row at c_in(sigma_k) x and K = tab[row]:
 *     D0  = K[COUT] F + K[CSKIP] x;  FLAG_CLIP: D0 = clamp(D0, -1, 1)
 *     b and acc as dxmi_unipc_stage forms them
 * then x = acc and xc = b in place, hist[row % 4] = D0, t_out[n] = K[T_NEXT], on a row without FLAG_LAST x_in = K[CIN_NEXT] acc and,
 * on the row with FLAG_LAST, out = clamp(acc, -1, 1).  History, xc and the control block as dxmi_unipc_stage (a poisoned row gives
 * NaN in x_in too); DXMI_EDM_UNIPC_FIRST and the x_in == NULL rule as dxmi_edm_dpm_stage.
 * tab: fp32 [rows][DXMI_EUT_COLS]: the columns of DXMI_ET_* (S's place holds the corrector's order) and the corrector's five. */
#define DXMI_EDM_UNIPC_FIRST 0
#define DXMI_EDM_UNIPC_STEP  1
#define DXMI_EUT_T         0   /* time of the evaluation the launch follows: 250 ln(sigma_k + 1e-44) */
#define DXMI_EUT_T_NEXT    1   /* time of the next evaluation (0 on the last row) */
#define DXMI_EUT_CX        2   /* sigma_{k+1} / sigma_k; 0 on the last row */
#define DXMI_EUT_W0        3   /* predictor weight of D_k (1 on the last row) */
#define DXMI_EUT_W1        4   /* predictor weight of D_{k-1} */
#define DXMI_EUT_W2        5   /* predictor weight of D_{k-2} */
#define DXMI_EUT_CORDER    6   /* the corrector's order q (0: the row is not corrected); not read by the kernel */
#define DXMI_EUT_CSKIP     7   /* c_skip(sigma_k) */
#define DXMI_EUT_COUT      8   /* c_out(sigma_k) */
#define DXMI_EUT_FLAGS     9   /* DXMI_EUT_FLAG_* summed, stored as a float */
#define DXMI_EUT_ORDER    10   /* the predictor's order p (1-3); not read by the kernel */
#define DXMI_EUT_CIN      11   /* c_in(sigma_k): FIRST's factor of x_in */
#define DXMI_EUT_CIN_NEXT 12   /* c_in(sigma_{k+1}) (0 on the last row, where x_in is not written) */
#define DXMI_EUT_XSCALE   13   /* FIRST's factor of x: sigma_max */
#define DXMI_EUT_SIGMA    14   /* sigma_k; not read by the kernel */
#define DXMI_EUT_CCX      15   /* sigma_k / sigma_{k-1}: the corrector's factor of xc */
#define DXMI_EUT_CV0      16   /* corrector weight of D_k */
#define DXMI_EUT_CV1      17   /* corrector weight of D_{k-1} */
#define DXMI_EUT_CV2      18   /* corrector weight of D_{k-2}; 0 below q = 2 */
#define DXMI_EUT_CV3      19   /* corrector weight of D_{k-3}; 0 below q = 3 */
#define DXMI_EUT_COLS     20
#define DXMI_EUT_FLAG_CLIP 1
#define DXMI_EUT_FLAG_LAST 2
#define DXMI_EUT_FLAG_CORR 4
int dxmi_edm_unipc_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, float* x, float* xc,
                         const float* model_out, float* hist, float* x_in, float* t_out, float* out, float* pred_xstart, int32_t N,
                         int32_t CHW, void* stream);

/* Likelihood (bits/dim) of the EDM nets and the DDPM teacher by the probability-flow ODE (csrc/pf_likelihood.hip;
 * models/cm/likelihood.py, models/DxMI/likelihood.py; the reference tree computes no likelihood, so there is no reference call
 * site).  In the EDM variable dx/dsigma = k = (x - D(x; sigma)) / sigma, d log p / dsigma = -div k; Heun on (x, l) over the nodes
 * sigma_0 < ... < sigma_S.  Each evaluation is a forward F = net(x_in, time) and the input-only backward g = d(e . F)/d(x_in) at the
 * probe e (input_vjp); dxmi_pf_ll_stage is the ONE launch after it.  Row i of the table describes the step sigma_i -> sigma_{i+1}.
 * With K = tab[row], per element in fp32, one rounding per operation (no fused multiply-add), in this order:
 *   DXMI_PF_LL_FIRST    x = x K[XSCALE] in place, x_in = K[CIN] x, t_out[n] = K[T], ell[n] = K[LOGDET0]
 *   DXMI_PF_LL_PREDICT  (after the evaluation at (x_i, sigma_i); x is read only)
 *       k1 = K[KA] x + K[KB] F;  xt = x + K[H] k1;  x_in = K[CIN_NEXT] xt;  t_out[n] = K[T_NEXT]
 *       div1[n] = sum_i ( K[KA] (e_i e_i) + K[DB] (e_i g_i) )              k1 is written to its buffer, xt when not NULL
 *   DXMI_PF_LL_CORRECT  (after the evaluation at (xt, sigma_{i+1}))
 *       xt = x + K[H] k1 (the bits PREDICT formed);  k2 = K[KA2] xt + K[KB2] F;  x = x + K[HH] (k1 + k2) in place
 *       x_in = K[CIN_NEXT] x (not on the row flagged last);  t_out[n] = K[T_NEXT]
 *       div2 = sum_i ( K[KA2] (e_i e_i) + K[DB2] (e_i g_i) );  ell[n] = ell[n] + K[HH] (div1[n] + div2)
 *       on the row with FLAG_LAST: prior[n] = K[PRIOR_Q] sum_i x_i^2 + K[PRIOR_C], logp[n] = ell[n] + prior[n],
 *       bpd[n] = logp[n] K[BPD_SCALE] + 7
 * Sums: one workgroup per image; a lane's running sum in index order, the xor-shuffle tree of a wave, a fixed pairing of the four
 *   wave partials: bitwise equal run to run, and an image's result does not depend on the batch it rides in.
 * Probe: eps given (any fp32 tensor: Gaussian probes, tests), or eps == NULL and sample_index (int64 [N], DEVICE): Rademacher signs
 *   made here, e = +1 where the normal dxmi_randn_indexed gives for (seed, sample_index[n], draw, element) is >= 0, else -1.  Exactly
 *   one of the two (PREDICT, CORRECT); PREDICT and CORRECT of a trajectory pass the same draw.
 * Control: as dxmi_edm_dpm_stage: ctl NULL: row, draw and seed by value, a row outside [0, rows) is DXMI_EINVAL; ctl an int32[4]
 *   DEVICE block (row, draw, seed low, seed high): a row outside [0, rows) read there gives NaN in every output of the mode (CORRECT:
 *   prior, logp and bpd too); nothing outside the table is read.
 * x_in may be NULL only in CORRECT on the table's last row given by value.  x, k1, xt and x_in are distinct tensors.
 * tab: fp32 [rows][DXMI_PL_COLS] on the device, every entry formed in float64 on the host and rounded once.  x, model_out, vjp, eps,
 * k1, xt, x_in: 16-byte aligned; CHW % 4 != 0 takes 4-byte aligned vector accesses and a scalar tail.  N in [1, 65535], CHW < 2^30.
 * t_out, div1, ell, prior, logp, bpd: fp32 [N].  No workspace, no atomics. */
#define DXMI_PF_LL_FIRST   0
#define DXMI_PF_LL_PREDICT 1
#define DXMI_PF_LL_CORRECT 2
#define DXMI_PL_T          0   /* time of the evaluation at sigma_i (EDM: 250 ln(sigma_i + 1e-44); DDPM: the integer step) */
#define DXMI_PL_T_NEXT     1   /* time of the evaluation at sigma_{i+1} */
#define DXMI_PL_CIN        2   /* c_in(sigma_i): FIRST's factor of x_in */
#define DXMI_PL_CIN_NEXT   3   /* c_in(sigma_{i+1}) */
#define DXMI_PL_XSCALE     4   /* FIRST's factor of x (EDM 1; DDPM 1 / sqrt(alpha_bar of the first step)) */
#define DXMI_PL_LOGDET0    5   /* FIRST's ell (EDM 0; DDPM -(d / 2) ln alpha_bar of the first step) */
#define DXMI_PL_KA         6   /* (1 - c_skip(sigma_i)) / sigma_i: weight of x in k1 and of e e in div1 */
#define DXMI_PL_KB         7   /* -c_out(sigma_i) / sigma_i: weight of F in k1 */
#define DXMI_PL_DB         8   /* -c_out(sigma_i) c_in(sigma_i) / sigma_i: weight of e g in div1 */
#define DXMI_PL_KA2        9   /* the same three at sigma_{i+1} */
#define DXMI_PL_KB2       10
#define DXMI_PL_DB2       11
#define DXMI_PL_H         12   /* sigma_{i+1} - sigma_i */
#define DXMI_PL_HH        13   /* (sigma_{i+1} - sigma_i) / 2 */
#define DXMI_PL_FLAGS     14   /* DXMI_PL_FLAG_* summed, stored as a float */
#define DXMI_PL_PRIOR_Q   15   /* -1 / (2 prior_var) */
#define DXMI_PL_PRIOR_C   16   /* -(d / 2) ln(2 pi prior_var) */
#define DXMI_PL_BPD_SCALE 17   /* -1 / (d ln 2) */
#define DXMI_PL_SIGMA     18   /* sigma_i; not read by the kernel */
#define DXMI_PL_SIGMA_NEXT 19  /* sigma_{i+1}; not read by the kernel */
#define DXMI_PL_COLS      20
#define DXMI_PL_FLAG_LAST  2
int dxmi_pf_ll_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw, uint64_t seed,
                     float* x, const float* model_out, const float* vjp, const float* eps, const int64_t* sample_index, float* k1,
                     float* xt, float* x_in, float* t_out, float* div1, float* ell, float* prior, float* logp, float* bpd, int32_t N,
                     int32_t CHW, void* stream);

/* ---- DMD2's GAN term (csrc/gan_head.hip) -----------------------------------------------------------------------------------------
 * Yin et al. 2024, "Improved Distribution Matching Distillation for Fast Image Synthesis" (DMD2), section 4.3: a classifier on the
 * fake denoiser's bottleneck features, trained with the fake denoiser to tell noised real images from noised generated ones, which
 * gives the generator one more gradient.  The head (models/cm/gan_head.py) is
 *   Conv2d(C, C, 4, stride 2, pad 1) - GroupNorm - SiLU - Conv2d(C, C, map/2, stride map/2) - GroupNorm - SiLU - Conv2d(C, 1, 1);
 * its whole-map conv runs on dxmi_linear_* and its GroupNorms on dxmi_groupnorm_generic_*; the entry points here are the rest.
 * Activations are NHWC bf16, bf16 MFMA operands with fp32 accumulation.  Every launch is bitwise reproducible: the split
 * contractions write fp32 slabs into the caller's workspace and a second launch sums them in slice order (no float atomics).
 * DXMI_EINVAL with a message and no launch: a null pointer (but the optional ones), N outside [1, 4096], H not 4 or 8, a C that
 * dxmi_gan_head_supported refuses, a workspace smaller than dxmi_gan_conv4s2_workspace_bytes, an activation, pack, gradient or
 * workspace that is not 16-byte aligned (the fp32 parameters w, bias and b may sit at any 4-byte offset: a trainer keeps them as
 * views into one flat tensor).
 *
 * dxmi_gan_head_supported: DXMI_OK where the kernels serve C channels on a map_size x map_size bottleneck (C a multiple of 64 in
 *   [64, 1024]: 128, 192, 256, 768 and 1024 among them; map_size 4 or 8), else DXMI_EINVAL and a message that names the value.
 * dxmi_gan_conv4s2_slices(dgrad): the number of fp32 slabs summed per output element (16 filter taps forward, 4 for the data
 *   gradient): the depth the error bound of a result adds to its contraction length.
 * dxmi_gan_conv4s2_workspace_bytes(N, H, C, dgrad): bytes of the slab workspace (0: unsupported shape).
 * dxmi_gan_conv4s2_pack: w fp32 OIHW [C, C, 4, 4] -> w_fwd bf16 [16][Cout][Cin] and w_t bf16 [16][Cin][Cout] (32 C^2 bytes each).
 * dxmi_gan_conv4s2_fwd: x [N, H, H, C] -> y [N, H/2, H/2, C] = conv(x, w, stride 2, pad 1) + bias (bias NULL: none).  Rows
 *   outside the map contribute zero.
 * dxmi_gan_conv4s2_dgrad: dy [N, H/2, H/2, C] -> dx [N, H, H, C], the transposed conv on w_t.
 * dxmi_gan_conv4s2_wgrad: dw fp32 OIHW [C, C, 4, 4] and db [C] from x and dy (no workspace: the contraction over the rows is
 *   not split).
 * dxmi_gan_logit_loss_fwd: a bf16 [N, C], w [C], b [1], sign [N] (-1 or +1) -> logit[n] = w . a[n] + b and
 *   loss[n] = softplus(sign[n] logit[n]) in the form max(v, 0) + log1p(exp(-|v|)).
 * dxmi_gan_logit_loss_bwd: with coef[n] = upstream[n] weight sign[n] sigmoid(sign[n] logit[n]):  d_a[n] = coef[n] w (bf16),
 *   dw = sum_n coef[n] a[n] and db = sum_n coef[n], summed in sample order.  dw and db NULL: not wanted (the input-only backward).
 * dxmi_gan_join: out = g + (CHW weight c_in(t)) d_xin, t = t_table[indices[n]], c_in = 1 / sqrt(t^2 + sigma_data^2): the DM
 *   direction g of dxmi_dm_grad_fwd joined with the GAN term's gradient d_xin with respect to the fake denoiser's input, so that
 *   dxmi_dm_gen_bwd's g / CHW carries both.  out may be g itself; N, CHW and the table as in dxmi_dm_grad_fwd. */
int dxmi_gan_head_supported(int32_t C, int32_t map_size);
int64_t dxmi_gan_conv4s2_slices(int32_t dgrad);
int64_t dxmi_gan_conv4s2_workspace_bytes(int32_t N, int32_t H, int32_t C, int32_t dgrad);
int dxmi_gan_conv4s2_pack(const float* w, void* w_fwd, void* w_t, int32_t C, void* stream);
int dxmi_gan_conv4s2_fwd(const void* x, const void* w_fwd, const float* bias, void* y, void* workspace, int64_t workspace_bytes,
                         int32_t N, int32_t H, int32_t C, void* stream);
int dxmi_gan_conv4s2_dgrad(const void* dy, const void* w_t, void* dx, void* workspace, int64_t workspace_bytes, int32_t N, int32_t H,
                           int32_t C, void* stream);
int dxmi_gan_conv4s2_wgrad(const void* x, const void* dy, float* dw, float* db, int32_t N, int32_t H, int32_t C, void* stream);
int dxmi_gan_logit_loss_fwd(const void* a, const float* w, const float* b, const float* sign, float* logit, float* loss, int32_t N,
                            int32_t C, void* stream);
int dxmi_gan_logit_loss_bwd(const void* a, const float* w, const float* sign, const float* logit, const float* upstream, float weight,
                            void* d_a, float* dw, float* db, int32_t N, int32_t C, void* stream);
int dxmi_gan_join(const float* g, const float* d_xin, const int64_t* indices, const float* t_table, int32_t num_scales, float* out,
                  int32_t N, int32_t CHW, float weight, float sigma_data, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DXMI_HIP_H */
