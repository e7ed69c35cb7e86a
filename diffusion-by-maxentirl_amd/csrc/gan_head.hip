// DMD2's GAN term (Yin et al. 2024, "Improved Distribution Matching Distillation for Fast Image Synthesis", section 4.3 and its
// ImageNet-64 classifier head): a small classifier on the fake denoiser's bottleneck features,
//   Conv2d(C, C, 4, stride 2, pad 1) - GroupNorm - SiLU - Conv2d(C, C, map/2, stride map/2) - GroupNorm - SiLU - Conv2d(C, 1, 1).
// The launches that models/cm/gan_head.py has no existing kernel for:
//   dxmi_gan_conv4s2_pack    fp32 OIHW [C, C, 4, 4] -> bf16 [16 taps][Cout][Cin] and its transpose [16 taps][Cin][Cout]
//   dxmi_gan_conv4s2_fwd     NHWC bf16 [N, H, H, C] -> [N, H/2, H/2, C], implicit GEMM straight from the map
//   dxmi_gan_conv4s2_dgrad   its data gradient  [N, H/2, H/2, C] -> [N, H, H, C]
//   dxmi_gan_conv4s2_wgrad   its weight gradient (fp32 OIHW) and bias gradient
//   dxmi_gan_logit_loss_fwd  logit_n = w . a_n + b and softplus(sign_n logit_n), one launch
//   dxmi_gan_logit_loss_bwd  the cotangent of a, d w and d b
//   dxmi_gan_join            g_total = g + (CHW weight c_in(t)) d_xin: the generator's combined direction
// (the whole-map conv is a dense layer and runs on dxmi_linear_*; the two GroupNorms on dxmi_groupnorm_generic_*).
//
// The first conv is skinny and weight-bound: N (H/2)^2 output rows (256 at N = 16, H = 8) against K = 16 C and 32 C^2 bytes of
// weights (18.9 MB at C = 768).  Cout tiles x row tiles alone are 6 x 8 workgroups at that shape, so the contraction is split
// over the filter taps: tap (kh, kw) of the forward is a [rows, C] x [C, C] product on a shifted view of the map, one grid slice
// each (16); the data gradient has 4 taps per input pixel, by the pixel's parity (rows are tiled per parity class), one grid
// slice each (4).  Every slice writes an fp32 slab of the workspace with plain stores and a second launch sums the slabs in slice
// order, adds the bias and rounds to bf16 once: no atomics, the same bits at every run.  The weight gradient contracts over the
// rows and has C^2 / 1024 x 4 independent tiles: no split.  Rows outside the map contribute zero (never read).
// MFMA 32x32x16 bf16, fp32 accumulation; both operands come from global memory in 64-byte runs per lane (the k order inside a
// 64-channel step is the same permutation for both operands, which a contraction does not see).
#include "dsm_common.h"
#include "ew_common.h"

namespace {

constexpr int GAN_TAPS = 16;
constexpr int GAN_DGRAD_SLICES = 4;

__device__ __forceinline__ bf16x8 ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

__global__ __launch_bounds__(256) void gan_pack_kernel(const float* __restrict__ w, bf16* __restrict__ wf, bf16* __restrict__ wt, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
    if (i >= C) return;
    const float* src = w + ((size_t)o * C + i) * GAN_TAPS;
    float v[GAN_TAPS];      // (a parameter may be a view into a trainer's flat master at any 4-byte offset: no 16-byte loads)
#pragma unroll
    for (int tap = 0; tap < GAN_TAPS; ++tap) v[tap] = src[tap];
#pragma unroll
    for (int tap = 0; tap < GAN_TAPS; ++tap) {
        const bf16 b = (bf16)v[tap];
        wf[((size_t)tap * C + o) * C + i] = b;
        wt[((size_t)tap * C + i) * C + o] = b;
    }
}

// One row of a 32-row tile: where its operand row starts (ok false: the tap falls outside the map, or the row is past the end),
// which tap's weights it meets and which row of the slab it writes (-1: past the end).
struct GanRow {
    size_t off;
    bool ok;
    int tap, out_row;
};

// DGRAD = 0: rows are output pixels (n, oh, ow), slice z = tap.  DGRAD = 1: rows are the input pixels of one parity class
// cls = (ih & 1) * 2 + (iw & 1), (n, ih / 2, iw / 2) in that order; slice z = (a, b) names tap kh = 1 - (ih & 1) + 2 a,
// kw = 1 - (iw & 1) + 2 b, the output pixel is oh = (ih + 1 - kh) / 2 (exact), and the tap is uniform over the tile.
template <int DGRAD>
__device__ __forceinline__ GanRow gan_row(int m, int Mc, int cls, int z, int H, int lgO, int C) {
    GanRow r;
    const int OH = 1 << lgO;
    const int n = m >> (2 * lgO), i = (m >> lgO) & (OH - 1), j = m & (OH - 1);
    if (!DGRAD) {
        const int kh = z >> 2, kw = z & 3;
        const int ih = 2 * i - 1 + kh, iw = 2 * j - 1 + kw;
        r.tap = z;
        r.out_row = m < Mc ? m : -1;
        r.ok = m < Mc && ih >= 0 && ih < H && iw >= 0 && iw < H;
        r.off = r.ok ? ((size_t)(n * H + ih) * H + iw) * C : 0;
    } else {
        const int pih = cls >> 1, piw = cls & 1;
        const int ih = 2 * i + pih, iw = 2 * j + piw;
        const int kh = 1 - pih + 2 * (z >> 1), kw = 1 - piw + 2 * (z & 1);
        const int th = ih + 1 - kh, tw = iw + 1 - kw;          // even; -2 at the top / left border
        r.tap = kh * 4 + kw;
        r.out_row = m < Mc ? (n * H + ih) * H + iw : -1;
        r.ok = m < Mc && th >= 0 && (th >> 1) < OH && tw >= 0 && (tw >> 1) < OH;
        r.off = r.ok ? ((size_t)(n * OH + (th >> 1)) * OH + (tw >> 1)) * C : 0;
    }
    return r;
}

// grid (row tiles [x 4 parity classes], ceil(C / 128), slices); a wave owns 32 rows x 32 output channels.  w: [16][out][in].
template <int DGRAD>
__global__ __launch_bounds__(256) void gan_gemm_kernel(const bf16* __restrict__ src, const bf16* __restrict__ w, float* __restrict__ part,
                                                       int Mc, int tiles, int rows_out, int H, int lgO, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cb = blockIdx.y * 4 + wave;
    if (cb * 32 >= C) return;                     // (no barrier below)
    const int r = lane & 31, half = lane >> 5;
    const int cls = DGRAD ? blockIdx.x / tiles : 0;
    const int m0 = (DGRAD ? blockIdx.x % tiles : blockIdx.x) * 32;
    const int z = blockIdx.z;
    const GanRow row = gan_row<DGRAD>(m0 + r, Mc, cls, z, H, lgO, C);
    const bf16* ap = src + row.off + half * 32;
    const bf16* bp = w + ((size_t)row.tap * C + cb * 32 + r) * C + half * 32;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < C; k0 += 64) {
        bf16x8 a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            b[q] = ld8(bp + k0 + q * 8);
            if (row.ok) a[q] = ld8(ap + k0 + q * 8);
            else
#pragma unroll
                for (int e = 0; e < 8; ++e) a[q][e] = (bf16)0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q], b[q], acc, 0, 0, 0);
    }
    // acc[i]: row (i / 4) * 8 + half * 4 + i % 4 of the tile, column r
    float* slab = part + (size_t)z * rows_out * C + cb * 32 + r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = m0 + (i >> 2) * 8 + half * 4 + (i & 3);
        const GanRow o = gan_row<DGRAD>(m, Mc, cls, z, H, lgO, C);
        if (o.out_row >= 0) slab[(size_t)o.out_row * C] = acc[i];
    }
}

// out = bf16((slab 0 + slab 1 + ... in slice order) + bias): 4 channels per lane
__global__ __launch_bounds__(256) void gan_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias, bf16* __restrict__ out,
                                                         int S, int rows, int C) {
    const size_t total4 = (size_t)rows * C / 4;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    f32x4 s = *reinterpret_cast<const f32x4*>(part + i * 4);
    for (int z = 1; z < S; ++z) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(part + (size_t)z * rows * C + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += v[e];
    }
    if (bias) {
        const int c0 = (int)((i * 4) % C);      // (scalar loads: the bias may sit at any 4-byte offset of a flat master)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += bias[c0 + e];
    }
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (bf16)s[e];
    *reinterpret_cast<bf16x4*>(out + i * 4) = o;
}

// dW[co][ci][kh][kw] = sum over the output pixels m of dy[m][co] x[pixel(m) + tap][ci].  grid (C / 32 ci tiles, ceil(C / 128), 4 kh);
// a wave owns 32 co x 32 ci x the four kw of its kh, the contraction runs over the rows in steps of 16.  The contraction index is the
// row, so an operand's 8 k-values are 8 rows of one channel: scalar 2-byte loads at stride C, 40 per lane for 4 MFMAs (coalesced across
// the 32 lanes of a row).  This is the slowest launch of the head (132 us at C = 768, N = 16); a transposing LDS stage is not built.
__global__ __launch_bounds__(256) void gan_wgrad_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy, float* __restrict__ dw, int M,
                                                        int H, int lgO, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cb = blockIdx.y * 4 + wave;
    if (cb * 32 >= C) return;
    const int r = lane & 31, half = lane >> 5;
    const int OH = 1 << lgO, kh = blockIdx.z;
    const int co = cb * 32 + r, ci = blockIdx.x * 32 + r;
    f32x16 acc[4];
#pragma unroll
    for (int kw = 0; kw < 4; ++kw)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[kw][i] = 0.f;
    for (int m0 = 0; m0 < M; m0 += 16) {
        bf16x8 a, b[4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int m = m0 + half * 8 + e;
            const bool in = m < M;
            a[e] = in ? dy[(size_t)m * C + co] : (bf16)0.f;
            const int n = m >> (2 * lgO), oh = (m >> lgO) & (OH - 1), ow = m & (OH - 1);
            const int ih = 2 * oh - 1 + kh;
            const bool rowok = in && ih >= 0 && ih < H;
#pragma unroll
            for (int kw = 0; kw < 4; ++kw) {
                const int iw = 2 * ow - 1 + kw;
                b[kw][e] = (rowok && iw >= 0 && iw < H) ? x[((size_t)(n * H + ih) * H + iw) * C + ci] : (bf16)0.f;
            }
        }
#pragma unroll
        for (int kw = 0; kw < 4; ++kw) acc[kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[kw], acc[kw], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int o = cb * 32 + (i >> 2) * 8 + half * 4 + (i & 3);
        f32x4 v;
#pragma unroll
        for (int kw = 0; kw < 4; ++kw) v[kw] = acc[kw][i];
        *reinterpret_cast<f32x4*>(dw + ((size_t)o * C + ci) * GAN_TAPS + kh * 4) = v;
    }
}

// db[c] = sum over the rows, in row order
__global__ __launch_bounds__(256) void gan_colsum_kernel(const bf16* __restrict__ dy, float* __restrict__ db, int M, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += (float)dy[(size_t)m * C + c];
    db[c] = s;
}

__device__ __forceinline__ float gan_softplus(float v) { return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))); }
// d softplus(v) / dv = sigmoid(v), in the form that does not overflow
__device__ __forceinline__ float gan_sigmoid(float v) {
    const float e = expf(-fabsf(v));
    return v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// one workgroup per sample
__global__ __launch_bounds__(EW_BLOCK) void gan_logit_loss_fwd_kernel(const bf16* __restrict__ a, const float* __restrict__ w,
                                                                       const float* __restrict__ b, const float* __restrict__ sign,
                                                                       float* __restrict__ logit, float* __restrict__ loss, int C) {
    __shared__ float red[EW_BLOCK / 64];
    const int n = blockIdx.x;
    float acc = 0.f;
    for (int c = threadIdx.x; c < C; c += EW_BLOCK) acc += w[c] * (float)a[(size_t)n * C + c];
    const float l = block_sum(acc, red) + b[0];
    if (threadIdx.x == 0) {
        logit[n] = l;
        loss[n] = gan_softplus(sign[n] * l);
    }
}

// a lane per channel: coef_n = upstream_n weight sign_n sigmoid(sign_n logit_n); d a[n][c] = coef_n w[c]; d w[c] = sum_n coef_n a[n][c]
// in sample order; d b = sum_n coef_n.
__global__ __launch_bounds__(EW_BLOCK) void gan_logit_loss_bwd_kernel(const bf16* __restrict__ a, const float* __restrict__ w,
                                                                       const float* __restrict__ sign, const float* __restrict__ logit,
                                                                       const float* __restrict__ up, float weight, bf16* __restrict__ d_a,
                                                                       float* __restrict__ dw, float* __restrict__ db, int N, int C) {
    const int c = blockIdx.x * EW_BLOCK + threadIdx.x;
    if (c >= C) return;
    const float wc = w[c];
    float sw = 0.f, sb = 0.f;
    for (int n = 0; n < N; ++n) {
        const float coef = ((up[n] * weight) * sign[n]) * gan_sigmoid(sign[n] * logit[n]);
        d_a[(size_t)n * C + c] = (bf16)(coef * wc);
        sw += coef * (float)a[(size_t)n * C + c];
        sb += coef;
    }
    if (dw) dw[c] = sw;
    if (db && c == 0) db[0] = sb;
}

__global__ __launch_bounds__(EW_BLOCK) void gan_join_kernel(const float* __restrict__ g, const float* __restrict__ d, const int64_t* __restrict__ idx,
                                                            const float* __restrict__ tab, int S, float* __restrict__ out, int CHW, float cw,
                                                            float sd2) {
    const int b = blockIdx.y;
    const float s = cw * dsm_c_in(ew_level(idx, tab, S, b), sd2);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 gv[EW_UNROLL], dv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u)
            if (i0 + u * EW_BLOCK < n4) {
                gv[u] = ld4(g, base, i0 + u * EW_BLOCK);
                dv[u] = ld4(d, base, i0 + u * EW_BLOCK);
            }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = gv[u][e] + s * dv[u][e];
            st4(out, base, i, o);
        }
    }
}

int gan_lg(int H) { return H == 8 ? 2 : 1; }          // log2(H / 2)

}  // namespace

#define GAN_CHECK_SHAPE(fn)                                                                                                          \
    do {                                                                                                                             \
        DXMI_CHECK_ARG(N > 0 && N <= 4096, fn ": N (%d) must be in [1, 4096]", N);                                                   \
        DXMI_CHECK_ARG(H == 4 || H == 8, fn ": H (%d) must be 4 or 8", H);                                                           \
        DXMI_CHECK_ARG(dxmi_gan_head_supported(C, H) == DXMI_OK, fn ": C (%d) must be a multiple of 64 in [64, 1024]", C);           \
    } while (0)

extern "C" int dxmi_gan_head_supported(int32_t C, int32_t map_size) {
    DXMI_CHECK_ARG(map_size == 4 || map_size == 8, "dxmi_gan_head_supported: map size (%d) must be 4 or 8", map_size);
    DXMI_CHECK_ARG(C >= 64 && C <= 1024 && C % 64 == 0, "dxmi_gan_head_supported: C (%d) must be a multiple of 64 in [64, 1024]", C);
    return DXMI_OK;
}

extern "C" int64_t dxmi_gan_conv4s2_slices(int32_t dgrad) { return dgrad ? GAN_DGRAD_SLICES : GAN_TAPS; }

extern "C" int64_t dxmi_gan_conv4s2_workspace_bytes(int32_t N, int32_t H, int32_t C, int32_t dgrad) {
    if (N <= 0 || N > 4096 || (H != 4 && H != 8) || dxmi_gan_head_supported(C, H) != DXMI_OK) return 0;
    const int64_t rows = dgrad ? (int64_t)N * H * H : (int64_t)N * (H / 2) * (H / 2);
    return (dgrad ? GAN_DGRAD_SLICES : GAN_TAPS) * rows * C * 4;
}

extern "C" int dxmi_gan_conv4s2_pack(const float* w, void* w_fwd, void* w_t, int32_t C, void* stream) {
    DXMI_CHECK_ARG(w && w_fwd && w_t, "dxmi_gan_conv4s2_pack: null pointer");
    DXMI_CHECK_ARG(dxmi_gan_head_supported(C, 8) == DXMI_OK, "dxmi_gan_conv4s2_pack: C (%d) must be a multiple of 64 in [64, 1024]", C);
    DXMI_CHECK_ARG(ew_aligned((const char*)w_fwd, (const char*)w_t), "dxmi_gan_conv4s2_pack: packs must be 16-byte aligned");
    hipLaunchKernelGGL(gan_pack_kernel, dim3((C + 255) / 256, C), dim3(256), 0, (hipStream_t)stream, w, (bf16*)w_fwd, (bf16*)w_t, C);
    DXMI_CHECK_LAUNCH("dxmi_gan_conv4s2_pack");
    return DXMI_OK;
}

extern "C" int dxmi_gan_conv4s2_fwd(const void* x, const void* w_fwd, const float* bias, void* y, void* workspace, int64_t workspace_bytes,
                                    int32_t N, int32_t H, int32_t C, void* stream) {
    DXMI_CHECK_ARG(x && w_fwd && y && workspace, "dxmi_gan_conv4s2_fwd: null pointer");
    GAN_CHECK_SHAPE("dxmi_gan_conv4s2_fwd");
    DXMI_CHECK_ARG(workspace_bytes >= dxmi_gan_conv4s2_workspace_bytes(N, H, C, 0), "dxmi_gan_conv4s2_fwd: workspace of %lld bytes, %lld needed",
                   (long long)workspace_bytes, (long long)dxmi_gan_conv4s2_workspace_bytes(N, H, C, 0));
    DXMI_CHECK_ARG(ew_aligned((const char*)x, (const char*)w_fwd, (const char*)y, (const char*)workspace),
                   "dxmi_gan_conv4s2_fwd: tensors must be 16-byte aligned");
    const int lgO = gan_lg(H), M = N << (2 * lgO), tiles = (M + 31) / 32;
    hipLaunchKernelGGL(gan_gemm_kernel<0>, dim3(tiles, (C / 32 + 3) / 4, GAN_TAPS), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                       (const bf16*)w_fwd, (float*)workspace, M, tiles, M, H, lgO, C);
    DXMI_CHECK_LAUNCH("dxmi_gan_conv4s2_fwd");
    hipLaunchKernelGGL(gan_reduce_kernel, dim3((M * (C / 4) + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, bias,
                       (bf16*)y, GAN_TAPS, M, C);
    DXMI_CHECK_LAUNCH("dxmi_gan_conv4s2_fwd(reduce)");
    return DXMI_OK;
}

extern "C" int dxmi_gan_conv4s2_dgrad(const void* dy, const void* w_t, void* dx, void* workspace, int64_t workspace_bytes, int32_t N,
                                      int32_t H, int32_t C, void* stream) {
    DXMI_CHECK_ARG(dy && w_t && dx && workspace, "dxmi_gan_conv4s2_dgrad: null pointer");
    GAN_CHECK_SHAPE("dxmi_gan_conv4s2_dgrad");
    DXMI_CHECK_ARG(workspace_bytes >= dxmi_gan_conv4s2_workspace_bytes(N, H, C, 1), "dxmi_gan_conv4s2_dgrad: workspace of %lld bytes, %lld needed",
                   (long long)workspace_bytes, (long long)dxmi_gan_conv4s2_workspace_bytes(N, H, C, 1));
    DXMI_CHECK_ARG(ew_aligned((const char*)dy, (const char*)w_t, (const char*)dx, (const char*)workspace),
                   "dxmi_gan_conv4s2_dgrad: tensors must be 16-byte aligned");
    const int lgO = gan_lg(H), Mc = N << (2 * lgO), tiles = (Mc + 31) / 32, rows = N * H * H;
    hipLaunchKernelGGL(gan_gemm_kernel<1>, dim3(tiles * 4, (C / 32 + 3) / 4, GAN_DGRAD_SLICES), dim3(256), 0, (hipStream_t)stream,
                       (const bf16*)dy, (const bf16*)w_t, (float*)workspace, Mc, tiles, rows, H, lgO, C);
    DXMI_CHECK_LAUNCH("dxmi_gan_conv4s2_dgrad");
    hipLaunchKernelGGL(gan_reduce_kernel, dim3((rows * (C / 4) + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)workspace,
                       (const float*)nullptr, (bf16*)dx, GAN_DGRAD_SLICES, rows, C);
    DXMI_CHECK_LAUNCH("dxmi_gan_conv4s2_dgrad(reduce)");
    return DXMI_OK;
}

extern "C" int dxmi_gan_conv4s2_wgrad(const void* x, const void* dy, float* dw, float* db, int32_t N, int32_t H, int32_t C, void* stream) {
    DXMI_CHECK_ARG(x && dy && dw && db, "dxmi_gan_conv4s2_wgrad: null pointer");
    GAN_CHECK_SHAPE("dxmi_gan_conv4s2_wgrad");
    DXMI_CHECK_ARG(ew_aligned((const char*)x, (const char*)dy, dw, db), "dxmi_gan_conv4s2_wgrad: tensors must be 16-byte aligned");
    const int lgO = gan_lg(H), M = N << (2 * lgO);
    hipLaunchKernelGGL(gan_wgrad_kernel, dim3(C / 32, (C / 32 + 3) / 4, 4), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)dy,
                       dw, M, H, lgO, C);
    DXMI_CHECK_LAUNCH("dxmi_gan_conv4s2_wgrad");
    hipLaunchKernelGGL(gan_colsum_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const bf16*)dy, db, M, C);
    DXMI_CHECK_LAUNCH("dxmi_gan_conv4s2_wgrad(bias)");
    return DXMI_OK;
}

#define GAN_CHECK_NC(fn)                                                                                                            \
    DXMI_CHECK_ARG(N > 0 && N <= 65535 && C > 0 && C <= 4096 && C % 8 == 0, fn ": N (%d) must be in [1, 65535] and C (%d) a "       \
                   "multiple of 8 in [8, 4096]", N, C)

extern "C" int dxmi_gan_logit_loss_fwd(const void* a, const float* w, const float* b, const float* sign, float* logit, float* loss,
                                       int32_t N, int32_t C, void* stream) {
    DXMI_CHECK_ARG(a && w && b && sign && logit && loss, "dxmi_gan_logit_loss_fwd: null pointer");
    GAN_CHECK_NC("dxmi_gan_logit_loss_fwd");
    hipLaunchKernelGGL(gan_logit_loss_fwd_kernel, dim3(N), dim3(EW_BLOCK), 0, (hipStream_t)stream, (const bf16*)a, w, b, sign, logit, loss, C);
    DXMI_CHECK_LAUNCH("dxmi_gan_logit_loss_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_gan_logit_loss_bwd(const void* a, const float* w, const float* sign, const float* logit, const float* upstream,
                                       float weight, void* d_a, float* dw, float* db, int32_t N, int32_t C, void* stream) {
    DXMI_CHECK_ARG(a && w && sign && logit && upstream && d_a, "dxmi_gan_logit_loss_bwd: null pointer");
    GAN_CHECK_NC("dxmi_gan_logit_loss_bwd");
    DXMI_CHECK_ARG(weight == weight && weight <= 3.0e38f && weight >= -3.0e38f, "dxmi_gan_logit_loss_bwd: weight (%g) must be finite",
                   (double)weight);
    hipLaunchKernelGGL(gan_logit_loss_bwd_kernel, dim3((C + EW_BLOCK - 1) / EW_BLOCK), dim3(EW_BLOCK), 0, (hipStream_t)stream, (const bf16*)a, w,
                       sign, logit, upstream, weight, (bf16*)d_a, dw, db, N, C);
    DXMI_CHECK_LAUNCH("dxmi_gan_logit_loss_bwd");
    return DXMI_OK;
}

extern "C" int dxmi_gan_join(const float* g, const float* d_xin, const int64_t* indices, const float* t_table, int32_t num_scales, float* out,
                             int32_t N, int32_t CHW, float weight, float sigma_data, void* stream) {
    DXMI_CHECK_ARG(g && d_xin && indices && t_table && out, "dxmi_gan_join: null pointer");
    EW_CHECK_SHAPE("dxmi_gan_join");
    EW_CHECK_SCALES("dxmi_gan_join");
    DXMI_CHECK_ARG(weight == weight && weight <= 3.0e38f && weight >= -3.0e38f, "dxmi_gan_join: weight (%g) must be finite", (double)weight);
    EW_CHECK_POS("dxmi_gan_join", sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_gan_join", g, d_xin, out);
    DXMI_CHECK_ARG(out != d_xin, "dxmi_gan_join: out may alias g only");
    hipLaunchKernelGGL(gan_join_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, g, d_xin, indices, t_table, num_scales, out,
                       CHW, (float)CHW * weight, sigma_data * sigma_data);
    DXMI_CHECK_LAUNCH("dxmi_gan_join");
    return DXMI_OK;
}
