// LPIPS (VGG16, piq's LPIPS(replace_pooling=True, reduction="none")) as a differentiable device loss: the launches around the 13
// convolutions, which themselves go through dxmi_gconv_fwd (inception_ops.hip) forward and, with transposed-and-flipped packed
// weights, backward.  Activations and gradients are NHWC bf16, sums fp32.
//   lpips_front_fwd_kernel   NCHW fp32 [M, 3, IH, IW] in [0, 1] -> bilinear resize (align_corners False; the identity when the sizes
//                            agree) -> (v - mean) / std -> NHWC bf16 with the 3 channels padded to 16 (zeros)
//   lpips_front_bwd_kernel   its transpose: every source pixel gathers the output pixels that tap it, in index order (no atomics),
//                            and divides by std
//   avgpool2x2_{fwd,bwd}     AvgPool2d(2, 2, 0): floor(size / 2); the backward writes zero into a dropped last row / column
//   lpips_tap_fwd_kernel     per pixel: f / (|f| + 1e-10) of both maps, sum_c w_c (fx^ - fy^)^2; a group of C / 8 lanes holds one
//                            pixel (16-byte loads), both passes out of registers; a workgroup's sum goes to partials[n][block] and
//                            lpips_tap_finish_kernel adds them in block order: out[n] (+)= sum / HW (bitwise reproducible)
//   lpips_tap_bwd_kernel     d fx of that for the per-sample upstream g[n] / HW, through the normalisation:
//                            q = 2 w (fx^ - fy^) s;  d fx = q / (|fx| + eps) - fx (fx . q) / (|fx| (|fx| + eps)^2)   (0 at |fx| = 0)
//   relu_mask_acc_kernel     g = (g_above + g_tap) * (act > 0), bf16
#include "common.h"

namespace {

constexpr int BLK = 256;
constexpr float LP_EPS = 1e-10f;
constexpr int TAP_MAX_BLOCKS = 128;

__constant__ float LP_MEAN[3] = {0.485f, 0.456f, 0.406f};
__constant__ float LP_STD[3] = {0.229f, 0.224f, 0.225f};

inline unsigned lp_grid(long total) {
    long g = (total + BLK - 1) / BLK;
    return (unsigned)(g > 65535L * 16 ? 65535L * 16 : (g < 1 ? 1 : g));
}

// torch's area_pixel_compute_source_index (align_corners False): src = (dst + 0.5) * scale - 0.5, clamped at 0
struct LTap {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ LTap lp_tap(int o, int in, float scale) {
    float src = ((float)o + 0.5f) * scale - 0.5f;
    src = src < 0.f ? 0.f : src;
    LTap r;
    r.i0 = (int)src;
    r.i0 = r.i0 > in - 1 ? in - 1 : r.i0;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

__global__ __launch_bounds__(BLK) void lpips_front_fwd_kernel(const float* __restrict__ x, bf16* __restrict__ out, int M, int IH, int IW,
                                                              int OH, int OW) {
    const long total = (long)M * OH * OW;
    const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;
    for (long idx = (long)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (long)gridDim.x * BLK) {
        const int ox = (int)(idx % OW);
        const long r = idx / OW;
        const int oy = (int)(r % OH), n = (int)(r / OH);
        const LTap ty = lp_tap(oy, IH, sy), tx = lp_tap(ox, IW, sx);
        bf16x8 lo, hi;
#pragma unroll
        for (int e = 0; e < 8; ++e) { lo[e] = (bf16)0.f; hi[e] = (bf16)0.f; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pl = x + ((size_t)n * 3 + c) * IH * IW;
            const float v = ty.l0 * (tx.l0 * pl[(size_t)ty.i0 * IW + tx.i0] + tx.l1 * pl[(size_t)ty.i0 * IW + tx.i1]) +
                            ty.l1 * (tx.l0 * pl[(size_t)ty.i1 * IW + tx.i0] + tx.l1 * pl[(size_t)ty.i1 * IW + tx.i1]);
            lo[c] = (bf16)((v - LP_MEAN[c]) / LP_STD[c]);
        }
        bf16* o = out + (size_t)idx * 16;
        *reinterpret_cast<bf16x8*>(o) = lo;
        *reinterpret_cast<bf16x8*>(o + 8) = hi;
    }
}

// one thread per source pixel: the outputs whose source index lies within one pixel of (y, x), the range widened by one on each
// side and every candidate checked exactly
__global__ __launch_bounds__(BLK) void lpips_front_bwd_kernel(const bf16* __restrict__ gz, float* __restrict__ dx, int N, int IH, int IW,
                                                              int OH, int OW) {
    const long total = (long)N * IH * IW;
    const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;
    for (long idx = (long)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (long)gridDim.x * BLK) {
        const int x = (int)(idx % IW);
        const long r = idx / IW;
        const int y = (int)(r % IH), n = (int)(r / IH);
        int oy0 = (int)floorf(((float)y - 0.5f) / sy - 0.5f) - 1, oy1 = (int)ceilf(((float)y + 1.5f) / sy - 0.5f) + 1;
        int ox0 = (int)floorf(((float)x - 0.5f) / sx - 0.5f) - 1, ox1 = (int)ceilf(((float)x + 1.5f) / sx - 0.5f) + 1;
        oy0 = oy0 < 0 ? 0 : oy0;
        ox0 = ox0 < 0 ? 0 : ox0;
        oy1 = oy1 > OH - 1 ? OH - 1 : oy1;
        ox1 = ox1 > OW - 1 ? OW - 1 : ox1;
        float acc[3] = {0.f, 0.f, 0.f};
        for (int oy = oy0; oy <= oy1; ++oy) {
            const LTap ty = lp_tap(oy, IH, sy);
            if (ty.i0 != y && ty.i1 != y) continue;
            const float wy = (ty.i0 == y ? ty.l0 : 0.f) + (ty.i1 == y ? ty.l1 : 0.f);
            for (int ox = ox0; ox <= ox1; ++ox) {
                const LTap tx = lp_tap(ox, IW, sx);
                if (tx.i0 != x && tx.i1 != x) continue;
                const float wx = (tx.i0 == x ? tx.l0 : 0.f) + (tx.i1 == x ? tx.l1 : 0.f);
                const bf16x4 g = *reinterpret_cast<const bf16x4*>(gz + (((size_t)n * OH + oy) * OW + ox) * 16);
                const float w = wy * wx;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += w * (float)g[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dx[(((size_t)n * 3 + c) * IH + y) * IW + x] = acc[c] / LP_STD[c];
    }
}

__global__ __launch_bounds__(BLK) void avgpool2x2_fwd_kernel(const bf16* __restrict__ x, bf16* __restrict__ out, int N, int IH, int IW, int C) {
    const int OH = IH / 2, OW = IW / 2, C8 = C / 8;
    const long total = (long)N * OH * OW * C8;
    for (long idx = (long)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (long)gridDim.x * BLK) {
        const int c8 = (int)(idx % C8);
        long r = idx / C8;
        const int ox = (int)(r % OW); r /= OW;
        const int oy = (int)(r % OH), n = (int)(r / OH);
        const bf16* p = x + (((size_t)n * IH + 2 * oy) * IW + 2 * ox) * C + c8 * 8;
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(p), b = *reinterpret_cast<const bf16x8*>(p + C);
        const bf16x8 c = *reinterpret_cast<const bf16x8*>(p + (size_t)IW * C), d = *reinterpret_cast<const bf16x8*>(p + (size_t)IW * C + C);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)((((float)a[e] + (float)b[e]) + ((float)c[e] + (float)d[e])) * 0.25f);
        *reinterpret_cast<bf16x8*>(out + (size_t)idx * 8) = o;
    }
}

__global__ __launch_bounds__(BLK) void avgpool2x2_bwd_kernel(const bf16* __restrict__ gout, bf16* __restrict__ gin, int N, int IH, int IW, int C) {
    const int OH = IH / 2, OW = IW / 2, C8 = C / 8;
    const long total = (long)N * IH * IW * C8;
    for (long idx = (long)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (long)gridDim.x * BLK) {
        const int c8 = (int)(idx % C8);
        long r = idx / C8;
        const int x = (int)(r % IW); r /= IW;
        const int y = (int)(r % IH), n = (int)(r / IH);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)0.f;
        if (y < 2 * OH && x < 2 * OW) {
            const bf16x8 g = *reinterpret_cast<const bf16x8*>(gout + (((size_t)n * OH + y / 2) * OW + x / 2) * C + c8 * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)((float)g[e] * 0.25f);
        }
        *reinterpret_cast<bf16x8*>(gin + (size_t)idx * 8) = o;
    }
}

// sum over the L lanes (a power of two, aligned) that hold one pixel: every lane of the group ends with the same value
__device__ __forceinline__ float group_sum(float v, int L) {
    for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct TapPix {
    float fx[8], fy[8], ax, ay, nx;      // the lane's 8 channels of both maps; 1 / (|f| + eps) of both; |fx|
};

__device__ __forceinline__ TapPix tap_load(const bf16* __restrict__ fx, const bf16* __restrict__ fy, size_t pix, int C, int c0, int L) {
    TapPix t;
    float sx = 0.f, sy = 0.f;
    if (c0 < C) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(fx + pix * C + c0), b = *reinterpret_cast<const bf16x8*>(fy + pix * C + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            t.fx[e] = (float)a[e];
            t.fy[e] = (float)b[e];
            sx += t.fx[e] * t.fx[e];
            sy += t.fy[e] * t.fy[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) t.fx[e] = t.fy[e] = 0.f;
    }
    t.nx = __builtin_sqrtf(group_sum(sx, L));
    t.ax = 1.f / (t.nx + LP_EPS);
    t.ay = 1.f / (__builtin_sqrtf(group_sum(sy, L)) + LP_EPS);
    return t;
}

// grid (G, N); pixel slots of 256 / L per workgroup.  Every lane of a wave runs the same number of iterations (the shuffles need
// all lanes): a slot past the last pixel computes on pixel 0 and adds nothing.
__global__ __launch_bounds__(BLK) void lpips_tap_fwd_kernel(const bf16* __restrict__ fx, const bf16* __restrict__ fy, const float* __restrict__ w,
                                                            float* __restrict__ partials, int HW, int C, int L) {
    __shared__ float red[BLK / 64];
    const int n = blockIdx.y, G = gridDim.x;
    const int per = BLK / L, slot = blockIdx.x * per + threadIdx.x / L, slots = G * per;
    const int c0 = (threadIdx.x % L) * 8;
    float wc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) wc[e] = c0 < C ? w[c0 + e] : 0.f;
    float acc = 0.f;
    const int iters = (HW + slots - 1) / slots;
    for (int it = 0; it < iters; ++it) {
        const int p = slot + it * slots;
        const bool ok = p < HW;
        const TapPix t = tap_load(fx, fy, (size_t)n * HW + (ok ? p : 0), C, c0, L);
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float u = t.fx[e] * t.ax - t.fy[e] * t.ay;
            d += wc[e] * (u * u);
        }
        acc += ok ? d : 0.f;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(size_t)n * G + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void lpips_tap_finish_kernel(const float* __restrict__ partials, const float* __restrict__ scale, float* __restrict__ out, int N,
                                        int G, float invHW, int accumulate) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += partials[(size_t)n * G + g];
    float v = s * invHW;
    if (accumulate) v = out[n] + v;
    out[n] = scale ? v * scale[n] : v;
}

__global__ __launch_bounds__(BLK) void lpips_tap_bwd_kernel(const float* __restrict__ g, const bf16* __restrict__ fx, const bf16* __restrict__ fy,
                                                            const float* __restrict__ w, bf16* __restrict__ dfx, int HW, int C, int L,
                                                            float invHW) {
    const int n = blockIdx.y, G = gridDim.x;
    const int per = BLK / L, slot = blockIdx.x * per + threadIdx.x / L, slots = G * per;
    const int c0 = (threadIdx.x % L) * 8;
    const float s = (g ? g[n] : 1.f) * invHW;
    float wc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) wc[e] = c0 < C ? w[c0 + e] : 0.f;
    const int iters = (HW + slots - 1) / slots;
    for (int it = 0; it < iters; ++it) {
        const int p = slot + it * slots;
        const bool ok = p < HW;
        const size_t pix = (size_t)n * HW + (ok ? p : 0);
        const TapPix t = tap_load(fx, fy, pix, C, c0, L);
        float q[8], dot = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            q[e] = (2.f * wc[e]) * (t.fx[e] * t.ax - t.fy[e] * t.ay) * s;
            dot += t.fx[e] * q[e];
        }
        dot = group_sum(dot, L);
        const float k = t.nx > 0.f ? dot * (t.ax * t.ax) / t.nx : 0.f;
        if (ok && c0 < C) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)(q[e] * t.ax - t.fx[e] * k);
            *reinterpret_cast<bf16x8*>(dfx + pix * C + c0) = o;
        }
    }
}

__global__ __launch_bounds__(BLK) void relu_mask_acc_kernel(const bf16* __restrict__ ga, const bf16* __restrict__ gb, const bf16* __restrict__ act,
                                                            bf16* __restrict__ out, long n8) {
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < n8; i += (long)gridDim.x * BLK) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(ga + i * 8), m = *reinterpret_cast<const bf16x8*>(act + i * 8);
        bf16x8 b;
        if (gb) b = *reinterpret_cast<const bf16x8*>(gb + i * 8);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = gb ? (float)a[e] + (float)b[e] : (float)a[e];
            o[e] = (bf16)((float)m[e] > 0.f ? v : 0.f);
        }
        *reinterpret_cast<bf16x8*>(out + i * 8) = o;
    }
}

inline bool lp_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

inline int tap_lanes(int C) {      // lanes per pixel: the power of two that covers C / 8
    int L = 2;
    while (L * 8 < C) L <<= 1;
    return L;
}

inline int tap_blocks(int HW, int L) {
    const int per = BLK / L, g = (HW + per - 1) / per;
    return g < TAP_MAX_BLOCKS ? g : TAP_MAX_BLOCKS;
}

}  // namespace

#define LP_CHECK_IMG(fn)                                                                                                              \
    DXMI_CHECK_ARG(N > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0 && IH <= 16384 && IW <= 16384 && OH <= 16384 && OW <= 16384,         \
                   fn ": N (%d) must be positive and the sizes %dx%d -> %dx%d in [1, 16384]", N, IH, IW, OH, OW)

extern "C" int dxmi_lpips_front_fwd(const float* x, void* out, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW, void* stream) {
    DXMI_CHECK_ARG(x && out, "dxmi_lpips_front_fwd: null pointer");
    LP_CHECK_IMG("dxmi_lpips_front_fwd");
    DXMI_CHECK_ARG(lp_aligned(out), "dxmi_lpips_front_fwd: out must be 16-byte aligned");
    hipLaunchKernelGGL(lpips_front_fwd_kernel, dim3(lp_grid((long)N * OH * OW)), dim3(BLK), 0, (hipStream_t)stream, x, (bf16*)out, N, IH, IW, OH, OW);
    DXMI_CHECK_LAUNCH("dxmi_lpips_front_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_lpips_front_bwd(const void* g_out, float* d_x, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW, void* stream) {
    DXMI_CHECK_ARG(g_out && d_x, "dxmi_lpips_front_bwd: null pointer");
    LP_CHECK_IMG("dxmi_lpips_front_bwd");
    DXMI_CHECK_ARG(lp_aligned(g_out), "dxmi_lpips_front_bwd: g_out must be 16-byte aligned");
    hipLaunchKernelGGL(lpips_front_bwd_kernel, dim3(lp_grid((long)N * IH * IW)), dim3(BLK), 0, (hipStream_t)stream, (const bf16*)g_out, d_x, N, IH, IW,
                       OH, OW);
    DXMI_CHECK_LAUNCH("dxmi_lpips_front_bwd");
    return DXMI_OK;
}

#define LP_CHECK_POOL(fn)                                                                                                             \
    DXMI_CHECK_ARG(N > 0 && IH >= 2 && IW >= 2 && C > 0 && C % 8 == 0, fn ": N (%d) must be positive, the map %dx%d at least 2x2 "    \
                   "and C (%d) a positive multiple of 8", N, IH, IW, C)

extern "C" int dxmi_avgpool2x2_fwd(const void* x, void* out, int32_t N, int32_t IH, int32_t IW, int32_t C, void* stream) {
    DXMI_CHECK_ARG(x && out, "dxmi_avgpool2x2_fwd: null pointer");
    LP_CHECK_POOL("dxmi_avgpool2x2_fwd");
    DXMI_CHECK_ARG(lp_aligned(x, out), "dxmi_avgpool2x2_fwd: tensors must be 16-byte aligned");
    hipLaunchKernelGGL(avgpool2x2_fwd_kernel, dim3(lp_grid((long)N * (IH / 2) * (IW / 2) * (C / 8))), dim3(BLK), 0, (hipStream_t)stream, (const bf16*)x,
                       (bf16*)out, N, IH, IW, C);
    DXMI_CHECK_LAUNCH("dxmi_avgpool2x2_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_avgpool2x2_bwd(const void* g_out, void* g_in, int32_t N, int32_t IH, int32_t IW, int32_t C, void* stream) {
    DXMI_CHECK_ARG(g_out && g_in, "dxmi_avgpool2x2_bwd: null pointer");
    LP_CHECK_POOL("dxmi_avgpool2x2_bwd");
    DXMI_CHECK_ARG(lp_aligned(g_out, g_in), "dxmi_avgpool2x2_bwd: tensors must be 16-byte aligned");
    hipLaunchKernelGGL(avgpool2x2_bwd_kernel, dim3(lp_grid((long)N * IH * IW * (C / 8))), dim3(BLK), 0, (hipStream_t)stream, (const bf16*)g_out,
                       (bf16*)g_in, N, IH, IW, C);
    DXMI_CHECK_LAUNCH("dxmi_avgpool2x2_bwd");
    return DXMI_OK;
}

#define LP_CHECK_TAP(fn)                                                                                                              \
    DXMI_CHECK_ARG(N > 0 && N <= 65535 && HW > 0 && C >= 16 && C <= 512 && C % 16 == 0, fn ": N (%d) must be in [1, 65535], HW (%d) " \
                   "positive and C (%d) a multiple of 16 in [16, 512]", N, HW, C)

extern "C" int64_t dxmi_lpips_tap_partials(int32_t HW, int32_t C) {
    if (HW <= 0 || C < 16 || C > 512 || C % 16 != 0) return 0;
    return tap_blocks(HW, tap_lanes(C));
}

extern "C" int dxmi_lpips_tap_fwd(const void* fx, const void* fy, const float* w, const float* scale, float* partials, float* out, int32_t N,
                                  int32_t HW, int32_t C, int32_t accumulate, void* stream) {
    DXMI_CHECK_ARG(fx && fy && w && partials && out, "dxmi_lpips_tap_fwd: null pointer");
    LP_CHECK_TAP("dxmi_lpips_tap_fwd");
    DXMI_CHECK_ARG(lp_aligned(fx, fy), "dxmi_lpips_tap_fwd: feature maps must be 16-byte aligned");
    const int L = tap_lanes(C), G = tap_blocks(HW, L);
    hipLaunchKernelGGL(lpips_tap_fwd_kernel, dim3(G, N), dim3(BLK), 0, (hipStream_t)stream, (const bf16*)fx, (const bf16*)fy, w, partials, HW, C, L);
    DXMI_CHECK_LAUNCH("dxmi_lpips_tap_fwd");
    hipLaunchKernelGGL(lpips_tap_finish_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, partials, scale, out, N, G,
                       (float)(1.0 / (double)HW), (int)(accumulate != 0));
    DXMI_CHECK_LAUNCH("dxmi_lpips_tap_fwd (finish)");
    return DXMI_OK;
}

extern "C" int dxmi_lpips_tap_bwd(const float* g, const void* fx, const void* fy, const float* w, void* d_fx, int32_t N, int32_t HW, int32_t C,
                                  void* stream) {
    DXMI_CHECK_ARG(fx && fy && w && d_fx, "dxmi_lpips_tap_bwd: null pointer");
    LP_CHECK_TAP("dxmi_lpips_tap_bwd");
    DXMI_CHECK_ARG(lp_aligned(fx, fy, d_fx), "dxmi_lpips_tap_bwd: feature maps must be 16-byte aligned");
    const int L = tap_lanes(C), G = tap_blocks(HW, L);
    hipLaunchKernelGGL(lpips_tap_bwd_kernel, dim3(G, N), dim3(BLK), 0, (hipStream_t)stream, g, (const bf16*)fx, (const bf16*)fy, w, (bf16*)d_fx, HW, C,
                       L, (float)(1.0 / (double)HW));
    DXMI_CHECK_LAUNCH("dxmi_lpips_tap_bwd");
    return DXMI_OK;
}

extern "C" int dxmi_relu_mask_acc(const void* g_a, const void* g_b, const void* act, void* out, int64_t numel, void* stream) {
    DXMI_CHECK_ARG(g_a && act && out, "dxmi_relu_mask_acc: null pointer");
    DXMI_CHECK_ARG(numel > 0 && numel % 8 == 0, "dxmi_relu_mask_acc: numel (%lld) must be a positive multiple of 8", (long long)numel);
    DXMI_CHECK_ARG(lp_aligned(g_a, g_b, act, out), "dxmi_relu_mask_acc: tensors must be 16-byte aligned");
    hipLaunchKernelGGL(relu_mask_acc_kernel, dim3(lp_grid(numel / 8)), dim3(BLK), 0, (hipStream_t)stream, (const bf16*)g_a, (const bf16*)g_b,
                       (const bf16*)act, (bf16*)out, (long)(numel / 8));
    DXMI_CHECK_LAUNCH("dxmi_relu_mask_acc");
    return DXMI_OK;
}
