// The InceptionV3 extractor of inception_ops.hip in fp32 end to end (reference pytorch_fid/inception.py:16-163, :193-310, which runs
// torch fp32; evaluations/evaluator.py:584-616): NHWC fp32 activations, fp32 weights that are a pure re-layout of the checkpoint's
// `conv.weight`, BatchNorm applied in the conv epilogue instead of folded into the weights.  A scoring path, off the hot path: one
// shape-agnostic kernel per op, one summation order per layer shape (a pixel's result does not depend on N).
//   gconv_f32_kernel      implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain), operands straight from
//                         global memory.  Lane l supplies A[cout l % 32][k = l / 32] and B[k = l / 32][pixel l % 32], one VGPR each;
//                         it loads the 4 consecutive channels c + 4 (l / 32) .. + 3 of its pixel and of its cout as one 16-byte
//                         load each, which feeds four MFMAs with the k pairs (c + e, c + 4 + e), e = 0..3: the channel granule is 8.
//                         One accumulator per wave (issue interval = dependent latency = 64 cycles); the next step's operands are
//                         loaded before the current step's MFMAs issue, and a SIMD holds several waves.  Epilogue:
//                         v = fma(acc, scale[co], shift[co]) (BatchNorm), ReLU, one fp32 store at a channel offset of a wider tensor.
//                         The accumulator rows are those of the 32x32 bf16 instruction (generic_conv_kernel's epilogue).
//   pack_gconv_f32_kernel [Cout, Cin, KH, KW] -> [ceil32(Cout)][KH * KW][ceil8(Cin)] copied bit for bit (padding zero);
//                         scale = gamma / sqrt(var + eps), shift = beta - mean * scale (no BatchNorm: 1 and the conv bias or 0).
//   pool3x3_f32_kernel / global_avgpool_f32_kernel / resize_f32_kernel / nhwc_to_nchw_f32_kernel: the fp32 forms of the bf16 file's.
#include "common.h"

namespace {

constexpr int GRAN = 8;     // channel granule of the fp32 maps: two 16-byte loads per pixel and k step

struct GConvF32Args {
    const float* x;       // [N, IH, IW, Cin]  Cin % 8 == 0
    const float* w;       // [CoutP, KH * KW, Cin]  CoutP % 32 == 0 (rows >= Cout are zero)
    const float* scale;   // [CoutP]
    const float* shift;   // [CoutP]
    float* out;           // [N, OH, OW, out_cs] written at channel offset out_co
    int N, IH, IW, Cin, OH, OW, Cout, CoutP, KH, KW, SH, SW, PH, PW, out_cs, out_co, relu;
};

__global__ __launch_bounds__(256) void gconv_f32_kernel(GConvF32Args p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wp = wave & 1, wc = wave >> 1;                 // pixel half / cout half of the 64 x 64 workgroup tile
    const long P = (long)p.N * p.OH * p.OW;
    const long pix = (long)blockIdx.x * 64 + wp * 32 + (lane & 31);
    const int co_row = blockIdx.y * 64 + wc * 32;            // first cout of this wave
    if (co_row >= p.CoutP) return;
    const int half = lane >> 5;                               // which k of an MFMA's two
    const bool pvalid = pix < P;
    int n = 0, oy = 0, ox = 0;
    if (pvalid) {
        n = (int)(pix / ((long)p.OH * p.OW));
        const int r = (int)(pix - (long)n * p.OH * p.OW);
        oy = r / p.OW;
        ox = r - oy * p.OW;
    }
    const int taps = p.KH * p.KW;
    const float* wrow = p.w + ((size_t)(co_row + (lane & 31)) * taps) * p.Cin + half * 4;
    const float* ximg = p.x + (size_t)n * p.IH * p.IW * p.Cin + half * 4;
    const int iy0 = oy * p.SH - p.PH, ix0 = ox * p.SW - p.PW;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // operands of step (ky, kx, c): loaded one step ahead of the MFMAs that use them
    int ky = 0, kx = 0, c = 0;
    auto load = [&](f32x4& a, f32x4& b) {
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool ok = pvalid && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW;
        b = ok ? *reinterpret_cast<const f32x4*>(ximg + ((size_t)iy * p.IW + ix) * p.Cin + c) : zero;
        a = *reinterpret_cast<const f32x4*>(wrow + (size_t)(ky * p.KW + kx) * p.Cin + c);
    };
    const int steps = taps * (p.Cin / GRAN);
    f32x4 a, b;
    load(a, b);
    for (int s = 0; s < steps; ++s) {
        const f32x4 a0 = a, b0 = b;
        c += GRAN;
        if (c == p.Cin) {
            c = 0;
            if (++kx == p.KW) { kx = 0; ++ky; }
        }
        if (s + 1 < steps) load(a, b);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b0[e], acc, 0, 0, 0);
    }
    if (!pvalid) return;
    float* op = p.out + (size_t)pix * p.out_cs + p.out_co;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co_row + (r & 3) + 8 * (r >> 2) + 4 * half;        // accumulator row of element r
        if (co < p.Cout) {
            float v = fmaf(acc[r], p.scale[co], p.shift[co]);
            if (p.relu) v = v > 0.f ? v : 0.f;
            op[co] = v;
        }
    }
}

__global__ void pack_gconv_f32_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                      const float* __restrict__ conv_bias, float* __restrict__ wp, float* __restrict__ scale,
                                      float* __restrict__ shift, int Cout, int Cin, int KH, int KW, int CoutP, int CinP) {
    const long total = (long)CoutP * KH * KW * CinP;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(i % CinP);
        long r = i / CinP;
        const int t = (int)(r % (KH * KW));
        const int co = (int)(r / (KH * KW));
        wp[i] = (co < Cout && ci < Cin) ? w[(((size_t)co * Cin + ci) * KH + t / KW) * KW + t % KW] : 0.f;
    }
    for (int co = blockIdx.x * blockDim.x + threadIdx.x; co < CoutP; co += gridDim.x * blockDim.x) {
        float sc = 0.f, sh = 0.f;
        if (co < Cout) {
            sc = gamma ? gamma[co] / sqrtf(var[co] + eps) : 1.f;
            sh = gamma ? beta[co] - mean[co] * sc : (conv_bias ? conv_bias[co] : 0.f);
        }
        scale[co] = sc;
        shift[co] = sh;
    }
}

__global__ void pool3x3_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int IH, int IW, int C, int OH, int OW,
                                   int stride, int pad, int avg, int out_cs, int out_co) {
    const int C4 = C / 4;
    const long total = (long)N * OH * OW * C4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        long r = idx / C4;
        const int ox = (int)(r % OW); r /= OW;
        const int oy = (int)(r % OH);
        const int n = (int)(r / OH);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = avg ? 0.f : -INFINITY;
        int cnt = 0;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * stride - pad + ky;
            if (iy < 0 || iy >= IH) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * stride - pad + kx;
                if (ix < 0 || ix >= IW) continue;
                const f32x4 a = *reinterpret_cast<const f32x4*>(x + (((size_t)n * IH + iy) * IW + ix) * C + c4 * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = avg ? v[e] + a[e] : fmaxf(v[e], a[e]);
                ++cnt;
            }
        }
        if (avg) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] / (float)cnt;
        }
        *reinterpret_cast<f32x4*>(out + (((size_t)n * OH + oy) * OW + ox) * out_cs + out_co + c4 * 4) = v;
    }
}

__global__ void global_avgpool_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int HW, int C) {
    const long total = (long)N * C;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C), n = (int)(idx / C);
        float acc = 0.f;
        for (int p = 0; p < HW; ++p) acc += x[((size_t)n * HW + p) * C + c];
        out[idx] = acc / (float)HW;
    }
}

// the expressions of resize_norm_kernel (inception_ops.hip), stored as fp32 into 8 channels (3..7 zero)
__global__ void resize_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int IH, int IW, int OH, int OW, int normalize) {
    const long total = (long)N * OH * OW;
    const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int ox = (int)(idx % OW);
        long r = idx / OW;
        const int oy = (int)(r % OH), n = (int)(r / OH);
        float fy = ((float)oy + 0.5f) * sy - 0.5f, fx = ((float)ox + 0.5f) * sx - 0.5f;
        fy = fy < 0.f ? 0.f : fy;
        fx = fx < 0.f ? 0.f : fx;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < IH - 1 ? 1 : 0), x1 = x0 + (x0 < IW - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        f32x4 lo = {0.f, 0.f, 0.f, 0.f};
        const f32x4 hi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pl = x + ((size_t)n * 3 + c) * IH * IW;
            float v = (1.f - ly) * ((1.f - lx) * pl[(size_t)y0 * IW + x0] + lx * pl[(size_t)y0 * IW + x1]) +
                      ly * ((1.f - lx) * pl[(size_t)y1 * IW + x0] + lx * pl[(size_t)y1 * IW + x1]);
            if (normalize) v = 2.f * v - 1.f;
            lo[c] = v;
        }
        float* o = out + (size_t)idx * GRAN;
        *reinterpret_cast<f32x4*>(o) = lo;
        *reinterpret_cast<f32x4*>(o + 4) = hi;
    }
}

__global__ void nhwc_to_nchw_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int N, int C, int HW) {
    const long total = (long)N * C * HW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int px = (int)(idx % HW);
        const long r = idx / HW;
        const int c = (int)(r % C);
        const int n = (int)(r / C);
        out[idx] = in[((size_t)n * HW + px) * C + c];
    }
}

inline unsigned grid1d(long total, int block) {
    long g = (total + block - 1) / block;
    return (unsigned)(g > 65535L * 16 ? 65535L * 16 : (g < 1 ? 1 : g));
}

constexpr long MAX_ELEMS = 1L << 40;      // far beyond any device tensor; keeps every index product inside 64 bits

}  // namespace

extern "C" int64_t dxmi_gconv_f32_packed_elems(int32_t Cout, int32_t Cin, int32_t KH, int32_t KW) {
    if (Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return 0;
    const int64_t CoutP = ((int64_t)Cout + 31) / 32 * 32, CinP = ((int64_t)Cin + GRAN - 1) / GRAN * GRAN;
    return CoutP * KH * KW * CinP;
}

extern "C" int dxmi_gconv_f32_pack(const float* w, const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var,
                                   float bn_eps, const float* conv_bias, float* w_packed, float* scale, float* shift, int32_t Cout,
                                   int32_t Cin, int32_t KH, int32_t KW, void* stream) {
    DXMI_CHECK_ARG(w && w_packed && scale && shift, "dxmi_gconv_f32_pack: null pointer");
    DXMI_CHECK_ARG(Cout > 0 && Cin > 0 && KH > 0 && KW > 0, "dxmi_gconv_f32_pack: bad shape (Cout %d, Cin %d, k %dx%d)", Cout, Cin, KH, KW);
    DXMI_CHECK_ARG(!bn_gamma || (bn_beta && bn_mean && bn_var), "dxmi_gconv_f32_pack: BatchNorm needs gamma, beta, mean and var");
    DXMI_CHECK_ARG(!(bn_gamma && conv_bias), "dxmi_gconv_f32_pack: a conv bias excludes BatchNorm");
    const int64_t elems = dxmi_gconv_f32_packed_elems(Cout, Cin, KH, KW);
    DXMI_CHECK_ARG(elems < (1L << 31), "dxmi_gconv_f32_pack: packed weight too large (%lld elements)", (long long)elems);
    const int CoutP = (Cout + 31) / 32 * 32, CinP = (Cin + GRAN - 1) / GRAN * GRAN;
    hipLaunchKernelGGL(pack_gconv_f32_kernel, dim3(grid1d(elems, 256)), dim3(256), 0, (hipStream_t)stream, w, bn_gamma, bn_beta, bn_mean,
                       bn_var, bn_eps, conv_bias, w_packed, scale, shift, Cout, Cin, KH, KW, CoutP, CinP);
    DXMI_CHECK_LAUNCH("dxmi_gconv_f32_pack");
    return DXMI_OK;
}

extern "C" int dxmi_gconv_f32_fwd(const float* x, const float* w_packed, const float* scale, const float* shift, float* out, int32_t N,
                                  int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t SH, int32_t SW,
                                  int32_t PH, int32_t PW, int32_t out_cstride, int32_t out_coff, int32_t relu, void* stream) {
    DXMI_CHECK_ARG(x && w_packed && scale && shift && out, "dxmi_gconv_f32_fwd: null pointer");
    DXMI_CHECK_ARG(N > 0 && IH > 0 && IW > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && SH > 0 && SW > 0 && PH >= 0 && PW >= 0,
                   "dxmi_gconv_f32_fwd: bad shape (N %d, in %dx%dx%d, Cout %d, k %dx%d, s %dx%d, p %dx%d)", N, IH, IW, Cin, Cout, KH, KW, SH, SW, PH, PW);
    DXMI_CHECK_ARG(Cin % GRAN == 0, "dxmi_gconv_f32_fwd: Cin %d is not a multiple of 8 (the packed weight's padded channel count)", Cin);
    DXMI_CHECK_ARG((long)IH + 2L * PH >= KH && (long)IW + 2L * PW >= KW, "dxmi_gconv_f32_fwd: the %dx%d kernel does not fit the padded %ldx%ld map", KH, KW,
                   (long)IH + 2L * PH, (long)IW + 2L * PW);
    GConvF32Args a;
    a.x = x; a.w = w_packed; a.scale = scale; a.shift = shift; a.out = out;
    a.N = N; a.IH = IH; a.IW = IW; a.Cin = Cin; a.Cout = Cout; a.CoutP = (Cout + 31) / 32 * 32;
    a.KH = KH; a.KW = KW; a.SH = SH; a.SW = SW; a.PH = PH; a.PW = PW;
    a.OH = (IH + 2 * PH - KH) / SH + 1; a.OW = (IW + 2 * PW - KW) / SW + 1;
    DXMI_CHECK_ARG(out_coff >= 0 && (long)out_cstride >= (long)out_coff + Cout, "dxmi_gconv_f32_fwd: channel window [%d, %ld) outside the output's %d channels",
                   out_coff, (long)out_coff + Cout, out_cstride);
    a.out_cs = out_cstride; a.out_co = out_coff; a.relu = relu;
    const long P = (long)N * a.OH * a.OW;
    DXMI_CHECK_ARG((P + 63) / 64 < (1L << 31) && (long)N * IH * IW < (1L << 31) && (long)KH * KW * (Cin / GRAN) < (1L << 31),
                   "dxmi_gconv_f32_fwd: too many pixels (%ld outputs)", P);
    hipLaunchKernelGGL(gconv_f32_kernel, dim3((unsigned)((P + 63) / 64), (unsigned)((a.CoutP + 63) / 64)), dim3(256), 0, (hipStream_t)stream, a);
    DXMI_CHECK_LAUNCH("dxmi_gconv_f32_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_pool3x3_f32(const float* x, float* out, int32_t N, int32_t IH, int32_t IW, int32_t C, int32_t stride, int32_t pad,
                                int32_t avg_exclude_pad, int32_t out_cstride, int32_t out_coff, void* stream) {
    DXMI_CHECK_ARG(x && out, "dxmi_pool3x3_f32: null pointer");
    DXMI_CHECK_ARG(N > 0 && IH > 0 && IW > 0 && C > 0 && stride > 0 && pad >= 0 && pad <= 1, "dxmi_pool3x3_f32: bad shape (N %d, in %dx%dx%d, stride %d, pad %d)",
                   N, IH, IW, C, stride, pad);
    DXMI_CHECK_ARG(C % GRAN == 0, "dxmi_pool3x3_f32: C %d is not a multiple of 8", C);
    DXMI_CHECK_ARG(out_coff >= 0 && out_cstride % 4 == 0 && out_coff % 4 == 0 && (long)out_cstride >= (long)out_coff + C,
                   "dxmi_pool3x3_f32: channel window [%d, %ld) must be 4-aligned inside the output's %d channels", out_coff, (long)out_coff + C, out_cstride);
    DXMI_CHECK_ARG(IH + 2 * pad >= 3 && IW + 2 * pad >= 3, "dxmi_pool3x3_f32: the 3x3 window does not fit the padded %dx%d map", IH + 2 * pad, IW + 2 * pad);
    const int OH = (IH + 2 * pad - 3) / stride + 1, OW = (IW + 2 * pad - 3) / stride + 1;
    DXMI_CHECK_ARG((long)N * IH * IW < (1L << 31) && (long)N * OH * OW * (C / 4) < MAX_ELEMS, "dxmi_pool3x3_f32: too many pixels");
    hipLaunchKernelGGL(pool3x3_f32_kernel, dim3(grid1d((long)N * OH * OW * (C / 4), 256)), dim3(256), 0, (hipStream_t)stream, x, out, N, IH, IW, C, OH,
                       OW, stride, pad, avg_exclude_pad, out_cstride, out_coff);
    DXMI_CHECK_LAUNCH("dxmi_pool3x3_f32");
    return DXMI_OK;
}

extern "C" int dxmi_global_avgpool_f32(const float* x, float* out, int32_t N, int32_t HW, int32_t C, void* stream) {
    DXMI_CHECK_ARG(x && out, "dxmi_global_avgpool_f32: null pointer");
    DXMI_CHECK_ARG(N > 0 && HW > 0 && C > 0, "dxmi_global_avgpool_f32: bad shape (N %d, HW %d, C %d)", N, HW, C);
    DXMI_CHECK_ARG(C % GRAN == 0, "dxmi_global_avgpool_f32: C %d is not a multiple of 8", C);
    DXMI_CHECK_ARG((long)N * HW < (1L << 31) && (long)N * C < (1L << 31), "dxmi_global_avgpool_f32: too many pixels");
    hipLaunchKernelGGL(global_avgpool_f32_kernel, dim3(grid1d((long)N * C, 256)), dim3(256), 0, (hipStream_t)stream, x, out, N, HW, C);
    DXMI_CHECK_LAUNCH("dxmi_global_avgpool_f32");
    return DXMI_OK;
}

extern "C" int dxmi_resize_bilinear_nhwc_f32(const float* x, float* out, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW,
                                             int32_t normalize, void* stream) {
    DXMI_CHECK_ARG(x && out, "dxmi_resize_bilinear_nhwc_f32: null pointer");
    DXMI_CHECK_ARG(N > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0, "dxmi_resize_bilinear_nhwc_f32: bad shape (N %d, %dx%d -> %dx%d)", N, IH, IW, OH, OW);
    DXMI_CHECK_ARG((long)N * OH * OW < (1L << 31) && (long)N * 3 * IH * IW < MAX_ELEMS, "dxmi_resize_bilinear_nhwc_f32: too many pixels");
    hipLaunchKernelGGL(resize_f32_kernel, dim3(grid1d((long)N * OH * OW, 256)), dim3(256), 0, (hipStream_t)stream, x, out, N, IH, IW, OH, OW, normalize);
    DXMI_CHECK_LAUNCH("dxmi_resize_bilinear_nhwc_f32");
    return DXMI_OK;
}

extern "C" int dxmi_nhwc_f32_to_nchw_f32(const float* in, float* out, int32_t N, int32_t C, int32_t HW, void* stream) {
    DXMI_CHECK_ARG(in && out, "dxmi_nhwc_f32_to_nchw_f32: null pointer");
    DXMI_CHECK_ARG(N > 0 && C > 0 && HW > 0, "dxmi_nhwc_f32_to_nchw_f32: bad shape (N %d, C %d, HW %d)", N, C, HW);
    DXMI_CHECK_ARG((long)N * HW < (1L << 31) && (long)N * C * HW < MAX_ELEMS, "dxmi_nhwc_f32_to_nchw_f32: too many pixels");
    hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3(grid1d((long)N * C * HW, 256)), dim3(256), 0, (hipStream_t)stream, in, out, N, C, HW);
    DXMI_CHECK_LAUNCH("dxmi_nhwc_f32_to_nchw_f32");
    return DXMI_OK;
}
