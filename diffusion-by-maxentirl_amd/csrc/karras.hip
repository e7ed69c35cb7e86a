// Karras samplers of the EDM teacher (Heun, DPM-2, Euler, Euler-ancestral; reference models/cm/karras_diffusion.py:354-640):
// ONE launch between two network evaluations.  Each launch finishes the update that the evaluation it follows belongs to and
// writes the next evaluation's preconditioned input c_in(s') x' and time 250 ln(s' + 1e-44), or, after the last evaluation,
// the clamped sample.  Every per-step scalar (sigmas, scalings, step sizes, churn) is read from a small fp32 table built once
// per schedule on the host (models/cm/karras_diffusion.py), so a captured graph of the whole loop needs no host inputs.
#include "common.h"

// the reference's fp32 operation order, one rounding per torch op: no fused multiply-add between them
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }   // NaN passes, as torch.clamp

__global__ __launch_bounds__(256) void karras_stage_kernel(int mode, int last, const float* __restrict__ row, float* x,
                                                           float* x2, float* dbuf, const float* __restrict__ F,
                                                           const float* __restrict__ noise, float* __restrict__ x_in,
                                                           float* __restrict__ t_out, float* __restrict__ out,
                                                           float* __restrict__ denoised_out, int CHW) {
    const int b = blockIdx.y;
    const float sig = row[DXMI_KT_SIGMA], c_skip = row[DXMI_KT_CSKIP], c_out = row[DXMI_KT_COUT], dt = row[DXMI_KT_DT];
    const float s_up = row[DXMI_KT_SIGMA_UP], churn = row[DXMI_KT_CHURN], s_noise = row[DXMI_KT_SNOISE];
    const float c_in = row[DXMI_KT_CIN], x_scale = row[DXMI_KT_XSCALE];
    const bool clip = row[DXMI_KT_CLIP] != 0.f;
    if (!last && blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = row[DXMI_KT_T];
    const size_t base = (size_t)b * CHW;
    for (int i = (blockIdx.x * 256 + threadIdx.x) * 4; i < CHW; i += gridDim.x * 256 * 4) {
        const size_t o = base + i;
        f32x4 xn;
        if (mode == DXMI_KARRAS_FIRST) {
            xn = *reinterpret_cast<const f32x4*>(x + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) xn[e] = xn[e] * x_scale;                 // x_T = randn * sigma_max
        } else {
            const bool corr = mode == DXMI_KARRAS_HEUN_CORR || mode == DXMI_KARRAS_DPM_CORR;
            const f32x4 xe = *reinterpret_cast<const f32x4*>((corr ? x2 : x) + o);   // the point F was evaluated at
            const f32x4 fv = *reinterpret_cast<const f32x4*>(F + o);
            f32x4 den, d;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                den[e] = c_out * fv[e] + c_skip * xe[e];                          // denoise() (:348-351)
                if (clip) den[e] = clamp1(den[e]);                                // clip_denoised (:408-412)
                d[e] = (xe[e] - den[e]) / sig;                                    // to_d (:432-434)
            }
            if (denoised_out) *reinterpret_cast<f32x4*>(denoised_out + o) = den;
            if (mode == DXMI_KARRAS_PRED) {                                       // x_2 = x_hat + d dt_1 (:541-542, :614-617)
                *reinterpret_cast<f32x4*>(dbuf + o) = d;
#pragma unroll
                for (int e = 0; e < 4; ++e) xn[e] = xe[e] + d[e] * dt;
                *reinterpret_cast<f32x4*>(x2 + o) = xn;
            } else if (mode == DXMI_KARRAS_HEUN_CORR) {                           // x = x_hat + ((d + d_2) / 2) dt (:543-546)
                const f32x4 xh = *reinterpret_cast<const f32x4*>(x + o);
                const f32x4 d1 = *reinterpret_cast<const f32x4*>(dbuf + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) xn[e] = xh[e] + ((d1[e] + d[e]) / 2.f) * dt;
            } else if (mode == DXMI_KARRAS_DPM_CORR) {                            // x = x_hat + d_2 dt_2 (:618-620)
                const f32x4 xh = *reinterpret_cast<const f32x4*>(x + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) xn[e] = xh[e] + d[e] * dt;
            } else {                                                              // Euler (:537-539, :576-577) / ancestral (:476-478)
#pragma unroll
                for (int e = 0; e < 4; ++e) xn[e] = xe[e] + d[e] * dt;
                if (mode == DXMI_KARRAS_ANCESTRAL && noise) {
                    const f32x4 z = *reinterpret_cast<const f32x4*>(noise + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) xn[e] = xn[e] + z[e] * s_up;
                }
            }
        }
        if (mode == DXMI_KARRAS_PRED) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = c_in * xn[e];
            *reinterpret_cast<f32x4*>(x_in + o) = v;
            continue;
        }
        if (last) {                                                               // karras_sample's x_0.clamp(-1, 1) (:420)
#pragma unroll
            for (int e = 0; e < 4; ++e) xn[e] = clamp1(xn[e]);
            *reinterpret_cast<f32x4*>(out + o) = xn;
            continue;
        }
        if (noise && mode != DXMI_KARRAS_ANCESTRAL) {                             // next step's churn (:523-527)
            const f32x4 ev = *reinterpret_cast<const f32x4*>(noise + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) xn[e] = xn[e] + (ev[e] * s_noise) * churn;
        }
        *reinterpret_cast<f32x4*>(x + o) = xn;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c_in * xn[e];
        *reinterpret_cast<f32x4*>(x_in + o) = v;
    }
}

}  // namespace

extern "C" int dxmi_karras_stage(int32_t mode, int32_t last, const float* tab, int32_t row, float* x, float* x2, float* d,
                                 const float* model_out, const float* noise, float* x_in, float* t_out, float* out,
                                 float* denoised, int32_t N, int32_t CHW, void* stream) {
    DXMI_CHECK_ARG(mode >= DXMI_KARRAS_FIRST && mode <= DXMI_KARRAS_ANCESTRAL, "dxmi_karras_stage: unknown mode %d", mode);
    DXMI_CHECK_ARG(N > 0 && CHW > 0 && CHW % 4 == 0, "dxmi_karras_stage: N (%d) must be > 0 and CHW (%d) a positive multiple of 4",
                   N, CHW);
    DXMI_CHECK_ARG(N <= 65535 && row >= 0, "dxmi_karras_stage: N (%d) above 65535 or negative table row (%d)", N, row);
    DXMI_CHECK_ARG(tab && x, "dxmi_karras_stage: null table or state");
    const bool first = mode == DXMI_KARRAS_FIRST, pred = mode == DXMI_KARRAS_PRED;
    DXMI_CHECK_ARG(first || model_out, "dxmi_karras_stage: null model output");
    DXMI_CHECK_ARG(!(first && last), "dxmi_karras_stage: the first stage cannot be the last");
    DXMI_CHECK_ARG(!(pred && last), "dxmi_karras_stage: a predictor stage cannot be the last");
    DXMI_CHECK_ARG(!(pred || mode == DXMI_KARRAS_HEUN_CORR || mode == DXMI_KARRAS_DPM_CORR) || x2,
                   "dxmi_karras_stage: predictor/corrector stages need x2");
    DXMI_CHECK_ARG(!(pred || mode == DXMI_KARRAS_HEUN_CORR) || d, "dxmi_karras_stage: heun/dpm predictor and heun corrector need d");
    DXMI_CHECK_ARG(last ? out != nullptr : (x_in && t_out), "dxmi_karras_stage: null output (out when last, else x_in and t)");
    DXMI_CHECK_ARG(!(pred && noise), "dxmi_karras_stage: a predictor stage draws no noise");
    const int chunks = (CHW / 4 + 255) / 256;
    const dim3 grid(chunks < 16 ? chunks : 16, N);
    hipLaunchKernelGGL(karras_stage_kernel, grid, dim3(256), 0, (hipStream_t)stream, mode, last, tab + (size_t)row * DXMI_KT_COLS, x,
                       x2, d, model_out, noise, x_in, t_out, out, denoised, CHW);
    DXMI_CHECK_LAUNCH("dxmi_karras_stage");
    return DXMI_OK;
}
