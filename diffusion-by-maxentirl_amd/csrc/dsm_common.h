// Karras scalings, loss weights, input scaling and time shared by the DSM loss (edm_dsm.hip) and the consistency, progressive and
// distribution-matching launches (cm_train.hip, pd_train.hip, dm_train.hip, sid_train.hip).
#pragma once
#include "common.h"

// the reference's fp32 operation order, one rounding per torch op: no fused multiply-add between them.  The pragma is at file
// scope: it holds for the rest of every file that includes this header.
#pragma clang fp contract(off)

namespace {

struct DsmScal {
    float c_skip, c_out, c_in, w;
};

// KarrasDenoiser.get_scalings / get_scalings_for_boundary_condition (:64-80) and get_weightings (:18-31) on the fp32 sigma, in
// torch's forms: x**2 = x*x, x**0.5 = sqrt, python scalar / tensor = reciprocal(tensor) * scalar, x**-2 = 1 / (x*x).
__device__ __forceinline__ DsmScal dsm_scalings(float s, float sd, float sd2, float sigma_min, int distill, int sched, float inv_sd2) {
    DsmScal r;
    const float den = s * s + sd2;
    const float root = __builtin_sqrtf(den);
    r.c_in = 1.f / root;
    if (distill) {
        const float sm = s - sigma_min;
        r.c_skip = (1.f / (sm * sm + sd2)) * sd2;
        r.c_out = (sm * sd) / root;
    } else {
        r.c_skip = (1.f / den) * sd2;
        r.c_out = (s * sd) / root;
    }
    const float snr = 1.f / (s * s);
    switch (sched) {
        case DXMI_DSM_W_SNR:       r.w = snr; break;
        case DXMI_DSM_W_SNR_P1:    r.w = snr + 1.f; break;
        case DXMI_DSM_W_KARRAS:    r.w = snr + inv_sd2; break;
        case DXMI_DSM_W_TRUNC_SNR: r.w = snr < 1.f ? 1.f : snr; break;    // th.clamp(snrs, min=1.0): NaN passes
        default:                   r.w = 1.f; break;                      // UNIFORM; DXMI_DSM_W_ICT needs two levels: loss_scalings (cm_train.hip)
    }
    return r;
}

// the network's input scaling and time at level s (denoise(), :348-349): c_in alone, and 1000 * 0.25 * th.log(sigmas + 1e-44)
__device__ __forceinline__ float dsm_c_in(float s, float sd2) { return 1.f / __builtin_sqrtf(s * s + sd2); }
__device__ __forceinline__ float dsm_time(float s) { return 250.f * logf(s + 1e-44f); }

}  // namespace
