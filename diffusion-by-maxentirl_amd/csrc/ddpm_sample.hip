// Ancestral / DDIM sampling of the DDPM teacher (models/DxMI/ddpm_sample.py; Ho et al. 2020, "Denoising Diffusion Probabilistic
// Models", Algorithm 2 and eq. 7; Song et al. 2021, "Denoising Diffusion Implicit Models", eq. 12 and 16).
//   dxmi_ddpm_stage  finishes the transition the evaluation it follows belongs to: the stage launch of stage_common.h (the
//                    control block, the table row, the noise, the loop and the tail are there) with the element below, which is
//                    Ho et al.'s clip form or the VAR sampler's linear form, and with no history.
// HBM-bound with explicit noise; with fused noise the Philox rounds and logf / sinf / cosf make it VALU-bound, which buys one launch
// and one write plus read of z per transition.
// One rounding per operation (stage_common.h turns contraction off for everything below it); the one explicit fused multiply-add
// is the linear form's, as in dxmi_var_step_fwd (assoc 1).
#include "stage_common.h"

namespace {

struct DdpmStage {
    static constexpr int COLS = DXMI_DT_COLS, T = DXMI_DT_T, T_NEXT = DXMI_DT_T_NEXT, FLAGS = DXMI_DT_FLAGS;
    static constexpr int FLAG_LAST = DXMI_DT_FLAG_LAST, HIST = 0;
    static constexpr bool XIN = false, CORR = false;

    struct StageCoef {
        float xm, c, s, a, b, q, r, c0, c1;
        bool clip, noisy;
    };

    // a poisoned row: every coefficient NaN and no noise (s = 0: neither z nor the generator is touched)
    static __device__ __forceinline__ StageCoef fill(const float* r, bool ok, int flags) {
        const float nan = __builtin_nanf("");
        StageCoef k;
        k.xm = ok ? r[DXMI_DT_XM] : nan, k.c = ok ? r[DXMI_DT_C] : nan, k.s = ok ? r[DXMI_DT_S] : 0.f;
        k.a = ok ? r[DXMI_DT_A] : nan, k.b = ok ? r[DXMI_DT_B] : nan, k.q = ok ? r[DXMI_DT_Q] : nan, k.r = ok ? r[DXMI_DT_R] : nan;
        k.c0 = ok ? r[DXMI_DT_C0] : nan, k.c1 = ok ? r[DXMI_DT_C1] : nan;
        k.clip = (flags & DXMI_DT_FLAG_CLIP) != 0;
        return k;
    }

    // one element of the transition -> x'; *pred = the predicted x_0 (clamped in the clip form); no history
    static __device__ __forceinline__ float stage_elem(const StageCoef& k, float x, float e, const float*, float z, float* pred) {
        const float pa = k.a * x, pb = k.b * e;
        const float x0 = pa - pb;                                 // x / sqrt(a_t) - sqrt(1 / a_t - 1) eps
        if (k.clip) {
            const float x0c = clamp1(x0);
            *pred = x0c;
            const float eh = (x - k.q * x0c) * k.r;               // the noise that x0c implies
            const float m = k.c0 * x0c + k.c1 * eh;
            return k.noisy ? m + k.s * z : m;
        }
        *pred = x0;
        const float xs = k.xm * x, ct = k.c * e;
        // x *= xm; x += control + sigma z.  dxmi_var_step_fwd (assoc 1), whose file leaves contraction on, evaluates control +
        // sigma z as ONE fused multiply-add on rounded xs and control; it is written out here so that the two launches agree bit
        // for bit.
        return k.noisy ? xs + __builtin_fmaf(k.s, z, ct) : xs + ct;
    }
};

template <bool ALIGNED>
__global__ __launch_bounds__(STAGE_BLOCK) void ddpm_stage_kernel(int first, const float* __restrict__ tab, int rows,
                                                                 const int32_t* __restrict__ ctl, int row_v, uint32_t draw_v,
                                                                 uint32_t k0_v, uint32_t k1_v, float* x, const float* __restrict__ eps,
                                                                 const float* __restrict__ z, const int64_t* __restrict__ sample_index,
                                                                 float* __restrict__ t_out, float* __restrict__ out,
                                                                 float* __restrict__ pred, int CHW) {
    stage_body<DdpmStage, ALIGNED>(first, tab, rows, ctl, row_v, draw_v, k0_v, k1_v, x, eps, z, sample_index, nullptr, t_out, out, pred,
                                   0, CHW);
}

}  // namespace

extern "C" int dxmi_ddpm_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw,
                               uint64_t seed, float* x, const float* eps, const float* z, const int64_t* sample_index, float* t_out,
                               float* out, float* pred_xstart, int32_t N, int32_t CHW, void* stream) {
    const char* fn = "dxmi_ddpm_stage";
    const bool first = mode == DXMI_DDPM_FIRST;
    if (int e = stage_check_launch(fn, mode, first || mode == DXMI_DDPM_STEP, first, tab, rows, ctl, row, x, eps, t_out, out, N, CHW))
        return e;
    if (!first)
        if (int e = stage_check_tensors(fn, x, eps, z, sample_index, nullptr, out, pred_xstart)) return e;
    return stage_launch(fn, ddpm_stage_kernel<true>, ddpm_stage_kernel<false>, first, N, CHW, stream, (int)first, tab, (int)rows, ctl,
                        (int)row, draw, (uint32_t)seed, (uint32_t)(seed >> 32), x, eps, z, sample_index, t_out, out, pred_xstart,
                        (int)CHW);
}
