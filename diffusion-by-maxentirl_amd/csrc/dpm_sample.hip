// DPM-Solver++ sampling of the DDPM teacher (models/DxMI/dpm_sample.py; Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided
// Sampling of Diffusion Probabilistic Models", Algorithm 2 and its SDE variant).
//   dxmi_dpm_stage  turns the evaluation it follows into the data prediction D_k, files it in the history and finishes the
//                   multistep transition: the stage launch of stage_common.h (the control block, the table row, the noise, the
//                   history ring, the loop and the tail are there) with the element below and two history reads.
// The history is fp32 [3][N][CHW]: D_k goes to slot k % 3, D_{k-1} and D_{k-2} come from slots (k + 2) % 3 and (k + 1) % 3, all
// three derived in the launch from the row number.  A weight that is exactly 0 means its slot is NOT read: the warm-up rows and the
// rows lower_order_final lowers never touch history that was never written (0 * NaN would be NaN).
// Per element, one rounding per operation (stage_common.h turns contraction off for everything below it), in this order:
//   1. D0 = a x - b eps;  D0 = clamp(D0, -1, 1) with FLAG_CLIP (NaN passes)
//   2. acc = cx x + w0 D0
//   3. acc += w1 D1    if w1 != 0
//   4. acc += w2 D2    if w2 != 0
//   5. acc += s z      if s != 0
// HBM-bound.
#include "stage_common.h"

namespace {

struct DpmStage {
    static constexpr int COLS = DXMI_MT_COLS, T = DXMI_MT_T, T_NEXT = DXMI_MT_T_NEXT, FLAGS = DXMI_MT_FLAGS;
    static constexpr int FLAG_LAST = DXMI_MT_FLAG_LAST, HIST = 2;
    static constexpr bool XIN = false, CORR = false;

    struct StageCoef {
        float cx, w0, w1, w2, s, a, b;
        bool clip, noisy, rd[2];
    };

    static __device__ __forceinline__ StageCoef fill(const float* r, bool ok, int flags) {
        const float nan = __builtin_nanf("");
        StageCoef k;
        k.cx = ok ? r[DXMI_MT_CX] : nan, k.w0 = ok ? r[DXMI_MT_W0] : nan, k.a = ok ? r[DXMI_MT_A] : nan, k.b = ok ? r[DXMI_MT_B] : nan;
        k.w1 = ok ? r[DXMI_MT_W1] : 0.f, k.w2 = ok ? r[DXMI_MT_W2] : 0.f, k.s = ok ? r[DXMI_MT_S] : 0.f;   // a poisoned launch reads no slot
        k.clip = (flags & DXMI_MT_FLAG_CLIP) != 0;
        k.rd[0] = k.w1 != 0.f, k.rd[1] = k.w2 != 0.f;        // a zero weight: the slot is not read
        return k;
    }

    // one element of the transition -> x'; d = (D_{k-1}, D_{k-2}); *d0 = the data prediction of this evaluation (clamped in the
    // clip form)
    static __device__ __forceinline__ float stage_elem(const StageCoef& k, float x, float e, const float* d, float z, float* d0) {
        const float pa = k.a * x, pb = k.b * e;
        float D = pa - pb;
        if (k.clip) D = clamp1(D);
        *d0 = D;
        const float px = k.cx * x, p0 = k.w0 * D;
        float acc = px + p0;
        if (k.rd[0]) { const float p1 = k.w1 * d[0]; acc = acc + p1; }
        if (k.rd[1]) { const float p2 = k.w2 * d[1]; acc = acc + p2; }
        if (k.noisy) { const float pz = k.s * z; acc = acc + pz; }
        return acc;
    }
};

template <bool ALIGNED>
__global__ __launch_bounds__(STAGE_BLOCK) void dpm_stage_kernel(int first, const float* __restrict__ tab, int rows,
                                                                const int32_t* __restrict__ ctl, int row_v, uint32_t draw_v,
                                                                uint32_t k0_v, uint32_t k1_v, float* x, const float* __restrict__ eps,
                                                                const float* __restrict__ z, const int64_t* __restrict__ sample_index,
                                                                float* hist, float* __restrict__ t_out, float* __restrict__ out,
                                                                float* __restrict__ pred, int N, int CHW) {
    stage_body<DpmStage, ALIGNED>(first, tab, rows, ctl, row_v, draw_v, k0_v, k1_v, x, eps, z, sample_index, hist, t_out, out, pred, N,
                                  CHW);
}

}  // namespace

extern "C" int dxmi_dpm_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw,
                              uint64_t seed, float* x, const float* eps, const float* z, const int64_t* sample_index, float* hist,
                              float* t_out, float* out, float* pred_xstart, int32_t N, int32_t CHW, void* stream) {
    const char* fn = "dxmi_dpm_stage";
    const bool first = mode == DXMI_DPM_FIRST;
    if (int e = stage_check_launch(fn, mode, first || mode == DXMI_DPM_STEP, first, tab, rows, ctl, row, x, eps, t_out, out, N, CHW))
        return e;
    if (!first) {
        DXMI_CHECK_ARG(hist, "%s: null pointer (a transition needs the history [3][N][CHW])", fn);
        if (int e = stage_check_tensors(fn, x, eps, z, sample_index, hist, out, pred_xstart)) return e;
    }
    return stage_launch(fn, dpm_stage_kernel<true>, dpm_stage_kernel<false>, first, N, CHW, stream, (int)first, tab, (int)rows, ctl,
                        (int)row, draw, (uint32_t)seed, (uint32_t)(seed >> 32), x, eps, z, sample_index, hist, t_out, out, pred_xstart,
                        (int)N, (int)CHW);
}
