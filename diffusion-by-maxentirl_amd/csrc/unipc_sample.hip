// UniPC sampling of the DDPM teacher (models/DxMI/unipc_sample.py; Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework
// for Fast Sampling of Diffusion Models", arXiv:2302.04867: the multistep data-prediction predictor UniP with the corrector UniC,
// orders 1-3, ODE only).
//   dxmi_unipc_stage  turns the evaluation it follows into the data prediction D_k, re-does the step that led to this evaluation with
//                     D_k as a node at its end point (the corrector, from the corrected state xc), predicts the next state from the
//                     result and files D_k in the history: the stage launch of stage_common.h (the control block, the table row, the
//                     history ring, the second state stream, the loop and the tail are there) with the element below and three
//                     history reads.  The solver adds no noise: the entry has no z and no sample_index.
// The history is fp32 [4][N][CHW]: D_k goes to slot k % 4, D_{k-1}, D_{k-2} and D_{k-3} come from slots (k + 3) % 4, (k + 2) % 4 and
// (k + 1) % 4, derived in the launch from the row number.  Slot j is read only if one of its two weights (predictor w_j, corrector
// cv_j on a corrected row) is not 0: 0 * NaN would be NaN.  xc is read only on a row with FLAG_CORR; xc == NULL: no corrected state,
// every row runs uncorrected whatever its flags, and the launch is dxmi_dpm_stage's ODE row on a ring of four.
// Per element, one rounding per operation (stage_common.h turns contraction off for everything below it), in this order:
//   1. D0 = a x - b eps;  D0 = clamp(D0, -1, 1) with FLAG_CLIP (NaN passes)
//   2. corrected row: b = ccx xc;  b += cv0 D0;  b += cv1 D1;  b += cv2 D2 if cv2 != 0;  b += cv3 D3 if cv3 != 0.  Otherwise b = x
//   3. acc = cx b + w0 D0;  acc += w1 D1 if w1 != 0;  acc += w2 D2 if w2 != 0
//   4. x = acc, xc = b, slot k % 4 = D0
// An order-3 corrected row moves 36 bytes per element (reads x, eps, xc, D1, D2, D3; writes x, xc, one slot).  HBM-bound.
#include "stage_common.h"

namespace {

struct UnipcStage {
    static constexpr int COLS = DXMI_UT_COLS, T = DXMI_UT_T, T_NEXT = DXMI_UT_T_NEXT, FLAGS = DXMI_UT_FLAGS;
    static constexpr int FLAG_LAST = DXMI_UT_FLAG_LAST, HIST = 3;
    static constexpr bool XIN = false, CORR = true;

    struct StageCoef {
        float cx, w0, w1, w2, ccx, cv0, cv1, cv2, cv3, s, a, b;
        bool clip, noisy, corr, rd[3];
    };

    static __device__ __forceinline__ StageCoef fill(const float* r, bool ok, int flags) {
        const float nan = __builtin_nanf("");
        StageCoef k;
        k.cx = ok ? r[DXMI_UT_CX] : nan, k.w0 = ok ? r[DXMI_UT_W0] : nan, k.a = ok ? r[DXMI_UT_A] : nan, k.b = ok ? r[DXMI_UT_B] : nan;
        k.w1 = ok ? r[DXMI_UT_W1] : 0.f, k.w2 = ok ? r[DXMI_UT_W2] : 0.f, k.s = 0.f;      // a poisoned launch reads no slot and no xc
        k.corr = (flags & DXMI_UT_FLAG_CORR) != 0;
        k.ccx = k.corr ? r[DXMI_UT_CCX] : 0.f, k.cv0 = k.corr ? r[DXMI_UT_CV0] : 0.f, k.cv1 = k.corr ? r[DXMI_UT_CV1] : 0.f;
        k.cv2 = k.corr ? r[DXMI_UT_CV2] : 0.f, k.cv3 = k.corr ? r[DXMI_UT_CV3] : 0.f;
        k.clip = (flags & DXMI_UT_FLAG_CLIP) != 0;
        k.rd[0] = k.w1 != 0.f || k.cv1 != 0.f, k.rd[1] = k.w2 != 0.f || k.cv2 != 0.f, k.rd[2] = k.cv3 != 0.f;
        return k;
    }

    // no corrected state was given: the row runs uncorrected, and reads what its predictor alone reads
    static __device__ __forceinline__ void uncorrect(StageCoef& k) {
        k.corr = false, k.cv1 = 0.f, k.cv2 = 0.f, k.cv3 = 0.f;
        k.rd[0] = k.w1 != 0.f, k.rd[1] = k.w2 != 0.f, k.rd[2] = false;
    }

    // one element of the transition -> x'; d = (D_{k-1}, D_{k-2}, D_{k-3}); xc: the corrected state of the evaluation before (read
    // on a corrected row); *d0 = the data prediction of this evaluation (clamped in the clip form), *bo = the state the predictor
    // starts from: the corrected x_k, or x
    static __device__ __forceinline__ float stage_elem(const StageCoef& k, float x, float e, const float* d, float xc, float* d0,
                                                       float* bo) {
        const float pa = k.a * x, pb = k.b * e;
        float D = pa - pb;
        if (k.clip) D = clamp1(D);
        *d0 = D;
        float b = x;
        if (k.corr) {
            const float c0 = k.cv0 * D, c1 = k.cv1 * d[0];
            b = k.ccx * xc;
            b = b + c0;
            b = b + c1;
            if (k.cv2 != 0.f) { const float c2 = k.cv2 * d[1]; b = b + c2; }
            if (k.cv3 != 0.f) { const float c3 = k.cv3 * d[2]; b = b + c3; }
        }
        *bo = b;
        const float px = k.cx * b, p0 = k.w0 * D;
        float acc = px + p0;
        if (k.w1 != 0.f) { const float p1 = k.w1 * d[0]; acc = acc + p1; }
        if (k.w2 != 0.f) { const float p2 = k.w2 * d[1]; acc = acc + p2; }
        return acc;
    }
};

template <bool ALIGNED>
__global__ __launch_bounds__(STAGE_BLOCK) void unipc_stage_kernel(int first, const float* __restrict__ tab, int rows,
                                                                  const int32_t* __restrict__ ctl, int row_v, float* x, float* xc,
                                                                  const float* __restrict__ eps, float* hist, float* __restrict__ t_out,
                                                                  float* __restrict__ out, float* __restrict__ pred, int N, int CHW) {
    stage_body<UnipcStage, ALIGNED>(first, tab, rows, ctl, row_v, 0u, 0u, 0u, x, eps, nullptr, nullptr, hist, t_out, out, pred, N, CHW,
                                    nullptr, xc);
}

}  // namespace

extern "C" int dxmi_unipc_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, float* x, float* xc,
                                const float* eps, float* hist, float* t_out, float* out, float* pred_xstart, int32_t N, int32_t CHW,
                                void* stream) {
    const char* fn = "dxmi_unipc_stage";
    const bool first = mode == DXMI_UNIPC_FIRST;
    if (int e = stage_check_launch(fn, mode, first || mode == DXMI_UNIPC_STEP, first, tab, rows, ctl, row, x, eps, t_out, out, N, CHW))
        return e;
    if (!first) {
        DXMI_CHECK_ARG(hist, "%s: null pointer (a transition needs the history [4][N][CHW])", fn);
        if (int e = stage_check_tensors(fn, x, eps, nullptr, nullptr, hist, out, pred_xstart)) return e;
        DXMI_CHECK_ARG((((uintptr_t)xc) & 15) == 0, "%s: tensors must be 16-byte aligned (xc)", fn);
        DXMI_CHECK_ARG(xc != x, "%s: xc and x are two states: they may not be one tensor", fn);
    }
    return stage_launch(fn, unipc_stage_kernel<true>, unipc_stage_kernel<false>, first, N, CHW, stream, (int)first, tab, (int)rows, ctl,
                        (int)row, x, xc, eps, hist, t_out, out, pred_xstart, (int)N, (int)CHW);
}
