// DPM-Solver++ sampling of the EDM nets (models/cm/dpm_sample.py; Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of
// Diffusion Probabilistic Models", Algorithm 2 and its SDE variant, in the EDM parametrisation x = x_0 + sigma e: alpha = 1,
// lambda = -ln sigma).
//   dxmi_edm_dpm_stage  turns the evaluation it follows into the data prediction D_k by the Karras preconditioning, files it in the
//                       history, finishes the multistep transition and writes the next evaluation's preconditioned input and time:
//                       the stage launch of stage_common.h (the control block, the table row, the noise, the history ring, the loop,
//                       the tail and the second output stream are there) with the element below and two history reads.
// The history is fp32 [3][N][CHW], addressed as dxmi_dpm_stage addresses it: D_k goes to slot k % 3, D_{k-1} and D_{k-2} come from
// slots (k + 2) % 3 and (k + 1) % 3.  A weight that is exactly 0 means its slot is NOT read (0 * NaN would be NaN).
// Per element, one rounding per operation (stage_common.h turns contraction off for everything below it), in this order:
//   1. D0 = c_out F + c_skip x  (karras_stage_kernel's order);  D0 = clamp(D0, -1, 1) with FLAG_CLIP (NaN passes)
//   2. acc = cx x + w0 D0
//   3. acc += w1 D1    if w1 != 0
//   4. acc += w2 D2    if w2 != 0
//   5. acc += s z      if s != 0
//   6. x' = acc;  x_in = c_in_next x' on every row that is not last (the skeleton's second stream)
// An order-2 ODE row moves 24 bytes per element (reads x, F, D1; writes x, x_in, one slot).  HBM-bound.
#include "stage_common.h"

namespace {

struct EdmDpmStage {
    static constexpr int COLS = DXMI_ET_COLS, T = DXMI_ET_T, T_NEXT = DXMI_ET_T_NEXT, FLAGS = DXMI_ET_FLAGS;
    static constexpr int FLAG_LAST = DXMI_ET_FLAG_LAST, HIST = 2;
    static constexpr bool XIN = true, CORR = false;
    static constexpr int CIN = DXMI_ET_CIN, CIN_NEXT = DXMI_ET_CIN_NEXT, XSCALE = DXMI_ET_XSCALE;

    struct StageCoef {
        float cx, w0, w1, w2, s, c_skip, c_out;
        bool clip, noisy, rd[2];
    };

    static __device__ __forceinline__ StageCoef fill(const float* r, bool ok, int flags) {
        const float nan = __builtin_nanf("");
        StageCoef k;
        k.cx = ok ? r[DXMI_ET_CX] : nan, k.w0 = ok ? r[DXMI_ET_W0] : nan;
        k.c_skip = ok ? r[DXMI_ET_CSKIP] : nan, k.c_out = ok ? r[DXMI_ET_COUT] : nan;
        k.w1 = ok ? r[DXMI_ET_W1] : 0.f, k.w2 = ok ? r[DXMI_ET_W2] : 0.f, k.s = ok ? r[DXMI_ET_S] : 0.f;   // a poisoned launch reads no slot
        k.clip = (flags & DXMI_ET_FLAG_CLIP) != 0;
        k.rd[0] = k.w1 != 0.f, k.rd[1] = k.w2 != 0.f;        // a zero weight: the slot is not read
        return k;
    }

    // one element of the transition -> x'; f: the network output; d = (D_{k-1}, D_{k-2}); *d0 = the data prediction of this
    // evaluation (clamped in the clip form)
    static __device__ __forceinline__ float stage_elem(const StageCoef& k, float x, float f, const float* d, float z, float* d0) {
        const float po = k.c_out * f, ps = k.c_skip * x;
        float D = po + ps;
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
__global__ __launch_bounds__(STAGE_BLOCK) void edm_dpm_stage_kernel(int first, const float* __restrict__ tab, int rows,
                                                                    const int32_t* __restrict__ ctl, int row_v, uint32_t draw_v,
                                                                    uint32_t k0_v, uint32_t k1_v, float* x,
                                                                    const float* __restrict__ model_out, const float* __restrict__ z,
                                                                    const int64_t* __restrict__ sample_index, float* hist,
                                                                    float* __restrict__ x_in, float* __restrict__ t_out,
                                                                    float* __restrict__ out, float* __restrict__ pred, int N, int CHW) {
    stage_body<EdmDpmStage, ALIGNED>(first, tab, rows, ctl, row_v, draw_v, k0_v, k1_v, x, model_out, z, sample_index, hist, t_out, out,
                                     pred, N, CHW, x_in);
}

}  // namespace

extern "C" int dxmi_edm_dpm_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw,
                                  uint64_t seed, float* x, const float* model_out, const float* z, const int64_t* sample_index,
                                  float* hist, float* x_in, float* t_out, float* out, float* pred_xstart, int32_t N, int32_t CHW,
                                  void* stream) {
    const char* fn = "dxmi_edm_dpm_stage";
    const bool first = mode == DXMI_EDM_DPM_FIRST;
    if (int e = stage_check_launch(fn, mode, first || mode == DXMI_EDM_DPM_STEP, first, tab, rows, ctl, row, x, model_out, t_out, out, N,
                                   CHW))
        return e;
    if (first) {
        DXMI_CHECK_ARG(x && x_in, "%s: null pointer (FIRST scales x and writes x_in)", fn);
        if (int e = stage_check_tensors(fn, x, nullptr, nullptr, nullptr, nullptr, x_in, nullptr)) return e;
    } else {
        DXMI_CHECK_ARG(hist, "%s: null pointer (a transition needs the history [3][N][CHW])", fn);
        // the table's last row is the one flagged last; through the control block the row is not known here
        DXMI_CHECK_ARG(x_in || (!ctl && row == rows - 1), "%s: null pointer (x_in: only the last row, given by value, writes none)", fn);
        if (int e = stage_check_tensors(fn, x, model_out, z, sample_index, hist, out, pred_xstart)) return e;
        DXMI_CHECK_ARG((((uintptr_t)x_in) & 15) == 0, "%s: tensors must be 16-byte aligned (x_in)", fn);
    }
    // FIRST moves every element too: the transition's grid
    return stage_launch(fn, edm_dpm_stage_kernel<true>, edm_dpm_stage_kernel<false>, false, N, CHW, stream, (int)first, tab, (int)rows,
                        ctl, (int)row, draw, (uint32_t)seed, (uint32_t)(seed >> 32), x, model_out, z, sample_index, hist, x_in, t_out,
                        out, pred_xstart, (int)N, (int)CHW);
}
