// DPM-Solver++ sampling of the DDPM teacher (models/DxMI/dpm_sample.py; Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided
// Sampling of Diffusion Probabilistic Models", Algorithm 2 and its SDE variant): ONE launch between two network evaluations.
//   dxmi_dpm_stage  turns the evaluation it follows into the data prediction D_k, files it in the history, finishes the multistep
//                   transition (x' in place), writes the next evaluation's time and, on the row flagged last, the clamped sample
// Every per-transition scalar is read from one fp32 table row built on the host, the last-step behaviour included, and the row
// number, the draw number and the seed can be read from a small device block: one captured launch serves every transition.
// The history is fp32 [3][N][CHW]: D_k goes to slot k % 3, D_{k-1} and D_{k-2} come from slots (k + 2) % 3 and (k + 1) % 3, all
// three derived here from the row number.  A weight that is exactly 0 means its slot is NOT read: the warm-up rows and the rows
// lower_order_final lowers never touch history that was never written (0 * NaN would be NaN).
// Per element, one rounding per operation (contraction off), in this order:
//   1. D0 = a x - b eps;  D0 = clamp(D0, -1, 1) with FLAG_CLIP (NaN passes)
//   2. acc = cx x + w0 D0
//   3. acc += w1 D1    if w1 != 0
//   4. acc += w2 D2    if w2 != 0
//   5. acc += s z      if s != 0
// The noise is either given or made here, from the counter layout of dxmi_randn_indexed (philox_normal.h: the same bits).
// HBM-bound (one workgroup row per image, 16 bytes per lane, four vectors in flight per stream).  No LDS, no atomics, plain
// vector stores.  A table row outside [0, rows) gives NaN; nothing outside the table is read and no history slot is read.
#include "common.h"
#include "philox_normal.h"

#pragma clang fp contract(off)

namespace {

constexpr int MS_BLOCK = 256;
constexpr int MS_UNROLL = 4;      // f32x4 per stream per lane in flight

// rows whose base is not 16-byte aligned (CHW % 4 != 0) go through this type: the widest access the stated alignment allows
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }   // NaN passes, as torch.clamp

struct StageCoef {
    float cx, w0, w1, w2, s, a, b;
    bool clip, r1, r2, noisy;
};

// one element of the transition -> x'; *d0 = the data prediction of this evaluation (clamped in the clip form)
__device__ __forceinline__ float stage_elem(const StageCoef& k, float x, float e, float d1, float d2, float z, float* d0) {
    const float pa = k.a * x, pb = k.b * e;
    float D = pa - pb;
    if (k.clip) D = clamp1(D);
    *d0 = D;
    const float px = k.cx * x, p0 = k.w0 * D;
    float acc = px + p0;
    if (k.r1) { const float p1 = k.w1 * d1; acc = acc + p1; }
    if (k.r2) { const float p2 = k.w2 * d2; acc = acc + p2; }
    if (k.noisy) { const float pz = k.s * z; acc = acc + pz; }
    return acc;
}

template <bool ALIGNED>
__device__ __forceinline__ f32x4 load4(const float* p) {
    if (ALIGNED) return *reinterpret_cast<const f32x4*>(p);
    return *reinterpret_cast<const f32x4_a4*>(p);
}

template <bool ALIGNED>
__device__ __forceinline__ void store4(float* p, f32x4 v) {
    if (ALIGNED) *reinterpret_cast<f32x4*>(p) = v;
    else *reinterpret_cast<f32x4_a4*>(p) = v;
}

template <bool ALIGNED>
__global__ __launch_bounds__(MS_BLOCK) void dpm_stage_kernel(int first, const float* __restrict__ tab, int rows,
                                                             const int32_t* __restrict__ ctl, int row_v, uint32_t draw_v,
                                                             uint32_t k0_v, uint32_t k1_v, float* x, const float* __restrict__ eps,
                                                             const float* __restrict__ z, const int64_t* __restrict__ sample_index,
                                                             float* hist, float* __restrict__ t_out, float* __restrict__ out,
                                                             float* __restrict__ pred, int N, int CHW) {
    const int n = blockIdx.y;
    const int row = ctl ? ctl[0] : row_v;
    const uint32_t draw = ctl ? (uint32_t)ctl[1] : draw_v;
    const uint32_t k0 = ctl ? (uint32_t)ctl[2] : k0_v, k1 = ctl ? (uint32_t)ctl[3] : k1_v;
    const bool ok = row >= 0 && row < rows;
    const float* r = tab + (size_t)(ok ? row : 0) * DXMI_MT_COLS;      // the read is clamped, the values are not
    const float nan = __builtin_nanf("");
    if (first) {
        if (blockIdx.x == 0 && threadIdx.x == 0) t_out[n] = ok ? r[DXMI_MT_T] : nan;
        return;
    }
    const int flags = ok ? (int)r[DXMI_MT_FLAGS] : 0;
    StageCoef k;
    k.cx = ok ? r[DXMI_MT_CX] : nan, k.w0 = ok ? r[DXMI_MT_W0] : nan, k.a = ok ? r[DXMI_MT_A] : nan, k.b = ok ? r[DXMI_MT_B] : nan;
    k.w1 = ok ? r[DXMI_MT_W1] : 0.f, k.w2 = ok ? r[DXMI_MT_W2] : 0.f, k.s = ok ? r[DXMI_MT_S] : 0.f;   // a poisoned launch reads no slot
    k.clip = (flags & DXMI_MT_FLAG_CLIP) != 0;
    k.r1 = k.w1 != 0.f, k.r2 = k.w2 != 0.f;                  // a zero weight: the slot is not read
    const bool fused = !z && sample_index;
    k.noisy = k.s != 0.f && (z || fused);                    // rows with s == 0 touch neither z nor the generator
    const bool last = !ok || (flags & DXMI_MT_FLAG_LAST) != 0;          // a poisoned launch poisons the sample too
    if (blockIdx.x == 0 && threadIdx.x == 0) t_out[n] = ok ? r[DXMI_MT_T_NEXT] : nan;
    uint32_t i_lo = 0, i_hi = 0;
    if (fused && k.noisy) {
        const uint64_t index = (uint64_t)sample_index[n];
        i_lo = (uint32_t)index, i_hi = (uint32_t)(index >> 32);
    }
    // the history slots of this row: D_k -> k % 3, D_{k-1} <- (k - 1) % 3, D_{k-2} <- (k - 2) % 3
    const int s0 = ok ? row % 3 : 0;
    const size_t slot = (size_t)N * CHW, base = (size_t)n * CHW;
    float* h0 = hist + (size_t)s0 * slot;
    const float* h1 = hist + (size_t)((s0 + 2) % 3) * slot;
    const float* h2 = hist + (size_t)((s0 + 1) % 3) * slot;
    const int n4 = CHW / 4, rem = CHW % 4;
    for (int i0 = blockIdx.x * MS_BLOCK * MS_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * MS_BLOCK * MS_UNROLL) {
        f32x4 xv[MS_UNROLL], ev[MS_UNROLL], av[MS_UNROLL], bv[MS_UNROLL], zv[MS_UNROLL];
#pragma unroll
        for (int u = 0; u < MS_UNROLL; ++u) {
            const int i = i0 + u * MS_BLOCK;
            if (i < n4) {
                const size_t o = base + (size_t)i * 4;
                xv[u] = load4<ALIGNED>(x + o);
                ev[u] = load4<ALIGNED>(eps + o);
                if (k.r1) av[u] = load4<ALIGNED>(h1 + o);
                if (k.r2) bv[u] = load4<ALIGNED>(h2 + o);
                if (k.noisy && !fused) zv[u] = load4<ALIGNED>(z + o);
            }
        }
#pragma unroll
        for (int u = 0; u < MS_UNROLL; ++u) {
            const int i = i0 + u * MS_BLOCK;
            if (i >= n4) continue;
            const size_t o = base + (size_t)i * 4;
            if (k.noisy && fused) zv[u] = normals(philox4x32_10((uint32_t)i, draw, i_lo, i_hi, k0, k1));
            f32x4 xn, dv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float d;
                xn[e] = stage_elem(k, xv[u][e], ev[u][e], k.r1 ? av[u][e] : 0.f, k.r2 ? bv[u][e] : 0.f, k.noisy ? zv[u][e] : 0.f, &d);
                dv[e] = d;
            }
            store4<ALIGNED>(x + o, xn);
            store4<ALIGNED>(h0 + o, dv);
            if (pred) store4<ALIGNED>(pred + o, dv);
            if (last) {
#pragma unroll
                for (int e = 0; e < 4; ++e) xn[e] = clamp1(xn[e]);
                store4<ALIGNED>(out + o, xn);
            }
        }
    }
    if (rem && blockIdx.x == 0 && threadIdx.x == 0) {        // the tail: the first `rem` values of block n4, one element per access
        f32x4 zt;
        zt[0] = zt[1] = zt[2] = zt[3] = 0.f;
        if (k.noisy && fused) zt = normals(philox4x32_10((uint32_t)n4, draw, i_lo, i_hi, k0, k1));
        for (int e = 0; e < rem; ++e) {
            const size_t o = base + (size_t)n4 * 4 + e;
            if (k.noisy && !fused) zt[e] = z[o];
            float d;
            const float xn = stage_elem(k, x[o], eps[o], k.r1 ? h1[o] : 0.f, k.r2 ? h2[o] : 0.f, zt[e], &d);
            x[o] = xn;
            h0[o] = d;
            if (pred) pred[o] = d;
            if (last) out[o] = clamp1(xn);
        }
    }
}

}  // namespace

extern "C" int dxmi_dpm_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw,
                              uint64_t seed, float* x, const float* eps, const float* z, const int64_t* sample_index, float* hist,
                              float* t_out, float* out, float* pred_xstart, int32_t N, int32_t CHW, void* stream) {
    const char* fn = "dxmi_dpm_stage";
    DXMI_CHECK_ARG(mode == DXMI_DPM_FIRST || mode == DXMI_DPM_STEP, "%s: unknown mode %d", fn, mode);
    DXMI_CHECK_ARG(tab && t_out, "%s: null pointer (table or t_out)", fn);
    DXMI_CHECK_ARG(N > 0 && N <= 65535, "%s: N (%d) must be in [1, 65535]", fn, N);
    DXMI_CHECK_ARG(CHW > 0, "%s: CHW (%d) must be positive", fn, CHW);
    DXMI_CHECK_ARG(rows >= 1, "%s: the table needs at least one row, got %d", fn, rows);
    DXMI_CHECK_ARG(ctl || (row >= 0 && row < rows), "%s: row (%d) outside the table's [0, %d)", fn, row, rows);
    DXMI_CHECK_ARG((((uintptr_t)ctl) & 3) == 0 && (((uintptr_t)tab) & 3) == 0 && (((uintptr_t)t_out) & 3) == 0,
                   "%s: the control block, the table and t_out must be 4-byte aligned", fn);
    const bool first = mode == DXMI_DPM_FIRST;
    if (!first) {
        DXMI_CHECK_ARG(x && eps && out, "%s: null pointer (x, eps or out)", fn);
        DXMI_CHECK_ARG(hist, "%s: null pointer (a transition needs the history [3][N][CHW])", fn);
        DXMI_CHECK_ARG(!(z && sample_index), "%s: noise is either given (z) or made here (sample_index), not both", fn);
        DXMI_CHECK_ARG(((((uintptr_t)x) | ((uintptr_t)eps) | ((uintptr_t)z) | ((uintptr_t)hist) | ((uintptr_t)out) |
                         ((uintptr_t)pred_xstart)) & 15) == 0 && (((uintptr_t)sample_index) & 7) == 0,
                       "%s: tensors must be 16-byte aligned (sample_index 8-byte)", fn);
    }
    const int chunks = first ? 1 : (CHW / 4 + MS_BLOCK * MS_UNROLL - 1) / (MS_BLOCK * MS_UNROLL);
    const dim3 grid(chunks < 1 ? 1 : (chunks < 64 ? chunks : 64), N);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (CHW % 4 == 0)
        hipLaunchKernelGGL(dpm_stage_kernel<true>, grid, dim3(MS_BLOCK), 0, (hipStream_t)stream, (int)first, tab, (int)rows, ctl,
                           (int)row, draw, k0, k1, x, eps, z, sample_index, hist, t_out, out, pred_xstart, (int)N, (int)CHW);
    else
        hipLaunchKernelGGL(dpm_stage_kernel<false>, grid, dim3(MS_BLOCK), 0, (hipStream_t)stream, (int)first, tab, (int)rows, ctl,
                           (int)row, draw, k0, k1, x, eps, z, sample_index, hist, t_out, out, pred_xstart, (int)N, (int)CHW);
    DXMI_CHECK_LAUNCH(fn);
    return DXMI_OK;
}
