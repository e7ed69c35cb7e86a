// Ancestral / DDIM sampling of the DDPM teacher (models/DxMI/ddpm_sample.py; Ho et al. 2020, "Denoising Diffusion Probabilistic
// Models", Algorithm 2 and eq. 7; Song et al. 2021, "Denoising Diffusion Implicit Models", eq. 12 and 16): ONE launch between two
// network evaluations.
//   dxmi_ddpm_stage  finishes the transition the evaluation it follows belongs to (x' in place), writes the next evaluation's time
//                    and, on the row flagged last, the clamped sample
// Every per-transition scalar is read from one fp32 table row built on the host, the last-step behaviour included, and the row
// number, the draw number and the seed can be read from a small device block: one captured launch serves every transition.
// The noise is either given or made here, from the counter layout of dxmi_randn_indexed (philox_normal.h: the same bits).
// HBM-bound with explicit noise (one workgroup row per image, 16 bytes per lane, several loads in flight per wave); with fused noise
// the Philox rounds and logf / sinf / cosf make it VALU-bound, which buys one launch and one write plus read of z per transition.
// No LDS, no atomics, plain vector stores.  A table row outside [0, rows) gives NaN; nothing outside the table is read.
#include "common.h"
#include "philox_normal.h"

// one rounding per operation; the one explicit fused multiply-add is the linear form's, as in dxmi_var_step_fwd (assoc 1)
#pragma clang fp contract(off)

namespace {

constexpr int DS_BLOCK = 256;
constexpr int DS_UNROLL = 4;      // f32x4 per stream per lane in flight

// rows whose base is not 16-byte aligned (CHW % 4 != 0) go through this type: the widest access the stated alignment allows
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }   // NaN passes, as torch.clamp

struct StageCoef {
    float xm, c, s, a, b, q, r, c0, c1;
    bool clip, noisy;
};

// one element of the transition -> x'; *pred = the predicted x_0 (clamped in the clip form)
__device__ __forceinline__ float stage_elem(const StageCoef& k, float x, float e, float z, float* pred) {
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
    // x *= xm; x += control + sigma z.  dxmi_var_step_fwd (assoc 1), whose file leaves contraction on, evaluates control + sigma z as
    // ONE fused multiply-add on rounded xs and control; it is written out here so that the two launches agree bit for bit.
    return k.noisy ? xs + __builtin_fmaf(k.s, z, ct) : xs + ct;
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
__global__ __launch_bounds__(DS_BLOCK) void ddpm_stage_kernel(int first, const float* __restrict__ tab, int rows,
                                                              const int32_t* __restrict__ ctl, int row_v, uint32_t draw_v,
                                                              uint32_t k0_v, uint32_t k1_v, float* x, const float* __restrict__ eps,
                                                              const float* __restrict__ z, const int64_t* __restrict__ sample_index,
                                                              float* __restrict__ t_out, float* __restrict__ out,
                                                              float* __restrict__ pred, int CHW) {
    const int n = blockIdx.y;
    const int row = ctl ? ctl[0] : row_v;
    const uint32_t draw = ctl ? (uint32_t)ctl[1] : draw_v;
    const uint32_t k0 = ctl ? (uint32_t)ctl[2] : k0_v, k1 = ctl ? (uint32_t)ctl[3] : k1_v;
    const bool ok = row >= 0 && row < rows;
    const float* r = tab + (size_t)(ok ? row : 0) * DXMI_DT_COLS;      // the read is clamped, the values are not
    const float nan = __builtin_nanf("");
    if (first) {
        if (blockIdx.x == 0 && threadIdx.x == 0) t_out[n] = ok ? r[DXMI_DT_T] : nan;
        return;
    }
    const int flags = ok ? (int)r[DXMI_DT_FLAGS] : 0;
    StageCoef k;
    k.xm = ok ? r[DXMI_DT_XM] : nan, k.c = ok ? r[DXMI_DT_C] : nan, k.s = ok ? r[DXMI_DT_S] : 0.f;
    k.a = ok ? r[DXMI_DT_A] : nan, k.b = ok ? r[DXMI_DT_B] : nan, k.q = ok ? r[DXMI_DT_Q] : nan, k.r = ok ? r[DXMI_DT_R] : nan;
    k.c0 = ok ? r[DXMI_DT_C0] : nan, k.c1 = ok ? r[DXMI_DT_C1] : nan;
    k.clip = (flags & DXMI_DT_FLAG_CLIP) != 0;
    const bool fused = !z && sample_index;
    k.noisy = k.s != 0.f && (z || fused);                    // rows with s == 0 touch neither z nor the generator
    const bool last = !ok || (flags & DXMI_DT_FLAG_LAST) != 0;          // a poisoned launch poisons the sample too
    if (blockIdx.x == 0 && threadIdx.x == 0) t_out[n] = ok ? r[DXMI_DT_T_NEXT] : nan;
    uint32_t i_lo = 0, i_hi = 0;
    if (fused && k.noisy) {
        const uint64_t index = (uint64_t)sample_index[n];
        i_lo = (uint32_t)index, i_hi = (uint32_t)(index >> 32);
    }
    const size_t base = (size_t)n * CHW;
    const int n4 = CHW / 4, rem = CHW % 4;
    for (int i0 = blockIdx.x * DS_BLOCK * DS_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * DS_BLOCK * DS_UNROLL) {
        f32x4 xv[DS_UNROLL], ev[DS_UNROLL], zv[DS_UNROLL];
#pragma unroll
        for (int u = 0; u < DS_UNROLL; ++u) {
            const int i = i0 + u * DS_BLOCK;
            if (i < n4) {
                const size_t o = base + (size_t)i * 4;
                xv[u] = load4<ALIGNED>(x + o);
                ev[u] = load4<ALIGNED>(eps + o);
                if (k.noisy && !fused) zv[u] = load4<ALIGNED>(z + o);
            }
        }
#pragma unroll
        for (int u = 0; u < DS_UNROLL; ++u) {
            const int i = i0 + u * DS_BLOCK;
            if (i >= n4) continue;
            const size_t o = base + (size_t)i * 4;
            if (k.noisy && fused) zv[u] = normals(philox4x32_10((uint32_t)i, draw, i_lo, i_hi, k0, k1));
            f32x4 xn, pv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float p;
                xn[e] = stage_elem(k, xv[u][e], ev[u][e], k.noisy ? zv[u][e] : 0.f, &p);
                pv[e] = p;
            }
            store4<ALIGNED>(x + o, xn);
            if (pred) store4<ALIGNED>(pred + o, pv);
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
            float p;
            const float xn = stage_elem(k, x[o], eps[o], zt[e], &p);
            x[o] = xn;
            if (pred) pred[o] = p;
            if (last) out[o] = clamp1(xn);
        }
    }
}

}  // namespace

extern "C" int dxmi_ddpm_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw,
                               uint64_t seed, float* x, const float* eps, const float* z, const int64_t* sample_index, float* t_out,
                               float* out, float* pred_xstart, int32_t N, int32_t CHW, void* stream) {
    const char* fn = "dxmi_ddpm_stage";
    DXMI_CHECK_ARG(mode == DXMI_DDPM_FIRST || mode == DXMI_DDPM_STEP, "%s: unknown mode %d", fn, mode);
    DXMI_CHECK_ARG(tab && t_out, "%s: null pointer (table or t_out)", fn);
    DXMI_CHECK_ARG(N > 0 && N <= 65535, "%s: N (%d) must be in [1, 65535]", fn, N);
    DXMI_CHECK_ARG(CHW > 0, "%s: CHW (%d) must be positive", fn, CHW);
    DXMI_CHECK_ARG(rows >= 1, "%s: the table needs at least one row, got %d", fn, rows);
    DXMI_CHECK_ARG(ctl || (row >= 0 && row < rows), "%s: row (%d) outside the table's [0, %d)", fn, row, rows);
    DXMI_CHECK_ARG((((uintptr_t)ctl) & 3) == 0 && (((uintptr_t)tab) & 3) == 0 && (((uintptr_t)t_out) & 3) == 0,
                   "%s: the control block, the table and t_out must be 4-byte aligned", fn);
    const bool first = mode == DXMI_DDPM_FIRST;
    if (!first) {
        DXMI_CHECK_ARG(x && eps && out, "%s: null pointer (x, eps or out)", fn);
        DXMI_CHECK_ARG(!(z && sample_index), "%s: noise is either given (z) or made here (sample_index), not both", fn);
        DXMI_CHECK_ARG(((((uintptr_t)x) | ((uintptr_t)eps) | ((uintptr_t)z) | ((uintptr_t)out) | ((uintptr_t)pred_xstart)) & 15) == 0 &&
                       (((uintptr_t)sample_index) & 7) == 0, "%s: tensors must be 16-byte aligned (sample_index 8-byte)", fn);
    }
    const int chunks = first ? 1 : (CHW / 4 + DS_BLOCK * DS_UNROLL - 1) / (DS_BLOCK * DS_UNROLL);
    const dim3 grid(chunks < 1 ? 1 : (chunks < 64 ? chunks : 64), N);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (CHW % 4 == 0)
        hipLaunchKernelGGL(ddpm_stage_kernel<true>, grid, dim3(DS_BLOCK), 0, (hipStream_t)stream, (int)first, tab, (int)rows, ctl,
                           (int)row, draw, k0, k1, x, eps, z, sample_index, t_out, out, pred_xstart, (int)CHW);
    else
        hipLaunchKernelGGL(ddpm_stage_kernel<false>, grid, dim3(DS_BLOCK), 0, (hipStream_t)stream, (int)first, tab, (int)rows, ctl,
                           (int)row, draw, k0, k1, x, eps, z, sample_index, t_out, out, pred_xstart, (int)CHW);
    DXMI_CHECK_LAUNCH(fn);
    return DXMI_OK;
}
