// The stage launch of the DDPM teacher's samplers (csrc/ddpm_sample.hip, csrc/dpm_sample.hip, csrc/unipc_sample.hip) and of the EDM
// nets' multistep solvers (csrc/edm_dpm_sample.hip, csrc/edm_unipc_sample.hip), written once: ONE launch between two
// network evaluations finishes a transition in place (x'), writes the next evaluation's time and, on the row flagged last, the
// clamped sample.  Every per-transition scalar is read from one fp32 table row built on the host, the last-step behaviour
// included, and the row number, the draw number and the seed can be read from a small device block: one captured launch serves
// every transition.  The noise is either given or made here, from the counter layout of dxmi_randn_indexed (philox_normal.h: the
// same bits).  One workgroup row per image, 16 bytes per lane, STAGE_UNROLL vectors in flight per stream; no LDS, no atomics, plain
// vector stores.  A table row outside [0, rows) gives NaN; nothing outside the table is read and no history slot is read.
//
// A sampler supplies a policy P, resolved at compile time (nothing here asks which sampler it serves):
//   COLS, T, T_NEXT, FLAGS, FLAG_LAST   the table's row length, the shared columns and the last-row flag
//   HIST                                how many earlier predictions an element reads (0, 2 or 3), kept in a ring of HIST + 1 slots
//                                       fp32 [HIST + 1][N][CHW]: this row's goes to slot row % (HIST + 1), the one j + 1 rows back
//                                       comes from slot (row - 1 - j) % (HIST + 1).  HIST == 0: no pointer, load or register
//   XIN                                 whether the launch has a second output stream: the next evaluation's preconditioned input
//                                       x_in = K[CIN_NEXT] x', written on every row that is not last (and, NaN, on a poisoned one); the
//                                       policy then names the columns CIN, CIN_NEXT and XSCALE too, and FIRST scales x in place by
//                                       K[XSCALE] and writes x_in = K[CIN] x next to t_out.  false: no pointer, product or store
//   CORR                                whether the launch carries a second in-place state stream xc (UniPC's corrected state): on a
//                                       row the policy marks corrected (k.corr) xc is read, on every row b, the state the step
//                                       starts from, is written to it (NaN on a poisoned row).  xc == NULL: P::uncorrect(k) clears
//                                       k.corr and the reads only the corrector asked for; xc is then neither read nor written.  The
//                                       element is then stage_elem(k, x, e, d, xc, &pred, &b).  false: no pointer, load or register
//   StageCoef                           the row's scalars; members s (the noise scale) and noisy, and with HIST rd[HIST]: whether
//                                       slot j is read (a slot never written holds anything, and 0 * NaN would be NaN)
//   fill(r, ok, flags)                  StageCoef from the row r; !ok: the row is poisoned, what must be NaN and what must be 0
//   stage_elem(k, x, e, d, z, &pred)    one element -> x'; d[j]: the prediction j + 1 rows back (0 if not read), *pred: this row's
// philox_normal.h (which turns contraction off for its own functions) comes before the pragma, as in randn_indexed.hip; every
// operation of a transition, the policy's included, is compiled below the pragma: one rounding per operation, and a fused
// multiply-add only where one is written out.  A sampler's file includes this header before any code of its own.
#pragma once
#include "common.h"
#include "philox_normal.h"

#pragma clang fp contract(off)

namespace {

constexpr int STAGE_BLOCK = 256;
constexpr int STAGE_UNROLL = 4;      // f32x4 per stream per lane in flight

// rows whose base is not 16-byte aligned (CHW % 4 != 0) go through this type: the widest access the stated alignment allows
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }   // NaN passes, as torch.clamp

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

// FIRST of a policy with XIN: x *= K[XSCALE] in place (x_T = randn * sigma_max), x_in = K[CIN] x; a poisoned row gives NaN in both
template <class P, bool ALIGNED>
__device__ __forceinline__ void stage_first_xin(const float* __restrict__ r, bool ok, float* x, float* __restrict__ x_in, size_t base,
                                                int CHW) {
    const float nan = __builtin_nanf("");
    const float scale = ok ? r[P::XSCALE] : nan, c_in = ok ? r[P::CIN] : nan;
    const int n4 = CHW / 4, rem = CHW % 4;
    for (int i = blockIdx.x * STAGE_BLOCK + threadIdx.x; i < n4; i += gridDim.x * STAGE_BLOCK) {
        const size_t o = base + (size_t)i * 4;
        f32x4 v = load4<ALIGNED>(x + o), w;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * scale, w[e] = c_in * v[e];
        store4<ALIGNED>(x + o, v);
        store4<ALIGNED>(x_in + o, w);
    }
    if (rem && blockIdx.x == 0 && threadIdx.x == 0) {
        for (int e = 0; e < rem; ++e) {
            const size_t o = base + (size_t)n4 * 4 + e;
            const float v = x[o] * scale;
            x[o] = v;
            x_in[o] = c_in * v;
        }
    }
}

// the body of <sampler>_stage_kernel<ALIGNED>; hist and N are used with P::HIST alone, x_in with P::XIN alone, xc with P::CORR alone
template <class P, bool ALIGNED>
__device__ __forceinline__ void stage_body(int first, const float* __restrict__ tab, int rows, const int32_t* __restrict__ ctl,
                                           int row_v, uint32_t draw_v, uint32_t k0_v, uint32_t k1_v, float* x,
                                           const float* __restrict__ eps, const float* __restrict__ z,
                                           const int64_t* __restrict__ sample_index, float* hist, float* __restrict__ t_out,
                                           float* __restrict__ out, float* __restrict__ pred, int N, int CHW,
                                           float* __restrict__ x_in = nullptr, float* xc = nullptr) {
    constexpr int H = P::HIST, HD = H ? H : 1;
    const int n = blockIdx.y;
    const int row = ctl ? ctl[0] : row_v;
    const uint32_t draw = ctl ? (uint32_t)ctl[1] : draw_v;
    const uint32_t k0 = ctl ? (uint32_t)ctl[2] : k0_v, k1 = ctl ? (uint32_t)ctl[3] : k1_v;
    const bool ok = row >= 0 && row < rows;
    const float* r = tab + (size_t)(ok ? row : 0) * P::COLS;           // the read is clamped, the values are not
    const float nan = __builtin_nanf("");
    if (first) {
        if (blockIdx.x == 0 && threadIdx.x == 0) t_out[n] = ok ? r[P::T] : nan;
        if constexpr (P::XIN) stage_first_xin<P, ALIGNED>(r, ok, x, x_in, (size_t)n * CHW, CHW);
        return;
    }
    const int flags = ok ? (int)r[P::FLAGS] : 0;
    typename P::StageCoef k = P::fill(r, ok, flags);
    const bool fused = !z && sample_index;
    k.noisy = k.s != 0.f && (z || fused);                    // rows with s == 0 touch neither z nor the generator
    if constexpr (P::CORR) {
        if (!xc) P::uncorrect(k);
    }
    const bool last = !ok || (flags & P::FLAG_LAST) != 0;              // a poisoned launch poisons the sample too
    if (blockIdx.x == 0 && threadIdx.x == 0) t_out[n] = ok ? r[P::T_NEXT] : nan;
    uint32_t i_lo = 0, i_hi = 0;
    if (fused && k.noisy) {
        const uint64_t index = (uint64_t)sample_index[n];
        i_lo = (uint32_t)index, i_hi = (uint32_t)(index >> 32);
    }
    const size_t base = (size_t)n * CHW;
    float c_next = 0.f;
    bool feed = false;                                       // whether x_in is written: not on the last row, where nothing follows
    if constexpr (P::XIN) c_next = ok ? r[P::CIN_NEXT] : nan, feed = x_in && (!last || !ok);
    float* h0 = nullptr;
    const float* hp[HD] = {};
    if constexpr (H > 0) {
        const int s0 = ok ? row % (H + 1) : 0;
        const size_t slot = (size_t)N * CHW;
        h0 = hist + (size_t)s0 * slot;
#pragma unroll
        for (int j = 0; j < H; ++j) hp[j] = hist + (size_t)((s0 + H - j) % (H + 1)) * slot;
    }
    const int n4 = CHW / 4, rem = CHW % 4;
    for (int i0 = blockIdx.x * STAGE_BLOCK * STAGE_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * STAGE_BLOCK * STAGE_UNROLL) {
        f32x4 xv[STAGE_UNROLL], ev[STAGE_UNROLL], hv[HD][STAGE_UNROLL], zv[STAGE_UNROLL], cv[P::CORR ? STAGE_UNROLL : 1];
#pragma unroll
        for (int u = 0; u < STAGE_UNROLL; ++u) {
            const int i = i0 + u * STAGE_BLOCK;
            if (i < n4) {
                const size_t o = base + (size_t)i * 4;
                xv[u] = load4<ALIGNED>(x + o);
                ev[u] = load4<ALIGNED>(eps + o);
                if constexpr (H > 0) {
#pragma unroll
                    for (int j = 0; j < H; ++j)
                        if (k.rd[j]) hv[j][u] = load4<ALIGNED>(hp[j] + o);
                }
                if (k.noisy && !fused) zv[u] = load4<ALIGNED>(z + o);
                if constexpr (P::CORR) {
                    if (k.corr) cv[u] = load4<ALIGNED>(xc + o);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < STAGE_UNROLL; ++u) {
            const int i = i0 + u * STAGE_BLOCK;
            if (i >= n4) continue;
            const size_t o = base + (size_t)i * 4;
            if (k.noisy && fused) zv[u] = normals(philox4x32_10((uint32_t)i, draw, i_lo, i_hi, k0, k1));
            f32x4 xn, pv, bv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float d[HD] = {}, p;
                if constexpr (H > 0) {
#pragma unroll
                    for (int j = 0; j < H; ++j) d[j] = k.rd[j] ? hv[j][u][e] : 0.f;
                }
                if constexpr (P::CORR) {
                    float b;
                    xn[e] = P::stage_elem(k, xv[u][e], ev[u][e], d, k.corr ? cv[u][e] : 0.f, &p, &b);
                    bv[e] = ok ? b : nan;
                } else {
                    xn[e] = P::stage_elem(k, xv[u][e], ev[u][e], d, k.noisy ? zv[u][e] : 0.f, &p);
                }
                pv[e] = p;
            }
            store4<ALIGNED>(x + o, xn);
            if constexpr (P::CORR) {
                if (xc) store4<ALIGNED>(xc + o, bv);
            }
            if constexpr (H > 0) store4<ALIGNED>(h0 + o, pv);
            if (pred) store4<ALIGNED>(pred + o, pv);
            if constexpr (P::XIN) {
                if (feed) {
                    f32x4 xi;
#pragma unroll
                    for (int e = 0; e < 4; ++e) xi[e] = c_next * xn[e];
                    store4<ALIGNED>(x_in + o, xi);
                }
            }
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
            float d[HD] = {}, p;
            if constexpr (H > 0) {
#pragma unroll
                for (int j = 0; j < H; ++j) d[j] = k.rd[j] ? hp[j][o] : 0.f;
            }
            float xn;
            if constexpr (P::CORR) {
                float b;
                xn = P::stage_elem(k, x[o], eps[o], d, k.corr ? xc[o] : 0.f, &p, &b);
                if (xc) xc[o] = ok ? b : nan;
            } else {
                xn = P::stage_elem(k, x[o], eps[o], d, zt[e], &p);
            }
            x[o] = xn;
            if constexpr (H > 0) h0[o] = p;
            if (pred) pred[o] = p;
            if constexpr (P::XIN) {
                if (feed) x_in[o] = c_next * xn;
            }
            if (last) out[o] = clamp1(xn);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host side
// what every stage entry checks before anything of its own; mode_ok: the mode is one of the entry's two
inline int stage_check_launch(const char* fn, int32_t mode, bool mode_ok, bool first, const float* tab, int32_t rows,
                              const int32_t* ctl, int32_t row, const float* x, const float* eps, const float* t_out,
                              const float* out, int32_t N, int32_t CHW) {
    DXMI_CHECK_ARG(mode_ok, "%s: unknown mode %d", fn, mode);
    DXMI_CHECK_ARG(tab && t_out, "%s: null pointer (table or t_out)", fn);
    DXMI_CHECK_ARG(N > 0 && N <= 65535, "%s: N (%d) must be in [1, 65535]", fn, N);
    DXMI_CHECK_ARG(CHW > 0, "%s: CHW (%d) must be positive", fn, CHW);
    DXMI_CHECK_ARG(rows >= 1, "%s: the table needs at least one row, got %d", fn, rows);
    DXMI_CHECK_ARG(ctl || (row >= 0 && row < rows), "%s: row (%d) outside the table's [0, %d)", fn, row, rows);
    DXMI_CHECK_ARG((((uintptr_t)ctl) & 3) == 0 && (((uintptr_t)tab) & 3) == 0 && (((uintptr_t)t_out) & 3) == 0,
                   "%s: the control block, the table and t_out must be 4-byte aligned", fn);
    if (!first) DXMI_CHECK_ARG(x && eps && out, "%s: null pointer (x, eps or out)", fn);
    return DXMI_OK;
}

// the noise source and the alignment of a transition's tensors; hist: the history ring, or null for a sampler without one
inline int stage_check_tensors(const char* fn, const float* x, const float* eps, const float* z, const int64_t* sample_index,
                               const float* hist, const float* out, const float* pred_xstart) {
    DXMI_CHECK_ARG(!(z && sample_index), "%s: noise is either given (z) or made here (sample_index), not both", fn);
    DXMI_CHECK_ARG(((((uintptr_t)x) | ((uintptr_t)eps) | ((uintptr_t)z) | ((uintptr_t)hist) | ((uintptr_t)out) |
                     ((uintptr_t)pred_xstart)) & 15) == 0 && (((uintptr_t)sample_index) & 7) == 0,
                   "%s: tensors must be 16-byte aligned (sample_index 8-byte)", fn);
    return DXMI_OK;
}

// grid (min(chunks, 64), N) of STAGE_BLOCK threads; `aligned` when every row base is 16-byte aligned (CHW % 4 == 0)
template <typename... Params, typename... Args>
int stage_launch(const char* fn, void (*aligned)(Params...), void (*unaligned)(Params...), bool first, int32_t N, int32_t CHW,
                 void* stream, Args... args) {
    const int chunks = first ? 1 : (CHW / 4 + STAGE_BLOCK * STAGE_UNROLL - 1) / (STAGE_BLOCK * STAGE_UNROLL);
    const dim3 grid(chunks < 1 ? 1 : (chunks < 64 ? chunks : 64), N);
    hipLaunchKernelGGL(CHW % 4 == 0 ? aligned : unaligned, grid, dim3(STAGE_BLOCK), 0, (hipStream_t)stream, args...);
    DXMI_CHECK_LAUNCH(fn);
    return DXMI_OK;
}

}  // namespace
