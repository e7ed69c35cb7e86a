// Likelihood of the EDM nets and the DDPM teacher by the probability-flow ODE (models/cm/likelihood.py, models/DxMI/likelihood.py;
// Chen et al. 2018, "Neural Ordinary Differential Equations", the instantaneous change of variables; Song et al. 2021, "Score-Based
// Generative Modeling through Stochastic Differential Equations", appendix D.2; Hutchinson's trace estimator).  In the EDM variable
// dx/dsigma = k(x, sigma) = (x - D(x; sigma)) / sigma and d log p / dsigma = -div k; Heun on the augmented state (x, l) over the
// nodes sigma_0 < ... < sigma_S costs two network evaluations per step, each a forward F = net(c_in x, time) and the input-only
// backward g = d(eps . F)/d(net input) at the probe eps (unet_train.input_vjp).
//   dxmi_pf_ll_stage  the ONE launch after each evaluation: FIRST before the first, PREDICT after the evaluation at (x_i, sigma_i),
//                     CORRECT after the one at (x~, sigma_{i+1}).  It finishes the step, writes the next evaluation's preconditioned
//                     input and time, and reduces per image: the divergence estimate, and on the row flagged last |x|^2 of the prior.
// Conventions of stage_common.h (the control block, the table row, the poisoned row, load4 / store4 and the unaligned path, the
// Philox counter layout of dxmi_randn_indexed) and of dm_train.hip (one workgroup per image, per-image sums in a fixed order): fp32,
// one rounding per written operation, 16 bytes per lane, no atomics, plain vector stores.  An image's sums are a function of its own
// elements alone: a lane's running sum in index order, the xor-shuffle tree of a wave, a fixed pairing of the four wave partials,
// the CHW % 4 tail taken by the lane whose turn its block of four would have been.  So the results are bitwise equal run to run and
// do not depend on the batch an image rides in.
// Per element, with K = tab[row], e the probe, in this order:
//   PREDICT  k1 = K[KA] x + K[KB] F;  x~ = x + K[H] k1;  x_in = K[CIN_NEXT] x~;  d += K[KA] (e e) + K[DB] (e g)
//   CORRECT  x~ = x + K[H] k1 (the bits PREDICT wrote);  k2 = K[KA2] x~ + K[KB2] F;  x' = x + K[HH] (k1 + k2);  x_in = K[CIN_NEXT] x';
//            d += K[KA2] (e e) + K[DB2] (e g);  row flagged last: q += x' x'
// Per image:  PREDICT div1 = d;  CORRECT l += K[HH] (div1 + d);  last: prior = K[PRIOR_Q] q + K[PRIOR_C], logp = l + prior,
//             bpd = logp K[BPD_SCALE] + 7.
// CORRECT moves 32 bytes per element with a given probe (reads x, k1, F, g, e; writes x, x_in), 28 with the probe made here.
#include "stage_common.h"
#include "ew_common.h"

namespace {

constexpr int PL_UNROLL = 2;      // f32x4 per stream per lane in flight: five streams in CORRECT

struct PlCoef {
    float ka, kb, db, h, hh, c_next;
};

__device__ __forceinline__ float pl_sign(float z) { return z >= 0.f ? 1.f : -1.f; }

// one element of PREDICT (CORRECT = false) or CORRECT -> the state written (x~ or x'); *kout: k1 (PREDICT); *term: the element's
// share of the divergence estimate
template <bool CORRECT>
__device__ __forceinline__ float pl_elem(const PlCoef& k, float x, float f, float g, float e, float k1, float* kout, float* term) {
    const float e2 = e * e, eg = e * g;
    const float ta = k.ka * e2, tb = k.db * eg;
    *term = ta + tb;
    if (!CORRECT) {
        const float pa = k.ka * x, pb = k.kb * f;
        const float kk = pa + pb;
        *kout = kk;
        const float hk = k.h * kk;
        return x + hk;
    }
    const float hk = k.h * k1;
    const float xt = x + hk;
    const float pa = k.ka * xt, pb = k.kb * f;
    const float k2 = pa + pb;
    const float ks = k1 + k2;
    const float hs = k.hh * ks;
    return x + hs;
}

// MODE: DXMI_PF_LL_FIRST / _PREDICT / _CORRECT.  One workgroup per image.
template <int MODE, bool ALIGNED>
__global__ __launch_bounds__(STAGE_BLOCK) void pf_ll_stage_kernel(const float* __restrict__ tab, int rows, const int32_t* __restrict__ ctl,
                                                                  int row_v, uint32_t draw_v, uint32_t k0_v, uint32_t k1_v, float* x,
                                                                  const float* __restrict__ F, const float* __restrict__ G,
                                                                  const float* __restrict__ eps, const int64_t* __restrict__ sample_index,
                                                                  float* k1buf, float* __restrict__ xt_out, float* __restrict__ x_in,
                                                                  float* __restrict__ t_out, float* div1, float* ell,
                                                                  float* __restrict__ prior, float* __restrict__ logp,
                                                                  float* __restrict__ bpd, int CHW) {
    __shared__ float red[2][STAGE_BLOCK / 64];
    constexpr bool CORRECT = MODE == DXMI_PF_LL_CORRECT;
    const int n = blockIdx.x;
    const int row = ctl ? ctl[0] : row_v;
    const uint32_t draw = ctl ? (uint32_t)ctl[1] : draw_v;
    const uint32_t k0 = ctl ? (uint32_t)ctl[2] : k0_v, k1s = ctl ? (uint32_t)ctl[3] : k1_v;
    const bool ok = row >= 0 && row < rows;
    const float* r = tab + (size_t)(ok ? row : 0) * DXMI_PL_COLS;         // the read is clamped, the values are not
    const float nan = __builtin_nanf("");
    const size_t base = (size_t)n * CHW;
    const int n4 = CHW / 4, rem = CHW % 4;
    if (MODE == DXMI_PF_LL_FIRST) {
        const float scale = ok ? r[DXMI_PL_XSCALE] : nan, c_in = ok ? r[DXMI_PL_CIN] : nan;
        if (threadIdx.x == 0) {
            t_out[n] = ok ? r[DXMI_PL_T] : nan;
            ell[n] = ok ? r[DXMI_PL_LOGDET0] : nan;
        }
        for (int i = threadIdx.x; i < n4; i += STAGE_BLOCK) {
            const size_t o = base + (size_t)i * 4;
            f32x4 v = load4<ALIGNED>(x + o), w;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] * scale, w[e] = c_in * v[e];
            store4<ALIGNED>(x + o, v);
            store4<ALIGNED>(x_in + o, w);
        }
        if (rem && threadIdx.x == 0) {
            for (int e = 0; e < rem; ++e) {
                const size_t o = base + (size_t)n4 * 4 + e;
                const float v = x[o] * scale;
                x[o] = v;
                x_in[o] = c_in * v;
            }
        }
        return;
    }
    const int flags = ok ? (int)r[DXMI_PL_FLAGS] : 0;
    const bool last = CORRECT && (!ok || (flags & DXMI_PL_FLAG_LAST) != 0);      // a poisoned launch poisons logp and bpd too
    const bool feed = x_in && (!last || !ok);                                    // nothing follows the last row
    PlCoef k;
    k.ka = ok ? r[CORRECT ? DXMI_PL_KA2 : DXMI_PL_KA] : nan;
    k.kb = ok ? r[CORRECT ? DXMI_PL_KB2 : DXMI_PL_KB] : nan;
    k.db = ok ? r[CORRECT ? DXMI_PL_DB2 : DXMI_PL_DB] : nan;
    k.h = ok ? r[DXMI_PL_H] : nan, k.hh = ok ? r[DXMI_PL_HH] : nan, k.c_next = ok ? r[DXMI_PL_CIN_NEXT] : nan;
    if (threadIdx.x == 0) t_out[n] = ok ? r[DXMI_PL_T_NEXT] : nan;
    const bool fused = !eps;
    uint32_t i_lo = 0, i_hi = 0;
    if (fused) {
        const uint64_t index = (uint64_t)sample_index[n];
        i_lo = (uint32_t)index, i_hi = (uint32_t)(index >> 32);
    }
    float acc = 0.f, acc2 = 0.f;
    for (int i0 = threadIdx.x; i0 < n4; i0 += STAGE_BLOCK * PL_UNROLL) {
        f32x4 xv[PL_UNROLL], fv[PL_UNROLL], gv[PL_UNROLL], ev[PL_UNROLL], kv[PL_UNROLL];
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const int i = i0 + u * STAGE_BLOCK;
            if (i < n4) {
                const size_t o = base + (size_t)i * 4;
                xv[u] = load4<ALIGNED>(x + o);
                fv[u] = load4<ALIGNED>(F + o);
                gv[u] = load4<ALIGNED>(G + o);
                if (!fused) ev[u] = load4<ALIGNED>(eps + o);
                if (CORRECT) kv[u] = load4<ALIGNED>(k1buf + o);
            }
        }
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const int i = i0 + u * STAGE_BLOCK;
            if (i >= n4) continue;
            const size_t o = base + (size_t)i * 4;
            if (fused) {
                const f32x4 z = normals(philox4x32_10((uint32_t)i, draw, i_lo, i_hi, k0, k1s));
#pragma unroll
                for (int e = 0; e < 4; ++e) ev[u][e] = pl_sign(z[e]);
            }
            f32x4 xn, kk, xi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float ko = 0.f, term;
                xn[e] = pl_elem<CORRECT>(k, xv[u][e], fv[u][e], gv[u][e], ev[u][e], CORRECT ? kv[u][e] : 0.f, &ko, &term);
                kk[e] = ko;
                xi[e] = k.c_next * xn[e];
                acc += term;
                if (last) acc2 += xn[e] * xn[e];
            }
            if (CORRECT) {
                store4<ALIGNED>(x + o, xn);
            } else {
                store4<ALIGNED>(k1buf + o, kk);
                if (xt_out) store4<ALIGNED>(xt_out + o, xn);
            }
            if (feed) store4<ALIGNED>(x_in + o, xi);
        }
    }
    // the tail: the first `rem` values of block n4, one element per access, by the lane whose turn block n4 would have been; its
    // terms join that lane's running sum in index order
    if (rem && threadIdx.x == n4 % STAGE_BLOCK) {
        f32x4 et;
        et[0] = et[1] = et[2] = et[3] = 0.f;
        if (fused) {
            const f32x4 z = normals(philox4x32_10((uint32_t)n4, draw, i_lo, i_hi, k0, k1s));
#pragma unroll
            for (int e = 0; e < 4; ++e) et[e] = pl_sign(z[e]);
        }
        for (int e = 0; e < rem; ++e) {
            const size_t o = base + (size_t)n4 * 4 + e;
            const float ep = fused ? et[e] : eps[o];
            float ko = 0.f, term;
            const float xn = pl_elem<CORRECT>(k, x[o], F[o], G[o], ep, CORRECT ? k1buf[o] : 0.f, &ko, &term);
            acc += term;
            if (last) acc2 += xn * xn;
            if (CORRECT) {
                x[o] = xn;
            } else {
                k1buf[o] = ko;
                if (xt_out) xt_out[o] = xn;
            }
            if (feed) x_in[o] = k.c_next * xn;
        }
    }
    const float d = block_sum(acc, red[0]);
    if (!CORRECT) {
        if (threadIdx.x == 0) div1[n] = d;
        return;
    }
    const float q = block_sum(acc2, red[1]);      // every lane takes part (last is uniform; acc2 is 0 where it is not set)
    if (threadIdx.x == 0) {
        const float ds = div1[n] + d;
        const float dl = k.hh * ds;
        const float l = ell[n] + dl;
        ell[n] = l;
        if (last) {
            const float pq = (ok ? r[DXMI_PL_PRIOR_Q] : nan) * q;
            const float pr = pq + (ok ? r[DXMI_PL_PRIOR_C] : nan);
            const float lp = l + pr;
            const float bs = lp * (ok ? r[DXMI_PL_BPD_SCALE] : nan);
            prior[n] = pr;
            logp[n] = lp;
            bpd[n] = bs + 7.f;
        }
    }
}

template <int MODE>
int pl_launch(const char* fn, int32_t N, int32_t CHW, void* stream, const float* tab, int rows, const int32_t* ctl, int row, uint32_t draw,
              uint64_t seed, float* x, const float* F, const float* G, const float* eps, const int64_t* sample_index, float* k1,
              float* xt, float* x_in, float* t_out, float* div1, float* ell, float* prior, float* logp, float* bpd) {
    auto* aligned = pf_ll_stage_kernel<MODE, true>;
    auto* unaligned = pf_ll_stage_kernel<MODE, false>;
    hipLaunchKernelGGL(CHW % 4 == 0 ? aligned : unaligned, dim3(N), dim3(STAGE_BLOCK), 0, (hipStream_t)stream, tab, rows, ctl, row, draw, (uint32_t)seed, (uint32_t)(seed >> 32), x, F, G, eps, sample_index,
                       k1, xt, x_in, t_out, div1, ell, prior, logp, bpd, (int)CHW);
    DXMI_CHECK_LAUNCH(fn);
    return DXMI_OK;
}

}  // namespace

extern "C" int dxmi_pf_ll_stage(int32_t mode, const float* tab, int32_t rows, const int32_t* ctl, int32_t row, uint32_t draw,
                                uint64_t seed, float* x, const float* model_out, const float* vjp, const float* eps,
                                const int64_t* sample_index, float* k1, float* xt, float* x_in, float* t_out, float* div1, float* ell,
                                float* prior, float* logp, float* bpd, int32_t N, int32_t CHW, void* stream) {
    const char* fn = "dxmi_pf_ll_stage";
    const bool first = mode == DXMI_PF_LL_FIRST, predict = mode == DXMI_PF_LL_PREDICT, correct = mode == DXMI_PF_LL_CORRECT;
    DXMI_CHECK_ARG(first || predict || correct, "%s: unknown mode %d", fn, mode);
    DXMI_CHECK_ARG(tab && t_out, "%s: null pointer (table or t_out)", fn);
    DXMI_CHECK_ARG(N > 0 && N <= 65535, "%s: N (%d) must be in [1, 65535]", fn, N);
    DXMI_CHECK_ARG(CHW > 0 && CHW < (1 << 30), "%s: CHW (%d) must be in [1, 2^30)", fn, CHW);
    DXMI_CHECK_ARG(rows >= 1, "%s: the table needs at least one row, got %d", fn, rows);
    DXMI_CHECK_ARG(ctl || (row >= 0 && row < rows), "%s: row (%d) outside the table's [0, %d)", fn, row, rows);
    DXMI_CHECK_ARG(((((uintptr_t)ctl) | ((uintptr_t)tab) | ((uintptr_t)t_out) | ((uintptr_t)div1) | ((uintptr_t)ell) | ((uintptr_t)prior) |
                     ((uintptr_t)logp) | ((uintptr_t)bpd)) & 3) == 0,
                   "%s: the control block, the table and the per-image vectors must be 4-byte aligned", fn);
    DXMI_CHECK_ARG(x && (x_in || (correct && !ctl && row == rows - 1)),
                   "%s: null pointer (x, or x_in: only CORRECT on the last row, given by value, writes none)", fn);
    DXMI_CHECK_ARG(((((uintptr_t)x) | ((uintptr_t)model_out) | ((uintptr_t)vjp) | ((uintptr_t)eps) | ((uintptr_t)k1) | ((uintptr_t)xt) |
                     ((uintptr_t)x_in)) & 15) == 0 && (((uintptr_t)sample_index) & 7) == 0,
                   "%s: tensors must be 16-byte aligned (sample_index 8-byte)", fn);
    if (first) {
        DXMI_CHECK_ARG(ell, "%s: null pointer (FIRST sets ell)", fn);
        return pl_launch<DXMI_PF_LL_FIRST>(fn, N, CHW, stream, tab, rows, ctl, row, draw, seed, x, nullptr, nullptr, nullptr, nullptr, nullptr,
                                           nullptr, x_in, t_out, nullptr, ell, nullptr, nullptr, nullptr);
    }
    DXMI_CHECK_ARG(model_out && vjp && k1 && div1, "%s: null pointer (model_out, vjp, k1 or div1)", fn);
    DXMI_CHECK_ARG(!(eps && sample_index), "%s: the probe is either given (eps) or made here (sample_index), not both", fn);
    DXMI_CHECK_ARG(eps || sample_index, "%s: the probe is either given (eps) or made here (sample_index), not neither", fn);
    DXMI_CHECK_ARG(k1 != x && k1 != x_in && x_in != x && xt != x && (!xt || (xt != k1 && xt != x_in)),
                   "%s: x, k1, xt and x_in are four tensors: none may be another", fn);
    if (predict)
        return pl_launch<DXMI_PF_LL_PREDICT>(fn, N, CHW, stream, tab, rows, ctl, row, draw, seed, x, model_out, vjp, eps, sample_index, k1, xt,
                                             x_in, t_out, div1, nullptr, nullptr, nullptr, nullptr);
    DXMI_CHECK_ARG(ell && prior && logp && bpd, "%s: null pointer (CORRECT updates ell and, on the last row, writes prior, logp and bpd)", fn);
    return pl_launch<DXMI_PF_LL_CORRECT>(fn, N, CHW, stream, tab, rows, ctl, row, draw, seed, x, model_out, vjp, eps, sample_index, k1,
                                         nullptr, x_in, t_out, div1, ell, prior, logp, bpd);
}
