// Consistency distillation (CD) and consistency training (CT) losses (reference models/cm/karras_diffusion.py:108-241
// KarrasDenoiser.consistency_losses, with denoise :337-351, get_scalings / get_scalings_for_boundary_condition :64-80 and
// get_weightings :18-31).  One launch between two network evaluations:
//   dxmi_cd_prep      t = table[index]; x_t = x_start + noise t (kept); the online net's input c_in(t) x_t and time
//                     250 ln(t + 1e-44); the teacher's input too where its sigma_data differs
//   dxmi_cd_solver    EULER_X0 (CT: the Euler step with denoiser = x_start), HEUN_PRED (after teacher evaluation 1: d, the
//                     predictor samples and the teacher's second input), HEUN_CORR (after teacher evaluation 2: x_t2); EULER_X0
//                     and HEUN_CORR also write the target net's input c_in(t2) x_t2 and its time
//   dxmi_cd_loss_fwd  distiller = c_out(t) F_s + c_skip(t) x_t, target = c_out(t2) F_tg + c_skip(t2) x_t2, the norm (l1, l2,
//                     l2 after the two-tap bilinear resize to 32 x 32) and mean_flat(.) * get_weightings(snr(t))
//   dxmi_cd_loss_bwd  dF_s of that loss for a per-sample upstream gradient
//   dxmi_cd_huber_fwd / _bwd  the pseudo-Huber metric of improved consistency training (Song and Dhariwal 2023) on the same
//                     difference: ssq = sum(df^2) (kept for the backward), loss = w ssq / (sqrt(ssq + c^2) + c); the weight schedules
//                     above and DXMI_DSM_W_ICT, w = 1 / (t - t2)
// Elementwise streams: one workgroup row per image, 16 bytes per lane, several loads in flight; per-sample sums in a fixed order
// (bitwise reproducible).  The time levels are gathered from one small device table by index; an index outside [0, S - 2] gives
// NaN levels (nothing is read outside the table).
#include "dsm_common.h"
#include "ew_common.h"

namespace {

constexpr int RS = 32;            // F.interpolate(size=32)

struct Levels {
    float t, t2;
};

__device__ __forceinline__ Levels cd_levels(const int64_t* __restrict__ idx, const float* __restrict__ tab, int S, int b) {
    const int64_t i = idx[b];
    const bool ok = i >= 0 && i + 1 < (int64_t)S;
    Levels r;
    r.t = ok ? tab[i] : __builtin_nanf("");
    r.t2 = ok ? tab[i + 1] : __builtin_nanf("");
    return r;
}

__global__ __launch_bounds__(EW_BLOCK) void cd_prep_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                           const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                           float* __restrict__ x_t, float* __restrict__ x_in,
                                                           float* __restrict__ t_out, float* __restrict__ x_in_te, int CHW,
                                                           float sd2, float sd2_te) {
    const int b = blockIdx.y;
    const float t = cd_levels(idx, tab, S, b).t;
    const float c_in = dsm_c_in(t, sd2), c_in_te = dsm_c_in(t, sd2_te);
    if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = dsm_time(t);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 xv[EW_UNROLL], nv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                xv[u] = ld4(x0, base, i);
                nv[u] = ld4(noise, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 xt, o, ot;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xt[e] = xv[u][e] + nv[u][e] * t;      // x_t = x_start + noise * t (:190)
                o[e] = c_in * xt[e];                  // c_in * x_t (:348-349)
                ot[e] = c_in_te * xt[e];
            }
            st4(x_t, base, i, xt);
            st4(x_in, base, i, o);
            if (x_in_te) st4(x_in_te, base, i, ot);
        }
    }
}

// heun_solver / euler_solver (:144-174).  `sc`: the scalings of the diffusion whose denoise() forms the denoiser (the teacher's);
// sd2_next: sigma_data^2 of the diffusion whose network reads x_in_next (HEUN_PRED: the teacher's; otherwise the student's).
template <int MODE>
__global__ __launch_bounds__(EW_BLOCK) void cd_solver_kernel(const float* __restrict__ x0, const float* __restrict__ x_t,
                                                             const float* __restrict__ F, float* __restrict__ d_buf,
                                                             float* __restrict__ samples, const int64_t* __restrict__ idx,
                                                             const float* __restrict__ tab, int S, float* __restrict__ x_t2,
                                                             float* __restrict__ x_in_next, float* __restrict__ t_next, int CHW,
                                                             float sd, float sd2, float sigma_min, int distill, float sd2_next) {
    const int b = blockIdx.y;
    const Levels L = cd_levels(idx, tab, S, b);
    const float t = L.t, t2 = L.t2;
    const float dt = t2 - t, half_dt = dt / 2.f;                                  // next_t - t; (next_t - t) / 2 (:160)
    // EULER_X0 forms no denoiser: it has no scalings, and the solver_* arguments of the entry point mean nothing to it
    const DsmScal c = MODE == DXMI_CD_EULER_X0 ? DsmScal{0.f, 0.f, 0.f, 0.f}
                                               : dsm_scalings(MODE == DXMI_CD_HEUN_CORR ? t2 : t, sd, sd2, sigma_min, distill, DXMI_DSM_W_UNIFORM, 0.f);
    const float c_in_next = dsm_c_in(t2, sd2_next);
    if (blockIdx.x == 0 && threadIdx.x == 0) t_next[b] = dsm_time(t2);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 av[EW_UNROLL], bv[EW_UNROLL], cv[EW_UNROLL], dv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                av[u] = ld4(x_t, base, i);
                if (MODE == DXMI_CD_EULER_X0) bv[u] = ld4(x0, base, i);
                else bv[u] = ld4(F, base, i);
                if (MODE == DXMI_CD_HEUN_CORR) {
                    cv[u] = ld4(samples, base, i);
                    dv[u] = ld4(d_buf, base, i);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o, on, od;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = av[u][e];
                if (MODE == DXMI_CD_EULER_X0) {
                    const float d = (x - bv[u][e]) / t;                           // (x - denoiser) / t, denoiser = x0 (:171)
                    o[e] = x + d * dt;                                            // (:172)
                } else if (MODE == DXMI_CD_HEUN_PRED) {
                    const float den = c.c_out * bv[u][e] + c.c_skip * x;          // denoise() (:350), no clamp
                    const float d = (x - den) / t;                                // (:152)
                    od[e] = d;
                    o[e] = x + d * dt;                                            // (:153)
                } else {
                    const float s = cv[u][e];
                    const float den = c.c_out * bv[u][e] + c.c_skip * s;
                    const float nd = (s - den) / t2;                              // (:159)
                    o[e] = x + (dv[u][e] + nd) * half_dt;                         // (:160)
                }
                on[e] = c_in_next * o[e];
            }
            if (MODE == DXMI_CD_HEUN_PRED) {
                st4(d_buf, base, i, od);
                st4(samples, base, i, o);
            } else {
                st4(x_t2, base, i, o);
            }
            st4(x_in_next, base, i, on);
        }
    }
}

struct LossScal {
    float cs_o, cs_s, ct_o, ct_s, w;      // c_out / c_skip at t (online) and at t2 (target); get_weightings(snr(t))
};

__device__ __forceinline__ LossScal loss_scalings(Levels L, float sd, float sd2, float sigma_min, int distill, int sched, float inv_sd2) {
    const DsmScal a = dsm_scalings(L.t, sd, sd2, sigma_min, distill, sched, inv_sd2);
    const DsmScal b = dsm_scalings(L.t2, sd, sd2, sigma_min, distill, sched, inv_sd2);
    // DXMI_DSM_W_ICT needs both levels (the ladder descends: t > t2); only the pseudo-Huber entry points let it through
    return LossScal{a.c_out, a.c_skip, b.c_out, b.c_skip, sched == DXMI_DSM_W_ICT ? 1.f / (L.t - L.t2) : a.w};
}

// l1 / l2 on the full-resolution difference; one workgroup per image
template <int NORM>
__global__ __launch_bounds__(EW_BLOCK) void cd_loss_fwd_kernel(const float* __restrict__ Fs, const float* __restrict__ Ft,
                                                               const float* __restrict__ x_t, const float* __restrict__ x_t2,
                                                               const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                               float* __restrict__ loss, int CHW, float sd, float sd2,
                                                               float sigma_min, int distill, int sched, float inv_sd2) {
    __shared__ float red[EW_BLOCK / 64];
    const int b = blockIdx.x;
    const LossScal c = loss_scalings(cd_levels(idx, tab, S, b), sd, sd2, sigma_min, distill, sched, inv_sd2);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    float acc = 0.f;
    for (int i0 = threadIdx.x; i0 < n4; i0 += EW_BLOCK * EW_UNROLL) {
        f32x4 fs[EW_UNROLL], ft[EW_UNROLL], xa[EW_UNROLL], xb[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fs[u] = ld4(Fs, base, i);
                xa[u] = ld4(x_t, base, i);
                ft[u] = ld4(Ft, base, i);
                xb[u] = ld4(x_t2, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ds = c.cs_o * fs[u][e] + c.cs_s * xa[u][e];          // distiller (:193)
                const float dt = c.ct_o * ft[u][e] + c.ct_s * xb[u][e];          // distiller_target (:201)
                const float df = ds - dt;
                acc += NORM == DXMI_CD_NORM_L1 ? __builtin_fabsf(df) : df * df;   // (:207, :210)
            }
        }
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) loss[b] = (tot / (float)CHW) * c.w;                     // mean_flat(diffs) * weights
}

template <int NORM>
__global__ __launch_bounds__(EW_BLOCK) void cd_loss_bwd_kernel(const float* __restrict__ g, const float* __restrict__ Fs,
                                                               const float* __restrict__ Ft, const float* __restrict__ x_t,
                                                               const float* __restrict__ x_t2, const int64_t* __restrict__ idx,
                                                               const float* __restrict__ tab, int S, float* __restrict__ dFs,
                                                               int CHW, float sd, float sd2, float sigma_min, int distill,
                                                               int sched, float inv_sd2, float invD) {
    const int b = blockIdx.y;
    const LossScal c = loss_scalings(cd_levels(idx, tab, S, b), sd, sd2, sigma_min, distill, sched, inv_sd2);
    const float gs = (g[b] * c.w) * invD;       // mul by weights -> g * w; mean -> / D
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 fs[EW_UNROLL], ft[EW_UNROLL], xa[EW_UNROLL], xb[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fs[u] = ld4(Fs, base, i);
                xa[u] = ld4(x_t, base, i);
                ft[u] = ld4(Ft, base, i);
                xb[u] = ld4(x_t2, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ds = c.cs_o * fs[u][e] + c.cs_s * xa[u][e];
                const float dt = c.ct_o * ft[u][e] + c.ct_s * xb[u][e];
                const float df = ds - dt;
                float gd;
                if (NORM == DXMI_CD_NORM_L1) gd = gs * (df > 0.f ? 1.f : (df < 0.f ? -1.f : (df == 0.f ? 0.f : df)));   // sign, sign(0) = 0
                else gd = gs * (2.f * df);
                o[e] = gd * c.cs_o;
            }
            st4(dFs, base, i, o);
        }
    }
}

// Pseudo-Huber metric on the full-resolution difference: the l2 stream and sum order of cd_loss_fwd_kernel, the sum kept.
// w * ssq / (sqrt(ssq + c^2) + c) is sqrt(ssq + c^2) - c without the cancellation at ssq << c^2 (a converged model).
__global__ __launch_bounds__(EW_BLOCK) void cd_huber_fwd_kernel(const float* __restrict__ Fs, const float* __restrict__ Ft,
                                                                const float* __restrict__ x_t, const float* __restrict__ x_t2,
                                                                const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                                float* __restrict__ loss, float* __restrict__ ssq, int CHW, float hc,
                                                                float sd, float sd2, float sigma_min, int distill, int sched,
                                                                float inv_sd2) {
    __shared__ float red[EW_BLOCK / 64];
    const int b = blockIdx.x;
    const LossScal c = loss_scalings(cd_levels(idx, tab, S, b), sd, sd2, sigma_min, distill, sched, inv_sd2);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    float acc = 0.f;
    for (int i0 = threadIdx.x; i0 < n4; i0 += EW_BLOCK * EW_UNROLL) {
        f32x4 fs[EW_UNROLL], ft[EW_UNROLL], xa[EW_UNROLL], xb[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fs[u] = ld4(Fs, base, i);
                xa[u] = ld4(x_t, base, i);
                ft[u] = ld4(Ft, base, i);
                xb[u] = ld4(x_t2, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ds = c.cs_o * fs[u][e] + c.cs_s * xa[u][e];
                const float dt = c.ct_o * ft[u][e] + c.ct_s * xb[u][e];
                const float df = ds - dt;
                acc += df * df;
            }
        }
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) {
        ssq[b] = tot;
        loss[b] = c.w * (tot / (__builtin_sqrtf(tot + hc * hc) + hc));
    }
}

// dF_s = ((g w) / sqrt(ssq + c^2)) df c_out(t), ssq as the forward wrote it
__global__ __launch_bounds__(EW_BLOCK) void cd_huber_bwd_kernel(const float* __restrict__ g, const float* __restrict__ ssq,
                                                                const float* __restrict__ Fs, const float* __restrict__ Ft,
                                                                const float* __restrict__ x_t, const float* __restrict__ x_t2,
                                                                const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                                float* __restrict__ dFs, int CHW, float hc, float sd, float sd2,
                                                                float sigma_min, int distill, int sched, float inv_sd2) {
    const int b = blockIdx.y;
    const LossScal c = loss_scalings(cd_levels(idx, tab, S, b), sd, sd2, sigma_min, distill, sched, inv_sd2);
    const float gs = (g[b] * c.w) / __builtin_sqrtf(ssq[b] + hc * hc);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 fs[EW_UNROLL], ft[EW_UNROLL], xa[EW_UNROLL], xb[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fs[u] = ld4(Fs, base, i);
                xa[u] = ld4(x_t, base, i);
                ft[u] = ld4(Ft, base, i);
                xb[u] = ld4(x_t2, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ds = c.cs_o * fs[u][e] + c.cs_s * xa[u][e];
                const float dt = c.ct_o * ft[u][e] + c.ct_s * xb[u][e];
                o[e] = (gs * (ds - dt)) * c.cs_o;
            }
            st4(dFs, base, i, o);
        }
    }
}

// F.interpolate(size=32, mode="bilinear"), align_corners False, no antialias: source index (o + 0.5) in / 32 - 0.5 clamped at 0,
// taps i0 = floor, i1 = min(i0 + 1, in - 1), weights 1 - lambda and lambda.  Two taps per axis; at 64 -> 32 the 2x2 mean.
struct Tap {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Tap tap_of(int o, int in, float scale) {
    float src = scale * ((float)o + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Tap r;
    r.i0 = (int)src;
    r.i0 = r.i0 > in - 1 ? in - 1 : r.i0;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

// (distiller - target) after both were resized, at output pixel (oy, ox) of one channel plane
__device__ __forceinline__ float resized_diff(const float* __restrict__ Fs, const float* __restrict__ Ft, const float* __restrict__ xa,
                                              const float* __restrict__ xb, const LossScal& c, Tap ty, Tap tx, int W) {
    const int r0 = ty.i0 * W, r1 = ty.i1 * W;
    const int p00 = r0 + tx.i0, p01 = r0 + tx.i1, p10 = r1 + tx.i0, p11 = r1 + tx.i1;
    const float s00 = c.cs_o * Fs[p00] + c.cs_s * xa[p00], s01 = c.cs_o * Fs[p01] + c.cs_s * xa[p01];
    const float s10 = c.cs_o * Fs[p10] + c.cs_s * xa[p10], s11 = c.cs_o * Fs[p11] + c.cs_s * xa[p11];
    const float t00 = c.ct_o * Ft[p00] + c.ct_s * xb[p00], t01 = c.ct_o * Ft[p01] + c.ct_s * xb[p01];
    const float t10 = c.ct_o * Ft[p10] + c.ct_s * xb[p10], t11 = c.ct_o * Ft[p11] + c.ct_s * xb[p11];
    const float s = ty.l0 * (tx.l0 * s00 + tx.l1 * s01) + ty.l1 * (tx.l0 * s10 + tx.l1 * s11);
    const float t = ty.l0 * (tx.l0 * t00 + tx.l1 * t01) + ty.l1 * (tx.l0 * t10 + tx.l1 * t11);
    return s - t;
}

__global__ __launch_bounds__(EW_BLOCK) void cd_loss32_fwd_kernel(const float* __restrict__ Fs, const float* __restrict__ Ft,
                                                                 const float* __restrict__ x_t, const float* __restrict__ x_t2,
                                                                 const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                                 float* __restrict__ loss, int C, int H, int W, float sd, float sd2,
                                                                 float sigma_min, int distill, int sched, float inv_sd2) {
    __shared__ float red[EW_BLOCK / 64];
    const int b = blockIdx.x;
    const LossScal c = loss_scalings(cd_levels(idx, tab, S, b), sd, sd2, sigma_min, distill, sched, inv_sd2);
    const float sy = (float)H / (float)RS, sx = (float)W / (float)RS;
    const size_t base = (size_t)b * C * H * W;
    float acc = 0.f;
    for (int o = threadIdx.x; o < C * RS * RS; o += EW_BLOCK) {
        const int ch = o / (RS * RS), oy = (o / RS) % RS, ox = o % RS;
        const size_t pb = base + (size_t)ch * H * W;
        const float df = resized_diff(Fs + pb, Ft + pb, x_t + pb, x_t2 + pb, c, tap_of(oy, H, sy), tap_of(ox, W, sx), W);
        acc += df * df;                                                           // (:219)
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) loss[b] = (tot / (float)(C * RS * RS)) * c.w;
}

// The transpose of the resize, one workgroup per channel plane (grid N x C): the 32 x 32 upstream values go to LDS, then every input pixel gathers the
// outputs that tap it (in index order: no atomics).
__global__ __launch_bounds__(EW_BLOCK) void cd_loss32_bwd_kernel(const float* __restrict__ g, const float* __restrict__ Fs,
                                                                 const float* __restrict__ Ft, const float* __restrict__ x_t,
                                                                 const float* __restrict__ x_t2, const int64_t* __restrict__ idx,
                                                                 const float* __restrict__ tab, int S, float* __restrict__ dFs, int C,
                                                                 int H, int W, float sd, float sd2, float sigma_min, int distill,
                                                                 int sched, float inv_sd2, float invD) {
    __shared__ float E[RS * RS];
    const int b = blockIdx.x;
    const LossScal c = loss_scalings(cd_levels(idx, tab, S, b), sd, sd2, sigma_min, distill, sched, inv_sd2);
    const float gs = (g[b] * c.w) * invD;
    const float sy = (float)H / (float)RS, sx = (float)W / (float)RS;
    {
        const int ch = blockIdx.y;            // one workgroup per channel plane
        const size_t pb = ((size_t)b * C + ch) * H * W;
        for (int o = threadIdx.x; o < RS * RS; o += EW_BLOCK) {
            const float df = resized_diff(Fs + pb, Ft + pb, x_t + pb, x_t2 + pb, c, tap_of(o / RS, H, sy), tap_of(o % RS, W, sx), W);
            E[o] = gs * (2.f * df);
        }
        __syncthreads();
        for (int p = threadIdx.x; p < H * W; p += EW_BLOCK) {
            const int y = p / W, x = p % W;
            // outputs whose source index lies within one pixel of (y, x), widened by one on each side; each is checked exactly
            int oy0 = (int)floorf(((float)y - 0.5f) / sy - 0.5f) - 1, oy1 = (int)ceilf(((float)y + 1.5f) / sy - 0.5f) + 1;
            int ox0 = (int)floorf(((float)x - 0.5f) / sx - 0.5f) - 1, ox1 = (int)ceilf(((float)x + 1.5f) / sx - 0.5f) + 1;
            oy0 = oy0 < 0 ? 0 : oy0;
            ox0 = ox0 < 0 ? 0 : ox0;
            oy1 = oy1 > RS - 1 ? RS - 1 : oy1;
            ox1 = ox1 > RS - 1 ? RS - 1 : ox1;
            float acc = 0.f;
            for (int oy = oy0; oy <= oy1; ++oy) {
                const Tap ty = tap_of(oy, H, sy);
                const float wy = (ty.i0 == y ? ty.l0 : 0.f) + (ty.i1 == y ? ty.l1 : 0.f);
                if (ty.i0 != y && ty.i1 != y) continue;
                for (int ox = ox0; ox <= ox1; ++ox) {
                    const Tap tx = tap_of(ox, W, sx);
                    if (tx.i0 != x && tx.i1 != x) continue;
                    const float wx = (tx.i0 == x ? tx.l0 : 0.f) + (tx.i1 == x ? tx.l1 : 0.f);
                    acc += (wy * wx) * E[oy * RS + ox];
                }
            }
            dFs[pb + p] = acc * c.cs_o;
        }
    }
}

// loss_norm lpips: the two images the LPIPS network reads, (distiller + 1) / 2 in rows [0, N) and (target + 1) / 2 in rows [N, 2 N) of one
// stacked batch (reference :232-233), and get_weightings(snr(t)) per sample
__global__ __launch_bounds__(EW_BLOCK) void cd_lpips_images_kernel(const float* __restrict__ Fs, const float* __restrict__ Ft,
                                                                   const float* __restrict__ x_t, const float* __restrict__ x_t2,
                                                                   const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                                   float* __restrict__ x01, float* __restrict__ wout, int N, int CHW,
                                                                   float sd, float sd2, float sigma_min, int distill, int sched,
                                                                   float inv_sd2) {
    const int b = blockIdx.y;
    const LossScal c = loss_scalings(cd_levels(idx, tab, S, b), sd, sd2, sigma_min, distill, sched, inv_sd2);
    if (blockIdx.x == 0 && threadIdx.x == 0) wout[b] = c.w;
    const size_t base = (size_t)b * CHW, base_t = (size_t)(N + b) * CHW;
    const int n4 = CHW / 4;
    for (int i = blockIdx.x * EW_BLOCK + threadIdx.x; i < n4; i += gridDim.x * EW_BLOCK) {
        const f32x4 fs = ld4(Fs, base, i), xa = ld4(x_t, base, i), ft = ld4(Ft, base, i), xb = ld4(x_t2, base, i);
        f32x4 o, ot;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = ((c.cs_o * fs[e] + c.cs_s * xa[e]) + 1.f) / 2.f;
            ot[e] = ((c.ct_o * ft[e] + c.ct_s * xb[e]) + 1.f) / 2.f;
        }
        st4(x01, base, i, o);
        st4(x01, base_t, i, ot);
    }
}

// dF_s = ((g w) d_x01 / 2) c_out(t): autograd's nodes in its order, for d_x01 of the LPIPS value at unit upstream
__global__ __launch_bounds__(EW_BLOCK) void cd_lpips_bwd_kernel(const float* __restrict__ g, const float* __restrict__ dx01,
                                                                const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                                float* __restrict__ dFs, int CHW, float sd, float sd2, float sigma_min,
                                                                int distill, int sched, float inv_sd2) {
    const int b = blockIdx.y;
    const LossScal c = loss_scalings(cd_levels(idx, tab, S, b), sd, sd2, sigma_min, distill, sched, inv_sd2);
    const float gs = g[b] * c.w;
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i = blockIdx.x * EW_BLOCK + threadIdx.x; i < n4; i += gridDim.x * EW_BLOCK) {
        const f32x4 d = ld4(dx01, base, i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = ((gs * d[e]) / 2.f) * c.cs_o;
        st4(dFs, base, i, o);
    }
}

}  // namespace

#define CD_CHECK_SHAPE(fn)                                                                                                       \
    EW_CHECK_SHAPE(fn);                                                                                                          \
    DXMI_CHECK_ARG(num_scales >= 2, fn ": num_scales (%d) must be at least 2", num_scales)

extern "C" int dxmi_cd_prep(const float* x_start, const float* noise, const int64_t* indices, const float* t_table, int32_t num_scales,
                            float* x_t, float* x_in, float* t_out, float* x_in_teacher, int32_t N, int32_t CHW, float sigma_data,
                            float teacher_sigma_data, void* stream) {
    DXMI_CHECK_ARG(x_start && noise && indices && t_table && x_t && x_in && t_out, "dxmi_cd_prep: null pointer");
    CD_CHECK_SHAPE("dxmi_cd_prep");
    EW_CHECK_ALIGNED("dxmi_cd_prep", x_start, noise, x_t, x_in, x_in_teacher);
    hipLaunchKernelGGL(cd_prep_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, x_start, noise, indices, t_table,
                       num_scales, x_t, x_in, t_out, x_in_teacher, CHW, sigma_data * sigma_data, teacher_sigma_data * teacher_sigma_data);
    DXMI_CHECK_LAUNCH("dxmi_cd_prep");
    return DXMI_OK;
}

extern "C" int dxmi_cd_solver(int32_t mode, const float* x_start, const float* x_t, const float* model_out, float* d, float* samples,
                              const int64_t* indices, const float* t_table, int32_t num_scales, float* x_t2, float* x_in_next,
                              float* t_next, int32_t N, int32_t CHW, float solver_sigma_data, float solver_sigma_min,
                              int32_t solver_distillation, float next_sigma_data, void* stream) {
    DXMI_CHECK_ARG(mode >= DXMI_CD_EULER_X0 && mode <= DXMI_CD_HEUN_CORR, "dxmi_cd_solver: unknown mode %d", mode);
    DXMI_CHECK_ARG(x_t && indices && t_table && x_in_next && t_next, "dxmi_cd_solver: null pointer");
    if (mode == DXMI_CD_EULER_X0) DXMI_CHECK_ARG(x_start && x_t2, "dxmi_cd_solver: EULER_X0 needs x_start and x_t2");
    if (mode == DXMI_CD_HEUN_PRED) DXMI_CHECK_ARG(model_out && d && samples, "dxmi_cd_solver: HEUN_PRED needs model_out, d and samples");
    if (mode == DXMI_CD_HEUN_CORR)
        DXMI_CHECK_ARG(model_out && d && samples && x_t2, "dxmi_cd_solver: HEUN_CORR needs model_out, d, samples and x_t2");
    CD_CHECK_SHAPE("dxmi_cd_solver");
    EW_CHECK_ALIGNED("dxmi_cd_solver", x_start, x_t, model_out, d, samples, x_t2, x_in_next);
    const dim3 grid = ew_grid(N, CHW), block(EW_BLOCK);
    const float sd = solver_sigma_data, sd2 = sd * sd, sd2n = next_sigma_data * next_sigma_data;
    const int dist = (int)(solver_distillation != 0);
#define CD_SOLVER_LAUNCH(M)                                                                                                        \
    hipLaunchKernelGGL(cd_solver_kernel<M>, grid, block, 0, (hipStream_t)stream, x_start, x_t, model_out, d, samples, indices, t_table, \
                       num_scales, x_t2, x_in_next, t_next, CHW, sd, sd2, solver_sigma_min, dist, sd2n)
    switch (mode) {
        case DXMI_CD_EULER_X0:  CD_SOLVER_LAUNCH(DXMI_CD_EULER_X0); break;
        case DXMI_CD_HEUN_PRED: CD_SOLVER_LAUNCH(DXMI_CD_HEUN_PRED); break;
        default:                CD_SOLVER_LAUNCH(DXMI_CD_HEUN_CORR); break;
    }
#undef CD_SOLVER_LAUNCH
    DXMI_CHECK_LAUNCH("dxmi_cd_solver");
    return DXMI_OK;
}

#define CD_CHECK_LOSS(fn)                                                                                                        \
    DXMI_CHECK_ARG(C > 0 && H > 0 && W > 0 && (int64_t)C * H * W < ((int64_t)1 << 30), fn ": C, H, W (%d, %d, %d) must be "      \
                   "positive and C H W below 2^30", C, H, W);                                                                    \
    const int32_t CHW = C * H * W;                                                                                               \
    CD_CHECK_SHAPE(fn);                                                                                                          \
    DXMI_CHECK_ARG(loss_norm >= DXMI_CD_NORM_L1 && loss_norm <= DXMI_CD_NORM_L2_32, fn ": unknown loss norm %d", loss_norm);     \
    DXMI_CHECK_ARG(weight_schedule >= DXMI_DSM_W_SNR && weight_schedule <= DXMI_DSM_W_UNIFORM, fn ": unknown weight schedule %d", \
                   weight_schedule)

extern "C" int dxmi_cd_loss_fwd(const float* f_online, const float* f_target, const float* x_t, const float* x_t2,
                                const int64_t* indices, const float* t_table, int32_t num_scales, float* loss, int32_t N, int32_t C,
                                int32_t H, int32_t W, int32_t loss_norm, float sigma_data, float sigma_min, int32_t distillation,
                                int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(f_online && f_target && x_t && x_t2 && indices && t_table && loss, "dxmi_cd_loss_fwd: null pointer");
    CD_CHECK_LOSS("dxmi_cd_loss_fwd");
    EW_CHECK_ALIGNED("dxmi_cd_loss_fwd", f_online, f_target, x_t, x_t2);
    const float sd2 = sigma_data * sigma_data, inv_sd2 = (float)(1.0 / ((double)sigma_data * (double)sigma_data));
    const int dist = (int)(distillation != 0);
    const dim3 grid(N), block(EW_BLOCK);
    if (loss_norm == DXMI_CD_NORM_L2_32)
        hipLaunchKernelGGL(cd_loss32_fwd_kernel, grid, block, 0, (hipStream_t)stream, f_online, f_target, x_t, x_t2, indices, t_table,
                           num_scales, loss, C, H, W, sigma_data, sd2, sigma_min, dist, weight_schedule, inv_sd2);
    else if (loss_norm == DXMI_CD_NORM_L1)
        hipLaunchKernelGGL(cd_loss_fwd_kernel<DXMI_CD_NORM_L1>, grid, block, 0, (hipStream_t)stream, f_online, f_target, x_t, x_t2, indices,
                           t_table, num_scales, loss, CHW, sigma_data, sd2, sigma_min, dist, weight_schedule, inv_sd2);
    else
        hipLaunchKernelGGL(cd_loss_fwd_kernel<DXMI_CD_NORM_L2>, grid, block, 0, (hipStream_t)stream, f_online, f_target, x_t, x_t2, indices,
                           t_table, num_scales, loss, CHW, sigma_data, sd2, sigma_min, dist, weight_schedule, inv_sd2);
    DXMI_CHECK_LAUNCH("dxmi_cd_loss_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_cd_loss_bwd(const float* g_loss, const float* f_online, const float* f_target, const float* x_t, const float* x_t2,
                                const int64_t* indices, const float* t_table, int32_t num_scales, float* d_f_online, int32_t N,
                                int32_t C, int32_t H, int32_t W, int32_t loss_norm, float sigma_data, float sigma_min,
                                int32_t distillation, int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(g_loss && f_online && f_target && x_t && x_t2 && indices && t_table && d_f_online, "dxmi_cd_loss_bwd: null pointer");
    CD_CHECK_LOSS("dxmi_cd_loss_bwd");
    DXMI_CHECK_ARG(C <= 65535, "dxmi_cd_loss_bwd: C (%d) must be at most 65535", C);
    EW_CHECK_ALIGNED("dxmi_cd_loss_bwd", f_online, f_target, x_t, x_t2, d_f_online);
    const float sd2 = sigma_data * sigma_data, inv_sd2 = (float)(1.0 / ((double)sigma_data * (double)sigma_data));
    const int dist = (int)(distillation != 0);
    const dim3 block(EW_BLOCK);
    if (loss_norm == DXMI_CD_NORM_L2_32)
        hipLaunchKernelGGL(cd_loss32_bwd_kernel, dim3(N, C), block, 0, (hipStream_t)stream, g_loss, f_online, f_target, x_t, x_t2, indices,
                           t_table, num_scales, d_f_online, C, H, W, sigma_data, sd2, sigma_min, dist, weight_schedule, inv_sd2,
                           (float)(1.0 / (double)(C * RS * RS)));
    else if (loss_norm == DXMI_CD_NORM_L1)
        hipLaunchKernelGGL(cd_loss_bwd_kernel<DXMI_CD_NORM_L1>, ew_grid(N, CHW), block, 0, (hipStream_t)stream, g_loss, f_online, f_target,
                           x_t, x_t2, indices, t_table, num_scales, d_f_online, CHW, sigma_data, sd2, sigma_min, dist, weight_schedule,
                           inv_sd2, (float)(1.0 / (double)CHW));
    else
        hipLaunchKernelGGL(cd_loss_bwd_kernel<DXMI_CD_NORM_L2>, ew_grid(N, CHW), block, 0, (hipStream_t)stream, g_loss, f_online, f_target,
                           x_t, x_t2, indices, t_table, num_scales, d_f_online, CHW, sigma_data, sd2, sigma_min, dist, weight_schedule,
                           inv_sd2, (float)(1.0 / (double)CHW));
    DXMI_CHECK_LAUNCH("dxmi_cd_loss_bwd");
    return DXMI_OK;
}

#define CD_CHECK_HUBER(fn)                                                                                                       \
    CD_CHECK_SHAPE(fn);                                                                                                          \
    DXMI_CHECK_ARG(huber_c > 0.f && huber_c <= 3.4028234663852886e38f, fn ": huber_c (%g) must be finite and positive",          \
                   (double)huber_c);                                                                                             \
    DXMI_CHECK_ARG(weight_schedule >= DXMI_DSM_W_SNR && weight_schedule <= DXMI_DSM_W_ICT, fn ": unknown weight schedule %d",    \
                   weight_schedule)

extern "C" int dxmi_cd_huber_fwd(const float* f_online, const float* f_target, const float* x_t, const float* x_t2,
                                 const int64_t* indices, const float* t_table, int32_t num_scales, float* loss, float* ssq, int32_t N,
                                 int32_t CHW, float huber_c, float sigma_data, float sigma_min, int32_t distillation,
                                 int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(f_online && f_target && x_t && x_t2 && indices && t_table && loss && ssq, "dxmi_cd_huber_fwd: null pointer");
    CD_CHECK_HUBER("dxmi_cd_huber_fwd");
    EW_CHECK_ALIGNED("dxmi_cd_huber_fwd", f_online, f_target, x_t, x_t2);
    const float sd2 = sigma_data * sigma_data, inv_sd2 = (float)(1.0 / ((double)sigma_data * (double)sigma_data));
    hipLaunchKernelGGL(cd_huber_fwd_kernel, dim3(N), dim3(EW_BLOCK), 0, (hipStream_t)stream, f_online, f_target, x_t, x_t2, indices, t_table,
                       num_scales, loss, ssq, CHW, huber_c, sigma_data, sd2, sigma_min, (int)(distillation != 0), weight_schedule, inv_sd2);
    DXMI_CHECK_LAUNCH("dxmi_cd_huber_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_cd_huber_bwd(const float* g_loss, const float* ssq, const float* f_online, const float* f_target, const float* x_t,
                                 const float* x_t2, const int64_t* indices, const float* t_table, int32_t num_scales, float* d_f_online,
                                 int32_t N, int32_t CHW, float huber_c, float sigma_data, float sigma_min, int32_t distillation,
                                 int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(g_loss && ssq && f_online && f_target && x_t && x_t2 && indices && t_table && d_f_online,
                   "dxmi_cd_huber_bwd: null pointer");
    CD_CHECK_HUBER("dxmi_cd_huber_bwd");
    EW_CHECK_ALIGNED("dxmi_cd_huber_bwd", f_online, f_target, x_t, x_t2, d_f_online);
    const float sd2 = sigma_data * sigma_data, inv_sd2 = (float)(1.0 / ((double)sigma_data * (double)sigma_data));
    hipLaunchKernelGGL(cd_huber_bwd_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, g_loss, ssq, f_online, f_target, x_t,
                       x_t2, indices, t_table, num_scales, d_f_online, CHW, huber_c, sigma_data, sd2, sigma_min, (int)(distillation != 0),
                       weight_schedule, inv_sd2);
    DXMI_CHECK_LAUNCH("dxmi_cd_huber_bwd");
    return DXMI_OK;
}

#define CD_CHECK_LPIPS(fn)                                                                                                       \
    CD_CHECK_SHAPE(fn);                                                                                                          \
    DXMI_CHECK_ARG(weight_schedule >= DXMI_DSM_W_SNR && weight_schedule <= DXMI_DSM_W_UNIFORM, fn ": unknown weight schedule %d", \
                   weight_schedule)

extern "C" int dxmi_cd_lpips_images(const float* f_online, const float* f_target, const float* x_t, const float* x_t2,
                                    const int64_t* indices, const float* t_table, int32_t num_scales, float* x01, float* weights,
                                    int32_t N, int32_t CHW, float sigma_data, float sigma_min, int32_t distillation,
                                    int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(f_online && f_target && x_t && x_t2 && indices && t_table && x01 && weights, "dxmi_cd_lpips_images: null pointer");
    CD_CHECK_LPIPS("dxmi_cd_lpips_images");
    EW_CHECK_ALIGNED("dxmi_cd_lpips_images", f_online, f_target, x_t, x_t2, x01);
    const float sd2 = sigma_data * sigma_data, inv_sd2 = (float)(1.0 / ((double)sigma_data * (double)sigma_data));
    hipLaunchKernelGGL(cd_lpips_images_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, f_online, f_target, x_t, x_t2, indices,
                       t_table, num_scales, x01, weights, N, CHW, sigma_data, sd2, sigma_min, (int)(distillation != 0), weight_schedule, inv_sd2);
    DXMI_CHECK_LAUNCH("dxmi_cd_lpips_images");
    return DXMI_OK;
}

extern "C" int dxmi_cd_lpips_bwd(const float* g_loss, const float* d_x01, const int64_t* indices, const float* t_table, int32_t num_scales,
                                 float* d_f_online, int32_t N, int32_t CHW, float sigma_data, float sigma_min, int32_t distillation,
                                 int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(g_loss && d_x01 && indices && t_table && d_f_online, "dxmi_cd_lpips_bwd: null pointer");
    CD_CHECK_LPIPS("dxmi_cd_lpips_bwd");
    EW_CHECK_ALIGNED("dxmi_cd_lpips_bwd", d_x01, d_f_online);
    const float sd2 = sigma_data * sigma_data, inv_sd2 = (float)(1.0 / ((double)sigma_data * (double)sigma_data));
    hipLaunchKernelGGL(cd_lpips_bwd_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, g_loss, d_x01, indices, t_table, num_scales,
                       d_f_online, CHW, sigma_data, sd2, sigma_min, (int)(distillation != 0), weight_schedule, inv_sd2);
    DXMI_CHECK_LAUNCH("dxmi_cd_lpips_bwd");
    return DXMI_OK;
}
