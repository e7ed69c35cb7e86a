// Progressive distillation loss (reference models/cm/karras_diffusion.py:243-335 KarrasDenoiser.progdist_losses, with denoise
// :337-351, get_scalings / get_scalings_for_boundary_condition :64-80 and get_weightings :18-31).  The launches between the
// network evaluations of one call (the first, x_t and the inputs at t, is dxmi_cd_prep of cm_train.hip on the coarse ladder):
//   dxmi_pd_solver MID   after teacher evaluation 1 at (x_t, t): the Euler step to t2, the teacher's second input and its time
//   dxmi_pd_solver END   after teacher evaluation 2 at (x_t2, t2): the Euler step to t3 (x_t3 is never stored) and
//                        target_x = euler_to_denoiser(x_t, t, x_t3, t3)
//   dxmi_pd_loss_fwd     denoised = c_out(t) F_online + c_skip(t) x_t, the norm (l1, l2) against target_x and
//                        mean_flat(.) * get_weightings(snr(t))
//   dxmi_pd_loss_bwd     dF_online of that loss for a per-sample upstream gradient
//   dxmi_pd_lpips_images the stacked (denoised + 1) / 2, (target_x + 1) / 2 batch of the lpips norm and the per-sample weights
// Conventions of cm_train.hip: one workgroup row per image, 16 bytes per lane, several loads in flight; per-sample sums in a fixed
// order (bitwise reproducible).  The levels are gathered from one device table of 2 S + 1 entries by index: t = tab[i], t3 = tab[i + 1]
// (the coarse ladder, S + 1 levels) and t2 = tab[S + 1 + i] (the half steps, S levels).  An index outside [0, S - 1] gives NaN levels
// (nothing is read outside the table).
#include "dsm_common.h"
#include "ew_common.h"

namespace {

struct Levels {
    float t, t2, t3;
};

__device__ __forceinline__ Levels pd_levels(const int64_t* __restrict__ idx, const float* __restrict__ tab, int S, int b) {
    const int64_t i = idx[b];
    const bool ok = i >= 0 && i < (int64_t)S;
    Levels r;
    r.t = ok ? tab[i] : __builtin_nanf("");
    r.t3 = ok ? tab[i + 1] : __builtin_nanf("");
    r.t2 = ok ? tab[(int64_t)S + 1 + i] : __builtin_nanf("");
    return r;
}

// euler_solver (:267-274) twice and euler_to_denoiser (:276-281).  `sd`, `sigma_min`, `distill`: the scalings of the diffusion
// whose denoise() forms the denoiser (the teacher's); sd2_next: sigma_data^2 of the diffusion whose network reads x_in_next.
template <int MODE>
__global__ __launch_bounds__(EW_BLOCK) void pd_solver_kernel(const float* __restrict__ x_t, const float* __restrict__ x_t2_in,
                                                             const float* __restrict__ F, const int64_t* __restrict__ idx,
                                                             const float* __restrict__ tab, int S, float* __restrict__ out,
                                                             float* __restrict__ x_in_next, float* __restrict__ t_next, int CHW,
                                                             float sd, float sd2, float sigma_min, int distill, float sd2_next) {
    const int b = blockIdx.y;
    const Levels L = pd_levels(idx, tab, S, b);
    const float t = L.t, t2 = L.t2, t3 = L.t3;
    const float s_eval = MODE == DXMI_PD_MID ? t : t2;                             // where the teacher was evaluated
    const float dt = MODE == DXMI_PD_MID ? t2 - t : t3 - t2;                       // next_t - t (:272)
    const float dt3 = t3 - t;                                                      // next_t - t of euler_to_denoiser (:279)
    const DsmScal c = dsm_scalings(s_eval, sd, sd2, sigma_min, distill, DXMI_DSM_W_UNIFORM, 0.f);
    const float c_in_next = dsm_c_in(t2, sd2_next);
    if (MODE == DXMI_PD_MID && blockIdx.x == 0 && threadIdx.x == 0) t_next[b] = dsm_time(t2);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 av[EW_UNROLL], bv[EW_UNROLL], cv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                av[u] = ld4(x_t, base, i);
                bv[u] = ld4(F, base, i);
                if (MODE == DXMI_PD_END) cv[u] = ld4(x_t2_in, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o, on;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xt = av[u][e];
                const float x = MODE == DXMI_PD_MID ? xt : cv[u][e];
                const float den = c.c_out * bv[u][e] + c.c_skip * x;               // denoise() (:350), no clamp
                const float d = (x - den) / s_eval;                                // (:271)
                const float nx = x + d * dt;                                       // (:272)
                if (MODE == DXMI_PD_MID) {
                    o[e] = nx;                                                     // x_t2
                    on[e] = c_in_next * nx;
                } else {
                    o[e] = xt - (t * (nx - xt)) / dt3;                             // x_t - t * (x_t3 - x_t) / (t3 - t) (:278-280)
                }
            }
            st4(out, base, i, o);
            if (MODE == DXMI_PD_MID) st4(x_in_next, base, i, on);
        }
    }
}

// l1 / l2 against the stored target; one workgroup per image
template <int NORM>
__global__ __launch_bounds__(EW_BLOCK) void pd_loss_fwd_kernel(const float* __restrict__ Fs, const float* __restrict__ x_t,
                                                               const float* __restrict__ target, const int64_t* __restrict__ idx,
                                                               const float* __restrict__ tab, int S, float* __restrict__ loss, int CHW,
                                                               float sd, float sd2, float sigma_min, int distill, int sched,
                                                               float inv_sd2) {
    __shared__ float red[EW_BLOCK / 64];
    const int b = blockIdx.x;
    const DsmScal c = dsm_scalings(pd_levels(idx, tab, S, b).t, sd, sd2, sigma_min, distill, sched, inv_sd2);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    float acc = 0.f;
    for (int i0 = threadIdx.x; i0 < n4; i0 += EW_BLOCK * EW_UNROLL) {
        f32x4 fs[EW_UNROLL], xa[EW_UNROLL], tg[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fs[u] = ld4(Fs, base, i);
                xa[u] = ld4(x_t, base, i);
                tg[u] = ld4(target, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ds = c.c_out * fs[u][e] + c.c_skip * xa[u][e];       // denoised_x (:302)
                const float df = ds - tg[u][e];
                acc += NORM == DXMI_CD_NORM_L1 ? __builtin_fabsf(df) : df * df;   // (:312, :315)
            }
        }
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) loss[b] = (tot / (float)CHW) * c.w;                     // mean_flat(diffs) * weights
}

template <int NORM>
__global__ __launch_bounds__(EW_BLOCK) void pd_loss_bwd_kernel(const float* __restrict__ g, const float* __restrict__ Fs,
                                                               const float* __restrict__ x_t, const float* __restrict__ target,
                                                               const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                               float* __restrict__ dFs, int CHW, float sd, float sd2, float sigma_min,
                                                               int distill, int sched, float inv_sd2, float invD) {
    const int b = blockIdx.y;
    const DsmScal c = dsm_scalings(pd_levels(idx, tab, S, b).t, sd, sd2, sigma_min, distill, sched, inv_sd2);
    const float gs = (g[b] * c.w) * invD;       // mul by weights -> g * w; mean -> / D
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 fs[EW_UNROLL], xa[EW_UNROLL], tg[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fs[u] = ld4(Fs, base, i);
                xa[u] = ld4(x_t, base, i);
                tg[u] = ld4(target, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ds = c.c_out * fs[u][e] + c.c_skip * xa[u][e];
                const float df = ds - tg[u][e];
                float gd;
                if (NORM == DXMI_CD_NORM_L1) gd = gs * (df > 0.f ? 1.f : (df < 0.f ? -1.f : (df == 0.f ? 0.f : df)));   // sign, sign(0) = 0
                else gd = gs * (2.f * df);
                o[e] = gd * c.c_out;
            }
            st4(dFs, base, i, o);
        }
    }
}

// loss_norm lpips: (denoised + 1) / 2 in rows [0, N) and (target_x + 1) / 2 in rows [N, 2 N) of one stacked batch (reference
// :322-325), and get_weightings(snr(t)) per sample
__global__ __launch_bounds__(EW_BLOCK) void pd_lpips_images_kernel(const float* __restrict__ Fs, const float* __restrict__ x_t,
                                                                   const float* __restrict__ target, const int64_t* __restrict__ idx,
                                                                   const float* __restrict__ tab, int S, float* __restrict__ x01,
                                                                   float* __restrict__ wout, int N, int CHW, float sd, float sd2,
                                                                   float sigma_min, int distill, int sched, float inv_sd2) {
    const int b = blockIdx.y;
    const DsmScal c = dsm_scalings(pd_levels(idx, tab, S, b).t, sd, sd2, sigma_min, distill, sched, inv_sd2);
    if (blockIdx.x == 0 && threadIdx.x == 0) wout[b] = c.w;
    const size_t base = (size_t)b * CHW, base_t = (size_t)(N + b) * CHW;
    const int n4 = CHW / 4;
    for (int i = blockIdx.x * EW_BLOCK + threadIdx.x; i < n4; i += gridDim.x * EW_BLOCK) {
        const f32x4 fs = ld4(Fs, base, i), xa = ld4(x_t, base, i), tg = ld4(target, base, i);
        f32x4 o, ot;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = ((c.c_out * fs[e] + c.c_skip * xa[e]) + 1.f) / 2.f;
            ot[e] = (tg[e] + 1.f) / 2.f;
        }
        st4(x01, base, i, o);
        st4(x01, base_t, i, ot);
    }
}

}  // namespace

#define PD_CHECK_SHAPE(fn) \
    EW_CHECK_SHAPE(fn);    \
    EW_CHECK_SCALES(fn)

#define PD_CHECK_LOSS(fn)                                                                                                        \
    PD_CHECK_SHAPE(fn);                                                                                                          \
    DXMI_CHECK_ARG(loss_norm == DXMI_CD_NORM_L1 || loss_norm == DXMI_CD_NORM_L2, fn ": loss norm %d is neither L1 nor L2",       \
                   loss_norm);                                                                                                   \
    DXMI_CHECK_ARG(weight_schedule >= DXMI_DSM_W_SNR && weight_schedule <= DXMI_DSM_W_UNIFORM, fn ": unknown weight schedule %d", \
                   weight_schedule)

extern "C" int dxmi_pd_solver(int32_t mode, const float* x_t, const float* x_t2_in, const float* model_out, const int64_t* indices,
                              const float* t_table, int32_t num_scales, float* out, float* x_in_next, float* t_next, int32_t N,
                              int32_t CHW, float solver_sigma_data, float solver_sigma_min, int32_t solver_distillation,
                              float next_sigma_data, void* stream) {
    DXMI_CHECK_ARG(mode == DXMI_PD_MID || mode == DXMI_PD_END, "dxmi_pd_solver: unknown mode %d", mode);
    DXMI_CHECK_ARG(x_t && model_out && indices && t_table && out, "dxmi_pd_solver: null pointer");
    if (mode == DXMI_PD_MID) DXMI_CHECK_ARG(x_in_next && t_next, "dxmi_pd_solver: MID needs x_in_next and t_next");
    if (mode == DXMI_PD_END) DXMI_CHECK_ARG(x_t2_in, "dxmi_pd_solver: END needs x_t2");
    PD_CHECK_SHAPE("dxmi_pd_solver");
    EW_CHECK_ALIGNED("dxmi_pd_solver", x_t, x_t2_in, model_out, out, x_in_next);
    const dim3 grid = ew_grid(N, CHW), block(EW_BLOCK);
    const float sd = solver_sigma_data, sd2 = sd * sd, sd2n = next_sigma_data * next_sigma_data;
    const int dist = (int)(solver_distillation != 0);
    if (mode == DXMI_PD_MID)
        hipLaunchKernelGGL(pd_solver_kernel<DXMI_PD_MID>, grid, block, 0, (hipStream_t)stream, x_t, x_t2_in, model_out, indices, t_table,
                           num_scales, out, x_in_next, t_next, CHW, sd, sd2, solver_sigma_min, dist, sd2n);
    else
        hipLaunchKernelGGL(pd_solver_kernel<DXMI_PD_END>, grid, block, 0, (hipStream_t)stream, x_t, x_t2_in, model_out, indices, t_table,
                           num_scales, out, x_in_next, t_next, CHW, sd, sd2, solver_sigma_min, dist, sd2n);
    DXMI_CHECK_LAUNCH("dxmi_pd_solver");
    return DXMI_OK;
}

extern "C" int dxmi_pd_loss_fwd(const float* f_online, const float* x_t, const float* target_x, const int64_t* indices,
                                const float* t_table, int32_t num_scales, float* loss, int32_t N, int32_t CHW, int32_t loss_norm,
                                float sigma_data, float sigma_min, int32_t distillation, int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(f_online && x_t && target_x && indices && t_table && loss, "dxmi_pd_loss_fwd: null pointer");
    PD_CHECK_LOSS("dxmi_pd_loss_fwd");
    EW_CHECK_ALIGNED("dxmi_pd_loss_fwd", f_online, x_t, target_x);
    const float sd2 = sigma_data * sigma_data, inv_sd2 = (float)(1.0 / ((double)sigma_data * (double)sigma_data));
    const int dist = (int)(distillation != 0);
    const dim3 grid(N), block(EW_BLOCK);
    if (loss_norm == DXMI_CD_NORM_L1)
        hipLaunchKernelGGL(pd_loss_fwd_kernel<DXMI_CD_NORM_L1>, grid, block, 0, (hipStream_t)stream, f_online, x_t, target_x, indices,
                           t_table, num_scales, loss, CHW, sigma_data, sd2, sigma_min, dist, weight_schedule, inv_sd2);
    else
        hipLaunchKernelGGL(pd_loss_fwd_kernel<DXMI_CD_NORM_L2>, grid, block, 0, (hipStream_t)stream, f_online, x_t, target_x, indices,
                           t_table, num_scales, loss, CHW, sigma_data, sd2, sigma_min, dist, weight_schedule, inv_sd2);
    DXMI_CHECK_LAUNCH("dxmi_pd_loss_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_pd_loss_bwd(const float* g_loss, const float* f_online, const float* x_t, const float* target_x,
                                const int64_t* indices, const float* t_table, int32_t num_scales, float* d_f_online, int32_t N,
                                int32_t CHW, int32_t loss_norm, float sigma_data, float sigma_min, int32_t distillation,
                                int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(g_loss && f_online && x_t && target_x && indices && t_table && d_f_online, "dxmi_pd_loss_bwd: null pointer");
    PD_CHECK_LOSS("dxmi_pd_loss_bwd");
    EW_CHECK_ALIGNED("dxmi_pd_loss_bwd", f_online, x_t, target_x, d_f_online);
    const float sd2 = sigma_data * sigma_data, inv_sd2 = (float)(1.0 / ((double)sigma_data * (double)sigma_data));
    const int dist = (int)(distillation != 0);
    const dim3 grid = ew_grid(N, CHW), block(EW_BLOCK);
    if (loss_norm == DXMI_CD_NORM_L1)
        hipLaunchKernelGGL(pd_loss_bwd_kernel<DXMI_CD_NORM_L1>, grid, block, 0, (hipStream_t)stream, g_loss, f_online, x_t, target_x, indices,
                           t_table, num_scales, d_f_online, CHW, sigma_data, sd2, sigma_min, dist, weight_schedule, inv_sd2,
                           (float)(1.0 / (double)CHW));
    else
        hipLaunchKernelGGL(pd_loss_bwd_kernel<DXMI_CD_NORM_L2>, grid, block, 0, (hipStream_t)stream, g_loss, f_online, x_t, target_x, indices,
                           t_table, num_scales, d_f_online, CHW, sigma_data, sd2, sigma_min, dist, weight_schedule, inv_sd2,
                           (float)(1.0 / (double)CHW));
    DXMI_CHECK_LAUNCH("dxmi_pd_loss_bwd");
    return DXMI_OK;
}

extern "C" int dxmi_pd_lpips_images(const float* f_online, const float* x_t, const float* target_x, const int64_t* indices,
                                    const float* t_table, int32_t num_scales, float* x01, float* weights, int32_t N, int32_t CHW,
                                    float sigma_data, float sigma_min, int32_t distillation, int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(f_online && x_t && target_x && indices && t_table && x01 && weights, "dxmi_pd_lpips_images: null pointer");
    PD_CHECK_SHAPE("dxmi_pd_lpips_images");
    DXMI_CHECK_ARG(weight_schedule >= DXMI_DSM_W_SNR && weight_schedule <= DXMI_DSM_W_UNIFORM,
                   "dxmi_pd_lpips_images: unknown weight schedule %d", weight_schedule);
    EW_CHECK_ALIGNED("dxmi_pd_lpips_images", f_online, x_t, target_x, x01);
    const float sd2 = sigma_data * sigma_data, inv_sd2 = (float)(1.0 / ((double)sigma_data * (double)sigma_data));
    hipLaunchKernelGGL(pd_lpips_images_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, f_online, x_t, target_x, indices,
                       t_table, num_scales, x01, weights, N, CHW, sigma_data, sd2, sigma_min, (int)(distillation != 0), weight_schedule,
                       inv_sd2);
    DXMI_CHECK_LAUNCH("dxmi_pd_lpips_images");
    return DXMI_OK;
}
