// Denoising score-matching (DSM) loss of the EDM teacher and the EMA of its weights (reference models/cm/karras_diffusion.py:18-31
// get_weightings, :82-106 KarrasDenoiser.training_losses; models/cm/nn.py:57-67 update_ema; models/cm/train_util.py:29-264).
//   dxmi_edm_dsm_prep      x_in = c_in(s) (x_start + s noise), t = 250 ln(s + 1e-44): the network input of a batch, one launch
//   dxmi_edm_dsm_loss_fwd  denoised = c_out F + c_skip x_t; per sample mean_flat((denoised - x_start)^2) and its weighted twin
//   dxmi_edm_dsm_loss_bwd  dF of the two terms, the upstream gradients read from device memory
//   dxmi_ema_update        ema_k = rate_k ema_k + (1 - rate_k) src over many tensors and up to DXMI_EMA_MAX_RATES rates
// x_t is never stored: the loss kernels recompute it with the prep kernel's operations.  All four are HBM-bound: 16 bytes per
// lane, several loads in flight per wave; the per-sample sums are reduced in a fixed order (bitwise reproducible).
#include "dsm_common.h"
#include "ew_common.h"

namespace {

__global__ __launch_bounds__(EW_BLOCK) void dsm_prep_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                            const float* __restrict__ sigma, float* __restrict__ x_in,
                                                            float* __restrict__ t_out, int CHW, float sd2) {
    const int b = blockIdx.y;
    const float s = sigma[b];
    const float c_in = dsm_c_in(s, sd2);
    if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = dsm_time(s);
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
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xt = xv[u][e] + nv[u][e] * s;     // x_t = x_start + noise * sigma (:91)
                o[e] = c_in * xt;                             // c_in * x_t (:348-349)
            }
            st4(x_in, base, i, o);
        }
    }
}

// One workgroup per sample: each lane sums its elements in index order, then block_sum.
__global__ __launch_bounds__(EW_BLOCK) void dsm_loss_fwd_kernel(const float* __restrict__ F, const float* __restrict__ x0,
                                                                const float* __restrict__ noise, const float* __restrict__ sigma,
                                                                float* __restrict__ xs_mse, float* __restrict__ mse, int CHW,
                                                                float sd, float sd2, float sigma_min, int distill, int sched,
                                                                float inv_sd2) {
    __shared__ float red[2][EW_BLOCK / 64];
    const int b = blockIdx.x;
    const float s = sigma[b];
    const DsmScal c = dsm_scalings(s, sd, sd2, sigma_min, distill, sched, inv_sd2);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    float acc_xs = 0.f, acc_w = 0.f;
    for (int i0 = threadIdx.x; i0 < n4; i0 += EW_BLOCK * EW_UNROLL) {
        f32x4 fv[EW_UNROLL], xv[EW_UNROLL], nv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fv[u] = ld4(F, base, i);
                xv[u] = ld4(x0, base, i);
                nv[u] = ld4(noise, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xt = xv[u][e] + nv[u][e] * s;
                const float den = c.c_out * fv[u][e] + c.c_skip * xt;     // denoise() (:350)
                const float d = den - xv[u][e];
                const float sq = d * d;
                acc_xs += sq;                                             // (denoised - x_start) ** 2 (:102)
                acc_w += c.w * sq;                                        // weights * (denoised - x_start) ** 2 (:103)
            }
        }
    }
    const float tot_xs = block_sum(acc_xs, red[0]), tot_w = block_sum(acc_w, red[1]);
    if (threadIdx.x == 0) {
        const float fD = (float)CHW;
        xs_mse[b] = tot_xs / fD;       // mean_flat
        mse[b] = tot_w / fD;
    }
}

// autograd of the two terms, node by node: mean -> g / D; weights * sq -> (g / D) * w; pow(., 2) -> . * (2 e);
// the two branches meet at `denoised`; c_out * F -> . * c_out.
__global__ __launch_bounds__(EW_BLOCK) void dsm_loss_bwd_kernel(const float* __restrict__ g_mse, const float* __restrict__ g_xs,
                                                                const float* __restrict__ F, const float* __restrict__ x0,
                                                                const float* __restrict__ noise, const float* __restrict__ sigma,
                                                                float* __restrict__ dF, int CHW, float sd, float sd2,
                                                                float sigma_min, int distill, int sched, float inv_sd2, float invD) {
    const int b = blockIdx.y;
    const float s = sigma[b];
    const DsmScal c = dsm_scalings(s, sd, sd2, sigma_min, distill, sched, inv_sd2);
    const bool has_m = g_mse != nullptr, has_x = g_xs != nullptr;
    const float ga = has_m ? (g_mse[b] * invD) * c.w : 0.f;
    const float gb = has_x ? g_xs[b] * invD : 0.f;
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 fv[EW_UNROLL], xv[EW_UNROLL], nv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fv[u] = ld4(F, base, i);
                xv[u] = ld4(x0, base, i);
                nv[u] = ld4(noise, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xt = xv[u][e] + nv[u][e] * s;
                const float den = c.c_out * fv[u][e] + c.c_skip * xt;
                const float d2 = 2.f * (den - xv[u][e]);
                float g;
                if (has_m && has_x) g = ga * d2 + gb * d2;
                else g = has_m ? ga * d2 : gb * d2;
                o[e] = g * c.c_out;
            }
            st4(dF, base, i, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// EMA over a tensor list, the multi-tensor table of optim.hip: DXMI_MT_MAX tensors per launch by value, 4096 elements per
// workgroup, the source read once for all K rates.  torch's targ.mul_(rate).add_(src, alpha=1-rate): t = t * rate, then
// t + alpha * src, which ATen's add kernel evaluates as one fused multiply-add.
constexpr int EMA_BLOCK = 256;
constexpr int EMA_CHUNK = 4096;

struct EmaTable {
    const float* src[DXMI_MT_MAX];
    float* ema[DXMI_EMA_MAX_RATES][DXMI_MT_MAX];
    int64_t numel[DXMI_MT_MAX];
    int32_t first_block[DXMI_MT_MAX + 1];
    int32_t count;
};

struct EmaRates {
    float rate[DXMI_EMA_MAX_RATES], alpha[DXMI_EMA_MAX_RATES];
};

// rate 0 (the target of improved consistency training: the stop-gradient student) is a copy, bit for bit: 0 * ema + src turns a
// source of -0 into +0 and a non-finite ema into NaN
__device__ __forceinline__ float ema_one(float rate, float alpha, float src, float ema) {
    return rate == 0.f ? src : __builtin_fmaf(alpha, src, ema * rate);
}

template <int K>
__global__ __launch_bounds__(EMA_BLOCK) void ema_kernel(EmaTable t, EmaRates r, const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.f) return;     // the EMA follows the optimiser: an overflow step leaves it (train_util.py:190-193)
    int ti = 0;
#pragma unroll 1
    for (int i = 1; i < t.count; ++i) ti = ((int)blockIdx.x >= t.first_block[i]) ? i : ti;
    const int64_t n = t.numel[ti];
    const int64_t base = (int64_t)(blockIdx.x - t.first_block[ti]) * EMA_CHUNK;
    const float* __restrict__ S = t.src[ti];
    uintptr_t align = (uintptr_t)S;
#pragma unroll
    for (int k = 0; k < K; ++k) align |= (uintptr_t)t.ema[k][ti];
    constexpr int R = EMA_CHUNK / (EMA_BLOCK * 4);
    if ((align & 15) == 0 && base + EMA_CHUNK <= n) {
        f32x4 sv[R], ev[K][R];
#pragma unroll
        for (int q = 0; q < R; ++q) sv[q] = *(const f32x4*)(S + base + (int64_t)(q * EMA_BLOCK + threadIdx.x) * 4);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int q = 0; q < R; ++q) ev[k][q] = *(const f32x4*)(t.ema[k][ti] + base + (int64_t)(q * EMA_BLOCK + threadIdx.x) * 4);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int q = 0; q < R; ++q) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = ema_one(r.rate[k], r.alpha[k], sv[q][e], ev[k][q][e]);
                *(f32x4*)(t.ema[k][ti] + base + (int64_t)(q * EMA_BLOCK + threadIdx.x) * 4) = o;
            }
        return;
    }
    const int64_t end = base + EMA_CHUNK < n ? base + EMA_CHUNK : n;
    for (int64_t i = base + threadIdx.x; i < end; i += EMA_BLOCK) {
        const float sv = S[i];
#pragma unroll
        for (int k = 0; k < K; ++k) t.ema[k][ti][i] = ema_one(r.rate[k], r.alpha[k], sv, t.ema[k][ti][i]);
    }
}

}  // namespace

extern "C" int dxmi_edm_dsm_prep(const float* x_start, const float* noise, const float* sigma, float* x_in, float* t_out, int32_t N,
                                 int32_t CHW, float sigma_data, void* stream) {
    DXMI_CHECK_ARG(x_start && noise && sigma && x_in && t_out, "dxmi_edm_dsm_prep: null pointer");
    EW_CHECK_SHAPE("dxmi_edm_dsm_prep");
    EW_CHECK_ALIGNED("dxmi_edm_dsm_prep", x_start, noise, x_in);
    hipLaunchKernelGGL(dsm_prep_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, x_start, noise, sigma, x_in, t_out,
                       CHW, sigma_data * sigma_data);
    DXMI_CHECK_LAUNCH("dxmi_edm_dsm_prep");
    return DXMI_OK;
}

extern "C" int dxmi_edm_dsm_loss_fwd(const float* model_out, const float* x_start, const float* noise, const float* sigma,
                                     float* xs_mse, float* mse, int32_t N, int32_t CHW, float sigma_data, float sigma_min,
                                     int32_t distillation, int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(model_out && x_start && noise && sigma && xs_mse && mse, "dxmi_edm_dsm_loss_fwd: null pointer");
    EW_CHECK_SHAPE("dxmi_edm_dsm_loss_fwd");
    DXMI_CHECK_ARG(weight_schedule >= DXMI_DSM_W_SNR && weight_schedule <= DXMI_DSM_W_UNIFORM,
                   "dxmi_edm_dsm_loss_fwd: unknown weight schedule %d", weight_schedule);
    EW_CHECK_ALIGNED("dxmi_edm_dsm_loss_fwd", model_out, x_start, noise);
    hipLaunchKernelGGL(dsm_loss_fwd_kernel, dim3(N), dim3(EW_BLOCK), 0, (hipStream_t)stream, model_out, x_start, noise, sigma, xs_mse,
                       mse, CHW, sigma_data, sigma_data * sigma_data, sigma_min, (int)(distillation != 0), weight_schedule,
                       (float)(1.0 / ((double)sigma_data * (double)sigma_data)));
    DXMI_CHECK_LAUNCH("dxmi_edm_dsm_loss_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_edm_dsm_loss_bwd(const float* g_mse, const float* g_xs, const float* model_out, const float* x_start,
                                     const float* noise, const float* sigma, float* d_model_out, int32_t N, int32_t CHW,
                                     float sigma_data, float sigma_min, int32_t distillation, int32_t weight_schedule, void* stream) {
    DXMI_CHECK_ARG(model_out && x_start && noise && sigma && d_model_out, "dxmi_edm_dsm_loss_bwd: null pointer");
    DXMI_CHECK_ARG(g_mse || g_xs, "dxmi_edm_dsm_loss_bwd: no upstream gradient (g_mse and g_xs both null)");
    EW_CHECK_SHAPE("dxmi_edm_dsm_loss_bwd");
    DXMI_CHECK_ARG(weight_schedule >= DXMI_DSM_W_SNR && weight_schedule <= DXMI_DSM_W_UNIFORM,
                   "dxmi_edm_dsm_loss_bwd: unknown weight schedule %d", weight_schedule);
    EW_CHECK_ALIGNED("dxmi_edm_dsm_loss_bwd", model_out, x_start, noise, d_model_out);
    hipLaunchKernelGGL(dsm_loss_bwd_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, g_mse, g_xs, model_out, x_start,
                       noise, sigma, d_model_out, CHW, sigma_data, sigma_data * sigma_data, sigma_min, (int)(distillation != 0),
                       weight_schedule, (float)(1.0 / ((double)sigma_data * (double)sigma_data)), (float)(1.0 / (double)CHW));
    DXMI_CHECK_LAUNCH("dxmi_edm_dsm_loss_bwd");
    return DXMI_OK;
}

extern "C" int dxmi_ema_update(void* const* ema, const void* const* src, const int64_t* numel, int32_t count, int32_t n_rates,
                               const double* rates, const float* found_inf, void* stream) {
    DXMI_CHECK_ARG(ema && src && numel && rates && count > 0, "dxmi_ema_update: null argument or empty list");
    DXMI_CHECK_ARG(n_rates >= 1 && n_rates <= DXMI_EMA_MAX_RATES, "dxmi_ema_update: n_rates (%d) outside [1, %d]", n_rates,
                   DXMI_EMA_MAX_RATES);
    EmaRates r = {};
    for (int k = 0; k < n_rates; ++k) {
        r.rate[k] = (float)rates[k];                  // python doubles rounded once, as ATen's Scalar -> fp32
        r.alpha[k] = (float)(1.0 - rates[k]);
    }
    // the whole list is validated before the first launch: a bad tensor never leaves the EMA half updated
    for (int off = 0; off < count; off += DXMI_MT_MAX) {
        const int c = count - off < DXMI_MT_MAX ? count - off : DXMI_MT_MAX;
        int64_t nb = 0;
        for (int i = off; i < off + c; ++i) {
            DXMI_CHECK_ARG(numel[i] > 0 && src[i], "dxmi_ema_update: empty or null tensor %d", i);
            for (int k = 0; k < n_rates; ++k)
                DXMI_CHECK_ARG(ema[(size_t)k * count + i], "dxmi_ema_update: null EMA tensor (rate %d, tensor %d)", k, i);
            nb += (numel[i] + EMA_CHUNK - 1) / EMA_CHUNK;
            DXMI_CHECK_ARG(nb < ((int64_t)1 << 31), "dxmi_ema_update: too many elements in one launch");
        }
    }
    for (int off = 0; off < count; off += DXMI_MT_MAX) {
        const int c = count - off < DXMI_MT_MAX ? count - off : DXMI_MT_MAX;
        EmaTable t;
        t.count = c;
        int64_t nb = 0;
        for (int i = 0; i < c; ++i) {
            t.src[i] = (const float*)src[off + i];
            for (int k = 0; k < n_rates; ++k) t.ema[k][i] = (float*)ema[(size_t)k * count + off + i];
            t.numel[i] = numel[off + i];
            t.first_block[i] = (int32_t)nb;
            nb += (numel[off + i] + EMA_CHUNK - 1) / EMA_CHUNK;
        }
        t.first_block[c] = (int32_t)nb;
        const dim3 grid((unsigned)nb), block(EMA_BLOCK);
        switch (n_rates) {
            case 1: hipLaunchKernelGGL(ema_kernel<1>, grid, block, 0, (hipStream_t)stream, t, r, found_inf); break;
            case 2: hipLaunchKernelGGL(ema_kernel<2>, grid, block, 0, (hipStream_t)stream, t, r, found_inf); break;
            case 3: hipLaunchKernelGGL(ema_kernel<3>, grid, block, 0, (hipStream_t)stream, t, r, found_inf); break;
            default: hipLaunchKernelGGL(ema_kernel<4>, grid, block, 0, (hipStream_t)stream, t, r, found_inf); break;
        }
    }
    DXMI_CHECK_LAUNCH("dxmi_ema_update");
    return DXMI_OK;
}
