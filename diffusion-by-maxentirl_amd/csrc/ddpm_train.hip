// Noise-prediction training of the DDPM U-Net (Ho et al. 2020, "Denoising Diffusion Probabilistic Models": the forward process
// q(x_t | x_0) of eq. 4 and the simplified objective L_simple of eq. 14), on the linear-beta tables of
// models/DxMI/var_sampler.py calc_diffusion_hyperparams.
//   dxmi_ddpm_prep      x_t = sqrt(alpha_bar_t) x_start + sqrt(1 - alpha_bar_t) noise and the network's time input, one launch
//   dxmi_ddpm_loss_fwd  per sample mean_flat((eps_pred - noise)^2)
//   dxmi_ddpm_loss_bwd  d eps_pred of that term, the upstream gradient read from device memory
// All three are HBM-bound: one workgroup row per image, 16 bytes per lane, several loads in flight per wave; the per-sample sum is
// reduced in a fixed order (bitwise reproducible).  The two coefficients are gathered from one small device table by index; an
// index outside [0, T) gives NaN coefficients (nothing is read outside the table).
#include "ew_common.h"

namespace {

__global__ __launch_bounds__(EW_BLOCK) void ddpm_prep_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                             const int64_t* __restrict__ t_idx, const float* __restrict__ table,
                                                             int T, float* __restrict__ x_t, float* __restrict__ t_out, int CHW) {
    const int b = blockIdx.y;
    const int64_t t = t_idx[b];
    const bool ok = t >= 0 && t < (int64_t)T;
    const int64_t tc = ok ? t : 0;                  // the read is clamped, the value is not
    const float ta = table[tc], tb = table[(int64_t)T + tc];
    const float ca = ok ? ta : __builtin_nanf(""), cb = ok ? tb : __builtin_nanf("");
    if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = (float)t;
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
                const float px = ca * xv[u][e], pn = cb * nv[u][e];     // two products, one sum
                o[e] = px + pn;
            }
            st4(x_t, base, i, o);
        }
    }
}

// One workgroup per sample: each lane sums its elements in index order, then block_sum.
__global__ __launch_bounds__(EW_BLOCK) void ddpm_loss_fwd_kernel(const float* __restrict__ eps, const float* __restrict__ noise,
                                                                 float* __restrict__ loss, int CHW) {
    __shared__ float red[EW_BLOCK / 64];
    const int b = blockIdx.x;
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    float acc = 0.f;
    for (int i0 = threadIdx.x; i0 < n4; i0 += EW_BLOCK * EW_UNROLL) {
        f32x4 ev[EW_UNROLL], nv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                ev[u] = ld4(eps, base, i);
                nv[u] = ld4(noise, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = ev[u][e] - nv[u][e];
                acc += d * d;                               // (eps_pred - noise) ** 2
            }
        }
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) loss[b] = tot / (float)CHW;       // mean_flat
}

// autograd of ((a - b) ** 2).mean(dim), node by node: mean -> g / D; pow(., 2) -> . * (2 e).
__global__ __launch_bounds__(EW_BLOCK) void ddpm_loss_bwd_kernel(const float* __restrict__ g_loss, const float* __restrict__ eps,
                                                                 const float* __restrict__ noise, float* __restrict__ d_eps, int CHW) {
    const int b = blockIdx.y;
    const float g = g_loss[b] / (float)CHW;
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 ev[EW_UNROLL], nv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                ev[u] = ld4(eps, base, i);
                nv[u] = ld4(noise, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = g * (2.f * (ev[u][e] - nv[u][e]));
            st4(d_eps, base, i, o);
        }
    }
}

}  // namespace

extern "C" int dxmi_ddpm_prep(const float* x_start, const float* noise, const int64_t* t_idx, const float* table, int32_t T,
                              float* x_t, float* t_out, int32_t N, int32_t CHW, void* stream) {
    DXMI_CHECK_ARG(x_start && noise && t_idx && table && x_t && t_out, "dxmi_ddpm_prep: null pointer");
    EW_CHECK_SHAPE("dxmi_ddpm_prep");
    DXMI_CHECK_ARG(T >= 1, "dxmi_ddpm_prep: T (%d) must be at least 1", T);
    EW_CHECK_ALIGNED("dxmi_ddpm_prep", x_start, noise, x_t);
    hipLaunchKernelGGL(ddpm_prep_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, x_start, noise, t_idx, table,
                       (int)T, x_t, t_out, CHW);
    DXMI_CHECK_LAUNCH("dxmi_ddpm_prep");
    return DXMI_OK;
}

extern "C" int dxmi_ddpm_loss_fwd(const float* eps_pred, const float* noise, float* loss, int32_t N, int32_t CHW, void* stream) {
    DXMI_CHECK_ARG(eps_pred && noise && loss, "dxmi_ddpm_loss_fwd: null pointer");
    EW_CHECK_SHAPE("dxmi_ddpm_loss_fwd");
    EW_CHECK_ALIGNED("dxmi_ddpm_loss_fwd", eps_pred, noise);
    hipLaunchKernelGGL(ddpm_loss_fwd_kernel, dim3(N), dim3(EW_BLOCK), 0, (hipStream_t)stream, eps_pred, noise, loss, CHW);
    DXMI_CHECK_LAUNCH("dxmi_ddpm_loss_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_ddpm_loss_bwd(const float* g_loss, const float* eps_pred, const float* noise, float* d_eps, int32_t N,
                                  int32_t CHW, void* stream) {
    DXMI_CHECK_ARG(g_loss && eps_pred && noise && d_eps, "dxmi_ddpm_loss_bwd: null pointer");
    EW_CHECK_SHAPE("dxmi_ddpm_loss_bwd");
    EW_CHECK_ALIGNED("dxmi_ddpm_loss_bwd", eps_pred, noise, d_eps);
    hipLaunchKernelGGL(ddpm_loss_bwd_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, g_loss, eps_pred, noise, d_eps,
                       CHW);
    DXMI_CHECK_LAUNCH("dxmi_ddpm_loss_bwd");
    return DXMI_OK;
}
