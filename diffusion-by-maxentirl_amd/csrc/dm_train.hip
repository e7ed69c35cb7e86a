// Distribution matching distillation of the EDM teacher into a one-step generator G(z) = D_theta(sigma_G z, sigma_G): Diff-Instruct
// (Luo et al. 2023, eq. 8 / Algorithm 1), DMD (Yin et al. 2023, eq. 7-8) and DMD2 (Yin et al. 2024, eq. 2-3; its GAN term: gan_head.hip).
// The launches between the three network evaluations of one generator step (KarrasDenoiser.dm_generator_losses):
//   dxmi_dm_gen_in     latents -> generator: x_in = c_in(sigma_G) (sigma_G z), time = 250 ln(sigma_G + 1e-44)
//   dxmi_dm_gen_out    generator -> images (sampling): x = c_skip(sigma_G) (sigma_G z) + c_out(sigma_G) F_g, clamped when asked
//   dxmi_dm_gen_prep   generator -> the real and the fake denoiser (training): the same x, t = tab[idx], x_t = x + noise t, the
//                      inputs of both nets and their time, in one launch (F_g, z and noise are read once)
//   dxmi_dm_grad_fwd   after both denoisers: D_r, D_f, s = mean|x - D_r|, g = (D_f - D_r) / s (DMD eq. 8) or D_f - D_r (Diff-Instruct),
//                      loss = 0.5 mean(g^2); one workgroup per image
//   dxmi_dm_gen_bwd    dF_g = upstream c_out(sigma_G) g / CHW: the gradient reaches the generator through x only (DMD eq. 7)
// Conventions of cm_train.hip / pd_train.hip: fp32, one rounding per written operation, 16 bytes per lane, several loads in flight,
// per-sample sums in a fixed order (bitwise reproducible), no atomics.  The level is gathered from the device table of S entries
// (cd_levels) by an int64 index; these launches need only t, so the index S - 1 is legal.  An index outside [0, S - 1] gives a NaN
// level (nothing is read outside the table).
//
// The K-step generator of DMD2 (Yin et al. 2024, section 4.4-4.5: backward simulation; KarrasDenoiser.dm_generator_losses with gen_sigmas):
// the ladder sigma_0 > ... > sigma_{K-1} is a device table of K fp32 entries, image n's graded step an int64 steps[n], gathered by
// ew_level's rule (a step outside [0, K - 1] gives a NaN level for that image; nothing is read outside the ladder).
//   dxmi_dmms_in       latents -> step 0: x = sigma_0 z (kept), x_in = c_in(sigma_0) x, time = 250 ln(sigma_0 + 1e-44)
//   dxmi_dmms_stage    ONE launch between generator evaluations j and j + 1, in place: x' = G_j(x) + sigma_{j+1} eps, x_in =
//                      c_in(sigma_{j+1}) x', its time; an image whose step is <= j is frozen (its rows are neither read nor written),
//                      so after stages 0 .. K-2 x[n] is x_{k_n} and x_in / time are the graded evaluation's operands.  eps is given
//                      or made here (philox_normal.h: the bits of dxmi_randn_indexed)
//   dxmi_dmms_prep     dxmi_dm_gen_prep with x_k for sigma_G z and the image's own sigma_{steps[n]} for sigma_G
//   dxmi_dmms_bwd      dxmi_dm_gen_bwd with c_out(sigma_{steps[n]})
//   dxmi_dmms_out      G_{K-1}, clamped when asked (sampling)
// philox_normal.h stands ahead of the contraction pragma of the two headers below, as in stage_common.h.
#include "philox_normal.h"
#include "dsm_common.h"
#include "ew_common.h"

namespace {

// dm_grad_fwd keeps D_f - D_r of a whole image in registers between its two sums: at most DM_REG_V4 f32x4 (48 fp32 VGPRs) per lane,
// i.e. CHW <= 256 * 4 * DM_REG_V4 = 12288 = 3x64x64, the largest image of the programs here.  A larger image takes the two-pass
// kernel.  (The compiler issues all 48 loads of a lane before the first use: 244 VGPRs + 16 AGPRs, no scratch, one wave per SIMD,
// which one workgroup per image does not feel.)
constexpr int DM_REG_V4 = 12;
constexpr int DM_REG_CHW = EW_BLOCK * 4 * DM_REG_V4;

// EDM scalings of the generator's diffusion at sigma_G (distillation=False)
__device__ __forceinline__ DsmScal dm_gen_scalings(float sg, float sd, float sd2) {
    return dsm_scalings(sg, sd, sd2, 0.f, 0, DXMI_DSM_W_UNIFORM, 0.f);
}

__global__ __launch_bounds__(EW_BLOCK) void dm_gen_in_kernel(const float* __restrict__ z, float* __restrict__ x_in, float* __restrict__ t_out,
                                                             int CHW, float sg, float sd2) {
    const int b = blockIdx.y;
    const float c_in = dsm_c_in(sg, sd2);
    if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = dsm_time(sg);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 zv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u)
            if (i0 + u * EW_BLOCK < n4) zv[u] = ld4(z, base, i0 + u * EW_BLOCK);
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = c_in * (zv[u][e] * sg);
            st4(x_in, base, i, o);
        }
    }
}

// PREP = 0: dxmi_dm_gen_out (x, clamped when asked).  PREP = 1: dxmi_dm_gen_prep (x, x_t and the inputs of the two denoisers).
template <int PREP>
__global__ __launch_bounds__(EW_BLOCK) void dm_gen_x_kernel(const float* __restrict__ Fg, const float* __restrict__ z,
                                                            const float* __restrict__ noise, const int64_t* __restrict__ idx,
                                                            const float* __restrict__ tab, int S, float* __restrict__ x,
                                                            float* __restrict__ x_t, float* __restrict__ x_in_real,
                                                            float* __restrict__ t_out, float* __restrict__ x_in_fake, int CHW, float sg,
                                                            float sd, float sd2, float sd2_real, float sd2_fake, int clip) {
    const int b = blockIdx.y;
    const DsmScal c = dm_gen_scalings(sg, sd, sd2);
    float t = 0.f, cr = 0.f, cf = 0.f;
    if (PREP) {
        t = ew_level(idx, tab, S, b);
        cr = dsm_c_in(t, sd2_real);
        cf = dsm_c_in(t, sd2_fake);
        if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = dsm_time(t);
    }
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 fv[EW_UNROLL], zv[EW_UNROLL], nv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fv[u] = ld4(Fg, base, i);
                zv[u] = ld4(z, base, i);
                if (PREP) nv[u] = ld4(noise, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 xo, xt, ir, jf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = c.c_out * fv[u][e] + c.c_skip * (zv[u][e] * sg);          // denoise() at sigma_G
                if (!PREP && clip) v = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);      // th.clamp(-1, 1): NaN passes
                xo[e] = v;
                if (PREP) {
                    xt[e] = v + nv[u][e] * t;
                    ir[e] = cr * xt[e];
                    jf[e] = cf * xt[e];
                }
            }
            st4(x, base, i, xo);
            if (PREP) {
                st4(x_t, base, i, xt);
                st4(x_in_real, base, i, ir);
                if (x_in_fake) st4(x_in_fake, base, i, jf);
            }
        }
    }
}

// s == 0: the sample sits on the teacher's denoised image already, and the normalised direction does not exist: g = 0
__device__ __forceinline__ float dm_g(float df, float s, int weighting) {
    if (s == 0.f) return 0.f;
    return weighting == DXMI_DM_W_DMD ? df / s : df;
}

// One workgroup per image, the image's D_f - D_r in registers (NV f32x4 per lane): every input is read from memory once.
template <int NV>
__global__ __launch_bounds__(EW_BLOCK) void dm_grad_fwd_reg_kernel(const float* __restrict__ Fr, const float* __restrict__ Ff,
                                                                   const float* __restrict__ x, const float* __restrict__ x_t,
                                                                   const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                                   float* __restrict__ g, float* __restrict__ loss, float* __restrict__ s_out,
                                                                   int CHW, int weighting, float sdr, float sdr2,
                                                                   float smin_r, int dist_r, float sdf, float sdf2, float smin_f, int dist_f) {
    __shared__ float red[2][EW_BLOCK / 64];
    const int b = blockIdx.x;
    const float t = ew_level(idx, tab, S, b);
    const DsmScal cr = dsm_scalings(t, sdr, sdr2, smin_r, dist_r, DXMI_DSM_W_UNIFORM, 0.f);
    const DsmScal cf = dsm_scalings(t, sdf, sdf2, smin_f, dist_f, DXMI_DSM_W_UNIFORM, 0.f);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    f32x4 df[NV];
    float acc = 0.f;
#pragma unroll
    for (int k0 = 0; k0 < NV; k0 += EW_UNROLL) {
        f32x4 fr[EW_UNROLL], ff[EW_UNROLL], xv[EW_UNROLL], xt[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = threadIdx.x + (k0 + u) * EW_BLOCK;
            if (i < n4) {
                fr[u] = ld4(Fr, base, i);
                ff[u] = ld4(Ff, base, i);
                xv[u] = ld4(x, base, i);
                xt[u] = ld4(x_t, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = threadIdx.x + (k0 + u) * EW_BLOCK;
            if (i >= n4) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dr = cr.c_out * fr[u][e] + cr.c_skip * xt[u][e];
                const float dfk = cf.c_out * ff[u][e] + cf.c_skip * xt[u][e];
                df[k0 + u][e] = dfk - dr;
                acc += __builtin_fabsf(xv[u][e] - dr);
            }
        }
    }
    const float s = block_sum(acc, red[0]) / (float)CHW;
    float acc2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = threadIdx.x + k * EW_BLOCK;
        if (i >= n4) continue;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = dm_g(df[k][e], s, weighting);
            acc2 += o[e] * o[e];
        }
        st4(g, base, i, o);
    }
    const float tot2 = block_sum(acc2, red[1]);
    if (threadIdx.x == 0) {
        s_out[b] = s;
        loss[b] = 0.5f * (tot2 / (float)CHW);
    }
}

// The same for an image above the register budget: a second pass over the inputs forms D_f - D_r again (the same operations on
// the same operands: the same bits).
__global__ __launch_bounds__(EW_BLOCK) void dm_grad_fwd_2pass_kernel(const float* __restrict__ Fr, const float* __restrict__ Ff,
                                                                     const float* __restrict__ x, const float* __restrict__ x_t,
                                                                     const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                                     float* __restrict__ g, float* __restrict__ loss, float* __restrict__ s_out,
                                                                     int CHW, int weighting, float sdr, float sdr2, float smin_r, int dist_r,
                                                                     float sdf, float sdf2, float smin_f, int dist_f) {
    __shared__ float red[2][EW_BLOCK / 64];
    const int b = blockIdx.x;
    const float t = ew_level(idx, tab, S, b);
    const DsmScal cr = dsm_scalings(t, sdr, sdr2, smin_r, dist_r, DXMI_DSM_W_UNIFORM, 0.f);
    const DsmScal cf = dsm_scalings(t, sdf, sdf2, smin_f, dist_f, DXMI_DSM_W_UNIFORM, 0.f);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    float acc = 0.f;
    for (int i0 = threadIdx.x; i0 < n4; i0 += EW_BLOCK * EW_UNROLL) {
        f32x4 fr[EW_UNROLL], xv[EW_UNROLL], xt[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fr[u] = ld4(Fr, base, i);
                xv[u] = ld4(x, base, i);
                xt[u] = ld4(x_t, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            if (i0 + u * EW_BLOCK >= n4) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += __builtin_fabsf(xv[u][e] - (cr.c_out * fr[u][e] + cr.c_skip * xt[u][e]));
        }
    }
    const float s = block_sum(acc, red[0]) / (float)CHW;
    float acc2 = 0.f;
    for (int i0 = threadIdx.x; i0 < n4; i0 += EW_BLOCK * EW_UNROLL) {
        f32x4 fr[EW_UNROLL], ff[EW_UNROLL], xt[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fr[u] = ld4(Fr, base, i);
                ff[u] = ld4(Ff, base, i);
                xt[u] = ld4(x_t, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dr = cr.c_out * fr[u][e] + cr.c_skip * xt[u][e];
                const float dfk = cf.c_out * ff[u][e] + cf.c_skip * xt[u][e];
                o[e] = dm_g(dfk - dr, s, weighting);
                acc2 += o[e] * o[e];
            }
            st4(g, base, i, o);
        }
    }
    const float tot2 = block_sum(acc2, red[1]);
    if (threadIdx.x == 0) {
        s_out[b] = s;
        loss[b] = 0.5f * (tot2 / (float)CHW);
    }
}

__global__ __launch_bounds__(EW_BLOCK) void dm_gen_bwd_kernel(const float* __restrict__ up, const float* __restrict__ g,
                                                              float* __restrict__ dF, int CHW, float c_out, float invD) {
    const int b = blockIdx.y;
    const float gs = up[b] * invD;              // mean -> / CHW
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 gv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u)
            if (i0 + u * EW_BLOCK < n4) gv[u] = ld4(g, base, i0 + u * EW_BLOCK);
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (gs * gv[u][e]) * c_out;
            st4(dF, base, i, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- K-step generator
// the generator's level of image b: ladder[steps[b]] by ew_level's rule
__device__ __forceinline__ float dmms_level(const int64_t* __restrict__ steps, const float* __restrict__ sig, int K, int b) {
    return ew_level(steps, sig, K, b);
}

__global__ __launch_bounds__(EW_BLOCK) void dmms_in_kernel(const float* __restrict__ z, const float* __restrict__ sig,
                                                           float* __restrict__ x, float* __restrict__ x_in, float* __restrict__ t_out,
                                                           int CHW, float sd2) {
    const int b = blockIdx.y;
    const float sg = sig[0];
    const float c_in = dsm_c_in(sg, sd2);
    if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = dsm_time(sg);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 zv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u)
            if (i0 + u * EW_BLOCK < n4) zv[u] = ld4(z, base, i0 + u * EW_BLOCK);
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 xo, o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xo[e] = zv[u][e] * sg;
                o[e] = c_in * xo[e];
            }
            st4(x, base, i, xo);
            st4(x_in, base, i, o);
        }
    }
}

// Stage j (0 <= j <= K - 2, checked on the host).  x and x_in are updated in place by the lane that read them.
__global__ __launch_bounds__(EW_BLOCK) void dmms_stage_kernel(const float* __restrict__ F, const float* __restrict__ eps,
                                                              const int64_t* __restrict__ sample_index, uint32_t draw, uint32_t k0,
                                                              uint32_t k1, const int64_t* __restrict__ steps,
                                                              const float* __restrict__ sig, int K, int j, float* x,
                                                              float* __restrict__ x_in, float* __restrict__ t_out, int CHW, float sd,
                                                              float sd2) {
    const int b = blockIdx.y;
    bool ok = true;
    if (steps) {
        const int64_t k = steps[b];
        ok = k >= 0 && k < (int64_t)K;
        if (ok && k <= (int64_t)j) return;                          // frozen: this image's rows are neither read nor written
    }
    const float nan = __builtin_nanf("");
    const float s = ok ? sig[j] : nan, sn = ok ? sig[j + 1] : nan;     // a step outside the ladder poisons the image
    const DsmScal c = dm_gen_scalings(s, sd, sd2);
    const float cn = dsm_c_in(sn, sd2);
    if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = dsm_time(sn);
    uint32_t i_lo = 0, i_hi = 0;
    if (!eps) {
        const uint64_t index = (uint64_t)sample_index[b];
        i_lo = (uint32_t)index, i_hi = (uint32_t)(index >> 32);
    }
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 fv[EW_UNROLL], xv[EW_UNROLL], ev[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fv[u] = ld4(F, base, i);
                xv[u] = ld4(x, base, i);
                if (eps) ev[u] = ld4(eps, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            if (!eps) ev[u] = normals(philox4x32_10((uint32_t)i, draw, i_lo, i_hi, k0, k1));
            f32x4 xo, o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = c.c_out * fv[u][e] + c.c_skip * xv[u][e];           // denoise() at sigma_j, not clamped
                xo[e] = d + ev[u][e] * sn;
                o[e] = cn * xo[e];
            }
            st4(x, base, i, xo);
            st4(x_in, base, i, o);
        }
    }
}

// PREP = 0: dxmi_dmms_out (G_{K-1}, clamped when asked).  PREP = 1: dxmi_dmms_prep.  dm_gen_x_kernel with x_k for sigma_G z and the
// level from the ladder; x may be x_k itself (a lane writes what it read).
template <int PREP>
__global__ __launch_bounds__(EW_BLOCK) void dmms_x_kernel(const float* __restrict__ Fg, const float* xk, const float* __restrict__ noise,
                                                          const int64_t* __restrict__ steps, const float* __restrict__ sig, int K,
                                                          const int64_t* __restrict__ idx, const float* __restrict__ tab, int S, float* x,
                                                          float* __restrict__ x_t, float* __restrict__ x_in_real,
                                                          float* __restrict__ t_out, float* __restrict__ x_in_fake, int CHW, float sd,
                                                          float sd2, float sd2_real, float sd2_fake, int clip) {
    const int b = blockIdx.y;
    const float sg = PREP ? dmms_level(steps, sig, K, b) : sig[K - 1];
    const DsmScal c = dm_gen_scalings(sg, sd, sd2);
    float t = 0.f, cr = 0.f, cf = 0.f;
    if (PREP) {
        t = ew_level(idx, tab, S, b);
        cr = dsm_c_in(t, sd2_real);
        cf = dsm_c_in(t, sd2_fake);
        if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = dsm_time(t);
    }
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 fv[EW_UNROLL], kv[EW_UNROLL], nv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fv[u] = ld4(Fg, base, i);
                kv[u] = ld4(xk, base, i);
                if (PREP) nv[u] = ld4(noise, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 xo, xt, ir, jf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = c.c_out * fv[u][e] + c.c_skip * kv[u][e];                // denoise() at the image's level
                if (!PREP && clip) v = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);      // th.clamp(-1, 1): NaN passes
                xo[e] = v;
                if (PREP) {
                    xt[e] = v + nv[u][e] * t;
                    ir[e] = cr * xt[e];
                    jf[e] = cf * xt[e];
                }
            }
            st4(x, base, i, xo);
            if (PREP) {
                st4(x_t, base, i, xt);
                st4(x_in_real, base, i, ir);
                if (x_in_fake) st4(x_in_fake, base, i, jf);
            }
        }
    }
}

__global__ __launch_bounds__(EW_BLOCK) void dmms_bwd_kernel(const float* __restrict__ up, const float* __restrict__ g,
                                                            const int64_t* __restrict__ steps, const float* __restrict__ sig, int K,
                                                            float* __restrict__ dF, int CHW, float sd, float sd2, float invD) {
    const int b = blockIdx.y;
    const float c_out = dm_gen_scalings(dmms_level(steps, sig, K, b), sd, sd2).c_out;
    const float gs = up[b] * invD;              // mean -> / CHW
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 gv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u)
            if (i0 + u * EW_BLOCK < n4) gv[u] = ld4(g, base, i0 + u * EW_BLOCK);
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (gs * gv[u][e]) * c_out;
            st4(dF, base, i, o);
        }
    }
}

// c_out(sigma_G) with the device's operations, for the backward's scalar
float dm_host_c_out(float sg, float sd) {
    const float den = sg * sg + sd * sd;
    return (sg * sd) / __builtin_sqrtf(den);
}

}  // namespace

extern "C" int dxmi_dm_gen_in(const float* z, float* x_in, float* t_out, int32_t N, int32_t CHW, float gen_sigma, float sigma_data,
                              void* stream) {
    DXMI_CHECK_ARG(z && x_in && t_out, "dxmi_dm_gen_in: null pointer");
    EW_CHECK_SHAPE("dxmi_dm_gen_in");
    EW_CHECK_POS("dxmi_dm_gen_in", gen_sigma, "gen_sigma");
    EW_CHECK_POS("dxmi_dm_gen_in", sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dm_gen_in", z, x_in);
    hipLaunchKernelGGL(dm_gen_in_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, z, x_in, t_out, CHW, gen_sigma,
                       sigma_data * sigma_data);
    DXMI_CHECK_LAUNCH("dxmi_dm_gen_in");
    return DXMI_OK;
}

extern "C" int dxmi_dm_gen_out(const float* f_gen, const float* z, float* x, int32_t N, int32_t CHW, float gen_sigma, float sigma_data,
                               int32_t clip, void* stream) {
    DXMI_CHECK_ARG(f_gen && z && x, "dxmi_dm_gen_out: null pointer");
    EW_CHECK_SHAPE("dxmi_dm_gen_out");
    EW_CHECK_POS("dxmi_dm_gen_out", gen_sigma, "gen_sigma");
    EW_CHECK_POS("dxmi_dm_gen_out", sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dm_gen_out", f_gen, z, x);
    const float sd2 = sigma_data * sigma_data;
    hipLaunchKernelGGL(dm_gen_x_kernel<0>, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, f_gen, z, (const float*)nullptr,
                       (const int64_t*)nullptr, (const float*)nullptr, 0, x, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                       (float*)nullptr, CHW, gen_sigma, sigma_data, sd2, 0.f, 0.f, (int)(clip != 0));
    DXMI_CHECK_LAUNCH("dxmi_dm_gen_out");
    return DXMI_OK;
}

extern "C" int dxmi_dm_gen_prep(const float* f_gen, const float* z, const float* noise, const int64_t* indices, const float* t_table,
                                int32_t num_scales, float* x, float* x_t, float* x_in_real, float* t_out, float* x_in_fake, int32_t N,
                                int32_t CHW, float gen_sigma, float gen_sigma_data, float real_sigma_data, float fake_sigma_data,
                                void* stream) {
    DXMI_CHECK_ARG(f_gen && z && noise && indices && t_table && x && x_t && x_in_real && t_out, "dxmi_dm_gen_prep: null pointer");
    EW_CHECK_SHAPE("dxmi_dm_gen_prep");
    EW_CHECK_SCALES("dxmi_dm_gen_prep");
    EW_CHECK_POS("dxmi_dm_gen_prep", gen_sigma, "gen_sigma");
    EW_CHECK_POS("dxmi_dm_gen_prep", gen_sigma_data, "sigma_data");
    EW_CHECK_POS("dxmi_dm_gen_prep", real_sigma_data, "sigma_data");
    EW_CHECK_POS("dxmi_dm_gen_prep", fake_sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dm_gen_prep", f_gen, z, noise, x, x_t, x_in_real, x_in_fake);
    hipLaunchKernelGGL(dm_gen_x_kernel<1>, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, f_gen, z, noise, indices, t_table,
                       num_scales, x, x_t, x_in_real, t_out, x_in_fake, CHW, gen_sigma, gen_sigma_data, gen_sigma_data * gen_sigma_data,
                       real_sigma_data * real_sigma_data, fake_sigma_data * fake_sigma_data, 0);
    DXMI_CHECK_LAUNCH("dxmi_dm_gen_prep");
    return DXMI_OK;
}

extern "C" int dxmi_dm_grad_fwd(const float* f_real, const float* f_fake, const float* x, const float* x_t, const int64_t* indices,
                                const float* t_table, int32_t num_scales, float* g, float* loss, float* s, int32_t N, int32_t CHW,
                                int32_t weighting, float real_sigma_data, float real_sigma_min, int32_t real_distillation,
                                float fake_sigma_data, float fake_sigma_min, int32_t fake_distillation, void* stream) {
    DXMI_CHECK_ARG(f_real && f_fake && x && x_t && indices && t_table && g && loss && s, "dxmi_dm_grad_fwd: null pointer");
    EW_CHECK_SHAPE("dxmi_dm_grad_fwd");
    EW_CHECK_SCALES("dxmi_dm_grad_fwd");
    DXMI_CHECK_ARG(weighting == DXMI_DM_W_DMD || weighting == DXMI_DM_W_NONE, "dxmi_dm_grad_fwd: unknown weighting %d", weighting);
    EW_CHECK_POS("dxmi_dm_grad_fwd", real_sigma_data, "sigma_data");
    EW_CHECK_POS("dxmi_dm_grad_fwd", fake_sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dm_grad_fwd", f_real, f_fake, x, x_t, g);
    const dim3 grid(N), block(EW_BLOCK);
    const float sdr2 = real_sigma_data * real_sigma_data, sdf2 = fake_sigma_data * fake_sigma_data;
    const int dr = (int)(real_distillation != 0), df = (int)(fake_distillation != 0);
    if (CHW <= EW_BLOCK * 4 * 4)
        hipLaunchKernelGGL(dm_grad_fwd_reg_kernel<4>, grid, block, 0, (hipStream_t)stream, f_real, f_fake, x, x_t, indices, t_table,
                           num_scales, g, loss, s, CHW, weighting, real_sigma_data, sdr2, real_sigma_min, dr, fake_sigma_data, sdf2,
                           fake_sigma_min, df);
    else if (CHW <= DM_REG_CHW)
        hipLaunchKernelGGL(dm_grad_fwd_reg_kernel<DM_REG_V4>, grid, block, 0, (hipStream_t)stream, f_real, f_fake, x, x_t, indices, t_table,
                           num_scales, g, loss, s, CHW, weighting, real_sigma_data, sdr2, real_sigma_min, dr, fake_sigma_data, sdf2,
                           fake_sigma_min, df);
    else
        hipLaunchKernelGGL(dm_grad_fwd_2pass_kernel, grid, block, 0, (hipStream_t)stream, f_real, f_fake, x, x_t, indices, t_table,
                           num_scales, g, loss, s, CHW, weighting, real_sigma_data, sdr2, real_sigma_min, dr, fake_sigma_data, sdf2,
                           fake_sigma_min, df);
    DXMI_CHECK_LAUNCH("dxmi_dm_grad_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_dm_gen_bwd(const float* upstream, const float* g, float* d_f_gen, int32_t N, int32_t CHW, float gen_sigma,
                               float sigma_data, void* stream) {
    DXMI_CHECK_ARG(upstream && g && d_f_gen, "dxmi_dm_gen_bwd: null pointer");
    EW_CHECK_SHAPE("dxmi_dm_gen_bwd");
    EW_CHECK_POS("dxmi_dm_gen_bwd", gen_sigma, "gen_sigma");
    EW_CHECK_POS("dxmi_dm_gen_bwd", sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dm_gen_bwd", g, d_f_gen);
    hipLaunchKernelGGL(dm_gen_bwd_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, upstream, g, d_f_gen, CHW,
                       dm_host_c_out(gen_sigma, sigma_data), (float)(1.0 / (double)CHW));
    DXMI_CHECK_LAUNCH("dxmi_dm_gen_bwd");
    return DXMI_OK;
}

// ---------------------------------------------------------------------------------------------------- K-step generator
// the ladder: K fp32 levels on the device; steps: one int64 per image
#define DMMS_CHECK_LADDER(fn)                                                                                                    \
    DXMI_CHECK_ARG(num_steps >= 1 && num_steps < (1 << 30), fn ": num_steps (%d) must be in [1, 2^30)", num_steps);              \
    DXMI_CHECK_ARG((((uintptr_t)gen_sigmas) & 3) == 0, fn ": gen_sigmas must be 4-byte aligned")
#define DMMS_CHECK_STEPS(fn) DXMI_CHECK_ARG((((uintptr_t)steps) & 7) == 0, fn ": steps must be 8-byte aligned")

extern "C" int dxmi_dmms_in(const float* z, const float* gen_sigmas, int32_t num_steps, float* x, float* x_in, float* t_out, int32_t N,
                            int32_t CHW, float sigma_data, void* stream) {
    DXMI_CHECK_ARG(z && gen_sigmas && x && x_in && t_out, "dxmi_dmms_in: null pointer");
    EW_CHECK_SHAPE("dxmi_dmms_in");
    DMMS_CHECK_LADDER("dxmi_dmms_in");
    EW_CHECK_POS("dxmi_dmms_in", sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dmms_in", z, x, x_in);
    hipLaunchKernelGGL(dmms_in_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, z, gen_sigmas, x, x_in, t_out, CHW,
                       sigma_data * sigma_data);
    DXMI_CHECK_LAUNCH("dxmi_dmms_in");
    return DXMI_OK;
}

extern "C" int dxmi_dmms_stage(const float* f_gen, const float* eps, const int64_t* sample_index, uint32_t draw, uint64_t seed,
                               const int64_t* steps, const float* gen_sigmas, int32_t num_steps, int32_t stage, float* x, float* x_in,
                               float* t_out, int32_t N, int32_t CHW, float sigma_data, void* stream) {
    DXMI_CHECK_ARG(f_gen && gen_sigmas && x && x_in && t_out, "dxmi_dmms_stage: null pointer");
    DXMI_CHECK_ARG(!(eps && sample_index), "dxmi_dmms_stage: noise is either given (eps) or made here (sample_index), not both");
    DXMI_CHECK_ARG(eps || sample_index, "dxmi_dmms_stage: noise is needed: eps, or sample_index to make it here");
    EW_CHECK_SHAPE("dxmi_dmms_stage");
    DMMS_CHECK_LADDER("dxmi_dmms_stage");
    DXMI_CHECK_ARG(stage >= 0 && stage < num_steps - 1, "dxmi_dmms_stage: stage (%d) must be in [0, num_steps - 2 = %d]", stage,
                   num_steps - 2);
    DMMS_CHECK_STEPS("dxmi_dmms_stage");
    DXMI_CHECK_ARG((((uintptr_t)sample_index) & 7) == 0, "dxmi_dmms_stage: sample_index must be 8-byte aligned");
    EW_CHECK_POS("dxmi_dmms_stage", sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dmms_stage", f_gen, eps, x, x_in);
    hipLaunchKernelGGL(dmms_stage_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, f_gen, eps, sample_index, draw,
                       (uint32_t)seed, (uint32_t)(seed >> 32), steps, gen_sigmas, num_steps, stage, x, x_in, t_out, CHW, sigma_data,
                       sigma_data * sigma_data);
    DXMI_CHECK_LAUNCH("dxmi_dmms_stage");
    return DXMI_OK;
}

extern "C" int dxmi_dmms_prep(const float* f_gen, const float* x_k, const float* noise, const int64_t* steps, const float* gen_sigmas,
                              int32_t num_steps, const int64_t* indices, const float* t_table, int32_t num_scales, float* x, float* x_t,
                              float* x_in_real, float* t_out, float* x_in_fake, int32_t N, int32_t CHW, float gen_sigma_data,
                              float real_sigma_data, float fake_sigma_data, void* stream) {
    DXMI_CHECK_ARG(f_gen && x_k && noise && steps && gen_sigmas && indices && t_table && x && x_t && x_in_real && t_out,
                   "dxmi_dmms_prep: null pointer");
    EW_CHECK_SHAPE("dxmi_dmms_prep");
    DMMS_CHECK_LADDER("dxmi_dmms_prep");
    DMMS_CHECK_STEPS("dxmi_dmms_prep");
    EW_CHECK_SCALES("dxmi_dmms_prep");
    EW_CHECK_POS("dxmi_dmms_prep", gen_sigma_data, "sigma_data");
    EW_CHECK_POS("dxmi_dmms_prep", real_sigma_data, "sigma_data");
    EW_CHECK_POS("dxmi_dmms_prep", fake_sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dmms_prep", f_gen, x_k, noise, x, x_t, x_in_real, x_in_fake);
    hipLaunchKernelGGL(dmms_x_kernel<1>, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, f_gen, x_k, noise, steps, gen_sigmas,
                       num_steps, indices, t_table, num_scales, x, x_t, x_in_real, t_out, x_in_fake, CHW, gen_sigma_data,
                       gen_sigma_data * gen_sigma_data, real_sigma_data * real_sigma_data, fake_sigma_data * fake_sigma_data, 0);
    DXMI_CHECK_LAUNCH("dxmi_dmms_prep");
    return DXMI_OK;
}

extern "C" int dxmi_dmms_out(const float* f_gen, const float* x_k, const float* gen_sigmas, int32_t num_steps, float* x, int32_t N,
                             int32_t CHW, float sigma_data, int32_t clip, void* stream) {
    DXMI_CHECK_ARG(f_gen && x_k && gen_sigmas && x, "dxmi_dmms_out: null pointer");
    EW_CHECK_SHAPE("dxmi_dmms_out");
    DMMS_CHECK_LADDER("dxmi_dmms_out");
    EW_CHECK_POS("dxmi_dmms_out", sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dmms_out", f_gen, x_k, x);
    hipLaunchKernelGGL(dmms_x_kernel<0>, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, f_gen, x_k, (const float*)nullptr,
                       (const int64_t*)nullptr, gen_sigmas, num_steps, (const int64_t*)nullptr, (const float*)nullptr, 0, x,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, CHW, sigma_data, sigma_data * sigma_data, 0.f,
                       0.f, (int)(clip != 0));
    DXMI_CHECK_LAUNCH("dxmi_dmms_out");
    return DXMI_OK;
}

extern "C" int dxmi_dmms_bwd(const float* upstream, const float* g, const int64_t* steps, const float* gen_sigmas, int32_t num_steps,
                             float* d_f_gen, int32_t N, int32_t CHW, float sigma_data, void* stream) {
    DXMI_CHECK_ARG(upstream && g && steps && gen_sigmas && d_f_gen, "dxmi_dmms_bwd: null pointer");
    EW_CHECK_SHAPE("dxmi_dmms_bwd");
    DMMS_CHECK_LADDER("dxmi_dmms_bwd");
    DMMS_CHECK_STEPS("dxmi_dmms_bwd");
    EW_CHECK_POS("dxmi_dmms_bwd", sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_dmms_bwd", g, d_f_gen);
    hipLaunchKernelGGL(dmms_bwd_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, upstream, g, steps, gen_sigmas,
                       num_steps, d_f_gen, CHW, sigma_data, sigma_data * sigma_data, (float)(1.0 / (double)CHW));
    DXMI_CHECK_LAUNCH("dxmi_dmms_bwd");
    return DXMI_OK;
}
