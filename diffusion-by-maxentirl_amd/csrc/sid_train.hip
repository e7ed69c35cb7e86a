// Score identity Distillation of the EDM teacher into the one-step generator of dm_train.hip (SiD: Zhou, Zheng, Wang, Yin, Huang,
// "Score identity Distillation: Exponentially Fast Distillation of Pretrained Diffusion Models for One-Step Generation", ICML
// 2024: its fused generator loss L~_theta^(alpha) = L^(2) - alpha L^(1); in its released code (github.com/mingyuanzhou/SiD) the
// generator's loss (y_real - y_fake) * ((y_real - y) - alpha (y_real - y_fake)) / weight_factor).  Unlike the DMD gradient of dm_grad_fwd the loss
// is differentiated THROUGH both denoisers with respect to their input x_t; no parameter of either receives a gradient.  The two
// launches around the two input-only backward walks (models.cm.unet_train.input_forward / input_backward) of one generator step
// (KarrasDenoiser.sid_generator_losses), with delta = D_r - D_f, e = D_f - x and s = mean|x - D_r| under stop-gradient:
//   dxmi_sid_grad_fwd  after both forwards: loss = ((1 - alpha) sum(delta^2) + sum(delta e)) / (CHW s), and with
//                      a_r = 2 (1 - alpha) delta + e = dL/dD_r and a_f = (2 alpha - 1) delta - e = dL/dD_f (both times CHW s)
//                      the cotangents v_r = c_out_r a_r on F_r and v_f = c_out_f a_f on F_f, and the paths to x that pass through
//                      no network, d_dir = (c_skip_r a_r + c_skip_f a_f) - delta: all three WITHOUT the 1 / s
//   dxmi_sid_join      after both backwards: g = ((d_dir + c_in_r g_r) + c_in_f g_f) / s, d loss_n / d x = g_n / CHW: the operand
//                      of dxmi_dm_gen_bwd
// Nothing written per element needs the image's sums (1 / s is applied once, in the join: the nets are linear in their cotangent),
// and the loss needs only the three sums and one division, so ONE pass over the operands does all of it at every image size: each
// of F_r, F_f, x and x_t is read once, and no image-sized state is kept in registers (dm_grad_fwd has to keep D_f - D_r because
// its g is divided by s element by element).
// Conventions of dm_train.hip: fp32, one rounding per written operation, 16 bytes per lane, several loads in flight, one workgroup
// per image in dxmi_sid_grad_fwd, per-sample sums in a fixed order (bitwise reproducible), no atomics.  An index outside
// [0, S - 1] gives a NaN level (nothing is read outside the table).  s == 0 gives loss = 0 and g = 0 (SiD's code clips the
// normaliser at 1e-5 instead).
#include "dsm_common.h"
#include "ew_common.h"

namespace {

__global__ __launch_bounds__(EW_BLOCK) void sid_grad_fwd_kernel(const float* __restrict__ Fr, const float* __restrict__ Ff,
                                                                const float* __restrict__ x, const float* __restrict__ x_t,
                                                                const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                                float* __restrict__ v_r, float* __restrict__ v_f,
                                                                float* __restrict__ d_dir, float* __restrict__ loss,
                                                                float* __restrict__ s_out, int CHW, float oma, float k_r, float k_f,
                                                                float sdr, float sdr2, float smin_r, int dist_r, float sdf, float sdf2,
                                                                float smin_f, int dist_f) {
    __shared__ float red[3][EW_BLOCK / 64];
    const int b = blockIdx.x;
    const float t = ew_level(idx, tab, S, b);
    const DsmScal cr = dsm_scalings(t, sdr, sdr2, smin_r, dist_r, DXMI_DSM_W_UNIFORM, 0.f);
    const DsmScal cf = dsm_scalings(t, sdf, sdf2, smin_f, dist_f, DXMI_DSM_W_UNIFORM, 0.f);
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    float acc_s = 0.f, acc_a = 0.f, acc_b = 0.f;
    for (int i0 = threadIdx.x; i0 < n4; i0 += EW_BLOCK * EW_UNROLL) {
        f32x4 fr[EW_UNROLL], ff[EW_UNROLL], xv[EW_UNROLL], xt[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                fr[u] = ld4(Fr, base, i);
                ff[u] = ld4(Ff, base, i);
                xv[u] = ld4(x, base, i);
                xt[u] = ld4(x_t, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 ovr, ovf, od;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dr = cr.c_out * fr[u][e] + cr.c_skip * xt[u][e];
                const float dfk = cf.c_out * ff[u][e] + cf.c_skip * xt[u][e];
                const float delta = dr - dfk;
                const float ex = dfk - xv[u][e];
                const float ar = k_r * delta + ex;
                const float af = k_f * delta - ex;
                ovr[e] = cr.c_out * ar;
                ovf[e] = cf.c_out * af;
                od[e] = (cr.c_skip * ar + cf.c_skip * af) - delta;
                acc_s += __builtin_fabsf(xv[u][e] - dr);
                acc_a += delta * delta;
                acc_b += delta * ex;
            }
            st4(v_r, base, i, ovr);
            st4(v_f, base, i, ovf);
            st4(d_dir, base, i, od);
        }
    }
    const float s = block_sum(acc_s, red[0]) / (float)CHW;
    const float A = block_sum(acc_a, red[1]);
    const float B = block_sum(acc_b, red[2]);
    if (threadIdx.x == 0) {
        s_out[b] = s;
        loss[b] = s == 0.f ? 0.f : (oma * A + B) / ((float)CHW * s);
    }
}

// g may alias d_dir: every lane reads its own elements before it writes them
__global__ __launch_bounds__(EW_BLOCK) void sid_join_kernel(const float* d_dir, const float* __restrict__ g_r,
                                                            const float* __restrict__ g_f, const float* __restrict__ s_in,
                                                            const int64_t* __restrict__ idx, const float* __restrict__ tab, int S,
                                                            float* g, int CHW, float sdr2, float sdf2) {
    const int b = blockIdx.y;
    const float t = ew_level(idx, tab, S, b);
    const float ci_r = dsm_c_in(t, sdr2), ci_f = dsm_c_in(t, sdf2);
    const float s = s_in[b];
    const size_t base = (size_t)b * CHW;
    const int n4 = CHW / 4;
    for (int i0 = blockIdx.x * EW_BLOCK * EW_UNROLL + threadIdx.x; i0 < n4; i0 += gridDim.x * EW_BLOCK * EW_UNROLL) {
        f32x4 dv[EW_UNROLL], rv[EW_UNROLL], fv[EW_UNROLL];
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i < n4) {
                dv[u] = ld4(d_dir, base, i);
                rv[u] = ld4(g_r, base, i);
                fv[u] = ld4(g_f, base, i);
            }
        }
#pragma unroll
        for (int u = 0; u < EW_UNROLL; ++u) {
            const int i = i0 + u * EW_BLOCK;
            if (i >= n4) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = s == 0.f ? 0.f : ((dv[u][e] + ci_r * rv[u][e]) + ci_f * fv[u][e]) / s;
            st4(g, base, i, o);
        }
    }
}

}  // namespace

extern "C" int dxmi_sid_grad_fwd(const float* f_real, const float* f_fake, const float* x, const float* x_t, const int64_t* indices,
                                 const float* t_table, int32_t num_scales, float alpha, float* v_real, float* v_fake, float* d_dir,
                                 float* loss, float* s, int32_t N, int32_t CHW, float real_sigma_data, float real_sigma_min,
                                 int32_t real_distillation, float fake_sigma_data, float fake_sigma_min, int32_t fake_distillation,
                                 void* stream) {
    DXMI_CHECK_ARG(f_real && f_fake && x && x_t && indices && t_table && v_real && v_fake && d_dir && loss && s,
                   "dxmi_sid_grad_fwd: null pointer");
    EW_CHECK_SHAPE("dxmi_sid_grad_fwd");
    EW_CHECK_SCALES("dxmi_sid_grad_fwd");
    DXMI_CHECK_ARG(alpha >= -3.0e38f && alpha <= 3.0e38f, "dxmi_sid_grad_fwd: alpha (%g) must be finite", (double)alpha);
    EW_CHECK_POS("dxmi_sid_grad_fwd", real_sigma_data, "sigma_data");
    EW_CHECK_POS("dxmi_sid_grad_fwd", fake_sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_sid_grad_fwd", f_real, f_fake, x, x_t, v_real, v_fake, d_dir);
    const float oma = 1.f - alpha;
    hipLaunchKernelGGL(sid_grad_fwd_kernel, dim3(N), dim3(EW_BLOCK), 0, (hipStream_t)stream, f_real, f_fake, x, x_t, indices, t_table,
                       num_scales, v_real, v_fake, d_dir, loss, s, CHW, oma, 2.f * oma, 2.f * alpha - 1.f, real_sigma_data,
                       real_sigma_data * real_sigma_data, real_sigma_min, (int)(real_distillation != 0), fake_sigma_data,
                       fake_sigma_data * fake_sigma_data, fake_sigma_min, (int)(fake_distillation != 0));
    DXMI_CHECK_LAUNCH("dxmi_sid_grad_fwd");
    return DXMI_OK;
}

extern "C" int dxmi_sid_join(const float* d_dir, const float* g_real, const float* g_fake, const float* s, const int64_t* indices,
                             const float* t_table, int32_t num_scales, float* g, int32_t N, int32_t CHW, float real_sigma_data,
                             float fake_sigma_data, void* stream) {
    DXMI_CHECK_ARG(d_dir && g_real && g_fake && s && indices && t_table && g, "dxmi_sid_join: null pointer");
    EW_CHECK_SHAPE("dxmi_sid_join");
    EW_CHECK_SCALES("dxmi_sid_join");
    EW_CHECK_POS("dxmi_sid_join", real_sigma_data, "sigma_data");
    EW_CHECK_POS("dxmi_sid_join", fake_sigma_data, "sigma_data");
    EW_CHECK_ALIGNED("dxmi_sid_join", d_dir, g_real, g_fake, g);
    DXMI_CHECK_ARG(g != g_real && g != g_fake, "dxmi_sid_join: g may alias d_dir only");
    hipLaunchKernelGGL(sid_join_kernel, ew_grid(N, CHW), dim3(EW_BLOCK), 0, (hipStream_t)stream, d_dir, g_real, g_fake, s, indices,
                       t_table, num_scales, g, CHW, real_sigma_data * real_sigma_data, fake_sigma_data * fake_sigma_data);
    DXMI_CHECK_LAUNCH("dxmi_sid_join");
    return DXMI_OK;
}
