// Consistency-model sampling and zero-shot editing (reference models/cm/karras_diffusion.py: sample_onestep :644-655,
// stochastic_iterative_sampler :658-683, iterative_colorization / _inpainting / _superres :722-951): ONE launch between two
// network evaluations.  With F the output just computed at noise level t, each launch forms denoised = c_out F + c_skip x
// (boundary-condition or plain scalings, as the host table says), clamps it, applies the editing replacement against the
// fixed reference view, adds the next step's noise z sqrt(next_t^2 - t_min^2) and writes the next evaluation's input
// c_in(next_t) x' and time 250 ln(next_t + 1e-44), or, after the last evaluation, the final output.  Every per-step scalar
// comes from a small fp32 table built once per schedule on the host (models/cm/karras_diffusion.py, CMSchedule).
#include "common.h"

// the reference's fp32 operation order, one rounding per torch op: no fused multiply-add between them
#pragma clang fp contract(off)

namespace {

constexpr int PATCH = 8, PD = PATCH * PATCH;     // iterative_superres: 8x8 patches, a 64-dim orthogonal basis per patch
constexpr int PATCHES_PER_BLOCK = 16;            // 16 threads per patch, each owns 4 contiguous in-patch indices d = 4j..4j+3

__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }   // NaN passes, as torch.clamp

struct Row {
    float c_skip, c_out, noise, c_in, t, x_scale;
    bool clip, out_clamp;
};

__device__ __forceinline__ Row load_row(const float* __restrict__ r) {
    Row w;
    w.c_skip = r[DXMI_CT_CSKIP];
    w.c_out = r[DXMI_CT_COUT];
    w.noise = r[DXMI_CT_NOISE];
    w.c_in = r[DXMI_CT_CIN];
    w.t = r[DXMI_CT_T];
    w.x_scale = r[DXMI_CT_XSCALE];
    w.clip = r[DXMI_CT_CLIP] != 0.f;
    w.out_clamp = r[DXMI_CT_OUTCLAMP] != 0.f;
    return w;
}

// denoise() (:348-351) and the clamp (clip_denoised :408-412; the editing loops' th.clamp)
__device__ __forceinline__ f32x4 denoise4(const Row& w, f32x4 f, f32x4 x) {
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        d[e] = w.c_out * f[e] + w.c_skip * x[e];
        if (w.clip) d[e] = clamp1(d[e]);
    }
    return d;
}

// x' = x0 + z sqrt(next_t^2 - t_min^2), then either the next input (x, x_in) or the output.  noise NULL: z = 0 (not drawn).
__device__ __forceinline__ void finish4(const Row& w, int last, f32x4 x0, const float* __restrict__ noise, float* x,
                                        float* __restrict__ x_in, float* __restrict__ out, size_t o) {
    f32x4 xn = x0;
    if (noise) {
        const f32x4 z = *reinterpret_cast<const f32x4*>(noise + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) xn[e] = x0[e] + z[e] * w.noise;
    }
    if (last) {
        if (w.out_clamp) {                                                     // karras_sample's x_0.clamp(-1, 1) (:420)
#pragma unroll
            for (int e = 0; e < 4; ++e) xn[e] = clamp1(xn[e]);
        }
        *reinterpret_cast<f32x4*>(out + o) = xn;
        return;
    }
    *reinterpret_cast<f32x4*>(x + o) = xn;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = w.c_in * xn[e];
    *reinterpret_cast<f32x4*>(x_in + o) = v;
}

// FIRST, NONE and MASK: element-wise over each image's C*H*W values
__global__ __launch_bounds__(256) void cm_elementwise_kernel(int mode, int edit, int last, const float* __restrict__ row, float* x,
                                                             const float* __restrict__ F, const float* __restrict__ noise,
                                                             const float* __restrict__ ref, const float* __restrict__ mask,
                                                             float* __restrict__ x_in, float* __restrict__ t_out,
                                                             float* __restrict__ out, float* __restrict__ denoised_out, int CHW) {
    const int b = blockIdx.y;
    const Row w = load_row(row);
    if (!last && blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = w.t;
    const size_t base = (size_t)b * CHW;
    for (int i = (blockIdx.x * 256 + threadIdx.x) * 4; i < CHW; i += gridDim.x * 256 * 4) {
        const size_t o = base + i;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + o);
        if (mode == DXMI_CM_FIRST) {                                           // x_T = randn * sigma_max
            f32x4 xn, v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xn[e] = xv[e] * w.x_scale;
                v[e] = w.c_in * xn[e];
            }
            *reinterpret_cast<f32x4*>(x + o) = xn;
            *reinterpret_cast<f32x4*>(x_in + o) = v;
            continue;
        }
        f32x4 x0 = denoise4(w, *reinterpret_cast<const f32x4*>(F + o), xv);
        if (denoised_out) *reinterpret_cast<f32x4*>(denoised_out + o) = x0;
        if (edit == DXMI_CM_EDIT_MASK) {                                       // iterative_inpainting's replacement (:803-805)
            const f32x4 r = *reinterpret_cast<const f32x4*>(ref + o);
            const f32x4 m = *reinterpret_cast<const f32x4*>(mask + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) x0[e] = r[e] * m[e] + x0[e] * (1.f - m[e]);
        }
        finish4(w, last, x0, noise, x, x_in, out, o);
    }
}

// COLOUR: per pixel y = x^T Q over the three channel planes; coefficient 0 (luma) from ref, 1-2 from x0; back with Q (:737-746)
__global__ __launch_bounds__(256) void cm_colour_kernel(int last, const float* __restrict__ row, const float* __restrict__ Qg,
                                                        float* x, const float* __restrict__ F, const float* __restrict__ noise,
                                                        const float* __restrict__ ref, float* __restrict__ x_in,
                                                        float* __restrict__ t_out, float* __restrict__ out,
                                                        float* __restrict__ denoised_out, int HW) {
    const int b = blockIdx.y;
    const Row w = load_row(row);
    float Q[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) Q[c][d] = Qg[c * 3 + d];
    if (!last && blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = w.t;
    const size_t base = (size_t)b * 3 * HW;
    for (int i = (blockIdx.x * 256 + threadIdx.x) * 4; i < HW; i += gridDim.x * 256 * 4) {
        f32x4 x0[3], r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t o = base + (size_t)c * HW + i;
            x0[c] = denoise4(w, *reinterpret_cast<const f32x4*>(F + o), *reinterpret_cast<const f32x4*>(x + o));
            if (denoised_out) *reinterpret_cast<f32x4*>(denoised_out + o) = x0[c];
            r[c] = *reinterpret_cast<const f32x4*>(ref + o);
        }
        f32x4 y[3];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            y[0][e] = r[0][e] * Q[0][0] + r[1][e] * Q[1][0] + r[2][e] * Q[2][0];
#pragma unroll
            for (int d = 1; d < 3; ++d) y[d][e] = x0[0][e] * Q[0][d] + x0[1][e] * Q[1][d] + x0[2][e] * Q[2][d];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = y[0][e] * Q[c][0] + y[1][e] * Q[c][1] + y[2][e] * Q[c][2];
            finish4(w, last, v, noise, x, x_in, out, base + (size_t)c * HW + i);
        }
    }
}

// PATCH: per 8x8 patch of each channel plane, y = v^T Q with the 64x64 Q; coefficient 0 from ref, 1..63 from x0; back with Q
// (:858-900).  In-patch index d = 8 row + col (the reference's permute(0,1,2,4,3,5) flattening).  A block takes 16 patches at a
// time; thread j of a patch owns d = 4j..4j+3, i.e. row j/2, columns 4(j%2)..+3: one f32x4 access per tensor.  Q and Q^T sit in
// LDS; the f32x4 reads of a Q row by the 16 threads of a patch are contiguous, and the patches of a block read the same rows
// (broadcast), so the reads are conflict-free.
__global__ __launch_bounds__(256) void cm_patch_kernel(int last, const float* __restrict__ row, const float* __restrict__ Qg,
                                                       float* x, const float* __restrict__ F, const float* __restrict__ noise,
                                                       const float* __restrict__ ref, float* __restrict__ x_in,
                                                       float* __restrict__ t_out, float* __restrict__ out,
                                                       float* __restrict__ denoised_out, int N, int H, int W, long long n_patch) {
    __shared__ __attribute__((aligned(16))) float sQ[PD * PD];     // sQ[d][e] = Q[d][e]
    __shared__ __attribute__((aligned(16))) float sQt[PD * PD];    // sQt[e][d] = Q[d][e]
    __shared__ __attribute__((aligned(16))) float sv[PATCHES_PER_BLOCK][PD];
    __shared__ __attribute__((aligned(16))) float sy[PATCHES_PER_BLOCK][PD];
    const int tid = threadIdx.x, p = tid / 16, j = tid % 16;
    const Row w = load_row(row);
    for (int i = tid; i < PD * PD; i += 256) {
        const float q = Qg[i];
        sQ[i] = q;
        sQt[(i % PD) * PD + i / PD] = q;
    }
    if (!last && blockIdx.x == 0)
        for (int n = tid; n < N; n += 256) t_out[n] = w.t;
    __syncthreads();
    const int pw_n = W / PATCH, ph_n = H / PATCH;
    const long long patches_per_plane = (long long)pw_n * ph_n;
    const long long groups = (n_patch + PATCHES_PER_BLOCK - 1) / PATCHES_PER_BLOCK;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long P = g * PATCHES_PER_BLOCK + p;
        const bool live = P < n_patch;
        size_t o = 0;
        f32x4 x0 = {0.f, 0.f, 0.f, 0.f};
        float part = 0.f;
        if (live) {
            const long long plane = P / patches_per_plane, q = P % patches_per_plane;
            const int ph = (int)(q / pw_n), pw = (int)(q % pw_n);
            o = (size_t)plane * H * W + (size_t)(ph * PATCH + j / 2) * W + pw * PATCH + (j % 2) * 4;
            x0 = denoise4(w, *reinterpret_cast<const f32x4*>(F + o), *reinterpret_cast<const f32x4*>(x + o));
            if (denoised_out) *reinterpret_cast<f32x4*>(denoised_out + o) = x0;
            const f32x4 r = *reinterpret_cast<const f32x4*>(ref + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) part += r[e] * sQ[(4 * j + e) * PD];     // ref's coefficient 0, this thread's 4 terms
        }
        *reinterpret_cast<f32x4*>(&sv[p][4 * j]) = x0;
        // the 16 lanes of a patch are consecutive lanes of one wave
#pragma unroll
        for (int s = 8; s >= 1; s /= 2) part += __shfl_xor(part, s, 16);
        __syncthreads();
        f32x4 y = {0.f, 0.f, 0.f, 0.f};                                         // y_e = sum_d v_d Q[d][e], e = 4j..4j+3
        for (int d = 0; d < PD; ++d) {
            const float v = sv[p][d];
            const f32x4 q = *reinterpret_cast<const f32x4*>(&sQ[d * PD + 4 * j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = y[e] + v * q[e];
        }
        if (j == 0) y[0] = part;                                                 // x_mix[..., 0] = x0[..., 0] (ref)
        *reinterpret_cast<f32x4*>(&sy[p][4 * j]) = y;
        __syncthreads();
        f32x4 v = {0.f, 0.f, 0.f, 0.f};                                         // out_d = sum_e y_e Q[d][e], d = 4j..4j+3
        for (int e = 0; e < PD; ++e) {
            const float ye = sy[p][e];
            const f32x4 q = *reinterpret_cast<const f32x4*>(&sQt[e * PD + 4 * j]);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = v[k] + ye * q[k];
        }
        if (live) finish4(w, last, v, noise, x, x_in, out, o);
        __syncthreads();                                                         // sv / sy are reused by the next group
    }
}

}  // namespace

extern "C" int dxmi_cm_stage(int32_t mode, int32_t edit, int32_t last, const float* tab, int32_t row, const float* Q, float* x,
                             const float* model_out, const float* noise, const float* ref, const float* mask, float* x_in,
                             float* t_out, float* out, float* denoised, int32_t N, int32_t C, int32_t H, int32_t W,
                             void* stream) {
    DXMI_CHECK_ARG(mode == DXMI_CM_FIRST || mode == DXMI_CM_STEP, "dxmi_cm_stage: unknown mode %d", mode);
    DXMI_CHECK_ARG(edit >= DXMI_CM_EDIT_NONE && edit <= DXMI_CM_EDIT_PATCH, "dxmi_cm_stage: unknown edit kind %d", edit);
    DXMI_CHECK_ARG(N > 0 && N <= 65535 && C > 0 && H > 0 && W > 0, "dxmi_cm_stage: bad shape N=%d C=%d H=%d W=%d (N <= 65535)", N,
                   C, H, W);
    DXMI_CHECK_ARG((int64_t)C * H * W <= INT32_MAX, "dxmi_cm_stage: C*H*W above 2^31 - 1");
    DXMI_CHECK_ARG(row >= 0, "dxmi_cm_stage: negative table row (%d)", row);
    DXMI_CHECK_ARG(tab && x, "dxmi_cm_stage: null table or state");
    const bool first = mode == DXMI_CM_FIRST;
    DXMI_CHECK_ARG(!(first && last), "dxmi_cm_stage: the first stage cannot be the last");
    DXMI_CHECK_ARG(!(first && edit != DXMI_CM_EDIT_NONE), "dxmi_cm_stage: the first stage applies no edit");
    DXMI_CHECK_ARG(!(first && noise), "dxmi_cm_stage: the first stage draws no noise");
    DXMI_CHECK_ARG(first || model_out, "dxmi_cm_stage: null model output");
    DXMI_CHECK_ARG(last ? out != nullptr : (x_in && t_out), "dxmi_cm_stage: null output (out when last, else x_in and t)");
    DXMI_CHECK_ARG(edit == DXMI_CM_EDIT_NONE || ref, "dxmi_cm_stage: edit kind %d needs ref", edit);
    DXMI_CHECK_ARG(edit != DXMI_CM_EDIT_MASK || mask, "dxmi_cm_stage: the mask edit needs mask");
    DXMI_CHECK_ARG(!(edit == DXMI_CM_EDIT_COLOUR || edit == DXMI_CM_EDIT_PATCH) || Q, "dxmi_cm_stage: edit kind %d needs Q", edit);
    const int CHW = C * H * W;
    const float* r = tab + (size_t)row * DXMI_CT_COLS;
    const hipStream_t s = (hipStream_t)stream;
    if (edit == DXMI_CM_EDIT_NONE || edit == DXMI_CM_EDIT_MASK) {
        DXMI_CHECK_ARG(CHW % 4 == 0, "dxmi_cm_stage: C*H*W (%d) must be a multiple of 4", CHW);
        const int chunks = (CHW / 4 + 255) / 256;
        hipLaunchKernelGGL(cm_elementwise_kernel, dim3(chunks < 16 ? chunks : 16, N), dim3(256), 0, s, mode, edit, last, r, x,
                           model_out, noise, ref, mask, x_in, t_out, out, denoised, CHW);
    } else if (edit == DXMI_CM_EDIT_COLOUR) {
        DXMI_CHECK_ARG(C == 3, "dxmi_cm_stage: the colour edit needs C = 3 (got %d)", C);
        DXMI_CHECK_ARG((H * W) % 4 == 0, "dxmi_cm_stage: H*W (%d) must be a multiple of 4 in the colour edit", H * W);
        const int chunks = (H * W / 4 + 255) / 256;
        hipLaunchKernelGGL(cm_colour_kernel, dim3(chunks < 16 ? chunks : 16, N), dim3(256), 0, s, last, r, Q, x, model_out, noise,
                           ref, x_in, t_out, out, denoised, H * W);
    } else {
        DXMI_CHECK_ARG(H % PATCH == 0 && W % PATCH == 0, "dxmi_cm_stage: H (%d) and W (%d) must be multiples of 8 in the patch edit",
                       H, W);
        const long long n_patch = (long long)N * C * (H / PATCH) * (W / PATCH);
        const long long groups = (n_patch + PATCHES_PER_BLOCK - 1) / PATCHES_PER_BLOCK;
        const int grid = (int)(groups < 1024 ? groups : 1024);
        hipLaunchKernelGGL(cm_patch_kernel, dim3(grid), dim3(256), 0, s, last, r, Q, x, model_out, noise, ref, x_in, t_out, out,
                           denoised, N, H, W, n_patch);
    }
    DXMI_CHECK_LAUNCH("dxmi_cm_stage");
    return DXMI_OK;
}
