// The two DxMI sampler transitions with their noise made in the launch:
//   dxmi_var_step_fwd_indexed   dxmi_var_step_fwd (csrc/elementwise.hip) without its z operand
//   dxmi_edm_step_fwd_indexed   dxmi_edm_step_fwd (csrc/elementwise.hip) without its z operand
// z[n][e] is the value dxmi_randn_indexed writes for (seed, sample_index[n], draw, e): the counter layout of csrc/randn_indexed.hip
// through the functions of philox_normal.h, so the bits are the same.  What a launch returns is, bit for bit, what the indexed draw
// followed by the transition with z returns; it saves that pair one launch and one write plus read of z.
//
// Contraction.  csrc/elementwise.hip leaves floating-point contraction on, and the compiler fuses some of the two transitions'
// multiply-adds there; this file turns it off (philox_normal.h needs one rounding per operation) and WRITES OUT every fused
// multiply-add the two kernels of elementwise.hip are compiled to (read from their gfx950 code):
//   VAR   mean = fma(xmul, x, control)                     control = cmul eps, rounded
//         assoc 1: x' = xmul x + fma(sigma, z, control)     xmul x rounded on its own
//         assoc 0: x' = fma(sigma, z, mean)
//         the log-probability term has no fused operation: -(d d) / (2 sigma sigma) - log sigma - log sqrt(2 pi), summed in the
//         same lane order, wave order and final division as var_step_kernel
//   EDM   denoised = fma(c_out, F, c_skip x)   mean = fma(sigma_down - sigma, d, x)   x' = fma(sigma_up, z, mean)
//         s s + sd sd, c_skip, c_out and d = (x - denoised) / sigma: one rounding per operation
// tests/test_hip_step_indexed.py holds the two forms together bit for bit; if a compiler release fuses elementwise.hip differently,
// that test says so.
//
// Shape of the launches.  VAR: one workgroup of 256 lanes per image, lane l takes elements 4 l .. 4 l + 3 of every 1024-element
// trip, as var_step_kernel does: the per-image sum of the log-probability is a fixed-order fp32 reduction, so the order is part of
// the result.  EDM has no reduction: grid (trips up to 64, N).  Loads are issued before the ten Philox rounds and the Box-Muller of
// the trip, so their latency is under the arithmetic; with the generator the launch is VALU-bound (csrc/randn_indexed.hip).
// Control block (the convention of dxmi_ddpm_stage): ctl NULL: draw and seed by value; else an int32[4] device block (unused, draw,
// seed low word, seed high word) read by the kernel, so a captured launch is fed per replay.
#include "common.h"
#include "philox_normal.h"

// one rounding per operation; a fused multiply-add only where one is written out
#pragma clang fp contract(off)

namespace {

constexpr int SI_BLOCK = 256;
constexpr int SI_TRIP = SI_BLOCK * 4;      // elements per workgroup trip
constexpr int SI_MAX_TRIPS = 64;           // grid.x of the EDM launch

struct SiKey {
    uint32_t draw, k0, k1, i_lo, i_hi;
};

__device__ __forceinline__ SiKey si_key(const int32_t* __restrict__ ctl, uint32_t draw_v, uint32_t k0_v, uint32_t k1_v,
                                        const int64_t* __restrict__ sample_index, int n) {
    SiKey k;
    k.draw = ctl ? (uint32_t)ctl[1] : draw_v;
    k.k0 = ctl ? (uint32_t)ctl[2] : k0_v;
    k.k1 = ctl ? (uint32_t)ctl[3] : k1_v;
    const uint64_t index = (uint64_t)sample_index[n];
    k.i_lo = (uint32_t)index, k.i_hi = (uint32_t)(index >> 32);
    return k;
}

// elements i .. i + 3 of the row (i % 4 == 0): block i / 4 of the row's draw
__device__ __forceinline__ f32x4 si_normals(const SiKey& k, int i) {
    return normals(philox4x32_10((uint32_t)(i >> 2), k.draw, k.i_lo, k.i_hi, k.k0, k.k1));
}

__global__ __launch_bounds__(SI_BLOCK) void var_step_indexed_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                                    const int64_t* __restrict__ sample_index,
                                                                    const int32_t* __restrict__ ctl, uint32_t draw_v, uint32_t k0_v,
                                                                    uint32_t k1_v, const float* __restrict__ xmul,
                                                                    const float* __restrict__ cmul, const float* __restrict__ sigma,
                                                                    float* __restrict__ x_next, float* __restrict__ mean,
                                                                    float* __restrict__ control, float* __restrict__ logp, int CHW,
                                                                    int assoc) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const SiKey key = si_key(ctl, draw_v, k0_v, k1_v, sample_index, b);
    const float xm = xmul[b], cm = cmul[b], sg = sigma[b];
    const float var2 = 2.f * sg * sg;
    const float log_sg = logf(sg);
    const float half_log_2pi = 0.918938533204672742f;  // log(sqrt(2*pi))
    const size_t base = (size_t)b * CHW;
    float acc = 0.f;
    for (int i = threadIdx.x * 4; i < CHW; i += SI_TRIP) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + base + i);
        const f32x4 ev = *reinterpret_cast<const f32x4*>(eps + base + i);
        const f32x4 zv = si_normals(key, i);
        f32x4 xn, mu, ct;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xs = xv[e] * xm;
            ct[e] = cm * ev[e];
            mu[e] = __builtin_fmaf(xm, xv[e], ct[e]);
            xn[e] = assoc ? xs + __builtin_fmaf(sg, zv[e], ct[e]) : __builtin_fmaf(sg, zv[e], mu[e]);
            const float d = xn[e] - mu[e];
            acc += -(d * d) / var2 - log_sg - half_log_2pi;
        }
        *reinterpret_cast<f32x4*>(x_next + base + i) = xn;
        if (mean) *reinterpret_cast<f32x4*>(mean + base + i) = mu;
        if (control) *reinterpret_cast<f32x4*>(control + base + i) = ct;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && logp) logp[b] = (red[0] + red[1] + red[2] + red[3]) / (float)CHW;
}

__global__ __launch_bounds__(SI_BLOCK) void edm_step_indexed_kernel(const float* __restrict__ x, const float* __restrict__ fout,
                                                                    const int64_t* __restrict__ sample_index,
                                                                    const int32_t* __restrict__ ctl, uint32_t draw_v, uint32_t k0_v,
                                                                    uint32_t k1_v, const float* __restrict__ sigma,
                                                                    const float* __restrict__ sigma_down,
                                                                    const float* __restrict__ sigma_up, float* __restrict__ sample,
                                                                    float* __restrict__ mean, int CHW, float sd) {
    const int b = blockIdx.y;
    const SiKey key = si_key(ctl, draw_v, k0_v, k1_v, sample_index, b);
    const float s = sigma[b], sdn = sigma_down[b], sup = sigma_up[b];
    const float sd2 = sd * sd;
    const float den = s * s + sd2;
    const float c_skip = sd2 / den;
    const float c_out = s * sd / powf(den, 0.5f);
    const float dt = sdn - s;
    const size_t base = (size_t)b * CHW;
    for (int i = blockIdx.x * SI_TRIP + threadIdx.x * 4; i < CHW; i += gridDim.x * SI_TRIP) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + base + i);
        const f32x4 fv = *reinterpret_cast<const f32x4*>(fout + base + i);
        const f32x4 zv = si_normals(key, i);
        f32x4 mu, sm;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float den_ = __builtin_fmaf(c_out, fv[e], c_skip * xv[e]);
            const float d = (xv[e] - den_) / s;
            mu[e] = __builtin_fmaf(dt, d, xv[e]);
            sm[e] = __builtin_fmaf(sup, zv[e], mu[e]);
        }
        *reinterpret_cast<f32x4*>(mean + base + i) = mu;
        *reinterpret_cast<f32x4*>(sample + base + i) = sm;
    }
}

inline bool si_aligned16(const void* a, const void* b, const void* c, const void* d, const void* e, const void* f) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d) | ((uintptr_t)e) | ((uintptr_t)f)) & 15) == 0;
}

inline bool si_aligned4(const void* a, const void* b, const void* c, const void* d, const void* e) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d) | ((uintptr_t)e)) & 3) == 0;
}

}  // namespace

// CHW % 4 == 0: every row base is 16-byte aligned when the tensor is.  CHW <= 2^30: the element index of a lane stays an int past the
// row's end (it overshoots by less than one grid of trips)
#define SI_CHECK_SHAPE(fn)                                                                                          \
    DXMI_CHECK_ARG(N > 0, fn ": N (%d) must be positive", N);                                                       \
    DXMI_CHECK_ARG(CHW > 0 && CHW % 4 == 0 && CHW <= (1 << 30), fn ": CHW (%d) must be a multiple of 4 in [4, 2^30]", CHW)

extern "C" int dxmi_var_step_fwd_indexed(const float* x, const float* eps, const int64_t* sample_index, const int32_t* ctl,
                                         uint32_t draw, uint64_t seed, const float* xmul, const float* cmul, const float* sigma,
                                         float* x_next, float* mean, float* control, float* logp, int32_t N, int32_t CHW,
                                         int32_t assoc, void* stream) {
    DXMI_CHECK_ARG(x && eps && sample_index && xmul && cmul && sigma && x_next, "dxmi_var_step_fwd_indexed: null pointer");
    SI_CHECK_SHAPE("dxmi_var_step_fwd_indexed");
    DXMI_CHECK_ARG(assoc == 0 || assoc == 1, "dxmi_var_step_fwd_indexed: assoc (%d) must be 0 or 1", assoc);
    DXMI_CHECK_ARG(si_aligned16(x, eps, x_next, mean, control, nullptr) && (((uintptr_t)sample_index) & 7) == 0 &&
                       si_aligned4(ctl, xmul, cmul, sigma, logp),
                   "dxmi_var_step_fwd_indexed: x, eps, x_next, mean and control must be 16-byte aligned (sample_index 8-byte; ctl, "
                   "xmul, cmul, sigma and logp 4-byte)");
    hipLaunchKernelGGL(var_step_indexed_kernel, dim3(N), dim3(SI_BLOCK), 0, (hipStream_t)stream, x, eps, sample_index, ctl, draw,
                       (uint32_t)seed, (uint32_t)(seed >> 32), xmul, cmul, sigma, x_next, mean, control, logp, (int)CHW, (int)assoc);
    DXMI_CHECK_LAUNCH("dxmi_var_step_fwd_indexed");
    return DXMI_OK;
}

extern "C" int dxmi_edm_step_fwd_indexed(const float* x, const float* model_out, const int64_t* sample_index, const int32_t* ctl,
                                         uint32_t draw, uint64_t seed, const float* sigma, const float* sigma_down,
                                         const float* sigma_up, float* sample, float* mean, int32_t N, int32_t CHW, float sigma_data,
                                         void* stream) {
    DXMI_CHECK_ARG(x && model_out && sample_index && sigma && sigma_down && sigma_up && sample && mean,
                   "dxmi_edm_step_fwd_indexed: null pointer");
    SI_CHECK_SHAPE("dxmi_edm_step_fwd_indexed");
    DXMI_CHECK_ARG(N <= 65535, "dxmi_edm_step_fwd_indexed: N (%d) must be at most 65535", N);
    DXMI_CHECK_ARG(si_aligned16(x, model_out, sample, mean, nullptr, nullptr) && (((uintptr_t)sample_index) & 7) == 0 &&
                       si_aligned4(ctl, sigma, sigma_down, sigma_up, nullptr),
                   "dxmi_edm_step_fwd_indexed: x, model_out, sample and mean must be 16-byte aligned (sample_index 8-byte; ctl, "
                   "sigma, sigma_down and sigma_up 4-byte)");
    const int trips = (CHW + SI_TRIP - 1) / SI_TRIP;
    hipLaunchKernelGGL(edm_step_indexed_kernel, dim3(trips < SI_MAX_TRIPS ? trips : SI_MAX_TRIPS, N), dim3(SI_BLOCK), 0,
                       (hipStream_t)stream, x, model_out, sample_index, ctl, draw, (uint32_t)seed, (uint32_t)(seed >> 32), sigma,
                       sigma_down, sigma_up, sample, mean, (int)CHW, sigma_data);
    DXMI_CHECK_LAUNCH("dxmi_edm_step_fwd_indexed");
    return DXMI_OK;
}
