// Adversarial Score identity Distillation (SiDA: Zhou, Zheng and co-authors, "Adversarial Score identity Distillation", 2024) on the
// one-step generator of sid_train.hip: the discriminator has NO parameters of its own.  It reads the fake denoiser's bottleneck
// activation h (the output of middle_block, NHWC bf16 [N, P = hb wb, Cb]) and takes the channel mean as one logit per position:
//   logit[n, p] = (1 / Cb) sum_c h[n, p, c]          a_n(sign) = (1 / P) sum_p softplus(sign logit[n, p])
// The two launches between the fake net's forward and the backward walk that takes their result as a second cotangent at the
// bottleneck (models.cm.unet_train.input_forward(tap=True) / input_backward(d_tap=...), encoder_forward / encoder_backward):
//   dxmi_sida_map_fwd   h -> logit [N, P] and a [N] for a per-image sign (the generator's term: -1; the discriminator's 2N batch:
//                       +1 for the generated half, -1 for the real half, one call)
//   dxmi_sida_map_bwd   d_h[n, p, :] = bf16((coef_n up_n) sign_n sigmoid(sign_n logit[n, p]) / (P Cb)): the cotangent of
//                       coef_n up_n a_n with respect to h, the same value on every channel of a position
// sign and coef are HOST arrays: they are known where the call is made (no tensor of signs exists on the device), they are checked
// there (a sign that is not -1 / +1 and a non-finite coef are DXMI_EINVAL), and they travel as kernel arguments, SIDA_CHUNK images to
// a launch: N <= 64 is one launch, and no copy and no synchronisation is made.  up is the optional per-image upstream gradient of an
// autograd backward, on the device.
// Sum order (fixed, the same whatever batch an image rides in): one workgroup per image, a wave per position p = wave, wave + 4, ...;
// a lane sums the 8 channels of its 16-byte vector in channel order, its vectors (lane, lane + 64, ...) in index order, then the
// xor-shuffle tree of the wave, one division by Cb.  a_n: a wave's softplus values in position order, the four wave partials in the
// fixed pairing of block_sum, one division by P.  fp32 throughout, no atomics; contraction off (ew_common.h).
#include <cfloat>

#include "ew_common.h"

namespace {

constexpr int SIDA_CHUNK = 64;      // images per launch: their signs are one 64-bit mask, their coefficients 64 floats of kernel argument
constexpr int SIDA_WAVES = EW_BLOCK / 64;

struct SidaSign {
    uint64_t minus;                 // bit i: image i of the chunk has sign -1
};
struct SidaCoef {
    float c[SIDA_CHUNK];            // coef_n sign_n
};

__device__ __forceinline__ float sida_softplus(float v) { return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))); }
__device__ __forceinline__ float sida_sigmoid(float v) {
    const float e = expf(-fabsf(v));
    return v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// grid (images of the chunk); h, logit, a already point at the chunk's first image
__global__ __launch_bounds__(EW_BLOCK) void sida_map_fwd_kernel(const bf16* __restrict__ h, SidaSign sg, float* __restrict__ logit,
                                                                float* __restrict__ a, int P, int Cb) {
    __shared__ float red[SIDA_WAVES];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float sign = ((sg.minus >> n) & 1) ? -1.f : 1.f;
    const int nv = Cb / 8;
    const bf16* hn = h + (size_t)n * P * Cb;
    float* ln = logit + (size_t)n * P;
    float acc_a = 0.f;
    for (int p = wave; p < P; p += SIDA_WAVES) {
        const bf16* row = hn + (size_t)p * Cb;
        float acc = 0.f;
        for (int v0 = lane; v0 < nv; v0 += 64 * EW_UNROLL) {
            bf16x8 hv[EW_UNROLL];
#pragma unroll
            for (int u = 0; u < EW_UNROLL; ++u)
                if (v0 + u * 64 < nv) hv[u] = *reinterpret_cast<const bf16x8*>(row + (size_t)(v0 + u * 64) * 8);
#pragma unroll
            for (int u = 0; u < EW_UNROLL; ++u) {
                if (v0 + u * 64 >= nv) continue;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += (float)hv[u][e];
            }
        }
        const float l = wave_sum(acc) / (float)Cb;
        if (lane == 0) ln[p] = l;
        acc_a += sida_softplus(sign * l);         // (every lane of the wave holds the same l)
    }
    if (lane == 0) red[wave] = acc_a;
    __syncthreads();
    if (threadIdx.x == 0) a[n] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)P;
}

// grid (ceil(P / SIDA_WAVES), images of the chunk): a wave per position, 16-byte stores of one value
__global__ __launch_bounds__(EW_BLOCK) void sida_map_bwd_kernel(const float* __restrict__ logit, SidaSign sg, SidaCoef cf,
                                                                const float* __restrict__ up, bf16* __restrict__ d_h, int P, int Cb) {
    const int n = blockIdx.y, lane = threadIdx.x & 63;
    const int p = blockIdx.x * SIDA_WAVES + (threadIdx.x >> 6);
    if (p >= P) return;
    const float sign = ((sg.minus >> n) & 1) ? -1.f : 1.f;
    float c = cf.c[n];
    if (up) c = c * up[n];
    const float v = (c * sida_sigmoid(sign * logit[(size_t)n * P + p])) / ((float)P * (float)Cb);
    const bf16 b = (bf16)v;
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = b;
    bf16* row = d_h + ((size_t)n * P + p) * Cb;
    for (int i = lane; i < Cb / 8; i += 64) *reinterpret_cast<bf16x8*>(row + (size_t)i * 8) = o;
}

// the chunk's signs as a mask; false: a value that is neither -1 nor +1 (its index in *bad)
bool sida_signs(const int32_t* sign, int n0, int cnt, SidaSign* out, int* bad) {
    out->minus = 0;
    for (int i = 0; i < cnt; ++i) {
        const int32_t s = sign[n0 + i];
        if (s != 1 && s != -1) {
            *bad = n0 + i;
            return false;
        }
        if (s < 0) out->minus |= (uint64_t)1 << i;
    }
    return true;
}

}  // namespace

// P Cb elements of an image and the N P logits are indexed in size_t; P (Cb / 8) and the grid dimensions stay in int
#define SIDA_CHECK_SHAPE(fn)                                                                                                       \
    do {                                                                                                                           \
        DXMI_CHECK_ARG(N > 0 && N <= 65535, fn ": N (%d) must be in [1, 65535]", N);                                               \
        DXMI_CHECK_ARG(P > 0 && P <= (1 << 20), fn ": P (%d) must be in [1, 2^20]", P);                                            \
        DXMI_CHECK_ARG(Cb > 0 && Cb <= 4096 && Cb % 8 == 0, fn ": Cb (%d) must be a multiple of 8 in [8, 4096]", Cb);              \
    } while (0)

extern "C" int dxmi_sida_map_fwd(const void* h, const int32_t* sign, float* logit, float* a, int32_t N, int32_t P, int32_t Cb,
                                 void* stream) {
    DXMI_CHECK_ARG(h && sign && logit && a, "dxmi_sida_map_fwd: null pointer");
    SIDA_CHECK_SHAPE("dxmi_sida_map_fwd");
    DXMI_CHECK_ARG(ew_aligned((const char*)h), "dxmi_sida_map_fwd: h must be 16-byte aligned");
    DXMI_CHECK_ARG((((uintptr_t)logit | (uintptr_t)a) & 3) == 0, "dxmi_sida_map_fwd: logit and a must be 4-byte aligned");
    for (int n0 = 0; n0 < N; n0 += SIDA_CHUNK) {      // every sign is checked before the first launch
        SidaSign sg;
        int bad = 0;
        DXMI_CHECK_ARG(sida_signs(sign, n0, N - n0 < SIDA_CHUNK ? N - n0 : SIDA_CHUNK, &sg, &bad),
                       "dxmi_sida_map_fwd: sign[%d] (%d) must be -1 or +1", bad, (int)sign[bad]);
    }
    for (int n0 = 0; n0 < N; n0 += SIDA_CHUNK) {
        const int cnt = N - n0 < SIDA_CHUNK ? N - n0 : SIDA_CHUNK;
        SidaSign sg;
        int bad = 0;
        sida_signs(sign, n0, cnt, &sg, &bad);
        hipLaunchKernelGGL(sida_map_fwd_kernel, dim3(cnt), dim3(EW_BLOCK), 0, (hipStream_t)stream,
                           (const bf16*)h + (size_t)n0 * P * Cb, sg, logit + (size_t)n0 * P, a + n0, P, Cb);
        DXMI_CHECK_LAUNCH("dxmi_sida_map_fwd");
    }
    return DXMI_OK;
}

extern "C" int dxmi_sida_map_bwd(const float* logit, const int32_t* sign, const float* coef, const float* upstream, void* d_h,
                                 int32_t N, int32_t P, int32_t Cb, void* stream) {
    DXMI_CHECK_ARG(logit && sign && coef && d_h, "dxmi_sida_map_bwd: null pointer");
    SIDA_CHECK_SHAPE("dxmi_sida_map_bwd");
    DXMI_CHECK_ARG(ew_aligned((const char*)d_h), "dxmi_sida_map_bwd: d_h must be 16-byte aligned");
    DXMI_CHECK_ARG((((uintptr_t)logit | (uintptr_t)upstream) & 3) == 0, "dxmi_sida_map_bwd: logit and upstream must be 4-byte aligned");
    for (int n0 = 0; n0 < N; n0 += SIDA_CHUNK) {
        SidaSign sg;
        int bad = 0;
        DXMI_CHECK_ARG(sida_signs(sign, n0, N - n0 < SIDA_CHUNK ? N - n0 : SIDA_CHUNK, &sg, &bad),
                       "dxmi_sida_map_bwd: sign[%d] (%d) must be -1 or +1", bad, (int)sign[bad]);
    }
    for (int n = 0; n < N; ++n)
        DXMI_CHECK_ARG(coef[n] >= -FLT_MAX && coef[n] <= FLT_MAX, "dxmi_sida_map_bwd: coef[%d] (%g) must be finite", n, (double)coef[n]);
    for (int n0 = 0; n0 < N; n0 += SIDA_CHUNK) {
        const int cnt = N - n0 < SIDA_CHUNK ? N - n0 : SIDA_CHUNK;
        SidaSign sg;
        SidaCoef cf;
        int bad = 0;
        sida_signs(sign, n0, cnt, &sg, &bad);
        for (int i = 0; i < SIDA_CHUNK; ++i) cf.c[i] = i < cnt ? coef[n0 + i] * (float)sign[n0 + i] : 0.f;
        hipLaunchKernelGGL(sida_map_bwd_kernel, dim3((P + SIDA_WAVES - 1) / SIDA_WAVES, cnt), dim3(EW_BLOCK), 0, (hipStream_t)stream,
                           logit + (size_t)n0 * P, sg, cf, upstream ? upstream + n0 : (const float*)nullptr,
                           (bf16*)d_h + (size_t)n0 * P * Cb, P, Cb);
        DXMI_CHECK_LAUNCH("dxmi_sida_map_bwd");
    }
    return DXMI_OK;
}
