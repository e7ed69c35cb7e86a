// What the launches of dm_train.hip and sid_train.hip share: the level gather, 16-byte loads and stores, the fixed-order block
// sum, the elementwise grid and the argument checks.  Included after `#pragma clang fp contract(off)` and dsm_common.h.
#pragma once
#include "common.h"
#include "dsm_common.h"

namespace {

constexpr int EW_BLOCK = 256;
constexpr int EW_UNROLL = 4;      // f32x4 per stream per lane in flight

__device__ __forceinline__ float dm_level(const int64_t* __restrict__ idx, const float* __restrict__ tab, int S, int b) {
    const int64_t i = idx[b];
    return (i >= 0 && i < (int64_t)S) ? tab[i] : __builtin_nanf("");
}

__device__ __forceinline__ float dm_c_in(float s, float sd2) { return 1.f / __builtin_sqrtf(s * s + sd2); }
__device__ __forceinline__ float dm_time(float s) { return 250.f * logf(s + 1e-44f); }      // 1000 * 0.25 * th.log(sigmas + 1e-44)

__device__ __forceinline__ f32x4 ld4(const float* p, size_t base, int i) { return *reinterpret_cast<const f32x4*>(p + base + (size_t)i * 4); }
__device__ __forceinline__ void st4(float* p, size_t base, int i, f32x4 v) { *reinterpret_cast<f32x4*>(p + base + (size_t)i * 4) = v; }

// fixed order: a lane's running sum in index order, the xor-shuffle tree of a wave, a fixed pairing of the four wave partials
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

bool dm_aligned(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr,
                const void* f = nullptr, const void* g = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d) | ((uintptr_t)e) | ((uintptr_t)f) | ((uintptr_t)g)) & 15) == 0;
}

dim3 dm_grid(int N, int CHW) {
    const int chunks = (CHW / 4 + EW_BLOCK * EW_UNROLL - 1) / (EW_BLOCK * EW_UNROLL);
    return dim3(chunks < 64 ? chunks : 64, N);
}

}  // namespace

#define DM_CHECK_SHAPE(fn)                                                                                                       \
    DXMI_CHECK_ARG(N > 0 && N <= 65535 && CHW > 0 && CHW % 4 == 0 && CHW < (1 << 30), fn ": N (%d) must be in [1, 65535] and "   \
                   "CHW (%d) a positive multiple of 4 below 2^30", N, CHW)
#define DM_CHECK_SCALES(fn)                                                                                                      \
    DXMI_CHECK_ARG(num_scales >= 1 && num_scales < (1 << 30), fn ": num_scales (%d) must be in [1, 2^30)", num_scales)
#define DM_CHECK_POS(fn, v, what)                                                                                                \
    DXMI_CHECK_ARG((v) > 0.f && (v) <= 3.0e38f, fn ": " what " (%g) must be positive and finite", (double)(v))
