// What the elementwise training launches share (ddpm_train.hip, edm_dsm.hip, cm_train.hip, pd_train.hip, dm_train.hip,
// sid_train.hip; pf_likelihood.hip takes block_sum): the 16-byte loads and stores, the fixed-order block sum, the single-level
// gather, the grid and the argument checks.  One workgroup row per image, 16 bytes per lane, EW_UNROLL loads per stream in flight.
#pragma once
#include "common.h"

// one rounding per written operation: no fused multiply-add between them.  The pragma is at file scope: it holds for the rest of
// every file that includes this header, wherever among its includes this one stands.
#pragma clang fp contract(off)

namespace {

constexpr int EW_BLOCK = 256;
constexpr int EW_UNROLL = 4;      // f32x4 per stream per lane in flight

__device__ __forceinline__ f32x4 ld4(const float* p, size_t base, int i) { return *reinterpret_cast<const f32x4*>(p + base + (size_t)i * 4); }
__device__ __forceinline__ void st4(float* p, size_t base, int i, f32x4 v) { *reinterpret_cast<f32x4*>(p + base + (size_t)i * 4) = v; }

// fixed order: a lane's running sum in index order, the xor-shuffle tree of a wave, a fixed pairing of the four wave partials.
// There is no barrier after the read: two sums in one kernel need two `red` arrays (EW_BLOCK / 64 floats each).
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// the level of image b from a device table of S entries; an index outside [0, S) gives NaN (nothing is read outside the table)
__device__ __forceinline__ float ew_level(const int64_t* __restrict__ idx, const float* __restrict__ tab, int S, int b) {
    const int64_t i = idx[b];
    return (i >= 0 && i < (int64_t)S) ? tab[i] : __builtin_nanf("");
}

// every image-sized operand of a launch; a null (absent) one passes
template <class... P>
bool ew_aligned(const P*... p) {
    return ((... | (uintptr_t)p) & 15) == 0;
}

// the map launches: at most 64 workgroups share an image by grid stride, EW_BLOCK * EW_UNROLL vectors each per trip
dim3 ew_grid(int N, int CHW) {
    const int chunks = (CHW / 4 + EW_BLOCK * EW_UNROLL - 1) / (EW_BLOCK * EW_UNROLL);
    return dim3(chunks < 64 ? chunks : 64, N);
}

}  // namespace

// N is a grid dimension; CHW / 4 vectors and the 2 N CHW elements of a stacked batch are indexed in int
#define EW_CHECK_SHAPE(fn)                                                                                                       \
    DXMI_CHECK_ARG(N > 0 && N <= 65535 && CHW > 0 && CHW % 4 == 0 && CHW < (1 << 30), fn ": N (%d) must be in [1, 65535] and "   \
                   "CHW (%d) a positive multiple of 4 below 2^30", N, CHW)
#define EW_CHECK_SCALES(fn)                                                                                                      \
    DXMI_CHECK_ARG(num_scales >= 1 && num_scales < (1 << 30), fn ": num_scales (%d) must be in [1, 2^30)", num_scales)
#define EW_CHECK_POS(fn, v, what)                                                                                                \
    DXMI_CHECK_ARG((v) > 0.f && (v) <= 3.0e38f, fn ": " what " (%g) must be positive and finite", (double)(v))
#define EW_CHECK_ALIGNED(fn, ...) DXMI_CHECK_ARG(ew_aligned(__VA_ARGS__), fn ": tensors must be 16-byte aligned")
