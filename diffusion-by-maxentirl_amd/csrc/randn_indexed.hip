// Batch- and rank-invariant sampling noise (models/cm/random_util.py; the reference's DeterministicGenerator /
// DeterministicIndividualGenerator, models/cm/random_util.py:28-182): a counter-based generator.  Every value of a draw is a pure
// function of (seed, global sample index, draw number, element index), so image i sees the same noise whatever batch carries it and
// however many ranks share the run, and ONE launch produces a draw for the whole batch.
//   dxmi_randn_indexed    standard normals, fp32 [N, per_sample]
//   dxmi_randint_indexed  integers in [low, high), int64 [N, per_sample]
// Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants): key =
// the two halves of the seed, counter = (block, draw, index low word, index high word); one call gives elements 4 block .. 4 block + 3
// of the row.  One workgroup row per image (grid.y), one Philox call per lane per trip; ALU-bound (ten rounds of two 32 x 32 -> 64
// multiplies, then two logf / sqrtf / sinf / cosf per four floats).  Stores only: no loads besides the row's index, no LDS, no atomics.
#include "common.h"
#include "philox_normal.h"

// one rounding per operation: the bits of a normal are part of the interface
#pragma clang fp contract(off)

namespace {

constexpr int RN_BLOCK = 256;
constexpr int RN_MAX_CHUNKS = 64;
// rows whose base is not 16-byte aligned (per_sample % 4 != 0, or odd for int64) store through these: the compiler picks the widest
// store the target allows at the stated alignment
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
typedef int64_t i64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

// A row is a function of its own index only: the counter holds the element block and the row's global index, never n, N or the grid.
__global__ __launch_bounds__(RN_BLOCK) void randn_indexed_kernel(float* __restrict__ out, const int64_t* __restrict__ sample_index,
                                                                 int per_sample, uint32_t k0, uint32_t k1, uint32_t draw) {
    const int n = blockIdx.y;
    const uint64_t index = (uint64_t)sample_index[n];
    const uint32_t i_lo = (uint32_t)index, i_hi = (uint32_t)(index >> 32);
    float* row = out + (size_t)n * per_sample;
    const int n4 = per_sample / 4, rem = per_sample % 4;
    const bool aligned = rem == 0;            // out is 16-byte aligned, so every row is
    for (int b = blockIdx.x * RN_BLOCK + threadIdx.x; b < n4; b += gridDim.x * RN_BLOCK) {
        const f32x4 z = normals(philox4x32_10((uint32_t)b, draw, i_lo, i_hi, k0, k1));
        if (aligned) *reinterpret_cast<f32x4*>(row + (size_t)b * 4) = z;
        else *reinterpret_cast<f32x4_a4*>(row + (size_t)b * 4) = z;
    }
    if (rem && blockIdx.x == 0 && threadIdx.x == 0) {      // the tail: the first `rem` values of block n4, one element per store
        const f32x4 z = normals(philox4x32_10((uint32_t)n4, draw, i_lo, i_hi, k0, k1));
        for (int e = 0; e < rem; ++e) row[(size_t)n4 * 4 + e] = z[e];
    }
}

// low + (x mod range) over one 32-bit word per element; range = high - low in [1, 2^31]
__global__ __launch_bounds__(RN_BLOCK) void randint_indexed_kernel(int64_t* __restrict__ out, const int64_t* __restrict__ sample_index,
                                                                   int per_sample, int64_t low, uint32_t range, uint32_t k0, uint32_t k1,
                                                                   uint32_t draw) {
    const int n = blockIdx.y;
    const uint64_t index = (uint64_t)sample_index[n];
    const uint32_t i_lo = (uint32_t)index, i_hi = (uint32_t)(index >> 32);
    int64_t* row = out + (size_t)n * per_sample;
    const int n4 = per_sample / 4, rem = per_sample % 4;
    const bool aligned = per_sample % 2 == 0;
    for (int b = blockIdx.x * RN_BLOCK + threadIdx.x; b < n4; b += gridDim.x * RN_BLOCK) {
        const u32x4 w = philox4x32_10((uint32_t)b, draw, i_lo, i_hi, k0, k1);
        i64x2 a, c;
        a[0] = low + (int64_t)(w[0] % range), a[1] = low + (int64_t)(w[1] % range);
        c[0] = low + (int64_t)(w[2] % range), c[1] = low + (int64_t)(w[3] % range);
        int64_t* p = row + (size_t)b * 4;
        if (aligned) {
            *reinterpret_cast<i64x2*>(p) = a;
            *reinterpret_cast<i64x2*>(p + 2) = c;
        } else {
            *reinterpret_cast<i64x2_a8*>(p) = a;
            *reinterpret_cast<i64x2_a8*>(p + 2) = c;
        }
    }
    if (rem && blockIdx.x == 0 && threadIdx.x == 0) {
        const u32x4 w = philox4x32_10((uint32_t)n4, draw, i_lo, i_hi, k0, k1);
        for (int e = 0; e < rem; ++e) row[(size_t)n4 * 4 + e] = low + (int64_t)(w[e] % range);
    }
}

dim3 rn_grid(int N, int per_sample) {
    const int chunks = (per_sample / 4 + RN_BLOCK - 1) / RN_BLOCK;
    return dim3(chunks < 1 ? 1 : (chunks < RN_MAX_CHUNKS ? chunks : RN_MAX_CHUNKS), N);
}

}  // namespace

#define RN_CHECK(fn)                                                                                                              \
    DXMI_CHECK_ARG(out && sample_index, fn ": null pointer");                                                                     \
    DXMI_CHECK_ARG(N > 0 && N <= 65535, fn ": N (%d) must be in [1, 65535]", N);                                                  \
    DXMI_CHECK_ARG(per_sample > 0 && per_sample <= (int64_t)INT32_MAX, fn ": per_sample (%lld) must be in [1, 2^31 - 1]",         \
                   (long long)per_sample);                                                                                        \
    DXMI_CHECK_ARG((((uintptr_t)out) & 15) == 0 && (((uintptr_t)sample_index) & 7) == 0, fn ": out must be 16-byte aligned "      \
                   "(sample_index 8-byte)")

extern "C" int dxmi_randn_indexed(float* out, const int64_t* sample_index, int32_t N, int64_t per_sample, uint64_t seed, uint32_t draw,
                                  void* stream) {
    RN_CHECK("dxmi_randn_indexed");
    hipLaunchKernelGGL(randn_indexed_kernel, rn_grid(N, (int)per_sample), dim3(RN_BLOCK), 0, (hipStream_t)stream, out, sample_index,
                       (int)per_sample, (uint32_t)seed, (uint32_t)(seed >> 32), draw);
    DXMI_CHECK_LAUNCH("dxmi_randn_indexed");
    return DXMI_OK;
}

extern "C" int dxmi_randint_indexed(int64_t* out, const int64_t* sample_index, int32_t N, int64_t per_sample, int64_t low, int64_t high,
                                    uint64_t seed, uint32_t draw, void* stream) {
    RN_CHECK("dxmi_randint_indexed");
    // high - low as unsigned: exact for every int64 pair with high > low
    DXMI_CHECK_ARG(high > low && (uint64_t)high - (uint64_t)low <= ((uint64_t)1 << 31), "dxmi_randint_indexed: [low, high) = [%lld, %lld) "
                   "must hold between 1 and 2^31 values (one 32-bit word per element)", (long long)low, (long long)high);
    hipLaunchKernelGGL(randint_indexed_kernel, rn_grid(N, (int)per_sample), dim3(RN_BLOCK), 0, (hipStream_t)stream, out, sample_index,
                       (int)per_sample, low, (uint32_t)((uint64_t)high - (uint64_t)low), (uint32_t)seed, (uint32_t)(seed >> 32), draw);
    DXMI_CHECK_LAUNCH("dxmi_randint_indexed");
    return DXMI_OK;
}
