// The counter-based generator behind the indexed draws (csrc/randn_indexed.hip) and the fused noise of dxmi_ddpm_stage and
// dxmi_dpm_stage (csrc/stage_common.h): Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the
// Random123 constants), the 23-bit uniform and Box-Muller.  ONE definition: the bits of a normal are part of the interface
// (include/dxmi_hip.h), so every launch that makes one goes through these three functions, contraction off.
#pragma once
#include "common.h"

// one rounding per operation (the pragma is file-scoped: it holds for the including file from here on, which both users want)
#pragma clang fp contract(off)

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // Weyl key increments (golden ratio, sqrt(3) - 1)

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;      // the key is bumped between rounds (the bump after the tenth is unused)
        k1 += PHILOX_W1;
    }
    u32x4 o;
    o[0] = c0, o[1] = c1, o[2] = c2, o[3] = c3;
    return o;
}

// ((x >> 9) + 0.5) 2^-23: 23 bits and the half fit fp32's 24-bit significand, so the value is exact and lies in [2^-24, 1 - 2^-24]
__device__ __forceinline__ float uniform23(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-7f; }

// Box-Muller on the pairs (x0, x1) and (x2, x3): r = sqrtf(-2 logf(u_a)), z0 = r cosf(2 pi u_b), z1 = r sinf(2 pi u_b); |z| <= sqrt(48 ln 2)
__device__ __forceinline__ f32x4 normals(u32x4 w) {
    f32x4 z;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float ua = uniform23(w[2 * p]), ub = uniform23(w[2 * p + 1]);
        const float r = __builtin_sqrtf(-2.f * logf(ua));
        const float th = 6.2831855f * ub;
        z[2 * p] = r * cosf(th);
        z[2 * p + 1] = r * sinf(th);
    }
    return z;
}

}  // namespace
