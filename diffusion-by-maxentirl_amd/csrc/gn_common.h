// GroupNorm device code shared by the streaming apply pass (gn_apply_kernel / gn_finalize_kernel, groupnorm.hip) and the fused
// norm1 + nin_shortcut kernel (conv1x1_rw.hip): the per-(image, channel) scale / offset both form from the block statistics and the
// per-element transform.  One definition, so the two paths give the same bits by construction.
#pragma once
#include "common.h"

constexpr int GN_APPLY_MAXP = 8;        // partials per image kept in flight per channel pair (ops.MAX_APPLY_PARTIALS folds larger P)

// Channel-pair sums of image n from block statistics st [N][P][nbs][2] -> pair_s[off + b], b < nbs: the <= GN_APPLY_MAXP partials of a
// pair are loaded together and added in partial order (uniform base + 32-bit lane offsets).
__device__ __forceinline__ void gn_pair_sums(float2* pair_s, const float* st, int n, int P, int nbs, int off, int tid) {
    const float2* const base = reinterpret_cast<const float2*>(st) + (size_t)n * P * nbs;
    for (int b = tid; b < nbs; b += 256) {
        float2 t[GN_APPLY_MAXP];
#pragma unroll
        for (int k = 0; k < GN_APPLY_MAXP; ++k)
            if (k < P) t[k] = base[(unsigned)(k * nbs + b)];
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int k = 0; k < GN_APPLY_MAXP; ++k)
            if (k < P) {
                s += t[k].x;
                q += t[k].y;
            }
        for (int k = GN_APPLY_MAXP; k < P; ++k) {       // more partials than the host folds to: correct, just serial
            const float2 tk = base[(unsigned)(k * nbs + b)];
            s += tk.x;
            q += tk.y;
        }
        pair_s[off + b] = make_float2(s, q);
    }
}

// Group g's mean / rstd from the pair sums, pairs added in channel order (thread g of the workgroup, g < groups).  Groups may straddle
// the in0 | in1 boundary: the pair sums of both halves sit side by side in pair_s.
__device__ __forceinline__ void gn_group_moments(const float2* pair_s, int g, int cpg, int HW, float eps, float* mean_s, float* rstd_s) {
    const int bpg = cpg >> 1;
    float s = 0.f, q = 0.f;
    for (int b = g * bpg; b < (g + 1) * bpg; ++b) {
        s += pair_s[b].x;
        q += pair_s[b].y;
    }
    const float cnt = (float)HW * (float)cpg;
    const float m = s / cnt;
    mean_s[g] = m;
    rstd_s[g] = rsqrtf(fmaxf(q / cnt - m * m, 0.f) + eps);
}

// Per-channel (scale, offset): y = x * a + b, then the optional FiLM scale-shift (models/cm/unet.py:252-256)
__device__ __forceinline__ void gn_channel_ab(float mean, float rstd, float gamma, float beta, float& a, float& b) {
    a = rstd * gamma;
    b = beta - mean * a;
}
__device__ __forceinline__ void gn_film(float& a, float& b, float scale, float shift) {
    const float sc = 1.f + scale;
    a *= sc;
    b = b * sc + shift;
}

// Eight channels of one pixel, rounded once to bf16
__device__ __forceinline__ bf16x8 gn_norm8(const bf16x8& v, const float* A, const float* B, int silu) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float y = (float)v[e] * A[e] + B[e];
        if (silu) y = dxmi_silu_fast(y);
        o[e] = (bf16)y;
    }
    return o;
}

// Launches gn_finalize_kernel (groupnorm.hip): ab[n][c] = (scale, offset) of every channel of every image, exactly what the apply
// pass's statistics prologue forms (no FiLM scale-shift).  Validates like dxmi_groupnorm_apply.
int gn_finalize_launch(const float* stats0, int P0, int C0, const float* stats1, int P1, int C1, const float* gamma, const float* beta,
                       float* ab, int N, int HW, int groups, float eps, hipStream_t st);
