// Nearest x2 upsample + 3x3 convolution on full-width tiles: every weight x pixel product is computed once.
//
// Output pixel (Y, X), tap (a, b) of an upsampled conv reads low-res pixel ((Y+a-1)>>1, (X+b-1)>>1), so conv_ws_kernel
// (ups = 1) computes the K = Cin dot product w[a][b] . x[r][s] for two values of X (and two of Y).  This kernel, the second
// launch target of ConvKernel::ws, shares it between the two output COLUMNS: per hi-res row Y, low-res column s and column
// tap b it accumulates, by MFMA over the three row taps and all channels,
//     R_b[Y][s] = sum_a sum_c w[a][b][c] * x[(Y+a-1)>>1][s][c]
// into three separate fp32 accumulators and combines them with fp32 adds in the epilogue:
//     out[Y][2s]   = R_0[Y][s-1] + R_1[Y][s] + R_2[Y][s]
//     out[Y][2s+1] = R_0[Y][s]   + R_1[Y][s] + R_2[Y][s+1]           (out-of-range s: zero = the conv's zero padding)
// Nine MFMAs per 32 output pixels x 16 couts x 32 channels instead of 18; the nine bf16 weights stay as they are (a sum of
// bf16 weights is not a bf16 number), so every product is exact and an output is still ONE fp32 sum of its 9 Cin products.
// In the 16x16x32 accumulator lane l holds pixel column l % 16 = s: R_0[s-1] / R_2[s+1] are the row_shr:1 / row_shl:1 DPP
// operands of an add, whose zero fill at the row ends is the padding.  At IW = 8 a 16-lane row holds low-res rows (r, r+1) of
// hi-res rows (Y, Y+2): the shifted operand is zeroed at lanes 8 / 7 as well.
//
// One workgroup of 8 waves per CU, persistent over (256 hi-res pixels, 64 couts) tiles — 8 whole rows of a 32x32 map, a whole
// 16x16 map; the 64-cout tile halves the weight bytes per MFMA against a (128-pixel, 128-cout) tile of equal accumulator count:
//   waves 0-3  MFMA: 16 couts x 256 pixels each = 8 blocks (hi-res row x 16 low-res columns) x 3 column taps = 96 accumulator
//              registers.  Operands from LDS only: per 32-channel chunk the 6 (IW 16) / 9 (IW 8) distinct low-res row
//              fragments once, and one weight fragment per tap for 8 MFMAs.  One barrier per chunk (72 MFMAs per wave),
//              placed in front of the last tap's MFMAs so that the next chunk's operand reads fly under them.
//   waves 4-6  loaders, register-staged: chunk g + 2 is requested (global_load_dwordx4) before the barrier that ends chunk g
//              and written (ds_write_b128) into the buffer chunk g used, behind it: 36 KiB of weights + the low-res rows the
//              tile touches (6 / 5 KiB; no column halo, no upsampled copies: conv_ws_kernel stages 22 KiB).
//   wave 7     drain: the previous tile's output, LDS -> 128-byte NHWC row pieces, spread over the chunks; stores only.
// Bias / per-image vector / residual or mask source are read from global memory by the MFMA waves in the epilogue (they issue
// no other vector-memory instruction, so nothing in the K loop ever waits for them).
//
// Scope: ups == 1, OW == 2 IW in {16, 32}, OH == 2 IH, no virtual concat, Cout % 64 == 0, and what conv_ws_select checks
// (an even number >= 4 of 32-channel chunks, ...).  Everything else with ups == 1 stays on conv_ws_kernel.
// Block statistics: same partials and layout as conv_ws_kernel ([pixel tile * 2 + pixel half][Cout / 2][2]).
#include "ws_common.h"
#include <type_traits>

namespace {

constexpr int UP_A_CHUNK = 9 * 4096;     // weights of one 32-channel chunk x 64 couts: [tap][k-step][32-cout block] 1-KiB fragments
constexpr int UP_HALO = 6 * 1024;        // low-res rows of one chunk: 6 rows x 16 px (IW 16) or 10 rows x 8 px (IW 8) x 64 B
constexpr int UP_RO = 256 * 128;         // output tile: 256 px x 64 couts bf16
constexpr int UP_LDS = 2 * UP_A_CHUNK + 2 * UP_HALO + UP_RO;

struct UpTile {
    int cot, pt, n0, oy0;
};

template <int TW>
__global__ __launch_bounds__(512, 1) void conv_ws_up_kernel(ConvArgs p) {
    constexpr int IW = TW / 2, TH = 256 / TW, ROWB = IW * 64;
    constexpr int NF = TW == 32 ? 6 : 9;              // distinct B fragments (16 consecutive low-res pixels) per chunk
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    char* const abuf = smem;
    char* const hbuf = smem + 2 * UP_A_CHUNK;
    char* const ro = hbuf + 2 * UP_HALO;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tyn = p.OH / TH;
    const int nchunks = p.C0 / 32;
    const int ntiles = p.PT * p.CT;                  // (pixel tile, 64-cout tile) pairs, cout fastest
    auto tile_of = [&](int q, UpTile& t) {
        t.cot = q % p.CT;
        t.pt = q / p.CT;
        t.n0 = t.pt / tyn;
        t.oy0 = (t.pt % tyn) * TH;
    };
    const int q0 = dxmi_xcd_logical(blockIdx.x, gridDim.x, p.xcd_order);
    int q = q0;
    if (q >= ntiles) return;
    const int qstride = gridDim.x;
    const int px = lane & 15, kg = lane >> 4;

    if (wave < 4) {
        // ================================================================ MFMA waves: couts 16 w .. + 15 of the tile, all 256 pixels
        const int w = wave;
        // block j: hi-res tile row Yl(j) (lanes 8-15 at IW 8: Yl + 2), low-res column px (px & 7)
        auto Yl = [](int j) { return TW == 32 ? j : (j >> 1) * 4 + (j & 1); };
        const char* const bbase = hbuf + px * 64 + ((kg ^ (2 * ((px >> 2) & 1))) << 4);
        const char* const abase = abuf + (kg >> 1) * 2048 + (w >> 1) * 1024 + ((px + 32 * (kg & 1) + 16 * (w & 1)) << 4);
        f32x4 acc[3][8];
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[b][j][e] = 0.f;
        bf16x8 A[2], Bf[2][NF];
        auto read_a = [&](int P, int t, bf16x8& a) { a = *reinterpret_cast<const bf16x8*>(abase + P * UP_A_CHUNK + t * 4096); };
        auto read_b = [&](int P, bf16x8 (&B)[NF]) {
#pragma unroll
            for (int h = 0; h < NF; ++h) B[h] = *reinterpret_cast<const bf16x8*>(bbase + P * UP_HALO + h * ROWB);
        };
        const float slope = dxmi_act_slope(p.act);
        const bool has_res = p.residual != nullptr, is_mask = has_res && p.res_is_mask, want_stats = p.gn_stats != nullptr;
        // output tile: pixel row of 128 B in eight 16-byte slots, cout piece c8 in slot c8 ^ ((pixel >> 1) & 7)
        const int lanepix = TW == 32 ? 2 * px : (px >> 3) * 32 + 2 * (px & 7);
        char* const rob = ro + lanepix * 128 + (((w * 2 + (kg >> 1)) ^ (px & 7)) << 4) + (kg & 1) * 8;

        lds_barrier();                                   // P0: chunk 0 of the first tile is in LDS
        read_b(0, Bf[0]);
        read_a(0, 0, A[0]);
        for (;;) {
            const bool more = q + qstride < ntiles;
            UpTile cur;
            tile_of(q, cur);
            // K loop: two chunks (18 taps) of straight-line code per trip.  The barrier that ends a chunk stands in front of its
            // last tap's MFMAs: the next chunk's fragments (in LDS when it opens) are requested under them.
            for (int c = 0; c < nchunks; c += 2) {
#pragma unroll
                for (int u = 0; u < 18; ++u) {
                    const int P = u / 9, t = u % 9, a = t / 3, b = t % 3;
                    if (t < 8) {
                        read_a(P, t + 1, A[(u + 1) & 1]);
                    } else {
                        lds_barrier();
                        read_b(P ^ 1, Bf[P ^ 1]);
                        read_a(P ^ 1, 0, A[(u + 1) & 1]);
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        acc[b][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[u & 1], Bf[P][(Yl(j) + a + 1) >> 1], acc[b][j], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            {
                // combine the three column-tap sums, + bias + per-image vector (+ residual / mask) -> activation -> bf16 -> LDS
                const int co = cur.cot * 64 + w * 16 + 4 * kg;
                f32x4 bv = {0.f, 0.f, 0.f, 0.f};
                if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + co);
                if (p.addvec) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(p.addvec + (size_t)cur.n0 * p.addvec_ld + co);
#pragma unroll
                    for (int e = 0; e < 4; ++e) bv[e] += av[e];
                }
                const size_t tile_px = ((size_t)cur.n0 * p.OH + cur.oy0) * TW;
                float* const stp = want_stats ? p.gn_stats + (size_t)cur.pt * 2 * p.Cout + co : nullptr;
                auto epi = [&](auto RES, auto MASK, auto STATS) {
                    constexpr bool kRes = decltype(RES)::value, kMask = decltype(MASK)::value, kStats = decltype(STATS)::value;
                    bf16x4 r[8][2];
                    if constexpr (kRes) {
                        const bf16* const rp = p.residual + (tile_px + lanepix) * p.Cout + co;
#pragma unroll
                        for (int j = 0; j < 8; ++j)
#pragma unroll
                            for (int x = 0; x < 2; ++x) r[j][x] = *reinterpret_cast<const bf16x4*>(rp + (size_t)(Yl(j) * TW + x) * p.Cout);
                    }
                    float st[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        f32x4 v[2];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            // lane s: R_0 of lane s - 1 (row_shr:1) and R_2 of lane s + 1 (row_shl:1); zero past the DPP row's ends
                            // (inline asm: hipcc folds the four __builtin_amdgcn_update_dpp calls on the elements of one f32x4 into the
                            // first element's; the s_nop covers the two wait states between a VALU write and a DPP read)
                            float r0s, r2s;
                            asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(r0s) : "v"(acc[0][j][e]));
                            asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(r2s) : "v"(acc[2][j][e]));
                            if (TW == 16) {             // two low-res rows of 8 per DPP row: nothing crosses lanes 7 / 8
                                r0s = (px & 7) == 0 ? 0.f : r0s;
                                r2s = (px & 7) == 7 ? 0.f : r2s;
                            }
                            v[0][e] = (r0s + acc[1][j][e]) + acc[2][j][e];
                            v[1][e] = (acc[0][j][e] + acc[1][j][e]) + r2s;
                        }
#pragma unroll
                        for (int x = 0; x < 2; ++x) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[x][e] += bv[e];
                            if constexpr (kRes) {
                                if constexpr (kMask) {
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[x][e] *= ((float)r[j][x][e] > 0.f ? 1.f : p.mask_slope);
                                } else {
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[x][e] += (float)r[j][x][e];
                                }
                            }
                            bf16x4 o;
#pragma unroll
                            for (int e = 0; e < 4; ++e) o[e] = (bf16)dxmi_act_lin(v[x][e], slope);    // slope 1: the value itself
                            *reinterpret_cast<bf16x4*>(rob + (Yl(j) * TW + x) * 128) = o;
                            if constexpr (kStats) dxmi_stats4(o, st);
                        }
#pragma unroll
                        for (int b = 0; b < 3; ++b)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[b][j][e] = 0.f;
                        if constexpr (kStats) {
                            if (j == 3 || j == 7) {     // blocks 0-3 are tile pixels 0 .. 127: one partial per pixel half
                                f32x4 sv;
#pragma unroll
                                for (int e = 0; e < 4; ++e) { sv[e] = dxmi_row16_sum(st[e]); st[e] = 0.f; }
                                if (px == 0) *reinterpret_cast<f32x4*>(stp + (size_t)(j >> 2) * p.Cout) = sv;
                            }
                        }
                    }
                };
                using T_ = std::true_type;
                using F_ = std::false_type;
                if (is_mask) { if (want_stats) epi(T_{}, T_{}, T_{}); else epi(T_{}, T_{}, F_{}); }
                else if (has_res) { if (want_stats) epi(T_{}, F_{}, T_{}); else epi(T_{}, F_{}, F_{}); }
                else { if (want_stats) epi(F_{}, F_{}, T_{}); else epi(F_{}, F_{}, F_{}); }
            }
            lds_barrier();                               // E: output tile complete
            if (!more) break;
            q += qstride;
        }
    } else if (wave < 7) {
        // ================================================================ loaders (waves 4-6): 12 weight + 2 low-res row pieces each
        const int lw = wave - 4;
        const char* const wb = reinterpret_cast<const char*>(p.w) + (size_t)lane * 16;
        // low-res row pieces lw * 2, lw * 2 + 1 (1 KiB = 16 pixels): lane = pixel * 4 + slot, slot holds channel piece
        // slot ^ (2 * ((pixel >> 2) & 1)) (conv_ws_kernel's swizzle: the B fragment reads are bank-conflict free)
        const int p16 = lane >> 2, j8 = ((lane & 3) ^ (2 * ((p16 >> 2) & 1))) * 8;
        int hrow[2], hcol;
#pragma unroll
        for (int m = 0; m < 2; ++m) hrow[m] = TW == 32 ? lw * 2 + m : (lw * 2 + m) * 2 + (p16 >> 3);
        hcol = TW == 32 ? p16 : p16 & 7;
        int fq = q, fc = 0;                              // the chunk the next fetch() requests
        u32x4 fw[12], fh[2];
        bool hok[2];
        auto fetch = [&]() {
            UpTile t;
            tile_of(fq, t);
            const char* src = wb + ((size_t)(fc * 2) * p.CB + t.cot * 2) * 1024;
#pragma unroll
            for (int m = 0; m < 12; ++m) {
                const int tap = lw * 3 + (m >> 2), ks = (m >> 1) & 1, cbl = m & 1;
                fw[m] = *reinterpret_cast<const u32x4*>(src + ((size_t)(tap * p.KST + ks) * p.CB + cbl) * 1024);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int r = (t.oy0 >> 1) - 1 + hrow[m];
                hok[m] = r >= 0 && r < p.IH;
                const int rc = r < 0 ? 0 : (r < p.IH ? r : p.IH - 1);
                fh[m] = *reinterpret_cast<const u32x4*>(p.in0 + (((size_t)t.n0 * p.IH + rc) * IW + hcol) * p.C0 + fc * 32 + j8);
            }
            // past the last chunk of the last tile: the last tile's first chunk again (never consumed)
            if (++fc == nchunks) {
                fc = 0;
                if (fq + qstride < ntiles) fq += qstride;
            }
        };
        auto store = [&](int P) {
            char* const da = abuf + P * UP_A_CHUNK + (lw * 12) * 1024 + lane * 16;
#pragma unroll
            for (int m = 0; m < 12; ++m) *reinterpret_cast<u32x4*>(da + m * 1024) = fw[m];
            char* const dh = hbuf + P * UP_HALO + (lw * 2) * 1024 + lane * 16;
#pragma unroll
            for (int m = 0; m < 2; ++m) *reinterpret_cast<u32x4*>(dh + m * 1024) = hok[m] ? fh[m] : u32x4{0u, 0u, 0u, 0u};
        };
        fetch();
        store(0);
        fetch();
        lds_barrier();                                   // P0
        for (;;) {
            const bool more = q + qstride < ntiles;
            for (int c = 0; c < nchunks; c += 2) {
#pragma unroll
                for (int P = 0; P < 2; ++P) {
                    store(P ^ 1);                       // chunk g + 1, requested before the previous barrier
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    fetch();                            // chunk g + 2
                    lds_barrier();                       // end of chunk g
                }
            }
            lds_barrier();                               // E
            if (!more) break;
            q += qstride;
        }
    } else {
        // ================================================================ drain (wave 7): previous tile's output, LDS -> global
        // piece k (1 KiB): pixels 8 k .. 8 k + 7, lane = pixel * 8 + slot
        const int dpx = lane >> 3, dsl = lane & 7;
        const int nchunks_d = nchunks - 1;              // the last chunk of a tile carries no pieces
        const int kpc = (32 + nchunks_d - 1) / nchunks_d;
        bool have_prev = false;
        bf16* out_prev = reinterpret_cast<bf16*>(p.out);
        for (int i = 0;; ++i) {
            const bool more = q + qstride < ntiles;
            if (i == 0) lds_barrier();                   // P0
            for (int c = 0; c < nchunks; ++c) {
                if (have_prev) {
                    const int ka = c * kpc < 32 ? c * kpc : 32, kb = ka + kpc < 32 ? ka + kpc : 32;
#pragma unroll 2
                    for (int k = ka; k < kb; ++k) {
                        const int pix = k * 8 + dpx;
                        const bf16x8 v = *reinterpret_cast<const bf16x8*>(ro + (k * 64 + lane) * 16);
                        *reinterpret_cast<bf16x8*>(out_prev + (size_t)pix * p.Cout + (dsl ^ ((pix >> 1) & 7)) * 8) = v;
                    }
                }
                lds_barrier();                           // end of chunk c (its lgkmcnt(0): the pieces are out of LDS)
            }
            lds_barrier();                               // E
            UpTile cur;
            tile_of(q, cur);
            out_prev = reinterpret_cast<bf16*>(p.out) + (((size_t)cur.n0 * p.OH + cur.oy0) * TW) * p.Cout + cur.cot * 64;
            have_prev = true;
            if (!more) break;
            q += qstride;
        }
    }

    // ==================================================================== last tile out: all eight waves, four pieces each
    {
        UpTile lt;
        tile_of(q0 + ((ntiles - 1 - q0) / qstride) * qstride, lt);
        bf16* const ob = reinterpret_cast<bf16*>(p.out) + (((size_t)lt.n0 * p.OH + lt.oy0) * TW) * p.Cout + lt.cot * 64;
        bf16x8 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const bf16x8*>(ro + ((wave * 4 + u) * 64 + lane) * 16);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int pix = (wave * 4 + u) * 8 + (lane >> 3);
            *reinterpret_cast<bf16x8*>(ob + (size_t)pix * p.Cout + ((lane & 7) ^ ((pix >> 1) & 7)) * 8) = v[u];
        }
    }
}

}  // namespace

// Called by conv_ws_select for a shape it accepted: whether the product-sharing kernel runs it, and its own tiling.  The plan
// keeps kind, id and stats_tile of the family.
bool conv_ws_up_select(const ConvArgs& a, ConvPlan* p) {
    if (a.ups != 1 || a.C1 != 0 || a.OW != 2 * a.IW || a.OH != 2 * a.IH || (a.OW != 32 && a.OW != 16)) return false;
    if (a.Cout % 64 != 0 || a.C0 % 64 != 0 || a.C0 < 128 || a.OH % (256 / a.OW) != 0) return false;
    ConvArgs& b = p->args;
    b.PT = a.N * (a.OH / (256 / a.OW));
    b.CT = a.Cout / 64;
    p->t1 = 1;
    p->grid = b.PT * b.CT < 256 ? b.PT * b.CT : 256;
    p->lds = UP_LDS;
    return true;
}

int conv_ws_up_launch(const ConvPlan& p, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_ws_up_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_ws_up_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    if (p.t0 == 32) hipLaunchKernelGGL(conv_ws_up_kernel<32>, dim3(p.grid), dim3(512), p.lds, st, p.args);
    else hipLaunchKernelGGL(conv_ws_up_kernel<16>, dim3(p.grid), dim3(512), p.lds, st, p.args);
    DXMI_CHECK_LAUNCH("dxmi_conv2d_fwd(ws up)");
    return DXMI_OK;
}
