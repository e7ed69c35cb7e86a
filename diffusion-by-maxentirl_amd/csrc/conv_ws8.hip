// conv_ws_kernel's design (conv_ws.hip: MFMA waves fed only from LDS, dedicated mover waves, 16x16x32 MFMAs) for the 8x8
// maps of the U-Nets (level 2 of the CIFAR-10 DDPM net: 13 of its 49 convs), where a 256-pixel x 128-cout tile would leave
// only 128 workgroups for 256 CUs.  Here a tile is FOUR whole 8x8 images x 64 couts:
//   * 256 images x 256 couts = 256 tiles: one per CU, same 512-thread workgroup (waves 0-3 MFMA, 4-5 weights, 6-7 the rest);
//   * MFMA wave w owns image w of the tile: 64 couts x 64 pixels (4 x 4 accumulator blocks of 16 x 16), operands by
//     ds_read_b128 at a per-lane base + compile-time offset; a step (one tap of one 32-channel chunk) is 16 MFMAs;
//   * halo image: per image 10 rows x 8 pixels x 64 B (5 KB; 20 KB per chunk), channel piece j of column x in slot
//     j ^ ((x & 4) >> 1) (bank-conflict free for every tap at row pitch 8, brute-forced: tools/ws8_swizzle.py).  Only the 64
//     interior pixels are ever fetched: four 1-KiB DMAs per image and chunk.  The zero rows above and below (rows 0 and 9 of
//     the image's block) are written once per launch; a lane whose tap column falls left or right of the map reads a 5 KB zero
//     strip instead (its per-lane base points there: no padding column is stored, none is fetched);
//   * weight ring 6 x 4 KB; output / residual tile 32 KB; bias + one temb row per image;
//   * everything else as in conv_ws.hip: one barrier per step, movers issue a few DMAs per step, exact in-order vmcnt counts.
// Scope: 3x3 / stride 1 / pad 1 on 8x8 maps, NHWC bf16 in (virtual concat) and out, any batch, Cout % 64 == 0,
// an even number (>= 4) of 32-channel chunks.
#include "ws_common.h"
#include <stdlib.h>
#include <type_traits>


namespace {

constexpr int W8_ROW = 8 * 64;                      // halo row pitch: the 8 interior pixels x 64 B (no padding columns)
constexpr int W8_IMG = 10 * W8_ROW;                 // an image's block: zero row, 8 interior rows (4 KiB contiguous), zero row
constexpr int W8_HALO_BLOCKS = 16;                  // 1-KiB DMAs per chunk: 4 images x 4 row pairs
constexpr int W8_HALO = 4 * W8_IMG;                 // 20 KiB per buffer
constexpr int W8_STRIP = W8_IMG;                    // zero strip behind the two buffers: what a tap column outside 0..7 reads
constexpr int W8_A_SLOT = 4096;                     // one (chunk, tap): 2 k-steps x 2 cout blocks x 1 KiB fragments
#ifndef W8_RING_SLOTS
#define W8_RING_SLOTS 6
#endif
constexpr int W8_RING = W8_RING_SLOTS;        // must divide 18 (the MFMA waves index slots by the step inside a chunk pair)
constexpr int W8_A_RING = W8_RING * W8_A_SLOT;
constexpr int W8_RO = 256 * 128;                    // 256 px x 64 co bf16
constexpr int W8_TB = 2048;                         // bias[64] | temb[4][64] fp32

WS_ZERO_PAGE(w8_zero16);

// (diagnostic build, make STAMPS=1: DXMI_CONV_WS8_DBG bits 1 no weight stream, 2 no halo stream, 4 no step barriers — wrong
// results; tools/conv_ws8_ab.py)

struct W8Tile {
    int cot, n0;
};

// GN: GroupNorm(+SiLU) of the output written INSTEAD of the raw output (dxmi_conv_desc.gn_out with gn_flags bit 1): MFMA wave w
// holds all 64 pixels of its image for the tile's 64 couts = eight whole groups of 8 channels, so the statistics are 16
// in-lane values, one DPP row sum and one exchange with lane ^ 16 per group.
template <bool GN>
__global__ __launch_bounds__(512, 1) void conv_ws8_kernel(ConvArgs p) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    char* const halo0 = smem;
    char* const aring = smem + 2 * W8_HALO + W8_STRIP;
    char* const ro = aring + W8_A_RING;
    float* const tb = reinterpret_cast<float*>(ro + W8_RO);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nchunks = (p.C0 + p.C1) / 32;
    const int S = 9 * nchunks;                       // steps per tile
    const int ntiles = p.PT * p.CT;                  // (4-image tile, 64-cout tile) pairs, cout fastest

    auto tile_of = [&](int q, W8Tile& t) {
        t.cot = q % p.CT;
        t.n0 = (q / p.CT) * 4;
    };

    int q = dxmi_xcd_logical(blockIdx.x, gridDim.x, p.xcd_order);
    if (q >= ntiles) return;
    const int qstride = gridDim.x;

    if (wave < 4) {
        // ================================================================ MFMA waves: image `wave` of the tile, 64 couts
        const int px = lane & 15, kg = lane >> 4;      // B: pixel / channel piece; A: cout / 8-channel group; D: pixel / 4-cout group
        // per halo buffer and kx: a column outside the map points into the zero strip, at the low address bits (banks) of the
        // slot it replaces; the strip is zero at every row offset read_b adds
        int bbase[2][3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int col = (px & 7) + kx - 1;
            const int low = (px >> 3) * W8_ROW + ((kg ^ ((col & 4) >> 1)) << 4);
            const bool inside = col >= 0 && col < 8;
#pragma unroll
            for (int b = 0; b < 2; ++b)
                bbase[b][kx] = inside ? b * W8_HALO + wave * W8_IMG + col * 64 + low : 2 * W8_HALO + (col & 3) * 64 + low;
        }
        const char* const abase = aring + ((kg >> 1) * 2048) + ((px + 32 * (kg & 1)) << 4);   // + slot*4096 + (cb16>>1)*1024 + (cb16&1)*256
        f32x4 acc[4][4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[cb][nb][r] = 0.f;
        bf16x8 A0[4], A1[4], Bx[2], By[2];
        // operands of step u of a chunk PAIR (u = 0..17: chunk parity u / 9, tap u % 9; u = 18 wraps)
        auto read_a = [&](int u, bf16x8 (&A)[4]) {
            const char* as = abase + (u % W8_RING) * W8_A_SLOT;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) A[cb] = *reinterpret_cast<const bf16x8*>(as + (cb >> 1) * 1024 + (cb & 1) * 256);
        };
        auto read_b = [&](int u, int half, bf16x8 (&B)[2]) {      // 16-pixel blocks 2 half, 2 half + 1: image rows 2 nb, 2 nb + 1
            const int t = u % 9, ky = t / 3, kx = t % 3;
            const char* hb = halo0 + bbase[(u / 9) & 1][kx];
#pragma unroll
            for (int i = 0; i < 2; ++i) B[i] = *reinterpret_cast<const bf16x8*>(hb + (2 * (half * 2 + i) + ky) * W8_ROW);
        };
        auto mfma8 = [&](const bf16x8 (&A)[4], const bf16x8 (&B)[2], int half) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
                    acc[cb][half * 2 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[cb], B[i], acc[cb][half * 2 + i], 0, 0, 0);
        };
        const float slope = dxmi_act_slope(p.act);
        const bool has_res = p.residual != nullptr;

        // the padding no DMA ever touches, once per launch: this wave's image's rows 0 and 9 in both buffers, and the strip
        {
            const uint4 z = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int b = 0; b < 2; ++b)
                *reinterpret_cast<uint4*>(halo0 + b * W8_HALO + wave * W8_IMG + (lane >> 5) * 9 * W8_ROW + (lane & 31) * 16) = z;
            for (int i = wave; i < W8_STRIP / 1024; i += 4) *reinterpret_cast<uint4*>(halo0 + 2 * W8_HALO + i * 1024 + lane * 16) = z;
        }
        lds_barrier();                                   // P0: tap 0 and the first halo chunk have landed, the padding is written
        read_a(0, A0);
        read_b(0, 0, Bx);
        for (;;) {
            const bool more = q + qstride < ntiles;
            f32x4 gam[4], bet[4];
            if constexpr (GN) {          // this tile's affine parameters: in flight under the K loop
                const int co0 = (q % p.CT) * 64 + 4 * kg;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    gam[cb] = *reinterpret_cast<const f32x4*>(p.gn_gamma + co0 + cb * 16);
                    bet[cb] = *reinterpret_cast<const f32x4*>(p.gn_beta + co0 + cb * 16);
                }
            }
            for (int c = 0; c < nchunks; c += 2) {
                // 8 MFMAs per half step with 2 / 6 operand reads spread between them; the barrier ends a group of three steps: the
                // next group's weights (at a chunk end: the next halo image) landed
                ws_k_pair<2, 3, 2, 6, 1, 2>(A0, A1, Bx, By, read_a, read_b, mfma8, [&](int) { if (!(WS_DBG(4))) lds_barrier(); });
            }
            lds_barrier();                               // E1: residual tile + bias / temb table of this tile landed
            {
                // per-lane base + compile-time offsets, the residual pieces of a cout block requested together, no activation
                // code when there is none (as conv_ws.hip)
                const bool plain = p.act == DXMI_ACT_NONE;
                char* const rowb = ro + ((wave * 64 + px) << 7) + 8 * (kg & 1);      // pixel row of block 0: blocks are 2 KiB apart
                // run-time switches hoisted out of the 16 (cb, nb) bodies (as conv_ws.hip, round 4): straight-line code per combination
                auto epi = [&](auto RES, auto MASK, auto ACT) {
                    constexpr bool kRes = decltype(RES)::value, kMask = decltype(MASK)::value, kAct = decltype(ACT)::value;
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) {
                        const int co = cb * 16 + 4 * kg;
                        const f32x4 b0 = *reinterpret_cast<const f32x4*>(tb + co), t0 = *reinterpret_cast<const f32x4*>(tb + 64 + wave * 64 + co);
                        f32x4 bv;
#pragma unroll
                        for (int e = 0; e < 4; ++e) bv[e] = b0[e] + t0[e];
                        char* const a0 = rowb + (((cb * 2 + (kg >> 1)) ^ (px & 7)) << 4);
                        bf16x4 r[4];
                        if constexpr (kRes) {
#pragma unroll
                            for (int nb = 0; nb < 4; ++nb) r[nb] = *reinterpret_cast<const bf16x4*>(a0 + nb * 2048);
                        }
#pragma unroll
                        for (int nb = 0; nb < 4; ++nb) {
                            f32x4 v;
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = acc[cb][nb][e] + bv[e];
                            if constexpr (kRes) {
                                if constexpr (kMask) {          // data gradient through a LeakyReLU: the fetched tile is the mask source
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[e] *= ((float)r[nb][e] > 0.f ? 1.f : p.mask_slope);
                                } else {
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[e] += (float)r[nb][e];
                                }
                            }
                            if constexpr (kAct) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) v[e] = dxmi_act_lin(v[e], slope);
                            }
                            bf16x4 o;
#pragma unroll
                            for (int e = 0; e < 4; ++e) o[e] = (bf16)v[e];
                            if constexpr (GN) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc[cb][nb][e] = (float)o[e];     // the value a separate launch would read
                            } else {
                                *reinterpret_cast<bf16x4*>(a0 + nb * 2048) = o;
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc[cb][nb][e] = 0.f;
                            }
                        }
                        if constexpr (GN) {
                            // group = couts cb * 16 + 8 (kg >> 1) .. + 7 over the image's 64 pixels: two-pass statistics, fixed order
                            float s = 0.f;
#pragma unroll
                            for (int nb = 0; nb < 4; ++nb) s += (acc[cb][nb][0] + acc[cb][nb][1]) + (acc[cb][nb][2] + acc[cb][nb][3]);
                            s = dxmi_row16_sum(s);
                            s += __shfl_xor(s, 16, 64);
                            const float mean = s * (1.f / 512.f);
                            float qv = 0.f;
#pragma unroll
                            for (int nb = 0; nb < 4; ++nb) {
                                float d[4];
#pragma unroll
                                for (int e = 0; e < 4; ++e) d[e] = acc[cb][nb][e] - mean;
                                qv += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
                            }
                            qv = dxmi_row16_sum(qv);
                            qv += __shfl_xor(qv, 16, 64);
                            const float rstd = rsqrtf(qv * (1.f / 512.f) + p.gn_eps);
                            float ga[4], be[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                ga[e] = gam[cb][e] * rstd;               // same form as groupnorm_silu_kernel
                                be[e] = bet[cb][e] - mean * ga[e];
                            }
#pragma unroll
                            for (int nb = 0; nb < 4; ++nb) {
                                bf16x4 y;
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    float t = acc[cb][nb][e] * ga[e] + be[e];
                                    if (p.gn_flags & 1) t = dxmi_silu_fast(t);
                                    y[e] = (bf16)t;
                                    acc[cb][nb][e] = 0.f;
                                }
                                *reinterpret_cast<bf16x4*>(a0 + nb * 2048) = y;
                            }
                        }
                    }
                };
                using T_ = std::true_type;
                using F_ = std::false_type;
                const bool is_mask = has_res && p.res_is_mask;
                if (plain && !is_mask) { if (has_res) epi(T_{}, F_{}, F_{}); else epi(F_{}, F_{}, F_{}); }
                else if (is_mask) { if (plain) epi(T_{}, T_{}, F_{}); else epi(T_{}, T_{}, T_{}); }
                else if (has_res) epi(T_{}, F_{}, T_{});
                else epi(F_{}, F_{}, T_{});
            }
            lds_barrier();                               // E2: output tile complete, the bulk movers may drain it
            if (!more) break;
            q += qstride;
        }
        return;
    }

    if (wave < 6) {
        // ================================================================ weight loaders (waves 4, 5): k-step lw of every tap
        const int lw = wave - 4;
        const char* const wb = reinterpret_cast<const char*>(p.w) + (size_t)lane * 16;
        W8Tile cur;
        tile_of(q, cur);
        // register-staged weight stream, two 1-KiB fragments per tap and loader, handed over in groups of three steps
        const int NG = S / 3;                           // groups per tile (even)
        u32x4 fq[2][3][2];
        const WsWeightStream<2, false> ws{p, aring, wb, lw, lane, NG, fq};
        static_assert(ws.SLOT == W8_A_SLOT && ws.RING == W8_RING, "group hand-over needs the six-slot ring");
        // residual pieces of a tile switch (see the bulk movers: piece L = k*128 + t2, t2 = lw*64 + lane): fetched here one
        // group step after the bulk movers drained the piece (conv_ws.hip, round 4)
        const int t2l = lw * 64 + lane;
        const int kpc_l = (16 + nchunks - 2) / (nchunks - 1), pps_l = (kpc_l + 7) >> 3;
        const char* const zero_page_l = reinterpret_cast<const char*>(p.mask_src);
        auto piece_off_l = [&](const W8Tile& t, int k) -> long {
            const int lp = k * 16 + (t2l >> 3);
            const int c8 = (t2l & 7) ^ (lp & 7);
            const int n = t.n0 + (lp >> 6);
            if (n >= p.N) return -1;
            return (long)((((size_t)n * 8 + ((lp >> 3) & 7)) * 8 + (lp & 7)) * p.Cout + t.cot * 64 + c8 * 8);
        };
        bool first_tile_l = true;
        ws.prologue(cur.cot);
        lds_barrier();                                       // P0
        for (;;) {
            const bool more = q + qstride < ntiles;
            W8Tile nxt = cur;
            if (more) tile_of(q + qstride, nxt);
            const bool res_here = !first_tile_l && p.residual != nullptr;
            first_tile_l = false;
            for (int G0 = 0; G0 < NG; G0 += 2) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int G = G0 + j;
                    ws.hand_over(j, G);
                    if (res_here && G > 0) {
                        const int cg = (G - 1) / 3, g3 = (G - 1) - cg * 3;     // the group step whose pieces were drained
                        if (cg + 1 < nchunks) {
                            const int k0 = cg * kpc_l < 16 ? cg * kpc_l : 16, k1 = k0 + kpc_l < 16 ? k0 + kpc_l : 16;
                            const int s0 = 3 * g3, s1 = g3 < 2 ? 3 * g3 + 3 : 8;       // steps of the group that carry pieces (t < 8)
                            const int ka = k0 + s0 * pps_l < k1 ? k0 + s0 * pps_l : k1, kb = k0 + s1 * pps_l < k1 ? k0 + s1 * pps_l : k1;
#pragma unroll 1
                            for (int k = ka; k < kb; ++k) {
                                const long o = piece_off_l(cur, k);
                                const void* g = o >= 0 ? (const void*)(p.residual + o) : (const void*)zero_page_l;
                                __builtin_amdgcn_global_load_lds(WS_GPTR(g), WS_LPTR(ro + (k * 128 + lw * 64) * 16), 16, 0, 0);
                            }
                        }
                    }
                    ws.refill(j, G, cur.cot, more ? nxt.cot : cur.cot);
                    if (!(WS_DBG(4))) lds_barrier();                         // end of group step G
                }
            }
            lds_barrier();                                        // E1
            lds_barrier();                                        // E2
            if (!more) break;
            q += qstride;
            cur = nxt;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }

    // ==================================================================== bulk movers (waves 6, 7)
    {
        const int bw = wave - 6;
        const int t2 = bw * 64 + lane;                     // 0..127 over the two waves
        constexpr int HB2 = W8_HALO_BLOCKS / 2;            // halo blocks per wave (block bw + 2k): row pair blk & 3 of image blk >> 2
        // per tile each lane keeps the BYTE offset of its source piece inside either concat part (-1: an image past the end of
        // the batch): a DMA address per chunk is then one 64-bit add and a select (no 64-bit multiply, no GOT load of the zero
        // page per DMA).  Every block is interior pixels only.
        const char* const zero_page = reinterpret_cast<const char*>(p.mask_src);    // 16 zero bytes (host: &w8_zero16)
        int hoff0[HB2], hoff1[HB2];
        auto halo_plan = [&](const W8Tile& t) {
#pragma unroll
            for (int k = 0; k < HB2; ++k) {
                const int blk = bw + 2 * k;
                const int sub = blk >> 2, iy = (blk & 3) * 2 + (lane >> 5), ix = (lane >> 2) & 7;
                const bool ok = t.n0 + sub < p.N;
                // nearest x2 upsample in front of the conv (Upsample 4x4 -> 8x8): virtual pixel (iy, ix) is source pixel (iy / 2, ix / 2)
                const int pix = p.ups ? ((t.n0 + sub) * 4 + (iy >> 1)) * 4 + (ix >> 1) : ((t.n0 + sub) * 8 + iy) * 8 + ix;
                const int j8 = ((lane & 3) ^ ((ix & 4) >> 1)) * 8;
                hoff0[k] = ok ? (pix * p.C0 + j8) * 2 : -1;
                hoff1[k] = ok ? (pix * p.C1 + j8) * 2 : -1;
            }
        };
        auto halo_issue = [&](int c, char* buf, int ka, int kb) {     // blocks ka .. kb-1 of this wave's share (compile-time range)
            if (WS_DBG(2)) return;
            const int cbase = c * 32;
            const bool first = cbase < p.C0;
            const char* base = reinterpret_cast<const char*>(first ? p.in0 : p.in1) + (first ? cbase : cbase - p.C0) * 2;
#pragma unroll
            for (int k = 0; k < HB2; ++k) {
                if (k < ka || k >= kb) continue;
                const int blk = bw + 2 * k;
                const int off = first ? hoff0[k] : hoff1[k];
                const char* g = off >= 0 ? base + off : zero_page;
                __builtin_amdgcn_global_load_lds(WS_GPTR(g), WS_LPTR(buf + (blk >> 2) * W8_IMG + W8_ROW + (blk & 3) * 1024), 16, 0, 0);
            }
        };
        // output-tile pieces of this thread: L = k*128 + t2 (k = 0..15): pixel lp = k*16 + (t2 >> 3), cout piece (t2 & 7) ^ (lp & 7)
        // (-1: the piece belongs to an image past the end of the batch — the last tile of a batch that is not a multiple of 4)
        auto piece_off = [&](const W8Tile& t, int k) -> long {
            const int lp = k * 16 + (t2 >> 3);
            const int c8 = (t2 & 7) ^ (lp & 7);
            const int n = t.n0 + (lp >> 6);
            if (n >= p.N) return -1;
            return (long)((((size_t)n * 8 + ((lp >> 3) & 7)) * 8 + (lp & 7)) * p.Cout + t.cot * 64 + c8 * 8);
        };
        auto fetch_table = [&](const W8Tile& t) {            // bias[64] and the four images' temb rows: 4-byte DMA, 256 B per instruction
            if (bw != 0) return;
            if (p.bias) __builtin_amdgcn_global_load_lds(WS_GPTR(p.bias + t.cot * 64 + lane), WS_LPTR(tb), 4, 0, 0);
            if (p.addvec) {
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    const int n = t.n0 + sub < p.N ? t.n0 + sub : p.N - 1;      // images past the batch: any valid row (results discarded)
                    __builtin_amdgcn_global_load_lds(WS_GPTR(p.addvec + (size_t)n * p.addvec_ld + t.cot * 64 + lane),
                                                     WS_LPTR(tb + 64 + sub * 64), 4, 0, 0);
                }
            }
        };
        bool do_res = p.residual != nullptr;       // prologue only: from the second tile on the loaders fetch the residual tile
        auto fetch_residual = [&](const W8Tile& t, int k0, int k1) {
            if (!do_res) return;
#pragma unroll 1
            for (int k = k0; k < k1; ++k) {
                const long o = piece_off(t, k);
                const void* g = o >= 0 ? (const void*)(p.residual + o) : (const void*)zero_page;
                __builtin_amdgcn_global_load_lds(WS_GPTR(g), WS_LPTR(ro + (k * 128 + bw * 64) * 16), 16, 0, 0);
            }
        };
        // pieces k0 .. k1-1 of the tile switch: previous tile's output pieces out, this tile's residual pieces into the same
        // LDS rows (a wave refills exactly the rows it drained).  Returns the vector-memory operations it issued.
        auto tile_switch = [&](const W8Tile& pt, const W8Tile& ct, int k0, int k1) -> int {
#pragma unroll 1
            for (int k = k0; k < k1; k += 2) {
                const int n = k1 - k < 2 ? k1 - k : 2;
                bf16x8 v[2];
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (u < n) v[u] = *reinterpret_cast<const bf16x8*>(ro + ((k + u) * 128 + t2) * 16);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const long o = u < n ? piece_off(pt, k + u) : -1;
                    // predicated per lane; the store still counts once in vmcnt for the wave whenever u < n
                    if (u < n) {
                        if (o >= 0) *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16*>(p.out) + o) = v[u];
                    }
                }
                fetch_residual(ct, k, k + n);
            }
            // a store whose lanes all belong to images past the batch is skipped entirely: such tiles' stores are not counted
            // (a count that is too LOW only waits for more)
            return (k1 - k0) * ((pt.n0 + 4 <= p.N ? 1 : 0) + (do_res ? 1 : 0));
        };

        W8Tile cur;
        tile_of(q, cur);
        // table rows that no DMA fills stay zero
        if (bw == 0) {
            if (!p.bias) tb[lane] = 0.f;
            if (!p.addvec) { tb[64 + lane] = 0.f; tb[128 + lane] = 0.f; tb[192 + lane] = 0.f; tb[256 + lane] = 0.f; }
        }
        halo_plan(cur);
        halo_issue(0, halo0, 0, HB2);
        fetch_table(cur);
        fetch_residual(cur, 0, 16);
        // P0 needs the halo image and the table, not the residual tile (16 younger DMAs; E1's vmcnt(0) covers them)
        if (do_res) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();                                           // P0
        do_res = false;
        bool have_prev = false;
        W8Tile prev = cur;
        const int kpc = (16 + nchunks - 2) / (nchunks - 1);      // tile-switch pieces per chunk (first nchunks-1 chunks)
        const int pps = (kpc + 7) >> 3;                          // ... per step
        for (;;) {
            const bool more = q + qstride < ntiles;
            W8Tile nxt = cur;
            if (more) tile_of(q + qstride, nxt);
            for (int c = 0; c < nchunks; ++c) {
                const bool wrap = c + 1 == nchunks;
                if (c == 0 && have_prev) fetch_table(cur);       // older than this chunk's halo DMAs: complete at its last barrier
                if (wrap && more) halo_plan(nxt);
                const bool do_halo = !wrap || more;
                char* const hbuf = halo0 + ((c + 1) & 1) * W8_HALO;
                const int hc = wrap ? 0 : c + 1;
                int k0 = 16, k1 = 16;
                if (have_prev && !wrap) {
                    k0 = c * kpc < 16 ? c * kpc : 16;
                    k1 = k0 + kpc < 16 ? k0 + kpc : 16;
                }
                int young = 0;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    if (t < 6 && do_halo) halo_issue(hc, hbuf, t < 2 ? 2 * t : t + 2, t < 2 ? 2 * t + 2 : t + 3);    // 2, 2, 1, 1, 1, 1
                    if (t < 8) {
                        const int ka = k0 + t * pps < k1 ? k0 + t * pps : k1, kb = ka + pps < k1 ? ka + pps : k1;
                        if (ka < kb) {
                            const int n = tile_switch(prev, cur, ka, kb);
                            if (t >= 5) young += n;              // issued after the last halo block of this chunk
                        }
                    }
                    if (t == 8) {
                        // halo image (and everything older) landed; at the last chunk E1 needs the whole residual tile
                        if (wrap) ws_wait_vm<12>(0);
                        else ws_wait_vm<12>(young);
                    }
                    if (t % 3 == 2 && !(WS_DBG(4))) lds_barrier();                // end of a group step
                }
            }
            lds_barrier();                                        // E1
            lds_barrier();                                        // E2
            prev = cur;
            have_prev = true;
            if (!more) break;
            q += qstride;
            cur = nxt;
        }
        // last tile out
#pragma unroll 1
        for (int k = 0; k < 16; k += 4) {
            bf16x8 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const bf16x8*>(ro + ((k + u) * 128 + t2) * 16);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long o = piece_off(prev, k + u);
                if (o >= 0) *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16*>(p.out) + o) = v[u];
            }
        }
    }
}

}  // namespace

// The 8x8-map wave-specialised kernel's scope and tiling.
bool conv_ws8_select(const ConvArgs& a, ConvPlan* p) {
    if (a.in_mode != DXMI_IN_NHWC_BF16 || a.out_mode != DXMI_OUT_NHWC_BF16) return false;
    if (a.ksize != 3 || a.stride != 1 || a.pad != 1 || a.ups == 2 || (a.mask_src && a.residual) || a.act == DXMI_ACT_SILU) return false;   // a mask alone rides the residual path
    if (a.OH != 8 || a.OW != 8) return false;
    if (a.ups ? (a.IH != 4 || a.IW != 4) : (a.IH != 8 || a.IW != 8)) return false;     // ups: nearest x2 upsample of a 4x4 map in front
    if (a.Cout % 64 != 0 || (a.C0 + a.C1) % 32 != 0 || a.C0 % 32 != 0) return false;
    const int nchunks = (a.C0 + a.C1) / 32;
    if (nchunks < 4 || nchunks % 2 != 0 || (9 * nchunks) % W8_RING != 0) return false;
    // no batch-size condition: an image's result must not depend on the batch it rides in (the kernels differ in summation order)
    if ((long)a.N * 64 * (a.C0 > a.C1 ? a.C0 : a.C1) * 2 >= (1L << 31)) return false;   // 32-bit byte offsets inside either input part
    p->gn_out = (a.gn_flags & 2) != 0;       // the fused GroupNorm replaces the raw output (one output tile in LDS)
    if (a.gn_out && !p->gn_out) return false;
    ConvArgs& b = p->args;
    if (a.mask_src) { b.residual = a.mask_src; b.res_is_mask = 1; }
    if (a.gn_out) b.out = a.gn_out;       // the movers drain the (normalised) tile to the fused output
    b.SUBS = 4;
    b.PT = (a.N + 3) / 4;      // the last tile may hold fewer than four images (masked)
    b.CT = a.Cout / 64;
    b.tile_px = 256;
    b.xcd_order = 1;
    p->kind = ConvKernel::ws8; p->t0 = a.gn_out != nullptr;
    p->grid = b.PT * b.CT < 256 ? b.PT * b.CT : 256;
    p->lds = 2 * W8_HALO + W8_STRIP + W8_A_RING + W8_RO + W8_TB;
    p->id = 400008;    // conv_ws8_kernel
    return true;
}

int conv_ws8_launch(const ConvPlan& p, hipStream_t st) {
    static const void* zero_page = nullptr;
    DXMI_CHECK_ARG(conv_zero_page(zero_page, HIP_SYMBOL(w8_zero16)), "dxmi_conv2d_fwd(ws8): hipGetSymbolAddress(w8_zero16) failed");
    ConvArgs b = p.args;
    b.mask_src = reinterpret_cast<const bf16*>(zero_page);    // the field carries the zero page (a mask source travels in `residual`)
#ifdef DXMI_CONV_STAMPS
    static const int dbg = getenv("DXMI_CONV_WS8_DBG") ? atoi(getenv("DXMI_CONV_WS8_DBG")) : 0;
    b.stagger = dbg;
#endif
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_ws8_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_ws8_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    if (p.t0) hipLaunchKernelGGL(conv_ws8_kernel<true>, dim3(p.grid), dim3(512), p.lds, st, b);
    else hipLaunchKernelGGL(conv_ws8_kernel<false>, dim3(p.grid), dim3(512), p.lds, st, b);
    DXMI_CHECK_LAUNCH("dxmi_conv2d_fwd(ws8)");
    return DXMI_OK;
}
