// Shared pieces of the wave-specialised kernels (MFMA waves fed from LDS only, dedicated mover waves): the address-space casts of
// the LDS DMA builtin, exact vmcnt waits, the MFMA / LDS-read interleave, the diagnostic build's ablation switch and the zero page
// (conv_ws, conv_ws8, conv_ws_up, conv_sm, conv1x1_rw, conv1x1_rw8, conv_head, conv_wgrad, attention, attn_block), and the two
// pieces conv_ws_kernel and conv_ws8_kernel run in the same form: the MFMA waves' K loop over a chunk pair (ws_k_pair) and the
// weight loaders' register-staged stream (WsWeightStream).  The workgroup barrier of these kernels is common.h's lds_barrier().
// What is shared, what stayed per kernel and the instruction-stream comparison: DESIGN.md 5.38.
#pragma once
#include "conv_common.h"

// operands of __builtin_amdgcn_global_load_lds
#define WS_GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define WS_LPTR(p) ((__attribute__((address_space(3))) void*)(p))

// 16 zero bytes in global memory, the DMA source of padding and out-of-range pieces.  One symbol per translation unit: each
// launcher takes its own page's address (conv_zero_page).
#define WS_ZERO_PAGE(name) __device__ uint4 name = {0u, 0u, 0u, 0u}

// Timing-only ablations of the diagnostic build (make STAMPS=1): bits of the family's DXMI_CONV_*_DBG variable, handed to the
// kernel in ConvArgs::stagger (`p` at the point of use); compiled out of the product library.
#ifdef DXMI_CONV_STAMPS
#define WS_DBG(bit) (p.stagger & (bit))
#else
#define WS_DBG(bit) 0
#endif

// `reps` x (`m` MFMAs, one LDS read), then `tail` MFMAs: how the operand reads of the next half step are spread between the
// MFMAs (16 cycles each) of the current one
#define WS_INTERLEAVE(reps, m, tail)                                  \
    do {                                                              \
        _Pragma("unroll") for (int i_ = 0; i_ < (reps); ++i_) {       \
            __builtin_amdgcn_sched_group_barrier(0x008, (m), 0);      \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);        \
        }                                                             \
        __builtin_amdgcn_sched_group_barrier(0x008, (tail), 0);       \
    } while (0)

// s_waitcnt vmcnt(n) for a wave-uniform run-time n (the instruction takes an immediate): n is rounded DOWN to an even count and
// capped at MAX (even, <= 26), both of which only wait for more.  MAX is the largest count the caller can have in flight.
template <int MAX>
__device__ __forceinline__ void ws_wait_vm(int n) {
    static_assert(MAX % 2 == 0 && MAX <= 26, "vmcnt case list");
#define WS_VM_CASE(k)                                                       \
    case k:                                                                 \
        if constexpr (2 * (k) < MAX) {                                      \
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (k)) : "memory");  \
            break;                                                          \
        }                                                                   \
        [[fallthrough]];
    switch (n >> 1) {
        WS_VM_CASE(0) WS_VM_CASE(1) WS_VM_CASE(2) WS_VM_CASE(3) WS_VM_CASE(4) WS_VM_CASE(5) WS_VM_CASE(6)
        WS_VM_CASE(7) WS_VM_CASE(8) WS_VM_CASE(9) WS_VM_CASE(10) WS_VM_CASE(11) WS_VM_CASE(12)
    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MAX) : "memory"); break;
    }
#undef WS_VM_CASE
}

// The MFMA waves' K loop over one chunk PAIR: 18 steps (chunk parity u / 9, tap u % 9) of straight-line code, no branches inside
// (a branch makes hipcc wait lgkmcnt(0) at the join, which exposes the latency of the operand reads just issued).  A step is two
// half steps of NB pixel blocks x 4 cout blocks of MFMAs; every half step requests the operands of the next one: the other NB
// pixel blocks of this step, then — behind the barrier that says they landed — the weights and first NB blocks of the next step.
// The loaders hand over three ring slots at a time, so there is one barrier per GROUP of three steps (a barrier per step cost
// 11-15 % by itself).  Step 18's first operands (the next pair's, or the next tile's: in LDS when the last barrier opens) are
// requested unconditionally.
//   read_a(u, A) / read_b(u, half, B): operand reads of step u at per-lane bases + compile-time offsets (the halo layouts differ);
//   mfma(A, B, half): the half step's MFMAs; barrier(u): the group barrier behind step u (u % 3 == 2);
//   R0, M0, T0 / R1, M1, T1: WS_INTERLEAVE shape (reps, m, tail) of the first / second half step.
template <int R0, int M0, int T0, int R1, int M1, int T1, int NB, class ReadA, class ReadB, class Mfma, class Barrier>
__device__ __forceinline__ void ws_k_pair(bf16x8 (&A0)[4], bf16x8 (&A1)[4], bf16x8 (&Bx)[NB], bf16x8 (&By)[NB], ReadA read_a, ReadB read_b,
                                          Mfma mfma, Barrier barrier) {
#pragma unroll
    for (int u = 0; u < 18; ++u) {
        read_b(u, 1, By);
        if (u & 1) mfma(A1, Bx, 0); else mfma(A0, Bx, 0);
        WS_INTERLEAVE(R0, M0, T0);
        if (u % 3 == 2) barrier(u);
        if (u & 1) read_a(u + 1, A0); else read_a(u + 1, A1);
        read_b(u + 1, 0, Bx);
        if (u & 1) mfma(A1, By, 1); else mfma(A0, By, 1);
        WS_INTERLEAVE(R1, M1, T1);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The weight loaders' register-staged stream (waves 4 and 5: k-step lw of every tap), handed over in GROUPS of three steps.  The
// ring's six slots are two groups: the MFMA waves read group G (slots of parity G & 1) while the loader writes group G + 1 into
// the other three slots (last read in group G - 1: complete at the barrier that ended it) from registers, with ds_write_b128.  The
// fragments were requested two group steps earlier by plain global_load_dwordx4 into one of two register sets of 3 x FR x 4
// registers: a `global_load_lds` costs its wave ~190 cycles of issue and takes twice the issue slots from the MFMA wave on its
// SIMD (tools/dma_probe.hip, tools/stage_probe.hip).  vmcnt retires in order: each wait leaves the 3 FR loads of the younger
// group in flight.
//   FR: 1-KiB fragments per tap and loader (a ring slot is 2 FR KiB);
//   CLAMP: the cout tile may be half empty (Cout % 128 == 64): its missing fragments re-read the last valid one, results unused;
//          without it fragment k of cout tile cot is block cot * FR + k.
template <int FR, bool CLAMP>
struct WsWeightStream {
    static constexpr int SLOT = 2 * FR * 1024, RING = 6;
    // The kernel's own variables, by reference as the lambdas this replaced captured them: the form that compiles to the same
    // instructions.  `wb` must stay computed in the kernel IN FRONT of tile_of(): behind it hipcc recomputes the tile's division
    // in the loader branch and the kernels' scalar spill counts change.
    const ConvArgs& p;
    char* const& aring;
    const char* const& wb;       // packed weights + this lane's 16 bytes of a fragment
    const int& lw;
    const int& lane;
    const int& NG;               // groups per tile: 3 nchunks (even)
    u32x4 (&fq)[2][3][FR];       // the two register sets

    __device__ __forceinline__ void load_tap(int cot, int g, u32x4 (&f)[FR]) const {       // (chunk, tap) g = 9 c + t of cout tile cot
        if (!CLAMP && WS_DBG(1)) return;       // diagnostic build, conv_ws8 only: no weight stream
        const int c = g / 9, t = g - c * 9;
        const char* src = wb + ((size_t)(t * p.KST + c * 2 + lw) * p.CB + (CLAMP ? 0 : cot * FR)) * 1024;
#pragma unroll
        for (int k = 0; k < FR; ++k) {
            const int cb = !CLAMP ? k : cot * FR + k < p.CB ? cot * FR + k : p.CB - 1;
            // inline asm: hipcc's own wait-count pass loses the count of loads in flight across the loop's back edge and
            // drains the queue (s_waitcnt vmcnt(0)) before the first ds_write of every trip; the waits below are exact
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(f[k]) : "v"(src + (size_t)cb * 1024) : "memory");
        }
    }
    __device__ __forceinline__ void store_tap(int g, const u32x4 (&f)[FR]) const {
        char* dst = aring + (g % RING) * SLOT + lw * (FR * 1024) + lane * 16;
#pragma unroll
        for (int k = 0; k < FR; ++k) *reinterpret_cast<u32x4*>(dst + k * 1024) = f[k];
    }
    // group G of the current tile, or group G - NG of the next one (past the last tile: the current tile's again, unused)
    __device__ __forceinline__ void load_group(int G, int cot_cur, int cot_nxt, u32x4 (&f)[3][FR]) const {
        const bool nx = G >= NG;
        const int g0 = (nx ? G - NG : G) * 3, cot = nx ? cot_nxt : cot_cur;
#pragma unroll
        for (int j = 0; j < 3; ++j) load_tap(cot, g0 + j, f[j]);
    }
    __device__ __forceinline__ void store_group(int G, const u32x4 (&f)[3][FR]) const {     // ring slots depend on G's parity only (NG even)
#pragma unroll
        for (int j = 0; j < 3; ++j) store_tap((G & 1) * 3 + j, f[j]);
    }
    __device__ __forceinline__ void wait_group() const { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * FR) : "memory"); }

    // up to the barrier P0 (whose lgkmcnt(0) says group 0 is in LDS): group 0 written, groups 1 and 2 in flight
    __device__ __forceinline__ void prologue(int cot) const {
        load_group(0, cot, cot, fq[0]);
        load_group(1, cot, cot, fq[1]);
        wait_group();
        store_group(0, fq[0]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        load_group(2, cot, cot, fq[0]);
    }
    // Group step G = G0 + j, j = G & 1 a compile-time constant (the MFMA waves read group G; the caller ends the step with the group
    // barrier).  hand_over: group G + 1, in set (j + 1) & 1 since group step G - 1, has landed and is written; refill: the set is
    // requested again, for group G + 3.  The kernel issues its residual-piece DMAs between the two: older than the refill, so the
    // next wait but one covers them.
    __device__ __forceinline__ void hand_over(int j, int G) const {
        wait_group();                                       // group G + 2's loads stay in flight
        store_group(G + 1, fq[(j + 1) & 1]);
        // the barrier's lgkmcnt(0) must precede the refill: a ds_write reads its data registers when it executes
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __device__ __forceinline__ void refill(int j, int G, int cot_cur, int cot_nxt) const { load_group(G + 3, cot_cur, cot_nxt, fq[(j + 1) & 1]); }
};
