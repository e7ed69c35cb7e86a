// Sample-quality metrics of the ADM evaluator on the device: improved precision / recall (k-NN radii and manifold
// membership, Kynkaenniemi et al.) and the Inception Score's softmax statistics.
//
// Reference: evaluations/evaluator.py.  ManifoldEstimator.manifold_radii (:243-280: the k-th entry of np.partition of each row
// of the set-against-itself squared-distance matrix, nhood_sizes=(3,), clamp_to_percentile=None), evaluate_pr /
// DistanceBlock.less_thans (:328-417: any_i d(a_i, b_j) <= r_a[i] and any_j d(a_i, b_j) <= r_b[j]), _batch_pairwise_distances
// (:420-436: max(|u|^2 - 2 u.v + |v|^2, 0)), Evaluator.compute_inception_score (:179-193: softmax(pool3 . W) with the
// `softmax/logits/MatMul` weight only, splits of 5000, exp of the mean KL to the split marginal, mean over splits).
//
// One distance definition, used by every kernel here:
//     d(u, v) = max((|u|^2 + |v|^2) - 2 (u . v), 0)                                              (f32)
// u . v is a K-ordered fmaf chain: v_mfma_f32_32x32x2_f32 over the feature index in increasing order, one accumulator per pair
// and no K split (the MFMA's f32 products are exact and it accumulates k0 then k1, MI355X_MICROARCH.md).  |u|^2 is the same chain
// of u against itself (row_sqnorm_kernel), so d(u, u) == 0 exactly, and a pair's distance is bitwise the same value whatever its
// tile, its column split, which kernel computed it and whether it was evaluated as (u, v) or (v, u).  There is no fp16 path: the
// reference's fp16 distances with an fp32 retry on overflow are one f32 path here.
//
//   row_sqnorm_kernel     X [N, D] -> |x|^2 [N] (one thread per row, sequential fmaf)
//   knn_radii_kernel      (row tile 128) x (a contiguous range of 128-column tiles, one split): 128 x 128 dot tile on the f32 MFMA
//                         (4 waves x 64 x 64, K chunks of 16 through LDS), distances into LDS, two threads per row keep the k+1
//                         smallest values of their 64 columns in registers (min/max insertion network) across the split
//   knn_merge_kernel      per row: the 2 S partial lists -> the value at sorted position k = radius
//   flags_clear_kernel    zero both flag arrays
//   pr_member_kernel      one 128 x 128 tile of |A| x |B| distances, both OR-reductions in the epilogue (column flags per lane,
//                         row flags by a wave ballot), flags written as plain stores of 1 (idempotent)
//   is_logits_kernel      logits = pool3 [n, D] . W^T with W = fc.weight [C, D] (the same dot tile), f32
//   is_softmax_kernel     row softmax in f32 (one wave per row)
//   is_marginal_kernel    log p_bar[c] = log(sum_r p[r][c] / n) in fp64, sequential over rows
//   is_kl_kernel          kl[r] = sum_c p (log p - log p_bar) in fp64 (one wave per row, fixed shuffle tree)
//   is_split_mean_kernel  mean_r kl[r] in fp64, fixed order -> one value per split (exp and the mean over splits: host)
//
// Two metrics on the same dot / distance that the reference evaluator does not have:
//   kid_tile_kernel       Kernel Inception Distance (Binkowski et al. 2018): one 128 x 128 dot tile of one subset's X.X, Y.Y or
//                         X.Y (rows gathered through the subset's index list in the tile loader), k = ((double)dot gamma + coef0)^3
//                         and the tile's sum in fp64 -> one partial per workgroup.  X.X and Y.Y: tiles with column tile >= row
//                         tile only, strictly upper tiles doubled, i == j dropped.  One launch over all subsets, no atomics
//   kid_reduce_kernel     per subset: its partials -> Sxx, Syy, Sxy in a fixed order; NaN for an index out of range
//   dc_count_kernel       density / coverage (Naeem et al. 2020): knn_radii_kernel's grid; counts[i] = #{j : d(a_i, b_j) < rA[i]}
//                         (strict), per-row counts in registers by ballot + popcount, one int per row and split
//   dc_merge_kernel       per row: the sum over the splits
//
// Roofline (f32 MFMA, 155 TFLOP/s measured, MI355X_MICROARCH.md):
//   radii      2 N^2 D FLOP over N D 4 bytes read (each 128-row panel re-read once per column tile from L2/HBM: 32 FLOP per
//              byte of L2 traffic, 2 N^2 D 4 / 128 ... bytes); MFMA-bound.  N = 50 000, D = 2048: 10.2 TFLOP, floor 66 ms.
//   membership 2 |A| |B| D FLOP; 10 000 x 50 000 x 2048: 2.0 TFLOP, floor 13 ms.  Epilogue: ~4 VALU per distance against
//              4096 MFMA FLOP per distance.
//   KID        2 D (mx (mx + 1) / 2 + my (my + 1) / 2 + mx my) FLOP per subset with the symmetric halves; 100 x 1000 x 1000 at
//              D = 2048: 0.82 TFLOP, floor 5.3 ms; all rows of 50 000 x 50 000: 20 TFLOP, floor 132 ms.  Epilogue: ~6 fp64 VALU
//              per pair.  counts: membership's FLOP and floor; epilogue one compare and a ballot per pair row.
//   IS logits  2 N D C FLOP (50 000 x 2048 x 1008: 0.21 TFLOP, floor 1.3 ms); the softmax and fp64 reductions read N C 4 bytes
//              three times (HBM-bound, ~0.1 ms at 50 000 x 1008).
#include "common.h"

namespace {

constexpr int EM_T = 128;            // tile edge: rows of the row set, rows of the column set
constexpr int EM_KC = 16;            // features per LDS chunk
constexpr int EM_LD = EM_T + 4;      // staging row pitch (floats)
constexpr int EM_DLD = EM_T + 1;     // distance tile pitch (floats): thread-per-row scans are conflict-free
constexpr int EM_STAGE_FLOATS = 2 * 2 * EM_KC * EM_LD;       // 2 buffers x 2 operands
constexpr int EM_DTILE_FLOATS = EM_T * EM_DLD;
constexpr int EM_KMAX = 7;           // largest neighbourhood size k (k + 1 kept values per row)

__device__ __forceinline__ float em_pair_dist(float nu, float nv, float dot) {
    // (nu + nv) is commutative in f32 and 2 * dot is exact, so the value does not depend on which vector is the row
    return fmaxf((nu + nv) - 2.f * dot, 0.f);
}

__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ x, float* __restrict__ out, long N, int D) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const float* row = x + r * D;
    float s = 0.f;
    if ((D & 3) == 0) {
        for (int k = 0; k < D; k += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
            s = fmaf(v[0], v[0], s); s = fmaf(v[1], v[1], s); s = fmaf(v[2], v[2], s); s = fmaf(v[3], v[3], s);
        }
    } else {
        for (int k = 0; k < D; ++k) s = fmaf(row[k], row[k], s);
    }
    out[r] = s;
}

// acc[u][v] (32 x 32 MFMA accumulators) <- X[r0 + i] . Y[c0 + j] over the full feature range, i, j < 128.  Rows at or past nx / ny
// read as zeros.  D layout of the 32x32 MFMA: j = wj*64 + v*32 + lane%32, i = wi*64 + u*32 + (lane/32)*4 + 8q + e (register 4q + e).
// GATHER: tile row n is X[ix[n]] for n < mx and column n is Y[iy[n]] for n < my (a subset addressed through its index list, no
// gathered copy); positions past mx / my and indices outside [0, nx) / [0, ny) read as zeros and are never dereferenced.
template <bool GATHER = false>
__device__ __forceinline__ void em_dot_tile(const float* __restrict__ X, long nx, const float* __restrict__ Y, long ny, int D, long r0,
                                            long c0, float* smem, f32x16 (&acc)[2][2], const int32_t* __restrict__ ix = nullptr,
                                            long mx = 0, const int32_t* __restrict__ iy = nullptr, long my = 0) {
    float (*As)[EM_KC][EM_LD] = reinterpret_cast<float (*)[EM_KC][EM_LD]>(smem);
    float (*Bs)[EM_KC][EM_LD] = reinterpret_cast<float (*)[EM_KC][EM_LD]>(smem + 2 * EM_KC * EM_LD);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = wave >> 1, wj = wave & 1;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    // loader: element p (0, 1) of thread tid -> tile row (tid + 256 p) / 4, feature quad (tid % 4); 4 lanes read one row's 64 bytes
    const int kq = tid & 3, rl = tid >> 2;
    const bool vec = (D & 3) == 0;
    f32x4 ra[2], rb[2];
    auto load_row = [&](const float* base, long n, long lim, int k0) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (n < lim) {
            const float* p = base + n * D;
            const int k = k0 + kq * 4;
            if (vec && k + 3 < D) v = *reinterpret_cast<const f32x4*>(p + k);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (k + e < D) v[e] = p[k + e];
            }
        }
        return v;
    };
    // source rows of this thread's two tile rows and two tile columns (nx / ny: reads as zeros)
    long ga[2], gb[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        ga[p] = r0 + rl + 64 * p;
        gb[p] = c0 + rl + 64 * p;
        if constexpr (GATHER) {
            const long a = ga[p] < mx ? (long)ix[ga[p]] : -1, b = gb[p] < my ? (long)iy[gb[p]] : -1;
            ga[p] = a >= 0 && a < nx ? a : nx;
            gb[p] = b >= 0 && b < ny ? b : ny;
        }
    }
    auto fetch = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            ra[p] = load_row(X, ga[p], nx, k0);
            rb[p] = load_row(Y, gb[p], ny, k0);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                As[buf][kq * 4 + e][rl + 64 * p] = ra[p][e];
                Bs[buf][kq * 4 + e][rl + 64 * p] = rb[p][e];
            }
    };
    const int nchunks = (D + EM_KC - 1) / EM_KC;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) fetch((c + 1) * EM_KC);         // next chunk's loads fly under this chunk's MFMAs
#pragma unroll
        for (int kk = 0; kk < EM_KC / 2; ++kk) {
            const int kr = kk * 2 + (lane >> 5), cl = lane & 31;
            float a[2], b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[u] = As[buf][kr][wi * 64 + u * 32 + cl];
                b[u] = Bs[buf][kr][wj * 64 + u * 32 + cl];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[v], acc[u][v], 0, 0, 0);
        }
        if (c + 1 < nchunks) stage(buf ^ 1);
        __syncthreads();
    }
}

// sorted list L[0..K1) of the K1 smallest values seen; insert v (branch-free min/max network, top down on the old values)
template <int K1>
__device__ __forceinline__ void em_insert(float (&L)[K1], float v) {
#pragma unroll
    for (int t = K1 - 1; t > 0; --t) L[t] = fminf(L[t], fmaxf(L[t - 1], v));
    L[0] = fminf(L[0], v);
}

// XCD-aware order: blocks b and b + 8 share an XCD under round-robin placement, so logical index
// (b % 8) * (nwg8 / 8) + b / 8 gives each XCD a contiguous run of the logical grid (speed only, never correctness)
__device__ __forceinline__ long em_xcd_logical(long nwg8) { return (long)(blockIdx.x % 8) * (nwg8 / 8) + blockIdx.x / 8; }

template <int K1>
__global__ __launch_bounds__(256) void knn_radii_kernel(const float* __restrict__ x, const float* __restrict__ nrm, float* __restrict__ part,
                                                       long N, int D, int RT, int CT, int S, int tiles_per_split, long nwg8) {
    __shared__ float smem[EM_DTILE_FLOATS > EM_STAGE_FLOATS ? EM_DTILE_FLOATS : EM_STAGE_FLOATS];
    const long logical = em_xcd_logical(nwg8);
    if (logical >= (long)RT * S) return;
    const int split = (int)(logical / RT), rt = (int)(logical % RT);     // consecutive logical blocks share the split's columns
    const int ct0 = split * tiles_per_split, ct1 = min(CT, ct0 + tiles_per_split);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = wave >> 1, wj = wave & 1;
    const long r0 = (long)rt * EM_T;
    float (*Dt)[EM_DLD] = reinterpret_cast<float (*)[EM_DLD]>(smem);
    // scanning thread: row (tid % 128) of the tile, columns (tid / 128) * 64 .. + 64 (one half per wave pair: conflict-free reads)
    const int srow = tid & (EM_T - 1), shalf = tid >> 7;
    float L[K1];
#pragma unroll
    for (int t = 0; t < K1; ++t) L[t] = __builtin_inff();
    float rn[2][4][4];                                   // row norms of this lane's accumulator rows
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long i = r0 + wi * 64 + u * 32 + (lane >> 5) * 4 + q * 8 + e;
                rn[u][q][e] = i < N ? nrm[i] : 0.f;
            }
    for (int ct = ct0; ct < ct1; ++ct) {
        const long c0 = (long)ct * EM_T;
        f32x16 acc[2][2];
        em_dot_tile(x, N, x, N, D, r0, c0, smem, acc);
        // the staging buffers are dead after the K loop's last barrier: the distance tile reuses the LDS
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int j = wj * 64 + v * 32 + (lane & 31);
            const float cn = c0 + j < N ? nrm[c0 + j] : 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = wi * 64 + u * 32 + (lane >> 5) * 4 + q * 8 + e;
                        Dt[i][j] = em_pair_dist(rn[u][q][e], cn, acc[u][v][q * 4 + e]);
                    }
        }
        __syncthreads();
        const long cend = N - c0 < EM_T ? N - c0 : EM_T;           // valid columns of this tile
        const int jb = shalf * 64;
        const int je = (int)(cend < jb + 64 ? cend : jb + 64);
        for (int j = jb; j < je; ++j) em_insert<K1>(L, Dt[srow][j]);
        __syncthreads();                                             // the next tile's staging overwrites Dt
    }
    const long row = r0 + srow;
    if (row < N) {
        float* dst = part + ((long)(split * 2 + shalf) * N + row) * K1;
#pragma unroll
        for (int t = 0; t < K1; ++t) dst[t] = L[t];
    }
}

template <int K1>
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ part, float* __restrict__ radii, long N, int P) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    float L[K1];
#pragma unroll
    for (int t = 0; t < K1; ++t) L[t] = __builtin_inff();
    for (int p = 0; p < P; ++p) {
        const float* src = part + ((long)p * N + row) * K1;
#pragma unroll
        for (int t = 0; t < K1; ++t) em_insert<K1>(L, src[t]);
    }
    radii[row] = L[K1 - 1];
}

__global__ __launch_bounds__(256) void flags_clear_kernel(int32_t* __restrict__ a, long na, int32_t* __restrict__ b, long nb) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < na) a[t] = 0;
    else if (t < na + nb) b[t - na] = 0;
}

__global__ __launch_bounds__(256) void pr_member_kernel(const float* __restrict__ A, const float* __restrict__ nA, const float* __restrict__ rA,
                                                       long NA, const float* __restrict__ B, const float* __restrict__ nB,
                                                       const float* __restrict__ rB, long NB, int D, int RT, int CT, long nwg8,
                                                       int32_t* __restrict__ a_in_b, int32_t* __restrict__ b_in_a) {
    __shared__ float smem[EM_STAGE_FLOATS];
    const long logical = em_xcd_logical(nwg8);
    if (logical >= (long)RT * CT) return;
    const int ct = (int)(logical / RT), rt = (int)(logical % RT);       // an XCD's blocks share B's column tile
    const long r0 = (long)rt * EM_T, c0 = (long)ct * EM_T;
    f32x16 acc[2][2];
    em_dot_tile(A, NA, B, NB, D, r0, c0, smem, acc);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wi = wave >> 1, wj = wave & 1;
    bool rowin[2][4][4];
    float rn[2][4][4], rr[2][4][4];                      // norms and radii of this lane's accumulator rows (rr < 0: past NA)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long i = r0 + wi * 64 + u * 32 + (lane >> 5) * 4 + q * 8 + e;
                rowin[u][q][e] = false;
                rn[u][q][e] = i < NA ? nA[i] : 0.f;
                rr[u][q][e] = i < NA ? rA[i] : -1.f;
            }
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const long j = c0 + wj * 64 + v * 32 + (lane & 31);
        const bool jv = j < NB;
        const float cn = jv ? nB[j] : 0.f, cr = jv ? rB[j] : -1.f;
        bool colin = false;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // d >= 0 > the -1 radius sentinels; the stores below also check the bounds
                    const float d = em_pair_dist(rn[u][q][e], cn, acc[u][v][q * 4 + e]);
                    colin |= d <= rr[u][q][e];               // b_j inside a_i's sphere: precision
                    rowin[u][q][e] |= d <= cr;               // a_i inside b_j's sphere: recall
                }
        if (colin && jv) b_in_a[j] = 1;
    }
    // row flags: lanes 0-31 hold row 8q + e of the sub-tile, lanes 32-63 row 4 + 8q + e
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint64_t m = __ballot(rowin[u][q][e]);
                const long i = r0 + wi * 64 + u * 32 + (lane >> 5) * 4 + q * 8 + e;
                const bool mine = (lane & 31) == 0 && ((lane >> 5) ? (m >> 32) != 0 : (m & 0xffffffffull) != 0);
                if (mine && i < NA) a_in_b[i] = 1;
            }
}

__global__ __launch_bounds__(256) void is_logits_kernel(const float* __restrict__ X, long n, const float* __restrict__ W, int C, int D,
                                                       float* __restrict__ logits) {
    __shared__ float smem[EM_STAGE_FLOATS];
    const int ctiles = (C + EM_T - 1) / EM_T;
    const long r0 = (long)(blockIdx.x / ctiles) * EM_T, c0 = (long)(blockIdx.x % ctiles) * EM_T;
    f32x16 acc[2][2];
    em_dot_tile(X, n, W, C, D, r0, c0, smem, acc);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wi = wave >> 1, wj = wave & 1;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long i = r0 + wi * 64 + u * 32 + (lane >> 5) * 4 + q * 8 + e, j = c0 + wj * 64 + v * 32 + (lane & 31);
                    if (i < n && j < C) logits[i * C + j] = acc[u][v][q * 4 + e];
                }
}

__global__ __launch_bounds__(256) void is_softmax_kernel(float* __restrict__ p, long n, int C) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    float* row = p + r * C;
    float m = -__builtin_inff();
    for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(row[c] - m);
    s = wave_sum(s);
    const float inv = 1.f / s;
    for (int c = lane; c < C; c += 64) row[c] = expf(row[c] - m) * inv;
}

__global__ __launch_bounds__(256) void is_marginal_kernel(const float* __restrict__ p, long n, int C, double* __restrict__ logpbar) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (long r = 0; r < n; ++r) s += (double)p[r * C + c];
    logpbar[c] = log(s / (double)n);
}

__device__ __forceinline__ double em_wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void is_kl_kernel(const float* __restrict__ p, long n, int C, const double* __restrict__ logpbar,
                                                   double* __restrict__ kl) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    const float* row = p + r * C;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double v = (double)row[c];
        if (v > 0.0) s += v * (log(v) - logpbar[c]);            // p log p -> 0 as p -> 0
    }
    s = em_wave_sum_f64(s);
    if (lane == 0) kl[r] = s;
}

__global__ __launch_bounds__(256) void is_split_mean_kernel(const double* __restrict__ kl, long n, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (long r = threadIdx.x; r < n; r += 256) s += kl[r];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0] / (double)n;
}

// Tiles of one KID subset, in the order of their partials: the X.X tiles with column tile >= row tile (row-major over the upper
// triangle), the Y.Y tiles likewise, then every X.Y tile.  A function of (mx, my) alone.
struct KidPlan {
    int Tx, Ty;
    long nxx, nyy, P;
};

KidPlan kid_plan(long mx, long my) {
    KidPlan p;
    p.Tx = (int)((mx + EM_T - 1) / EM_T);
    p.Ty = (int)((my + EM_T - 1) / EM_T);
    p.nxx = (long)p.Tx * (p.Tx + 1) / 2;
    p.nyy = (long)p.Ty * (p.Ty + 1) / 2;
    p.P = p.nxx + p.nyy + (long)p.Tx * p.Ty;
    return p;
}

// One 128 x 128 tile of one subset's X.X, Y.Y or X.Y dots -> one fp64 partial sum of k = ((double)dot * gamma + coef0)^3 over the
// tile's valid pairs (i != j on a diagonal tile; a strictly upper tile of a symmetric product counts twice: the dot is bitwise
// symmetric).  Order: each lane adds its 64 pairs in register order, a wave's lanes through the xor shuffle tree, the four waves
// in wave order.
template <bool GATHER>
__global__ __launch_bounds__(256) void kid_tile_kernel(const float* __restrict__ X, long NX, const float* __restrict__ Y, long NY, int D,
                                                      const int32_t* __restrict__ idx_x, const int32_t* __restrict__ idx_y, long mx, long my,
                                                      KidPlan p, long nblocks, long nwg8, double gamma, double coef0,
                                                      double* __restrict__ part) {
    __shared__ float smem[EM_STAGE_FLOATS];
    __shared__ double red[4];
    const long logical = em_xcd_logical(nwg8);
    if (logical >= nblocks) return;
    const long s = logical / p.P, t = logical % p.P;
    int rt, ct;
    const bool sym = t < p.nxx + p.nyy, ofy = t >= p.nxx;       // ofy: the row set is Y (only with sym)
    if (sym) {
        const int T = ofy ? p.Ty : p.Tx;
        long rem = ofy ? t - p.nxx : t;
        rt = 0;
        while (rem >= T - rt) { rem -= T - rt; ++rt; }
        ct = rt + (int)rem;
    } else {
        const long rem = t - p.nxx - p.nyy;
        rt = (int)(rem / p.Ty);
        ct = (int)(rem % p.Ty);
    }
    const bool rowy = sym && ofy, colx = sym && !ofy;
    const float* R = rowy ? Y : X;
    const float* C = colx ? X : Y;
    const long nR = rowy ? NY : NX, nC = colx ? NX : NY, mR = rowy ? my : mx, mC = colx ? mx : my;
    const int32_t* iR = nullptr;
    const int32_t* iC = nullptr;
    if constexpr (GATHER) {
        iR = rowy ? idx_y + s * my : idx_x + s * mx;
        iC = colx ? idx_x + s * mx : idx_y + s * my;
    }
    const long r0 = (long)rt * EM_T, c0 = (long)ct * EM_T;
    f32x16 acc[2][2];
    em_dot_tile<GATHER>(R, nR, C, nC, D, r0, c0, smem, acc, iR, mR, iC, mC);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wi = wave >> 1, wj = wave & 1;
    const bool diag = sym && rt == ct;
    double sum = 0.0;
    {
#pragma clang fp contract(off)                                   // t and its cube round as the definition states them: no fma
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const long i = r0 + wi * 64 + u * 32 + (lane >> 5) * 4 + q * 8 + e, j = c0 + wj * 64 + v * 32 + (lane & 31);
                        const double tt = (double)acc[u][v][q * 4 + e] * gamma + coef0;
                        const double k3 = (tt * tt) * tt;
                        const bool in = i < mR && j < mC && !(diag && i == j);
                        sum += in ? k3 : 0.0;
                    }
    }
    sum = em_wave_sum_f64(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tot = ((red[0] + red[1]) + red[2]) + red[3];
        part[s * p.P + t] = sym && ct > rt ? 2.0 * tot : tot;
    }
}

// Per subset: Sxx, Syy, Sxy = the subset's partials of each kind added in a fixed order (thread-strided, then an LDS tree).  A
// subset with an index outside [0, NX) / [0, NY) gets three NaNs (the tile kernel read zeros in that row's place).
__global__ __launch_bounds__(256) void kid_reduce_kernel(const double* __restrict__ part, KidPlan p, const int32_t* __restrict__ idx_x,
                                                        const int32_t* __restrict__ idx_y, long mx, long my, long NX, long NY,
                                                        double* __restrict__ sums) {
    __shared__ double red[256];
    __shared__ int bad;
    const long s = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    __syncthreads();
    if (idx_x) {
        bool b = false;
        for (long i = tid; i < mx; i += 256) { const long g = idx_x[s * mx + i]; b |= g < 0 || g >= NX; }
        for (long i = tid; i < my; i += 256) { const long g = idx_y[s * my + i]; b |= g < 0 || g >= NY; }
        if (b) bad = 1;
    }
    const long lo[4] = {0, p.nxx, p.nxx + p.nyy, p.P};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a = 0.0;
        for (long t = lo[c] + tid; t < lo[c + 1]; t += 256) a += part[s * p.P + t];
        red[tid] = a;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) sums[s * 3 + c] = bad ? __builtin_nan("") : red[0];
        __syncthreads();
    }
}

// Ball counts, on knn_radii_kernel's grid: (row tile of A) x (a contiguous range of B's column tiles, one split).  Each lane keeps
// the count of its 32 accumulator rows over its half-wave's columns (a ballot and a popcount per row, as pr_member_kernel forms
// its row flags); the two waves of a row band meet in LDS at the end.  part[split][i] = #{ j in the split : d(a_i, b_j) < rA[i] }.
__global__ __launch_bounds__(256) void dc_count_kernel(const float* __restrict__ A, const float* __restrict__ nA, const float* __restrict__ rA,
                                                      long NA, const float* __restrict__ B, const float* __restrict__ nB, long NB, int D,
                                                      int RT, int CT, int S, int tiles_per_split, long nwg8, int32_t* __restrict__ part) {
    __shared__ float smem[EM_STAGE_FLOATS];
    const long logical = em_xcd_logical(nwg8);
    if (logical >= (long)RT * S) return;
    const int split = (int)(logical / RT), rt = (int)(logical % RT);
    const int ct0 = split * tiles_per_split, ct1 = min(CT, ct0 + tiles_per_split);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = wave >> 1, wj = wave & 1;
    const long r0 = (long)rt * EM_T;
    float rn[2][4][4], rr[2][4][4];                      // norms and radii of this lane's accumulator rows (rr < 0: past NA)
    // a ballot gives every lane of a half-wave the same count: lane (lane % 32) == 16 u + 4 q + e keeps that row's, one register
    const int slot = lane & 31;
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long i = r0 + wi * 64 + u * 32 + (lane >> 5) * 4 + q * 8 + e;
                rn[u][q][e] = i < NA ? nA[i] : 0.f;
                rr[u][q][e] = i < NA ? rA[i] : -1.f;
            }
    for (int ct = ct0; ct < ct1; ++ct) {
        const long c0 = (long)ct * EM_T;
        f32x16 acc[2][2];
        em_dot_tile(A, NA, B, NB, D, r0, c0, smem, acc);
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const long j = c0 + wj * 64 + v * 32 + (lane & 31);
            const bool jv = j < NB;
            const float cn = jv ? nB[j] : 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // strict: a pair at distance exactly r is outside (prdc's comparison); d >= 0 > the -1 sentinel
                        const uint64_t m = __ballot(jv && em_pair_dist(rn[u][q][e], cn, acc[u][v][q * 4 + e]) < rr[u][q][e]);
                        const int c = (lane >> 5) ? __popc((uint32_t)(m >> 32)) : __popc((uint32_t)m);
                        cnt += slot == u * 16 + q * 4 + e ? c : 0;
                    }
        }
    }
    // the staging buffers are dead after the K loop's last barrier: [2][128] counts, one column half per wave of a row band
    int* cs = reinterpret_cast<int*>(smem);
    cs[wj * EM_T + wi * 64 + (slot >> 4) * 32 + (lane >> 5) * 4 + ((slot >> 2) & 3) * 8 + (slot & 3)] = cnt;
    __syncthreads();
    if (tid < EM_T && r0 + tid < NA) part[(long)split * NA + r0 + tid] = cs[tid] + cs[EM_T + tid];
}

__global__ __launch_bounds__(256) void dc_merge_kernel(const int32_t* __restrict__ part, int32_t* __restrict__ counts, long NA, int S) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= NA) return;
    int c = 0;
    for (int s = 0; s < S; ++s) c += part[(long)s * NA + row];
    counts[row] = c;
}

struct DcPlan {
    int RT, CT, S, tps;
    size_t off_nb, off_part, total;
};

DcPlan dc_plan(long NA, long NB, int splits) {
    DcPlan p;
    p.RT = (int)((NA + EM_T - 1) / EM_T);
    p.CT = (int)((NB + EM_T - 1) / EM_T);
    int S = splits > 0 ? splits : (4096 + p.RT - 1) / p.RT;     // as radii_plan: ~4096 workgroups
    if (S > p.CT) S = p.CT;
    if (S < 1) S = 1;
    p.tps = (p.CT + S - 1) / S;
    p.S = (p.CT + p.tps - 1) / p.tps;
    p.off_nb = ((size_t)NA * 4 + 255) / 256 * 256;             // row norms of A, then of B, then the per-split counts
    p.off_part = p.off_nb + ((size_t)NB * 4 + 255) / 256 * 256;
    p.total = p.off_part + (size_t)p.S * NA * 4;
    return p;
}

struct RadiiPlan {
    int RT, CT, S, tps;
    size_t off_part, total;
};

RadiiPlan radii_plan(long N, int k, int splits) {
    RadiiPlan p;
    p.RT = (int)((N + EM_T - 1) / EM_T);
    p.CT = p.RT;
    int S = splits > 0 ? splits : (4096 + p.RT - 1) / p.RT;     // ~4096 workgroups: >= 8 rounds of 2 per CU on 256 CUs
    if (S > p.CT) S = p.CT;
    if (S < 1) S = 1;
    p.tps = (p.CT + S - 1) / S;
    p.S = (p.CT + p.tps - 1) / p.tps;
    p.off_part = ((size_t)N * 4 + 255) / 256 * 256;            // row norms first
    p.total = p.off_part + (size_t)2 * p.S * N * (k + 1) * 4;
    return p;
}

template <int K1>
int radii_launch(const float* x, const float* nrm, float* part, float* radii, long N, int D, const RadiiPlan& p, hipStream_t st) {
    const long nwg = (long)p.RT * p.S, nwg8 = (nwg + 7) / 8 * 8;
    hipLaunchKernelGGL(knn_radii_kernel<K1>, dim3((unsigned)nwg8), dim3(256), 0, st, x, nrm, part, N, D, p.RT, p.CT, p.S, p.tps, nwg8);
    DXMI_CHECK_LAUNCH("dxmi_knn_radii(tiles)");
    hipLaunchKernelGGL(knn_merge_kernel<K1>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const float*)part, radii, N, 2 * p.S);
    DXMI_CHECK_LAUNCH("dxmi_knn_radii(merge)");
    return DXMI_OK;
}

size_t is_split_rows(long N, int split) { return (size_t)(split < N ? split : N); }

}  // namespace

extern "C" int64_t dxmi_knn_radii_workspace_bytes(int64_t N, int32_t D, int32_t k, int32_t splits) {
    if (N < 2 || D <= 0 || k < 1 || k > EM_KMAX || N < k + 1 || splits < 0) return 0;
    return (int64_t)radii_plan(N, k, splits).total;
}

extern "C" int dxmi_knn_radii(const float* x, int64_t N, int32_t D, int32_t k, int32_t splits, float* radii, void* workspace, void* stream) {
    DXMI_CHECK_ARG(x && radii && workspace, "dxmi_knn_radii: null pointer");
    DXMI_CHECK_ARG(k >= 1 && k <= EM_KMAX, "dxmi_knn_radii: k %d out of range [1, %d]", k, EM_KMAX);
    DXMI_CHECK_ARG(N >= k + 1 && N <= (int64_t)1 << 30, "dxmi_knn_radii: need k + 1 <= N <= 2^30 rows (N %lld, k %d)", (long long)N, k);
    DXMI_CHECK_ARG(D > 0 && D <= 65536, "dxmi_knn_radii: need 0 < D <= 65536 (D %d)", D);
    DXMI_CHECK_ARG(splits >= 0, "dxmi_knn_radii: splits %d must be >= 0 (0: automatic)", splits);
    const RadiiPlan p = radii_plan(N, k, splits);
    char* ws = reinterpret_cast<char*>(workspace);
    float* nrm = reinterpret_cast<float*>(ws);
    float* part = reinterpret_cast<float*>(ws + p.off_part);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, x, nrm, (long)N, D);
    DXMI_CHECK_LAUNCH("dxmi_knn_radii(norms)");
    switch (k + 1) {
        case 2: return radii_launch<2>(x, nrm, part, radii, N, D, p, st);
        case 3: return radii_launch<3>(x, nrm, part, radii, N, D, p, st);
        case 4: return radii_launch<4>(x, nrm, part, radii, N, D, p, st);
        case 5: return radii_launch<5>(x, nrm, part, radii, N, D, p, st);
        case 6: return radii_launch<6>(x, nrm, part, radii, N, D, p, st);
        case 7: return radii_launch<7>(x, nrm, part, radii, N, D, p, st);
        default: return radii_launch<8>(x, nrm, part, radii, N, D, p, st);
    }
}

extern "C" int64_t dxmi_pr_membership_workspace_bytes(int64_t NA, int64_t NB) {
    if (NA < 1 || NB < 1) return 0;
    return (int64_t)((((size_t)NA * 4 + 255) / 256 * 256) + (size_t)NB * 4);
}

extern "C" int dxmi_pr_membership(const float* A, int64_t NA, const float* rA, const float* B, int64_t NB, const float* rB, int32_t D,
                                  int32_t* a_in_b, int32_t* b_in_a, void* workspace, void* stream) {
    DXMI_CHECK_ARG(A && rA && B && rB && a_in_b && b_in_a && workspace, "dxmi_pr_membership: null pointer");
    DXMI_CHECK_ARG(NA >= 1 && NB >= 1 && NA <= (int64_t)1 << 30 && NB <= (int64_t)1 << 30,
                   "dxmi_pr_membership: need 1 <= NA, NB <= 2^30 (NA %lld, NB %lld)", (long long)NA, (long long)NB);
    DXMI_CHECK_ARG(D > 0 && D <= 65536, "dxmi_pr_membership: need 0 < D <= 65536 (D %d)", D);
    char* ws = reinterpret_cast<char*>(workspace);
    float* nA = reinterpret_cast<float*>(ws);
    float* nB = reinterpret_cast<float*>(ws + ((size_t)NA * 4 + 255) / 256 * 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(flags_clear_kernel, dim3((unsigned)((NA + NB + 255) / 256)), dim3(256), 0, st, a_in_b, (long)NA, b_in_a, (long)NB);
    DXMI_CHECK_LAUNCH("dxmi_pr_membership(clear)");
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)((NA + 255) / 256)), dim3(256), 0, st, A, nA, (long)NA, D);
    DXMI_CHECK_LAUNCH("dxmi_pr_membership(norms A)");
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)((NB + 255) / 256)), dim3(256), 0, st, B, nB, (long)NB, D);
    DXMI_CHECK_LAUNCH("dxmi_pr_membership(norms B)");
    const int RT = (int)((NA + EM_T - 1) / EM_T), CT = (int)((NB + EM_T - 1) / EM_T);
    const long nwg = (long)RT * CT, nwg8 = (nwg + 7) / 8 * 8;
    DXMI_CHECK_ARG(nwg8 < ((long)1 << 31), "dxmi_pr_membership: %lld tiles exceed one launch", (long long)nwg8);
    hipLaunchKernelGGL(pr_member_kernel, dim3((unsigned)nwg8), dim3(256), 0, st, A, (const float*)nA, rA, (long)NA, B, (const float*)nB, rB,
                       (long)NB, D, RT, CT, nwg8, a_in_b, b_in_a);
    DXMI_CHECK_LAUNCH("dxmi_pr_membership(tiles)");
    return DXMI_OK;
}

extern "C" int64_t dxmi_kid_sums_workspace_bytes(int64_t S, int64_t mx, int64_t my, int32_t D) {
    if (S < 1 || S > (int64_t)1 << 30 || mx < 2 || my < 2 || mx > (int64_t)1 << 30 || my > (int64_t)1 << 30 || D <= 0) return 0;
    const long P = kid_plan(mx, my).P;
    if (P >= (((long)1 << 31) - 8) / S) return 0;                // more tiles than one launch takes: dxmi_kid_sums refuses it
    return (int64_t)((size_t)S * P * 8);
}

extern "C" int dxmi_kid_sums(const float* X, int64_t NX, const float* Y, int64_t NY, int32_t D, const int32_t* idx_x, const int32_t* idx_y,
                             int64_t S, int64_t mx, int64_t my, double gamma, double coef0, double* sums, void* workspace, void* stream) {
    DXMI_CHECK_ARG(X && Y && sums && workspace, "dxmi_kid_sums: null pointer");
    DXMI_CHECK_ARG(D > 0 && D <= 65536, "dxmi_kid_sums: need 0 < D <= 65536 (D %d)", D);
    DXMI_CHECK_ARG(NX >= 1 && NY >= 1 && NX <= (int64_t)1 << 30 && NY <= (int64_t)1 << 30,
                   "dxmi_kid_sums: need 1 <= NX, NY <= 2^30 (NX %lld, NY %lld)", (long long)NX, (long long)NY);
    DXMI_CHECK_ARG(mx >= 2 && my >= 2 && mx <= (int64_t)1 << 30 && my <= (int64_t)1 << 30,
                   "dxmi_kid_sums: need 2 <= mx, my <= 2^30 rows per subset (mx %lld, my %lld)", (long long)mx, (long long)my);
    DXMI_CHECK_ARG(S >= 1 && S <= (int64_t)1 << 30, "dxmi_kid_sums: need 1 <= S <= 2^30 subsets (S %lld)", (long long)S);
    DXMI_CHECK_ARG((idx_x == nullptr) == (idx_y == nullptr), "dxmi_kid_sums: idx_x and idx_y must both be given or both be null");
    if (!idx_x) {
        DXMI_CHECK_ARG(S == 1, "dxmi_kid_sums: null indices mean one subset of all rows (S %lld)", (long long)S);
        DXMI_CHECK_ARG(mx == NX && my == NY, "dxmi_kid_sums: null indices mean all rows: need mx == NX and my == NY (mx %lld, NX %lld, my %lld, NY %lld)",
                       (long long)mx, (long long)NX, (long long)my, (long long)NY);
    }
    const KidPlan p = kid_plan(mx, my);
    DXMI_CHECK_ARG(p.P < (((long)1 << 31) - 8) / S, "dxmi_kid_sums: %lld subsets of %lld tiles exceed one launch", (long long)S, (long long)p.P);
    const long nblocks = (long)S * p.P, nwg8 = (nblocks + 7) / 8 * 8;
    double* part = reinterpret_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (idx_x)
        hipLaunchKernelGGL(kid_tile_kernel<true>, dim3((unsigned)nwg8), dim3(256), 0, st, X, (long)NX, Y, (long)NY, D, idx_x, idx_y, (long)mx,
                           (long)my, p, nblocks, nwg8, gamma, coef0, part);
    else
        hipLaunchKernelGGL(kid_tile_kernel<false>, dim3((unsigned)nwg8), dim3(256), 0, st, X, (long)NX, Y, (long)NY, D, idx_x, idx_y, (long)mx,
                           (long)my, p, nblocks, nwg8, gamma, coef0, part);
    DXMI_CHECK_LAUNCH("dxmi_kid_sums(tiles)");
    hipLaunchKernelGGL(kid_reduce_kernel, dim3((unsigned)S), dim3(256), 0, st, (const double*)part, p, idx_x, idx_y, (long)mx, (long)my,
                       (long)NX, (long)NY, sums);
    DXMI_CHECK_LAUNCH("dxmi_kid_sums(reduce)");
    return DXMI_OK;
}

extern "C" int64_t dxmi_dc_counts_workspace_bytes(int64_t NA, int64_t NB, int32_t splits) {
    if (NA < 1 || NB < 1 || NA > (int64_t)1 << 30 || NB > (int64_t)1 << 30 || splits < 0) return 0;
    return (int64_t)dc_plan(NA, NB, splits).total;
}

extern "C" int dxmi_dc_counts(const float* A, int64_t NA, const float* rA, const float* B, int64_t NB, int32_t D, int32_t splits,
                              int32_t* counts, void* workspace, void* stream) {
    DXMI_CHECK_ARG(A && rA && B && counts && workspace, "dxmi_dc_counts: null pointer");
    DXMI_CHECK_ARG(NA >= 1 && NB >= 1 && NA <= (int64_t)1 << 30 && NB <= (int64_t)1 << 30,
                   "dxmi_dc_counts: need 1 <= NA, NB <= 2^30 (NA %lld, NB %lld)", (long long)NA, (long long)NB);
    DXMI_CHECK_ARG(D > 0 && D <= 65536, "dxmi_dc_counts: need 0 < D <= 65536 (D %d)", D);
    DXMI_CHECK_ARG(splits >= 0, "dxmi_dc_counts: splits %d must be >= 0 (0: automatic)", splits);
    const DcPlan p = dc_plan(NA, NB, splits);
    char* ws = reinterpret_cast<char*>(workspace);
    float* nA = reinterpret_cast<float*>(ws);
    float* nB = reinterpret_cast<float*>(ws + p.off_nb);
    int32_t* part = reinterpret_cast<int32_t*>(ws + p.off_part);
    hipStream_t st = (hipStream_t)stream;
    const long nwg = (long)p.RT * p.S, nwg8 = (nwg + 7) / 8 * 8;
    DXMI_CHECK_ARG(nwg8 < ((long)1 << 31), "dxmi_dc_counts: %lld workgroups exceed one launch", (long long)nwg8);
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)((NA + 255) / 256)), dim3(256), 0, st, A, nA, (long)NA, D);
    DXMI_CHECK_LAUNCH("dxmi_dc_counts(norms A)");
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)((NB + 255) / 256)), dim3(256), 0, st, B, nB, (long)NB, D);
    DXMI_CHECK_LAUNCH("dxmi_dc_counts(norms B)");
    hipLaunchKernelGGL(dc_count_kernel, dim3((unsigned)nwg8), dim3(256), 0, st, A, (const float*)nA, rA, (long)NA, B, (const float*)nB, (long)NB,
                       D, p.RT, p.CT, p.S, p.tps, nwg8, part);
    DXMI_CHECK_LAUNCH("dxmi_dc_counts(tiles)");
    hipLaunchKernelGGL(dc_merge_kernel, dim3((unsigned)((NA + 255) / 256)), dim3(256), 0, st, (const int32_t*)part, counts, (long)NA, p.S);
    DXMI_CHECK_LAUNCH("dxmi_dc_counts(merge)");
    return DXMI_OK;
}

extern "C" int64_t dxmi_inception_score_workspace_bytes(int64_t N, int32_t C, int32_t split) {
    if (N < 1 || C < 1 || split < 1) return 0;
    const size_t n = is_split_rows(N, split);
    return (int64_t)((n * C * 4 + 255) / 256 * 256 + ((size_t)C * 8 + 255) / 256 * 256 + n * 8);
}

extern "C" int dxmi_inception_score(const float* pool, int64_t N, int32_t D, const float* w, int32_t C, int32_t split, double* kl_mean,
                                    void* workspace, void* stream) {
    DXMI_CHECK_ARG(pool && w && kl_mean && workspace, "dxmi_inception_score: null pointer");
    DXMI_CHECK_ARG(N >= 1 && N <= (int64_t)1 << 30, "dxmi_inception_score: need 1 <= N <= 2^30 (N %lld)", (long long)N);
    DXMI_CHECK_ARG(D > 0 && D <= 65536 && C > 0 && C <= 65536, "dxmi_inception_score: need 0 < D, C <= 65536 (D %d, C %d)", D, C);
    DXMI_CHECK_ARG(split >= 1, "dxmi_inception_score: split size %d must be >= 1", split);
    const size_t nmax = is_split_rows(N, split);
    char* ws = reinterpret_cast<char*>(workspace);
    float* prob = reinterpret_cast<float*>(ws);
    double* logpbar = reinterpret_cast<double*>(ws + (nmax * C * 4 + 255) / 256 * 256);
    double* kl = reinterpret_cast<double*>(ws + (nmax * C * 4 + 255) / 256 * 256 + ((size_t)C * 8 + 255) / 256 * 256);
    hipStream_t st = (hipStream_t)stream;
    const int ctiles = (C + EM_T - 1) / EM_T;
    for (int64_t s0 = 0, s = 0; s0 < N; s0 += split, ++s) {
        const long n = (long)(N - s0 < split ? N - s0 : split);
        const float* x = pool + s0 * D;
        hipLaunchKernelGGL(is_logits_kernel, dim3((unsigned)(((n + EM_T - 1) / EM_T) * ctiles)), dim3(256), 0, st, x, n, w, C, D, prob);
        DXMI_CHECK_LAUNCH("dxmi_inception_score(logits)");
        hipLaunchKernelGGL(is_softmax_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, prob, n, C);
        DXMI_CHECK_LAUNCH("dxmi_inception_score(softmax)");
        hipLaunchKernelGGL(is_marginal_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, (const float*)prob, n, C, logpbar);
        DXMI_CHECK_LAUNCH("dxmi_inception_score(marginal)");
        hipLaunchKernelGGL(is_kl_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const float*)prob, n, C, (const double*)logpbar, kl);
        DXMI_CHECK_LAUNCH("dxmi_inception_score(kl)");
        hipLaunchKernelGGL(is_split_mean_kernel, dim3(1), dim3(256), 0, st, (const double*)kl, n, kl_mean + s);
        DXMI_CHECK_LAUNCH("dxmi_inception_score(split mean)");
    }
    return DXMI_OK;
}
