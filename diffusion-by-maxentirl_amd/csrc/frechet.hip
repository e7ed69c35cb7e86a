// fp64 matrix kernels of the Frechet distance on the device.
//
// Reference: pytorch_fid/fid_score.py:224-281 takes tr sqrtm(S1 S2) with scipy's Schur square root on the host (a 2048 x 2048
// float64 problem, seconds).  Here the trace comes from the coupled Newton-Schulz iteration on SYMMETRIC matrices only
// (dxmi_hip/ops.py frechet_trace_sqrt drives it): R = S1^(1/2), then tr (R S2 R)^(1/2).  Every step is
//     C = alpha * A * B + diag * I            (T = 1.5 I - 0.5 Z Y;  Y <- Y T;  Z <- T Z;  R S2;  (R S2) R)
// on v_mfma_f64_16x16x4_f64, plus a Frobenius norm, a scale and (X + X^T) / 2.
//
//   gemm_f64_kernel       128 x 128 tile of C per workgroup, 4 waves x (64 x 64) = 4 x 4 MFMA tiles, 128 accumulator registers;
//                         K chunks of 8 of A [128][8] and B [8][128] through LDS, two buffers, the next chunk's global loads in
//                         flight under this chunk's 32 MFMAs per wave.  Rows / columns beyond n are staged as zeros and never stored,
//                         K is never padded (n % 16 == 0): Inf and NaN flow through as arithmetic.
//   trace_f64_kernel      trace(C) from the stored diagonal, one workgroup, fixed order
//   frob_partial / fold   ||X||_F: 256 partial sums in a fixed order, folded by one workgroup
//   scale_f64_kernel      Y = alpha * X
//   symmetrize_f64_kernel X <- (X + X^T) / 2 in place, one thread per pair (i < j)
// No atomics: two calls give the same bits.
// Operand maps of v_mfma_f64_16x16x4_f64: A lane -> A[i = lane & 15][k = lane >> 4], B lane -> B[k = lane >> 4][j = lane & 15],
// C/D register r of a lane -> C[(lane >> 4) + 4 r][lane & 15]  (NOT the C/D map of the other types).
// Roofline: 2 n^3 FLOP on the fp64 matrix pipe; 16 KB of operands per workgroup and chunk, served by L2 at these sizes.
#include "common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int GT = 128;            // tile edge of C
constexpr int GK = 8;              // K per LDS chunk
constexpr int LDA_S = GK + 2;      // A tile row stride (doubles): 16 rows x 20 words land in 16 distinct bank pairs
constexpr int LDB_S = GT + 16;     // B tile row stride: the next k row is 32 banks on
constexpr int FROB_BLOCKS = 256;

__global__ __launch_bounds__(256) void gemm_f64_kernel(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C,
                                                      int n, double alpha, double diag) {
    __shared__ double As[2][GT][LDA_S];
    __shared__ double Bs[2][GK][LDB_S];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = wave >> 1, wj = wave & 1;
    const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
    // loaders: A row ar, 4 doubles from k offset ak; B row bk, 4 doubles from column bc (n % 16 == 0: a quad is all in or all out)
    const int ar = tid >> 1, ak = (tid & 1) * 4;
    const int bk = tid >> 5, bc = (tid & 31) * 4;
    const bool va = m0 + ar < n, vb = n0 + bc < n;
    const double* const ap = A + (size_t)(va ? m0 + ar : 0) * n + ak;
    const double* const bp = B + (size_t)bk * n + (vb ? n0 + bc : 0);
    f64x2 ra[2], rb[2];
    auto fetch = [&](int k0) {
        const f64x2 z = {0.0, 0.0};
        ra[0] = ra[1] = rb[0] = rb[1] = z;
        if (va) {
            ra[0] = *reinterpret_cast<const f64x2*>(ap + k0);
            ra[1] = *reinterpret_cast<const f64x2*>(ap + k0 + 2);
        }
        if (vb) {
            const double* p = bp + (size_t)k0 * n;
            rb[0] = *reinterpret_cast<const f64x2*>(p);
            rb[1] = *reinterpret_cast<const f64x2*>(p + 2);
        }
    };
    auto stage = [&](int buf) {
        *reinterpret_cast<f64x2*>(&As[buf][ar][ak]) = ra[0];
        *reinterpret_cast<f64x2*>(&As[buf][ar][ak + 2]) = ra[1];
        *reinterpret_cast<f64x2*>(&Bs[buf][bk][bc]) = rb[0];
        *reinterpret_cast<f64x2*>(&Bs[buf][bk][bc + 2]) = rb[1];
    };
    f64x4 acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[u][v][e] = 0.0;
    const int nchunks = n / GK;
    fetch(0);
    stage(0);
    __syncthreads();
    const int li = lane & 15, lk = lane >> 4;
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) fetch((c + 1) * GK);                   // next chunk's loads fly under this chunk's MFMAs
#pragma unroll
        for (int kk = 0; kk < GK / 4; ++kk) {
            const int k = kk * 4 + lk;
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = As[buf][wi * 64 + u * 16 + li][k];
                b[u] = Bs[buf][k][wj * 64 + u * 16 + li];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
        }
        if (c + 1 < nchunks) stage(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = m0 + wi * 64 + u * 16 + lk + 4 * r, j = n0 + wj * 64 + v * 16 + li;
                if (i < n && j < n) C[(size_t)i * n + j] = alpha * acc[u][v][r] + (i == j ? diag : 0.0);
            }
}

// sum of the 256 values of a workgroup, the same tree every time
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(256) void trace_f64_kernel(const double* __restrict__ X, int n, double* __restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += X[(size_t)i * n + i];
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) *out = s;
}

__global__ __launch_bounds__(256) void frob_partial_kernel(const double* __restrict__ X, long count, double* __restrict__ part) {
    __shared__ double sh[256];
    const long stride = (long)FROB_BLOCKS * 256;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;                  // four chains: loads in flight; fixed order -> reproducible
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < count; i += 4 * stride) {
        const double a = X[i], b = X[i + stride], c = X[i + 2 * stride], d = X[i + 3 * stride];
        s0 += a * a; s1 += b * b; s2 += c * c; s3 += d * d;
    }
    for (; i < count; i += stride) s0 += X[i] * X[i];
    const double s = block_sum_256((s0 + s1) + (s2 + s3), sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void frob_fold_kernel(const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sh[256];
    const double s = block_sum_256(part[threadIdx.x], sh);
    if (threadIdx.x == 0) *out = sqrt(s);
}

__global__ __launch_bounds__(256) void scale_f64_kernel(const double* X, double* Y, long count, double alpha) {      // Y may be X
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) Y[i] = alpha * X[i];
}

__global__ __launch_bounds__(256) void symmetrize_f64_kernel(double* __restrict__ X, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= n || j <= i) return;
    const double s = 0.5 * (X[(size_t)i * n + j] + X[(size_t)j * n + i]);
    X[(size_t)i * n + j] = s;
    X[(size_t)j * n + i] = s;
}

inline bool f64_n_ok(int32_t n) { return n >= 16 && n <= 4096 && n % 16 == 0; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool overlap(const void* a, const void* b, int32_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * (uintptr_t)n * 8u;
    return x < y + len && y < x + len;
}

}  // namespace

#define DXMI_CHECK_F64_N(name, n) \
    DXMI_CHECK_ARG(f64_n_ok(n), name ": n (%d) must be a multiple of 16 with 16 <= n <= 4096", (int)(n))

extern "C" int64_t dxmi_frechet_workspace_bytes(int32_t n) {
    if (!f64_n_ok(n)) return 0;
    return (int64_t)FROB_BLOCKS * 8;
}

extern "C" int dxmi_gemm_f64(const double* A, const double* B, double* C, int32_t n, double alpha, double diag, double* trace,
                             void* stream) {
    DXMI_CHECK_ARG(A && B && C, "dxmi_gemm_f64: null pointer");
    DXMI_CHECK_F64_N("dxmi_gemm_f64", n);
    DXMI_CHECK_ARG(aligned16(A) && aligned16(B) && aligned16(C), "dxmi_gemm_f64: A, B and C must be 16-byte aligned");
    DXMI_CHECK_ARG(!overlap(C, A, n) && !overlap(C, B, n), "dxmi_gemm_f64: C must not alias A or B");
    DXMI_CHECK_ARG(!trace || ((uintptr_t)trace & 7) == 0, "dxmi_gemm_f64: trace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nb = (n + GT - 1) / GT;
    hipLaunchKernelGGL(gemm_f64_kernel, dim3(nb, nb), dim3(256), 0, st, A, B, C, (int)n, alpha, diag);
    DXMI_CHECK_LAUNCH("dxmi_gemm_f64");
    if (trace) {
        hipLaunchKernelGGL(trace_f64_kernel, dim3(1), dim3(256), 0, st, (const double*)C, (int)n, trace);
        DXMI_CHECK_LAUNCH("dxmi_gemm_f64(trace)");
    }
    return DXMI_OK;
}

extern "C" int dxmi_frob_norm_f64(const double* X, int32_t n, double* out, void* workspace, void* stream) {
    DXMI_CHECK_ARG(X && out && workspace, "dxmi_frob_norm_f64: null pointer");
    DXMI_CHECK_F64_N("dxmi_frob_norm_f64", n);
    DXMI_CHECK_ARG(((uintptr_t)X & 7) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                   "dxmi_frob_norm_f64: X, out and workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(frob_partial_kernel, dim3(FROB_BLOCKS), dim3(256), 0, st, X, (long)n * n, part);
    DXMI_CHECK_LAUNCH("dxmi_frob_norm_f64(partials)");
    hipLaunchKernelGGL(frob_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)part, out);
    DXMI_CHECK_LAUNCH("dxmi_frob_norm_f64(fold)");
    return DXMI_OK;
}

extern "C" int dxmi_scale_f64(const double* X, double* Y, int32_t n, double alpha, void* stream) {
    DXMI_CHECK_ARG(X && Y, "dxmi_scale_f64: null pointer");
    DXMI_CHECK_F64_N("dxmi_scale_f64", n);
    DXMI_CHECK_ARG(((uintptr_t)X & 7) == 0 && ((uintptr_t)Y & 7) == 0, "dxmi_scale_f64: X and Y must be 8-byte aligned");
    DXMI_CHECK_ARG(X == Y || !overlap(X, Y, n), "dxmi_scale_f64: Y must be X itself or not overlap it");
    const long count = (long)n * n;
    hipLaunchKernelGGL(scale_f64_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, X, Y, count, alpha);
    DXMI_CHECK_LAUNCH("dxmi_scale_f64");
    return DXMI_OK;
}

extern "C" int dxmi_symmetrize_f64(double* X, int32_t n, void* stream) {
    DXMI_CHECK_ARG(X, "dxmi_symmetrize_f64: null pointer");
    DXMI_CHECK_F64_N("dxmi_symmetrize_f64", n);
    DXMI_CHECK_ARG(((uintptr_t)X & 7) == 0, "dxmi_symmetrize_f64: X must be 8-byte aligned");
    hipLaunchKernelGGL(symmetrize_f64_kernel, dim3((n + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, X, (int)n);
    DXMI_CHECK_LAUNCH("dxmi_symmetrize_f64");
    return DXMI_OK;
}
