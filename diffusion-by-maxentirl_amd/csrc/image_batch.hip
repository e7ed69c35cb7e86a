// Training batches from a uint8 image array: gather rows by index, mirror along W, normalise and go from NHWC uint8 to
// NCHW fp32 in ONE launch.  store uint8 [n_rows, H, W, C] (the `arr_0` layout of the evaluator's .npz batches and of make_npz.py),
// out fp32 [B, C, H, W].
//   image_batch_vec_kernel<C>  W % 16 == 0 and a 16-byte aligned store (H*W*C is then a multiple of 16 too): a lane owns 16
//                              consecutive pixels of one image row = C 16-byte loads of interleaved pixels, de-interleaved in
//                              registers (byte extracts with compile-time positions: no LDS, no scratch), and writes 4 f32x4 per
//                              channel plane.  A mirrored image writes the same 16 pixels to columns W - 16 - x0 .. W - 1 - x0 in
//                              reversed order: the flip is a store index and a per-element select, not a second pass.
//   image_batch_scalar_kernel  any other shape or alignment: one output element per lane.
// Both normalisations round once per operation (IEEE division, no contraction).  A row index outside [0, n_rows) writes NaN into
// that image and reads nothing.  No atomics, no reductions: bitwise reproducible.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLK = 256;

inline unsigned ib_grid(long total) {
    long g = (total + BLK - 1) / BLK;
    return (unsigned)(g > 65535L * 16 ? 65535L * 16 : (g < 1 ? 1 : g));
}

// image_datasets.py:118 `arr.astype(np.float32) / 127.5 - 1`; ToTensor's `.div(255)` then train_cifar10.py:170 `2 * images - 1`
__device__ __forceinline__ float ib_norm(uint32_t byte, int norm) {
    const float v = (float)byte;
    return norm == DXMI_IMG_NORM_ADM ? v / 127.5f - 1.0f : 2.0f * (v / 255.0f) - 1.0f;
}

template <int C>
__global__ __launch_bounds__(BLK) void image_batch_vec_kernel(const uint8_t* __restrict__ store, long n_rows, const int64_t* __restrict__ idx,
                                                              const uint8_t* __restrict__ flip, float* __restrict__ out, int B, int H, int W,
                                                              int norm) {
    const int gpr = W >> 4;                                  // 16-pixel groups per image row
    const long gpi = (long)H * gpr, total = (long)B * gpi;
    const float nan = __builtin_nanf("");
    for (long g = (long)blockIdx.x * BLK + threadIdx.x; g < total; g += (long)gridDim.x * BLK) {
        const int b = (int)(g / gpi);
        const long grp = g - (long)b * gpi;
        const int y = (int)(grp / gpr), x0 = (int)(grp - (long)y * gpr) << 4;
        const long s = idx ? idx[b] : (long)b;
        const bool ok = s >= 0 && s < n_rows;
        const bool f = flip && flip[b] != 0;
        uint32_t w[4 * C];
        if (ok) {
            const u32x4* __restrict__ sp = reinterpret_cast<const u32x4*>(store + ((size_t)s * gpi + grp) * (16 * C));
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const u32x4 q = sp[j];
                w[4 * j] = q[0]; w[4 * j + 1] = q[1]; w[4 * j + 2] = q[2]; w[4 * j + 3] = q[3];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4 * C; ++j) w[j] = 0u;
        }
        const int xo = f ? W - 16 - x0 : x0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float v[16];
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const int k = p * C + c;                     // byte of pixel p, channel c
                v[p] = ok ? ib_norm((w[k >> 2] >> (8 * (k & 3))) & 0xFFu, norm) : nan;
            }
            float* __restrict__ op = out + (((size_t)b * C + c) * H + y) * W + xo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = f ? v[15 - 4 * q - e] : v[4 * q + e];
                *reinterpret_cast<f32x4*>(op + 4 * q) = o;
            }
        }
    }
}

__global__ __launch_bounds__(BLK) void image_batch_scalar_kernel(const uint8_t* __restrict__ store, long n_rows, const int64_t* __restrict__ idx,
                                                                 const uint8_t* __restrict__ flip, float* __restrict__ out, int B, int H, int W,
                                                                 int C, int norm) {
    const long chw = (long)C * H * W, total = (long)B * chw;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < total; i += (long)gridDim.x * BLK) {
        const int b = (int)(i / chw);
        long r = i - (long)b * chw;
        const int x = (int)(r % W); r /= W;
        const int y = (int)(r % H), c = (int)(r / H);
        const long s = idx ? idx[b] : (long)b;
        const int xs = (flip && flip[b] != 0) ? W - 1 - x : x;
        float v = __builtin_nanf("");
        if (s >= 0 && s < n_rows) v = ib_norm(store[(((size_t)s * H + y) * W + xs) * C + c], norm);
        out[i] = v;
    }
}

}  // namespace

extern "C" int dxmi_image_batch(const void* store, int64_t n_rows, const int64_t* idx, const uint8_t* flip, float* out, int32_t B, int32_t H,
                                int32_t W, int32_t C, int32_t norm, void* stream) {
    DXMI_CHECK_ARG(store && out, "dxmi_image_batch: null pointer");
    DXMI_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384 && n_rows > 0,
                   "dxmi_image_batch: B (%d) and n_rows (%lld) must be positive and the image %dx%d in [1, 16384]", B, (long long)n_rows, H, W);
    DXMI_CHECK_ARG(C == 3 || C == 1, "dxmi_image_batch: C (%d) must be 3 or 1", C);
    DXMI_CHECK_ARG(norm == DXMI_IMG_NORM_ADM || norm == DXMI_IMG_NORM_TOTENSOR, "dxmi_image_batch: norm (%d) must be DXMI_IMG_NORM_ADM or "
                   "DXMI_IMG_NORM_TOTENSOR", norm);
    DXMI_CHECK_ARG(idx || (int64_t)B <= n_rows, "dxmi_image_batch: without idx the batch (%d) reads rows 0 .. B-1 of %lld", B, (long long)n_rows);
    const bool vec = W % 16 == 0 && ((((uintptr_t)store) | ((uintptr_t)out)) & 15) == 0;
    if (vec && C == 3)
        hipLaunchKernelGGL(image_batch_vec_kernel<3>, dim3(ib_grid((long)B * H * (W / 16))), dim3(BLK), 0, (hipStream_t)stream, (const uint8_t*)store,
                           (long)n_rows, idx, flip, out, B, H, W, norm);
    else if (vec)
        hipLaunchKernelGGL(image_batch_vec_kernel<1>, dim3(ib_grid((long)B * H * (W / 16))), dim3(BLK), 0, (hipStream_t)stream, (const uint8_t*)store,
                           (long)n_rows, idx, flip, out, B, H, W, norm);
    else
        hipLaunchKernelGGL(image_batch_scalar_kernel, dim3(ib_grid((long)B * C * H * W)), dim3(BLK), 0, (hipStream_t)stream, (const uint8_t*)store,
                           (long)n_rows, idx, flip, out, B, H, W, C, norm);
    DXMI_CHECK_LAUNCH("dxmi_image_batch");
    return DXMI_OK;
}
