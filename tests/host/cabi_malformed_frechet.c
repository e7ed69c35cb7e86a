/* Host-side robustness driver for the fp64 matrix entry points of csrc/frechet.hip (dxmi_gemm_f64, dxmi_frob_norm_f64,
 * dxmi_scale_f64, dxmi_symmetrize_f64, dxmi_frechet_workspace_bytes), the stand-alone twin of cabi_malformed.c for these calls.
 * Built by `make -C diffusion-by-maxentirl_amd/csrc asan_frechet` against the HOST-ONLY AddressSanitizer + UBSan build of the
 * library's sources (no device code: hipcc --offload-host-only; never run on a GPU machine) and executed as a child process by
 * tests/test_frechet_host.py.  Every call hands an entry point a malformed argument set (null pointers, n % 16 != 0, n <= 0,
 * n > 4096, aliased or misaligned matrices): the contract (include/dxmi_hip.h, "Conventions") is DXMI_EINVAL + dxmi_last_error()
 * text, no crash, no sanitizer report.  Device pointers are fake non-null addresses: the host side must never dereference them.
 * Output: one line per case "ok <name> <status>" or "FAIL <name> <status>", exit code = number of failures. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dxmi_hip.h"

static int failures = 0;
#define FAKE(n) ((double*)(uintptr_t)(0x10000000ull * (n)))          /* 256 MiB apart: no two 4096 x 4096 matrices overlap */
#define OFF(p, bytes) ((double*)((uintptr_t)(p) + (bytes)))

static void expect_einval(const char* name, int status, const char* needle) {
    const char* msg = dxmi_last_error();
    if (status == DXMI_EINVAL && msg && strstr(msg, needle)) printf("ok   %-44s %d  (%s)\n", name, status, msg);
    else { printf("FAIL %-44s %d  (%s), expected \"%s\"\n", name, status, msg ? msg : "(null)", needle); ++failures; }
}
static void expect_negative(const char* name, int status) {   /* valid arguments, no device: launch / device error, still no crash */
    if (status < 0) printf("ok   %-44s %d\n", name, status);
    else { printf("FAIL %-44s %d\n", name, status); ++failures; }
}
static void expect_true(const char* name, int cond) {
    if (cond) printf("ok   %-44s\n", name);
    else { printf("FAIL %-44s\n", name); ++failures; }
}

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    double *A = FAKE(1), *B = FAKE(2), *C = FAKE(3), *T = FAKE(4), *W = FAKE(5);
    static const int32_t bad_n[] = {0, -16, -1, 8, 15, 17, 24, 100, 2047, 4097, 4112, 8192, INT32_MAX, INT32_MIN};
    char name[96];
    /* ---- dxmi_gemm_f64 ------------------------------------------------------------------------------------------- */
    expect_einval("gemm_f64(A NULL)", dxmi_gemm_f64(NULL, B, C, 64, 1.0, 0.0, T, NULL), "null pointer");
    expect_einval("gemm_f64(B NULL)", dxmi_gemm_f64(A, NULL, C, 64, 1.0, 0.0, T, NULL), "null pointer");
    expect_einval("gemm_f64(C NULL)", dxmi_gemm_f64(A, B, NULL, 64, 1.0, 0.0, NULL, NULL), "null pointer");
    for (size_t i = 0; i < sizeof bad_n / sizeof bad_n[0]; ++i) {
        snprintf(name, sizeof name, "gemm_f64(n = %d)", (int)bad_n[i]);
        expect_einval(name, dxmi_gemm_f64(A, B, C, bad_n[i], 1.0, 0.0, NULL, NULL), "multiple of 16");
    }
    expect_einval("gemm_f64(C is A)", dxmi_gemm_f64(A, B, A, 64, 1.0, 0.0, NULL, NULL), "alias");
    expect_einval("gemm_f64(C is B)", dxmi_gemm_f64(A, B, B, 64, -0.5, 1.5, T, NULL), "alias");
    expect_einval("gemm_f64(C inside A)", dxmi_gemm_f64(A, B, OFF(A, 64 * 64 * 8 - 16), 64, 1.0, 0.0, NULL, NULL), "alias");
    expect_einval("gemm_f64(B's end inside C)", dxmi_gemm_f64(A, OFF(C, -16), C, 64, 1.0, 0.0, NULL, NULL), "alias");
    expect_einval("gemm_f64(C overlaps A at n = 4096)", dxmi_gemm_f64(A, B, OFF(A, 4096u * 4096u * 8u - 16u), 4096, 1.0, 0.0, NULL, NULL),
                  "alias");
    expect_einval("gemm_f64(A + 8 bytes)", dxmi_gemm_f64(OFF(A, 8), B, C, 64, 1.0, 0.0, NULL, NULL), "16-byte aligned");
    expect_einval("gemm_f64(B + 4 bytes)", dxmi_gemm_f64(A, OFF(B, 4), C, 64, 1.0, 0.0, NULL, NULL), "16-byte aligned");
    expect_einval("gemm_f64(C + 1 byte)", dxmi_gemm_f64(A, B, OFF(C, 1), 64, 1.0, 0.0, NULL, NULL), "16-byte aligned");
    expect_einval("gemm_f64(trace + 4 bytes)", dxmi_gemm_f64(A, B, C, 64, 1.0, 0.0, OFF(T, 4), NULL), "8-byte aligned");
    /* ---- dxmi_frob_norm_f64 -------------------------------------------------------------------------------------- */
    expect_einval("frob_norm_f64(X NULL)", dxmi_frob_norm_f64(NULL, 64, T, W, NULL), "null pointer");
    expect_einval("frob_norm_f64(out NULL)", dxmi_frob_norm_f64(A, 64, NULL, W, NULL), "null pointer");
    expect_einval("frob_norm_f64(workspace NULL)", dxmi_frob_norm_f64(A, 64, T, NULL, NULL), "null pointer");
    for (size_t i = 0; i < sizeof bad_n / sizeof bad_n[0]; ++i) {
        snprintf(name, sizeof name, "frob_norm_f64(n = %d)", (int)bad_n[i]);
        expect_einval(name, dxmi_frob_norm_f64(A, bad_n[i], T, W, NULL), "multiple of 16");
    }
    expect_einval("frob_norm_f64(X + 4 bytes)", dxmi_frob_norm_f64(OFF(A, 4), 64, T, W, NULL), "8-byte aligned");
    /* ---- dxmi_scale_f64 ------------------------------------------------------------------------------------------ */
    expect_einval("scale_f64(X NULL)", dxmi_scale_f64(NULL, B, 64, 2.0, NULL), "null pointer");
    expect_einval("scale_f64(Y NULL)", dxmi_scale_f64(A, NULL, 64, 2.0, NULL), "null pointer");
    for (size_t i = 0; i < sizeof bad_n / sizeof bad_n[0]; ++i) {
        snprintf(name, sizeof name, "scale_f64(n = %d)", (int)bad_n[i]);
        expect_einval(name, dxmi_scale_f64(A, B, bad_n[i], 2.0, NULL), "multiple of 16");
    }
    expect_einval("scale_f64(Y shifted into X)", dxmi_scale_f64(A, OFF(A, 64), 64, 2.0, NULL), "overlap");
    expect_einval("scale_f64(Y + 2 bytes)", dxmi_scale_f64(A, OFF(B, 2), 64, 2.0, NULL), "8-byte aligned");
    /* ---- dxmi_symmetrize_f64 ------------------------------------------------------------------------------------- */
    expect_einval("symmetrize_f64(X NULL)", dxmi_symmetrize_f64(NULL, 64, NULL), "null pointer");
    for (size_t i = 0; i < sizeof bad_n / sizeof bad_n[0]; ++i) {
        snprintf(name, sizeof name, "symmetrize_f64(n = %d)", (int)bad_n[i]);
        expect_einval(name, dxmi_symmetrize_f64(A, bad_n[i], NULL), "multiple of 16");
    }
    expect_einval("symmetrize_f64(X + 4 bytes)", dxmi_symmetrize_f64(OFF(A, 4), 64, NULL), "8-byte aligned");
    /* ---- workspace size: a host-side function --------------------------------------------------------------------- */
    expect_true("frechet_workspace_bytes(bad n) == 0", dxmi_frechet_workspace_bytes(0) == 0 && dxmi_frechet_workspace_bytes(-64) == 0 &&
                dxmi_frechet_workspace_bytes(24) == 0 && dxmi_frechet_workspace_bytes(4112) == 0 && dxmi_frechet_workspace_bytes(INT32_MIN) == 0);
    expect_true("frechet_workspace_bytes(good n) > 0", dxmi_frechet_workspace_bytes(16) > 0 && dxmi_frechet_workspace_bytes(2048) > 0 &&
                dxmi_frechet_workspace_bytes(4096) > 0);
    /* ---- valid argument sets reach the launch: no device here, so a negative status that is not a crash ------------ */
    expect_negative("gemm_f64(valid, n = 16, no device)", dxmi_gemm_f64(A, B, C, 16, 1.0, 0.0, NULL, NULL));
    expect_negative("gemm_f64(valid, A is B, trace, n = 4096)", dxmi_gemm_f64(A, A, C, 4096, -0.5, 1.5, T, NULL));
    expect_negative("frob_norm_f64(valid, no device)", dxmi_frob_norm_f64(A, 2048, T, W, NULL));
    expect_negative("scale_f64(valid in place, no device)", dxmi_scale_f64(A, A, 192, 0.5, NULL));
    expect_negative("symmetrize_f64(valid, no device)", dxmi_symmetrize_f64(A, 80, NULL));

    printf("%d failure(s)\n", failures);
    return failures > 99 ? 99 : failures;
}
