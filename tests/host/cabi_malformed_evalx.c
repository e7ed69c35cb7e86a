/* Host-side robustness driver for the KID and density / coverage entry points of csrc/eval_metrics.hip (dxmi_kid_sums,
 * dxmi_kid_sums_workspace_bytes, dxmi_dc_counts, dxmi_dc_counts_workspace_bytes), the stand-alone twin of cabi_malformed.c for
 * these calls.  Built by `make -C diffusion-by-maxentirl_amd/csrc asan_evalx` against the HOST-ONLY AddressSanitizer + UBSan build
 * of the library's sources (no device code: hipcc --offload-host-only; never run on a GPU machine) and executed as a child process
 * by tests/test_eval_kid_dc.py.  Every call hands an entry point a malformed argument set (null pointers, D <= 0, subsets of fewer
 * than two rows, S < 1, one index list without the other, null indices that do not mean "all rows", empty sets, negative splits,
 * sizes whose tile count overflows a launch): the contract (include/dxmi_hip.h, "Conventions") is DXMI_EINVAL + dxmi_last_error()
 * text, no crash, no sanitizer report, and 0 from the workspace functions.  Device pointers are fake non-null addresses: the host
 * side must never dereference them.
 * Output: one line per case "ok <name> <status>" or "FAIL <name> <status>", exit code = number of failures. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dxmi_hip.h"

static int failures = 0;
#define FAKE(T, n) ((T*)(uintptr_t)(0x10000000ull * (n)))

static void expect_einval(const char* name, int status, const char* needle) {
    const char* msg = dxmi_last_error();
    if (status == DXMI_EINVAL && msg && strstr(msg, needle)) printf("ok   %-52s %d  (%s)\n", name, status, msg);
    else { printf("FAIL %-52s %d  (%s), expected \"%s\"\n", name, status, msg ? msg : "(null)", needle); ++failures; }
}
static void expect_negative(const char* name, int status) {   /* valid arguments, no device: launch / device error, still no crash */
    if (status < 0) printf("ok   %-52s %d\n", name, status);
    else { printf("FAIL %-52s %d\n", name, status); ++failures; }
}
static void expect_true(const char* name, int cond) {
    if (cond) printf("ok   %-52s\n", name);
    else { printf("FAIL %-52s\n", name); ++failures; }
}

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    float *X = FAKE(float, 1), *Y = FAKE(float, 2), *R = FAKE(float, 3);
    int32_t *IX = FAKE(int32_t, 4), *IY = FAKE(int32_t, 5), *C = FAKE(int32_t, 6);
    double* SUMS = FAKE(double, 7);
    void* W = FAKE(void, 8);
    const int64_t BIG = (int64_t)1 << 30;
    char name[96];
    /* ---- dxmi_kid_sums ------------------------------------------------------------------------------------------- */
    expect_einval("kid_sums(X NULL)", dxmi_kid_sums(NULL, 300, Y, 257, 16, IX, IY, 3, 50, 50, 0.0625, 1.0, SUMS, W, NULL), "null pointer");
    expect_einval("kid_sums(Y NULL)", dxmi_kid_sums(X, 300, NULL, 257, 16, IX, IY, 3, 50, 50, 0.0625, 1.0, SUMS, W, NULL), "null pointer");
    expect_einval("kid_sums(sums NULL)", dxmi_kid_sums(X, 300, Y, 257, 16, IX, IY, 3, 50, 50, 0.0625, 1.0, NULL, W, NULL), "null pointer");
    expect_einval("kid_sums(workspace NULL)", dxmi_kid_sums(X, 300, Y, 257, 16, IX, IY, 3, 50, 50, 0.0625, 1.0, SUMS, NULL, NULL), "null pointer");
    static const int32_t bad_d[] = {0, -1, -2048, 65537, INT32_MAX, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_d / sizeof bad_d[0]; ++i) {
        snprintf(name, sizeof name, "kid_sums(D = %d)", (int)bad_d[i]);
        expect_einval(name, dxmi_kid_sums(X, 300, Y, 257, bad_d[i], IX, IY, 3, 50, 50, 0.0625, 1.0, SUMS, W, NULL), "0 < D");
    }
    static const int64_t bad_n[] = {0, -1, -300, ((int64_t)1 << 30) + 1, INT64_MAX, INT64_MIN};
    for (size_t i = 0; i < sizeof bad_n / sizeof bad_n[0]; ++i) {
        snprintf(name, sizeof name, "kid_sums(NX = %lld)", (long long)bad_n[i]);
        expect_einval(name, dxmi_kid_sums(X, bad_n[i], Y, 257, 16, IX, IY, 3, 50, 50, 0.0625, 1.0, SUMS, W, NULL), "NX, NY");
        snprintf(name, sizeof name, "kid_sums(NY = %lld)", (long long)bad_n[i]);
        expect_einval(name, dxmi_kid_sums(X, 300, Y, bad_n[i], 16, IX, IY, 3, 50, 50, 0.0625, 1.0, SUMS, W, NULL), "NX, NY");
    }
    static const int64_t bad_m[] = {1, 0, -1, -50, ((int64_t)1 << 30) + 1, INT64_MAX, INT64_MIN};
    for (size_t i = 0; i < sizeof bad_m / sizeof bad_m[0]; ++i) {
        snprintf(name, sizeof name, "kid_sums(mx = %lld)", (long long)bad_m[i]);
        expect_einval(name, dxmi_kid_sums(X, 300, Y, 257, 16, IX, IY, 3, bad_m[i], 50, 0.0625, 1.0, SUMS, W, NULL), "rows per subset");
        snprintf(name, sizeof name, "kid_sums(my = %lld)", (long long)bad_m[i]);
        expect_einval(name, dxmi_kid_sums(X, 300, Y, 257, 16, IX, IY, 3, 50, bad_m[i], 0.0625, 1.0, SUMS, W, NULL), "rows per subset");
    }
    static const int64_t bad_s[] = {0, -1, -100, ((int64_t)1 << 30) + 1, INT64_MAX, INT64_MIN};
    for (size_t i = 0; i < sizeof bad_s / sizeof bad_s[0]; ++i) {
        snprintf(name, sizeof name, "kid_sums(S = %lld)", (long long)bad_s[i]);
        expect_einval(name, dxmi_kid_sums(X, 300, Y, 257, 16, IX, IY, bad_s[i], 50, 50, 0.0625, 1.0, SUMS, W, NULL), "subsets");
    }
    expect_einval("kid_sums(idx_x NULL only)", dxmi_kid_sums(X, 300, Y, 257, 16, NULL, IY, 1, 300, 257, 0.0625, 1.0, SUMS, W, NULL), "both");
    expect_einval("kid_sums(idx_y NULL only)", dxmi_kid_sums(X, 300, Y, 257, 16, IX, NULL, 1, 300, 257, 0.0625, 1.0, SUMS, W, NULL), "both");
    expect_einval("kid_sums(null indices, S = 2)", dxmi_kid_sums(X, 300, Y, 257, 16, NULL, NULL, 2, 300, 257, 0.0625, 1.0, SUMS, W, NULL),
                  "one subset");
    expect_einval("kid_sums(null indices, mx < NX)", dxmi_kid_sums(X, 300, Y, 257, 16, NULL, NULL, 1, 299, 257, 0.0625, 1.0, SUMS, W, NULL),
                  "all rows");
    expect_einval("kid_sums(null indices, mx > NX)", dxmi_kid_sums(X, 300, Y, 257, 16, NULL, NULL, 1, 301, 257, 0.0625, 1.0, SUMS, W, NULL),
                  "all rows");
    expect_einval("kid_sums(null indices, my != NY)", dxmi_kid_sums(X, 300, Y, 257, 16, NULL, NULL, 1, 300, 2, 0.0625, 1.0, SUMS, W, NULL),
                  "all rows");
    /* tile counts past one launch: 2^30 rows are 2^23 tiles a side; 2^30 subsets of 1000 x 1000 are 2^30 * 164 tiles */
    expect_einval("kid_sums(all rows of 2^30 x 2^30)", dxmi_kid_sums(X, BIG, Y, BIG, 16, NULL, NULL, 1, BIG, BIG, 0.0625, 1.0, SUMS, W, NULL),
                  "exceed one launch");
    expect_einval("kid_sums(2^30 subsets of 1000)", dxmi_kid_sums(X, 5000, Y, 5000, 16, IX, IY, BIG, 1000, 1000, 0.0625, 1.0, SUMS, W, NULL),
                  "exceed one launch");
    expect_einval("kid_sums(2^30 subsets of 128)", dxmi_kid_sums(X, 5000, Y, 5000, 16, IX, IY, BIG, 128, 128, 0.0625, 1.0, SUMS, W, NULL), "exceed one launch");
    /* ---- dxmi_kid_sums_workspace_bytes ----------------------------------------------------------------------------- */
    expect_true("kid_sums_workspace_bytes(bad shapes) == 0",
                dxmi_kid_sums_workspace_bytes(0, 50, 50, 16) == 0 && dxmi_kid_sums_workspace_bytes(-1, 50, 50, 16) == 0 &&
                dxmi_kid_sums_workspace_bytes(3, 1, 50, 16) == 0 && dxmi_kid_sums_workspace_bytes(3, 50, 1, 16) == 0 &&
                dxmi_kid_sums_workspace_bytes(3, 50, -5, 16) == 0 && dxmi_kid_sums_workspace_bytes(3, 50, 50, 0) == 0 &&
                dxmi_kid_sums_workspace_bytes(3, 50, 50, -16) == 0 && dxmi_kid_sums_workspace_bytes(1, BIG, BIG, 16) == 0 &&
                dxmi_kid_sums_workspace_bytes(BIG, 1000, 1000, 16) == 0 && dxmi_kid_sums_workspace_bytes(INT64_MAX, 50, 50, 16) == 0 &&
                dxmi_kid_sums_workspace_bytes(3, INT64_MAX, 50, 16) == 0 && dxmi_kid_sums_workspace_bytes(INT64_MIN, INT64_MIN, INT64_MIN, 16) == 0);
    expect_true("kid_sums_workspace_bytes: one double per tile",
                dxmi_kid_sums_workspace_bytes(1, 2, 2, 16) == 3 * 8 && dxmi_kid_sums_workspace_bytes(7, 128, 129, 2048) == 7 * (1 + 3 + 2) * 8 &&
                dxmi_kid_sums_workspace_bytes(100, 1000, 1000, 2048) == 100 * (36 + 36 + 64) * 8 &&
                dxmi_kid_sums_workspace_bytes(1, 50000, 50000, 2048) == (int64_t)(2 * (391 * 392 / 2) + 391 * 391) * 8);
    /* ---- dxmi_dc_counts -------------------------------------------------------------------------------------------- */
    expect_einval("dc_counts(A NULL)", dxmi_dc_counts(NULL, 300, R, Y, 257, 16, 0, C, W, NULL), "null pointer");
    expect_einval("dc_counts(rA NULL)", dxmi_dc_counts(X, 300, NULL, Y, 257, 16, 0, C, W, NULL), "null pointer");
    expect_einval("dc_counts(B NULL)", dxmi_dc_counts(X, 300, R, NULL, 257, 16, 0, C, W, NULL), "null pointer");
    expect_einval("dc_counts(counts NULL)", dxmi_dc_counts(X, 300, R, Y, 257, 16, 0, NULL, W, NULL), "null pointer");
    expect_einval("dc_counts(workspace NULL)", dxmi_dc_counts(X, 300, R, Y, 257, 16, 0, C, NULL, NULL), "null pointer");
    for (size_t i = 0; i < sizeof bad_n / sizeof bad_n[0]; ++i) {
        snprintf(name, sizeof name, "dc_counts(NA = %lld)", (long long)bad_n[i]);
        expect_einval(name, dxmi_dc_counts(X, bad_n[i], R, Y, 257, 16, 0, C, W, NULL), "NA, NB");
        snprintf(name, sizeof name, "dc_counts(NB = %lld)", (long long)bad_n[i]);
        expect_einval(name, dxmi_dc_counts(X, 300, R, Y, bad_n[i], 16, 0, C, W, NULL), "NA, NB");
    }
    for (size_t i = 0; i < sizeof bad_d / sizeof bad_d[0]; ++i) {
        snprintf(name, sizeof name, "dc_counts(D = %d)", (int)bad_d[i]);
        expect_einval(name, dxmi_dc_counts(X, 300, R, Y, 257, bad_d[i], 0, C, W, NULL), "0 < D");
    }
    static const int32_t bad_splits[] = {-1, -8, INT32_MIN};
    for (size_t i = 0; i < sizeof bad_splits / sizeof bad_splits[0]; ++i) {
        snprintf(name, sizeof name, "dc_counts(splits = %d)", (int)bad_splits[i]);
        expect_einval(name, dxmi_dc_counts(X, 300, R, Y, 257, 16, bad_splits[i], C, W, NULL), "splits");
    }
    expect_einval("dc_counts(2^30 x 2^30, 2^23 splits)", dxmi_dc_counts(X, BIG, R, Y, BIG, 16, 1 << 23, C, W, NULL), "exceed one launch");
    /* ---- dxmi_dc_counts_workspace_bytes ---------------------------------------------------------------------------- */
    expect_true("dc_counts_workspace_bytes(bad shapes) == 0",
                dxmi_dc_counts_workspace_bytes(0, 257, 0) == 0 && dxmi_dc_counts_workspace_bytes(300, 0, 0) == 0 &&
                dxmi_dc_counts_workspace_bytes(-300, 257, 0) == 0 && dxmi_dc_counts_workspace_bytes(300, 257, -1) == 0 &&
                dxmi_dc_counts_workspace_bytes(INT64_MAX, 257, 0) == 0 && dxmi_dc_counts_workspace_bytes(300, INT64_MIN, 0) == 0 &&
                dxmi_dc_counts_workspace_bytes(300, 257, INT32_MIN) == 0);
    expect_true("dc_counts_workspace_bytes: norms + splits * NA counts",
                dxmi_dc_counts_workspace_bytes(300, 257, 1) == 1280 + 1280 + 1 * 300 * 4 &&
                dxmi_dc_counts_workspace_bytes(300, 257, 2) == 1280 + 1280 + 2 * 300 * 4 &&
                dxmi_dc_counts_workspace_bytes(300, 257, INT32_MAX) == 1280 + 1280 + 3 * 300 * 4 &&   /* at most one split per column tile */
                dxmi_dc_counts_workspace_bytes(10000, 50000, 0) < (int64_t)10000 * 4 * 400);
    /* ---- valid argument sets reach the launch: no device here, so a negative status that is not a crash ------------ */
    expect_negative("kid_sums(valid, 3 subsets of 50, no device)", dxmi_kid_sums(X, 300, Y, 257, 16, IX, IY, 3, 50, 50, 0.0625, 1.0, SUMS, W, NULL));
    expect_negative("kid_sums(valid, all rows, no device)", dxmi_kid_sums(X, 300, Y, 257, 2048, NULL, NULL, 1, 300, 257, 1.0 / 2048, 1.0, SUMS, W, NULL));
    expect_negative("kid_sums(valid, mx = my = 2, no device)", dxmi_kid_sums(X, 2, Y, 2, 1, NULL, NULL, 1, 2, 2, 1.0, 0.0, SUMS, W, NULL));
    expect_negative("kid_sums(valid, 50000 x 50000, no device)", dxmi_kid_sums(X, 50000, Y, 50000, 2048, NULL, NULL, 1, 50000, 50000, 1.0 / 2048, 1.0, SUMS, W, NULL));
    expect_negative("dc_counts(valid, no device)", dxmi_dc_counts(X, 300, R, Y, 257, 16, 0, C, W, NULL));
    expect_negative("dc_counts(valid, 7 splits, NA = NB = 1, no device)", dxmi_dc_counts(X, 1, R, Y, 1, 1, 7, C, W, NULL));
    expect_negative("dc_counts(valid, 10000 x 50000, no device)", dxmi_dc_counts(X, 10000, R, Y, 50000, 2048, 0, C, W, NULL));

    printf("%d failure(s)\n", failures);
    return failures > 99 ? 99 : failures;
}
