/* Host-side robustness driver for dxmi_dpm_stage (csrc/dpm_sample.hip), the stand-alone twin of cabi_malformed.c for this one
 * entry point.  Built by `make -C diffusion-by-maxentirl_amd/csrc asan_dpm` against the HOST-ONLY AddressSanitizer + UBSan build
 * of the library's sources (no device code: hipcc --offload-host-only; never run on a GPU machine) and executed as a child process
 * by tests/test_dpm_sample_host.py.  Every call hands the entry point a malformed argument set (null pointers, misaligned
 * pointers, sizes and rows out of range): the contract (include/dxmi_hip.h, "Conventions") is DXMI_EINVAL + dxmi_last_error()
 * text, no crash, no sanitizer report.  Device pointers are fake non-null addresses: the host side must never dereference them.
 * Output: one line per case "ok <name> <status>" or "FAIL <name> <status>", exit code = number of failures. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dxmi_hip.h"

static int failures = 0;
#define FAKE(n) ((void*)(uintptr_t)(0x100000ull * (n)))
#define OFF(p, bytes) ((void*)((uintptr_t)(p) + (bytes)))

static void expect_einval(const char* name, int status, const char* needle) {
    const char* msg = dxmi_last_error();
    if (status == DXMI_EINVAL && msg && strstr(msg, needle)) printf("ok   %-44s %d  (%s)\n", name, status, msg);
    else { printf("FAIL %-44s %d  (%s), expected \"%s\"\n", name, status, msg ? msg : "(null)", needle); ++failures; }
}
static void expect_negative(const char* name, int status) {   /* valid arguments, no device: launch / device error, still no crash */
    if (status < 0) printf("ok   %-44s %d\n", name, status);
    else { printf("FAIL %-44s %d\n", name, status); ++failures; }
}

typedef struct {
    int32_t mode, rows, row, N, CHW;
    const float* tab; const int32_t* ctl; float* x; const float* eps; const float* z; const int64_t* idx;
    float* hist; float* t_out; float* out; float* pred;
} dpm_args;

static dpm_args good(void) {
    dpm_args a;
    a.mode = DXMI_DPM_STEP; a.rows = 10; a.row = 4; a.N = 4; a.CHW = 3072;
    a.tab = (const float*)FAKE(1); a.ctl = NULL; a.x = (float*)FAKE(2); a.eps = (const float*)FAKE(3); a.z = (const float*)FAKE(4);
    a.idx = NULL; a.hist = (float*)FAKE(5); a.t_out = (float*)FAKE(6); a.out = (float*)FAKE(7); a.pred = (float*)FAKE(8);
    return a;
}

static int call(dpm_args a) {
    return dxmi_dpm_stage(a.mode, a.tab, a.rows, a.ctl, a.row, 3u, 0x123456789abcull, a.x, a.eps, a.z, a.idx, a.hist, a.t_out, a.out,
                          a.pred, a.N, a.CHW, NULL);
}

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    dpm_args a;
    /* ---- null pointers ------------------------------------------------------------------------------------------- */
    a = good(); a.tab = NULL;                 expect_einval("dpm_stage(tab NULL)", call(a), "null pointer");
    a = good(); a.t_out = NULL;               expect_einval("dpm_stage(t_out NULL)", call(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("dpm_stage(x NULL)", call(a), "null pointer");
    a = good(); a.eps = NULL;                 expect_einval("dpm_stage(eps NULL)", call(a), "null pointer");
    a = good(); a.out = NULL;                 expect_einval("dpm_stage(out NULL)", call(a), "null pointer");
    a = good(); a.hist = NULL;                expect_einval("dpm_stage(hist NULL in STEP mode)", call(a), "history");
    a = good(); a.mode = DXMI_DPM_FIRST; a.tab = NULL;
                                              expect_einval("dpm_stage(FIRST, tab NULL)", call(a), "null pointer");
    /* ---- sizes, rows, modes -------------------------------------------------------------------------------------- */
    a = good(); a.N = 0;                      expect_einval("dpm_stage(N = 0)", call(a), "N (0)");
    a = good(); a.N = -4;                     expect_einval("dpm_stage(N < 0)", call(a), "N (-4)");
    a = good(); a.N = 65536;                  expect_einval("dpm_stage(N = 65536)", call(a), "N (65536)");
    a = good(); a.N = INT32_MAX;              expect_einval("dpm_stage(N = INT32_MAX)", call(a), "N (");
    a = good(); a.CHW = 0;                    expect_einval("dpm_stage(CHW = 0)", call(a), "CHW (0)");
    a = good(); a.CHW = INT32_MIN;            expect_einval("dpm_stage(CHW = INT32_MIN)", call(a), "CHW (");
    a = good(); a.rows = 0;                   expect_einval("dpm_stage(rows = 0)", call(a), "at least one row");
    a = good(); a.rows = -3;                  expect_einval("dpm_stage(rows < 0)", call(a), "at least one row");
    a = good(); a.row = 10;                   expect_einval("dpm_stage(row = rows)", call(a), "row (10)");
    a = good(); a.row = -1;                   expect_einval("dpm_stage(row = -1)", call(a), "row (-1)");
    a = good(); a.row = INT32_MAX;            expect_einval("dpm_stage(row = INT32_MAX)", call(a), "row (");
    a = good(); a.mode = DXMI_DPM_FIRST; a.row = 10;
                                              expect_einval("dpm_stage(FIRST, row = rows)", call(a), "row (10)");
    a = good(); a.mode = 2;                   expect_einval("dpm_stage(mode 2)", call(a), "unknown mode");
    a = good(); a.mode = -1;                  expect_einval("dpm_stage(mode -1)", call(a), "unknown mode");
    /* ---- noise sources ------------------------------------------------------------------------------------------- */
    a = good(); a.idx = (const int64_t*)FAKE(9);
                                              expect_einval("dpm_stage(z and sample_index)", call(a), "not both");
    /* ---- alignment ----------------------------------------------------------------------------------------------- */
    a = good(); a.x = (float*)OFF(a.x, 4);    expect_einval("dpm_stage(x + 4 bytes)", call(a), "16-byte aligned");
    a = good(); a.eps = (const float*)OFF(a.eps, 8);
                                              expect_einval("dpm_stage(eps + 8 bytes)", call(a), "16-byte aligned");
    a = good(); a.z = (const float*)OFF(a.z, 12);
                                              expect_einval("dpm_stage(z + 12 bytes)", call(a), "16-byte aligned");
    a = good(); a.hist = (float*)OFF(a.hist, 4);
                                              expect_einval("dpm_stage(hist + 4 bytes)", call(a), "16-byte aligned");
    a = good(); a.out = (float*)OFF(a.out, 1);
                                              expect_einval("dpm_stage(out + 1 byte)", call(a), "16-byte aligned");
    a = good(); a.pred = (float*)OFF(a.pred, 8);
                                              expect_einval("dpm_stage(pred_xstart + 8 bytes)", call(a), "16-byte aligned");
    a = good(); a.z = NULL; a.idx = (const int64_t*)OFF(FAKE(9), 4);
                                              expect_einval("dpm_stage(sample_index + 4 bytes)", call(a), "16-byte aligned");
    a = good(); a.ctl = (const int32_t*)OFF(FAKE(10), 2);
                                              expect_einval("dpm_stage(ctl + 2 bytes)", call(a), "4-byte aligned");
    a = good(); a.tab = (const float*)OFF(a.tab, 1);
                                              expect_einval("dpm_stage(tab + 1 byte)", call(a), "4-byte aligned");
    a = good(); a.t_out = (float*)OFF(a.t_out, 2);
                                              expect_einval("dpm_stage(t_out + 2 bytes)", call(a), "4-byte aligned");
    /* ---- valid argument sets reach the launch: no device here, so a negative status that is not a crash ------------ */
    a = good();                               expect_negative("dpm_stage(valid STEP, no device)", call(a));
    a = good(); a.CHW = 75; a.pred = NULL; a.z = NULL; a.idx = (const int64_t*)FAKE(9); a.ctl = (const int32_t*)FAKE(10); a.row = 99;
                                              expect_negative("dpm_stage(valid STEP, ctl, CHW % 4 != 0, no device)", call(a));
    a = good(); a.mode = DXMI_DPM_FIRST; a.x = NULL; a.eps = NULL; a.z = NULL; a.hist = NULL; a.out = NULL; a.pred = NULL;
                                              expect_negative("dpm_stage(valid FIRST, no device)", call(a));

    printf("%d failure(s)\n", failures);
    return failures > 99 ? 99 : failures;
}
