/* Host-side robustness driver for dxmi_edm_dpm_stage (csrc/edm_dpm_sample.hip), the stand-alone twin of cabi_malformed_dpm.c for
 * this one entry point.  Built by `make -C diffusion-by-maxentirl_amd/csrc asan_edm_dpm` against the HOST-ONLY AddressSanitizer +
 * UBSan build of the library's sources (no device code: hipcc --offload-host-only; never run on a GPU machine) and executed as a
 * child process by tests/test_edm_dpm_sample_host.py.  Every call hands the entry point a malformed argument set (null pointers,
 * misaligned pointers, sizes and rows out of range, a missing x_in): the contract (include/dxmi_hip.h, "Conventions") is
 * DXMI_EINVAL + dxmi_last_error() text, no crash, no sanitizer report.  Device pointers are fake non-null addresses: the host
 * side must never dereference them.
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
    if (status == DXMI_EINVAL && msg && strstr(msg, needle)) printf("ok   %-48s %d  (%s)\n", name, status, msg);
    else { printf("FAIL %-48s %d  (%s), expected \"%s\"\n", name, status, msg ? msg : "(null)", needle); ++failures; }
}
static void expect_negative(const char* name, int status) {   /* valid arguments, no device: launch / device error, still no crash */
    if (status < 0) printf("ok   %-48s %d\n", name, status);
    else { printf("FAIL %-48s %d\n", name, status); ++failures; }
}

typedef struct {
    int32_t mode, rows, row, N, CHW;
    const float* tab; const int32_t* ctl; float* x; const float* F; const float* z; const int64_t* idx;
    float* hist; float* x_in; float* t_out; float* out; float* pred;
} edm_args;

static edm_args good(void) {
    edm_args a;
    a.mode = DXMI_EDM_DPM_STEP; a.rows = 10; a.row = 4; a.N = 4; a.CHW = 3072;
    a.tab = (const float*)FAKE(1); a.ctl = NULL; a.x = (float*)FAKE(2); a.F = (const float*)FAKE(3); a.z = (const float*)FAKE(4);
    a.idx = NULL; a.hist = (float*)FAKE(5); a.t_out = (float*)FAKE(6); a.out = (float*)FAKE(7); a.pred = (float*)FAKE(8);
    a.x_in = (float*)FAKE(11);
    return a;
}

static edm_args good_first(void) {
    edm_args a = good();
    a.mode = DXMI_EDM_DPM_FIRST; a.row = 0; a.F = NULL; a.z = NULL; a.hist = NULL; a.out = NULL; a.pred = NULL;
    return a;
}

static int call(edm_args a) {
    return dxmi_edm_dpm_stage(a.mode, a.tab, a.rows, a.ctl, a.row, 3u, 0x123456789abcull, a.x, a.F, a.z, a.idx, a.hist, a.x_in, a.t_out,
                              a.out, a.pred, a.N, a.CHW, NULL);
}

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    edm_args a;
    /* ---- null pointers ------------------------------------------------------------------------------------------- */
    a = good(); a.tab = NULL;                 expect_einval("edm_dpm_stage(tab NULL)", call(a), "null pointer");
    a = good(); a.t_out = NULL;               expect_einval("edm_dpm_stage(t_out NULL)", call(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("edm_dpm_stage(x NULL)", call(a), "null pointer");
    a = good(); a.F = NULL;                   expect_einval("edm_dpm_stage(model_out NULL)", call(a), "null pointer");
    a = good(); a.out = NULL;                 expect_einval("edm_dpm_stage(out NULL)", call(a), "null pointer");
    a = good(); a.hist = NULL;                expect_einval("edm_dpm_stage(hist NULL in STEP mode)", call(a), "history");
    a = good(); a.x_in = NULL;                expect_einval("edm_dpm_stage(x_in NULL on a row that is not last)", call(a), "x_in");
    a = good(); a.x_in = NULL; a.row = 0;     expect_einval("edm_dpm_stage(x_in NULL on row 0)", call(a), "x_in");
    a = good(); a.x_in = NULL; a.row = 9; a.ctl = (const int32_t*)FAKE(10);
                                              expect_einval("edm_dpm_stage(x_in NULL with a control block)", call(a), "x_in");
    a = good_first(); a.tab = NULL;           expect_einval("edm_dpm_stage(FIRST, tab NULL)", call(a), "null pointer");
    a = good_first(); a.x = NULL;             expect_einval("edm_dpm_stage(FIRST, x NULL)", call(a), "null pointer");
    a = good_first(); a.x_in = NULL;          expect_einval("edm_dpm_stage(FIRST, x_in NULL)", call(a), "null pointer");
    a = good_first(); a.t_out = NULL;         expect_einval("edm_dpm_stage(FIRST, t_out NULL)", call(a), "null pointer");
    /* ---- sizes, rows, modes -------------------------------------------------------------------------------------- */
    a = good(); a.N = 0;                      expect_einval("edm_dpm_stage(N = 0)", call(a), "N (0)");
    a = good(); a.N = -4;                     expect_einval("edm_dpm_stage(N < 0)", call(a), "N (-4)");
    a = good(); a.N = 65536;                  expect_einval("edm_dpm_stage(N = 65536)", call(a), "N (65536)");
    a = good(); a.N = INT32_MAX;              expect_einval("edm_dpm_stage(N = INT32_MAX)", call(a), "N (");
    a = good(); a.CHW = 0;                    expect_einval("edm_dpm_stage(CHW = 0)", call(a), "CHW (0)");
    a = good(); a.CHW = -3072;                expect_einval("edm_dpm_stage(CHW < 0)", call(a), "CHW (-3072)");
    a = good(); a.CHW = INT32_MIN;            expect_einval("edm_dpm_stage(CHW = INT32_MIN)", call(a), "CHW (");
    a = good_first(); a.CHW = 0;              expect_einval("edm_dpm_stage(FIRST, CHW = 0)", call(a), "CHW (0)");
    a = good(); a.rows = 0;                   expect_einval("edm_dpm_stage(rows = 0)", call(a), "at least one row");
    a = good(); a.rows = -3;                  expect_einval("edm_dpm_stage(rows < 0)", call(a), "at least one row");
    a = good(); a.row = 10;                   expect_einval("edm_dpm_stage(row = rows)", call(a), "row (10)");
    a = good(); a.row = -1;                   expect_einval("edm_dpm_stage(row = -1)", call(a), "row (-1)");
    a = good(); a.row = INT32_MAX;            expect_einval("edm_dpm_stage(row = INT32_MAX)", call(a), "row (");
    a = good(); a.row = INT32_MIN;            expect_einval("edm_dpm_stage(row = INT32_MIN)", call(a), "row (");
    a = good_first(); a.row = 10;             expect_einval("edm_dpm_stage(FIRST, row = rows)", call(a), "row (10)");
    a = good(); a.mode = 2;                   expect_einval("edm_dpm_stage(mode 2)", call(a), "unknown mode");
    a = good(); a.mode = -1;                  expect_einval("edm_dpm_stage(mode -1)", call(a), "unknown mode");
    /* ---- noise sources ------------------------------------------------------------------------------------------- */
    a = good(); a.idx = (const int64_t*)FAKE(9);
                                              expect_einval("edm_dpm_stage(z and sample_index)", call(a), "not both");
    /* ---- alignment ----------------------------------------------------------------------------------------------- */
    a = good(); a.x = (float*)OFF(a.x, 4);    expect_einval("edm_dpm_stage(x + 4 bytes)", call(a), "16-byte aligned");
    a = good(); a.F = (const float*)OFF(a.F, 8);
                                              expect_einval("edm_dpm_stage(model_out + 8 bytes)", call(a), "16-byte aligned");
    a = good(); a.z = (const float*)OFF(a.z, 12);
                                              expect_einval("edm_dpm_stage(z + 12 bytes)", call(a), "16-byte aligned");
    a = good(); a.hist = (float*)OFF(a.hist, 4);
                                              expect_einval("edm_dpm_stage(hist + 4 bytes)", call(a), "16-byte aligned");
    a = good(); a.x_in = (float*)OFF(a.x_in, 4);
                                              expect_einval("edm_dpm_stage(x_in + 4 bytes)", call(a), "16-byte aligned");
    a = good(); a.out = (float*)OFF(a.out, 1);
                                              expect_einval("edm_dpm_stage(out + 1 byte)", call(a), "16-byte aligned");
    a = good(); a.pred = (float*)OFF(a.pred, 8);
                                              expect_einval("edm_dpm_stage(pred_xstart + 8 bytes)", call(a), "16-byte aligned");
    a = good(); a.z = NULL; a.idx = (const int64_t*)OFF(FAKE(9), 4);
                                              expect_einval("edm_dpm_stage(sample_index + 4 bytes)", call(a), "16-byte aligned");
    a = good(); a.ctl = (const int32_t*)OFF(FAKE(10), 2);
                                              expect_einval("edm_dpm_stage(ctl + 2 bytes)", call(a), "4-byte aligned");
    a = good(); a.tab = (const float*)OFF(a.tab, 1);
                                              expect_einval("edm_dpm_stage(tab + 1 byte)", call(a), "4-byte aligned");
    a = good(); a.t_out = (float*)OFF(a.t_out, 2);
                                              expect_einval("edm_dpm_stage(t_out + 2 bytes)", call(a), "4-byte aligned");
    a = good_first(); a.x = (float*)OFF(a.x, 4);
                                              expect_einval("edm_dpm_stage(FIRST, x + 4 bytes)", call(a), "16-byte aligned");
    a = good_first(); a.x_in = (float*)OFF(a.x_in, 8);
                                              expect_einval("edm_dpm_stage(FIRST, x_in + 8 bytes)", call(a), "16-byte aligned");
    /* ---- valid argument sets reach the launch: no device here, so a negative status that is not a crash ------------ */
    a = good();                               expect_negative("edm_dpm_stage(valid STEP, no device)", call(a));
    a = good(); a.row = 9; a.x_in = NULL;     expect_negative("edm_dpm_stage(valid last row without x_in, no device)", call(a));
    a = good(); a.CHW = 75; a.pred = NULL; a.z = NULL; a.idx = (const int64_t*)FAKE(9); a.ctl = (const int32_t*)FAKE(10); a.row = 99;
                                              expect_negative("edm_dpm_stage(valid STEP, ctl, CHW % 4 != 0, no device)", call(a));
    a = good_first();                         expect_negative("edm_dpm_stage(valid FIRST, no device)", call(a));

    printf("%d failure(s)\n", failures);
    return failures > 99 ? 99 : failures;
}
