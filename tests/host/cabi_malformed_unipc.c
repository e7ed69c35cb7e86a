/* Host-side robustness driver for dxmi_unipc_stage (csrc/unipc_sample.hip) and dxmi_edm_unipc_stage (csrc/edm_unipc_sample.hip), the
 * stand-alone twin of cabi_malformed_edm_dpm.c for these two entry points.  Built by `make -C diffusion-by-maxentirl_amd/csrc
 * asan_unipc` against the HOST-ONLY AddressSanitizer + UBSan build of the library's sources (no device code: hipcc
 * --offload-host-only; never run on a GPU machine) and executed as a child process by tests/test_unipc_sample_host.py.  Every call
 * hands an entry point a malformed argument set (null pointers, misaligned pointers, sizes and rows out of range, xc == x, a
 * missing x_in): the contract (include/dxmi_hip.h, "Conventions") is DXMI_EINVAL + dxmi_last_error() text, no crash, no sanitizer
 * report.  Device pointers are fake non-null addresses: the host side must never dereference them.  e = 0: dxmi_unipc_stage,
 * e = 1: dxmi_edm_unipc_stage.
 * Output: one line per case "ok <name> <status>" or "FAIL <name> <status>", exit code = number of failures. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dxmi_hip.h"

static int failures = 0;
#define FAKE(n) ((void*)(uintptr_t)(0x100000ull * (n)))
#define OFF(p, bytes) ((void*)((uintptr_t)(p) + (bytes)))
static const char* ENTRY[2] = {"unipc_stage", "edm_unipc_stage"};

static void expect_einval(int e, const char* what, int status, const char* needle) {
    const char* msg = dxmi_last_error();
    char name[96];
    snprintf(name, sizeof name, "%s(%s)", ENTRY[e], what);
    if (status == DXMI_EINVAL && msg && strstr(msg, needle)) printf("ok   %-56s %d  (%s)\n", name, status, msg);
    else { printf("FAIL %-56s %d  (%s), expected \"%s\"\n", name, status, msg ? msg : "(null)", needle); ++failures; }
}
static void expect_negative(int e, const char* what, int status) {   /* valid arguments, no device: a launch / device error, no crash */
    char name[96];
    snprintf(name, sizeof name, "%s(%s)", ENTRY[e], what);
    if (status < 0) printf("ok   %-56s %d\n", name, status);
    else { printf("FAIL %-56s %d\n", name, status); ++failures; }
}

typedef struct {
    int32_t mode, rows, row, N, CHW;
    const float* tab; const int32_t* ctl; float* x; float* xc; const float* eps; float* hist; float* x_in; float* t_out; float* out;
    float* pred;
} uni_args;

static uni_args good(void) {
    uni_args a;
    a.mode = DXMI_UNIPC_STEP; a.rows = 10; a.row = 4; a.N = 4; a.CHW = 3072;
    a.tab = (const float*)FAKE(1); a.ctl = NULL; a.x = (float*)FAKE(2); a.eps = (const float*)FAKE(3); a.xc = (float*)FAKE(4);
    a.hist = (float*)FAKE(5); a.t_out = (float*)FAKE(6); a.out = (float*)FAKE(7); a.pred = (float*)FAKE(8); a.x_in = (float*)FAKE(11);
    return a;
}

static uni_args good_first(void) {
    uni_args a = good();
    a.mode = DXMI_UNIPC_FIRST; a.row = 0; a.eps = NULL; a.xc = NULL; a.hist = NULL; a.out = NULL; a.pred = NULL;
    return a;
}

static int call(int e, uni_args a) {
    if (e) return dxmi_edm_unipc_stage(a.mode, a.tab, a.rows, a.ctl, a.row, a.x, a.xc, a.eps, a.hist, a.x_in, a.t_out, a.out, a.pred, a.N,
                                       a.CHW, NULL);
    return dxmi_unipc_stage(a.mode, a.tab, a.rows, a.ctl, a.row, a.x, a.xc, a.eps, a.hist, a.t_out, a.out, a.pred, a.N, a.CHW, NULL);
}

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    uni_args a;
    for (int e = 0; e < 2; ++e) {
        /* ---- null pointers --------------------------------------------------------------------------------------- */
        a = good(); a.tab = NULL;                 expect_einval(e, "tab NULL", call(e, a), "null pointer");
        a = good(); a.t_out = NULL;               expect_einval(e, "t_out NULL", call(e, a), "null pointer");
        a = good(); a.x = NULL;                   expect_einval(e, "x NULL", call(e, a), "null pointer");
        a = good(); a.eps = NULL;                 expect_einval(e, "eps / model_out NULL", call(e, a), "null pointer");
        a = good(); a.out = NULL;                 expect_einval(e, "out NULL", call(e, a), "null pointer");
        a = good(); a.hist = NULL;                expect_einval(e, "hist NULL in STEP mode", call(e, a), "history");
        a = good_first(); a.tab = NULL;           expect_einval(e, "FIRST, tab NULL", call(e, a), "null pointer");
        a = good_first(); a.t_out = NULL;         expect_einval(e, "FIRST, t_out NULL", call(e, a), "null pointer");
        /* ---- the two states -------------------------------------------------------------------------------------- */
        a = good(); a.xc = a.x;                   expect_einval(e, "xc == x", call(e, a), "two states");
        a = good(); a.xc = (float*)OFF(a.xc, 4);  expect_einval(e, "xc + 4 bytes", call(e, a), "16-byte aligned");
        /* ---- sizes, rows, modes ---------------------------------------------------------------------------------- */
        a = good(); a.N = 0;                      expect_einval(e, "N = 0", call(e, a), "N (0)");
        a = good(); a.N = -4;                     expect_einval(e, "N < 0", call(e, a), "N (-4)");
        a = good(); a.N = 65536;                  expect_einval(e, "N = 65536", call(e, a), "N (65536)");
        a = good(); a.N = INT32_MAX;              expect_einval(e, "N = INT32_MAX", call(e, a), "N (");
        a = good(); a.CHW = 0;                    expect_einval(e, "CHW = 0", call(e, a), "CHW (0)");
        a = good(); a.CHW = -3072;                expect_einval(e, "CHW < 0", call(e, a), "CHW (-3072)");
        a = good(); a.CHW = INT32_MIN;            expect_einval(e, "CHW = INT32_MIN", call(e, a), "CHW (");
        a = good_first(); a.CHW = 0;              expect_einval(e, "FIRST, CHW = 0", call(e, a), "CHW (0)");
        a = good(); a.rows = 0;                   expect_einval(e, "rows = 0", call(e, a), "at least one row");
        a = good(); a.rows = -3;                  expect_einval(e, "rows < 0", call(e, a), "at least one row");
        a = good(); a.row = 10;                   expect_einval(e, "row = rows", call(e, a), "row (10)");
        a = good(); a.row = -1;                   expect_einval(e, "row = -1", call(e, a), "row (-1)");
        a = good(); a.row = INT32_MAX;            expect_einval(e, "row = INT32_MAX", call(e, a), "row (");
        a = good(); a.row = INT32_MIN;            expect_einval(e, "row = INT32_MIN", call(e, a), "row (");
        a = good_first(); a.row = 10;             expect_einval(e, "FIRST, row = rows", call(e, a), "row (10)");
        a = good(); a.mode = 2;                   expect_einval(e, "mode 2", call(e, a), "unknown mode");
        a = good(); a.mode = -1;                  expect_einval(e, "mode -1", call(e, a), "unknown mode");
        /* ---- alignment ------------------------------------------------------------------------------------------- */
        a = good(); a.x = (float*)OFF(a.x, 4);    expect_einval(e, "x + 4 bytes", call(e, a), "16-byte aligned");
        a = good(); a.eps = (const float*)OFF(a.eps, 8);
                                                  expect_einval(e, "eps / model_out + 8 bytes", call(e, a), "16-byte aligned");
        a = good(); a.hist = (float*)OFF(a.hist, 4);
                                                  expect_einval(e, "hist + 4 bytes", call(e, a), "16-byte aligned");
        a = good(); a.out = (float*)OFF(a.out, 1);
                                                  expect_einval(e, "out + 1 byte", call(e, a), "16-byte aligned");
        a = good(); a.pred = (float*)OFF(a.pred, 8);
                                                  expect_einval(e, "pred_xstart + 8 bytes", call(e, a), "16-byte aligned");
        a = good(); a.ctl = (const int32_t*)OFF(FAKE(10), 2);
                                                  expect_einval(e, "ctl + 2 bytes", call(e, a), "4-byte aligned");
        a = good(); a.tab = (const float*)OFF(a.tab, 1);
                                                  expect_einval(e, "tab + 1 byte", call(e, a), "4-byte aligned");
        a = good(); a.t_out = (float*)OFF(a.t_out, 2);
                                                  expect_einval(e, "t_out + 2 bytes", call(e, a), "4-byte aligned");
        /* ---- valid argument sets reach the launch: no device here, so a negative status that is not a crash -------- */
        a = good();                               expect_negative(e, "valid STEP, no device", call(e, a));
        a = good(); a.xc = NULL;                  expect_negative(e, "valid STEP without xc, no device", call(e, a));
        a = good(); a.CHW = 75; a.pred = NULL; a.ctl = (const int32_t*)FAKE(10); a.row = 99;
                                                  expect_negative(e, "valid STEP, ctl, CHW % 4 != 0, no device", call(e, a));
        a = good_first();                         expect_negative(e, "valid FIRST, no device", call(e, a));
    }
    /* ---- the second output stream of the EDM entry ------------------------------------------------------------------ */
    a = good(); a.x_in = NULL;                    expect_einval(1, "x_in NULL on a row that is not last", call(1, a), "x_in");
    a = good(); a.x_in = NULL; a.row = 9; a.ctl = (const int32_t*)FAKE(10);
                                                  expect_einval(1, "x_in NULL with a control block", call(1, a), "x_in");
    a = good(); a.x_in = (float*)OFF(a.x_in, 4);  expect_einval(1, "x_in + 4 bytes", call(1, a), "16-byte aligned");
    a = good_first(); a.x = NULL;                 expect_einval(1, "FIRST, x NULL", call(1, a), "null pointer");
    a = good_first(); a.x_in = NULL;              expect_einval(1, "FIRST, x_in NULL", call(1, a), "null pointer");
    a = good_first(); a.x = (float*)OFF(a.x, 4);  expect_einval(1, "FIRST, x + 4 bytes", call(1, a), "16-byte aligned");
    a = good(); a.row = 9; a.x_in = NULL;         expect_negative(1, "valid last row without x_in, no device", call(1, a));

    printf("%d failure(s)\n", failures);
    return failures > 99 ? 99 : failures;
}
