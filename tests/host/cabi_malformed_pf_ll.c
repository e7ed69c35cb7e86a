/* Host-side robustness driver for dxmi_pf_ll_stage (csrc/pf_likelihood.hip), the stand-alone twin of cabi_malformed_edm_dpm.c for
 * this one entry point.  Built by `make -C diffusion-by-maxentirl_amd/csrc asan_pf_ll` against the HOST-ONLY AddressSanitizer +
 * UBSan build of the library's sources (no device code: hipcc --offload-host-only; never run on a GPU machine) and executed as a
 * child process by tests/test_likelihood_host.py.  Every call hands the entry point a malformed argument set (null pointers,
 * misaligned pointers, sizes and rows out of range, no probe or two, aliased tensors, a missing x_in): the contract
 * (include/dxmi_hip.h, "Conventions") is DXMI_EINVAL + dxmi_last_error() text, no crash, no sanitizer report.  Device pointers are
 * fake non-null addresses: the host side must never dereference them.
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
    if (status == DXMI_EINVAL && msg && strstr(msg, needle)) printf("ok   %-52s %d  (%s)\n", name, status, msg);
    else { printf("FAIL %-52s %d  (%s), expected \"%s\"\n", name, status, msg ? msg : "(null)", needle); ++failures; }
}
static void expect_negative(const char* name, int status) {   /* valid arguments, no device: launch / device error, still no crash */
    if (status < 0) printf("ok   %-52s %d\n", name, status);
    else { printf("FAIL %-52s %d\n", name, status); ++failures; }
}

typedef struct {
    int32_t mode, rows, row, N, CHW;
    const float* tab; const int32_t* ctl; float* x; const float* F; const float* g; const float* eps; const int64_t* idx;
    float* k1; float* xt; float* x_in; float* t_out; float* div1; float* ell; float* prior; float* logp; float* bpd;
} ll_args;

static ll_args good(int32_t mode) {
    ll_args a;
    a.mode = mode; a.rows = 10; a.row = 4; a.N = 4; a.CHW = 3072;
    a.tab = (const float*)FAKE(1); a.ctl = NULL; a.x = (float*)FAKE(2); a.F = (const float*)FAKE(3); a.g = (const float*)FAKE(4);
    a.eps = (const float*)FAKE(5); a.idx = NULL; a.k1 = (float*)FAKE(6); a.xt = NULL; a.x_in = (float*)FAKE(7);
    a.t_out = (float*)FAKE(8); a.div1 = (float*)FAKE(9); a.ell = (float*)FAKE(10); a.prior = (float*)FAKE(11);
    a.logp = (float*)FAKE(12); a.bpd = (float*)FAKE(13);
    return a;
}

static int call(ll_args a) {
    return dxmi_pf_ll_stage(a.mode, a.tab, a.rows, a.ctl, a.row, 3u, 0x123456789abcull, a.x, a.F, a.g, a.eps, a.idx, a.k1, a.xt, a.x_in,
                            a.t_out, a.div1, a.ell, a.prior, a.logp, a.bpd, a.N, a.CHW, NULL);
}

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    ll_args a;
    const int32_t P = DXMI_PF_LL_PREDICT, C = DXMI_PF_LL_CORRECT, F = DXMI_PF_LL_FIRST;
    /* ---- null pointers ------------------------------------------------------------------------------------------- */
    a = good(P); a.tab = NULL;                 expect_einval("pf_ll_stage(tab NULL)", call(a), "null pointer");
    a = good(P); a.t_out = NULL;               expect_einval("pf_ll_stage(t_out NULL)", call(a), "null pointer");
    a = good(P); a.x = NULL;                   expect_einval("pf_ll_stage(x NULL)", call(a), "null pointer");
    a = good(P); a.F = NULL;                   expect_einval("pf_ll_stage(model_out NULL)", call(a), "null pointer");
    a = good(P); a.g = NULL;                   expect_einval("pf_ll_stage(vjp NULL)", call(a), "null pointer");
    a = good(P); a.k1 = NULL;                  expect_einval("pf_ll_stage(k1 NULL)", call(a), "null pointer");
    a = good(P); a.div1 = NULL;                expect_einval("pf_ll_stage(div1 NULL)", call(a), "null pointer");
    a = good(P); a.x_in = NULL;                expect_einval("pf_ll_stage(PREDICT, x_in NULL)", call(a), "x_in");
    a = good(P); a.x_in = NULL; a.row = 9;     expect_einval("pf_ll_stage(PREDICT, x_in NULL on the last row)", call(a), "x_in");
    a = good(C); a.x_in = NULL;                expect_einval("pf_ll_stage(CORRECT, x_in NULL on a row that is not last)", call(a), "x_in");
    a = good(C); a.x_in = NULL; a.row = 9; a.ctl = (const int32_t*)FAKE(14);
                                               expect_einval("pf_ll_stage(CORRECT, x_in NULL with a control block)", call(a), "x_in");
    a = good(C); a.ell = NULL;                 expect_einval("pf_ll_stage(CORRECT, ell NULL)", call(a), "null pointer");
    a = good(C); a.prior = NULL;               expect_einval("pf_ll_stage(CORRECT, prior NULL)", call(a), "null pointer");
    a = good(C); a.logp = NULL;                expect_einval("pf_ll_stage(CORRECT, logp NULL)", call(a), "null pointer");
    a = good(C); a.bpd = NULL;                 expect_einval("pf_ll_stage(CORRECT, bpd NULL)", call(a), "null pointer");
    a = good(F); a.ell = NULL;                 expect_einval("pf_ll_stage(FIRST, ell NULL)", call(a), "null pointer");
    a = good(F); a.x = NULL;                   expect_einval("pf_ll_stage(FIRST, x NULL)", call(a), "null pointer");
    a = good(F); a.x_in = NULL;                expect_einval("pf_ll_stage(FIRST, x_in NULL)", call(a), "null pointer");
    a = good(F); a.tab = NULL;                 expect_einval("pf_ll_stage(FIRST, tab NULL)", call(a), "null pointer");
    /* ---- sizes, rows, mode ---------------------------------------------------------------------------------------- */
    a = good(P); a.N = 0;                      expect_einval("pf_ll_stage(N = 0)", call(a), "N (0)");
    a = good(P); a.N = -4;                     expect_einval("pf_ll_stage(N < 0)", call(a), "N (-4)");
    a = good(P); a.N = 65536;                  expect_einval("pf_ll_stage(N = 65536)", call(a), "N (65536)");
    a = good(P); a.N = INT32_MAX;              expect_einval("pf_ll_stage(N = INT32_MAX)", call(a), "N (");
    a = good(P); a.CHW = 0;                    expect_einval("pf_ll_stage(CHW = 0)", call(a), "CHW (0)");
    a = good(P); a.CHW = -3072;                expect_einval("pf_ll_stage(CHW < 0)", call(a), "CHW (-3072)");
    a = good(P); a.CHW = INT32_MIN;            expect_einval("pf_ll_stage(CHW = INT32_MIN)", call(a), "CHW (");
    a = good(P); a.CHW = 1 << 30;              expect_einval("pf_ll_stage(CHW = 2^30)", call(a), "CHW (");
    a = good(F); a.CHW = 0;                    expect_einval("pf_ll_stage(FIRST, CHW = 0)", call(a), "CHW (0)");
    a = good(P); a.rows = 0;                   expect_einval("pf_ll_stage(rows = 0)", call(a), "at least one row");
    a = good(P); a.rows = -3;                  expect_einval("pf_ll_stage(rows < 0)", call(a), "at least one row");
    a = good(P); a.row = 10;                   expect_einval("pf_ll_stage(row = rows)", call(a), "row (10)");
    a = good(C); a.row = -1;                   expect_einval("pf_ll_stage(row = -1)", call(a), "row (-1)");
    a = good(C); a.row = INT32_MAX;            expect_einval("pf_ll_stage(row = INT32_MAX)", call(a), "row (");
    a = good(P); a.row = INT32_MIN;            expect_einval("pf_ll_stage(row = INT32_MIN)", call(a), "row (");
    a = good(F); a.row = 10;                   expect_einval("pf_ll_stage(FIRST, row = rows)", call(a), "row (10)");
    a = good(3);                               expect_einval("pf_ll_stage(mode 3)", call(a), "unknown mode");
    a = good(-1);                              expect_einval("pf_ll_stage(mode -1)", call(a), "unknown mode");
    /* ---- the probe ------------------------------------------------------------------------------------------------ */
    a = good(P); a.idx = (const int64_t*)FAKE(15);
                                               expect_einval("pf_ll_stage(eps and sample_index)", call(a), "not both");
    a = good(C); a.eps = NULL;                 expect_einval("pf_ll_stage(neither eps nor sample_index)", call(a), "not neither");
    /* ---- aliased tensors ------------------------------------------------------------------------------------------ */
    a = good(P); a.k1 = a.x;                   expect_einval("pf_ll_stage(k1 is x)", call(a), "none may be another");
    a = good(P); a.x_in = a.x;                 expect_einval("pf_ll_stage(x_in is x)", call(a), "none may be another");
    a = good(C); a.x_in = a.k1;                expect_einval("pf_ll_stage(x_in is k1)", call(a), "none may be another");
    a = good(P); a.xt = a.x;                   expect_einval("pf_ll_stage(xt is x)", call(a), "none may be another");
    a = good(P); a.xt = a.k1;                  expect_einval("pf_ll_stage(xt is k1)", call(a), "none may be another");
    /* ---- alignment ------------------------------------------------------------------------------------------------ */
    a = good(P); a.x = (float*)OFF(a.x, 4);    expect_einval("pf_ll_stage(x + 4 bytes)", call(a), "16-byte aligned");
    a = good(P); a.F = (const float*)OFF(a.F, 8);
                                               expect_einval("pf_ll_stage(model_out + 8 bytes)", call(a), "16-byte aligned");
    a = good(P); a.g = (const float*)OFF(a.g, 12);
                                               expect_einval("pf_ll_stage(vjp + 12 bytes)", call(a), "16-byte aligned");
    a = good(C); a.eps = (const float*)OFF(a.eps, 4);
                                               expect_einval("pf_ll_stage(eps + 4 bytes)", call(a), "16-byte aligned");
    a = good(C); a.k1 = (float*)OFF(a.k1, 4);  expect_einval("pf_ll_stage(k1 + 4 bytes)", call(a), "16-byte aligned");
    a = good(P); a.xt = (float*)OFF(FAKE(16), 8);
                                               expect_einval("pf_ll_stage(xt + 8 bytes)", call(a), "16-byte aligned");
    a = good(P); a.x_in = (float*)OFF(a.x_in, 1);
                                               expect_einval("pf_ll_stage(x_in + 1 byte)", call(a), "16-byte aligned");
    a = good(P); a.eps = NULL; a.idx = (const int64_t*)OFF(FAKE(15), 4);
                                               expect_einval("pf_ll_stage(sample_index + 4 bytes)", call(a), "16-byte aligned");
    a = good(P); a.ctl = (const int32_t*)OFF(FAKE(14), 2);
                                               expect_einval("pf_ll_stage(ctl + 2 bytes)", call(a), "4-byte aligned");
    a = good(P); a.tab = (const float*)OFF(a.tab, 1);
                                               expect_einval("pf_ll_stage(tab + 1 byte)", call(a), "4-byte aligned");
    a = good(P); a.t_out = (float*)OFF(a.t_out, 2);
                                               expect_einval("pf_ll_stage(t_out + 2 bytes)", call(a), "4-byte aligned");
    a = good(C); a.bpd = (float*)OFF(a.bpd, 2);
                                               expect_einval("pf_ll_stage(bpd + 2 bytes)", call(a), "4-byte aligned");
    a = good(F); a.x = (float*)OFF(a.x, 4);    expect_einval("pf_ll_stage(FIRST, x + 4 bytes)", call(a), "16-byte aligned");
    /* ---- valid calls: no device here, so a launch error, never a crash ---------------------------------------------------- */
    a = good(F); a.row = 0;                    expect_negative("pf_ll_stage(valid FIRST, no device)", call(a));
    a = good(P);                               expect_negative("pf_ll_stage(valid PREDICT, no device)", call(a));
    a = good(P); a.xt = (float*)FAKE(16); a.eps = NULL; a.idx = (const int64_t*)FAKE(15); a.CHW = 3071; a.ctl = (const int32_t*)FAKE(14);
                                               expect_negative("pf_ll_stage(valid PREDICT, fused, ctl, CHW % 4 != 0, no device)", call(a));
    a = good(C);                               expect_negative("pf_ll_stage(valid CORRECT, no device)", call(a));
    a = good(C); a.row = 9; a.x_in = NULL;     expect_negative("pf_ll_stage(valid CORRECT on the last row without x_in, no device)", call(a));
    printf("%d failure(s)\n", failures);
    return failures;
}
