/* Host-side robustness driver for the score identity distillation entry points (csrc/sid_train.hip): dxmi_sid_grad_fwd and
 * dxmi_sid_join.  The stand-alone twin of cabi_malformed_dm.c.  Built by `make -C diffusion-by-maxentirl_amd/csrc asan_sid` against
 * the HOST-ONLY AddressSanitizer + UBSan build of the library's sources (no device code: hipcc --offload-host-only; never run on a
 * GPU machine) and executed as a child process by tests/test_sid_host.py.  Every call hands an entry point a malformed argument
 * set (null pointers, misaligned pointers, sizes and scalars out of range, an output aliasing an input it may not alias): the
 * contract (include/dxmi_hip.h, "Conventions") is DXMI_EINVAL + dxmi_last_error() text, no crash, no sanitizer report.  Device
 * pointers are fake non-null addresses: the host side must never dereference them.
 * Output: one line per case "ok <name> <status>" or "FAIL <name> <status>", exit code = number of failures. */
#include <math.h>
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
    int32_t S, N, CHW, dist_f;
    float alpha, sdr, sdf;
    const float* Fr; const float* Ff; const float* x; const float* x_t; const int64_t* idx; const float* tab;
    const float* g_r; const float* g_f;
    float* v_r; float* v_f; float* d_dir; float* loss; float* s; float* g;
} sid_args;

static sid_args good(void) {
    sid_args a;
    a.S = 18; a.N = 4; a.CHW = 768; a.dist_f = 0; a.alpha = 1.2f; a.sdr = 0.5f; a.sdf = 0.25f;
    a.Fr = (const float*)FAKE(1); a.Ff = (const float*)FAKE(2); a.x = (const float*)FAKE(3); a.x_t = (const float*)FAKE(4);
    a.idx = (const int64_t*)FAKE(5); a.tab = (const float*)FAKE(6); a.g_r = (const float*)FAKE(7); a.g_f = (const float*)FAKE(8);
    a.v_r = (float*)FAKE(9); a.v_f = (float*)FAKE(10); a.d_dir = (float*)FAKE(11); a.loss = (float*)FAKE(12); a.s = (float*)FAKE(13);
    a.g = (float*)FAKE(14);
    return a;
}

static int grad(sid_args a) {
    return dxmi_sid_grad_fwd(a.Fr, a.Ff, a.x, a.x_t, a.idx, a.tab, a.S, a.alpha, a.v_r, a.v_f, a.d_dir, a.loss, a.s, a.N, a.CHW, a.sdr,
                             0.002f, 0, a.sdf, 0.002f, a.dist_f, NULL);
}
static int join(sid_args a) {
    return dxmi_sid_join(a.d_dir, a.g_r, a.g_f, a.s, a.idx, a.tab, a.S, a.g, a.N, a.CHW, a.sdr, a.sdf, NULL);
}

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    sid_args a;
    /* ---- dxmi_sid_grad_fwd ----------------------------------------------------------------------------------------- */
    a = good(); a.Fr = NULL;                  expect_einval("sid_grad_fwd(f_real NULL)", grad(a), "null pointer");
    a = good(); a.Ff = NULL;                  expect_einval("sid_grad_fwd(f_fake NULL)", grad(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("sid_grad_fwd(x NULL)", grad(a), "null pointer");
    a = good(); a.x_t = NULL;                 expect_einval("sid_grad_fwd(x_t NULL)", grad(a), "null pointer");
    a = good(); a.idx = NULL;                 expect_einval("sid_grad_fwd(indices NULL)", grad(a), "null pointer");
    a = good(); a.tab = NULL;                 expect_einval("sid_grad_fwd(t_table NULL)", grad(a), "null pointer");
    a = good(); a.v_r = NULL;                 expect_einval("sid_grad_fwd(v_real NULL)", grad(a), "null pointer");
    a = good(); a.v_f = NULL;                 expect_einval("sid_grad_fwd(v_fake NULL)", grad(a), "null pointer");
    a = good(); a.d_dir = NULL;               expect_einval("sid_grad_fwd(d_dir NULL)", grad(a), "null pointer");
    a = good(); a.loss = NULL;                expect_einval("sid_grad_fwd(loss NULL)", grad(a), "null pointer");
    a = good(); a.s = NULL;                   expect_einval("sid_grad_fwd(s NULL)", grad(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("sid_grad_fwd(N = 0)", grad(a), "N (0)");
    a = good(); a.N = -3;                     expect_einval("sid_grad_fwd(N < 0)", grad(a), "N (-3)");
    a = good(); a.N = 65536;                  expect_einval("sid_grad_fwd(N = 65536)", grad(a), "N (65536)");
    a = good(); a.N = INT32_MAX;              expect_einval("sid_grad_fwd(N = INT32_MAX)", grad(a), "N (");
    a = good(); a.CHW = 770;                  expect_einval("sid_grad_fwd(CHW % 4 != 0)", grad(a), "CHW (770)");
    a = good(); a.CHW = 0;                    expect_einval("sid_grad_fwd(CHW = 0)", grad(a), "CHW (0)");
    a = good(); a.CHW = -8;                   expect_einval("sid_grad_fwd(CHW < 0)", grad(a), "CHW (-8)");
    a = good(); a.CHW = INT32_MIN;            expect_einval("sid_grad_fwd(CHW = INT32_MIN)", grad(a), "CHW (");
    a = good(); a.CHW = INT32_MAX - 3;        expect_einval("sid_grad_fwd(CHW = 2^31 - 4)", grad(a), "CHW (");
    a = good(); a.S = 0;                      expect_einval("sid_grad_fwd(num_scales = 0)", grad(a), "num_scales (0)");
    a = good(); a.S = -2;                     expect_einval("sid_grad_fwd(num_scales < 0)", grad(a), "num_scales (-2)");
    a = good(); a.S = INT32_MAX;              expect_einval("sid_grad_fwd(num_scales = INT32_MAX)", grad(a), "num_scales (");
    a = good(); a.alpha = NAN;                expect_einval("sid_grad_fwd(alpha NaN)", grad(a), "alpha");
    a = good(); a.alpha = INFINITY;           expect_einval("sid_grad_fwd(alpha inf)", grad(a), "alpha");
    a = good(); a.alpha = -INFINITY;          expect_einval("sid_grad_fwd(alpha -inf)", grad(a), "alpha");
    a = good(); a.sdr = 0.f;                  expect_einval("sid_grad_fwd(real sigma_data = 0)", grad(a), "sigma_data");
    a = good(); a.sdr = -0.5f;                expect_einval("sid_grad_fwd(real sigma_data < 0)", grad(a), "sigma_data");
    a = good(); a.sdf = NAN;                  expect_einval("sid_grad_fwd(fake sigma_data NaN)", grad(a), "sigma_data");
    a = good(); a.sdf = INFINITY;             expect_einval("sid_grad_fwd(fake sigma_data inf)", grad(a), "sigma_data");
    a = good(); a.Fr = (const float*)OFF(a.Fr, 4);
                                              expect_einval("sid_grad_fwd(f_real + 4 bytes)", grad(a), "16-byte aligned");
    a = good(); a.x_t = (const float*)OFF(a.x_t, 12);
                                              expect_einval("sid_grad_fwd(x_t + 12 bytes)", grad(a), "16-byte aligned");
    a = good(); a.v_r = (float*)OFF(a.v_r, 8);
                                              expect_einval("sid_grad_fwd(v_real + 8 bytes)", grad(a), "16-byte aligned");
    a = good(); a.v_f = (float*)OFF(a.v_f, 1);
                                              expect_einval("sid_grad_fwd(v_fake + 1 byte)", grad(a), "16-byte aligned");
    a = good(); a.d_dir = (float*)OFF(a.d_dir, 4);
                                              expect_einval("sid_grad_fwd(d_dir + 4 bytes)", grad(a), "16-byte aligned");
    /* ---- dxmi_sid_join --------------------------------------------------------------------------------------------- */
    a = good(); a.d_dir = NULL;               expect_einval("sid_join(d_dir NULL)", join(a), "null pointer");
    a = good(); a.g_r = NULL;                 expect_einval("sid_join(g_real NULL)", join(a), "null pointer");
    a = good(); a.g_f = NULL;                 expect_einval("sid_join(g_fake NULL)", join(a), "null pointer");
    a = good(); a.s = NULL;                   expect_einval("sid_join(s NULL)", join(a), "null pointer");
    a = good(); a.idx = NULL;                 expect_einval("sid_join(indices NULL)", join(a), "null pointer");
    a = good(); a.tab = NULL;                 expect_einval("sid_join(t_table NULL)", join(a), "null pointer");
    a = good(); a.g = NULL;                   expect_einval("sid_join(g NULL)", join(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("sid_join(N = 0)", join(a), "N (0)");
    a = good(); a.N = 65536;                  expect_einval("sid_join(N = 65536)", join(a), "N (65536)");
    a = good(); a.CHW = 6;                    expect_einval("sid_join(CHW = 6)", join(a), "CHW (6)");
    a = good(); a.CHW = INT32_MAX - 3;        expect_einval("sid_join(CHW = 2^31 - 4)", join(a), "CHW (");
    a = good(); a.S = 0;                      expect_einval("sid_join(num_scales = 0)", join(a), "num_scales (0)");
    a = good(); a.sdr = 0.f;                  expect_einval("sid_join(real sigma_data = 0)", join(a), "sigma_data");
    a = good(); a.sdf = -0.25f;               expect_einval("sid_join(fake sigma_data < 0)", join(a), "sigma_data");
    a = good(); a.g_r = (const float*)OFF(a.g_r, 4);
                                              expect_einval("sid_join(g_real + 4 bytes)", join(a), "16-byte aligned");
    a = good(); a.g = (float*)OFF(a.g, 8);    expect_einval("sid_join(g + 8 bytes)", join(a), "16-byte aligned");
    a = good(); a.g = (float*)a.g_r;          expect_einval("sid_join(g aliases g_real)", join(a), "alias d_dir only");
    a = good(); a.g = (float*)a.g_f;          expect_einval("sid_join(g aliases g_fake)", join(a), "alias d_dir only");
    /* ---- valid argument sets reach the launch: no device here, so a negative status that is not a crash ------------ */
    a = good();                               expect_negative("sid_grad_fwd(valid small image, no device)", grad(a));
    a = good(); a.CHW = 12288; a.alpha = 1.f; a.dist_f = 1;
                                              expect_negative("sid_grad_fwd(valid 3x64x64, no device)", grad(a));
    a = good(); a.CHW = 19200; a.S = 1;       expect_negative("sid_grad_fwd(valid 3x80x80, num_scales 1)", grad(a));
    a = good();                               expect_negative("sid_join(valid, no device)", join(a));
    a = good(); a.g = a.d_dir;                expect_negative("sid_join(valid, g aliases d_dir)", join(a));

    printf("%d failure(s)\n", failures);
    return failures > 99 ? 99 : failures;
}
