/* Host-side robustness driver for the distribution-matching entry points (csrc/dm_train.hip): dxmi_dm_gen_in, dxmi_dm_gen_out,
 * dxmi_dm_gen_prep, dxmi_dm_grad_fwd and dxmi_dm_gen_bwd.  The stand-alone twin of cabi_malformed_pd.c.  Built by
 * `make -C diffusion-by-maxentirl_amd/csrc asan_dm` against the HOST-ONLY AddressSanitizer + UBSan build of the library's sources
 * (no device code: hipcc --offload-host-only; never run on a GPU machine) and executed as a child process by
 * tests/test_dm_host.py.  Every call hands an entry point a malformed argument set (null pointers, misaligned pointers, sizes,
 * weightings and scalars out of range): the contract (include/dxmi_hip.h, "Conventions") is DXMI_EINVAL + dxmi_last_error()
 * text, no crash, no sanitizer report.  Device pointers are fake non-null addresses: the host side must never dereference them.
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
    int32_t S, N, CHW, weighting;
    float sg, sd, sdr, sdf;
    const float* z; const float* F; const float* noise; const float* Fr; const float* Ff; const float* up; const int64_t* idx;
    const float* tab;
    float* x; float* x_t; float* x_in; float* t_out; float* x_fk; float* g; float* loss; float* s;
} dm_args;

static dm_args good(void) {
    dm_args a;
    a.S = 18; a.N = 4; a.CHW = 768; a.weighting = DXMI_DM_W_DMD; a.sg = 80.f; a.sd = 0.5f; a.sdr = 0.5f; a.sdf = 0.25f;
    a.z = (const float*)FAKE(1); a.F = (const float*)FAKE(2); a.noise = (const float*)FAKE(3); a.Fr = (const float*)FAKE(4);
    a.Ff = (const float*)FAKE(5); a.up = (const float*)FAKE(6); a.idx = (const int64_t*)FAKE(7); a.tab = (const float*)FAKE(8);
    a.x = (float*)FAKE(9); a.x_t = (float*)FAKE(10); a.x_in = (float*)FAKE(11); a.t_out = (float*)FAKE(12); a.x_fk = (float*)FAKE(13);
    a.g = (float*)FAKE(14); a.loss = (float*)FAKE(15); a.s = (float*)FAKE(16);
    return a;
}

static int gen_in(dm_args a) { return dxmi_dm_gen_in(a.z, a.x_in, a.t_out, a.N, a.CHW, a.sg, a.sd, NULL); }
static int gen_out(dm_args a) { return dxmi_dm_gen_out(a.F, a.z, a.x, a.N, a.CHW, a.sg, a.sd, 1, NULL); }
static int prep(dm_args a) {
    return dxmi_dm_gen_prep(a.F, a.z, a.noise, a.idx, a.tab, a.S, a.x, a.x_t, a.x_in, a.t_out, a.x_fk, a.N, a.CHW, a.sg, a.sd, a.sdr,
                            a.sdf, NULL);
}
static int grad(dm_args a) {
    return dxmi_dm_grad_fwd(a.Fr, a.Ff, a.x, a.x_t, a.idx, a.tab, a.S, a.g, a.loss, a.s, a.N, a.CHW, a.weighting, a.sdr, 0.002f, 0,
                            a.sdf, 0.002f, 0, NULL);
}
static int bwd(dm_args a) { return dxmi_dm_gen_bwd(a.up, a.g, a.x, a.N, a.CHW, a.sg, a.sd, NULL); }

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    dm_args a;
    /* ---- dxmi_dm_gen_in -------------------------------------------------------------------------------------------- */
    a = good(); a.z = NULL;                   expect_einval("dm_gen_in(z NULL)", gen_in(a), "null pointer");
    a = good(); a.x_in = NULL;                expect_einval("dm_gen_in(x_in NULL)", gen_in(a), "null pointer");
    a = good(); a.t_out = NULL;               expect_einval("dm_gen_in(t_out NULL)", gen_in(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("dm_gen_in(N = 0)", gen_in(a), "N (0)");
    a = good(); a.N = -3;                     expect_einval("dm_gen_in(N < 0)", gen_in(a), "N (-3)");
    a = good(); a.N = 65536;                  expect_einval("dm_gen_in(N = 65536)", gen_in(a), "N (65536)");
    a = good(); a.CHW = 770;                  expect_einval("dm_gen_in(CHW % 4 != 0)", gen_in(a), "CHW (770)");
    a = good(); a.CHW = 0;                    expect_einval("dm_gen_in(CHW = 0)", gen_in(a), "CHW (0)");
    a = good(); a.CHW = INT32_MIN;            expect_einval("dm_gen_in(CHW = INT32_MIN)", gen_in(a), "CHW (");
    a = good(); a.CHW = INT32_MAX - 3;        expect_einval("dm_gen_in(CHW = 2^31 - 4)", gen_in(a), "CHW (");
    a = good(); a.sg = 0.f;                   expect_einval("dm_gen_in(gen_sigma = 0)", gen_in(a), "gen_sigma");
    a = good(); a.sg = -80.f;                 expect_einval("dm_gen_in(gen_sigma < 0)", gen_in(a), "gen_sigma");
    a = good(); a.sg = NAN;                   expect_einval("dm_gen_in(gen_sigma NaN)", gen_in(a), "gen_sigma");
    a = good(); a.sg = INFINITY;              expect_einval("dm_gen_in(gen_sigma inf)", gen_in(a), "gen_sigma");
    a = good(); a.sd = 0.f;                   expect_einval("dm_gen_in(sigma_data = 0)", gen_in(a), "sigma_data");
    a = good(); a.sd = -0.5f;                 expect_einval("dm_gen_in(sigma_data < 0)", gen_in(a), "sigma_data");
    a = good(); a.z = (const float*)OFF(a.z, 4);
                                              expect_einval("dm_gen_in(z + 4 bytes)", gen_in(a), "16-byte aligned");
    a = good(); a.x_in = (float*)OFF(a.x_in, 8);
                                              expect_einval("dm_gen_in(x_in + 8 bytes)", gen_in(a), "16-byte aligned");
    /* ---- dxmi_dm_gen_out ------------------------------------------------------------------------------------------- */
    a = good(); a.F = NULL;                   expect_einval("dm_gen_out(f_gen NULL)", gen_out(a), "null pointer");
    a = good(); a.z = NULL;                   expect_einval("dm_gen_out(z NULL)", gen_out(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("dm_gen_out(x NULL)", gen_out(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("dm_gen_out(N = 0)", gen_out(a), "N (0)");
    a = good(); a.CHW = 6;                    expect_einval("dm_gen_out(CHW = 6)", gen_out(a), "CHW (6)");
    a = good(); a.sg = 0.f;                   expect_einval("dm_gen_out(gen_sigma = 0)", gen_out(a), "gen_sigma");
    a = good(); a.sd = 0.f;                   expect_einval("dm_gen_out(sigma_data = 0)", gen_out(a), "sigma_data");
    a = good(); a.x = (float*)OFF(a.x, 1);    expect_einval("dm_gen_out(x + 1 byte)", gen_out(a), "16-byte aligned");
    /* ---- dxmi_dm_gen_prep ------------------------------------------------------------------------------------------ */
    a = good(); a.F = NULL;                   expect_einval("dm_gen_prep(f_gen NULL)", prep(a), "null pointer");
    a = good(); a.noise = NULL;               expect_einval("dm_gen_prep(noise NULL)", prep(a), "null pointer");
    a = good(); a.idx = NULL;                 expect_einval("dm_gen_prep(indices NULL)", prep(a), "null pointer");
    a = good(); a.tab = NULL;                 expect_einval("dm_gen_prep(t_table NULL)", prep(a), "null pointer");
    a = good(); a.x_t = NULL;                 expect_einval("dm_gen_prep(x_t NULL)", prep(a), "null pointer");
    a = good(); a.x_in = NULL;                expect_einval("dm_gen_prep(x_in_real NULL)", prep(a), "null pointer");
    a = good(); a.t_out = NULL;               expect_einval("dm_gen_prep(t_out NULL)", prep(a), "null pointer");
    a = good(); a.N = -1;                     expect_einval("dm_gen_prep(N < 0)", prep(a), "N (-1)");
    a = good(); a.CHW = 2;                    expect_einval("dm_gen_prep(CHW = 2)", prep(a), "CHW (2)");
    a = good(); a.S = 0;                      expect_einval("dm_gen_prep(num_scales = 0)", prep(a), "num_scales (0)");
    a = good(); a.S = -2;                     expect_einval("dm_gen_prep(num_scales < 0)", prep(a), "num_scales (-2)");
    a = good(); a.S = INT32_MAX;              expect_einval("dm_gen_prep(num_scales = INT32_MAX)", prep(a), "num_scales (");
    a = good(); a.sg = -1.f;                  expect_einval("dm_gen_prep(gen_sigma < 0)", prep(a), "gen_sigma");
    a = good(); a.sd = 0.f;                   expect_einval("dm_gen_prep(generator sigma_data = 0)", prep(a), "sigma_data");
    a = good(); a.sdr = 0.f;                  expect_einval("dm_gen_prep(real sigma_data = 0)", prep(a), "sigma_data");
    a = good(); a.sdf = -0.25f;               expect_einval("dm_gen_prep(fake sigma_data < 0)", prep(a), "sigma_data");
    a = good(); a.x_fk = (float*)OFF(a.x_fk, 4);
                                              expect_einval("dm_gen_prep(x_in_fake + 4 bytes)", prep(a), "16-byte aligned");
    a = good(); a.noise = (const float*)OFF(a.noise, 12);
                                              expect_einval("dm_gen_prep(noise + 12 bytes)", prep(a), "16-byte aligned");
    /* ---- dxmi_dm_grad_fwd ------------------------------------------------------------------------------------------ */
    a = good(); a.Fr = NULL;                  expect_einval("dm_grad_fwd(f_real NULL)", grad(a), "null pointer");
    a = good(); a.Ff = NULL;                  expect_einval("dm_grad_fwd(f_fake NULL)", grad(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("dm_grad_fwd(x NULL)", grad(a), "null pointer");
    a = good(); a.g = NULL;                   expect_einval("dm_grad_fwd(g NULL)", grad(a), "null pointer");
    a = good(); a.loss = NULL;                expect_einval("dm_grad_fwd(loss NULL)", grad(a), "null pointer");
    a = good(); a.s = NULL;                   expect_einval("dm_grad_fwd(s NULL)", grad(a), "null pointer");
    a = good(); a.weighting = 2;              expect_einval("dm_grad_fwd(weighting 2)", grad(a), "unknown weighting");
    a = good(); a.weighting = -1;             expect_einval("dm_grad_fwd(weighting -1)", grad(a), "unknown weighting");
    a = good(); a.N = 0;                      expect_einval("dm_grad_fwd(N = 0)", grad(a), "N (0)");
    a = good(); a.N = INT32_MAX;              expect_einval("dm_grad_fwd(N = INT32_MAX)", grad(a), "N (");
    a = good(); a.CHW = -8;                   expect_einval("dm_grad_fwd(CHW < 0)", grad(a), "CHW (-8)");
    a = good(); a.CHW = 12290;                expect_einval("dm_grad_fwd(CHW = 12290)", grad(a), "CHW (12290)");
    a = good(); a.S = 0;                      expect_einval("dm_grad_fwd(num_scales = 0)", grad(a), "num_scales (0)");
    a = good(); a.sdr = 0.f;                  expect_einval("dm_grad_fwd(real sigma_data = 0)", grad(a), "sigma_data");
    a = good(); a.sdf = NAN;                  expect_einval("dm_grad_fwd(fake sigma_data NaN)", grad(a), "sigma_data");
    a = good(); a.g = (float*)OFF(a.g, 8);    expect_einval("dm_grad_fwd(g + 8 bytes)", grad(a), "16-byte aligned");
    a = good(); a.x_t = (float*)OFF(a.x_t, 4);
                                              expect_einval("dm_grad_fwd(x_t + 4 bytes)", grad(a), "16-byte aligned");
    /* ---- dxmi_dm_gen_bwd ------------------------------------------------------------------------------------------- */
    a = good(); a.up = NULL;                  expect_einval("dm_gen_bwd(upstream NULL)", bwd(a), "null pointer");
    a = good(); a.g = NULL;                   expect_einval("dm_gen_bwd(g NULL)", bwd(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("dm_gen_bwd(d_f_gen NULL)", bwd(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("dm_gen_bwd(N = 0)", bwd(a), "N (0)");
    a = good(); a.CHW = 5;                    expect_einval("dm_gen_bwd(CHW = 5)", bwd(a), "CHW (5)");
    a = good(); a.sg = 0.f;                   expect_einval("dm_gen_bwd(gen_sigma = 0)", bwd(a), "gen_sigma");
    a = good(); a.sd = -1.f;                  expect_einval("dm_gen_bwd(sigma_data < 0)", bwd(a), "sigma_data");
    a = good(); a.x = (float*)OFF(a.x, 4);    expect_einval("dm_gen_bwd(d_f_gen + 4 bytes)", bwd(a), "16-byte aligned");
    /* ---- valid argument sets reach the launch: no device here, so a negative status that is not a crash ------------ */
    a = good();                               expect_negative("dm_gen_in(valid, no device)", gen_in(a));
    a = good();                               expect_negative("dm_gen_out(valid, no device)", gen_out(a));
    a = good();                               expect_negative("dm_gen_prep(valid, no device)", prep(a));
    a = good(); a.x_fk = NULL; a.S = 1;       expect_negative("dm_gen_prep(valid, no x_in_fake, num_scales 1)", prep(a));
    a = good(); a.CHW = 768;                  expect_negative("dm_grad_fwd(valid small image, no device)", grad(a));
    a = good(); a.CHW = 12288; a.weighting = DXMI_DM_W_NONE;
                                              expect_negative("dm_grad_fwd(valid 3x64x64, no device)", grad(a));
    a = good(); a.CHW = 49152;                expect_negative("dm_grad_fwd(valid two-pass, no device)", grad(a));
    a = good();                               expect_negative("dm_gen_bwd(valid, no device)", bwd(a));

    printf("%d failure(s)\n", failures);
    return failures > 99 ? 99 : failures;
}
