/* Host-side robustness driver for the K-step generator's entry points (csrc/dm_train.hip): dxmi_dmms_in, dxmi_dmms_stage,
 * dxmi_dmms_prep, dxmi_dmms_out and dxmi_dmms_bwd.  The stand-alone twin of cabi_malformed_dm.c.  Built by
 * `make -C diffusion-by-maxentirl_amd/csrc asan_dmms` against the HOST-ONLY AddressSanitizer + UBSan build of the library's sources
 * (no device code: hipcc --offload-host-only; never run on a GPU machine) and executed as a child process by
 * tests/test_dmms_host.py.  Every call hands an entry point a malformed argument set (null pointers, misaligned pointers, sizes,
 * stages and scalars out of range, both or neither noise source): the contract (include/dxmi_hip.h, "Conventions") is DXMI_EINVAL
 * + dxmi_last_error() text, no crash, no sanitizer report.  Device pointers are fake non-null addresses: the host side must never
 * dereference them.  Output: one line per case "ok <name> <status>" or "FAIL <name> <status>", exit code = number of failures. */
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
    int32_t S, K, stage, N, CHW;
    float sd, sdr, sdf;
    const float* z; const float* F; const float* noise; const float* eps; const float* up; const float* g; const int64_t* idx;
    const int64_t* steps; const int64_t* sample_index; const float* tab; const float* sig;
    float* x; float* x_t; float* x_in; float* t_out; float* x_fk; float* dF;
} ms_args;

static ms_args good(void) {
    ms_args a;
    a.S = 18; a.K = 4; a.stage = 1; a.N = 4; a.CHW = 768; a.sd = 0.5f; a.sdr = 0.5f; a.sdf = 0.25f;
    a.z = (const float*)FAKE(1); a.F = (const float*)FAKE(2); a.noise = (const float*)FAKE(3); a.eps = (const float*)FAKE(4);
    a.up = (const float*)FAKE(5); a.g = (const float*)FAKE(6); a.idx = (const int64_t*)FAKE(7); a.steps = (const int64_t*)FAKE(8);
    a.sample_index = NULL; a.tab = (const float*)FAKE(9); a.sig = (const float*)FAKE(10);
    a.x = (float*)FAKE(11); a.x_t = (float*)FAKE(12); a.x_in = (float*)FAKE(13); a.t_out = (float*)FAKE(14); a.x_fk = (float*)FAKE(15);
    a.dF = (float*)FAKE(16);
    return a;
}

static int ms_in(ms_args a) { return dxmi_dmms_in(a.z, a.sig, a.K, a.x, a.x_in, a.t_out, a.N, a.CHW, a.sd, NULL); }
static int stage(ms_args a) {
    return dxmi_dmms_stage(a.F, a.eps, a.sample_index, 3u, 0x123456789abcdefull, a.steps, a.sig, a.K, a.stage, a.x, a.x_in, a.t_out, a.N,
                           a.CHW, a.sd, NULL);
}
static int prep(ms_args a) {
    return dxmi_dmms_prep(a.F, a.x, a.noise, a.steps, a.sig, a.K, a.idx, a.tab, a.S, a.dF, a.x_t, a.x_in, a.t_out, a.x_fk, a.N, a.CHW,
                          a.sd, a.sdr, a.sdf, NULL);
}
static int ms_out(ms_args a) { return dxmi_dmms_out(a.F, a.z, a.sig, a.K, a.x, a.N, a.CHW, a.sd, 1, NULL); }
static int bwd(ms_args a) { return dxmi_dmms_bwd(a.up, a.g, a.steps, a.sig, a.K, a.dF, a.N, a.CHW, a.sd, NULL); }

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    ms_args a;
    /* ---- dxmi_dmms_in ---------------------------------------------------------------------------------------------- */
    a = good(); a.z = NULL;                   expect_einval("dmms_in(z NULL)", ms_in(a), "null pointer");
    a = good(); a.sig = NULL;                 expect_einval("dmms_in(gen_sigmas NULL)", ms_in(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("dmms_in(x NULL)", ms_in(a), "null pointer");
    a = good(); a.x_in = NULL;                expect_einval("dmms_in(x_in NULL)", ms_in(a), "null pointer");
    a = good(); a.t_out = NULL;               expect_einval("dmms_in(t_out NULL)", ms_in(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("dmms_in(N = 0)", ms_in(a), "N (0)");
    a = good(); a.N = 65536;                  expect_einval("dmms_in(N = 65536)", ms_in(a), "N (65536)");
    a = good(); a.CHW = 770;                  expect_einval("dmms_in(CHW % 4 != 0)", ms_in(a), "CHW (770)");
    a = good(); a.CHW = INT32_MIN;            expect_einval("dmms_in(CHW = INT32_MIN)", ms_in(a), "CHW (");
    a = good(); a.K = 0;                      expect_einval("dmms_in(num_steps = 0)", ms_in(a), "num_steps (0)");
    a = good(); a.K = -4;                     expect_einval("dmms_in(num_steps < 0)", ms_in(a), "num_steps (-4)");
    a = good(); a.K = INT32_MAX;              expect_einval("dmms_in(num_steps = INT32_MAX)", ms_in(a), "num_steps (");
    a = good(); a.sd = 0.f;                   expect_einval("dmms_in(sigma_data = 0)", ms_in(a), "sigma_data");
    a = good(); a.sd = NAN;                   expect_einval("dmms_in(sigma_data NaN)", ms_in(a), "sigma_data");
    a = good(); a.sig = (const float*)OFF(a.sig, 2);
                                              expect_einval("dmms_in(gen_sigmas + 2 bytes)", ms_in(a), "4-byte aligned");
    a = good(); a.z = (const float*)OFF(a.z, 4);
                                              expect_einval("dmms_in(z + 4 bytes)", ms_in(a), "16-byte aligned");
    a = good(); a.x = (float*)OFF(a.x, 8);    expect_einval("dmms_in(x + 8 bytes)", ms_in(a), "16-byte aligned");
    /* ---- dxmi_dmms_stage ------------------------------------------------------------------------------------------- */
    a = good(); a.F = NULL;                   expect_einval("dmms_stage(f_gen NULL)", stage(a), "null pointer");
    a = good(); a.sig = NULL;                 expect_einval("dmms_stage(gen_sigmas NULL)", stage(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("dmms_stage(x NULL)", stage(a), "null pointer");
    a = good(); a.x_in = NULL;                expect_einval("dmms_stage(x_in NULL)", stage(a), "null pointer");
    a = good(); a.t_out = NULL;               expect_einval("dmms_stage(t_out NULL)", stage(a), "null pointer");
    a = good(); a.sample_index = (const int64_t*)FAKE(17);
                                              expect_einval("dmms_stage(eps and sample_index)", stage(a), "not both");
    a = good(); a.eps = NULL;                 expect_einval("dmms_stage(neither eps nor sample_index)", stage(a), "noise is needed");
    a = good(); a.N = -1;                     expect_einval("dmms_stage(N < 0)", stage(a), "N (-1)");
    a = good(); a.CHW = 6;                    expect_einval("dmms_stage(CHW = 6)", stage(a), "CHW (6)");
    a = good(); a.K = 0;                      expect_einval("dmms_stage(num_steps = 0)", stage(a), "num_steps (0)");
    a = good(); a.K = 1; a.stage = 0;         expect_einval("dmms_stage(num_steps = 1: no stage)", stage(a), "stage (0)");
    a = good(); a.stage = -1;                 expect_einval("dmms_stage(stage < 0)", stage(a), "stage (-1)");
    a = good(); a.stage = 3;                  expect_einval("dmms_stage(stage = K - 1)", stage(a), "stage (3)");
    a = good(); a.stage = INT32_MAX;          expect_einval("dmms_stage(stage = INT32_MAX)", stage(a), "stage (");
    a = good(); a.sd = -0.5f;                 expect_einval("dmms_stage(sigma_data < 0)", stage(a), "sigma_data");
    a = good(); a.steps = (const int64_t*)OFF(a.steps, 4);
                                              expect_einval("dmms_stage(steps + 4 bytes)", stage(a), "8-byte aligned");
    a = good(); a.eps = NULL; a.sample_index = (const int64_t*)OFF(FAKE(17), 4);
                                              expect_einval("dmms_stage(sample_index + 4 bytes)", stage(a), "8-byte aligned");
    a = good(); a.eps = (const float*)OFF(a.eps, 4);
                                              expect_einval("dmms_stage(eps + 4 bytes)", stage(a), "16-byte aligned");
    a = good(); a.x_in = (float*)OFF(a.x_in, 12);
                                              expect_einval("dmms_stage(x_in + 12 bytes)", stage(a), "16-byte aligned");
    /* ---- dxmi_dmms_prep -------------------------------------------------------------------------------------------- */
    a = good(); a.F = NULL;                   expect_einval("dmms_prep(f_gen NULL)", prep(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("dmms_prep(x_k NULL)", prep(a), "null pointer");
    a = good(); a.noise = NULL;               expect_einval("dmms_prep(noise NULL)", prep(a), "null pointer");
    a = good(); a.steps = NULL;               expect_einval("dmms_prep(steps NULL)", prep(a), "null pointer");
    a = good(); a.sig = NULL;                 expect_einval("dmms_prep(gen_sigmas NULL)", prep(a), "null pointer");
    a = good(); a.idx = NULL;                 expect_einval("dmms_prep(indices NULL)", prep(a), "null pointer");
    a = good(); a.tab = NULL;                 expect_einval("dmms_prep(t_table NULL)", prep(a), "null pointer");
    a = good(); a.x_in = NULL;                expect_einval("dmms_prep(x_in_real NULL)", prep(a), "null pointer");
    a = good(); a.t_out = NULL;               expect_einval("dmms_prep(t_out NULL)", prep(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("dmms_prep(N = 0)", prep(a), "N (0)");
    a = good(); a.CHW = 2;                    expect_einval("dmms_prep(CHW = 2)", prep(a), "CHW (2)");
    a = good(); a.K = 0;                      expect_einval("dmms_prep(num_steps = 0)", prep(a), "num_steps (0)");
    a = good(); a.S = 0;                      expect_einval("dmms_prep(num_scales = 0)", prep(a), "num_scales (0)");
    a = good(); a.S = INT32_MAX;              expect_einval("dmms_prep(num_scales = INT32_MAX)", prep(a), "num_scales (");
    a = good(); a.sd = 0.f;                   expect_einval("dmms_prep(generator sigma_data = 0)", prep(a), "sigma_data");
    a = good(); a.sdr = INFINITY;             expect_einval("dmms_prep(real sigma_data inf)", prep(a), "sigma_data");
    a = good(); a.sdf = -0.25f;               expect_einval("dmms_prep(fake sigma_data < 0)", prep(a), "sigma_data");
    a = good(); a.steps = (const int64_t*)OFF(a.steps, 2);
                                              expect_einval("dmms_prep(steps + 2 bytes)", prep(a), "8-byte aligned");
    a = good(); a.x_fk = (float*)OFF(a.x_fk, 4);
                                              expect_einval("dmms_prep(x_in_fake + 4 bytes)", prep(a), "16-byte aligned");
    a = good(); a.noise = (const float*)OFF(a.noise, 12);
                                              expect_einval("dmms_prep(noise + 12 bytes)", prep(a), "16-byte aligned");
    /* ---- dxmi_dmms_out --------------------------------------------------------------------------------------------- */
    a = good(); a.F = NULL;                   expect_einval("dmms_out(f_gen NULL)", ms_out(a), "null pointer");
    a = good(); a.z = NULL;                   expect_einval("dmms_out(x_k NULL)", ms_out(a), "null pointer");
    a = good(); a.sig = NULL;                 expect_einval("dmms_out(gen_sigmas NULL)", ms_out(a), "null pointer");
    a = good(); a.x = NULL;                   expect_einval("dmms_out(x NULL)", ms_out(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("dmms_out(N = 0)", ms_out(a), "N (0)");
    a = good(); a.CHW = 5;                    expect_einval("dmms_out(CHW = 5)", ms_out(a), "CHW (5)");
    a = good(); a.K = -1;                     expect_einval("dmms_out(num_steps < 0)", ms_out(a), "num_steps (-1)");
    a = good(); a.sd = 0.f;                   expect_einval("dmms_out(sigma_data = 0)", ms_out(a), "sigma_data");
    a = good(); a.x = (float*)OFF(a.x, 1);    expect_einval("dmms_out(x + 1 byte)", ms_out(a), "16-byte aligned");
    /* ---- dxmi_dmms_bwd --------------------------------------------------------------------------------------------- */
    a = good(); a.up = NULL;                  expect_einval("dmms_bwd(upstream NULL)", bwd(a), "null pointer");
    a = good(); a.g = NULL;                   expect_einval("dmms_bwd(g NULL)", bwd(a), "null pointer");
    a = good(); a.steps = NULL;               expect_einval("dmms_bwd(steps NULL)", bwd(a), "null pointer");
    a = good(); a.sig = NULL;                 expect_einval("dmms_bwd(gen_sigmas NULL)", bwd(a), "null pointer");
    a = good(); a.dF = NULL;                  expect_einval("dmms_bwd(d_f_gen NULL)", bwd(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("dmms_bwd(N = 0)", bwd(a), "N (0)");
    a = good(); a.CHW = -8;                   expect_einval("dmms_bwd(CHW < 0)", bwd(a), "CHW (-8)");
    a = good(); a.K = 0;                      expect_einval("dmms_bwd(num_steps = 0)", bwd(a), "num_steps (0)");
    a = good(); a.sd = -1.f;                  expect_einval("dmms_bwd(sigma_data < 0)", bwd(a), "sigma_data");
    a = good(); a.dF = (float*)OFF(a.dF, 4);  expect_einval("dmms_bwd(d_f_gen + 4 bytes)", bwd(a), "16-byte aligned");
    /* ---- valid argument sets reach the launch: no device here, so a negative status that is not a crash ------------ */
    a = good();                               expect_negative("dmms_in(valid, no device)", ms_in(a));
    a = good(); a.K = 1;                      expect_negative("dmms_in(valid, one level)", ms_in(a));
    a = good();                               expect_negative("dmms_stage(valid, eps given)", stage(a));
    a = good(); a.eps = NULL; a.sample_index = (const int64_t*)FAKE(17); a.steps = NULL; a.stage = 2;
                                              expect_negative("dmms_stage(valid, noise made here, no steps)", stage(a));
    a = good();                               expect_negative("dmms_prep(valid, no device)", prep(a));
    a = good(); a.x_fk = NULL; a.K = 1;       expect_negative("dmms_prep(valid, no x_in_fake, one level)", prep(a));
    a = good();                               expect_negative("dmms_out(valid, no device)", ms_out(a));
    a = good();                               expect_negative("dmms_bwd(valid, no device)", bwd(a));

    printf("%d failure(s)\n", failures);
    return failures > 99 ? 99 : failures;
}
