/* Host-side robustness driver for the entry points of DMD2's GAN head (csrc/gan_head.hip): dxmi_gan_head_supported,
 * dxmi_gan_conv4s2_pack / _fwd / _dgrad / _wgrad, dxmi_gan_logit_loss_fwd / _bwd and dxmi_gan_join.  The stand-alone twin of
 * cabi_malformed_sid.c.  Built by `make -C diffusion-by-maxentirl_amd/csrc asan_gan` against the HOST-ONLY AddressSanitizer + UBSan
 * build of the library's sources (no device code: hipcc --offload-host-only; never run on a GPU machine) and executed as a child
 * process by tests/test_gan_host.py.  Every call hands an entry point a malformed argument set (null pointers, zero or negative N, an
 * unsupported C, H not in {4, 8}, a workspace that is too small, misaligned pointers): the contract (include/dxmi_hip.h,
 * "Conventions") is DXMI_EINVAL + dxmi_last_error() text before any launch, no crash, no sanitizer report.  Device pointers are fake
 * non-null addresses: the host side must never dereference them.
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
static void expect_value(const char* name, long long got, long long want) {
    if (got == want) printf("ok   %-44s %lld\n", name, got);
    else { printf("FAIL %-44s %lld, expected %lld\n", name, got, want); ++failures; }
}

typedef struct {
    int32_t N, H, C, S, CHW;
    int64_t ws_bytes;
    float weight, sd;
    const void* x; const void* w; const void* wt; const float* bias; void* y; void* ws;
    const void* dy; void* dx; float* dw; float* db;
    const float* sign; float* logit; float* loss; const float* up; void* d_a;
    const float* g; const float* d_xin; const int64_t* idx; const float* tab; float* out;
} gan_args;

static gan_args good(void) {
    gan_args a;
    a.N = 3; a.H = 8; a.C = 128; a.S = 18; a.CHW = 768; a.ws_bytes = 1 << 26; a.weight = 3e-3f; a.sd = 0.5f;
    a.x = FAKE(1); a.w = FAKE(2); a.wt = FAKE(3); a.bias = (const float*)FAKE(4); a.y = FAKE(5); a.ws = FAKE(6);
    a.dy = FAKE(7); a.dx = FAKE(8); a.dw = (float*)FAKE(9); a.db = (float*)FAKE(10);
    a.sign = (const float*)FAKE(11); a.logit = (float*)FAKE(12); a.loss = (float*)FAKE(13); a.up = (const float*)FAKE(14); a.d_a = FAKE(15);
    a.g = (const float*)FAKE(16); a.d_xin = (const float*)FAKE(17); a.idx = (const int64_t*)FAKE(18); a.tab = (const float*)FAKE(19);
    a.out = (float*)FAKE(20);
    return a;
}

static int fwd(gan_args a) { return dxmi_gan_conv4s2_fwd(a.x, a.w, a.bias, a.y, a.ws, a.ws_bytes, a.N, a.H, a.C, NULL); }
static int dgrad(gan_args a) { return dxmi_gan_conv4s2_dgrad(a.dy, a.wt, a.dx, a.ws, a.ws_bytes, a.N, a.H, a.C, NULL); }
static int wgrad(gan_args a) { return dxmi_gan_conv4s2_wgrad(a.x, a.dy, a.dw, a.db, a.N, a.H, a.C, NULL); }
static int pack(gan_args a) { return dxmi_gan_conv4s2_pack((const float*)a.x, (void*)a.w, (void*)a.wt, a.C, NULL); }
static int lfwd(gan_args a) { return dxmi_gan_logit_loss_fwd(a.x, (const float*)a.w, a.bias, a.sign, a.logit, a.loss, a.N, a.C, NULL); }
static int lbwd(gan_args a) {
    return dxmi_gan_logit_loss_bwd(a.x, (const float*)a.w, a.sign, a.logit, a.up, a.weight, a.d_a, a.dw, a.db, a.N, a.C, NULL);
}
static int join(gan_args a) { return dxmi_gan_join(a.g, a.d_xin, a.idx, a.tab, a.S, a.out, a.N, a.CHW, a.weight, a.sd, NULL); }

int main(void) {
    setvbuf(stdout, NULL, _IOLBF, 0);
    gan_args a;
    /* ---- dxmi_gan_head_supported / workspace ----------------------------------------------------------------------- */
    expect_einval("head_supported(C = 96)", dxmi_gan_head_supported(96, 8), "C (96)");
    expect_einval("head_supported(C = 0)", dxmi_gan_head_supported(0, 8), "C (0)");
    expect_einval("head_supported(C = -128)", dxmi_gan_head_supported(-128, 8), "C (-128)");
    expect_einval("head_supported(C = 2048)", dxmi_gan_head_supported(2048, 8), "C (2048)");
    expect_einval("head_supported(map 6)", dxmi_gan_head_supported(128, 6), "map size (6)");
    expect_einval("head_supported(map 16)", dxmi_gan_head_supported(128, 16), "map size (16)");
    {
        static const int served[] = {128, 192, 256, 768, 1024};
        for (int i = 0; i < 5; ++i) expect_value("head_supported(served C)", dxmi_gan_head_supported(served[i], 8), DXMI_OK);
    }
    expect_value("workspace_bytes(fwd 3, 8, 128)", dxmi_gan_conv4s2_workspace_bytes(3, 8, 128, 0), 16ll * 48 * 128 * 4);
    expect_value("workspace_bytes(dgrad 3, 8, 128)", dxmi_gan_conv4s2_workspace_bytes(3, 8, 128, 1), 4ll * 192 * 128 * 4);
    expect_value("workspace_bytes(N = 0)", dxmi_gan_conv4s2_workspace_bytes(0, 8, 128, 0), 0);
    expect_value("workspace_bytes(H = 16)", dxmi_gan_conv4s2_workspace_bytes(3, 16, 128, 0), 0);
    expect_value("workspace_bytes(C = 100)", dxmi_gan_conv4s2_workspace_bytes(3, 8, 100, 0), 0);
    expect_value("slices(fwd)", dxmi_gan_conv4s2_slices(0), 16);
    expect_value("slices(dgrad)", dxmi_gan_conv4s2_slices(1), 4);
    /* ---- dxmi_gan_conv4s2_pack ------------------------------------------------------------------------------------- */
    a = good(); a.x = NULL;                   expect_einval("conv4s2_pack(w NULL)", pack(a), "null pointer");
    a = good(); a.w = NULL;                   expect_einval("conv4s2_pack(w_fwd NULL)", pack(a), "null pointer");
    a = good(); a.wt = NULL;                  expect_einval("conv4s2_pack(w_t NULL)", pack(a), "null pointer");
    a = good(); a.C = 96;                     expect_einval("conv4s2_pack(C = 96)", pack(a), "C (96)");
    a = good(); a.C = 0;                      expect_einval("conv4s2_pack(C = 0)", pack(a), "C (0)");
    a = good(); a.w = OFF(a.w, 4);            expect_einval("conv4s2_pack(w_fwd + 4 bytes)", pack(a), "16-byte aligned");
    /* ---- dxmi_gan_conv4s2_fwd -------------------------------------------------------------------------------------- */
    a = good(); a.x = NULL;                   expect_einval("conv4s2_fwd(x NULL)", fwd(a), "null pointer");
    a = good(); a.w = NULL;                   expect_einval("conv4s2_fwd(w_fwd NULL)", fwd(a), "null pointer");
    a = good(); a.y = NULL;                   expect_einval("conv4s2_fwd(y NULL)", fwd(a), "null pointer");
    a = good(); a.ws = NULL;                  expect_einval("conv4s2_fwd(workspace NULL)", fwd(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("conv4s2_fwd(N = 0)", fwd(a), "N (0)");
    a = good(); a.N = -2;                     expect_einval("conv4s2_fwd(N < 0)", fwd(a), "N (-2)");
    a = good(); a.N = INT32_MAX;              expect_einval("conv4s2_fwd(N = INT32_MAX)", fwd(a), "N (");
    a = good(); a.H = 6;                      expect_einval("conv4s2_fwd(H = 6)", fwd(a), "H (6)");
    a = good(); a.H = 16;                     expect_einval("conv4s2_fwd(H = 16)", fwd(a), "H (16)");
    a = good(); a.H = 0;                      expect_einval("conv4s2_fwd(H = 0)", fwd(a), "H (0)");
    a = good(); a.C = 96;                     expect_einval("conv4s2_fwd(C = 96)", fwd(a), "C (96)");
    a = good(); a.C = 1088;                   expect_einval("conv4s2_fwd(C = 1088)", fwd(a), "C (1088)");
    a = good(); a.C = -64;                    expect_einval("conv4s2_fwd(C < 0)", fwd(a), "C (-64)");
    a = good(); a.ws_bytes = 16ll * 48 * 128 * 4 - 1;
                                              expect_einval("conv4s2_fwd(workspace 1 byte short)", fwd(a), "workspace of");
    a = good(); a.ws_bytes = 0;               expect_einval("conv4s2_fwd(workspace 0 bytes)", fwd(a), "workspace of");
    a = good(); a.ws_bytes = -1;              expect_einval("conv4s2_fwd(workspace < 0 bytes)", fwd(a), "workspace of");
    a = good(); a.x = OFF(a.x, 2);            expect_einval("conv4s2_fwd(x + 2 bytes)", fwd(a), "16-byte aligned");
    a = good(); a.y = OFF(a.y, 8);            expect_einval("conv4s2_fwd(y + 8 bytes)", fwd(a), "16-byte aligned");
    a = good(); a.ws = OFF(a.ws, 8);          expect_einval("conv4s2_fwd(workspace + 8 bytes)", fwd(a), "16-byte aligned");
    /* ---- dxmi_gan_conv4s2_dgrad ------------------------------------------------------------------------------------ */
    a = good(); a.dy = NULL;                  expect_einval("conv4s2_dgrad(dy NULL)", dgrad(a), "null pointer");
    a = good(); a.wt = NULL;                  expect_einval("conv4s2_dgrad(w_t NULL)", dgrad(a), "null pointer");
    a = good(); a.dx = NULL;                  expect_einval("conv4s2_dgrad(dx NULL)", dgrad(a), "null pointer");
    a = good(); a.ws = NULL;                  expect_einval("conv4s2_dgrad(workspace NULL)", dgrad(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("conv4s2_dgrad(N = 0)", dgrad(a), "N (0)");
    a = good(); a.N = 4097;                   expect_einval("conv4s2_dgrad(N = 4097)", dgrad(a), "N (4097)");
    a = good(); a.H = 2;                      expect_einval("conv4s2_dgrad(H = 2)", dgrad(a), "H (2)");
    a = good(); a.C = 160;                    expect_einval("conv4s2_dgrad(C = 160)", dgrad(a), "C (160)");
    a = good(); a.ws_bytes = 4ll * 192 * 128 * 4 - 16;
                                              expect_einval("conv4s2_dgrad(workspace 16 bytes short)", dgrad(a), "workspace of");
    a = good(); a.dx = OFF(a.dx, 8);          expect_einval("conv4s2_dgrad(dx + 8 bytes)", dgrad(a), "16-byte aligned");
    /* ---- dxmi_gan_conv4s2_wgrad ------------------------------------------------------------------------------------ */
    a = good(); a.x = NULL;                   expect_einval("conv4s2_wgrad(x NULL)", wgrad(a), "null pointer");
    a = good(); a.dy = NULL;                  expect_einval("conv4s2_wgrad(dy NULL)", wgrad(a), "null pointer");
    a = good(); a.dw = NULL;                  expect_einval("conv4s2_wgrad(dw NULL)", wgrad(a), "null pointer");
    a = good(); a.db = NULL;                  expect_einval("conv4s2_wgrad(db NULL)", wgrad(a), "null pointer");
    a = good(); a.N = -1;                     expect_einval("conv4s2_wgrad(N < 0)", wgrad(a), "N (-1)");
    a = good(); a.H = 12;                     expect_einval("conv4s2_wgrad(H = 12)", wgrad(a), "H (12)");
    a = good(); a.C = 32;                     expect_einval("conv4s2_wgrad(C = 32)", wgrad(a), "C (32)");
    a = good(); a.dw = (float*)OFF(a.dw, 4);  expect_einval("conv4s2_wgrad(dw + 4 bytes)", wgrad(a), "16-byte aligned");
    /* ---- dxmi_gan_logit_loss_fwd / _bwd ---------------------------------------------------------------------------- */
    a = good(); a.x = NULL;                   expect_einval("logit_loss_fwd(a NULL)", lfwd(a), "null pointer");
    a = good(); a.w = NULL;                   expect_einval("logit_loss_fwd(w NULL)", lfwd(a), "null pointer");
    a = good(); a.bias = NULL;                expect_einval("logit_loss_fwd(b NULL)", lfwd(a), "null pointer");
    a = good(); a.sign = NULL;                expect_einval("logit_loss_fwd(sign NULL)", lfwd(a), "null pointer");
    a = good(); a.logit = NULL;               expect_einval("logit_loss_fwd(logit NULL)", lfwd(a), "null pointer");
    a = good(); a.loss = NULL;                expect_einval("logit_loss_fwd(loss NULL)", lfwd(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("logit_loss_fwd(N = 0)", lfwd(a), "N (0)");
    a = good(); a.N = 65536;                  expect_einval("logit_loss_fwd(N = 65536)", lfwd(a), "N (65536)");
    a = good(); a.C = 0;                      expect_einval("logit_loss_fwd(C = 0)", lfwd(a), "C (0)");
    a = good(); a.C = 100;                    expect_einval("logit_loss_fwd(C = 100)", lfwd(a), "C (100)");
    a = good(); a.x = NULL;                   expect_einval("logit_loss_bwd(a NULL)", lbwd(a), "null pointer");
    a = good(); a.sign = NULL;                expect_einval("logit_loss_bwd(sign NULL)", lbwd(a), "null pointer");
    a = good(); a.logit = NULL;               expect_einval("logit_loss_bwd(logit NULL)", lbwd(a), "null pointer");
    a = good(); a.up = NULL;                  expect_einval("logit_loss_bwd(upstream NULL)", lbwd(a), "null pointer");
    a = good(); a.d_a = NULL;                 expect_einval("logit_loss_bwd(d_a NULL)", lbwd(a), "null pointer");
    a = good(); a.N = -5;                     expect_einval("logit_loss_bwd(N < 0)", lbwd(a), "N (-5)");
    a = good(); a.C = 8192;                   expect_einval("logit_loss_bwd(C = 8192)", lbwd(a), "C (8192)");
    a = good(); a.weight = NAN;               expect_einval("logit_loss_bwd(weight NaN)", lbwd(a), "weight");
    a = good(); a.weight = INFINITY;          expect_einval("logit_loss_bwd(weight inf)", lbwd(a), "weight");
    /* ---- dxmi_gan_join --------------------------------------------------------------------------------------------- */
    a = good(); a.g = NULL;                   expect_einval("gan_join(g NULL)", join(a), "null pointer");
    a = good(); a.d_xin = NULL;               expect_einval("gan_join(d_xin NULL)", join(a), "null pointer");
    a = good(); a.idx = NULL;                 expect_einval("gan_join(indices NULL)", join(a), "null pointer");
    a = good(); a.tab = NULL;                 expect_einval("gan_join(t_table NULL)", join(a), "null pointer");
    a = good(); a.out = NULL;                 expect_einval("gan_join(out NULL)", join(a), "null pointer");
    a = good(); a.N = 0;                      expect_einval("gan_join(N = 0)", join(a), "N (0)");
    a = good(); a.N = 65536;                  expect_einval("gan_join(N = 65536)", join(a), "N (65536)");
    a = good(); a.CHW = 770;                  expect_einval("gan_join(CHW % 4 != 0)", join(a), "CHW (770)");
    a = good(); a.CHW = INT32_MAX - 3;        expect_einval("gan_join(CHW = 2^31 - 4)", join(a), "CHW (");
    a = good(); a.S = 0;                      expect_einval("gan_join(num_scales = 0)", join(a), "num_scales (0)");
    a = good(); a.weight = NAN;               expect_einval("gan_join(weight NaN)", join(a), "weight");
    a = good(); a.weight = -INFINITY;         expect_einval("gan_join(weight -inf)", join(a), "weight");
    a = good(); a.sd = 0.f;                   expect_einval("gan_join(sigma_data = 0)", join(a), "sigma_data");
    a = good(); a.sd = NAN;                   expect_einval("gan_join(sigma_data NaN)", join(a), "sigma_data");
    a = good(); a.g = (const float*)OFF(a.g, 4);
                                              expect_einval("gan_join(g + 4 bytes)", join(a), "16-byte aligned");
    a = good(); a.out = (float*)a.d_xin;      expect_einval("gan_join(out aliases d_xin)", join(a), "alias g only");
    /* ---- valid argument sets reach the launch: no device here, so a negative status that is not a crash ------------ */
    a = good();                               expect_negative("conv4s2_pack(valid, no device)", pack(a));
    a = good();                               expect_negative("conv4s2_fwd(valid, no device)", fwd(a));
    a = good(); a.bias = (const float*)OFF(a.bias, 4); a.x = OFF(a.x, 4);
                                              expect_negative("conv4s2_pack(valid, w at a 4-byte offset)", pack(a));
    a = good(); a.bias = (const float*)OFF(a.bias, 4);
                                              expect_negative("conv4s2_fwd(valid, bias at a 4-byte offset)", fwd(a));
    a = good(); a.bias = NULL; a.H = 4; a.C = 768; a.N = 33;
                                              expect_negative("conv4s2_fwd(valid, no bias, no device)", fwd(a));
    a = good();                               expect_negative("conv4s2_dgrad(valid, no device)", dgrad(a));
    a = good();                               expect_negative("conv4s2_wgrad(valid, no device)", wgrad(a));
    a = good();                               expect_negative("logit_loss_fwd(valid, no device)", lfwd(a));
    a = good();                               expect_negative("logit_loss_bwd(valid, no device)", lbwd(a));
    a = good(); a.dw = NULL; a.db = NULL;     expect_negative("logit_loss_bwd(valid, input only)", lbwd(a));
    a = good();                               expect_negative("gan_join(valid, no device)", join(a));
    a = good(); a.out = (float*)a.g;          expect_negative("gan_join(valid, out aliases g)", join(a));

    printf("%d failure(s)\n", failures);
    return failures > 99 ? 99 : failures;
}
