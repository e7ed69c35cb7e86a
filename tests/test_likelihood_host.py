"""Probability-flow likelihood on the host: the torch expressions of models/cm/likelihood.py and models/DxMI/likelihood.py against
closed forms (no GPU).

Analytic Gaussian: data N(0, s^2 I), s = 0.5, so D(x; sigma) = s^2 / (s^2 + sigma^2) x.  The Jacobian is diagonal, Rademacher
probes are exact and log p = log N(x_0; 0, (s^2 + sigma_min^2) I).  Heun is second order: halving the step divides the error by 4.
Measured in float64 (d = 768, 4 images, worst |bpd - exact|):
    EDM, sigma 0.002 .. 80, rho 7:   40 steps 0.0392, 80 steps 0.00990, 160 steps 0.00249   (ratios 3.96, 3.98)
    DDPM, uniform steps of T = 1000: 40 steps 0.0599, 80 steps 0.01289, 160 steps 0.00297, 320 steps 0.00072   (ratios 4.65, 4.34, 4.12)
The DDPM ladder is checked at 80 / 160 / 320: its first uniform step at 40 spans the integer steps 0 .. 24, over which sigma rises
from 0.01 to 0.13 and the drift's curvature is largest, so 40 steps are not yet in Heun's asymptotic regime (ratio 4.65); the integer
grid also stops being a refinement of itself beyond T / 3 steps.  The fp32 torch path repeats the float64 run's figures to 2 %
(per-image sums of 768 terms: an error of order 768 u of 1e4 nats, 1e-6 bits/dim), so it is held to the same two assertions."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffusion-by-maxentirl_amd")
S_DATA, D, SHAPE = 0.5, 768, (4, 3, 16, 16)


def diffusion(**kw):
    from models.cm.karras_diffusion import KarrasDenoiser
    return KarrasDenoiser(**dict(dict(sigma_data=0.5, sigma_max=80.0, sigma_min=0.002), **kw))


def edm_gaussian_net(x_in, t, s=S_DATA, sd=0.5):
    """F of the EDM parametrisation such that D = s^2 / (s^2 + sigma^2) x."""
    sig = torch.exp(t / 250.0).view(-1, 1, 1, 1)
    c_skip, c_out, c_in = sd ** 2 / (sig ** 2 + sd ** 2), sig * sd / (sig ** 2 + sd ** 2) ** 0.5, 1 / (sig ** 2 + sd ** 2) ** 0.5
    return (s * s / (s * s + sig ** 2) - c_skip) / c_out * (x_in / c_in)


@functools.lru_cache(maxsize=None)
def alpha_bar():
    from models.DxMI.var_sampler import calc_diffusion_hyperparams
    return calc_diffusion_hyperparams(1000, 1e-4, 0.02)["Alpha_bar"].to(torch.float32).double()


def ddpm_gaussian_net(x_t, t, s=S_DATA):
    """eps_theta = x^ sigma / (s^2 + sigma^2) evaluated from x_t at the integer step t."""
    ab = alpha_bar()[t.round().long()].view(-1, 1, 1, 1).to(x_t.dtype)
    sig = ((1 - ab) / ab).sqrt()
    return (x_t / ab.sqrt()) * sig / (s * s + sig ** 2)


def gaussian_bpd(x, var):
    logp = -0.5 * (x.double() ** 2).flatten(1).sum(1) / var - 0.5 * D * math.log(2 * math.pi * var)
    return logp, -logp / (D * math.log(2)) + 7


def second_order(errors):
    print("worst |bpd - exact|:", [f"{v:.5f}" for v in errors], "ratios", [f"{a / b:.3f}" for a, b in zip(errors, errors[1:])])
    assert all(3.5 <= a / b <= 4.5 for a, b in zip(errors, errors[1:])), errors
    assert errors[-1] <= 0.005, errors


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_analytic_gaussian_edm(dtype):
    from models.cm.likelihood import edm_log_likelihood
    smin = float(np.float32(0.002))
    var = S_DATA ** 2 + smin ** 2
    x0 = (torch.randn(SHAPE, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * math.sqrt(var)).to(dtype)
    _, exact = gaussian_bpd(x0, var)
    errors = []
    for steps in (40, 80, 160):
        r = edm_log_likelihood(diffusion(), edm_gaussian_net, x0, steps=steps)
        assert r["nfe"] == 2 * steps and r["bpd"].dtype == dtype and r["bpd"].shape == (4,)
        assert torch.allclose(r["logp"], r["prior_logp"] + r["delta_logp"])
        errors.append((r["bpd"].double() - exact).abs().max().item())
    second_order(errors)
    # the Jacobian is diagonal: every Rademacher probe gives the same value, a Gaussian probe does not
    a, b = (edm_log_likelihood(diffusion(), edm_gaussian_net, x0, steps=40)["bpd"] for _ in range(2))
    g = edm_log_likelihood(diffusion(), edm_gaussian_net, x0, steps=40, probe="gaussian")["bpd"]
    assert torch.allclose(a, b, rtol=0, atol=1e-4 if dtype == torch.float32 else 1e-10)
    assert (g.double() - a.double()).abs().min() > 1e-3


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_analytic_gaussian_ddpm(dtype):
    from models.DxMI.likelihood import ddpm_ll_schedule, ddpm_log_likelihood
    ab0 = alpha_bar()[0].item()
    var = S_DATA ** 2 + (1 - ab0) / ab0
    x0 = (torch.randn(SHAPE, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * math.sqrt(var * ab0)).to(dtype)
    logp_hat, _ = gaussian_bpd(x0.double() / math.sqrt(ab0), var)
    logp = logp_hat - 0.5 * D * math.log(ab0)              # logdet0: the state starts as x_0 / sqrt(alpha_bar_0)
    exact = -logp / (D * math.log(2)) + 7
    errors = []
    for steps in (80, 160, 320):
        r = ddpm_log_likelihood(ddpm_gaussian_net, x0, steps=steps, skip_type="uniform")
        assert r["nfe"] == 2 * steps and r["bpd"].dtype == dtype
        errors.append((r["bpd"].double() - exact).abs().max().item())
    second_order(errors)
    tau = ddpm_ll_schedule(D, 80, "uniform").tau
    assert tau[0] == 0 and tau[-1] == 999 and len(tau) == 81 and all(b > a for a, b in zip(tau, tau[1:]))
    tau = ddpm_ll_schedule(D, 20, "logsnr").tau
    assert tau[0] == 0 and tau[-1] == 999 and len(tau) == 21
    with pytest.raises(ValueError, match="uniform"):       # 41 logsnr nodes collide at the low-noise end: the message says what works
        ddpm_log_likelihood(ddpm_gaussian_net, x0, steps=40, skip_type="logsnr")


def test_correlated_gaussian_probe_mean_and_single_probe():
    """Dense covariance C (d = 12): D(x; sigma) = C (C + sigma^2 I)^-1 x, log p = log N(x_0; 0, C + sigma_min^2 I).  The mean over
    many Gaussian probes approaches the exact value within its standard error (plus the solver's and the prior's own error, taken
    from the run with the exact trace); one probe alone does not come within a tenth of the probes' spread: the negative control."""
    from models.cm.likelihood import edm_log_likelihood
    d, n_probe, steps = 12, 4096, 100
    gen = torch.Generator().manual_seed(5)
    A = torch.randn(d, d, dtype=torch.float64, generator=gen)
    C = A @ A.T / d * 0.25 + 0.05 * torch.eye(d, dtype=torch.float64)
    dif, sd = diffusion(sigma_min=0.01, sigma_max=5.0), 0.5
    eye = torch.eye(d, dtype=torch.float64)

    def net(x_in, t):
        sig = torch.exp(t / 250.0)[0].item()
        c_skip, c_out, c_in = sd ** 2 / (sig ** 2 + sd ** 2), sig * sd / math.sqrt(sig ** 2 + sd ** 2), 1 / math.sqrt(sig ** 2 + sd ** 2)
        M = (C @ torch.linalg.inv(C + sig ** 2 * eye) - c_skip * eye) / (c_out * c_in)
        return (x_in.reshape(len(x_in), d) @ M.T).reshape(x_in.shape)
    smin = float(np.float32(0.01))
    x = torch.linalg.cholesky(C + smin ** 2 * eye) @ torch.randn(d, dtype=torch.float64, generator=gen)
    cov = C + smin ** 2 * eye
    exact = float(-0.5 * x @ torch.linalg.solve(cov, x) - 0.5 * torch.logdet(2 * math.pi * cov))
    x0 = x.reshape(1, d, 1, 1).repeat(n_probe, 1, 1, 1)
    eps = torch.randn(x0.shape, dtype=torch.float64, generator=gen)
    logp = edm_log_likelihood(dif, net, x0, steps=steps, probe="gaussian", eps=eps)["logp"]
    # the solver's own error: the same run with the exact trace, E[e^T J e] = tr J, from d orthogonal probes sqrt(d) e_k averaged
    basis = (math.sqrt(d) * eye).reshape(d, d, 1, 1)
    solver = float(edm_log_likelihood(dif, net, x0[:d], steps=steps, probe="gaussian", eps=basis)["logp"].mean()) - exact
    mean, spread = float(logp.mean()), float(logp.std(unbiased=True))
    se = spread / math.sqrt(n_probe)
    print(f"exact {exact:.4f}, mean of {n_probe} probes {mean:.4f} (standard error {se:.4f}, spread {spread:.4f}), solver error {solver:.2e}")
    assert abs(mean - exact - solver) <= 4 * se and abs(solver) <= 0.05
    assert spread > 0.1 and abs(float(logp[0]) - exact) > 0.1 * spread


def test_table_columns_against_float64_closed_forms():
    from dxmi_hip import ops
    from models.cm.likelihood import edm_ll_nodes, edm_ll_schedule
    from models.DxMI.likelihood import ddpm_ll_schedule
    d, S = 3072, 7
    sch = edm_ll_schedule(diffusion(), d, S)
    s = edm_ll_nodes(S, 0.002, 80.0, 7.0)
    from models.cm.karras_diffusion import get_sigmas_karras
    assert np.array_equal(s.astype(np.float32), get_sigmas_karras(S + 1, 0.002, 80.0, 7.0)[:-1].flip(0).numpy()) and len(s) == S + 1
    assert sch.table.shape == (S, ops.PL_COLS) and sch.table.dtype == torch.float32 and sch.steps == S
    tab, sd = sch.table.double().numpy(), 0.5
    close = lambda col, want: np.testing.assert_allclose(tab[:, col], want, rtol=2.0 ** -23, atol=0)
    for cols, sg in (((ops.PL_T, ops.PL_CIN, ops.PL_KA, ops.PL_KB, ops.PL_DB, ops.PL_SIGMA), s[:-1]),
                     ((ops.PL_T_NEXT, ops.PL_CIN_NEXT, ops.PL_KA2, ops.PL_KB2, ops.PL_DB2, ops.PL_SIGMA_NEXT), s[1:])):
        c_skip, c_out, c_in = sd ** 2 / (sg ** 2 + sd ** 2), sg * sd / np.sqrt(sg ** 2 + sd ** 2), 1 / np.sqrt(sg ** 2 + sd ** 2)
        for col, want in zip(cols, (250 * np.log(sg), c_in, (1 - c_skip) / sg, -c_out / sg, -c_out * c_in / sg, sg)):
            close(col, want)
    close(ops.PL_H, s[1:] - s[:-1])
    close(ops.PL_HH, (s[1:] - s[:-1]) / 2)
    close(ops.PL_XSCALE, np.ones(S))
    assert (tab[:, ops.PL_LOGDET0] == 0).all()
    assert tab[:, ops.PL_FLAGS].tolist() == [0.0] * (S - 1) + [float(ops.PL_FLAG_LAST)]
    pv = s[-1] ** 2                  # sigma_max as the fp32 ladder holds it, the node the trajectory ends at
    assert abs(s[-1] / 80.0 - 1) < 1e-6
    close(ops.PL_PRIOR_Q, np.full(S, -0.5 / pv))
    close(ops.PL_PRIOR_C, np.full(S, -0.5 * d * math.log(2 * math.pi * pv)))
    close(ops.PL_BPD_SCALE, np.full(S, -1 / (d * math.log(2))))
    assert edm_ll_schedule(diffusion(), d, S) is sch and edm_ll_schedule(diffusion(), d + 1, S) is not sch

    sch = ddpm_ll_schedule(d, S, "logsnr")
    tab, tau = sch.table.double().numpy(), sch.tau
    ab = alpha_bar().numpy()[tau]
    sg = np.sqrt((1 - ab) / ab)
    close = lambda col, want: np.testing.assert_allclose(tab[:, col], want, rtol=2.0 ** -23, atol=0)
    assert tab[:, ops.PL_T].tolist() == [float(v) for v in tau[:-1]] and tab[:, ops.PL_T_NEXT].tolist() == [float(v) for v in tau[1:]]
    close(ops.PL_CIN, np.sqrt(ab[:-1]))
    close(ops.PL_CIN_NEXT, np.sqrt(ab[1:]))
    assert (tab[:, ops.PL_KA] == 0).all() and (tab[:, ops.PL_KA2] == 0).all() and (tab[:, ops.PL_KB] == 1).all() and (tab[:, ops.PL_KB2] == 1).all()
    close(ops.PL_DB, 1 / np.sqrt(1 + sg[:-1] ** 2))
    close(ops.PL_DB2, 1 / np.sqrt(1 + sg[1:] ** 2))
    close(ops.PL_H, sg[1:] - sg[:-1])
    close(ops.PL_HH, (sg[1:] - sg[:-1]) / 2)
    close(ops.PL_XSCALE, np.full(S, 1 / math.sqrt(ab[0])))
    close(ops.PL_LOGDET0, np.full(S, -0.5 * d * math.log(ab[0])))
    close(ops.PL_PRIOR_Q, np.full(S, -0.5 * ab[-1]))
    close(ops.PL_PRIOR_C, np.full(S, -0.5 * d * math.log(2 * math.pi / ab[-1])))
    close(ops.PL_BPD_SCALE, np.full(S, -1 / (d * math.log(2))))
    assert tab[:, ops.PL_FLAGS].tolist() == [0.0] * (S - 1) + [float(ops.PL_FLAG_LAST)]


def test_refusals():
    from dxmi_hip import DxmiError
    from models.cm.likelihood import edm_log_likelihood, make_probe
    from models.cm.random_util import DeterministicGenerator
    from models.DxMI.likelihood import ddpm_log_likelihood
    x0 = torch.zeros(2, 3, 4, 4)
    net = lambda x, t, **kw: x
    with pytest.raises(NotImplementedError, match="no probability-flow ODE drift"):
        edm_log_likelihood(diffusion(distillation=True), net, x0)
    with pytest.raises(ValueError, match="model_kwargs"):
        edm_log_likelihood(diffusion(), net, x0, model_kwargs={"y": None, "cond": 1})
    with pytest.raises(TypeError):
        edm_log_likelihood(diffusion(), net, x0, use_graph=True)            # not offered
    with pytest.raises(TypeError):
        ddpm_log_likelihood(net, x0, use_graph=True)
    for steps in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="steps"):
            edm_log_likelihood(diffusion(), net, x0, steps=steps)
        with pytest.raises(ValueError, match="steps"):
            ddpm_log_likelihood(net, x0, steps=steps, skip_type="uniform")
    with pytest.raises(ValueError, match="probe"):
        edm_log_likelihood(diffusion(), net, x0, steps=2, probe="sobol")
    with pytest.raises(ValueError, match="eps"):
        edm_log_likelihood(diffusion(), net, x0, steps=2, eps=torch.zeros(2, 3, 4, 5))
    with pytest.raises(ValueError, match="x0"):
        edm_log_likelihood(diffusion(), net, torch.zeros(4), steps=2)
    with pytest.raises(ValueError, match="sigma_min"):
        edm_log_likelihood(diffusion(), net, x0, steps=2, sigma_min=3.0, sigma_max=1.0)
    with pytest.raises(ValueError, match="skip_type"):
        ddpm_log_likelihood(net, x0, steps=4, skip_type="cosine")
    if not torch.cuda.is_available():      # the counter-based draws are made on the device only
        with pytest.raises(DxmiError):
            make_probe("rademacher", (2, 3, 4, 4), "cpu", DeterministicGenerator(4, 0))
    # a network whose output does not depend on its input has a zero Jacobian: the divergence is the analytic part alone
    r = edm_log_likelihood(diffusion(), lambda x, t: torch.ones_like(x).detach(), x0, steps=2)
    assert torch.isfinite(r["bpd"]).all()


def test_dequantisation():
    from models.cm.likelihood import dequantize_u8
    u8 = torch.arange(256, dtype=torch.uint8).repeat(2, 3, 4, 1)                       # every byte value
    c = dequantize_u8(u8, "center")
    assert c.dtype == torch.float32 and c.shape == u8.shape
    assert torch.equal(c.double(), (u8.double() + 0.5) / 128 - 1)                     # exact
    torch.manual_seed(3)
    x = dequantize_u8(u8.repeat(8, 1, 1, 1), "uniform")
    lo, hi = u8.repeat(8, 1, 1, 1).double() / 128 - 1, (u8.repeat(8, 1, 1, 1).double() + 1) / 128 - 1
    assert (x.double() >= lo).all() and (x.double() < hi).all()
    xi = (x.double() + 1) * 128 - u8.repeat(8, 1, 1, 1).double()                        # recovered exactly: multiples of 2^-16 in [0, 1)
    assert torch.equal(xi * 65536, (xi * 65536).round()) and 0.45 < float(xi.mean()) < 0.55 and float(xi.max()) > 0.99
    assert not torch.equal(x, dequantize_u8(u8.repeat(8, 1, 1, 1), "uniform"))
    with pytest.raises(ValueError):
        dequantize_u8(u8, "logit")
    with pytest.raises(ValueError):
        dequantize_u8(u8.float(), "center")


def test_eval_bpd_arguments():
    sys.path.insert(0, PKG) if PKG not in sys.path else None
    import eval_bpd
    a = eval_bpd.parse_args(["--data_npz", "t.npz", "--pretrained", "edm.pt"])
    assert (a.config, a.steps, a.rho, a.skip_type, a.batchsize, a.repeats, a.probe, a.dequantize, a.generator, a.seed, a.n_images) == \
        ("builtin:imagenet64_T10", 40, 7.0, None, 64, 1, "rademacher", "uniform", "determ", 0, None)
    a = eval_bpd.parse_args(["--data_npz", "t.npz", "--teacher_ckpt", "ema.pt", "--steps", "20", "--skip_type", "logsnr", "--n_images", "100",
                             "--repeats", "3", "--probe", "gaussian", "--dequantize", "center", "--generator", "dummy", "--seed", "9"])
    assert (a.config, a.steps, a.skip_type, a.rho, a.n_images, a.repeats, a.probe, a.dequantize, a.generator, a.seed) == \
        ("builtin:cifar10_T10", 20, "logsnr", None, 100, 3, "gaussian", "center", "dummy", 9)
    assert eval_bpd.parse_args(["--data_npz", "t.npz", "--teacher_ckpt", "ema.pt"]).skip_type == "uniform"
    for bad in (["--data_npz", "t.npz"], ["--data_npz", "t.npz", "--pretrained", "a", "--teacher_ckpt", "b"], ["--pretrained", "a"],
                ["--data_npz", "t.npz", "--pretrained", "a", "--skip_type", "uniform"], ["--data_npz", "t.npz", "--teacher_ckpt", "a", "--rho", "5"],
                ["--data_npz", "t.npz", "--pretrained", "a", "--steps", "0"], ["--data_npz", "t.npz", "--pretrained", "a", "--probe", "sobol"],
                ["--data_npz", "t.npz", "--pretrained", "a", "--use_graph"], ["--data_npz", "t.npz", "--pretrained", "a", "--repeats", "0"]):
        with pytest.raises(SystemExit):
            eval_bpd.parse_args(bad)
    assert "bits/dim: 3.2500 ± " in eval_bpd.summary(torch.tensor([3.0, 3.5]), 2, 80) and "over 2 images (2 repeats), NFE 80" in eval_bpd.summary(torch.tensor([3.0, 3.5]), 2, 80)


def test_eval_bpd_shard_and_gather_order_on_the_cpu(tmp_path):
    """12 images, batches of 5: one rank and two ranks score image i identically and bpd comes back in global-index order.  The
    analytic Gaussian net has a diagonal Jacobian, so the value does not depend on the Rademacher draw; center dequantisation."""
    import eval_bpd
    from dxmi_hip.data import ImageStore
    from models.cm.likelihood import dequantize_u8, edm_log_likelihood
    n = 12
    arr = torch.randint(0, 256, (n, 4, 4, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).numpy()
    path = os.path.join(tmp_path, "imgs.npz")
    np.savez(path, arr, np.arange(n, dtype=np.int64))
    store = ImageStore(path, "cpu", "adm", batch_size=1, random_flip=False, class_cond=True)
    u8, y = store.raw([3, 0, 11])
    assert u8.dtype == torch.uint8 and torch.equal(u8, torch.from_numpy(arr[[3, 0, 11]]).permute(0, 3, 1, 2)) and y.tolist() == [3, 0, 11]
    with pytest.raises(ValueError):
        store.raw([12])
    assert [r.tolist() for _, r in eval_bpd.shard_rows(12, 5, 0, 1)] == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11]]
    assert [r.tolist() for _, r in eval_bpd.shard_rows(12, 5, 1, 2)] == [[1, 3, 5, 7, 9], [11]]
    assert [d for d, _ in eval_bpd.shard_rows(12, 5, 1, 2)] == [0, 10]
    seen = []

    def score(x0, labels, g):
        seen.extend(labels.tolist())
        assert g is None
        return edm_log_likelihood(diffusion(), edm_gaussian_net, x0.double(), steps=4)["bpd"]
    kw = dict(repeats=2, dequantize="center", generator="dummy")
    one = eval_bpd.merge(n, [eval_bpd.score_rank(score, store.raw, n, 5, 0, 1, **kw)])
    assert seen == list(range(n)) * 2 and one.shape == (n, 2)
    two = eval_bpd.merge(n, [eval_bpd.score_rank(score, store.raw, n, 5, r, 2, **kw) for r in (1, 0)])
    x_all = dequantize_u8(torch.from_numpy(arr).permute(0, 3, 1, 2).contiguous(), "center")
    want = edm_log_likelihood(diffusion(), edm_gaussian_net, x_all.double(), steps=4)["bpd"].float()
    for got in (one, two):
        assert torch.allclose(got[:, 0], want, rtol=0, atol=1e-5) and torch.allclose(got[:, 1], want, rtol=0, atol=1e-5)
    with pytest.raises(RuntimeError, match="exactly once"):
        eval_bpd.merge(n, [eval_bpd.score_rank(score, store.raw, n, 5, 0, 2, **kw)])


def test_pf_ll_stage_arguments_under_address_and_ub_sanitizers():
    """`make asan_pf_ll` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_pf_ll.c, a program with its own main, against it and a no-device HIP runtime stub.  Null, misaligned,
    aliased and out-of-range arguments, no probe or two and a missing x_in must each come back as DXMI_EINVAL with the message of
    their check: no crash, no sanitizer report.  The program runs as a child process; nothing is loaded into python.  A host-only
    build: machines without a GPU only."""
    import shutil
    import subprocess
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_pf_ll"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_pf_ll")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") >= 60
