"""The DDPM teacher's samplers on the host (models/DxMI/ddpm_sample.py): the steps, the table, the formulas in float64 against Ho et
al.'s posterior form, the torch path against the reference's VAR_sampling (tests/golden/ddpm_sample.npz), the draw count, the
refusals and the parser errors of generate_cifar10.py.  No GPU.

Golden tolerance: the reference's Gamma_bar is a running product and differs from Alpha_bar[tau] in the last bits, and sqrt / pow may
differ by one ulp between CPUs, so the agreement is a tolerance.  Measured on the build machine: the largest |difference| between
the torch path (clip_denoised=False, noise= the recorded draws) and the golden trajectories is 1.5258789e-05 (two ulps of values
near 90: nothing clips, so the states grow); the bound is 8 times that."""
import os

import numpy as np
import pytest
import torch

from dxmi_hip import ops
from models.DxMI.ddpm_sample import (DDPMSampleSchedule, ddpm_coefficients, ddpm_sample, ddpm_timesteps, ddpm_transition)
from models.DxMI.var_sampler import _step_tables, calc_diffusion_hyperparams

GOLDEN_MEASURED = 1.5258789e-05
GOLDEN_BOUND = 8 * GOLDEN_MEASURED


def analytic_net(x, t):
    return 0.8 * torch.tanh(0.9 * x + 1e-3 * t[:, None, None, None])


# ------------------------------------------------------------------------------------------ steps
@pytest.mark.parametrize("S", [1, 10, 50, 1000])
def test_uniform_steps(S):
    assert ddpm_timesteps(S) == list(range(0, 1000, 1000 // S))
    assert ddpm_timesteps(S, 1000, "uniform") == ddpm_timesteps(S)


def test_uniform_steps_when_S_does_not_divide_T():
    tau = ddpm_timesteps(6)
    assert tau == [0, 166, 333, 500, 666, 833]
    tau = ddpm_timesteps(7, T=20)
    assert tau[0] == 0 and tau[-1] < 20 and all(b > a for a, b in zip(tau, tau[1:])) and len(tau) == 7


@pytest.mark.parametrize("S", [2, 10, 29])
def test_quad_steps(S):
    tau = ddpm_timesteps(S, 1000, "quad")
    assert len(tau) == S and tau[0] == 0 and tau[-1] in (799, 800) and all(isinstance(t, int) for t in tau)
    assert all(b > a for a, b in zip(tau, tau[1:]))
    assert tau == [int((i * np.sqrt(0.8 * 1000) / (S - 1)) ** 2) for i in range(S)]
    gaps = np.diff(tau)
    assert S < 3 or gaps[-1] > gaps[0]           # dense near 0, sparse near T


def test_step_refusals():
    with pytest.raises(ValueError, match="largest S that works is 1000"):
        ddpm_timesteps(0)
    with pytest.raises(ValueError, match="largest S that works is 1000"):
        ddpm_timesteps(1001)
    with pytest.raises(ValueError, match="largest S that works is 29"):
        ddpm_timesteps(200, 1000, "quad")
    with pytest.raises(ValueError):
        ddpm_timesteps(1, 1000, "quad")
    with pytest.raises(ValueError):
        ddpm_timesteps(10, 1000, "cosine")
    assert len(ddpm_timesteps(29, 1000, "quad")) == 29
    with pytest.raises(ValueError):
        ddpm_timesteps(30, 1000, "quad")


# ------------------------------------------------------------------------------------------ the table
def ulps(got, want64):
    want = np.asarray(want64, dtype=np.float64)
    w32 = want.astype(np.float32)
    return np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(w32)).astype(np.float64)


@pytest.mark.parametrize("steps,eta,skip", [(10, 0.0, "uniform"), (10, 0.5, "uniform"), (50, 1.0, "uniform"), (1000, 1.0, "uniform"),
                                            (20, 0.3, "quad")])
def test_linear_rows_are_step_tables(steps, eta, skip):
    sch = DDPMSampleSchedule(steps, eta, "small", skip, clip_denoised=False)
    abar = calc_diffusion_hyperparams(1000, 1e-4, 0.02)["Alpha_bar"]
    xm, c, sigma = _step_tables(abar[sch.tau], eta)
    tab = sch.table
    assert tab.dtype == torch.float32 and tab.shape == (steps, ops.DT_COLS)
    assert torch.equal(tab[:, ops.DT_XM], xm) and torch.equal(tab[:, ops.DT_C], c) and torch.equal(tab[:, ops.DT_S], sigma)
    assert tab[:, ops.DT_T].tolist() == [float(t) for t in sch.tau[::-1]]
    assert tab[:-1, ops.DT_T_NEXT].tolist() == tab[1:, ops.DT_T].tolist()
    assert (tab[:, ops.DT_FLAGS] == torch.tensor([0.0] * (steps - 1) + [float(ops.DT_FLAG_LAST)])).all()
    assert sch.draws == [eta != 0.0] * (steps - 1) + [False] and sch.n_draws == (steps - 1) * (eta != 0.0)


@pytest.mark.parametrize("steps,eta,variance", [(10, 0.0, "small"), (7, 0.5, "small"), (50, 1.0, "small"), (13, 1.0, "large")])
def test_clip_coefficients_within_one_ulp_of_float64(steps, eta, variance):
    sch = DDPMSampleSchedule(steps, eta, variance, clip_denoised=True)
    abar = calc_diffusion_hyperparams(1000, 1e-4, 0.02)["Alpha_bar"].double().numpy()      # the fp32 table, widened
    t = sch.tau[::-1]
    a_t = abar[t]
    a_p = np.array([abar[p] for p in t[1:]] + [1.0])
    sig1 = np.sqrt((1 - a_p) / (1 - a_t)) * np.sqrt(1 - a_t / a_p)
    sigma = sig1 if variance == "large" else eta * sig1
    s = np.sqrt(1 - a_t / a_p) if variance == "large" else sigma.copy()
    s[-1] = 0
    want = {ops.DT_A: 1 / np.sqrt(a_t), ops.DT_B: np.sqrt(1 / a_t - 1), ops.DT_Q: np.sqrt(a_t), ops.DT_R: 1 / np.sqrt(1 - a_t),
            ops.DT_C0: np.sqrt(a_p), ops.DT_C1: np.sqrt(1 - a_p - sigma ** 2), ops.DT_S: s}
    tab = sch.table.numpy()
    for col, w in want.items():
        nz = w != 0
        assert (tab[:, col][~nz] == 0).all()
        assert (ulps(tab[:, col][nz], w[nz]) <= 1).all(), (col, ulps(tab[:, col][nz], w[nz]).max())
    assert (tab[:, ops.DT_FLAGS] == np.array([1.0] * (steps - 1) + [3.0])).all()


def test_large_variance_on_the_full_sequence_is_sqrt_beta():
    sch = DDPMSampleSchedule(1000, 1.0, "large")
    beta = calc_diffusion_hyperparams(1000, 1e-4, 0.02)["Beta"].double().numpy()
    s = sch.table[:, ops.DT_S].numpy()
    want = np.sqrt(beta)[::-1]
    assert (ulps(s[:-1], want[:-1]) <= 1).all()
    assert s[-1] == 0


@pytest.mark.parametrize("kw", [dict(), dict(eta=0.0), dict(variance="large"), dict(clip_denoised=False), dict(skip_type="quad", steps=9)])
def test_last_row(kw):
    sch = DDPMSampleSchedule(**dict(dict(steps=10), **kw))
    last = sch.table[-1]
    assert last[ops.DT_C0] == 1 and last[ops.DT_S] == 0 and int(last[ops.DT_FLAGS]) & ops.DT_FLAG_LAST
    assert last[ops.DT_T] == 0 and not sch.draws[-1]
    assert not any(int(f) & ops.DT_FLAG_LAST for f in sch.table[:-1, ops.DT_FLAGS])


# ------------------------------------------------------------------------------------------ the formulas in float64
def rows64(co, clip):
    n = len(co["s"])
    tab = torch.zeros(n, ops.DT_COLS, dtype=torch.float64)
    for col, k in ((ops.DT_XM, "xm"), (ops.DT_C, "c"), (ops.DT_S, "s"), (ops.DT_A, "a"), (ops.DT_B, "b"), (ops.DT_Q, "q"),
                   (ops.DT_R, "r"), (ops.DT_C0, "c0"), (ops.DT_C1, "c1")):
        tab[:, col] = torch.from_numpy(co[k])
    tab[:, ops.DT_FLAGS] = ops.DT_FLAG_CLIP if clip else 0
    tab[-1, ops.DT_FLAGS] += ops.DT_FLAG_LAST
    return tab


def small_table(T=20):
    beta = np.linspace(1e-4, 0.3, T)
    return beta, np.cumprod(1 - beta)


def test_ancestral_clip_form_is_ho_posterior():
    """eta = 1, variance small, clip_denoised: x' = coef1 x0c + coef2 x_t + sqrt(beta_tilde) z (Ho et al. 2020, eq. 6-7)."""
    T = 20
    beta, abar = small_table(T)
    tab = rows64(ddpm_coefficients(abar, range(T), 1.0, "small"), clip=True)
    gen = torch.Generator().manual_seed(3)
    worst = 0.0
    for k in range(T):
        t = T - 1 - k
        x = 1.5 * torch.randn(5, 3, 4, 4, dtype=torch.float64, generator=gen)
        eps = 1.2 * torch.randn(5, 3, 4, 4, dtype=torch.float64, generator=gen)
        z = torch.randn(5, 3, 4, 4, dtype=torch.float64, generator=gen)
        got, pred = ddpm_transition(x, eps, z, tab[k])
        a_prev = abar[t - 1] if t > 0 else 1.0
        x0c = (x / np.sqrt(abar[t]) - np.sqrt(1 / abar[t] - 1) * eps).clamp(-1, 1)
        assert (x0c.abs() == 1).any() and (x0c.abs() < 1).any()            # both branches of the clamp
        coef1 = beta[t] * np.sqrt(a_prev) / (1 - abar[t])
        coef2 = (1 - a_prev) * np.sqrt(1 - beta[t]) / (1 - abar[t])
        var = beta[t] * (1 - a_prev) / (1 - abar[t])
        want = coef1 * x0c + coef2 * x + (np.sqrt(var) * z if t > 0 else 0)
        worst = max(worst, (got - want).abs().max().item())
        assert (pred - x0c).abs().max() <= 1e-12          # x / sqrt(a) here, x * (1 / sqrt(a)) there
    print(f"clip form vs Ho's posterior: worst |difference| {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("eta,variance", [(0.0, "small"), (0.5, "small"), (1.0, "small"), (1.0, "large")])
def test_clip_form_is_linear_form_where_nothing_clips(eta, variance):
    T = 20
    beta, abar = small_table(T)
    tau = [0, 3, 4, 9, 15, 19]
    co = ddpm_coefficients(abar, tau, eta, variance, beta=beta)
    clip, lin = rows64(co, True), rows64(co, False)
    gen = torch.Generator().manual_seed(4)
    worst = 0.0
    for k, t in enumerate(tau[::-1]):
        x0 = torch.rand(5, 3, 4, 4, dtype=torch.float64, generator=gen) - 0.5
        e = torch.randn(5, 3, 4, 4, dtype=torch.float64, generator=gen)
        x = np.sqrt(abar[t]) * x0 + np.sqrt(1 - abar[t]) * e
        eps = e + 0.01 * torch.randn(5, 3, 4, 4, dtype=torch.float64, generator=gen)
        z = torch.randn(5, 3, 4, 4, dtype=torch.float64, generator=gen)
        a, pa = ddpm_transition(x, eps, z, clip[k])
        b, pb = ddpm_transition(x, eps, z, lin[k])
        assert pa.abs().max() < 1 and torch.equal(pa, pb)
        worst = max(worst, (a - b).abs().max().item())
    assert worst <= 1e-12, worst


# ------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("kappa", ["0.0", "0.5", "1.0"])
def test_torch_path_against_reference_var_sampling(golden_dir, kappa):
    g = np.load(os.path.join(golden_dir, "ddpm_sample.npz"))
    S = len(g["tau"])
    assert list(g["tau"]) == ddpm_timesteps(S)
    assert np.array_equal(g["alpha_bar"], calc_diffusion_hyperparams(1000, 1e-4, 0.02)["Alpha_bar"].numpy())
    assert np.abs(g["gamma_bar"] - g["alpha_bar"][g["tau"]]).max() <= 2e-7       # the running product follows the table to the last bits
    draws = [torch.from_numpy(d) for d in g[f"k{kappa}.draws"]]
    seen = []
    out = ddpm_sample(analytic_net, draws[0].shape, steps=S, eta=float(kappa), clip_denoised=False, device="cpu", noise=draws,
                      callback=lambda d: seen.append((d["i"], d["t"], d["x"].clone())))
    assert [i for i, _, _ in seen] == list(range(S)) and [t for _, t, _ in seen] == list(g["tau"][::-1])
    got = torch.stack([x for _, _, x in seen]).numpy()
    # the reference adds 0.001 z after its last step: its last mean stands for x_0
    want = np.concatenate([g[f"k{kappa}.x_seq"][1:S], g[f"k{kappa}.pred_mean"][-1:]])
    diff = np.abs(got - want).max()
    print(f"kappa {kappa}: torch path vs VAR_sampling, largest |difference| {diff:.7e} (bound {GOLDEN_BOUND:.7e}, measured "
          f"{GOLDEN_MEASURED:.7e})")
    assert diff <= GOLDEN_BOUND
    assert torch.equal(out, torch.from_numpy(got[-1]).clamp(-1, 1))


# ------------------------------------------------------------------------------------------ draws and refusals
class CountingGenerator:
    def __init__(self):
        self.randn_calls = self.randn_like_calls = 0
        self.gen = torch.Generator().manual_seed(11)

    def randn(self, *size, device=None, dtype=torch.float32):
        self.randn_calls += 1
        return torch.randn(*size, generator=self.gen)

    def randn_like(self, x):
        self.randn_like_calls += 1
        return torch.randn(x.shape, generator=self.gen)


def test_eta_zero_draws_x_T_alone():
    g = CountingGenerator()
    out = ddpm_sample(analytic_net, (2, 3, 8, 8), steps=5, eta=0.0, device="cpu", generator=g)
    assert (g.randn_calls, g.randn_like_calls) == (1, 0) and out.shape == (2, 3, 8, 8) and out.abs().max() <= 1
    g = CountingGenerator()
    ddpm_sample(analytic_net, (2, 3, 8, 8), steps=5, eta=1.0, device="cpu", generator=g)
    assert (g.randn_calls, g.randn_like_calls) == (1, 4)          # the last transition adds no noise


def test_recorded_noise_reproduces_a_generator_run():
    g = CountingGenerator()
    a = ddpm_sample(analytic_net, (2, 3, 8, 8), steps=4, eta=0.7, device="cpu", generator=g)
    gen = torch.Generator().manual_seed(11)
    noise = [torch.randn(2, 3, 8, 8, generator=gen) for _ in range(4)] + [torch.full((2, 3, 8, 8), float("nan"))]
    b = ddpm_sample(analytic_net, (2, 3, 8, 8), steps=4, eta=0.7, device="cpu", noise=noise)
    assert torch.equal(a, b)                                       # and the last entry of noise= is never read


def test_refusals():
    with pytest.raises(ValueError, match="5 draws"):
        ddpm_sample(analytic_net, (2, 3, 8, 8), steps=4, device="cpu", noise=[torch.zeros(2, 3, 8, 8)] * 4)
    with pytest.raises(ValueError, match="eta == 1.0"):
        ddpm_sample(analytic_net, (2, 3, 8, 8), steps=4, eta=0.5, variance="large", device="cpu")
    with pytest.raises(ValueError):
        DDPMSampleSchedule(10, 0.5, "large")
    with pytest.raises(ValueError):
        DDPMSampleSchedule(10, 1.5)
    with pytest.raises(ValueError):
        DDPMSampleSchedule(10, 1.0, "learned")
    with pytest.raises(ValueError):
        ddpm_sample(analytic_net, (2, 3, 8, 8), steps=2000, device="cpu")


def test_hip_model_is_refused_on_the_cpu():
    from dxmi_hip import DxmiError
    from models.DxMI.unet_small import Model
    net = Model(ch=32, out_ch=3, ch_mult=(1,), num_res_blocks=1, attn_resolutions=[], dropout=0.0, in_channels=3, resolution=8)
    with pytest.raises(DxmiError):
        ddpm_sample(net, (1, 3, 8, 8), steps=2, device="cpu")


# ------------------------------------------------------------------------------------------ command line
def test_generate_cifar10_parser():
    import generate_cifar10 as gc
    args = gc.parse_args(["--log_dir", "x", "--teacher_ckpt", "ema.pt"])
    assert (args.ddpm_steps, args.eta, args.variance, args.skip_type, args.no_clip, args.generator, args.config) == \
        (1000, 1.0, "small", "uniform", False, "dummy", None)
    args = gc.parse_args(["--log_dir", "x", "--teacher_ckpt", "ema.pt", "--ddpm_steps", "50", "--eta", "0", "--skip_type", "quad",
                          "--no_clip", "--generator", "determ", "--config", "builtin:cifar10_T10", "--variance", "small"])
    assert (args.ddpm_steps, args.eta, args.skip_type, args.no_clip, args.generator, args.config) == \
        (50, 0.0, "quad", True, "determ", "builtin:cifar10_T10")
    args = gc.parse_args(["--log_dir", "x", "--synthetic", "cifar10_T10"])          # today's call: untouched
    assert args.teacher_ckpt is None and args.synthetic == "cifar10_T10" and args.generator is None
    for flags in (["--ddpm_steps", "50"], ["--eta", "0.5"], ["--variance", "large"], ["--skip_type", "quad"], ["--no_clip"],
                  ["--generator", "determ"], ["--config", "builtin:cifar10_T10"]):
        with pytest.raises(SystemExit):
            gc.parse_args(["--log_dir", "x"] + flags)
    with pytest.raises(SystemExit):
        gc.parse_args(["--log_dir", "x", "--teacher_ckpt", "ema.pt", "--guidance_scale", "1.0"])
    with pytest.raises(SystemExit):
        gc.parse_args(["--log_dir", "x", "--teacher_ckpt", "ema.pt", "--variance", "large", "--eta", "0.5"])
    assert gc.parse_args(["--log_dir", "x", "--teacher_ckpt", "ema.pt", "--variance", "large"]).eta == 1.0
