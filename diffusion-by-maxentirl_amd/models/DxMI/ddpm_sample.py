"""Sample the CIFAR-10 DDPM teacher as a teacher: ancestral sampling (Ho et al. 2020, "Denoising Diffusion Probabilistic Models",
Algorithm 2), DDIM (Song et al. 2021, "Denoising Diffusion Implicit Models", eq. 12 and 16) and strided schedules between them,
on the noise-prediction network train_ddpm.py trains and the `Alpha_bar` table VARSampler is built on
(models/DxMI/var_sampler.py calc_diffusion_hyperparams; no second formula for the table).

  ddpm_timesteps       the integer steps tau_0 = 0 < ... < tau_{S-1} < T a run visits (uniform or quadratic spacing)
  ddpm_coefficients    every per-transition scalar in float64 (the host tests' statement of the formulas)
  DDPMSampleSchedule   one fp32 row per transition, noisiest first (columns ops.DT_*, include/dxmi_hip.h), built once on the host,
                       uploaded once per device.  Everything that differs from one transition to the next lives in the row, the
                       last-step behaviour included, so ONE captured step serves all of them.
  ddpm_transition      one transition as torch expressions on a row (the CPU path and the tests' float64 path)
  ddpm_sample          the loop (models/DxMI/stage_loop.py): per transition one network evaluation and one dxmi_ddpm_stage launch

One transition goes from t = tau_k to p = tau_{k-1}; a_t = Alpha_bar[t], a_p = Alpha_bar[p], a_p = 1 for the last one.
    sigma = eta sqrt((1 - a_p) / (1 - a_t)) sqrt(1 - a_t / a_p)                       eta in [0, 1]: 0 DDIM, 1 ancestral
    variance "small": the noise scale s = sigma.  "large" (Ho et al.'s fixedlarge, eta = 1 only): the mean of eta = 1 and
    s = sqrt(1 - a_t / a_p), which is sqrt(beta_t) between adjacent steps.  s = 0 on the last transition in both.
    clip_denoised (Ho et al.):  x0 = x / sqrt(a_t) - sqrt(1 / a_t - 1) eps;  x0c = clamp(x0, -1, 1);
                                eps_hat = (x - sqrt(a_t) x0c) / sqrt(1 - a_t);  x' = sqrt(a_p) x0c + sqrt(1 - a_p - sigma^2) eps_hat + s z
    otherwise the linear form   x' = xm x + (c eps + s z),  (xm, c, sigma) = _step_tables(Alpha_bar[tau], eta): the association of
                                the reference's VAR_sampling (models/DxMI/var_sampler.py:262-285).
The run starts from x_T ~ N(0, I) and returns clamp(x_0, -1, 1).
"""
import math

import numpy as np
import torch

from dxmi_hip import ops

from . import stage_loop as _loop
from ..cm.karras_diffusion import _memo
from .var_sampler import _step_tables, calc_diffusion_hyperparams

SKIP_TYPES = ("uniform", "quad")
VARIANCES = ("small", "large")


# ------------------------------------------------------------------------------------------------- host schedule
def _timestep_sequence(S, T, skip_type):
    if skip_type == "uniform":
        return [(i * T) // S for i in range(S)]
    return [int((i * math.sqrt(0.8 * T) / (S - 1)) ** 2) for i in range(S)]


def _timesteps_ok(S, T, skip_type):
    if S < 1 or S > T or (skip_type == "quad" and S < 2):
        return False
    tau = _timestep_sequence(S, T, skip_type)
    return tau[0] == 0 and tau[-1] < T and all(b > a for a, b in zip(tau, tau[1:]))


def ddpm_timesteps(S, T=1000, skip_type="uniform"):
    """The S steps of a run, increasing, tau_0 == 0.  uniform: tau_i = (i T) // S (range(0, T, T // S) when S divides T);
    quad: tau_i = int((i sqrt(0.8 T) / (S - 1))^2), S >= 2.  ValueError for S outside [1, T] and for a sequence that is not strictly
    increasing (quad with too many steps); the message names the largest S that works."""
    S, T = int(S), int(T)
    if skip_type not in SKIP_TYPES:
        raise ValueError(f"ddpm_timesteps: skip_type must be one of {SKIP_TYPES}, got {skip_type!r}")
    if T < 1:
        raise ValueError(f"ddpm_timesteps: T must be at least 1, got {T}")
    if not _timesteps_ok(S, T, skip_type):
        largest = max((n for n in range(T, 0, -1) if _timesteps_ok(n, T, skip_type)), default=None)
        low = 2 if skip_type == "quad" else 1
        raise ValueError(f"ddpm_timesteps: {S} {skip_type} steps do not give {low} <= S <= T = {T} strictly increasing steps; "
                         f"the largest S that works is {largest}")
    return _timestep_sequence(S, T, skip_type)


def _check_mode(eta, variance):
    if variance not in VARIANCES:
        raise ValueError(f"variance must be one of {VARIANCES}, got {variance!r}")
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta must lie in [0, 1], got {eta}")
    if variance == "large" and float(eta) != 1.0:
        raise ValueError(f"variance='large' is the ancestral sampler's fixedlarge variance: it needs eta == 1.0, got {eta}")


def ddpm_coefficients(alpha_bar, tau, eta=1.0, variance="small", beta=None):
    """The scalars of every transition in float64, noisiest first, from `alpha_bar` as given (any float array): a dict of arrays
    sigma, s, a, b, q, r, c0, c1 (the clip form), xm, c (the linear form).  beta: the table alpha_bar is the running product of;
    with it, variance 'large' takes s = sqrt(beta[t]) between ADJACENT steps (p == t - 1): the quotient of two rounded running
    products gives 1 - a_t / a_p only to their rounding error over beta_t, ~1e-4 relative in fp32."""
    _check_mode(eta, variance)
    ab = np.asarray(alpha_bar, dtype=np.float64)
    t = np.asarray(list(tau)[::-1], dtype=np.int64)
    a_t = ab[t]
    a_p = np.concatenate([ab[t[1:]], [1.0]])
    step = 1.0 - a_t / a_p
    sigma = (1.0 if variance == "large" else float(eta)) * np.sqrt((1.0 - a_p) / (1.0 - a_t)) * np.sqrt(step)
    if variance == "large":
        if beta is not None:
            adjacent = np.concatenate([t[:-1] - t[1:] == 1, [False]])
            step = np.where(adjacent, np.asarray(beta, dtype=np.float64)[t], step)
        s = np.sqrt(step)
    else:
        s = sigma.copy()
    s[-1] = 0.0
    c0, c1 = np.sqrt(a_p), np.sqrt(1.0 - a_p - sigma ** 2)
    xm = np.sqrt(a_p / a_t)
    return {"sigma": sigma, "s": s, "a": 1.0 / np.sqrt(a_t), "b": np.sqrt(1.0 / a_t - 1.0), "q": np.sqrt(a_t),
            "r": 1.0 / np.sqrt(1.0 - a_t), "c0": c0, "c1": c1, "xm": xm, "c": c1 - np.sqrt(1.0 - a_t) * xm}


class DDPMSampleSchedule(_loop.StageSchedule):
    """table: fp32 [S, ops.DT_COLS], row k = the transition tau_{S-1-k} -> tau_{S-2-k}.  The linear-form columns (XM, C, and S for
    variance 'small' without clipping) are _step_tables' scalar fp32 values; the clip-form columns, and S otherwise, are computed
    in float64 from the fp32 Alpha_bar and rounded once.  draws[k]: whether transition k adds noise (S != 0).  The class
    attributes are what stage_loop asks of a schedule."""
    sampler, hist_slots = "ddpm_sample", 0
    stage, FIRST, STEP, T_COL = staticmethod(ops.ddpm_stage), ops.DDPM_FIRST, ops.DDPM_STEP, ops.DT_T

    def __init__(self, steps=1000, eta=1.0, variance="small", skip_type="uniform", clip_denoised=True, T=1000, beta_0=1e-4,
                 beta_T=0.02):
        _check_mode(eta, variance)
        hp = calc_diffusion_hyperparams(int(T), beta_0, beta_T)
        alpha_bar = hp["Alpha_bar"].to(torch.float32)
        self.tau = ddpm_timesteps(steps, T, skip_type)
        self.steps, self.T = len(self.tau), int(T)
        self.eta, self.variance, self.skip_type, self.clip_denoised = float(eta), variance, skip_type, bool(clip_denoised)
        xm, c, sigma = _step_tables(alpha_bar[self.tau], 1.0 if variance == "large" else float(eta))
        co = ddpm_coefficients(alpha_bar.numpy(), self.tau, eta, variance, beta=hp["Beta"].to(torch.float32).numpy())
        S = self.steps
        tab = np.zeros((S, ops.DT_COLS), dtype=np.float32)
        times = np.asarray(self.tau[::-1], dtype=np.float32)
        tab[:, ops.DT_T] = times
        tab[:-1, ops.DT_T_NEXT] = times[1:]
        tab[:, ops.DT_XM], tab[:, ops.DT_C] = xm.numpy(), c.numpy()
        tab[:, ops.DT_S] = sigma.numpy() if (variance == "small" and not self.clip_denoised) else co["s"].astype(np.float32)
        for col, k in ((ops.DT_A, "a"), (ops.DT_B, "b"), (ops.DT_Q, "q"), (ops.DT_R, "r"), (ops.DT_C0, "c0"), (ops.DT_C1, "c1")):
            tab[:, col] = co[k].astype(np.float32)
        tab[:, ops.DT_FLAGS] = ops.DT_FLAG_CLIP if self.clip_denoised else 0
        tab[-1, ops.DT_FLAGS] += ops.DT_FLAG_LAST
        assert tab[-1, ops.DT_S] == 0 and tab[-1, ops.DT_C0] == 1
        super().__init__(torch.from_numpy(tab))
        self.draws = [bool(v != 0) for v in tab[:, ops.DT_S]]
        self.n_draws = sum(self.draws)

    def transition(self, x, eps, z, row, hist):
        return ddpm_transition(x, eps, z, row)

    def graph_name(self, shape, mode):
        return f"ddpm_sample{(self.steps, tuple(shape), mode)}"


_SCHEDULES = {}


def ddpm_sample_schedule(steps=1000, eta=1.0, variance="small", skip_type="uniform", clip_denoised=True, T=1000, beta_0=1e-4,
                         beta_T=0.02):
    """The (cached) DDPMSampleSchedule of these settings: one object per setting, so that a replay graph keyed on the table's
    identity is found again by the next call."""
    key = (int(steps), float(eta), variance, skip_type, bool(clip_denoised), int(T), float(beta_0), float(beta_T))
    return _memo(_SCHEDULES, key, 32, lambda: DDPMSampleSchedule(steps, eta, variance, skip_type, clip_denoised, T, beta_0, beta_T))


def ddpm_transition(x, eps, z, row):
    """One transition on `row` (a table row, or 16 coefficients of another dtype in its layout) as torch expressions in the
    operation order of dxmi_ddpm_stage -> (x', pred_xstart).  z None or row[DT_S] == 0: no noise is added.  (The launch forms the
    linear form's control + s z as one fused multiply-add, as dxmi_var_step_fwd does; here s z is rounded on its own.)"""
    s = row[ops.DT_S]
    noisy = z is not None and float(s) != 0.0
    x0 = row[ops.DT_A] * x - row[ops.DT_B] * eps
    if int(row[ops.DT_FLAGS]) & ops.DT_FLAG_CLIP:
        x0c = x0.clamp(-1, 1)
        eps_hat = (x - row[ops.DT_Q] * x0c) * row[ops.DT_R]
        mean = row[ops.DT_C0] * x0c + row[ops.DT_C1] * eps_hat
        return (mean + s * z if noisy else mean), x0c
    xs, control = row[ops.DT_XM] * x, row[ops.DT_C] * eps
    return (xs + (control + s * z) if noisy else xs + control), x0


def replay_graphs(net):
    """The StepGraphs ddpm_sample holds for `net` (their .captures / .replays count what ran)."""
    return _loop.replay_graphs(net, DDPMSampleSchedule.sampler)


def ddpm_sample(net, shape, steps=1000, eta=1.0, variance="small", skip_type="uniform", clip_denoised=True, device=None,
                generator=None, noise=None, callback=None, progress=False, use_graph=False, T=1000, beta_0=1e-4, beta_T=0.02):
    """Sample the DDPM teacher: `steps` transitions on ddpm_timesteps(steps, T, skip_type) -> clamp(x_0, -1, 1), [B, C, H, W].

    net: the HIP Model (bare or under .module), or any callable net(x, t_float [B]) -> eps.  On the device every transition is one
    network evaluation and one dxmi_ddpm_stage launch; a CPU `device` with a callable runs the same expressions in torch.
    noise: S + 1 recorded draws (x_T, then one per transition; those of transitions that add no noise are not read); nothing is
    drawn then.  callback({"i", "t", "x", "pred_xstart"}) after every transition (x: the new state, before the final clamp).
    generator: a models.cm.random_util generator.  None / dummy: torch's device generator.  determ / determ-indiv: x_T is
    generator.randn and every transition's z is made inside the stage launch from (generator.seed, generator.get_indices(B, device),
    draw number, element): bit for bit what generator.randn_like draws fed through noise= give, and generator.draw ends advanced by
    the draws made.  Only transitions whose noise scale is not 0 draw: eta = 0 draws x_T alone.
    use_graph: capture ONE transition as a StepGraph and replay it for every later transition of every call with the same network,
    shape, device, table and noise source (a key's first transition runs eagerly, its second is captured).  Off with callback,
    progress or noise=; ON with the deterministic generators (the fused draw needs no host-made tensor).  With torch's generator the
    captured step draws z in every transition, the last one's unused.  The returned tensor is then STATIC: the next call of the same
    key overwrites it."""
    sch = ddpm_sample_schedule(steps, eta, variance, skip_type, clip_denoised, T, beta_0, beta_T)
    return _loop.sample(sch, net, shape, device, generator, noise, callback, progress, use_graph, float64_state=False)
