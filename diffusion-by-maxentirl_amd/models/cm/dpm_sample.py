"""Sample the EDM nets (models/cm/unet.py) with DPM-Solver++ (Lu et al. 2022, arXiv:2211.01095): the multistep data-prediction
solver at orders 1-3 and its SDE variant at orders 1-2, the training-free baseline at a given number of network evaluations that
karras_sample's Heun (2 S - 1 evaluations), DPM-2 (2 S) and Euler (first order) cannot give.  NFE = steps.

  edm_sigmas             the ladder sigma_0 = sigma_max > ... > sigma_{S-1} = sigma_min a run evaluates at, fp32
  edm_dpm_coefficients   every per-transition scalar in float64 (the host tests' statement of the formulas)
  EDMDPMSchedule         one fp32 row per transition, noisiest first (columns ops.ET_*, include/dxmi_hip.h), built once on the host
  edm_dpm_transition     one transition as torch expressions on a row, in the operation order of dxmi_edm_dpm_stage
  edm_dpm_sample         the loop (models/DxMI/stage_loop.py): per transition one network evaluation and one dxmi_edm_dpm_stage launch

The EDM parametrisation is x = x_0 + sigma e: alpha = 1, sigma_t = sigma, lambda = -ln sigma, and the solver is
models/DxMI/dpm_sample.py's (multistep_coefficients, stated there once) on these three.  A run makes S evaluations and has S rows.
Row k < S - 1 goes from sigma_k to sigma_{k+1}, h = ln(sigma_k / sigma_{k+1}) > 0; row S - 1 goes to sigma = 0.  Evaluation k is
F = model(c_in(sigma_k) x, 250 ln(sigma_k + 1e-44), **model_kwargs) and gives the data prediction D_k = c_out(sigma_k) F +
c_skip(sigma_k) x, clamped to [-1, 1] with clip_denoised.  With alpha_p = 1:
    ODE  "dpmsolver++"      x' = (sigma_p / sigma_t) x + sum_j w_j D_{k-j}
    SDE  "sde-dpmsolver++"  x' = (sigma_p / sigma_t) e^-h x + sum_j w_j D_{k-j} + sigma_p sqrt(1 - e^-2h) z         (orders 1-2)
    the last row: x' = D (cx = 0, w_0 = 1, no noise); the run returns clamp(x', -1, 1).
The coefficients are computed in float64 from the fp32 ladder, the values the network's sigma is computed from, and rounded to fp32
once; the preconditioning's scalars are fp32 torch, KarrasSchedule's expressions (the same bits for the same sigma).  Order 1 of the
ODE on the karras ladder is sample_euler's map: cx + w0 = 1, cx = sigma_p / sigma_t.
"""
import numpy as np
import torch

from dxmi_hip import ops

from ..DxMI import stage_loop as _loop
from ..DxMI.dpm_sample import _check_mode, multistep_coefficients
from .karras_diffusion import _memo, _refuse_distillation, get_sigmas_karras

SKIP_TYPES = ("karras", "logsnr")


# ------------------------------------------------------------------------------------------------- host schedule
def edm_sigmas(steps, sigma_min=0.002, sigma_max=80.0, rho=7.0, skip_type="karras"):
    """The S = steps noise levels of a run, fp32 [S], strictly decreasing from fp32(sigma_max) to fp32(sigma_min).  karras:
    get_sigmas_karras(S, ...) without its trailing zero (the reference's fp32 values: sample_euler's ladder); logsnr:
    exp(linspace(ln sigma_max, ln sigma_min, S)) in float64, rounded to fp32, the two ends set exactly.  uniform / quad are the
    DDPM teacher's spacings of an integer time, which the EDM nets do not have: refused by name."""
    S = int(steps)
    if skip_type in ("uniform", "quad"):
        raise ValueError(f"edm_sigmas: skip_type {skip_type!r} spaces the integer time of the DDPM teacher (models/DxMI/dpm_sample.py); "
                         f"the EDM nets have none: use one of {SKIP_TYPES}")
    if skip_type not in SKIP_TYPES:
        raise ValueError(f"edm_sigmas: skip_type must be one of {SKIP_TYPES}, got {skip_type!r}")
    if S < 2:
        raise ValueError(f"edm_sigmas: at least 2 steps, got {steps}")
    if not 0 < sigma_min < sigma_max:
        raise ValueError(f"edm_sigmas: 0 < sigma_min < sigma_max, got {sigma_min}, {sigma_max}")
    if skip_type == "karras":
        sigmas = get_sigmas_karras(S, sigma_min, sigma_max, rho)[:-1].to(torch.float32)
    else:
        ladder = np.exp(np.linspace(np.log(float(sigma_max)), np.log(float(sigma_min)), S)).astype(np.float32)
        ladder[0], ladder[-1] = np.float32(sigma_max), np.float32(sigma_min)
        sigmas = torch.from_numpy(ladder)
    if not bool((sigmas[1:] < sigmas[:-1]).all()):
        raise ValueError(f"edm_sigmas: {S} {skip_type} steps from {sigma_max} to {sigma_min} are not strictly decreasing in fp32")
    return sigmas


def edm_dpm_coefficients(sigmas, algorithm="dpmsolver++", order=2, solver_type="midpoint", lower_order_final=True):
    """The scalars of every transition in float64, noisiest first, from `sigmas` as given (any float array, strictly decreasing,
    without a trailing zero): a dict of arrays cx, w0, w1, w2, s and order (int64).  A weight beyond a row's order is exactly 0."""
    _check_mode(algorithm, order, solver_type)
    sigma = np.asarray(sigmas, dtype=np.float64)
    return multistep_coefficients(np.ones_like(sigma), sigma, -np.log(sigma), algorithm, order, solver_type, lower_order_final,
                                  lambda k: f"edm_dpm_coefficients: sigma must fall from row {k} ({sigma[k]}) to row {k + 1} ({sigma[k + 1]})")


class EDMDPMSchedule(_loop.StageSchedule):
    """table: fp32 [S, ops.ET_COLS], row k = the transition sigma_k -> sigma_{k+1} (the last: -> 0): edm_dpm_coefficients on the
    fp32 ladder in float64, rounded once, and the preconditioning's scalars in fp32 torch as KarrasSchedule makes them.  sigmas:
    the fp32 ladder; draws[k]: whether transition k adds noise; coef: the float64 coefficients.  The class attributes are what
    stage_loop asks of a schedule: the network is evaluated on x_in = c_in x, which FIRST and every launch but the last write, and
    takes the labels y."""
    sampler, hist_slots, x_in, net_keywords = "edm_dpm_sample", 3, True, ("y",)
    FIRST, STEP, T_COL = ops.EDM_DPM_FIRST, ops.EDM_DPM_STEP, ops.ET_T

    @staticmethod
    def stage(mode, tab, t_out, eps=None, **kw):
        ops.edm_dpm_stage(mode, tab, t_out, model_out=eps, **kw)

    def __init__(self, diffusion, steps=10, order=2, algorithm="dpmsolver++", solver_type="midpoint", skip_type="karras",
                 lower_order_final=True, clip_denoised=True, sigma_min=0.002, sigma_max=80.0, rho=7.0):
        _check_mode(algorithm, order, solver_type)
        _refuse_distillation(diffusion)
        self.sigmas = sig = edm_sigmas(steps, sigma_min, sigma_max, rho, skip_type)
        self.steps = S = len(sig)
        self.order, self.algorithm, self.solver_type, self.skip_type = int(order), algorithm, solver_type, skip_type
        self.lower_order_final, self.clip_denoised, self.sigma_data = bool(lower_order_final), bool(clip_denoised), diffusion.sigma_data
        self.coef = co = edm_dpm_coefficients(sig.numpy(), algorithm, order, solver_type, lower_order_final)
        tab = torch.zeros((S, ops.ET_COLS), dtype=torch.float32)
        for col, k in ((ops.ET_CX, "cx"), (ops.ET_W0, "w0"), (ops.ET_W1, "w1"), (ops.ET_W2, "w2"), (ops.ET_S, "s"), (ops.ET_ORDER, "order")):
            tab[:, col] = torch.from_numpy(co[k].astype(np.float32))
        for k in range(S):
            s = sig[k].reshape(1)
            c_skip, c_out, c_in = diffusion.get_scalings(s)
            tab[k, ops.ET_SIGMA], tab[k, ops.ET_CSKIP], tab[k, ops.ET_COUT], tab[k, ops.ET_CIN] = s[0], c_skip[0], c_out[0], c_in[0]
            tab[k, ops.ET_T] = (1000 * 0.25 * torch.log(s + 1e-44))[0]          # denoise()'s time, as KarrasSchedule's KT_T
        tab[:-1, ops.ET_T_NEXT], tab[:-1, ops.ET_CIN_NEXT] = tab[1:, ops.ET_T], tab[1:, ops.ET_CIN]
        tab[:, ops.ET_XSCALE] = sigma_max
        tab[:, ops.ET_FLAGS] = ops.ET_FLAG_CLIP if self.clip_denoised else 0
        tab[-1, ops.ET_FLAGS] += ops.ET_FLAG_LAST
        assert tab[-1, ops.ET_S] == 0 and tab[-1, ops.ET_CX] == 0 and tab[-1, ops.ET_W0] == 1
        # a row reads exactly the history its order names: rows 0 and 1 and the lowered rows never touch an unwritten slot
        for k in range(S):
            assert (tab[k, ops.ET_W1] != 0) == (co["order"][k] >= 2) and (tab[k, ops.ET_W2] != 0) == (co["order"][k] >= 3), k
        super().__init__(tab)
        self.draws = [bool(v != 0) for v in tab[:, ops.ET_S]]
        self.n_draws = sum(self.draws)

    def initial(self, x, row):
        return x * row[ops.ET_XSCALE]

    def net_input(self, x, row):
        return row[ops.ET_CIN] * x

    def step_info(self, k):
        return {"sigma": self.sigmas[k]}

    def transition(self, x, F, z, row, hist):
        return edm_dpm_transition(x, F, z, row, hist)

    def graph_name(self, shape, mode):
        return f"edm_dpm_sample{(self.steps, self.order, self.algorithm, self.skip_type, tuple(shape), mode)}"


_SCHEDULES = {}


def edm_dpm_schedule(diffusion, steps=10, order=2, algorithm="dpmsolver++", solver_type="midpoint", skip_type="karras",
                     lower_order_final=True, clip_denoised=True, sigma_min=0.002, sigma_max=80.0, rho=7.0):
    """The (cached) EDMDPMSchedule of these settings: one object per setting, so that a replay graph keyed on the table's identity
    is found again by the next call.  Of `diffusion` the table holds sigma_data alone."""
    _check_mode(algorithm, order, solver_type)
    _refuse_distillation(diffusion)
    key = (float(diffusion.sigma_data), int(steps), int(order), algorithm, solver_type, skip_type, bool(lower_order_final),
           bool(clip_denoised), float(sigma_min), float(sigma_max), float(rho) if skip_type == "karras" else None)
    return _memo(_SCHEDULES, key, 32, lambda: EDMDPMSchedule(diffusion, steps, order, algorithm, solver_type, skip_type,
                                                             lower_order_final, clip_denoised, sigma_min, sigma_max, rho))


def edm_dpm_transition(x, F, z, row, hist=()):
    """One transition on `row` (a table row, or 16 coefficients of another dtype in its layout) as torch expressions in the
    operation order of dxmi_edm_dpm_stage -> (x', D0).  F: the network's output at row[ET_CIN] x; hist: (D_{k-1}, D_{k-2}) as far
    as the row's weights are not 0 (a zero weight reads nothing).  z None or row[ET_S] == 0: no noise is added."""
    d0 = row[ops.ET_COUT] * F + row[ops.ET_CSKIP] * x
    if int(row[ops.ET_FLAGS]) & ops.ET_FLAG_CLIP:
        d0 = d0.clamp(-1, 1)
    acc = row[ops.ET_CX] * x + row[ops.ET_W0] * d0
    for j, col in enumerate((ops.ET_W1, ops.ET_W2)):
        if float(row[col]) != 0.0:
            acc = acc + row[col] * hist[j]
    if z is not None and float(row[ops.ET_S]) != 0.0:
        acc = acc + row[ops.ET_S] * z
    return acc, d0


def replay_graphs(model):
    """The StepGraphs edm_dpm_sample holds for `model` (their .captures / .replays count what ran)."""
    return _loop.replay_graphs(model, EDMDPMSchedule.sampler)


def edm_dpm_sample(diffusion, model, shape, steps=10, order=2, algorithm="dpmsolver++", solver_type="midpoint", skip_type="karras",
                   lower_order_final=True, clip_denoised=True, model_kwargs=None, device=None, sigma_min=0.002, sigma_max=80.0,
                   rho=7.0, generator=None, noise=None, callback=None, progress=False, use_graph=False):
    """Sample an EDM net with multistep DPM-Solver++: `steps` network evaluations (NFE = steps) on edm_sigmas(steps, sigma_min,
    sigma_max, rho, skip_type) -> clamp(x_0, -1, 1), [B, C, H, W].  algorithm "dpmsolver++" (the ODE solver, orders 1-3) or
    "sde-dpmsolver++" (orders 1-2); solver_type "midpoint" or "exact" (the Lagrange weights) for the second-order rows;
    lower_order_final lowers the order of the last rows so that the last transition is first order.  diffusion: a KarrasDenoiser
    with distillation=False (a consistency-distilled model samples with onestep / multistep: refused).

    The contract of models.DxMI.dpm_sample.dpm_sample.  model(x_in, t, **model_kwargs): the HIP UNetModel, or any callable;
    model_kwargs: the labels y alone.  On the device every transition is one network evaluation and one dxmi_edm_dpm_stage launch,
    which also writes the next evaluation's input; a CPU `device` with a torch callable runs the same expressions in torch, in
    float64 when noise[0] is float64.  noise: S + 1 recorded draws (x_T before its scaling by sigma_max, then one per transition;
    those of transitions that add no noise are not read).  callback({"i", "sigma", "x", "pred_xstart"}) after every transition.
    generator: a models.cm.random_util generator.  None / dummy: torch's device generator.  determ / determ-indiv: x_T is
    generator.randn and every noisy transition's z is made inside its launch; generator.draw ends advanced by the draws made.
    use_graph: capture ONE transition as a StepGraph and replay it for every later transition of every call with the same
    network, shape, device, table, noise source and labels' shape; the labels are a static buffer.  Off with callback, progress or
    noise=.  The returned tensor is then STATIC: the next call of the same key overwrites it."""
    sch = edm_dpm_schedule(diffusion, steps, order, algorithm, solver_type, skip_type, lower_order_final, clip_denoised, sigma_min,
                           sigma_max, rho)
    return _loop.sample(sch, model, shape, device, generator, noise, callback, progress, use_graph, float64_state=True,
                        model_kwargs=model_kwargs)
