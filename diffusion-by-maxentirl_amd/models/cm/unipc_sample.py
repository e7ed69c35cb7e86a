"""Sample the EDM nets (models/cm/unet.py) with UniPC (Zhao et al. 2023, arXiv:2302.04867): the multistep data-prediction predictor
at orders 1-3 with the corrector UniC, ODE only, NFE = steps: the baseline the consistency-model and iCT tables put next to
DPM-Solver++ (models/cm/dpm_sample.py) at 10 network evaluations.

  EDMUniPCSchedule       one fp32 row per transition, noisiest first (columns ops.EUT_*, include/dxmi_hip.h), built once on the host
  edm_unipc_coefficients every per-transition scalar in float64 (the host tests' statement of the formulas)
  edm_unipc_transition   one transition as torch expressions on a row, in the operation order of dxmi_edm_unipc_stage
  edm_unipc_sample       the loop (models/DxMI/stage_loop.py): per transition one network evaluation and one dxmi_edm_unipc_stage launch

The EDM parametrisation of models/cm/dpm_sample.py (alpha = 1, sigma_t = sigma, lambda = -ln sigma, on edm_sigmas' ladder) and the
solver of models/DxMI/unipc_sample.py (unipc_coefficients, stated once in models/DxMI/dpm_sample.py): after evaluation k the
corrector re-does the step sigma_{k-1} -> sigma_k from the corrected state with D_k as one more node, and the predictor steps to
sigma_{k+1} from the result.  The preconditioning's scalars are EDMDPMSchedule's, the same bits for the same sigma.
"""
import numpy as np
import torch

from dxmi_hip import ops

from ..DxMI import stage_loop as _loop
from ..DxMI.dpm_sample import unipc_coefficients
from ..DxMI.unipc_sample import _check_mode, fill_unipc_columns, solver_update
from .dpm_sample import edm_sigmas
from .karras_diffusion import _memo, _refuse_distillation

EUT = {n[4:]: getattr(ops, n) for n in dir(ops) if n.startswith("EUT_")}


def edm_unipc_coefficients(sigmas, order=3, variant="bh1", corrector=True, lower_order_final=True):
    """unipc_coefficients of the EDM nets in float64, noisiest first, from `sigmas` as given (any float array, strictly decreasing,
    without a trailing zero): alpha = 1, lambda = -ln sigma."""
    sigma = np.asarray(sigmas, dtype=np.float64)
    return unipc_coefficients(np.ones_like(sigma), sigma, -np.log(sigma), order, variant, corrector, lower_order_final,
                              lambda k: f"edm_unipc_coefficients: sigma must fall from row {k} ({sigma[k]}) to row {k + 1} ({sigma[k + 1]})")


class EDMUniPCSchedule(_loop.StageSchedule):
    """table: fp32 [S, ops.EUT_COLS], row k = the transition sigma_k -> sigma_{k+1} (the last: -> 0): edm_unipc_coefficients on the
    fp32 ladder in float64, rounded once, and the preconditioning's scalars in fp32 torch as EDMDPMSchedule makes them.  The class
    attributes are what stage_loop asks of a schedule: the network is evaluated on x_in = c_in x and takes the labels y, the ring
    holds four predictions, and with the corrector the corrected state is carried."""
    sampler, hist_slots, x_in, net_keywords = "edm_unipc_sample", 4, True, ("y",)
    FIRST, STEP, T_COL = ops.EDM_UNIPC_FIRST, ops.EDM_UNIPC_STEP, ops.EUT_T

    @staticmethod
    def stage(mode, tab, t_out, eps=None, draw=0, seed=0, **kw):       # the solver adds no noise: no place for draw and seed
        ops.edm_unipc_stage(mode, tab, t_out, model_out=eps, **kw)

    def __init__(self, diffusion, steps=10, order=3, variant="bh1", corrector=True, skip_type="karras", lower_order_final=True,
                 clip_denoised=True, sigma_min=0.002, sigma_max=80.0, rho=7.0):
        _check_mode(order, variant)
        _refuse_distillation(diffusion)
        self.sigmas = sig = edm_sigmas(steps, sigma_min, sigma_max, rho, skip_type)
        self.steps = S = len(sig)
        self.order, self.variant, self.corrector, self.skip_type = int(order), variant, bool(corrector), skip_type
        self.lower_order_final, self.clip_denoised, self.sigma_data = bool(lower_order_final), bool(clip_denoised), diffusion.sigma_data
        self.carry = self.corrector
        self.coef = co = edm_unipc_coefficients(sig.numpy(), order, variant, corrector, lower_order_final)
        tab = torch.zeros((S, ops.EUT_COLS), dtype=torch.float32)
        for k in range(S):
            s = sig[k].reshape(1)
            c_skip, c_out, c_in = diffusion.get_scalings(s)
            tab[k, ops.EUT_SIGMA], tab[k, ops.EUT_CSKIP], tab[k, ops.EUT_COUT], tab[k, ops.EUT_CIN] = s[0], c_skip[0], c_out[0], c_in[0]
            tab[k, ops.EUT_T] = (1000 * 0.25 * torch.log(s + 1e-44))[0]         # denoise()'s time, as EDMDPMSchedule's ET_T
        tab[:-1, ops.EUT_T_NEXT], tab[:-1, ops.EUT_CIN_NEXT] = tab[1:, ops.EUT_T], tab[1:, ops.EUT_CIN]
        tab[:, ops.EUT_XSCALE] = sigma_max
        fill_unipc_columns(tab, co, EUT, self.clip_denoised)
        super().__init__(tab)
        self.draws, self.n_draws = [False] * S, 0

    def initial(self, x, row):
        return x * row[ops.EUT_XSCALE]

    def net_input(self, x, row):
        return row[ops.EUT_CIN] * x

    def step_info(self, k):
        return {"sigma": self.sigmas[k]}

    def transition(self, x, F, z, row, hist, xc=None):
        return edm_unipc_transition(x, F, row, hist, xc)[:3 if self.carry else 2]

    def graph_name(self, shape, mode):
        return f"edm_unipc_sample{(self.steps, self.order, self.variant, self.corrector, self.skip_type, tuple(shape), mode)}"


_SCHEDULES = {}


def edm_unipc_schedule(diffusion, steps=10, order=3, variant="bh1", corrector=True, skip_type="karras", lower_order_final=True,
                       clip_denoised=True, sigma_min=0.002, sigma_max=80.0, rho=7.0):
    """The (cached) EDMUniPCSchedule of these settings: one object per setting, so that a replay graph keyed on the table's
    identity is found again by the next call.  Of `diffusion` the table holds sigma_data alone."""
    _check_mode(order, variant)
    _refuse_distillation(diffusion)
    key = (float(diffusion.sigma_data), int(steps), int(order), variant, bool(corrector), skip_type, bool(lower_order_final),
           bool(clip_denoised), float(sigma_min), float(sigma_max), float(rho) if skip_type == "karras" else None)
    return _memo(_SCHEDULES, key, 32, lambda: EDMUniPCSchedule(diffusion, steps, order, variant, corrector, skip_type,
                                                               lower_order_final, clip_denoised, sigma_min, sigma_max, rho))


def edm_unipc_transition(x, F, row, hist=(), xc=None):
    """One transition on `row` (a table row, or its 20 coefficients in another dtype) as torch expressions in the operation order
    of dxmi_edm_unipc_stage -> (x', D0, xc').  F: the network's output at row[EUT_CIN] x; x: the predicted state; xc: the corrected
    state of the evaluation before, or None: the row then runs uncorrected, whatever its flags, and xc' = x."""
    d0 = row[ops.EUT_COUT] * F + row[ops.EUT_CSKIP] * x
    if int(row[ops.EUT_FLAGS]) & ops.EUT_FLAG_CLIP:
        d0 = d0.clamp(-1, 1)
    acc, b = solver_update(x, d0, row, hist, xc, EUT)
    return acc, d0, b


def replay_graphs(model):
    """The StepGraphs edm_unipc_sample holds for `model` (their .captures / .replays count what ran)."""
    return _loop.replay_graphs(model, EDMUniPCSchedule.sampler)


def edm_unipc_sample(diffusion, model, shape, steps=10, order=3, variant="bh1", corrector=True, skip_type="karras",
                     lower_order_final=True, clip_denoised=True, model_kwargs=None, device=None, sigma_min=0.002, sigma_max=80.0,
                     rho=7.0, generator=None, noise=None, callback=None, progress=False, use_graph=False):
    """Sample an EDM net with multistep UniPC: `steps` network evaluations (NFE = steps) on edm_sigmas(steps, sigma_min, sigma_max,
    rho, skip_type) -> clamp(x_0, -1, 1), [B, C, H, W].  order, variant, corrector and lower_order_final as
    models.DxMI.unipc_sample.unipc_sample.  diffusion: a KarrasDenoiser with distillation=False (a consistency-distilled model
    samples with onestep / multistep: refused).

    The contract of edm_dpm_sample.  model(x_in, t, **model_kwargs): the HIP UNetModel, or any callable; model_kwargs: the labels y
    alone.  On the device every transition is one network evaluation and one dxmi_edm_unipc_stage launch, which also writes the
    next evaluation's input; a CPU `device` with a torch callable runs the same expressions in torch, in float64 when noise[0] is
    float64.  noise: S + 1 entries of which only noise[0] (x_T before its scaling by sigma_max) is read.  callback({"i", "sigma",
    "x", "pred_xstart"}) after every transition (x: the predicted state).  generator: a models.cm.random_util generator; it gives
    x_T.  use_graph: capture ONE transition as a StepGraph and replay it for every later transition of every call with the same
    network, shape, device, table and labels' shape; the labels are a static buffer.  Off with callback, progress or noise=.  The
    returned tensor is then STATIC: the next call of the same key overwrites it."""
    sch = edm_unipc_schedule(diffusion, steps, order, variant, corrector, skip_type, lower_order_final, clip_denoised, sigma_min,
                             sigma_max, rho)
    return _loop.sample(sch, model, shape, device, generator, noise, callback, progress, use_graph, float64_state=True,
                        model_kwargs=model_kwargs)
