"""Sample the CIFAR-10 DDPM teacher with UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of
Diffusion Models", arXiv:2302.04867): the multistep data-prediction predictor UniP at orders 1-3 with the corrector UniC, ODE only,
the training-free baseline the consistency-model tables put next to DPM-Solver++ at 10 network evaluations.  The network, the
`Alpha_bar` table and the steps of models/DxMI/dpm_sample.py.

  unipc_timesteps      dpm_timesteps
  UniPCSchedule        one fp32 row per transition, noisiest first (columns ops.UT_*, include/dxmi_hip.h), built once on the host
  unipc_transition     one transition as torch expressions on a row, in the operation order of dxmi_unipc_stage
  unipc_sample         the loop (models/DxMI/stage_loop.py): per transition one network evaluation and one dxmi_unipc_stage launch

The formulas are stated once, in unipc_coefficients (models/DxMI/dpm_sample.py).  After evaluation k its data prediction D_k is
used twice: the corrector re-does the step that led to evaluation k, from the corrected state x_{k-1}, with D_k as one more node at
the end point (one order more than the predictor had), and the predictor takes the next step from that corrected x_k.  The network
sees the predicted states only, so NFE = steps: the corrector reuses the evaluation the next predictor needs anyway.  Two states
are carried: x (predicted, the network's input) and xc (corrected); the last row is the denoise row x' = D and has no corrector.
"""
import numpy as np
import torch

from dxmi_hip import ops

from . import stage_loop as _loop
from ..cm.karras_diffusion import _memo
from .dpm_sample import SKIP_TYPES, UNIPC_VARIANTS, dpm_timesteps, unipc_dpm_coefficients
from .var_sampler import calc_diffusion_hyperparams

unipc_timesteps = dpm_timesteps


def _check_mode(order, variant):
    if variant not in UNIPC_VARIANTS:
        raise ValueError(f"variant must be one of {UNIPC_VARIANTS}, got {variant!r}")
    if isinstance(order, bool) or int(order) != order or not 1 <= int(order) <= 3:
        raise ValueError(f"order must be 1, 2 or 3, got {order!r}")


def fill_unipc_columns(tab, co, cols, clip_denoised):
    """The solver's columns of a UniPC table (the DDPM teacher's or the EDM nets': `cols` is ops.UT_* or ops.EUT_* by name) from
    the float64 coefficients, rounded once, with the flags; asserts that a row reads exactly the history its two orders name."""
    S = len(co["order"])
    for name in ("cx", "w0", "w1", "w2", "ccx", "cv0", "cv1", "cv2", "cv3", "order"):
        tab[:, cols[name.upper()]] = torch.from_numpy(co[name].astype(np.float32))
    tab[:, cols["CORDER"]] = torch.from_numpy(co["corr_order"].astype(np.float32))
    tab[:, cols["FLAGS"]] = cols["FLAG_CLIP"] if clip_denoised else 0
    tab[-1, cols["FLAGS"]] += cols["FLAG_LAST"]
    tab[:, cols["FLAGS"]] += cols["FLAG_CORR"] * torch.from_numpy((co["corr_order"] > 0).astype(np.float32))
    assert tab[-1, cols["CX"]] == 0 and tab[-1, cols["W0"]] == 1 and co["corr_order"][-1] == 0 and co["corr_order"][0] == 0
    for k in range(S):
        p, q = int(co["order"][k]), int(co["corr_order"][k])
        assert [bool(tab[k, cols[c]] != 0) for c in ("W0", "W1", "W2")] == [j < p for j in range(3)], k
        assert [bool(tab[k, cols[c]] != 0) for c in ("CV0", "CV1", "CV2", "CV3")] == [q > 0 and j <= q for j in range(4)], k
        assert q <= k and p <= k + 1, k          # no row reads a prediction the run has not made


UT = {n[3:]: getattr(ops, n) for n in dir(ops) if n.startswith("UT_")}


class UniPCSchedule(_loop.StageSchedule):
    """table: fp32 [S, ops.UT_COLS], row k = the transition tau_{S-1-k} -> tau_{S-2-k}: unipc_dpm_coefficients on the fp32 Alpha_bar
    in float64, rounded once.  coef: the float64 coefficients.  The class attributes are what stage_loop asks of a schedule: a ring
    of four predictions, and with the corrector the carried corrected state (carry).  The solver draws x_T alone."""
    sampler, hist_slots = "unipc_sample", 4
    FIRST, STEP, T_COL = ops.UNIPC_FIRST, ops.UNIPC_STEP, ops.UT_T

    @staticmethod
    def stage(mode, tab, t_out, draw=0, seed=0, **kw):         # the solver adds no noise: the loop's draw and seed have no place
        ops.unipc_stage(mode, tab, t_out, **kw)

    def __init__(self, steps=10, order=3, variant="bh1", corrector=True, skip_type="logsnr", lower_order_final=True,
                 clip_denoised=True, T=1000, beta_0=1e-4, beta_T=0.02):
        _check_mode(order, variant)
        hp = calc_diffusion_hyperparams(int(T), beta_0, beta_T)
        alpha_bar = hp["Alpha_bar"].to(torch.float32).numpy()
        self.tau = unipc_timesteps(steps, T, skip_type, beta_0, beta_T)
        self.steps, self.T = len(self.tau), int(T)
        self.order, self.variant, self.corrector, self.skip_type = int(order), variant, bool(corrector), skip_type
        self.lower_order_final, self.clip_denoised = bool(lower_order_final), bool(clip_denoised)
        self.carry = self.corrector
        self.coef = co = unipc_dpm_coefficients(alpha_bar, self.tau, order, variant, corrector, lower_order_final)
        tab = torch.zeros((self.steps, ops.UT_COLS), dtype=torch.float32)
        times = torch.tensor(self.tau[::-1], dtype=torch.float32)
        tab[:, ops.UT_T] = times
        tab[:-1, ops.UT_T_NEXT] = times[1:]
        tab[:, ops.UT_A], tab[:, ops.UT_B] = (torch.from_numpy(co[k].astype(np.float32)) for k in ("a", "b"))
        fill_unipc_columns(tab, co, UT, self.clip_denoised)
        super().__init__(tab)
        self.draws, self.n_draws = [False] * self.steps, 0

    def transition(self, x, eps, z, row, hist, xc=None):
        return unipc_transition(x, eps, row, hist, xc)[:3 if self.carry else 2]

    def graph_name(self, shape, mode):
        return f"unipc_sample{(self.steps, self.order, self.variant, self.corrector, tuple(shape), mode)}"


_SCHEDULES = {}


def unipc_sample_schedule(steps=10, order=3, variant="bh1", corrector=True, skip_type="logsnr", lower_order_final=True,
                          clip_denoised=True, T=1000, beta_0=1e-4, beta_T=0.02):
    """The (cached) UniPCSchedule of these settings: one object per setting, so that a replay graph keyed on the table's identity
    is found again by the next call."""
    _check_mode(order, variant)
    key = (int(steps), int(order), variant, bool(corrector), skip_type, bool(lower_order_final), bool(clip_denoised), int(T),
           float(beta_0), float(beta_T))
    return _memo(_SCHEDULES, key, 32, lambda: UniPCSchedule(steps, order, variant, corrector, skip_type, lower_order_final,
                                                            clip_denoised, T, beta_0, beta_T))


def solver_update(x, d0, row, hist, xc, cols):
    """Steps 2 and 3 of the launches' element on `row` (columns by name: ops.UT_* or ops.EUT_*) -> (x', b): the corrector on a row
    flagged CORR when a corrected state is given (b = the corrected state, else b = x), then the predictor from b.  hist: (D_{k-1},
    D_{k-2}, D_{k-3}) as far as the row's weights are not 0 (a zero weight reads nothing)."""
    b = x
    if xc is not None and int(row[cols["FLAGS"]]) & cols["FLAG_CORR"]:
        b = row[cols["CCX"]] * xc
        b = b + row[cols["CV0"]] * d0
        b = b + row[cols["CV1"]] * hist[0]
        for j, c in ((1, "CV2"), (2, "CV3")):
            if float(row[cols[c]]) != 0.0:
                b = b + row[cols[c]] * hist[j]
    acc = row[cols["CX"]] * b + row[cols["W0"]] * d0
    for j, c in enumerate(("W1", "W2")):
        if float(row[cols[c]]) != 0.0:
            acc = acc + row[cols[c]] * hist[j]
    return acc, b


def unipc_transition(x, eps, row, hist=(), xc=None):
    """One transition on `row` (a table row, or its 16 coefficients in another dtype) as torch expressions in the operation order
    of dxmi_unipc_stage -> (x', D0, xc').  x: the predicted state the network saw; xc: the corrected state of the evaluation
    before, or None: the row then runs uncorrected, whatever its flags, and xc' = x."""
    d0 = row[ops.UT_A] * x - row[ops.UT_B] * eps
    if int(row[ops.UT_FLAGS]) & ops.UT_FLAG_CLIP:
        d0 = d0.clamp(-1, 1)
    acc, b = solver_update(x, d0, row, hist, xc, UT)
    return acc, d0, b


def replay_graphs(net):
    """The StepGraphs unipc_sample holds for `net` (their .captures / .replays count what ran)."""
    return _loop.replay_graphs(net, UniPCSchedule.sampler)


def unipc_sample(net, shape, steps=10, order=3, variant="bh1", corrector=True, skip_type="logsnr", lower_order_final=True,
                 clip_denoised=True, device=None, generator=None, noise=None, callback=None, progress=False, use_graph=False, T=1000,
                 beta_0=1e-4, beta_T=0.02):
    """Sample the DDPM teacher with multistep UniPC: `steps` network evaluations on unipc_timesteps(steps, T, skip_type) ->
    clamp(x_0, -1, 1), [B, C, H, W].  order 1-3: the predictor's; the corrector of a step has one order more.  variant "bh1"
    (B(h) = h) or "bh2" (B(h) = 1 - e^-h): they differ where the paper fixes rho = 1/2, the order-1 corrector and the order-2
    predictor.  corrector=False runs the predictor UniP alone (with bh2 and order <= 2: DPM-Solver++ 2M).  lower_order_final lowers
    the order of the last rows so that the last transition is first order.  The defaults are the official unconditional settings.

    The contract of dpm_sample.  net: the HIP Model (bare or under .module), or any callable net(x, t_float [B]) -> eps.  On the
    device every transition is one network evaluation and one dxmi_unipc_stage launch; a CPU `device` with a callable runs the same
    expressions in torch, in float64 when noise[0] is float64.  noise: S + 1 entries of which only noise[0], x_T, is read (the
    solver adds no noise); nothing is drawn then.  callback({"i", "t", "x", "pred_xstart"}) after every transition (x: the
    predicted state, what the network sees next; before the final clamp).  generator: a models.cm.random_util generator; it gives
    x_T.  use_graph: capture ONE transition as a StepGraph and replay it for every later transition of every call with the same
    network, shape, device and table; the predictions and the corrected state live in static buffers.  Off with callback, progress
    or noise=.  The returned tensor is then STATIC: the next call of the same key overwrites it."""
    if skip_type not in SKIP_TYPES:
        raise ValueError(f"unipc_sample: skip_type must be one of {SKIP_TYPES}, got {skip_type!r}")
    sch = unipc_sample_schedule(steps, order, variant, corrector, skip_type, lower_order_final, clip_denoised, T, beta_0, beta_T)
    return _loop.sample(sch, net, shape, device, generator, noise, callback, progress, use_graph, float64_state=True)
