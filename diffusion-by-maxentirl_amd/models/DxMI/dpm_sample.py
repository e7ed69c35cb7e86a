"""Sample the CIFAR-10 DDPM teacher with DPM-Solver++ (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion
Probabilistic Models", arXiv:2211.01095): the multistep data-prediction solver (Algorithm 2) at orders 1-3 and its SDE variant at
orders 1-2, the training-free baseline a 10-step or 4-step DxMI sampler is measured against.  The same network and the same
`Alpha_bar` table as models/DxMI/ddpm_sample.py (calc_diffusion_hyperparams; no second formula for the table).

  dpm_timesteps        the integer steps tau_0 = 0 < ... < tau_{S-1} a run visits: linear in the log-SNR, uniform or quadratic
  dpm_coefficients     every per-transition scalar in float64 (the host tests' statement of the formulas)
  DPMSampleSchedule    one fp32 row per transition, noisiest first (columns ops.MT_*, include/dxmi_hip.h), built once on the host
  dpm_transition       one transition as torch expressions on a row, in the operation order of dxmi_dpm_stage
  dpm_sample           the loop (models/DxMI/stage_loop.py): per transition one network evaluation and one dxmi_dpm_stage launch

ab = Alpha_bar (the fp32 table read into float64), alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log alpha - log sigma.  A run
makes S evaluations and has S rows.  Row k < S - 1 goes from t = tau_{S-1-k} to p = tau_{S-2-k}, h = lambda_p - lambda_t > 0; row
S - 1 goes from tau_0 to alpha_p = 1, sigma_p = 0.  Evaluation k gives the data prediction D_k = x / alpha_t - (sigma_t / alpha_t)
eps, clamped to [-1, 1] with clip_denoised.  With o_k = min(order, k + 1), with lower_order_final also min(o_k, S - k), and L_j the
Lagrange basis polynomial on the o_k nodes lambda of evaluations k, k - 1, ...:
    ODE  "dpmsolver++"      x' = (sigma_p / sigma_t) x + sum_j w_j D_{k-j}
         exact     w_j = sigma_p int_{lambda_t}^{lambda_p} e^lambda L_j dlambda       (order 1: alpha_p (1 - e^-h))
         midpoint  order-2 rows: w_0 = alpha_p (1 - e^-h)(1 + 1 / (2r)), w_1 = -alpha_p (1 - e^-h) / (2r), r = (lambda_t - lambda_prev) / h
    SDE  "sde-dpmsolver++"  x' = (sigma_p / sigma_t) e^-h x + sum_j w_j D_{k-j} + sigma_p sqrt(1 - e^-2h) z         (orders 1-2)
         exact     w_j = 2 alpha_p int_{lambda_t}^{lambda_p} e^{-2 (lambda_p - lambda)} L_j dlambda
         midpoint  order-2 rows: the ODE's with 1 - e^-2h in place of 1 - e^-h
    the last row: x' = D (cx = 0, w_0 = 1, no noise); the run returns clamp(x', -1, 1).
With v = lambda_p - lambda both integrals are alpha_p times sums of the moments M_n(h) = int_0^h e^-v v^n dv (the SDE's of 2h),
evaluated by their series below h = 1 (no cancellation for the h ~ 5e-3 of adjacent steps) and by the recurrence above it.
"""
import math

import numpy as np
import torch

from dxmi_hip import ops

from . import stage_loop as _loop
from ..cm.karras_diffusion import _memo
from .ddpm_sample import ddpm_timesteps
from .var_sampler import calc_diffusion_hyperparams

ALGORITHMS = ("dpmsolver++", "sde-dpmsolver++")
SOLVER_TYPES = ("midpoint", "exact")
SKIP_TYPES = ("logsnr", "uniform", "quad")


# ------------------------------------------------------------------------------------------------- host schedule
def _log_snr(alpha_bar):
    """lambda = log alpha - log sigma of a float64 Alpha_bar."""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    return 0.5 * (np.log(ab) - np.log1p(-ab))


def _logsnr_sequence(lam, S):
    """S values linear in lambda from lam[0] to lam[-1], each mapped to the step with the nearest lambda (a tie: the lowest index).
    lam is strictly decreasing."""
    target = np.linspace(lam[0], lam[-1], S)
    pos = np.clip(np.searchsorted(-lam, -target, side="left"), 1, len(lam) - 1)      # lam[pos - 1] >= target >= lam[pos]
    low = np.abs(lam[pos - 1] - target) <= np.abs(lam[pos] - target)
    return [int(v) for v in np.where(low, pos - 1, pos)]


def _logsnr_ok(lam, S):
    if S < 2 or S > len(lam):
        return False
    tau = _logsnr_sequence(lam, S)
    return tau[0] == 0 and tau[-1] == len(lam) - 1 and all(b > a for a, b in zip(tau, tau[1:]))


def dpm_timesteps(S, T=1000, skip_type="logsnr", beta_0=1e-4, beta_T=0.02):
    """The S steps of a run, increasing, tau_0 == 0.  uniform / quad: ddpm_timesteps.  logsnr (the DPM-Solver papers' spacing):
    S values linear in lambda from lambda[0] to lambda[T - 1], each mapped to the step with the nearest lambda (a tie: the lowest
    index), so tau_{S-1} == T - 1.  ValueError unless 2 <= S and the steps are strictly increasing (too many steps map two values to
    one integer step at the crowded low-noise end); the message names the largest S that works."""
    S, T = int(S), int(T)
    if skip_type not in SKIP_TYPES:
        raise ValueError(f"dpm_timesteps: skip_type must be one of {SKIP_TYPES}, got {skip_type!r}")
    if skip_type != "logsnr":
        return ddpm_timesteps(S, T, skip_type)
    if T < 2:
        raise ValueError(f"dpm_timesteps: logsnr spacing needs T >= 2, got {T}")
    lam = _log_snr(calc_diffusion_hyperparams(T, beta_0, beta_T)["Alpha_bar"].to(torch.float32).numpy())
    if not (np.diff(lam) < 0).all():
        raise ValueError("dpm_timesteps: the schedule's log-SNR is not strictly decreasing")
    if not _logsnr_ok(lam, S):
        largest = max((n for n in range(T, 1, -1) if _logsnr_ok(lam, n)), default=None)
        raise ValueError(f"dpm_timesteps: {S} logsnr steps do not give 2 <= S strictly increasing steps from 0 to T - 1 = {T - 1}; "
                         f"the largest S that works is {largest}")
    return _logsnr_sequence(lam, S)


def _check_mode(algorithm, order, solver_type):
    if algorithm not in ALGORITHMS:
        raise ValueError(f"algorithm must be one of {ALGORITHMS}, got {algorithm!r}")
    if solver_type not in SOLVER_TYPES:
        raise ValueError(f"solver_type must be one of {SOLVER_TYPES}, got {solver_type!r}")
    if isinstance(order, bool) or int(order) != order or not 1 <= int(order) <= 3:
        raise ValueError(f"order must be 1, 2 or 3, got {order!r}")
    if algorithm == "sde-dpmsolver++" and int(order) == 3:
        raise ValueError("sde-dpmsolver++ is defined for orders 1 and 2, got order 3")


def _moments(h, count):
    """M_n = int_0^h e^-v v^n dv for n < count, float64.  Below h = 1 the series h^(n+1) sum_k (-h)^k / (k! (n + k + 1)), whose
    terms fall at once (M_n ~ h^(n+1) / (n + 1): the recurrence would take it as the difference of two numbers 1 / h times as
    large); from h = 1 on the recurrence M_0 = -expm1(-h), M_n = n M_{n-1} - h^n e^-h."""
    if h < 1.0:
        out = []
        for n in range(count):
            term, total = 1.0, 0.0
            for k in range(40):
                total += term / (n + k + 1)
                term *= -h / (k + 1)
            out.append(h ** (n + 1) * total)
        return out
    out = [-math.expm1(-h)]
    for n in range(1, count):
        out.append(n * out[-1] - h ** n * math.exp(-h))
    return out


def _lagrange_weights(nodes, moments):
    """sum_n c_{j,n} moments[n] for every Lagrange basis polynomial L_j(v) = sum_n c_{j,n} v^n on `nodes`."""
    out = []
    for j, vj in enumerate(nodes):
        poly = np.poly1d([1.0])
        for i, vi in enumerate(nodes):
            if i != j:
                poly = poly * np.poly1d([1.0, -vi]) / (vj - vi)
        out.append(float(sum(c * moments[n] for n, c in enumerate(poly.coeffs[::-1]))))
    return out


def dpm_orders(S, order, lower_order_final=True):
    """The order of every row: min(order, k + 1), with lower_order_final also min(., S - k); the last (denoise) row has order 1."""
    o = [min(int(order), k + 1) for k in range(S)]
    if lower_order_final:
        o = [min(v, S - k) for k, v in enumerate(o)]
    o[-1] = 1
    return o


def dpm_coefficients(alpha_bar, tau, algorithm="dpmsolver++", order=2, solver_type="midpoint", lower_order_final=True):
    """The scalars of every transition in float64, noisiest first, from `alpha_bar` as given (any float array): a dict of arrays
    cx, w0, w1, w2, s, a, b and order (int64).  A weight beyond a row's order is exactly 0."""
    _check_mode(algorithm, order, solver_type)
    ab = np.asarray(alpha_bar, dtype=np.float64)
    t = np.asarray(list(tau)[::-1], dtype=np.int64)
    alpha, sigma, lam = np.sqrt(ab[t]), np.sqrt(1.0 - ab[t]), _log_snr(ab[t])
    co = multistep_coefficients(alpha, sigma, lam, algorithm, order, solver_type, lower_order_final,
                                lambda k: f"dpm_coefficients: the log-SNR must rise from step {t[k]} to step {t[k + 1]}")
    co["a"], co["b"] = 1.0 / alpha, sigma / alpha
    return co


def multistep_coefficients(alpha, sigma, lam, algorithm, order, solver_type, lower_order_final, not_rising):
    """The solver in its (alpha, sigma, lambda) form, stated once for every parametrisation (the DDPM teacher's here, the EDM nets'
    in models/cm/dpm_sample.py): float64 arrays of the S evaluations, noisiest first -> cx, w0, w1, w2, s and order (int64) of the
    S rows; the last row goes to alpha_p = 1, sigma_p = 0.  not_rising(k): the message when lambda does not rise over row k."""
    S = len(lam)
    sde = algorithm == "sde-dpmsolver++"
    rate = 2.0 if sde else 1.0
    orders = dpm_orders(S, order, lower_order_final)
    co = {k: np.zeros(S) for k in ("cx", "w0", "w1", "w2", "s")}
    co["order"] = np.asarray(orders, dtype=np.int64)
    for k in range(S - 1):
        o, h = orders[k], lam[k + 1] - lam[k]
        if not h > 0:
            raise ValueError(not_rising(k))
        alpha_p, sigma_p = alpha[k + 1], sigma[k + 1]
        gain = -math.expm1(-rate * h)                                  # 1 - e^-h (ODE), 1 - e^-2h (SDE)
        co["cx"][k] = sigma_p / sigma[k] * (math.exp(-h) if sde else 1.0)
        co["s"][k] = sigma_p * math.sqrt(-math.expm1(-2.0 * h)) if sde else 0.0
        if o == 2 and solver_type == "midpoint":
            r = (lam[k] - lam[k - 1]) / h
            w = [alpha_p * gain * (1.0 + 0.5 / r), -alpha_p * gain * 0.5 / r]
        else:
            # v = lambda_p - lambda: the nodes are h, h + (lambda_k - lambda_{k-1}), ...; the SDE's integrand e^-2v is the ODE's in 2v
            nodes = [rate * (lam[k + 1] - lam[k - j]) for j in range(o)]
            w = [alpha_p * v for v in _lagrange_weights(nodes, _moments(rate * h, o))]
        for j, v in enumerate(w):
            co[f"w{j}"][k] = v
    co["w0"][-1] = 1.0                                                 # the denoise row: x' = D, alpha_p = 1, sigma_p = 0
    return co


UNIPC_VARIANTS = ("bh1", "bh2")


def unipc_coefficients(alpha, sigma, lam, order, variant, corrector, lower_order_final, not_rising):
    """UniPC (Zhao et al. 2023, arXiv:2302.04867; multistep, data prediction, ODE) in the (alpha, sigma, lambda) form of
    multistep_coefficients: float64 arrays of the S evaluations, noisiest first -> the predictor's cx, w0, w1, w2 and order, and
    the corrector's ccx, cv0..cv3 and corr_order (0: the row is not corrected) of the S rows.  With B(h) = h (bh1) or 1 - e^-h
    (bh2) and g = 1 - e^-h, row k < S - 1 after evaluation k:
        corrector, k >= 1, order q = order[k - 1], h = lambda_k - lambda_{k-1}:
            x_k = (sigma_k / sigma_{k-1}) x_{k-1} + sum_{j <= q} cv_j D_{k-j}
            q = 1 (rho = 1/2): cv_0 = alpha_k B / 2, cv_1 = alpha_k (g - B / 2)
            q >= 2: cv_j = alpha_k int_0^h e^-v L_j(v) dv, L_j the Lagrange basis on the q + 1 nodes v_j = lambda_k - lambda_{k-j}
                    (UniPC's system R rho = b solved in closed form: B cancels)
        predictor, order p = order[k], h = lambda_{k+1} - lambda_k:
            xt_{k+1} = (sigma_{k+1} / sigma_k) x_k + sum_{j < p} w_j D_{k-j}
            p = 1: w_0 = alpha_{k+1} g;  p = 3: multistep_coefficients' "exact" rows (B cancels)
            p = 2 (rho = 1/2), r = (lambda_k - lambda_{k-1}) / h: w_0 = alpha_{k+1} (g + B / (2r)), w_1 = -alpha_{k+1} B / (2r);
                  with bh2 multistep_coefficients' "midpoint" row
    The last row is the denoise row and is never corrected.  A weight beyond a row's order is exactly 0."""
    if variant not in UNIPC_VARIANTS:
        raise ValueError(f"variant must be one of {UNIPC_VARIANTS}, got {variant!r}")
    if isinstance(order, bool) or int(order) != order or not 1 <= int(order) <= 3:
        raise ValueError(f"order must be 1, 2 or 3, got {order!r}")
    S = len(lam)
    co = multistep_coefficients(alpha, sigma, lam, "dpmsolver++", order, "exact", lower_order_final, not_rising)
    mid = multistep_coefficients(alpha, sigma, lam, "dpmsolver++", order, "midpoint", lower_order_final, not_rising)
    del co["s"]
    orders = [int(o) for o in co["order"]]
    for k in ("ccx", "cv0", "cv1", "cv2", "cv3"):
        co[k] = np.zeros(S)
    co["corr_order"] = np.zeros(S, dtype=np.int64)

    def bh(h):
        return h if variant == "bh1" else -math.expm1(-h)

    for k in range(S - 1):
        if orders[k] == 2:
            if variant == "bh2":
                co["w0"][k], co["w1"][k] = mid["w0"][k], mid["w1"][k]
            else:
                h = lam[k + 1] - lam[k]
                r = (lam[k] - lam[k - 1]) / h
                co["w0"][k] = alpha[k + 1] * (-math.expm1(-h) + bh(h) * 0.5 / r)
                co["w1"][k] = -alpha[k + 1] * bh(h) * 0.5 / r
        if corrector and k >= 1:
            q, h = orders[k - 1], lam[k] - lam[k - 1]
            co["corr_order"][k], co["ccx"][k] = q, sigma[k] / sigma[k - 1]
            if q == 1:
                half = bh(h) * 0.5
                cv = [alpha[k] * half, alpha[k] * (-math.expm1(-h) - half)]
            else:
                nodes = [lam[k] - lam[k - j] for j in range(q + 1)]
                cv = [alpha[k] * v for v in _lagrange_weights(nodes, _moments(h, q + 1))]
            for j, v in enumerate(cv):
                co[f"cv{j}"][k] = v
    return co


def unipc_dpm_coefficients(alpha_bar, tau, order=3, variant="bh1", corrector=True, lower_order_final=True):
    """unipc_coefficients of the DDPM teacher, from `alpha_bar` as given (any float array) on the steps tau, with a = 1 / alpha and
    b = sigma / alpha of every evaluation (dpm_coefficients' two)."""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    t = np.asarray(list(tau)[::-1], dtype=np.int64)
    alpha, sigma, lam = np.sqrt(ab[t]), np.sqrt(1.0 - ab[t]), _log_snr(ab[t])
    co = unipc_coefficients(alpha, sigma, lam, order, variant, corrector, lower_order_final,
                            lambda k: f"unipc_coefficients: the log-SNR must rise from step {t[k]} to step {t[k + 1]}")
    co["a"], co["b"] = 1.0 / alpha, sigma / alpha
    return co


class DPMSampleSchedule(_loop.StageSchedule):
    """table: fp32 [S, ops.MT_COLS], row k = the transition tau_{S-1-k} -> tau_{S-2-k}: dpm_coefficients on the fp32 Alpha_bar in
    float64, rounded once.  draws[k]: whether transition k adds noise (S != 0); coef: the float64 coefficients.  The class
    attributes are what stage_loop asks of a schedule; the torch loop's state is float64 when noise[0] is (a float64 network then
    runs in float64 on the widened fp32 table)."""
    sampler, hist_slots = "dpm_sample", 3
    stage, FIRST, STEP, T_COL = staticmethod(ops.dpm_stage), ops.DPM_FIRST, ops.DPM_STEP, ops.MT_T

    def __init__(self, steps=10, order=2, algorithm="dpmsolver++", solver_type="midpoint", skip_type="logsnr", lower_order_final=True,
                 clip_denoised=True, T=1000, beta_0=1e-4, beta_T=0.02):
        _check_mode(algorithm, order, solver_type)
        hp = calc_diffusion_hyperparams(int(T), beta_0, beta_T)
        alpha_bar = hp["Alpha_bar"].to(torch.float32).numpy()
        self.tau = dpm_timesteps(steps, T, skip_type, beta_0, beta_T)
        self.steps, self.T = len(self.tau), int(T)
        self.order, self.algorithm, self.solver_type, self.skip_type = int(order), algorithm, solver_type, skip_type
        self.lower_order_final, self.clip_denoised = bool(lower_order_final), bool(clip_denoised)
        self.coef = co = dpm_coefficients(alpha_bar, self.tau, algorithm, order, solver_type, lower_order_final)
        S = self.steps
        tab = np.zeros((S, ops.MT_COLS), dtype=np.float32)
        times = np.asarray(self.tau[::-1], dtype=np.float32)
        tab[:, ops.MT_T] = times
        tab[:-1, ops.MT_T_NEXT] = times[1:]
        for col, k in ((ops.MT_CX, "cx"), (ops.MT_W0, "w0"), (ops.MT_W1, "w1"), (ops.MT_W2, "w2"), (ops.MT_S, "s"), (ops.MT_A, "a"),
                       (ops.MT_B, "b"), (ops.MT_ORDER, "order")):
            tab[:, col] = co[k].astype(np.float32)
        tab[:, ops.MT_FLAGS] = ops.MT_FLAG_CLIP if self.clip_denoised else 0
        tab[-1, ops.MT_FLAGS] += ops.MT_FLAG_LAST
        assert tab[-1, ops.MT_S] == 0 and tab[-1, ops.MT_CX] == 0 and tab[-1, ops.MT_W0] == 1
        # a row reads exactly the history its order names: rows 0 and 1 and the lowered rows never touch an unwritten slot
        for k in range(S):
            assert (tab[k, ops.MT_W1] != 0) == (co["order"][k] >= 2) and (tab[k, ops.MT_W2] != 0) == (co["order"][k] >= 3), k
        super().__init__(torch.from_numpy(tab))
        self.draws = [bool(v != 0) for v in tab[:, ops.MT_S]]
        self.n_draws = sum(self.draws)

    def transition(self, x, eps, z, row, hist):
        return dpm_transition(x, eps, z, row, hist)

    def graph_name(self, shape, mode):
        return f"dpm_sample{(self.steps, self.order, self.algorithm, tuple(shape), mode)}"


_SCHEDULES = {}


def dpm_sample_schedule(steps=10, order=2, algorithm="dpmsolver++", solver_type="midpoint", skip_type="logsnr", lower_order_final=True,
                        clip_denoised=True, T=1000, beta_0=1e-4, beta_T=0.02):
    """The (cached) DPMSampleSchedule of these settings: one object per setting, so that a replay graph keyed on the table's
    identity is found again by the next call."""
    _check_mode(algorithm, order, solver_type)
    key = (int(steps), int(order), algorithm, solver_type, skip_type, bool(lower_order_final), bool(clip_denoised), int(T),
           float(beta_0), float(beta_T))
    return _memo(_SCHEDULES, key, 32, lambda: DPMSampleSchedule(steps, order, algorithm, solver_type, skip_type, lower_order_final,
                                                                clip_denoised, T, beta_0, beta_T))


def dpm_transition(x, eps, z, row, hist=()):
    """One transition on `row` (a table row, or 16 coefficients of another dtype in its layout) as torch expressions in the
    operation order of dxmi_dpm_stage -> (x', D0).  hist: (D_{k-1}, D_{k-2}), the data predictions of the evaluations before, as
    far as the row's weights are not 0 (a zero weight reads nothing).  z None or row[MT_S] == 0: no noise is added."""
    d0 = row[ops.MT_A] * x - row[ops.MT_B] * eps
    if int(row[ops.MT_FLAGS]) & ops.MT_FLAG_CLIP:
        d0 = d0.clamp(-1, 1)
    acc = row[ops.MT_CX] * x + row[ops.MT_W0] * d0
    for j, col in enumerate((ops.MT_W1, ops.MT_W2)):
        if float(row[col]) != 0.0:
            acc = acc + row[col] * hist[j]
    if z is not None and float(row[ops.MT_S]) != 0.0:
        acc = acc + row[ops.MT_S] * z
    return acc, d0


def replay_graphs(net):
    """The StepGraphs dpm_sample holds for `net` (their .captures / .replays count what ran)."""
    return _loop.replay_graphs(net, DPMSampleSchedule.sampler)


def dpm_sample(net, shape, steps=10, order=2, algorithm="dpmsolver++", solver_type="midpoint", skip_type="logsnr",
               lower_order_final=True, clip_denoised=True, device=None, generator=None, noise=None, callback=None, progress=False,
               use_graph=False, T=1000, beta_0=1e-4, beta_T=0.02):
    """Sample the DDPM teacher with multistep DPM-Solver++: `steps` network evaluations on dpm_timesteps(steps, T, skip_type) ->
    clamp(x_0, -1, 1), [B, C, H, W].  algorithm "dpmsolver++" (the ODE solver, orders 1-3) or "sde-dpmsolver++" (orders 1-2);
    solver_type "midpoint" (Algorithm 2 of the paper) or "exact" (the Lagrange weights) for the second-order rows;
    lower_order_final lowers the order of the last rows so that the last transition is first order.

    The contract of ddpm_sample.  net: the HIP Model (bare or under .module), or any callable net(x, t_float [B]) -> eps.  On the
    device every transition is one network evaluation and one dxmi_dpm_stage launch; a CPU `device` with a callable runs the same
    expressions in torch.  noise: S + 1 recorded draws (x_T, then one per transition; those of transitions that add no noise are not
    read); nothing is drawn then.  callback({"i", "t", "x", "pred_xstart"}) after every transition (x: the new state, before the
    final clamp).  generator: a models.cm.random_util generator.  None / dummy: torch's device generator.  determ / determ-indiv:
    x_T is generator.randn and every transition's z is made inside the stage launch: bit for bit what generator.randn_like draws
    fed through noise= give, and generator.draw ends advanced by the draws made.  The ODE solver draws x_T alone.
    use_graph: capture ONE transition as a StepGraph and replay it for every later transition of every call with the same network,
    shape, device, table and noise source; the data predictions a later row reads live in static buffers the captured launch
    addresses from the row number.  Off with callback, progress or noise=.  The returned tensor is then STATIC: the next call of the
    same key overwrites it."""
    sch = dpm_sample_schedule(steps, order, algorithm, solver_type, skip_type, lower_order_final, clip_denoised, T, beta_0, beta_T)
    return _loop.sample(sch, net, shape, device, generator, noise, callback, progress, use_graph, float64_state=True)
