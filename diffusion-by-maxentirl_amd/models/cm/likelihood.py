"""Likelihood (bits/dim) of the EDM nets by the probability-flow ODE, and the loop both network families share (the DDPM teacher's
entry point is models/DxMI/likelihood.py).  Chen et al. 2018 (the instantaneous change of variables), Song et al. 2021 app. D.2,
Hutchinson's trace estimator.  The reference tree computes no likelihood.

  pf_ll_table            every per-step scalar in float64 from the nodes' sigma, c_skip, c_out, c_in and time (the host tests'
                         statement of the formulas)
  PFLikelihoodSchedule   one fp32 row per Heun step (columns ops.PL_*, include/dxmi_hip.h), float64 rounded once
  pf_ll_predict / pf_ll_correct   the two halves of a step as torch expressions, in the operation order of dxmi_pf_ll_stage
  edm_ll_schedule        the schedule of an EDM net: the Karras ladder, ascending
  edm_log_likelihood     log p and bits/dim per image
  dequantize_u8          uint8 images -> x_0 = (u + xi) / 128 - 1

In the EDM variable the state is x(sigma), dx/dsigma = k = (x - D(x; sigma)) / sigma and d log p_sigma(x(sigma)) / dsigma = -div k, so
    log p_data(x_0) = logdet0 + log N(x(sigma_S); 0, prior_var I) + int_{sigma_0}^{sigma_S} div k dsigma.
With D = c_skip x + c_out F, F = net(c_in x, time), one probe e per image and g = d(e . F)/d(net input):
    k   = ((1 - c_skip) x - c_out F) / sigma
    div ~ sum_i ((1 - c_skip) e_i^2 - c_out c_in e_i g_i) / sigma          (e_i^2 is kept: Gaussian probes work too)
Heun on (x, l) over the nodes sigma_0 < ... < sigma_S, h = sigma_{i+1} - sigma_i:
    k1, div1 at (x_i, sigma_i);  x~ = x_i + h k1;  k2, div2 at (x~, sigma_{i+1});  x_{i+1} = x_i + (h / 2)(k1 + k2);  l += (h / 2)(div1 + div2)
2 S network evaluations, each a forward and an input-only backward (unet_train.input_vjp on the HIP nets: no parameter gradient is
formed); the same e along the whole trajectory.  bpd = -log p / (d ln 2) + 7 for images that enter as x_0 = (u + xi) / 128 - 1.
EDM nets: get_scalings, time = 250 ln sigma, the nodes get_sigmas_karras(S + 1, sigma_min, sigma_max, rho) without the appended zero,
ascending; prior_var = sigma_max^2 (not sigma_max^2 + sigma_data^2: the ladder's top is taken as pure noise, as the samplers start
from it), logdet0 = 0, and the data is taken as the state at sigma_min.
A HIP net on the device takes one dxmi_pf_ll_stage launch after each evaluation; anything else (the CPU, analytic callables,
float64 nets) runs the same expressions in torch with torch.autograd.grad for g.
"""
import math

import numpy as np
import torch

from dxmi_hip import ops
from dxmi_hip._lib import DxmiError

from .karras_diffusion import _HostTable, _hip_unet, _memo, get_sigmas_karras
from .random_util import DeterministicGenerator, DummyGenerator

PROBES = ("rademacher", "gaussian")
DEQUANTIZE = ("uniform", "center")
XI_BITS = 16      # the uniform dequantisation noise is a multiple of 2^-16: u + xi, / 128 and - 1 are then exact in fp32


# ------------------------------------------------------------------------------------------------- host schedule
def pf_ll_table(sigma, c_skip, c_out, c_in, time, d, xscale=1.0, logdet0=0.0, prior_var=None):
    """The float64 table [S, ops.PL_COLS] of the S = len(sigma) - 1 Heun steps over the nodes `sigma` (strictly increasing);
    c_skip, c_out, c_in, time: the preconditioning and the network's time at every node; d: elements per image; prior_var: the
    variance of the Gaussian the last node's state is scored under (None: sigma_S^2)."""
    s = np.asarray(sigma, dtype=np.float64)
    c_skip, c_out, c_in, time = (np.asarray(v, dtype=np.float64) for v in (c_skip, c_out, c_in, time))
    if s.ndim != 1 or len(s) < 2 or not (np.diff(s) > 0).all() or not s[0] > 0:
        raise ValueError("pf_ll_table: the nodes must be at least two strictly increasing positive sigmas")
    S = len(s) - 1
    pv = float(s[-1] ** 2 if prior_var is None else prior_var)
    ka, kb, db = (1.0 - c_skip) / s, -c_out / s, -c_out * c_in / s
    tab = np.zeros((S, ops.PL_COLS), dtype=np.float64)
    tab[:, ops.PL_T], tab[:, ops.PL_T_NEXT] = time[:-1], time[1:]
    tab[:, ops.PL_CIN], tab[:, ops.PL_CIN_NEXT] = c_in[:-1], c_in[1:]
    tab[:, ops.PL_XSCALE], tab[:, ops.PL_LOGDET0] = xscale, logdet0
    tab[:, ops.PL_KA], tab[:, ops.PL_KB], tab[:, ops.PL_DB] = ka[:-1], kb[:-1], db[:-1]
    tab[:, ops.PL_KA2], tab[:, ops.PL_KB2], tab[:, ops.PL_DB2] = ka[1:], kb[1:], db[1:]
    tab[:, ops.PL_H] = s[1:] - s[:-1]
    tab[:, ops.PL_HH] = 0.5 * (s[1:] - s[:-1])
    tab[-1, ops.PL_FLAGS] = ops.PL_FLAG_LAST
    tab[:, ops.PL_PRIOR_Q] = -0.5 / pv
    tab[:, ops.PL_PRIOR_C] = -0.5 * d * math.log(2.0 * math.pi * pv)
    tab[:, ops.PL_BPD_SCALE] = -1.0 / (d * math.log(2.0))
    tab[:, ops.PL_SIGMA], tab[:, ops.PL_SIGMA_NEXT] = s[:-1], s[1:]
    return tab


class PFLikelihoodSchedule(_HostTable):
    """table: fp32 [S, ops.PL_COLS], row i = the Heun step sigma_i -> sigma_{i+1}: pf_ll_table rounded once.  table64: the float64
    values; sigmas: the float64 nodes; d: elements per image; net_keywords: the model_kwargs the network takes."""

    def __init__(self, table64, sigmas, d, net_keywords=()):
        self.table64, self.sigmas, self.d, self.net_keywords = table64, np.asarray(sigmas, dtype=np.float64), int(d), tuple(net_keywords)
        self.steps = table64.shape[0]
        super().__init__(torch.from_numpy(table64.astype(np.float32)))


def _check_steps(what, steps):
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
        raise ValueError(f"{what}: steps must be an integer >= 1, got {steps!r}")
    return int(steps)


def _refuse_distillation(diffusion):
    if getattr(diffusion, "distillation", False):
        raise NotImplementedError("edm_log_likelihood: distillation=True is refused: a consistency model maps every level to the "
                                  "data in one evaluation, it is no probability-flow ODE drift, so the change-of-variables "
                                  "formula has nothing to integrate; score the EDM teacher it was distilled from")


def edm_ll_nodes(steps, sigma_min, sigma_max, rho=7.0):
    """The S + 1 nodes of a run, fp32 values as float64 [S + 1], ascending from fp32(sigma_min) to fp32(sigma_max):
    get_sigmas_karras(S + 1, ...) without its appended zero, reversed."""
    S = _check_steps("edm_ll_nodes", steps)
    if not 0 < sigma_min < sigma_max:
        raise ValueError(f"edm_ll_nodes: 0 < sigma_min < sigma_max, got {sigma_min}, {sigma_max}")
    sig = get_sigmas_karras(S + 1, sigma_min, sigma_max, rho)[:-1].to(torch.float32).flip(0).numpy().astype(np.float64)
    if not (np.diff(sig) > 0).all():
        raise ValueError(f"edm_ll_nodes: {S + 1} karras nodes from {sigma_min} to {sigma_max} are not strictly increasing in fp32")
    return sig


_SCHEDULES = {}


def edm_ll_schedule(diffusion, d, steps=40, rho=7.0, sigma_min=None, sigma_max=None):
    """The (cached) schedule of an EDM net for images of d elements.  Of `diffusion` it holds sigma_data alone."""
    _refuse_distillation(diffusion)
    smin = float(diffusion.sigma_min if sigma_min is None else sigma_min)
    smax = float(diffusion.sigma_max if sigma_max is None else sigma_max)
    key = (float(diffusion.sigma_data), int(d), _check_steps("edm_log_likelihood", steps), float(rho), smin, smax)

    def build():
        s, sd = edm_ll_nodes(steps, smin, smax, rho), float(diffusion.sigma_data)
        den = s * s + sd * sd
        # get_scalings in float64; denoise()'s time
        return PFLikelihoodSchedule(pf_ll_table(s, sd * sd / den, s * sd / np.sqrt(den), 1.0 / np.sqrt(den), 250.0 * np.log(s + 1e-44), d),
                                    s, d, net_keywords=("y",))
    return _memo(_SCHEDULES, key, 32, build)


# ------------------------------------------------------------------------------------------------- the step, as torch expressions
def _image_sum(v):
    return v.reshape(v.shape[0], -1).sum(1)


def pf_ll_divergence(ka, db, e, g):
    """The per-image Hutchinson estimate sum_i (ka e_i^2 + db e_i g_i), in the launch's operation order."""
    return _image_sum(ka * (e * e) + db * (e * g))


def pf_ll_predict(row, x, F, g, e):
    """PREDICT on `row` (a table row, or its coefficients in another dtype) -> (k1, x~, div1)."""
    k1 = row[ops.PL_KA] * x + row[ops.PL_KB] * F
    return k1, x + row[ops.PL_H] * k1, pf_ll_divergence(row[ops.PL_KA], row[ops.PL_DB], e, g)


def pf_ll_correct(row, x, k1, F, g, e, div1, ell):
    """CORRECT on `row`, F and g of the evaluation at x~ -> (x', ell')."""
    xt = x + row[ops.PL_H] * k1
    k2 = row[ops.PL_KA2] * xt + row[ops.PL_KB2] * F
    div2 = pf_ll_divergence(row[ops.PL_KA2], row[ops.PL_DB2], e, g)
    return x + row[ops.PL_HH] * (k1 + k2), ell + row[ops.PL_HH] * (div1 + div2)


def pf_ll_finish(row, x, ell):
    """The prior term on the last row -> (prior_logp, logp, bpd)."""
    prior = row[ops.PL_PRIOR_Q] * _image_sum(x * x) + row[ops.PL_PRIOR_C]
    logp = ell + prior
    return prior, logp, logp * row[ops.PL_BPD_SCALE] + 7.0


# ------------------------------------------------------------------------------------------------- evaluations
def autograd_vjp(model, x_in, t, e, kw):
    """(F, g) of a torch callable: F = model(x_in, t, **kw), g = d(e . F)/dx_in by torch.autograd.grad."""
    with torch.enable_grad():
        xi = x_in.detach().requires_grad_(True)
        F = model(xi, t, **kw)
        assert F.shape == x_in.shape, f"network output {tuple(F.shape)} != image shape {tuple(x_in.shape)}"
        g = torch.autograd.grad((F * e).sum(), xi, allow_unused=True)[0] if F.requires_grad else None
    return F.detach().to(x_in.dtype), (torch.zeros_like(x_in) if g is None else g.to(x_in.dtype))


def _edm_evaluator(model, kw):
    hip = _hip_unet(model)
    if hip is None:
        return None, lambda x_in, t, e: autograd_vjp(model, x_in, t, e, kw)
    from .unet_train import input_vjp
    return hip, lambda x_in, t, e: input_vjp(hip, x_in, t, e, kw.get("y"))


# ------------------------------------------------------------------------------------------------- probes and dequantisation
def _deterministic(generator):
    return generator if isinstance(generator, DeterministicGenerator) else None


def make_probe(probe, shape, device, generator=None, dtype=torch.float32):
    """One probe per image, [N, ...] -> (e, fused): gaussian: standard normals; rademacher: +1 where the normal is >= 0, else -1.
    A determ / determ-indiv generator draws the normals from its counter (image i's probe then depends on neither the batch size nor
    the rank) and `fused` = dict(sample_index, seed, draw): what makes dxmi_pf_ll_stage form the same signs in the launch (None for a
    Gaussian probe, which the launch reads).  None / dummy: torch's generator of the device."""
    if probe not in PROBES:
        raise ValueError(f"probe must be one of {PROBES}, got {probe!r}")
    det, fused = _deterministic(generator), None
    if det is not None:
        idx, draw = det.get_indices(shape[0], det._device(device)), det._next_draw()
        z = ops.randn_indexed(idx, tuple(shape[1:]), det.seed, draw)
        if probe == "rademacher":
            fused = dict(sample_index=idx, seed=det.seed, draw=draw)
    else:
        z = torch.randn(tuple(shape), device=device)
    e = z if probe == "gaussian" else torch.where(z >= 0, torch.ones_like(z), -torch.ones_like(z))
    return e.to(dtype), fused


def dequantize_u8(u8, mode="uniform", generator=None):
    """uint8 [N, ...] -> x_0 = (u + xi) / 128 - 1, fp32 of the same shape: log2 128 = 7 is exactly the offset of bits/dim.
    center: xi = 0.5.  uniform: xi uniform on the multiples of 2^-16 in [0, 1), so x_0 is exact and lies in [u / 128 - 1,
    (u + 1) / 128 - 1).  With a determ / determ-indiv generator xi comes from dxmi_randint_indexed's counter: image i's xi depends on
    neither the batch size nor the rank; None / dummy: torch.randint on the tensor's device."""
    if mode not in DEQUANTIZE:
        raise ValueError(f"dequantize_u8: mode must be one of {DEQUANTIZE}, got {mode!r}")
    if u8.dtype != torch.uint8 or u8.dim() < 2:
        raise ValueError(f"dequantize_u8: a uint8 batch [N, ...] is expected, got {u8.dtype} {tuple(u8.shape)}")
    u = u8.to(torch.float32)
    if mode == "center":
        return (u + 0.5) / 128.0 - 1.0
    det = _deterministic(generator)
    if det is not None:
        r = det.randint(0, 1 << XI_BITS, tuple(u8.shape), device=u8.device)
    else:
        r = torch.randint(0, 1 << XI_BITS, tuple(u8.shape), device=u8.device)
    return (u + r.to(torch.float32) / float(1 << XI_BITS)) / 128.0 - 1.0


# ------------------------------------------------------------------------------------------------- the loop
def _loop_torch(sch, evaluate, x0, e):
    """The steps as torch expressions in x0's dtype on the widened fp32 table (a float64 network runs in float64)."""
    N, tab = x0.shape[0], sch.table.to(device=x0.device, dtype=x0.dtype)
    time = lambda v: torch.full((N,), float(v), device=x0.device, dtype=x0.dtype)
    x = x0 * tab[0, ops.PL_XSCALE]
    ell = torch.full((N,), float(tab[0, ops.PL_LOGDET0]), device=x0.device, dtype=x0.dtype)
    for i in range(sch.steps):
        row = tab[i]
        F, g = evaluate(row[ops.PL_CIN] * x, time(row[ops.PL_T]), e)
        k1, xt, div1 = pf_ll_predict(row, x, F, g, e)
        F, g = evaluate(row[ops.PL_CIN_NEXT] * xt, time(row[ops.PL_T_NEXT]), e)
        x, ell = pf_ll_correct(row, x, k1, F, g, e, div1, ell)
    prior, logp, bpd = pf_ll_finish(tab[-1], x, ell)
    return {"logp": logp, "bpd": bpd, "prior_logp": prior, "delta_logp": ell}


def _loop_device(sch, evaluate, x0, e, fused):
    """One dxmi_pf_ll_stage launch after each evaluation; `fused`: the launch forms the Rademacher signs itself."""
    tab = sch.device_table(x0.device)
    N = x0.shape[0]
    x = x0.clone(memory_format=torch.contiguous_format)
    x_in, k1 = torch.empty_like(x), torch.empty_like(x)
    t, div1, ell, prior, logp, bpd = (torch.empty(N, dtype=torch.float32, device=x.device) for _ in range(6))
    probe = dict(eps=e) if fused is None else fused
    ops.pf_ll_stage(ops.PF_LL_FIRST, tab, t, row=0, x=x, x_in=x_in, ell=ell)
    for i in range(sch.steps):
        F, g = evaluate(x_in, t, e)
        ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, row=i, x=x, model_out=F, vjp=g, k1=k1, x_in=x_in, div1=div1, **probe)
        F, g = evaluate(x_in, t, e)
        ops.pf_ll_stage(ops.PF_LL_CORRECT, tab, t, row=i, x=x, model_out=F, vjp=g, k1=k1, x_in=x_in, div1=div1, ell=ell, prior=prior,
                        logp=logp, bpd=bpd, **probe)
    return {"logp": logp, "bpd": bpd, "prior_logp": prior, "delta_logp": ell}


def run(what, sch, hip, evaluate, x0, probe, eps, generator, launches=None):
    """The body of edm_log_likelihood / ddpm_log_likelihood on the schedule `sch`.  hip: the HIP net behind the model, or None;
    evaluate(x_in, t, e) -> (F, g); launches: None = the launches for a HIP net on the device, the torch expressions otherwise;
    False forces the torch expressions (the GPU tests compare the two)."""
    if not torch.is_tensor(x0) or x0.dim() < 2 or x0.numel() == 0 or not x0.is_floating_point():
        raise ValueError(f"{what}: x0 must be a non-empty floating-point batch [N, ...]")
    if x0[0].numel() != sch.d:
        raise ValueError(f"{what}: the schedule was built for {sch.d} elements per image, x0 has {x0[0].numel()}")
    if hip is not None and not x0.is_cuda:
        raise DxmiError(f"{what}: the HIP net runs only on the device (x0 on the CPU takes a torch callable)")
    if hip is not None and x0.dtype != torch.float32:
        raise DxmiError(f"{what}: the HIP net takes fp32 images, got {x0.dtype}")
    if isinstance(generator, DummyGenerator):       # it forwards to torch: the same draws as no generator
        generator = None
    fused = None
    if eps is None:
        e, fused = make_probe(probe, tuple(x0.shape), x0.device, generator, x0.dtype)
    else:
        if probe not in PROBES:
            raise ValueError(f"probe must be one of {PROBES}, got {probe!r}")
        if not torch.is_tensor(eps) or eps.shape != x0.shape:
            raise ValueError(f"{what}: eps must have x0's shape {tuple(x0.shape)}")
        e = eps.to(device=x0.device, dtype=x0.dtype).contiguous()
    use = hip is not None if launches is None else bool(launches)
    if use and (hip is None or not x0.is_cuda):
        raise DxmiError(f"{what}: the launches serve a HIP net on the device")
    with torch.no_grad():
        out = _loop_device(sch, evaluate, x0.contiguous(), e, fused) if use else _loop_torch(sch, evaluate, x0, e)
    out["nfe"] = 2 * sch.steps
    return out


def edm_log_likelihood(diffusion, model, x0, steps=40, rho=7.0, sigma_min=None, sigma_max=None, probe="rademacher", eps=None,
                       model_kwargs=None, generator=None, _launches=None):
    """log p(x0) and bits/dim of an EDM net under its probability-flow ODE (module docstring) -> {"logp", "bpd", "prior_logp",
    "delta_logp": [N] each, "nfe": 2 * steps}; logp = prior_logp + delta_logp, delta_logp the integrated divergence.

    diffusion: a KarrasDenoiser with distillation=False (a consistency model is no PF-ODE drift: refused).  model(x_in, t,
    **model_kwargs): the HIP UNetModel (x0 fp32 on the device: one dxmi_pf_ll_stage launch after each of the 2 * steps evaluations,
    each a forward and an input-only backward), or any torch callable (the same expressions in torch in x0's dtype, g by
    torch.autograd.grad).  model_kwargs: the labels y alone.  x0: [N, C, H, W] in the net's data scale, e.g. dequantize_u8's.
    sigma_min / sigma_max: None = the diffusion's.  probe: "rademacher" (exact for a diagonal Jacobian) or "gaussian"; eps: the
    probe given, x0's shape (any values).  generator: a models.cm.random_util generator for the probe: determ / determ-indiv make
    image i's probe independent of the batch size and the rank, and the Rademacher signs are then formed inside the launches."""
    kw = dict(model_kwargs or {})
    if not torch.is_tensor(x0) or x0.dim() < 2 or x0.numel() == 0:
        raise ValueError("edm_log_likelihood: x0 must be a non-empty batch [N, ...]")
    sch = edm_ll_schedule(diffusion, x0[0].numel(), steps, rho, sigma_min, sigma_max)
    extra = set(kw) - set(sch.net_keywords)
    if extra:
        raise ValueError(f"edm_log_likelihood: model_kwargs {sorted(extra)} are not inputs of its network (it takes {sch.net_keywords})")
    hip, evaluate = _edm_evaluator(model, kw)
    return run("edm_log_likelihood", sch, hip, evaluate, x0, probe, eps, generator, _launches)
