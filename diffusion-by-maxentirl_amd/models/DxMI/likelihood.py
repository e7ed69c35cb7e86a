"""Likelihood (bits/dim) of the DDPM teacher (models/DxMI/unet_small.py) by the probability-flow ODE: the loop, the launch and the
formulas of models/cm/likelihood.py in the noise-prediction parametrisation.

With ab = Alpha_bar (the fp32 table the samplers use, read into float64) the EDM variable of x_t is x^ = x_t / sqrt(ab) at
sigma = sqrt((1 - ab) / ab), and the net's eps_theta(x_t, step) is F: c_skip = 1, c_out = -sigma, c_in = 1 / sqrt(1 + sigma^2) =
sqrt(ab), so k = F and div = c_in sum_i e_i g_i.  The time is the integer step: the nodes are the steps 0 = tau_0 < ... < tau_S =
T - 1 of dpm_timesteps(S + 1, T, skip_type) (logsnr ends at T - 1 and accepts at most 37 steps for T = 1000; uniform and quad stop
short of it, and their last node is moved to T - 1).  The state starts as x^ = x_0 / sqrt(ab[tau_0]), so logdet0 = -(d / 2) ln ab[tau_0], and
the last node's state is scored under N(0, I / ab[T - 1]).  The integral bound (the ELBO) of the DDPM paper is another quantity and
is not computed here.
"""
import numpy as np
import torch

from ..cm import likelihood as _ll
from ..cm.karras_diffusion import _memo
from .ddpm_train import _hip_model
from .dpm_sample import dpm_timesteps
from .var_sampler import calc_diffusion_hyperparams

_SCHEDULES = {}


def ddpm_ll_schedule(d, steps=40, skip_type="logsnr", T=1000, beta_0=1e-4, beta_T=0.02):
    """The (cached) schedule of the DDPM teacher for images of d elements; .tau: the S + 1 integer steps."""
    key = (int(d), _ll._check_steps("ddpm_log_likelihood", steps), skip_type, int(T), float(beta_0), float(beta_T))

    def build():
        try:
            tau = list(dpm_timesteps(int(steps) + 1, T, skip_type, beta_0, beta_T))
        except ValueError as err:
            raise ValueError(f"ddpm_log_likelihood: steps = {steps} needs {int(steps) + 1} nodes: {err} (skip_type='uniform' accepts "
                             f"up to T - 1 steps)") from None
        tau[-1] = int(T) - 1      # uniform / quad stop short of T - 1: the last node is moved there, the prior is always step T - 1's
        ab = calc_diffusion_hyperparams(int(T), beta_0, beta_T)["Alpha_bar"].to(torch.float32).numpy().astype(np.float64)[tau]
        sigma = np.sqrt((1.0 - ab) / ab)
        sch = _ll.PFLikelihoodSchedule(_ll.pf_ll_table(sigma, np.ones_like(sigma), -sigma, np.sqrt(ab), np.asarray(tau, dtype=np.float64), d,
                                                       xscale=1.0 / np.sqrt(ab[0]), logdet0=-0.5 * d * np.log(ab[0]),
                                                       prior_var=1.0 / ab[-1]), sigma, d)
        sch.tau = list(tau)
        return sch
    return _memo(_SCHEDULES, key, 32, build)


def _evaluator(net):
    hip = _hip_model(net)
    if hip is None:
        return None, lambda x_in, t, e: _ll.autograd_vjp(net, x_in, t, e, {})
    from .unet_small_train import input_vjp
    return hip, lambda x_in, t, e: input_vjp(hip, x_in, t, e)


def ddpm_log_likelihood(net, x0, steps=40, skip_type="logsnr", probe="rademacher", eps=None, generator=None, T=1000, beta_0=1e-4,
                        beta_T=0.02, _launches=None):
    """NOTE the defaults: skip_type="logsnr" accepts at most 37 steps at T = 1000, so the default steps=40 with it raises ValueError
    (the message says so); pass skip_type="uniform", as eval_bpd.py does, or steps <= 37.

    log p(x0) and bits/dim of the DDPM teacher under its probability-flow ODE (module docstring) -> {"logp", "bpd", "prior_logp",
    "delta_logp": [N] each, "nfe": 2 * steps}; delta_logp holds logdet0 and the integrated divergence.

    net: the HIP Model (bare or under .module; x0 fp32 on the device: one dxmi_pf_ll_stage launch after each of the 2 * steps
    evaluations, each a forward and an input-only backward), or any torch callable net(x_t, t_float [N]) -> eps (the same expressions
    in torch in x0's dtype).  steps + 1 nodes must be steps dpm_timesteps accepts for skip_type.  probe, eps and generator as
    models.cm.likelihood.edm_log_likelihood."""
    if not torch.is_tensor(x0) or x0.dim() < 2 or x0.numel() == 0:
        raise ValueError("ddpm_log_likelihood: x0 must be a non-empty batch [N, ...]")
    sch = ddpm_ll_schedule(x0[0].numel(), steps, skip_type, T, beta_0, beta_T)
    hip, evaluate = _evaluator(net)
    return _ll.run("ddpm_log_likelihood", sch, hip, evaluate, x0, probe, eps, generator, _launches)
