"""Generate tests/golden/ddpm_sample.npz by running the REFERENCE's module-level VAR_sampling (models/DxMI/var_sampler.py:204-297)
on strided DDPM steps: the generalised-DDIM transition the teacher samplers of models/DxMI/ddpm_sample.py restate.

Runs ONLY in the build container, next to make_golden.py (same reference checkout and import stubs):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ddpm_sample.py

S = 6 uniform steps tau_i = (i T) // S of the T = 1000 linear-beta table, kappa in {0, 0.5, 1}, size [4, 3, 8, 8], an analytic
network 0.8 tanh(0.9 x + 1e-3 t).  user_defined_eta[i] = 1 - Alpha_bar[tau_i] / Alpha_bar[tau_{i-1}] (the first 1 - Alpha_bar[tau_0]),
formed in float64 from the reference's fp32 Alpha_bar, so that its running product Gamma_bar follows Alpha_bar[tau] to the last bits;
continuous_steps = the reversed tau as floats.  The reference draws with torch.randn inside the call: the draws are recorded by
wrapping torch.randn for the duration of the call; at kappa = 0 its Normal(pred_mean, 0) fails torch's argument validation, which is
switched off here (the log-probabilities are not recorded).  Arrays only:
  tau, alpha_bar, eta                        the steps, the reference's table, user_defined_eta
  gamma_bar                                  the reference's running product (:233-237) of 1 - eta in fp32
  k<kappa>.draws   [S + 1, 4, 3, 8, 8]       x_T, then the z of every step in order
  k<kappa>.x_seq   [S + 1, 4, 3, 8, 8]       the reference's x_seq (its last entry carries the 0.001 z the reference adds at the end)
  k<kappa>.pred_mean [S, 4, 3, 8, 8]         pred_mean_list
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference first on sys.path and installs its import stubs)

ref_vs = mg.ref_vs
S, T, BETA_0, BETA_T = 6, 1000, 1e-4, 0.02
SIZE = (4, 3, 8, 8)
KAPPAS = (0.0, 0.5, 1.0)


def net(x, t):
    return 0.8 * torch.tanh(0.9 * x + 1e-3 * t[:, None, None, None])


def main():
    hp = ref_vs.calc_diffusion_hyperparams(T, BETA_0, BETA_T)
    alpha_bar = hp["Alpha_bar"].to(torch.float32)
    tau = [(i * T) // S for i in range(S)]
    ab = alpha_bar.double().numpy()[tau]
    eta = np.concatenate([[1.0 - ab[0]], 1.0 - ab[1:] / ab[:-1]])
    gamma_bar = 1 - torch.from_numpy(eta).to(torch.float32)
    for t in range(1, S):
        gamma_bar[t] *= gamma_bar[t - 1]
    steps = [float(t) for t in tau[::-1]]
    arrays = dict(tau=np.asarray(tau), alpha_bar=alpha_bar, eta=eta, gamma_bar=gamma_bar)
    real_randn = torch.randn
    torch.distributions.Distribution.set_default_validate_args(False)
    for kappa in KAPPAS:
        draws = []

        def recording_randn(*a, **k):
            z = real_randn(*a, **k)
            draws.append(z.clone())
            return z

        torch.manual_seed(int(100 * kappa) + 7)
        torch.randn = recording_randn
        try:
            x_seq, _, _, pred_mean, _ = ref_vs.VAR_sampling(net, SIZE, hp, eta, kappa, steps, "cpu")
        finally:
            torch.randn = real_randn
        assert len(draws) == S + 1 and len(x_seq) == S + 1 and len(pred_mean) == S
        arrays[f"k{kappa}.draws"] = torch.stack(draws)
        arrays[f"k{kappa}.x_seq"] = torch.stack(x_seq)
        arrays[f"k{kappa}.pred_mean"] = torch.stack(pred_mean)
    mg.save("ddpm_sample", **arrays)


if __name__ == "__main__":
    main()
