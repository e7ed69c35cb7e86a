"""Noise-level sampler of the EDM DSM training loop (`models.cm.resample`).

The reference's TrainLoop imports `resample` (models/cm/train_util.py:14), but that module is absent from the reference tree, and
its default `UniformSampler(diffusion)` needs a `num_timesteps` that KarrasDenoiser does not have.  LogNormalSampler is therefore
not a restatement of reference code: it is the training distribution of the EDM paper (Karras et al. 2022, "Elucidating the
Design Space of Diffusion-Based Generative Models", Table 1: ln(sigma) ~ N(P_mean, P_std^2), P_mean = -1.2, P_std = 1.2),
returned in the reference's sampler shape `(sigmas, weights)` with unit weights.
"""
import torch


class LogNormalSampler:
    def __init__(self, p_mean=-1.2, p_std=1.2, generator=None):
        self.p_mean, self.p_std, self.generator = float(p_mean), float(p_std), generator

    def sample(self, batch_size, device):
        """-> (sigmas [batch_size] fp32 on `device`, weights = 1).  With a CPU `generator` the draw is made on the host."""
        if self.generator is not None:
            rnd = torch.randn(batch_size, generator=self.generator).to(device)
        else:
            rnd = torch.randn(batch_size, device=device)
        sigmas = (rnd * self.p_std + self.p_mean).exp()
        return sigmas, torch.ones_like(sigmas)
