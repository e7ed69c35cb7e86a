"""Noise-level sampler of the EDM DSM training loop (`models.cm.resample`).

The reference's TrainLoop imports `resample` (models/cm/train_util.py:14), but that module is absent from the reference tree, and
its default `UniformSampler(diffusion)` needs a `num_timesteps` that KarrasDenoiser does not have.  LogNormalSampler is therefore
not a restatement of reference code: it is the training distribution of the EDM paper (Karras et al. 2022, "Elucidating the
Design Space of Diffusion-Based Generative Models", Table 1: ln(sigma) ~ N(P_mean, P_std^2), P_mean = -1.2, P_std = 1.2),
returned in the reference's sampler shape `(sigmas, weights)` with unit weights.

DiscreteLogNormalSampler draws the ladder INDEX of a consistency-training pair from the discretised lognormal of improved consistency
training; it is an `index_sampler` of consistency_losses / CMTrainLoop, not a schedule_sampler.
"""
import math

import numpy as np
import torch

from dxmi_hip import graph as _graph
from dxmi_hip._lib import DxmiError
from .karras_diffusion import _HostTable, _memo, cd_levels


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


class _LevelCDF(_HostTable):
    """The fp32 CDF over the S - 1 level pairs of an S-level ladder, on the host; uploaded once per device."""

    def __init__(self, pmf, cdf32):
        super().__init__(cdf32)
        self.pmf, self.num_scales = pmf, int(cdf32.numel()) + 1


class DiscreteLogNormalSampler:
    """The level sampler of improved consistency training (Song and Dhariwal 2023, "Improved Techniques for Training Consistency
    Models", section 3.3; not in the reference tree): index i of the S-level ladder t_0 > ... > t_(S-1) of consistency_losses
    (cd_levels(S, ...).table, fp32) is drawn with probability
        p_i  proportional to  erf((ln t_i - P_mean) / (sqrt(2) P_std)) - erf((ln t_(i+1) - P_mean) / (sqrt(2) P_std)),  i = 0 .. S - 2,
    the mass a lognormal puts on [t_(i+1), t_i].  pmf and cdf = cumsum(p) / sum(p) are formed in float64; the CDF is rounded once to
    fp32 and its last entry set to 1.  A draw is u = rand(N), index = searchsorted(cdf, u, right=True): one tiny launch per microbatch,
    no kernel of its own.  Tables are memoised per S; KarrasDenoiser.consistency_losses(index_sampler=...) and CMTrainLoop take it."""

    def __init__(self, sigma_min=0.002, sigma_max=80.0, rho=7.0, p_mean=-1.1, p_std=2.0):
        if not (math.isfinite(float(p_mean)) and math.isfinite(float(p_std)) and float(p_std) > 0):
            raise ValueError(f"DiscreteLogNormalSampler: p_mean must be finite and p_std finite and > 0, got {p_mean!r}, {p_std!r}")
        self.sigma_min, self.sigma_max, self.rho = float(sigma_min), float(sigma_max), float(rho)
        self.p_mean, self.p_std = float(p_mean), float(p_std)
        self._tables = {}

    def cdf(self, num_scales):
        """-> the _LevelCDF of an S-level ladder: .pmf float64 [S - 1], .table fp32 [S - 1] (the CDF), device_table(device)."""
        return _memo(self._tables, int(num_scales), 64, lambda: self._build(int(num_scales)))

    def _build(self, S):
        levels = cd_levels(S, self.sigma_min, self.sigma_max, self.rho).table.tolist()      # fp32 values, as python floats
        e = [math.erf((math.log(t) - self.p_mean) / (math.sqrt(2.0) * self.p_std)) for t in levels]
        p = np.array([e[i] - e[i + 1] for i in range(S - 1)], dtype=np.float64)
        if not (np.isfinite(p).all() and (p >= 0).all() and p.sum() > 0):
            raise ValueError(f"DiscreteLogNormalSampler: no valid distribution over the {S}-level ladder (p_mean {self.p_mean}, "
                             f"p_std {self.p_std})")
        cdf32 = (np.cumsum(p) / p.sum()).astype(np.float32)
        cdf32[-1] = 1.0
        return _LevelCDF(torch.from_numpy(p / p.sum()), torch.from_numpy(cdf32))

    def indices_from_uniform(self, num_scales, u):
        """index of every u in [0, 1) (fp32, on the device the indices are wanted on) -> int64 in [0, S - 2]."""
        tab = self.cdf(num_scales)
        if _graph.capturing() and not tab.on_device(u.device):
            raise DxmiError(f"DiscreteLogNormalSampler inside a StepGraph capture: the CDF of num_scales {int(num_scales)} is not on "
                            f"{u.device} yet (cdf(num_scales).device_table(device) before the capture: an upload cannot be captured)")
        return torch.searchsorted(tab.device_table(u.device), u, right=True).clamp_(max=int(num_scales) - 2)

    def sample_indices(self, num_scales, batch_size, device, generator=None):
        """-> int64 [batch_size] on `device`.  With a `generator` the uniforms are drawn on its device and moved."""
        if generator is not None:
            u = torch.rand(batch_size, generator=generator, device=generator.device).to(device)
        else:
            u = torch.rand(batch_size, device=device)
        return self.indices_from_uniform(num_scales, u)
