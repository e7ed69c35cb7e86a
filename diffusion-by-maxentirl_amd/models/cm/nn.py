"""Small helpers of `models.cm.nn` that the DxMI scripts import (reference: models/cm/nn.py).

Layer factories return torch.nn modules used as PARAMETER CONTAINERS by models.cm.unet.UNetModel; the
compute runs through dxmi_hip.  timestep_embedding is the device kernel (order 1 = [cos | sin] with
freq = exp(-ln(P) i / half), reference :119-137).
"""
import torch
import torch.nn as nn

from dxmi_hip import ops


class GroupNorm32(nn.GroupNorm):
    """32-group norm container (reference :18-20); statistics are always fp32 in the HIP kernels."""


def conv_nd(dims, *args, **kwargs):
    if dims != 2:
        raise ValueError(f"unsupported dimensions: {dims} (the DxMI image models are 2-D)")
    return nn.Conv2d(*args, **kwargs)


def linear(*args, **kwargs):
    return nn.Linear(*args, **kwargs)


def zero_module(module):
    for p in module.parameters():
        p.detach().zero_()
    return module


def normalization(channels):
    return GroupNorm32(32, channels)


def mean_flat(tensor):
    return tensor.mean(dim=list(range(1, len(tensor.shape))))


def append_dims(x, target_dims):
    dims_to_append = target_dims - x.ndim
    if dims_to_append < 0:
        raise ValueError(f"input has {x.ndim} dims but target_dims is {target_dims}, which is less")
    return x[(...,) + (None,) * dims_to_append]


def append_zero(x):
    return torch.cat([x, x.new_zeros([1])])


def _ema_device_lists(targets, sources):
    ts = [t for ts_ in targets for t in ts_]
    return bool(sources) and all(len(t) == len(sources) for t in targets) and all(
        t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts + sources)


def update_ema(target_params, source_params, rate=0.99, found_inf=None):
    """Reference :57-67.  Lists of CUDA fp32 tensors take one dxmi_ema_update launch series; anything else the reference's loop.
    found_inf: device fp32 flag of the launch series (non-zero leaves the targets untouched); the loop has no such gate."""
    targets, sources = list(target_params), list(source_params)
    if _ema_device_lists([targets], sources):
        update_ema_rates([targets], sources, [rate], found_inf=found_inf)
        return
    if found_inf is not None:
        raise ValueError("update_ema: found_inf needs lists of contiguous CUDA fp32 tensors (the dxmi_ema_update launch series)")
    for targ, src in zip(targets, sources):
        if rate == 0:       # a copy, bit for bit: 0 * targ + src turns a source of -0 into +0 and a non-finite targ into NaN
            targ.detach().copy_(src)
        else:
            targ.detach().mul_(rate).add_(src, alpha=1 - rate)


def update_ema_rates(targets_per_rate, source_params, rates, found_inf=None):
    """update_ema for several rates over the same sources, the source read once for all of them (dxmi_ema_update, up to
    ops.EMA_MAX_RATES rates per launch series).  found_inf: device fp32 flag; non-zero leaves every EMA untouched."""
    sources = [s.detach() for s in source_params]
    targets = [[t.detach() for t in ts] for ts in targets_per_rate]
    for k in range(0, len(rates), ops.EMA_MAX_RATES):
        ops.ema_update(targets[k:k + ops.EMA_MAX_RATES], sources, rates[k:k + ops.EMA_MAX_RATES], found_inf=found_inf)
    torch.autograd.graph.increment_version([t for ts in targets for t in ts])      # written through raw pointers


def timestep_embedding(timesteps, dim, max_period=10000):
    return ops.timestep_embedding(timesteps, dim, order=1, max_period=float(max_period))
