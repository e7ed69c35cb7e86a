"""Noise-prediction training of the CIFAR-10 DDPM U-Net, the teacher `train_cifar10.py` starts from (`training.sampler_ckpt`).

The reference downloads that network (FastDPM's DDPM checkpoint) and has no code that trains it; this is Ho et al. 2020, "Denoising
Diffusion Probabilistic Models": the forward process q(x_t | x_0) = N(sqrt(alpha_bar_t) x_0, (1 - alpha_bar_t) I) (eq. 4) and the
simplified objective L_simple = E |eps - eps_theta(x_t, t)|^2 (eq. 14), on the linear-beta tables VARSampler is built on
(models/DxMI/var_sampler.py calc_diffusion_hyperparams).

  DDPMSchedule      sqrt(alpha_bar) and sqrt(1 - alpha_bar) as one fp32 [2, T] table, built once on the host, uploaded once per device;
                    training_losses(net, x_start, t=None, noise=None) -> {"loss", "mse"} per sample.  On the HIP Model with device
                    tensors the loss is ONE autograd node around the network: dxmi_ddpm_prep, the U-Net forward of
                    models/DxMI/unet_small_train.py, dxmi_ddpm_loss_fwd; its backward is dxmi_ddpm_loss_bwd, then the U-Net backward.
                    Nothing is read back.  Any other callable, or CPU tensors, gets the same expressions in torch.
  DDPMTrainLoop     Adam (dxmi_hip.optim.Adam, betas (0.9, 0.999), eps 1e-8) with a linear learning-rate warm-up, gradient clipping on
                    the device (ops.gradnorm_clip: its coefficient goes into the Adam launch as grad_scale, the gradients are not
                    rewritten), one EMA launch series for all rates, FlatGradSync across ranks, checkpoints model%06d.pt /
                    ema_{rate}_%06d.pt / opt%06d.pt: the first two are plain state_dict()s of the bare Model, so
                    `training.sampler_ckpt=.../ema_0.9999_NNNNNN.pt` is all train_cifar10.py needs.  Resumed from the model file's step.
                    The logged terms are summed on the device and read back once per log_interval (progress.jsonl).

use_graph=True replays the step from hipGraphs (dxmi_hip/graph.py StepGraph): the first run_step runs eagerly (weight packs, workspaces,
optimiser state, the flat gradient buffer), the second is captured, later ones are replayed.  The batch is the graph's tensor argument;
t and noise are torch device RNG (graph-aware); dropout seeds and Adam's step scalars (the learning rate among them, read live) are
host inputs; the gradient exchange is a graph cut.  What a capture freezes: the batch shape, the EMA rates, grad_clip and the set of
trainable parameters.  A CPU model is the torch path of the host tests: torch's own Adam (the base class of dxmi_hip.optim.Adam,
same state dict) and torch's clip_grad_norm_ stand in, and use_graph=True is refused.
"""
import json
import os

import torch
import torch.distributed as dist

from dxmi_hip import graph as _graph
from dxmi_hip import ops
from dxmi_hip._lib import DxmiError
from dxmi_hip.dist import FlatGradSync, broadcast_parameters, is_distributed
from dxmi_hip.optim import Adam

from ..cm.karras_diffusion import _HostTable
from ..cm.nn import update_ema, update_ema_rates
from ..cm.train_util import find_ema_checkpoint, parse_resume_step_from_filename
from .unet_small_train import train_backward, train_forward
from .var_sampler import calc_diffusion_hyperparams


def _hip_model(net):
    """The HIP DDPM U-Net behind `net` (itself, or a wrapper's `.module`), else None."""
    from .unet_small import Model
    inner = net.module if hasattr(net, "module") else net
    return inner if isinstance(inner, Model) else None


def mean_flat(x):
    return x.mean(dim=list(range(1, x.ndim)))


class _DDPMLossFn(torch.autograd.Function):
    """prep -> U-Net forward (models.DxMI.unet_small_train) -> per-sample loss, as one node."""

    @staticmethod
    def forward(ctx, net, x_start, noise, t, tab, *params):
        eps, ctx.tape = train_forward(net, *ops.ddpm_prep(x_start, noise, t, tab))
        ctx.eps, ctx.noise = eps, noise
        return ops.ddpm_loss_fwd(eps, noise)

    @staticmethod
    def backward(ctx, g):
        d_eps = ops.ddpm_loss_bwd(g.detach().float().contiguous(), ctx.eps, ctx.noise)
        ctx.eps = None
        grads = train_backward(ctx.tape, d_eps)
        ctx.tape = None
        return (None,) * 5 + grads


class DDPMSchedule(_HostTable):
    """The forward process VARSampler's tables are built on: table[0] = sqrt(alpha_bar), table[1] = sqrt(1 - alpha_bar), fp32 [2, T],
    alpha_bar = calc_diffusion_hyperparams(T, beta_0, beta_T)["Alpha_bar"]; the square roots are taken once, on the host."""

    def __init__(self, T=1000, beta_0=1e-4, beta_T=0.02):
        if int(T) < 1:
            raise ValueError(f"DDPMSchedule: T must be at least 1, got {T}")
        alpha_bar = calc_diffusion_hyperparams(int(T), beta_0, beta_T)["Alpha_bar"].to(torch.float32)
        super().__init__(torch.stack([torch.sqrt(alpha_bar), torch.sqrt(1 - alpha_bar)]).contiguous())
        self.T, self.beta_0, self.beta_T = int(T), beta_0, beta_T

    def training_losses(self, net, x_start, t=None, noise=None):
        """{"loss": [N], "mse": [N]}: mean_flat((eps_theta(x_t, t) - noise)^2), x_t = sqrt(alpha_bar_t) x_start +
        sqrt(1 - alpha_bar_t) noise.  t: int64 [N] in [0, T) (drawn uniformly when None); noise: as x_start (standard normal when
        None); both draws are torch device RNG."""
        N = x_start.shape[0]
        if t is None:
            t = torch.randint(0, self.T, (N,), device=x_start.device)
        if noise is None:
            noise = torch.randn_like(x_start)
        hip = _hip_model(net)
        if hip is not None and x_start.is_cuda:
            return self._training_losses_hip(hip, x_start, t, noise)
        tab = self.table if x_start.device.type == "cpu" else self.device_table(x_start.device)
        t = t.to(device=x_start.device, dtype=torch.int64)
        shape = (-1,) + (1,) * (x_start.ndim - 1)
        x_t = tab[0][t].reshape(shape) * x_start + tab[1][t].reshape(shape) * noise
        eps = net(x_t, t.to(torch.float32))
        mse = mean_flat((eps - noise) ** 2)
        return {"loss": mse, "mse": mse}

    def _training_losses_hip(self, net, x_start, t, noise):
        if x_start.requires_grad or noise.requires_grad:
            raise NotImplementedError("training_losses on the HIP U-Net differentiates the network parameters only: x_start and noise "
                                      "must not require grad")
        f32 = lambda v: v.detach().to(torch.float32).contiguous()
        x_start, noise = f32(x_start), f32(noise)
        t = t.detach().to(device=x_start.device, dtype=torch.int64).reshape(-1).contiguous()
        if noise.shape != x_start.shape or t.numel() != x_start.shape[0] or x_start.dim() != 4:
            raise ValueError(f"training_losses: noise {tuple(noise.shape)} must match x_start {tuple(x_start.shape)} [N, C, H, W] and t "
                             f"({t.numel()}) hold one step per sample")
        if _graph.capturing() and not self.on_device(x_start.device):
            raise DxmiError(f"training_losses inside a StepGraph capture: the {self.T}-step table is not on {x_start.device} yet "
                            "(schedule.device_table(device) before the capture: an upload cannot be captured)")
        tab = self.device_table(x_start.device)
        if torch.is_grad_enabled():
            mse = _DDPMLossFn.apply(net, x_start, noise, t, tab, *ops.fast_parameters(net))
        else:
            x_t, tf = ops.ddpm_prep(x_start, noise, t, tab)
            if net.training and net.dropout_p > 0:      # dropout is part of the loss in train mode: the training forward applies it
                eps = train_forward(net, x_t, tf)[0]
            else:
                eps = net.forward_inference(x_t, tf)
            mse = ops.ddpm_loss_fwd(eps, noise)
        return {"loss": mse, "mse": mse}


def _rank():
    return dist.get_rank() if is_distributed() else 0


def _world():
    return dist.get_world_size() if is_distributed() else 1


LOG_KEYS = ("loss", "mse", "grad_norm")


class DDPMTrainLoop:
    def __init__(self, *, model, schedule, data, batch_size, lr=2e-4, warmup_steps=5000, grad_clip=1.0, ema_rate="0.9999",
                 log_interval=100, save_interval=10000, resume_checkpoint="", log_dir=None, total_steps=0, use_graph=False):
        self.model, self.schedule, self.data = model, schedule, data
        self.batch_size = batch_size
        self.lr, self.warmup_steps, self.grad_clip = float(lr), max(1, int(warmup_steps)), float(grad_clip)
        self.ema_rate = [ema_rate] if isinstance(ema_rate, float) else [float(x) for x in str(ema_rate).split(",")]
        self.log_interval, self.save_interval = log_interval, save_interval
        self.resume_checkpoint = resume_checkpoint
        self.log_dir = log_dir or os.getcwd()
        self.total_steps = int(total_steps)
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.device = self.params[0].device
        self.on_gpu = self.device.type == "cuda"
        if use_graph and not self.on_gpu:
            raise NotImplementedError("DDPMTrainLoop: use_graph=True needs a model on the device (a StepGraph replays HIP launches)")
        self.global_batch = self.batch_size * _world()

        self.step = 0             # optimiser steps taken, the resumed ones included
        if resume_checkpoint:
            self.step = parse_resume_step_from_filename(resume_checkpoint)
            self.model.load_state_dict(torch.load(resume_checkpoint, map_location=self.device))
        broadcast_parameters(self.model)
        opt_cls = Adam if self.on_gpu else torch.optim.Adam      # (module docstring: the CPU stand-in)
        self.opt = opt_cls(self.params, lr=self.lr, betas=(0.9, 0.999), eps=1e-8)
        if resume_checkpoint:
            opt_file = os.path.join(os.path.dirname(resume_checkpoint), f"opt{self.step:06d}.pt")
            if os.path.exists(opt_file):
                self.opt.load_state_dict(torch.load(opt_file, map_location=self.device))
        self.ema_params = [self._load_ema(rate) for rate in self.ema_rate]
        self.sync = FlatGradSync(self.model)
        if self.on_gpu:
            self.schedule.device_table(self.device)       # uploaded here: a capture cannot hold the copy
        self._log_acc, self._log_count, self.logged = None, 0, []
        self.use_graph = bool(use_graph)
        self._graph = _graph.StepGraph(self._device_step, self.device, warmup=0, modules=_graph.pack_modules(self.model),
                                       name="DDPMTrainLoop.run_step") if self.use_graph else None
        self._warm = False

    # ------------------------------------------------------------------ checkpoints
    def _named(self):
        return [(n, p) for n, p in self.model.named_parameters() if p.requires_grad]

    def _load_ema(self, rate):
        ema = [p.detach().clone() for p in self.params]
        ckpt = find_ema_checkpoint(self.resume_checkpoint, self.step, rate) if self.resume_checkpoint else None
        if ckpt:
            sd = torch.load(ckpt, map_location=self.device)
            ema = [sd[n].detach().to(torch.float32).clone().contiguous() for n, _ in self._named()]
        if is_distributed():
            with torch.no_grad():
                for p in ema:
                    dist.broadcast(p, 0)
        return ema

    def _state_dict_of(self, params):
        """state_dict() of the bare model with `params` in the place of its trainable parameters."""
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for (n, _), p in zip(self._named(), params):
            sd[n] = p.detach().clone()
        return sd

    def save(self):
        os.makedirs(self.log_dir, exist_ok=True)
        if _rank() == 0:
            for rate, params in zip(self.ema_rate, self.ema_params):
                torch.save(self._state_dict_of(params), os.path.join(self.log_dir, f"ema_{rate}_{self.step:06d}.pt"))
            torch.save(self.opt.state_dict(), os.path.join(self.log_dir, f"opt{self.step:06d}.pt"))
            # last: a restart never finds a model without its opt / EMA files
            torch.save(self._state_dict_of(self.params), os.path.join(self.log_dir, f"model{self.step:06d}.pt"))
        if is_distributed():
            dist.barrier()

    # ------------------------------------------------------------------ loop
    def run_loop(self):
        saved = True
        while not self.total_steps or self.step < self.total_steps:
            batch = next(self.data)
            self.run_step(batch[0] if isinstance(batch, (tuple, list)) else batch)
            saved = False
            if self.step % self.log_interval == 0:
                self.dumpkvs()
            if self.step % self.save_interval == 0:
                self.save()
                saved = True
        if self._log_count:
            self.dumpkvs()
        if not saved:
            self.save()

    def current_lr(self):
        return self.lr * min(1.0, (self.step + 1) / self.warmup_steps)

    def run_step(self, batch):
        lr = self.current_lr()
        for group in self.opt.param_groups:         # Adam reads it live, under replay too (a host input of the graph)
            group["lr"] = lr
        batch = batch.to(self.device)
        if self.use_graph and self._warm:
            self._graph(batch)
        else:
            self._device_step(batch)
        self._warm = True
        self.step += 1
        self._log_count += 1
        self._lr_logged = lr

    def _device_step(self, batch):
        """Everything run_step does on the device; the body of the StepGraph."""
        for p in self.params:
            p.grad = None             # FlatGradSync re-binds .grad to its flat buffer: gradients are dropped, never accumulated into
        losses = self.schedule.training_losses(self.model, batch)
        loss = losses["loss"].mean()
        loss.backward()
        self.sync()
        norm = self._optimize()
        self._update_ema()
        with torch.no_grad():
            terms = torch.stack([loss.detach().float(), losses["mse"].detach().float().mean(), norm.detach().float().reshape(())])
            if self._log_acc is None:       # (the first step is never a captured one)
                self._log_acc = torch.zeros_like(terms)
            self._log_acc.add_(terms)

    def _optimize(self):
        """Clip and step -> the gradient norm before clipping (device scalar)."""
        if not self.on_gpu:
            norm = torch.nn.utils.clip_grad_norm_(self.params, self.grad_clip if self.grad_clip > 0 else float("inf"))
            self.opt.step()
            return norm
        st = ops.gradnorm_clip([p.grad for p in self.params], self.grad_clip, scale_in_place=False)
        self.opt.step(grad_scale=st[1:2] if self.grad_clip > 0 else None)
        return st[0]

    def _update_ema(self):
        if self.on_gpu:
            update_ema_rates(self.ema_params, self.params, self.ema_rate)
            return
        for rate, params in zip(self.ema_rate, self.ema_params):
            update_ema(params, [p.detach() for p in self.params], rate=rate)

    @property
    def captures(self):
        return self._graph.captures if self._graph is not None else 0

    @property
    def replays(self):
        return self._graph.replays if self._graph is not None else 0

    # ------------------------------------------------------------------ logging
    def dumpkvs(self):
        """Means of the logged terms since the last dump: ONE device-to-host read.  Appended to self.logged, and written as a JSON
        line to log_dir/progress.jsonl on rank 0."""
        row = {"step": self.step, "samples": self.step * self.global_batch}
        if self._log_count:
            vals = self._log_acc.tolist()
            self._log_acc.zero_()
            row.update({k: v / self._log_count for k, v in zip(LOG_KEYS, vals)})
            row["lr"] = self._lr_logged
        self._log_count = 0
        self.logged.append(row)
        if _rank() == 0:
            os.makedirs(self.log_dir, exist_ok=True)
            with open(os.path.join(self.log_dir, "progress.jsonl"), "a") as f:
                f.write(json.dumps(row) + "\n")
        return row
