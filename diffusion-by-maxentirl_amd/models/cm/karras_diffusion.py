"""EDM preconditioning and the Karras samplers of the EDM teacher (`models.cm.karras_diffusion`).

Reference: models/cm/karras_diffusion.py — KarrasDenoiser.__init__/get_snr/get_scalings (:33-68),
denoise (:337-351), karras_sample (:354-420), get_sigmas_karras (:423-429), get_ancestral_step (:437-444),
sample_euler_ancestral / sample_heun / sample_euler / sample_dpm (:447-640), and the consistency-model samplers
sample_onestep / stochastic_iterative_sampler (:644-683) with the zero-shot editing loops iterative_colorization /
iterative_inpainting / iterative_superres (:722-951), and the denoising score-matching loss training_losses with
get_weightings (:18-31, :82-106) that models.cm.train_util.TrainLoop trains the U-Net with, and the consistency distillation /
consistency training loss consistency_losses (:108-241) of models.cm.train_util.CMTrainLoop, its lpips norm (:221-234) through
models.cm.lpips once the caller supplies the weights, and progressive distillation: progdist_losses (:243-335) and its sampler
sample_progdist / progdist_sample (:378-379, :685-719).

training_losses on the HIP UNetModel (bare, or behind a wrapper that holds it as `.module`) is ONE autograd node: the network
input of the batch in one launch (dxmi_edm_dsm_prep), the U-Net forward of models.cm.unet_train, the per-sample terms in one
launch (dxmi_edm_dsm_loss_fwd); its backward forms d(model output) in one launch (dxmi_edm_dsm_loss_bwd) and runs the U-Net
backward.  x_t is never stored.  Any other callable model gets the reference's expressions in torch.

consistency_losses on HIP UNetModels (online, target and, for distillation, teacher: all three, else the torch expressions run) is
ONE autograd node around the online network: dxmi_cd_prep, the online training forward, per teacher evaluation (forward_inference,
eval, no grad) one dxmi_cd_solver launch, the target evaluation (no grad), dxmi_cd_loss_fwd; its backward is dxmi_cd_loss_bwd and the
U-Net backward.  The time ladder of a call is a host table (CDLevels: fp32 torch, the reference's expression, cached per (num_scales,
sigma_min, sigma_max, rho)), uploaded once per device; the kernels gather t and t2 by index.  The target runs in the mode it is in:
train mode with dropout > 0 takes the training forward with the dropout seeds the online forward just consumed (the reference restores
the RNG state between the two so that they share masks, :192,200); otherwise forward_inference.

loss_norm="pseudo-huber" with weight_schedule="ict" and an index_sampler (models.cm.resample.DiscreteLogNormalSampler) is improved
consistency training (Song and Dhariwal 2023; not in the reference): the same node, ending in dxmi_cd_huber_fwd (loss and the summed
squared difference, which the node keeps) and, backwards, dxmi_cd_huber_bwd.

denoise() keeps the reference signature for any callable `model`; neither sampler calls it on the hot path.
OpenAIDiffusion (the DxMI few-step sampler) uses the fused dxmi_edm_precond / dxmi_edm_step_fwd kernels.
karras_sample builds its schedule ONCE on the host, in fp32 torch with the reference's expressions (tables
bit-identical to the reference's), uploads it as one small device table, and runs ONE dxmi_karras_stage launch
between two network evaluations (denoised, clamp, d, the Heun / DPM-2 / Euler / ancestral update, the next step's
churn and the next preconditioned input; the clamped sample after the last evaluation).  The consistency-model samplers
and editing loops follow the same pattern with their own table (CMSchedule) and stage kernel (dxmi_cm_stage).

Host structure.  Both families run through ONE launch loop, _run_stages: a schedule (KarrasSchedule, CMSchedule) is a host table
(_HostTable: `table`, device_table) plus `launches`, one record per stage launch (last; the generator's draw there and whether it
is used; the callback's step index), the scratch buffers it needs, stage(), which launches its kernel, and callback_info().  The
loop itself knows no sampler.  karras_sample settles the sampler, builds denoiser and schedule, and ends for both families in
_sample_on_device: device, eager or hipGraph replay, the per-model graph cache _GRAPHS.  Schedules and CD levels are memoised by
_memo in plain dicts.  The two loss nodes run the U-Net through unet_train.train_forward / train_backward, which own the rule for
running its training program without an autograd ctx; _cd_loss is the consistency loss as a plain function, shared by the node
and the no-grad call.

progdist_losses on HIP UNetModels (online and teacher) is ONE autograd node around the online network in the same way (_pd_loss,
_PDLossFn): dxmi_cd_prep on the coarse ladder, the online training forward, teacher evaluation 1, dxmi_pd_solver MID, teacher
evaluation 2, dxmi_pd_solver END (target_x; x_t3 is never stored), dxmi_pd_loss_fwd; its backward is dxmi_pd_loss_bwd and the U-Net
backward.  Its levels are a host table of 2 S + 1 entries (PDLevels: the coarse ladder, then the half steps); num_scales = 1 is legal.
lpips goes through dxmi_pd_lpips_images and, backwards, dxmi_cd_lpips_bwd.  The reference has no l2-32 here: refused.
dm_generator_losses (not in the reference: Diff-Instruct / DMD / DMD2; gan_head=... adds DMD2's GAN term) trains a ONE-step generator
G(z) = D_theta(sigma_max z, sigma_max) against a frozen real and an online-trained fake denoiser; on HIP UNetModels it is ONE autograd
node around the generator (_dm_loss, _DMLossFn): dxmi_dm_gen_in, the generator's training forward, dxmi_dm_gen_prep, the two
denoisers' forward_inference, dxmi_dm_grad_fwd; its backward is dxmi_dm_gen_bwd and the U-Net backward.  dm_sample is its sampler
(dxmi_dm_gen_in, one evaluation, dxmi_dm_gen_out).  DESIGN 5.32.
sid_generator_losses (not in the reference: Score identity Distillation, Zhou et al., ICML 2024) trains the same generator with the
loss differentiated THROUGH both denoisers with respect to their input x_t (no parameter of either receives a gradient).  On HIP
UNetModels it is ONE node around the generator (_sid_loss, _SiDLossFn) whose forward already forms d loss / d x: dxmi_dm_gen_in, the
generator's training forward, dxmi_dm_gen_prep (the denoisers' time by _denoiser_time), input_forward on both denoisers, dxmi_sid_grad_fwd, input_backward on both,
dxmi_sid_join; its backward is dxmi_dm_gen_bwd and the U-Net backward, as _DMLossFn's.  DESIGN 5.34.
sida_generator_losses / sida_discriminator_losses (not in the reference: Adversarial Score identity Distillation, Zhou, Zheng et al.
2024) add a discriminator without parameters, the channel mean of the fake net's bottleneck: the generator's node (_sida_loss,
_SiDALossFn) is _SiDLossFn's with the fake net's input_forward(tap=True), dxmi_sida_map_fwd / _bwd and input_backward(d_tap=...), no
network pass more than SiD; the discriminator's node (_SiDADisLossFn) is encoder_forward, the two map launches, encoder_backward.
DESIGN 5.41.

The training_losses and consistency_losses nodes run inside a StepGraph capture (models.cm.train_util's use_graph): they read nothing back, allocate from the graph's
pool only, and their draws (randn_like, the index randint) are torch device RNG, which is graph-aware.  What a capture freezes is
what reaches the kernels by value: num_scales, the randint bound and the table pointer, so the loop keys its graph on them, and the
level table must be on the device before the capture (an upload cannot be captured: refused otherwise).  Dropout seeds are host
inputs of the graph (models/cm/unet_train.py); the target reads the online forward's device words.  loss_norm='lpips' keeps its
refusal under capture (models/cm/lpips.py).

Pairing (a deliberate restriction of the device path; the reference allows any combination): onestep and multistep run
only for a diffusion with distillation=True (boundary-condition scalings), and the EDM samplers only with distillation=False.
"""
import math
import weakref

import numpy as np
import torch

from dxmi_hip import graph as _graph
from dxmi_hip import ops
from dxmi_hip._lib import DxmiError
from .nn import append_dims, append_zero, mean_flat
from .random_util import DeterministicGenerator
from .unet_train import (encoder_backward, encoder_forward, encoder_input_backward, encoder_input_forward, input_backward,
                         input_forward, train_backward, train_forward)


def get_weightings(weight_schedule, snrs, sigma_data):
    if weight_schedule == "snr":
        weightings = snrs
    elif weight_schedule == "snr+1":
        weightings = snrs + 1
    elif weight_schedule == "karras":
        weightings = snrs + 1.0 / sigma_data ** 2
    elif weight_schedule == "truncated-snr":
        weightings = torch.clamp(snrs, min=1.0)
    elif weight_schedule == "uniform":
        weightings = torch.ones_like(snrs)
    elif weight_schedule == "ict":
        raise NotImplementedError(_ICT_PAIRING)
    else:
        raise NotImplementedError()
    return weightings


_ICT_PAIRING = ("weight_schedule='ict' (1 / (t - t2)) needs both levels of a consistency pair: it is valid only in consistency_losses "
                "with loss_norm='pseudo-huber'")
HUBER_C_PER_SQRT_DIM = 0.00054      # Song and Dhariwal 2023: c = 0.00054 sqrt(d), d the dimension of an image


def _hip_unet(model):
    """The HIP UNetModel behind `model` (itself, or a wrapper's `.module`), else None."""
    from .unet import UNetModel
    net = model.module if hasattr(model, "module") else model
    return net if isinstance(net, UNetModel) else None


class _DSMLossFn(torch.autograd.Function):
    """prep -> U-Net forward (models.cm.unet_train) -> per-sample terms, as one node; outputs (xs_mse, mse)."""

    @staticmethod
    def forward(ctx, diffusion, net, x_start, noise, sigmas, y, *params):
        F, tape = train_forward(net, *ops.edm_dsm_prep(x_start, noise, sigmas, diffusion.sigma_data), y)
        kw = dict(weight_schedule=diffusion.weight_schedule, sigma_data=diffusion.sigma_data, sigma_min=diffusion.sigma_min,
                  distillation=diffusion.distillation)
        xs, mse = ops.edm_dsm_loss_fwd(F, x_start, noise, sigmas, **kw)
        ctx.tape, ctx.F, ctx.kw, ctx.ops = tape, F, kw, (x_start, noise, sigmas)
        ctx.set_materialize_grads(False)
        return xs, mse

    @staticmethod
    def backward(ctx, g_xs, g_mse):
        n_params = len(ctx.needs_input_grad) - 6
        if g_xs is None and g_mse is None:
            return (None,) * (6 + n_params)
        x_start, noise, sigmas = ctx.ops
        cont = lambda g: None if g is None else g.detach().float().contiguous()
        dF = ops.edm_dsm_loss_bwd(cont(g_mse), cont(g_xs), ctx.F, x_start, noise, sigmas, **ctx.kw)
        ctx.F = None
        grads = train_backward(ctx.tape, dF)
        ctx.tape = None
        return (None,) * 6 + grads


class _HostTable:
    """A small fp32 table built once on the host (`table`) and uploaded once per device."""

    def __init__(self, table):
        self.table, self._dev = table, {}

    def device_table(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.table.to(device)
        return self._dev[key]

    def on_device(self, device):
        return str(device) in self._dev


def _memo(cache, key, cap, build):
    """cache[key], built on first use; a cache that has grown past `cap` entries is emptied first."""
    v = cache.get(key)
    if v is None:
        if len(cache) > cap:
            cache.clear()
        v = cache[key] = build()
    return v


class CDLevels(_HostTable):
    """The num_scales time levels of consistency_losses (reference :180-188), on the host in fp32 torch with the reference's own
    expression: `indices / (num_scales - 1)` is an int64 tensor over a python int, then `** rho`.  Bit-identical to the reference
    on the same CPU (1 ulp of pow across CPUs, as the sigma tables of the samplers).  table[i] = t of index i, table[i + 1] = t2."""

    def __init__(self, num_scales, sigma_min, sigma_max, rho):
        if int(num_scales) < 2:
            raise ValueError(f"consistency_losses: num_scales must be at least 2, got {num_scales}")
        indices = torch.arange(int(num_scales), dtype=torch.int64)
        t = sigma_max ** (1 / rho) + indices / (num_scales - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))
        super().__init__((t ** rho).to(torch.float32))
        self.num_scales = int(num_scales)


_CD_LEVELS = {}
_NO_LPIPS = ("loss_norm='lpips': no LPIPS weights are available to this package; the consistency losses run with l1, l2 and l2-32 "
             "unless DXMI_LPIPS_VGG16 and DXMI_LPIPS_LIN name the VGG16 and linear weight files (or lpips_loss= is given)")
LPIPS_RESIZE_BELOW, LPIPS_SIZE = 256, 224      # reference :222-230: images narrower than 256 go through F.interpolate(size=224)


def cd_levels(num_scales, sigma_min, sigma_max, rho):
    key = (int(num_scales), float(sigma_min), float(sigma_max), float(rho))
    return _memo(_CD_LEVELS, key, 256, lambda: CDLevels(num_scales, sigma_min, sigma_max, rho))


def _train_forward_no_grad(net, x_in, t, y, seeds=None):
    """The training forward of `net` without a tape kept (dropout applied).  seeds: the dropout seeds to use, site by site, and
    they must be consumed exactly (a net with more or fewer dropout sites is an error); None: the net draws its own."""
    if seeds is not None:
        net.__dict__["_dropout_seed_feed"] = list(seeds)
    try:
        with torch.no_grad():
            out, _ = train_forward(net, x_in, t, y)
        left = net.__dict__.get("_dropout_seed_feed")
        if left:
            raise RuntimeError(f"dropout seed hand-over: {len(left)} of {len(seeds)} seeds were not consumed (the two nets differ in "
                               "their dropout sites)")
        return out
    finally:
        net.__dict__.pop("_dropout_seed_feed", None)


def _cd_loss(diffusion, net, target, teacher, teacher_diffusion, x_start, noise, indices, tab, y, keep):
    """prep -> online U-Net forward -> solver stages around the teacher evaluations -> target evaluation -> per-sample loss.
    -> (loss, (tape, kw, operands, lpips)), the second being what _CDLossFn.backward reads.  keep=False: no backward follows, so
    LPIPS keeps no activations."""
    sd = diffusion.sigma_data
    x_t, x_in, t, x_te = ops.cd_prep(x_start, noise, indices, tab, sd, None if teacher is None else teacher_diffusion.sigma_data)
    F, tape = train_forward(net, x_in, t, y)
    seeds = list(net.dropout_seeds_used)
    if teacher is None:
        x_t2, tg_in, tg_t = ops.cd_solver(ops.CD_EULER_X0, x_t, indices, tab, x_start=x_start, next_sigma_data=sd)
    else:
        tk = dict(sigma_data=teacher_diffusion.sigma_data, sigma_min=teacher_diffusion.sigma_min,
                  distillation=teacher_diffusion.distillation)
        F1 = teacher.forward_inference(x_in if x_te is None else x_te, t, y)
        d, samples, te_in, te_t = ops.cd_solver(ops.CD_HEUN_PRED, x_t, indices, tab, model_out=F1,
                                                next_sigma_data=teacher_diffusion.sigma_data, **tk)
        F2 = teacher.forward_inference(te_in, te_t, y)
        x_t2, tg_in, tg_t = ops.cd_solver(ops.CD_HEUN_CORR, x_t, indices, tab, model_out=F2, d=d, samples=samples,
                                          next_sigma_data=sd, **tk)
    if target.training and target.dropout > 0:
        # an online forward that dropped nothing (eval mode, or dropout 0) has no masks to share: the target draws its own
        F_tg = _train_forward_no_grad(target, tg_in, tg_t, y, seeds if seeds else None)
    else:
        F_tg = target.forward_inference(tg_in, tg_t, y)
    kw = dict(loss_norm=diffusion.loss_norm, weight_schedule=diffusion.weight_schedule, sigma_data=sd,
              sigma_min=diffusion.sigma_min, distillation=diffusion.distillation)
    if diffusion.loss_norm == "lpips":
        from dxmi_hip import lpips_ops
        from .lpips import _lpips_forward
        del kw["loss_norm"]
        lp = diffusion._lpips()
        x01, w = lpips_ops.cd_lpips_images(F, F_tg, x_t, x_t2, indices, tab, **kw)
        loss, acts = _lpips_forward(lp, x01, LPIPS_SIZE if x_start.shape[-1] < LPIPS_RESIZE_BELOW else None, scale=w, keep=keep)
        return loss, (tape, kw, (indices, tab), (lp, acts, tuple(x_start.shape[2:])))
    if diffusion.loss_norm == "pseudo-huber":      # the norm travels as huber_c; ssq goes first among the saved operands
        del kw["loss_norm"]
        kw["huber_c"] = diffusion._huber_c(x_start)
        loss, ssq = ops.cd_huber_fwd(F, F_tg, x_t, x_t2, indices, tab, **kw)
        return loss, (tape, kw, (ssq, F, F_tg, x_t, x_t2, indices, tab), None)
    return ops.cd_loss_fwd(F, F_tg, x_t, x_t2, indices, tab, **kw), (tape, kw, (F, F_tg, x_t, x_t2, indices, tab), None)


class _CDLossFn(torch.autograd.Function):
    """_cd_loss as one node around the online network."""

    @staticmethod
    def forward(ctx, diffusion, net, target, teacher, teacher_diffusion, x_start, noise, indices, tab, y, *params):
        loss, (ctx.tape, ctx.kw, ctx.ops, ctx.lpips) = _cd_loss(diffusion, net, target, teacher, teacher_diffusion, x_start, noise,
                                                                indices, tab, y, keep=True)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * len(ctx.needs_input_grad)
        if ctx.lpips is not None:
            from dxmi_hip import lpips_ops
            from .lpips import _lpips_backward
            dF = lpips_ops.cd_lpips_bwd(g.detach().float().contiguous(), _lpips_backward(*ctx.lpips, None), *ctx.ops, **ctx.kw)
        elif "huber_c" in ctx.kw:
            dF = ops.cd_huber_bwd(g.detach().float().contiguous(), *ctx.ops, **ctx.kw)
        else:
            dF = ops.cd_loss_bwd(g.detach().float().contiguous(), *ctx.ops, **ctx.kw)
        ctx.ops = ctx.lpips = None
        grads = train_backward(ctx.tape, dF)
        ctx.tape = None
        return (None,) * 10 + grads


class PDLevels(_HostTable):
    """The levels of progdist_losses (reference :285-298) for num_scales = S >= 1, on the host in fp32 torch with the reference's
    own expressions: `indices / num_scales` is an int64 tensor over a python int, `indices + 0.5` a float tensor, then `** rho`.
    One table of 2 S + 1 entries: the coarse ladder arange(S + 1) / S first (t of index i = table[i], t3 = table[i + 1]: the
    reference's `(indices + 1) / num_scales` is the next coarse entry), then the half steps (arange(S) + 0.5) / S
    (t2 = table[S + 1 + i]).  Bit-identical to the reference's per-sample t, t2, t3 on the same CPU."""

    def __init__(self, num_scales, sigma_min, sigma_max, rho):
        S = int(num_scales)
        if S < 1:
            raise ValueError(f"progdist_losses: num_scales must be at least 1, got {num_scales}")
        coarse, half = torch.arange(S + 1, dtype=torch.int64), torch.arange(S, dtype=torch.int64)
        delta = sigma_min ** (1 / rho) - sigma_max ** (1 / rho)
        t = (sigma_max ** (1 / rho) + coarse / S * delta) ** rho
        t2 = (sigma_max ** (1 / rho) + (half + 0.5) / S * delta) ** rho
        super().__init__(torch.cat([t, t2]).to(torch.float32))
        self.num_scales = S

    def levels(self, indices):
        """-> (t, t2, t3) of every index, gathered on the host table's device."""
        tab, S = self.table.to(indices.device), self.num_scales
        return tab[indices], tab[S + 1 + indices], tab[indices + 1]


_PD_LEVELS = {}


def pd_levels(num_scales, sigma_min, sigma_max, rho):
    key = (int(num_scales), float(sigma_min), float(sigma_max), float(rho))
    return _memo(_PD_LEVELS, key, 256, lambda: PDLevels(num_scales, sigma_min, sigma_max, rho))


def _pd_loss(diffusion, net, teacher, teacher_diffusion, x_start, noise, indices, tab, y, keep):
    """prep -> online U-Net forward -> the two Euler stages around the teacher evaluations -> per-sample loss (reference :300-327).
    -> (loss, (tape, kw, operands, lpips)), the second being what _PDLossFn.backward reads.  tab: the 2 S + 1 levels of PDLevels;
    its first S + 1 entries are a ladder dxmi_cd_prep / dxmi_cd_lpips_bwd read as they read CDLevels."""
    sd, td = diffusion.sigma_data, teacher_diffusion
    coarse = tab[:(tab.numel() + 1) // 2]
    x_t, x_in, t, x_te = ops.cd_prep(x_start, noise, indices, coarse, sd, td.sigma_data)
    F, tape = train_forward(net, x_in, t, y)
    tk = dict(sigma_data=td.sigma_data, sigma_min=td.sigma_min, distillation=td.distillation)
    F1 = teacher.forward_inference(x_in if x_te is None else x_te, t, y)
    x_t2, te_in, te_t = ops.pd_solver(ops.PD_MID, x_t, F1, indices, tab, next_sigma_data=td.sigma_data, **tk)
    F2 = teacher.forward_inference(te_in, te_t, y)
    target_x = ops.pd_solver(ops.PD_END, x_t, F2, indices, tab, x_t2=x_t2, **tk)
    kw = dict(loss_norm=diffusion.loss_norm, weight_schedule=diffusion.weight_schedule, sigma_data=sd,
              sigma_min=diffusion.sigma_min, distillation=diffusion.distillation)
    if diffusion.loss_norm == "lpips":
        from dxmi_hip import lpips_ops
        from .lpips import _lpips_forward
        del kw["loss_norm"]
        lp = diffusion._lpips()
        x01, w = lpips_ops.pd_lpips_images(F, x_t, target_x, indices, tab, **kw)
        loss, acts = _lpips_forward(lp, x01, LPIPS_SIZE if x_start.shape[-1] < LPIPS_RESIZE_BELOW else None, scale=w, keep=keep)
        return loss, (tape, kw, (indices, coarse), (lp, acts, tuple(x_start.shape[2:])))
    return ops.pd_loss_fwd(F, x_t, target_x, indices, tab, **kw), (tape, kw, (F, x_t, target_x, indices, tab), None)


class _PDLossFn(torch.autograd.Function):
    """_pd_loss as one node around the online network."""

    @staticmethod
    def forward(ctx, diffusion, net, teacher, teacher_diffusion, x_start, noise, indices, tab, y, *params):
        loss, (ctx.tape, ctx.kw, ctx.ops, ctx.lpips) = _pd_loss(diffusion, net, teacher, teacher_diffusion, x_start, noise, indices,
                                                                tab, y, keep=True)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * len(ctx.needs_input_grad)
        if ctx.lpips is not None:
            from dxmi_hip import lpips_ops
            from .lpips import _lpips_backward
            dF = lpips_ops.cd_lpips_bwd(g.detach().float().contiguous(), _lpips_backward(*ctx.lpips, None), *ctx.ops, **ctx.kw)
        else:
            dF = ops.pd_loss_bwd(g.detach().float().contiguous(), *ctx.ops, **ctx.kw)
        ctx.ops = ctx.lpips = None
        grads = train_backward(ctx.tape, dF)
        ctx.tape = None
        return (None,) * 9 + grads


# ------------------------------------------------------------------------------------------------- distribution matching
DM_WEIGHTINGS = ("dmd", "none")


def dm_index_range(num_scales, min_step_frac=0.02, max_step_frac=0.98):
    """-> (lo, hi), both inclusive: the ladder indices dm_generator_losses draws from, [ceil(min (S - 1)), floor(max (S - 1))]
    (DMD's EDM runs: the middle 96 % of a 1000-level Karras ladder)."""
    S = int(num_scales)
    if not (0.0 <= min_step_frac <= max_step_frac <= 1.0):
        raise ValueError(f"dm_generator_losses: need 0 <= min_step_frac <= max_step_frac <= 1, got {min_step_frac}, {max_step_frac}")
    lo, hi = math.ceil(min_step_frac * (S - 1)), math.floor(max_step_frac * (S - 1))
    if lo > hi:
        raise ValueError(f"dm_generator_losses: no ladder index of {S} levels lies in [{min_step_frac}, {max_step_frac}] (S - 1)")
    return lo, hi


class GenLadder(_HostTable):
    """The levels sigma_0 > ... > sigma_{K-1} > 0 of a K-step generator (DMD2, Yin et al. 2024, section 4.4), as fp32 values:
    `sigmas` (python floats that are exactly the fp32 entries) and `table`, fp32 [K]."""

    def __init__(self, what, gen_sigmas):
        try:
            vals = [float(v) for v in gen_sigmas]
        except TypeError:
            raise ValueError(f"{what}: gen_sigmas must be a sequence of levels, got {gen_sigmas!r}") from None
        if not vals:
            raise ValueError(f"{what}: gen_sigmas must hold at least one level")
        if not all(math.isfinite(v) and v > 0 for v in vals):
            raise ValueError(f"{what}: every level of gen_sigmas must be positive and finite, got {vals}")
        table = torch.tensor(vals, dtype=torch.float64).to(torch.float32)
        self.sigmas = tuple(float(v) for v in table)
        if not all(math.isfinite(v) and v > 0 for v in self.sigmas) or any(a <= b for a, b in zip(self.sigmas, self.sigmas[1:])):
            raise ValueError(f"{what}: gen_sigmas must decrease strictly (as fp32 values) and stay positive and finite, got {vals}")
        super().__init__(table)

    def __len__(self):
        return len(self.sigmas)


_GEN_LADDERS = {}


def gen_ladder(what, gen_sigmas):
    """gen_sigmas checked -> its GenLadder (one per ladder: the device table is uploaded once)."""
    if isinstance(gen_sigmas, GenLadder):
        return gen_sigmas
    if torch.is_tensor(gen_sigmas):
        gen_sigmas = gen_sigmas.detach().reshape(-1).tolist()
    try:
        key = tuple(float(v) for v in gen_sigmas)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: gen_sigmas must be a sequence of levels, got {gen_sigmas!r}") from None
    return _memo(_GEN_LADDERS, key, 64, lambda: GenLadder(what, key))


def dm_step_sigmas(K, sigma_hi, sigma_lo, rho=7.0):
    """The Karras-spaced ladder of a K-step generator between its two ends -> K fp32 values as python floats, sigma_hi first:
    (hi^(1/rho) + j / (K - 1) (lo^(1/rho) - hi^(1/rho)))^rho; K = 1 gives (sigma_hi,).  A convenience: no ladder here is tuned."""
    K, hi, lo, rho = int(K), float(sigma_hi), float(sigma_lo), float(rho)
    if K < 1:
        raise ValueError(f"dm_step_sigmas: K must be at least 1, got {K}")
    if not (math.isfinite(hi) and math.isfinite(lo) and 0 < lo <= hi and math.isfinite(rho) and rho > 0) or (K > 1 and lo == hi):
        raise ValueError(f"dm_step_sigmas: need 0 < sigma_lo < sigma_hi (finite; equal ends only for K = 1) and rho > 0, got "
                         f"{sigma_hi}, {sigma_lo}, rho {rho}")
    a, b = hi ** (1 / rho), lo ** (1 / rho)
    vals = [(a + (j / (K - 1) if K > 1 else 0.0) * (b - a)) ** rho for j in range(K)]
    return gen_ladder("dm_step_sigmas", vals).sigmas


class _GenSteps:
    """What stands where gen_sigma stood in _dm_loss and its nodes when the generator has K > 1 steps: the ladder's device table,
    the per-image graded steps (int64 [N] on the device) and the simulation noise [K - 1, N, C, H, W]."""

    def __init__(self, tab, steps, sim_noise):
        self.tab, self.steps, self.sim_noise = tab, steps, sim_noise


def _dm_gen_bwd(up, g, gen, sigma_data):
    """dm_gen_bwd at sigma_G, or dmms_bwd at every image's own level."""
    if isinstance(gen, _GenSteps):
        return ops.dmms_bwd(up, g, gen.steps, gen.tab, sigma_data)
    return ops.dm_gen_bwd(up, g, gen, sigma_data)


class _DMSurrogate(torch.autograd.Function):
    """The distribution-matching term of x for the stop-gradient direction g (DMD eq. 7): the value is 0.5 mean_flat(g^2), the
    gradient d loss_n / d x = g_n / CHW, that of the surrogate 0.5 mean_flat((x - sg(x - g))^2) without its rounding of x - (x - g)."""

    @staticmethod
    def forward(ctx, x, g):
        ctx.save_for_backward(g)
        return 0.5 * mean_flat(g ** 2)

    @staticmethod
    def backward(ctx, up):
        g, = ctx.saved_tensors
        return append_dims(up, g.ndim) * g / g[0].numel(), None


class _SiDSurrogate(torch.autograd.Function):
    """The value `loss` of sid_generator_losses' torch path with the gradient already taken: d loss_n / d x = g_n / CHW."""

    @staticmethod
    def forward(ctx, x, g, loss):
        ctx.save_for_backward(g)
        return loss.clone()

    @staticmethod
    def backward(ctx, up):
        g, = ctx.saved_tensors
        return append_dims(up, g.ndim) * g / g[0].numel(), None, None


def _scal_kw(d):
    return dict(sigma_data=d.sigma_data, sigma_min=d.sigma_min, distillation=d.distillation)


def _dm_gen_forward(diffusion, net, z, y, gen_sigma, keep):
    """dm_gen_in -> the generator's forward -> (F, tape, None); keep=False as in _dm_loss.
    gen_sigma a _GenSteps: backward simulation (DMD2 section 4.5) -> (F, tape, x_k).  dmms_in, then K - 1 x (the no-grad forward of
    the whole batch, dmms_stage: images whose step is reached are frozen), which leaves x_k[n] = x_{k_n} and the graded
    evaluation's input and time in place; no tape is kept before the graded evaluation."""
    def no_grad_forward(x_in, t_g):
        return _train_forward_no_grad(net, x_in, t_g, y) if net.training and net.dropout > 0 else net.forward_inference(x_in, t_g, y)
    x_k = None
    if isinstance(gen_sigma, _GenSteps):
        ms = gen_sigma
        x_k, x_in, t_g = ops.dmms_in(z, ms.tab, diffusion.sigma_data)
        for j in range(ms.tab.numel() - 1):
            ops.dmms_stage(no_grad_forward(x_in, t_g), j, ms.tab, x_k, x_in, t_g, steps=ms.steps, eps=ms.sim_noise[j],
                           sigma_data=diffusion.sigma_data)
    else:
        x_in, t_g = ops.dm_gen_in(z, gen_sigma, diffusion.sigma_data)
    if keep:
        return train_forward(net, x_in, t_g, y) + (x_k,)
    return no_grad_forward(x_in, t_g), None, x_k


def _dm_gen_prep(diffusion, F, z, x_k, noise, indices, tab, gen_sigma, sdr, sdf):
    """dm_gen_prep at sigma_G, or dmms_prep on the simulated states x_k at every image's own level."""
    if isinstance(gen_sigma, _GenSteps):
        return ops.dmms_prep(F, x_k, noise, gen_sigma.steps, gen_sigma.tab, indices, tab, diffusion.sigma_data, sdr, sdf)
    return ops.dm_gen_prep(F, z, noise, indices, tab, gen_sigma, diffusion.sigma_data, sdr, sdf)


def _dm_gan_term(fake, fake_diffusion, x, g, tab, y, gan, keep):
    """DMD2's GAN term of the generator on the device -> (gan_loss [N], gan_logit [N]); with keep, g becomes the combined direction
    g + CHW w c_in(t_gan) d_xin in place: the fake net's encoder_input_forward, the head's features and dxmi_gan_logit_loss, the
    head's input-only backward, encoder_input_backward and dxmi_gan_join.  Both tapes are dropped here."""
    head, w, gan_noise, gan_indices = gan
    x_in, _ = ops.edm_dsm_prep(x, gan_noise, tab[gan_indices], fake_diffusion.sigma_data)
    h, etape = encoder_input_forward(fake, x_in, _denoiser_time(tab, gan_indices), y)
    with torch.no_grad():
        a2, saved = head.features(h)
        sign = torch.full((x.shape[0],), -1.0, dtype=torch.float32, device=x.device)
        logit, gan_loss = head.logit_loss(a2, sign)
        if keep:
            d_h, _ = head.backward(saved, sign, logit, torch.ones_like(sign), 1.0, params=False)
            d_xin = encoder_input_backward(etape, d_h)
            ops.gan_join(g, d_xin, gan_indices, tab, w, fake_diffusion.sigma_data, out=g)
    return gan_loss, logit


def _dm_loss(diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y, gen_sigma, weighting, keep, gan=None):
    """dm_gen_in -> generator forward -> dm_gen_prep -> the real and the fake denoiser -> dm_grad_fwd.
    -> (loss, x, s, (tape, g)), the last being what _DMLossFn.backward reads.  keep=False: no backward follows, so the generator
    runs forward_inference (the training forward where its dropout is live) and no tape is kept.
    gan = (head, weight, gan_noise, gan_indices): DMD2's GAN term (_dm_gan_term) joins the loss and the direction, and the result
    gains (gan_loss, gan_logit).  gen_sigma a _GenSteps: the K-step generator (_dm_gen_forward); from x on nothing differs."""
    F, tape, x_k = _dm_gen_forward(diffusion, net, z, y, gen_sigma, keep)
    x, x_t, xr_in, t, xf_in = _dm_gen_prep(diffusion, F, z, x_k, noise, indices, tab, gen_sigma, real_diffusion.sigma_data,
                                           fake_diffusion.sigma_data)
    F_r = real.forward_inference(xr_in, t, y)
    F_f = fake.forward_inference(xr_in if xf_in is None else xf_in, t, y)
    g, loss, s = ops.dm_grad_fwd(F_r, F_f, x, x_t, indices, tab, weighting, real=_scal_kw(real_diffusion), fake=_scal_kw(fake_diffusion))
    if gan is None:
        return loss, x, s, (tape, g)
    gan_loss, gan_logit = _dm_gan_term(fake, fake_diffusion, x, g, tab, y, gan, keep)
    return loss + gan[1] * gan_loss, x, s, (tape, g), gan_loss, gan_logit


class _DMLossFn(torch.autograd.Function):
    """_dm_loss as one node around the generator; outputs (loss, x, dm_norm), of which only loss is differentiable."""

    @staticmethod
    def forward(ctx, diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y, gen_sigma, weighting, *params):
        loss, x, s, (ctx.tape, ctx.g) = _dm_loss(diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y,
                                                 gen_sigma, weighting, keep=True)
        ctx.gen = (gen_sigma, diffusion.sigma_data)
        ctx.mark_non_differentiable(x, s)
        ctx.set_materialize_grads(False)
        return loss, x, s

    @staticmethod
    def backward(ctx, g_loss, g_x, g_s):
        if g_loss is None:
            return (None,) * len(ctx.needs_input_grad)
        dF = _dm_gen_bwd(g_loss.detach().float().contiguous(), ctx.g, *ctx.gen)
        ctx.g = None
        grads = train_backward(ctx.tape, dF)
        ctx.tape = None
        return (None,) * (len(ctx.needs_input_grad) - len(grads)) + grads


class _DMGanLossFn(torch.autograd.Function):
    """_DMLossFn with DMD2's GAN term: outputs (loss, x, dm_norm, gan_loss, gan_logit), of which only loss is differentiable.  The
    forward has walked the fake net's encoder and the head backward already (the shape of _SiDLossFn); the backward is _DMLossFn's."""

    @staticmethod
    def forward(ctx, diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y, gen_sigma, weighting, gan, *params):
        loss, x, s, (ctx.tape, ctx.g), gan_loss, gan_logit = _dm_loss(diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise,
                                                                      indices, tab, y, gen_sigma, weighting, keep=True, gan=gan)
        ctx.gen = (gen_sigma, diffusion.sigma_data)
        ctx.mark_non_differentiable(x, s, gan_loss, gan_logit)
        ctx.set_materialize_grads(False)
        return loss, x, s, gan_loss, gan_logit

    @staticmethod
    def backward(ctx, g_loss, *rest):
        return _DMLossFn.backward(ctx, g_loss, None, None)


class _GANDisLossFn(torch.autograd.Function):
    """The discriminator loss of DMD2's GAN term as one node around the fake net's encoder and the head: encoder_forward, the head's
    features and dxmi_gan_logit_loss forward; the head's full backward, then encoder_backward.  x holds the generated half first;
    outputs (loss [N], logit_fake [N], logit_real [N])."""

    @staticmethod
    def forward(ctx, diffusion, net, head, x, noise, indices, tab, y, *params):
        N = x.shape[0] // 2
        x_in, _ = ops.edm_dsm_prep(x, noise, tab[indices], diffusion.sigma_data)
        h, ctx.tape = encoder_forward(net, x_in, _denoiser_time(tab, indices), y)
        a2, saved = head.features(h)
        sign = torch.ones(2 * N, dtype=torch.float32, device=x.device)
        sign[N:] = -1.0
        logit, loss = head.logit_loss(a2, sign)
        ctx.head, ctx.saved, ctx.sign, ctx.logit = head, saved, sign, logit
        ctx.set_materialize_grads(False)
        lf, lr = logit[:N].clone(), logit[N:].clone()
        ctx.mark_non_differentiable(lf, lr)
        return loss[:N] + loss[N:], lf, lr

    @staticmethod
    def backward(ctx, g_loss, g_lf, g_lr):
        if g_loss is None:
            return (None,) * len(ctx.needs_input_grad)
        up = g_loss.detach().float().contiguous()
        d_h, head_grads = ctx.head.backward(ctx.saved, ctx.sign, ctx.logit, torch.cat([up, up]), 1.0, params=True)
        ctx.saved = None
        grads = encoder_backward(ctx.tape, d_h)
        ctx.tape = None
        return (None,) * 8 + grads + head_grads


def _denoiser_time(tab, indices):
    """The time input 250 ln(t + 1e-44) of both denoisers at t = tab[indices], by denoise()'s own torch expression on the device.
    dxmi_dm_gen_prep's logf and torch.log differ in the last bit at some levels (neither is the correctly rounded one throughout),
    and the bf16 nets turn one ulp of time into output differences of 1e-3 relative; with this the node and the torch path on
    the same device evaluate the denoisers at bitwise the same point.  An index outside the table is clamped here: its x_t is NaN
    already."""
    return 1000 * 0.25 * torch.log(tab[indices.clamp(0, tab.numel() - 1)] + 1e-44)


def _sid_loss(diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y, gen_sigma, alpha, keep):
    """Score identity distillation around the generator -> (loss, x, s, (tape, g)).  keep=True: both denoisers run input_forward,
    dxmi_sid_grad_fwd forms their cotangents, input_backward walks each tape (dropped at once), dxmi_sid_join forms g = CHW
    d loss / d x, which _SiDLossFn.backward hands to dxmi_dm_gen_bwd.  keep=False: no backward follows: the generator as in
    _dm_loss(keep=False), the denoisers' forward_inference, and only loss, x and s are formed."""
    F, tape, _ = _dm_gen_forward(diffusion, net, z, y, gen_sigma, keep)
    sdr, sdf = real_diffusion.sigma_data, fake_diffusion.sigma_data
    x, x_t, xr_in, _, xf_in = ops.dm_gen_prep(F, z, noise, indices, tab, gen_sigma, diffusion.sigma_data, sdr, sdf)
    xf_in = xr_in if xf_in is None else xf_in
    t = _denoiser_time(tab, indices)
    if keep:
        F_r, tape_r = input_forward(real, xr_in, t, y)
        F_f, tape_f = input_forward(fake, xf_in, t, y)
    else:
        F_r, F_f = real.forward_inference(xr_in, t, y), fake.forward_inference(xf_in, t, y)
    v_r, v_f, d_dir, loss, s = ops.sid_grad_fwd(F_r, F_f, x, x_t, indices, tab, alpha, real=_scal_kw(real_diffusion),
                                                fake=_scal_kw(fake_diffusion))
    if not keep:
        return loss, x, s, (None, None)
    g_r = input_backward(tape_r, v_r)
    del tape_r, v_r
    g_f = input_backward(tape_f, v_f)
    del tape_f, v_f
    g = ops.sid_join(d_dir, g_r, g_f, s, indices, tab, sdr, sdf, out=d_dir)
    return loss, x, s, (tape, g)


class _SiDLossFn(torch.autograd.Function):
    """_sid_loss as one node around the generator; outputs (loss, x, dm_norm), of which only loss is differentiable.  The forward
    has walked both denoisers backward already; the backward is _DMLossFn's."""

    @staticmethod
    def forward(ctx, diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y, gen_sigma, alpha, *params):
        loss, x, s, (ctx.tape, ctx.g) = _sid_loss(diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y,
                                                  gen_sigma, alpha, keep=True)
        ctx.gen = (gen_sigma, diffusion.sigma_data)
        ctx.mark_non_differentiable(x, s)
        ctx.set_materialize_grads(False)
        return loss, x, s

    backward = staticmethod(_DMLossFn.backward)


def _sida_value(loss_sid, adv, s, weight):
    """loss_n = sid_n + weight adv_n / s_n, 0 where s_n == 0 (a few [N]-sized expressions)."""
    live = s != 0
    return torch.where(live, loss_sid + weight * adv / torch.where(live, s, torch.ones_like(s)), torch.zeros_like(s))


def _sida_loss(diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y, gen_sigma, alpha, weight, keep):
    """_sid_loss with SiDA's adversarial term from the SAME evaluation of the fake net -> (loss, x, s, (tape, g), adv_loss [N],
    adv_logit [N, P]).  The fake net runs input_forward(tap=True): its bottleneck h feeds dxmi_sida_map_fwd (logit, adv = a(-1)),
    dxmi_sida_map_bwd forms the cotangent d_h = -(CHW weight) sigmoid(-logit) / (P Cb) without the 1 / s, and the fake net's ONE
    input_backward takes v_f at the output and d_h at the bottleneck; dxmi_sid_join's 1 / s covers both (the net is linear in its
    cotangents).  No network pass is added to _sid_loss.  keep=False: the fake net still runs input_forward(tap=True) (its tape is
    dropped), so that adv_loss and adv_logit are formed and F_f has the bits of the graded call."""
    F, tape, _ = _dm_gen_forward(diffusion, net, z, y, gen_sigma, keep)
    sdr, sdf = real_diffusion.sigma_data, fake_diffusion.sigma_data
    x, x_t, xr_in, _, xf_in = ops.dm_gen_prep(F, z, noise, indices, tab, gen_sigma, diffusion.sigma_data, sdr, sdf)
    xf_in = xr_in if xf_in is None else xf_in
    t = _denoiser_time(tab, indices)
    if keep:
        F_r, tape_r = input_forward(real, xr_in, t, y)
    else:
        F_r = real.forward_inference(xr_in, t, y)
    F_f, tape_f = input_forward(fake, xf_in, t, y, tap=True)
    h = tape_f.bottleneck
    v_r, v_f, d_dir, loss, s = ops.sid_grad_fwd(F_r, F_f, x, x_t, indices, tab, alpha, real=_scal_kw(real_diffusion),
                                                fake=_scal_kw(fake_diffusion))
    logit, adv = ops.sida_map_fwd(h, -1)
    loss = _sida_value(loss, adv, s, weight)
    if not keep:
        return loss, x, s, (None, None), adv, logit
    d_h = ops.sida_map_bwd(logit, -1, x[0].numel() * weight, h.shape[-1], shape=h.shape)
    del h
    g_r = input_backward(tape_r, v_r)
    del tape_r, v_r
    g_f = input_backward(tape_f, v_f, d_tap=d_h)
    del tape_f, v_f, d_h
    g = ops.sid_join(d_dir, g_r, g_f, s, indices, tab, sdr, sdf, out=d_dir)
    return loss, x, s, (tape, g), adv, logit


class _SiDALossFn(torch.autograd.Function):
    """_sida_loss as one node around the generator; outputs (loss, x, dm_norm, adv_loss, adv_logit), of which only loss is
    differentiable.  The forward has walked both denoisers backward already; the backward is _DMLossFn's."""

    @staticmethod
    def forward(ctx, diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y, gen_sigma, alpha, weight,
                *params):
        loss, x, s, (ctx.tape, ctx.g), adv, logit = _sida_loss(diffusion, net, real, real_diffusion, fake, fake_diffusion, z, noise,
                                                               indices, tab, y, gen_sigma, alpha, weight, keep=True)
        ctx.gen = (gen_sigma, diffusion.sigma_data)
        ctx.mark_non_differentiable(x, s, adv, logit)
        ctx.set_materialize_grads(False)
        return loss, x, s, adv, logit

    @staticmethod
    def backward(ctx, g_loss, *rest):
        return _DMLossFn.backward(ctx, g_loss, None, None)


class _SiDADisLossFn(torch.autograd.Function):
    """SiDA's discriminator loss as one node around the fake net's encoder: encoder_forward and dxmi_sida_map_fwd forward;
    dxmi_sida_map_bwd, then encoder_backward.  x holds the generated half first; outputs (loss [N], logit_fake [N, P],
    logit_real [N, P]).  The map has no parameters: every gradient is one of the fake net's."""

    @staticmethod
    def forward(ctx, diffusion, net, x, noise, indices, tab, y, *params):
        N = x.shape[0] // 2
        x_in, _ = ops.edm_dsm_prep(x, noise, tab[indices], diffusion.sigma_data)
        h, ctx.tape = encoder_forward(net, x_in, _denoiser_time(tab, indices), y)
        ctx.sign = [1] * N + [-1] * N
        ctx.logit, a = ops.sida_map_fwd(h, ctx.sign)
        ctx.h_shape = tuple(h.shape)
        ctx.set_materialize_grads(False)
        lf, lr = ctx.logit[:N].clone(), ctx.logit[N:].clone()
        ctx.mark_non_differentiable(lf, lr)
        return a[:N] + a[N:], lf, lr

    @staticmethod
    def backward(ctx, g_loss, g_lf, g_lr):
        if g_loss is None:
            return (None,) * len(ctx.needs_input_grad)
        up = g_loss.detach().float().contiguous()
        d_h = ops.sida_map_bwd(ctx.logit, ctx.sign, 1.0, ctx.h_shape[-1], upstream=torch.cat([up, up]), shape=ctx.h_shape)
        ctx.logit = None
        grads = encoder_backward(ctx.tape, d_h)
        ctx.tape = None
        return (None,) * 7 + grads


class KarrasDenoiser:
    def __init__(self, sigma_data: float = 0.5, sigma_max=80.0, sigma_min=0.002, rho=7.0, weight_schedule="karras",
                 distillation=False, loss_norm="l2", lpips_loss=None, huber_c=None):
        """huber_c: the constant of loss_norm="pseudo-huber"; None: 0.00054 sqrt(C H W) of the x_start of a call."""
        self.sigma_data, self.sigma_max, self.sigma_min = sigma_data, sigma_max, sigma_min
        self.weight_schedule, self.distillation, self.loss_norm, self.rho = weight_schedule, distillation, loss_norm, rho
        self.lpips_loss = lpips_loss
        self.huber_c = huber_c
        if huber_c is not None:
            self._huber_c(None)
        if loss_norm == "lpips":
            self._lpips()

    def _huber_c(self, x_start):
        """The pseudo-Huber constant of a call on x_start (set on the object after construction too, so checked at every use)."""
        c = self.huber_c
        if c is None:
            return HUBER_C_PER_SQRT_DIM * math.sqrt(x_start[0].numel())
        c = float(c)
        if not (math.isfinite(c) and c > 0):
            raise ValueError(f"huber_c must be finite and > 0 (None: {HUBER_C_PER_SQRT_DIM} sqrt(C H W)), got {self.huber_c!r}")
        return c

    def _refuse_ict(self, where):
        if self.weight_schedule == "ict":
            raise NotImplementedError(f"{where}: {_ICT_PAIRING}")

    def _lpips(self):
        """The LPIPS object of loss_norm='lpips': `lpips_loss` if set, else the one the two environment variables name (built once)."""
        if self.lpips_loss is None:
            from .lpips import LPIPS
            self.lpips_loss = LPIPS.from_env()
        if self.lpips_loss is None:
            raise NotImplementedError(_NO_LPIPS)
        return self.lpips_loss

    def get_snr(self, sigmas):
        return sigmas ** -2

    def get_sigmas(self, sigmas):
        return sigmas

    def get_scalings(self, sigma):
        c_skip = self.sigma_data ** 2 / (sigma ** 2 + self.sigma_data ** 2)
        c_out = sigma * self.sigma_data / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        c_in = 1 / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        return c_skip, c_out, c_in

    def get_scalings_for_boundary_condition(self, sigma):
        c_skip = self.sigma_data ** 2 / ((sigma - self.sigma_min) ** 2 + self.sigma_data ** 2)
        c_out = (sigma - self.sigma_min) * self.sigma_data / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        c_in = 1 / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        return c_skip, c_out, c_in

    def training_losses(self, model, x_start, sigmas, model_kwargs=None, noise=None):
        """DSM terms per sample (reference :82-106): xs_mse = mean_flat((denoised - x_start)^2), mse = the same weighted by
        get_weightings(weight_schedule, sigma^-2, sigma_data), loss = mse."""
        if model_kwargs is None:
            model_kwargs = {}
        if noise is None:
            noise = torch.randn_like(x_start)
        self._refuse_ict("training_losses")
        net = _hip_unet(model)
        if net is not None and x_start.is_cuda:
            return self._training_losses_hip(net, x_start, sigmas, model_kwargs, noise)
        terms = {}
        dims = x_start.ndim
        x_t = x_start + noise * append_dims(sigmas, dims)
        model_output, denoised = self.denoise(model, x_t, sigmas, **model_kwargs)
        snrs = self.get_snr(sigmas)
        weights = append_dims(get_weightings(self.weight_schedule, snrs, self.sigma_data), dims)
        terms["xs_mse"] = mean_flat((denoised - x_start) ** 2)
        terms["mse"] = mean_flat(weights * (denoised - x_start) ** 2)
        terms["loss"] = terms["mse"]
        return terms

    def _training_losses_hip(self, net, x_start, sigmas, model_kwargs, noise):
        if x_start.requires_grad or sigmas.requires_grad or noise.requires_grad:
            raise NotImplementedError("training_losses on the HIP U-Net differentiates the network parameters only: x_start, "
                                      "noise and sigmas must not require grad")
        extra = set(model_kwargs) - {"y"}
        if extra:
            raise NotImplementedError(f"training_losses on the HIP U-Net: model_kwargs {sorted(extra)} are not inputs of UNetModel")
        y = model_kwargs.get("y")
        if (y is not None) != (net.num_classes is not None):
            raise ValueError("must specify y if and only if the model is class-conditional")
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        x_start, noise, sigmas = f32(x_start), f32(noise), f32(sigmas).reshape(-1)
        if noise.shape != x_start.shape or sigmas.numel() != x_start.shape[0]:
            raise ValueError(f"training_losses: noise {tuple(noise.shape)} must match x_start {tuple(x_start.shape)} and sigmas "
                             f"({sigmas.numel()}) hold one level per sample")
        if torch.is_grad_enabled():
            xs, mse = _DSMLossFn.apply(self, net, x_start, noise, sigmas, y, *ops.fast_parameters(net))
        else:
            x_in, t = ops.edm_dsm_prep(x_start, noise, sigmas, self.sigma_data)
            # dropout is part of the loss in train mode: the training forward applies it
            F = train_forward(net, x_in, t, y)[0] if net.training and net.dropout > 0 else net.forward_inference(x_in, t, y)
            xs, mse = ops.edm_dsm_loss_fwd(F, x_start, noise, sigmas, self.weight_schedule, self.sigma_data, self.sigma_min,
                                           self.distillation)
        return {"xs_mse": xs, "mse": mse, "loss": mse}

    def consistency_losses(self, model, x_start, num_scales, model_kwargs=None, target_model=None, teacher_model=None,
                           teacher_diffusion=None, noise=None, indices=None, generator=None, index_sampler=None):
        """Consistency distillation (teacher_model given: the Heun step through teacher_diffusion) or consistency training
        (teacher_model None: the Euler step with denoiser = x_start) loss per sample (reference :108-241) -> {"loss": [N]}.
        indices: the ladder index of every sample (the reference draws th.randint(0, num_scales - 1, (N,)) inside; drawn here,
        from `generator` if given, when None; by index_sampler.sample_indices(num_scales, N, device, generator) where a sampler is
        given, e.g. models.cm.resample.DiscreteLogNormalSampler).
        loss_norm="pseudo-huber" (not in the reference: Song and Dhariwal 2023) is w s / (sqrt(s + c^2) + c) with s the SUM of the
        squared difference over the image and c = huber_c; weight_schedule="ict", w = 1 / (t - t2), goes with this norm only."""
        if model_kwargs is None:
            model_kwargs = {}
        if noise is None:
            noise = torch.randn_like(x_start)
        if target_model is None:
            raise NotImplementedError("Must have a target model")
        if self.loss_norm == "lpips":        # set on the object after construction, as the reference's callers set it
            self._lpips()
        if self.loss_norm not in ("l1", "l2", "l2-32", "lpips", "pseudo-huber"):
            raise ValueError(f"Unknown loss norm {self.loss_norm}")
        if self.loss_norm == "pseudo-huber":
            huber_c = self._huber_c(x_start)
        else:
            self._refuse_ict(f"consistency_losses with loss_norm={self.loss_norm!r}")
        if teacher_model is not None and teacher_diffusion is None:
            raise ValueError("consistency_losses: a teacher_model needs its teacher_diffusion")
        N = x_start.shape[0]
        if indices is None and index_sampler is not None:
            indices = index_sampler.sample_indices(num_scales, N, x_start.device, generator)
        if indices is None:
            if generator is not None:
                indices = torch.randint(0, num_scales - 1, (N,), generator=generator, device=generator.device).to(x_start.device)
            else:
                indices = torch.randint(0, num_scales - 1, (N,), device=x_start.device)
        nets = [_hip_unet(m) for m in (model, target_model) + ((teacher_model,) if teacher_model is not None else ())]
        if all(n is not None for n in nets) and x_start.is_cuda:
            return self._consistency_losses_hip(nets, x_start, num_scales, model_kwargs, teacher_diffusion, noise, indices)

        dims = x_start.ndim
        levels = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho).table.to(x_start.device)
        indices = indices.to(x_start.device)
        t, t2 = levels[indices], levels[indices + 1]

        @torch.no_grad()
        def teacher_denoise_fn(x, s):
            return teacher_diffusion.denoise(teacher_model, x, s, **model_kwargs)[1]

        x_t = x_start + noise * append_dims(t, dims)
        dropout_state = torch.get_rng_state()
        distiller = self.denoise(model, x_t, t, **model_kwargs)[1]
        with torch.no_grad():
            x = x_t
            denoiser = x_start if teacher_model is None else teacher_denoise_fn(x, t)
            d = (x - denoiser) / append_dims(t, dims)
            samples = x + d * append_dims(t2 - t, dims)
            if teacher_model is not None:                   # heun_solver (:144-162); euler_solver (:164-174) ends above
                denoiser = teacher_denoise_fn(samples, t2)
                next_d = (samples - denoiser) / append_dims(t2, dims)
                samples = x + (d + next_d) * append_dims((t2 - t) / 2, dims)
            x_t2 = samples.detach()
            torch.set_rng_state(dropout_state)
            distiller_target = self.denoise(target_model, x_t2, t2, **model_kwargs)[1].detach()

        weights = 1 / (t - t2) if self.weight_schedule == "ict" else get_weightings(self.weight_schedule, self.get_snr(t), self.sigma_data)
        if self.loss_norm == "l1":
            diffs = torch.abs(distiller - distiller_target)
        elif self.loss_norm == "l2":
            diffs = (distiller - distiller_target) ** 2
        elif self.loss_norm == "pseudo-huber":     # s / (sqrt(s + c^2) + c) = sqrt(s + c^2) - c, without its cancellation at s << c^2
            diffs = (distiller - distiller_target) ** 2
            s = diffs.flatten(1).sum(1)
            return {"loss": s / (torch.sqrt(s + huber_c ** 2) + huber_c) * weights}
        elif self.loss_norm == "lpips":
            resize = LPIPS_SIZE if x_start.shape[-1] < LPIPS_RESIZE_BELOW else None
            return {"loss": self._lpips()((distiller + 1) / 2.0, (distiller_target + 1) / 2.0, resize=resize) * weights}
        else:
            import torch.nn.functional as F
            distiller = F.interpolate(distiller, size=32, mode="bilinear")
            distiller_target = F.interpolate(distiller_target, size=32, mode="bilinear")
            diffs = (distiller - distiller_target) ** 2
        return {"loss": mean_flat(diffs) * weights}

    def progdist_losses(self, model, x_start, num_scales, model_kwargs=None, teacher_model=None, teacher_diffusion=None, noise=None,
                        indices=None, generator=None):
        """Progressive distillation loss per sample (reference :243-335) -> {"loss": [N]}: the student's denoised x at t against
        the denoiser that one Euler step from t to t3 would need to land where the teacher's two Euler steps t -> t2 -> t3 land.
        indices: the ladder index of every sample in [0, num_scales - 1] (the reference draws th.randint(0, num_scales, (N,))
        inside; drawn here, from `generator` if given, when None).  num_scales = 1 is legal (the schedule's last phase)."""
        if model_kwargs is None:
            model_kwargs = {}
        if noise is None:
            noise = torch.randn_like(x_start)
        if teacher_model is None or teacher_diffusion is None:
            raise NotImplementedError("progdist_losses: Must have a teacher model and its teacher_diffusion")
        if self.loss_norm == "lpips":        # set on the object after construction, as the reference's callers set it
            self._lpips()
        if self.loss_norm not in ("l1", "l2", "lpips"):      # no l2-32 here: the reference's else branch (:328-329); no pseudo-huber
            raise ValueError(f"Unknown loss norm {self.loss_norm}")
        self._refuse_ict("progdist_losses")
        N = x_start.shape[0]
        if indices is None:
            if generator is not None:
                indices = torch.randint(0, num_scales, (N,), generator=generator, device=generator.device).to(x_start.device)
            else:
                indices = torch.randint(0, num_scales, (N,), device=x_start.device)
        nets = [_hip_unet(m) for m in (model, teacher_model)]
        if all(n is not None for n in nets) and x_start.is_cuda:
            return self._progdist_losses_hip(nets, x_start, num_scales, model_kwargs, teacher_diffusion, noise, indices)

        dims = x_start.ndim
        t, t2, t3 = pd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho).levels(indices.to(x_start.device))

        @torch.no_grad()
        def euler_solver(x, s, next_s):
            denoiser = teacher_diffusion.denoise(teacher_model, x, s, **model_kwargs)[1]
            d = (x - denoiser) / append_dims(s, dims)
            return x + d * append_dims(next_s - s, dims)

        x_t = x_start + noise * append_dims(t, dims)
        denoised_x = self.denoise(model, x_t, t, **model_kwargs)[1]
        with torch.no_grad():
            x_t2 = euler_solver(x_t, t, t2).detach()
            x_t3 = euler_solver(x_t2, t2, t3).detach()
            target_x = (x_t - append_dims(t, dims) * (x_t3 - x_t) / append_dims(t3 - t, dims)).detach()     # euler_to_denoiser
        weights = get_weightings(self.weight_schedule, self.get_snr(t), self.sigma_data)
        if self.loss_norm == "l1":
            diffs = torch.abs(denoised_x - target_x)
        elif self.loss_norm == "l2":
            diffs = (denoised_x - target_x) ** 2
        else:
            resize = LPIPS_SIZE if x_start.shape[-1] < LPIPS_RESIZE_BELOW else None
            return {"loss": self._lpips()((denoised_x + 1) / 2.0, (target_x + 1) / 2.0, resize=resize) * weights}
        return {"loss": mean_flat(diffs) * weights}

    def _progdist_losses_hip(self, nets, x_start, num_scales, model_kwargs, teacher_diffusion, noise, indices):
        net, teacher = nets
        if x_start.requires_grad or noise.requires_grad:
            raise NotImplementedError("progdist_losses on the HIP U-Net differentiates the online network's parameters only: "
                                      "x_start and noise must not require grad")
        extra = set(model_kwargs) - {"y"}
        if extra:
            raise NotImplementedError(f"progdist_losses on the HIP U-Net: model_kwargs {sorted(extra)} are not inputs of UNetModel")
        y = model_kwargs.get("y")
        for n in nets:
            if (y is not None) != (n.num_classes is not None):
                raise ValueError("must specify y if and only if the model is class-conditional")
        f32 = lambda v: v.detach().to(torch.float32).contiguous()
        x_start, noise = f32(x_start), f32(noise)
        indices = indices.detach().to(device=x_start.device, dtype=torch.int64).reshape(-1).contiguous()
        if noise.shape != x_start.shape or indices.numel() != x_start.shape[0] or x_start.dim() != 4:
            raise ValueError(f"progdist_losses: noise {tuple(noise.shape)} must match x_start {tuple(x_start.shape)} [N, C, H, W] "
                             f"and indices ({indices.numel()}) hold one level per sample")
        levels = pd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho)
        if _graph.capturing() and not levels.on_device(x_start.device):
            raise DxmiError(f"progdist_losses inside a StepGraph capture: the level table of num_scales {int(num_scales)} is not on "
                            f"{x_start.device} yet (pd_levels(...).device_table(device) before the capture: an upload cannot be captured)")
        tab = levels.device_table(x_start.device)
        args = (self, net, teacher, teacher_diffusion, x_start, noise, indices, tab, y)
        if torch.is_grad_enabled():
            loss = _PDLossFn.apply(*args, *ops.fast_parameters(net))
        else:
            loss, _ = _pd_loss(*args, keep=False)
        return {"loss": loss}

    def _consistency_losses_hip(self, nets, x_start, num_scales, model_kwargs, teacher_diffusion, noise, indices):
        net, target = nets[0], nets[1]
        teacher = nets[2] if len(nets) > 2 else None
        if x_start.requires_grad or noise.requires_grad:
            raise NotImplementedError("consistency_losses on the HIP U-Net differentiates the online network's parameters only: "
                                      "x_start and noise must not require grad")
        extra = set(model_kwargs) - {"y"}
        if extra:
            raise NotImplementedError(f"consistency_losses on the HIP U-Net: model_kwargs {sorted(extra)} are not inputs of UNetModel")
        y = model_kwargs.get("y")
        for n in nets:
            if (y is not None) != (n.num_classes is not None):
                raise ValueError("must specify y if and only if the model is class-conditional")
        f32 = lambda v: v.detach().to(torch.float32).contiguous()
        x_start, noise = f32(x_start), f32(noise)
        indices = indices.detach().to(device=x_start.device, dtype=torch.int64).reshape(-1).contiguous()
        if noise.shape != x_start.shape or indices.numel() != x_start.shape[0] or x_start.dim() != 4:
            raise ValueError(f"consistency_losses: noise {tuple(noise.shape)} must match x_start {tuple(x_start.shape)} [N, C, H, W] "
                             f"and indices ({indices.numel()}) hold one level per sample")
        levels = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho)
        if _graph.capturing() and not levels.on_device(x_start.device):
            raise DxmiError(f"consistency_losses inside a StepGraph capture: the {int(num_scales)}-level table is not on {x_start.device} "
                            "yet (cd_levels(...).device_table(device) before the capture: an upload cannot be captured)")
        tab = levels.device_table(x_start.device)
        args = (self, net, target, teacher, teacher_diffusion, x_start, noise, indices, tab, y)
        if torch.is_grad_enabled():
            loss = _CDLossFn.apply(*args, *ops.fast_parameters(net))
        else:
            loss, _ = _cd_loss(*args, keep=False)
        return {"loss": loss}

    def dm_generator_losses(self, model, z, num_scales=1000, real_model=None, real_diffusion=None, fake_model=None, fake_diffusion=None,
                            model_kwargs=None, noise=None, indices=None, generator=None, gen_sigma=None, weighting="dmd",
                            min_step_frac=0.02, max_step_frac=0.98, gan_head=None, gan_gen_weight=3e-3, gan_noise=None, gan_indices=None,
                            gan_min_step_frac=0.0, gan_max_step_frac=1.0, gen_sigmas=None, steps=None, sim_noise=None):
        """Distribution-matching loss of the one-step generator G(z) = D_theta(sigma_G z, sigma_G) (Diff-Instruct, Luo et al. 2023;
        DMD, Yin et al. 2023, eq. 7-8; DMD2, Yin et al. 2024, its GAN term under gan_head below) -> {"loss": [N], "x": [N, C, H, W] detached fp32,
        "dm_norm": [N]}.  x = G(z) is diffused to x_t = x + noise t, t = cd_levels(num_scales)[index]; with D_r / D_f the denoised
        images of real_model under real_diffusion (the teacher) and fake_model under fake_diffusion (None: real_diffusion; trained
        online on x by training_losses), s = mean|x - D_r| ("dm_norm") and g = (D_f - D_r) / s (weighting "dmd") or D_f - D_r
        ("none"); a sample with s == 0 gets g = 0.  loss = 0.5 mean(g^2) per sample, and its gradient is DEFINED as
        d loss_n / d x = g_n / CHW: both denoisers are under stop-gradient, neither net receives a gradient, the generator receives
        it through x alone.  `self` is the generator's diffusion (distillation=False).  gen_sigma: None = sigma_max.
        indices: drawn uniformly from [ceil(min_step_frac (S - 1)), floor(max_step_frac (S - 1))] when None, then noise, both from
        `generator` where given.
        gan_head (models.cm.gan_head.GANHead; None: the code path without it): DMD2's GAN term.  With x_gan = x + gan_noise t_gan,
        t_gan = levels[gan_indices], logit = gan_head(bottleneck of fake_model at (c_in x_gan, t_gan)) and
        gan_loss_n = softplus(-logit_n): loss = the DM loss + gan_gen_weight gan_loss, d loss_n / d x = g_n / CHW + gan_gen_weight
        d gan_loss_n / d x, reaching the generator through x alone (neither the head nor the fake denoiser receives a gradient),
        and the result gains "gan_loss" and "gan_logit", [N], detached.  gan_indices (uniform over dm_index_range(S, gan_min_step_frac,
        gan_max_step_frac)) and then gan_noise are drawn after the draws above.  DESIGN 5.39.
        gen_sigmas (excludes gen_sigma): the ladder sigma_0 > ... > sigma_{K-1} > 0 of a K-step generator trained by backward
        simulation (DMD2, Yin et al. 2024, section 4.4-4.5).  Step j is G_j(x) = D_theta(x, sigma_j); the sampler's states
        are x_0 = sigma_0 z and x_{j+1} = G_j(x_j) + sigma_{j+1} eps_j (dm_sample), never clamped.  Image n draws a step k_n uniformly
        from {0 .. K-1}; x_{k_n} is made by the current generator under no_grad from x_0 with the noise sim_noise[j] of stage j, the
        graded evaluation is x = G_{k_n}(x_{k_n}), and from x on everything above holds unchanged; no gradient enters the simulation.
        steps: int64 [N] given, else drawn BEFORE every draw above; sim_noise: [K - 1, N, C, H, W] given, else one draw per stage,
        in stage order, AFTER every draw above; both from `generator` where given.  The result gains "steps" (int64 [N]).  K = 1
        makes neither draw and is the one-step call at gen_sigma = gen_sigmas[0]."""
        what = "dm_generator_losses"
        model_kwargs, fake_diffusion = self._dm_refusals(what, real_model, real_diffusion, fake_model, fake_diffusion, model_kwargs)
        if weighting not in DM_WEIGHTINGS:
            raise ValueError(f"dm_generator_losses: weighting {weighting!r} is not one of {DM_WEIGHTINGS}")
        ladder, steps = self._dm_ladder(what, z, gen_sigma, gen_sigmas, steps, sim_noise, generator)
        if ladder is not None and len(ladder) == 1:
            gen_sigma = ladder.sigmas[0]
        K = 1 if ladder is None else len(ladder)
        gen_sigma, indices, noise = self._dm_draws(what, z, num_scales, noise, indices, generator, 1.0 if K > 1 else gen_sigma,
                                                   min_step_frac, max_step_frac)
        if gan_head is not None:
            gan_gen_weight = float(gan_gen_weight)
            if not math.isfinite(gan_gen_weight):
                raise ValueError(f"dm_generator_losses: gan_gen_weight must be finite, got {gan_gen_weight!r}")
            _, gan_indices, gan_noise = self._dm_draws(what, z, num_scales, gan_noise, gan_indices, generator, gen_sigma, gan_min_step_frac,
                                                       gan_max_step_frac)
            if gan_noise.requires_grad:
                raise NotImplementedError("dm_generator_losses differentiates the generator's parameters only: gan_noise must not "
                                          "require grad")
        if K > 1:
            sim_noise = self._dm_sim_noise(what, z, K, sim_noise, generator)
        more = {} if ladder is None else {"steps": steps}
        nets = [_hip_unet(m) for m in (model, real_model, fake_model)]
        if all(n is not None for n in nets) and z.is_cuda:
            args = self._dm_hip_operands(what, nets, z, num_scales, model_kwargs, real_diffusion, fake_diffusion, noise, indices, gen_sigma)
            if K > 1:
                if sim_noise.requires_grad:
                    raise NotImplementedError(f"{what} on the HIP U-Net differentiates the generator's parameters only: "
                                              "sim_noise must not require grad")
                z32 = args[6]
                more["steps"] = steps = steps.to(device=z32.device, dtype=torch.int64).contiguous()
                args = args[:-1] + (_GenSteps(ladder.device_table(z32.device), steps,
                                              sim_noise.detach().to(device=z32.device, dtype=torch.float32).contiguous()),)
            if gan_head is not None:
                gan = (gan_head, gan_gen_weight) + self._dm_level_operands(what, args[6], gan_noise, gan_indices)
                if torch.is_grad_enabled():
                    loss, x, s, gl, lg = _DMGanLossFn.apply(*args, weighting, gan, *ops.fast_parameters(nets[0]))
                else:
                    loss, x, s, _, gl, lg = _dm_loss(*args, weighting, keep=False, gan=gan)
                return dict({"loss": loss, "x": x, "dm_norm": s, "gan_loss": gl, "gan_logit": lg}, **more)
            if torch.is_grad_enabled():
                loss, x, s = _DMLossFn.apply(*args, weighting, *ops.fast_parameters(nets[0]))
            else:
                loss, x, s, _ = _dm_loss(*args, weighting, keep=False)
            return dict({"loss": loss, "x": x, "dm_norm": s}, **more)
        if z.requires_grad or noise.requires_grad or (K > 1 and sim_noise.requires_grad):
            raise NotImplementedError("dm_generator_losses differentiates the generator's parameters only: z and noise must not "
                                      "require grad")
        if gan_head is not None and not hasattr(fake_model, "encode"):
            raise NotImplementedError("dm_generator_losses with a gan_head: the fake model must offer encode(x_in, t, **kw) -> "
                                      f"[N, C, h, w], the bottleneck features the head reads; {type(fake_model).__name__} has no encode")
        N, dims = z.shape[0], z.ndim
        levels = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho).table.to(z.device)
        t = levels[indices.to(z.device)]
        if K > 1:
            # backward simulation: the sampler's own states under no_grad, an image frozen once its step is reached
            more["steps"] = steps = steps.to(z.device)
            sig = ladder.table.to(z.device)
            x_k = z * ladder.sigmas[0]
            with torch.no_grad():
                for j in range(K - 1):
                    d_j = self.denoise(model, x_k, sig[j].expand(N), **model_kwargs)[1]
                    x_k = torch.where(append_dims(steps > j, dims), d_j + sim_noise[j].to(z.device) * ladder.sigmas[j + 1], x_k)
            x = self.denoise(model, x_k, sig[steps], **model_kwargs)[1]
        else:
            sigma_g = torch.full((N,), gen_sigma, dtype=torch.float32, device=z.device)
            x = self.denoise(model, z * gen_sigma, sigma_g, **model_kwargs)[1]
        with torch.no_grad():
            x_t = x + noise * append_dims(t, dims)
            d_real = real_diffusion.denoise(real_model, x_t, t, **model_kwargs)[1]
            d_fake = fake_diffusion.denoise(fake_model, x_t, t, **model_kwargs)[1]
            s = mean_flat(torch.abs(x - d_real))
            g = d_fake - d_real
            if weighting == "dmd":
                g = g / append_dims(s, dims)
            g = torch.where(append_dims(s, dims) == 0, torch.zeros_like(g), g)
        if gan_head is None:
            return dict({"loss": _DMSurrogate.apply(x, g), "x": x.detach().float(), "dm_norm": s}, **more)
        # the GAN term's d / d x is taken here, with respect to x alone: the head and the fake model see no backward
        keep = torch.is_grad_enabled()
        t_gan = levels[gan_indices.to(z.device)]
        with torch.enable_grad() if keep else torch.no_grad():
            xd = x.detach().requires_grad_(keep)
            x_gan = xd + gan_noise * append_dims(t_gan, dims)
            c_in = append_dims(fake_diffusion.get_scalings(t_gan)[2], dims)
            logit = gan_head(fake_model.encode(c_in * x_gan, 1000 * 0.25 * torch.log(t_gan + 1e-44), **model_kwargs))
            gan_loss = torch.nn.functional.softplus(-logit)
            g_gan = torch.autograd.grad(gan_loss.sum(), xd)[0] if keep else None
        gan_loss, logit = gan_loss.detach(), logit.detach()
        value = 0.5 * mean_flat(g ** 2) + gan_gen_weight * gan_loss
        if keep:
            value = _SiDSurrogate.apply(x, g + (x[0].numel() * gan_gen_weight) * g_gan, value)
        return dict({"loss": value, "x": x.detach().float(), "dm_norm": s, "gan_loss": gan_loss, "gan_logit": logit}, **more)

    def gan_discriminator_losses(self, fake_model, gan_head, x_fake, x_real, num_scales, model_kwargs=None, real_kwargs=None, noise=None,
                                 indices=None, generator=None, gan_min_step_frac=0.0, gan_max_step_frac=1.0):
        """The discriminator loss of DMD2's GAN term (Yin et al. 2024) -> {"loss": [N], "logit_fake": [N], "logit_real": [N]}.
        `self` is the fake denoiser's diffusion, as with training_losses.  The generated batch x_fake (model_kwargs) and the real batch
        x_real (real_kwargs) have one shape and run as one batch of 2N, generated half first: indices [2N] are drawn uniformly over
        dm_index_range(num_scales, gan_min_step_frac, gan_max_step_frac) when None, then noise [2N, C, H, W]; x_t = x + noise t,
        logit = gan_head(bottleneck of fake_model at (c_in x_t, t)), loss_n = softplus(logit_fake_n) + softplus(-logit_real_n).
        Gradients go to the head's parameters and to the fake net's encoder and embedding parameters; its decoder gets none.
        On the HIP U-Net it is one autograd node (_GANDisLossFn); any other fake model must offer encode(x_in, t, **kw)."""
        what = "gan_discriminator_losses"
        if tuple(x_fake.shape) != tuple(x_real.shape):
            raise ValueError(f"{what}: the generated batch {tuple(x_fake.shape)} and the real batch {tuple(x_real.shape)} must have one shape")
        model_kwargs, real_kwargs = model_kwargs or {}, real_kwargs or {}
        if set(model_kwargs) != set(real_kwargs):
            raise ValueError(f"{what}: model_kwargs {sorted(model_kwargs)} and real_kwargs {sorted(real_kwargs)} must name the same inputs")
        kw = {k: torch.cat([model_kwargs[k], real_kwargs[k].to(model_kwargs[k].device)]) for k in model_kwargs}
        x = torch.cat([x_fake.detach(), x_real.detach().to(x_fake.device)]).float()
        _, indices, noise = self._dm_draws(what, x, num_scales, noise, indices, generator, 1.0, gan_min_step_frac, gan_max_step_frac)
        N = x_fake.shape[0]
        if tuple(noise.shape) != tuple(x.shape) or indices.numel() != 2 * N:
            raise ValueError(f"{what}: noise {tuple(noise.shape)} must match the stacked batch {tuple(x.shape)} and indices "
                             f"({indices.numel()}) hold one level per sample of it")
        net = _hip_unet(fake_model)
        if net is not None and x.is_cuda:
            extra = set(kw) - {"y"}
            if extra:
                raise NotImplementedError(f"{what} on the HIP U-Net: model_kwargs {sorted(extra)} are not inputs of UNetModel")
            y = kw.get("y")
            if (y is not None) != (net.num_classes is not None):
                raise ValueError("must specify y if and only if the model is class-conditional")
            x, noise = x.contiguous(), noise.detach().to(torch.float32).contiguous()
            indices = indices.detach().to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
            tab = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho).device_table(x.device)
            loss, lf, lr = _GANDisLossFn.apply(self, net, gan_head, x, noise, indices, tab, y, *ops.fast_parameters(net),
                                               *ops.fast_parameters(gan_head))
            return {"loss": loss, "logit_fake": lf, "logit_real": lr}
        if not hasattr(fake_model, "encode"):
            raise NotImplementedError(f"{what}: the fake model must offer encode(x_in, t, **kw) -> [N, C, h, w], the bottleneck "
                                      f"features the head reads; {type(fake_model).__name__} has no encode")
        levels = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho).table.to(x.device)
        t = levels[indices.to(x.device)]
        x_t = x + noise * append_dims(t, x.ndim)
        c_in = append_dims(self.get_scalings(t)[2], x.ndim)
        logit = gan_head(fake_model.encode(c_in * x_t, 1000 * 0.25 * torch.log(t + 1e-44), **kw))
        sp = torch.nn.functional.softplus
        return {"loss": sp(logit[:N]) + sp(-logit[N:]), "logit_fake": logit[:N].detach(), "logit_real": logit[N:].detach()}

    def _dm_refusals(self, what, real_model, real_diffusion, fake_model, fake_diffusion, model_kwargs):
        """The refusals dm_generator_losses and sid_generator_losses share -> (model_kwargs, fake_diffusion)."""
        if self.distillation:
            raise NotImplementedError(f"{what}: the one-step generator keeps the EDM scalings (distillation=False); a "
                                      "diffusion with boundary-condition scalings belongs to the consistency losses")
        if real_model is None or real_diffusion is None or fake_model is None:
            raise NotImplementedError(f"{what}: Must have a real_model with its real_diffusion and a fake_model")
        return ({} if model_kwargs is None else model_kwargs), (real_diffusion if fake_diffusion is None else fake_diffusion)

    @staticmethod
    def _dm_ladder(what, z, gen_sigma, gen_sigmas, steps, sim_noise, generator):
        """The K-step arguments checked -> (GenLadder | None, steps int64 [N] | None).  With K > 1 and no steps given they are drawn
        here, uniformly over {0 .. K-1}: the first draw of the call.  K = 1 draws nothing (steps are zeros)."""
        N = z.shape[0]
        if gen_sigmas is None:
            if steps is not None or sim_noise is not None:
                raise ValueError(f"{what}: steps and sim_noise belong to a K-step generator: give gen_sigmas")
            return None, None
        if gen_sigma is not None:
            raise ValueError(f"{what}: gen_sigmas (the K-step ladder) excludes gen_sigma (the one-step level): give one of them")
        ladder = gen_ladder(what, gen_sigmas)
        K = len(ladder)
        if steps is not None:
            if not torch.is_tensor(steps) or steps.dtype != torch.int64 or steps.dim() != 1 or steps.numel() != N:
                raise ValueError(f"{what}: steps must be an int64 [N = {N}] tensor, got "
                                 f"{(steps.dtype, tuple(steps.shape)) if torch.is_tensor(steps) else type(steps).__name__}")
            lo, hi = int(steps.min()), int(steps.max())
            if lo < 0 or hi > K - 1:
                raise ValueError(f"{what}: steps must lie in [0, K - 1 = {K - 1}], got values in [{lo}, {hi}]")
            steps = steps.detach()
        elif K == 1:
            steps = torch.zeros(N, dtype=torch.int64, device=z.device)
        elif generator is not None:
            steps = torch.randint(0, K, (N,), generator=generator, device=generator.device).to(z.device)
        else:
            steps = torch.randint(0, K, (N,), device=z.device)
        if K == 1 and sim_noise is not None and (not torch.is_tensor(sim_noise) or tuple(sim_noise.shape) != (0,) + tuple(z.shape)):
            raise ValueError(f"{what}: sim_noise must be [K - 1, N, C, H, W] = {(0,) + tuple(z.shape)}")
        return ladder, steps

    @staticmethod
    def _dm_sim_noise(what, z, K, sim_noise, generator):
        """The simulation noise [K - 1, *z.shape] of a K-step call: checked, or drawn stage by stage, the last draws of the call."""
        shape = (K - 1,) + tuple(z.shape)
        if sim_noise is not None:
            if not torch.is_tensor(sim_noise) or tuple(sim_noise.shape) != shape:
                raise ValueError(f"{what}: sim_noise must be [K - 1, N, C, H, W] = {shape}, got "
                                 f"{tuple(sim_noise.shape) if torch.is_tensor(sim_noise) else type(sim_noise).__name__}")
            return sim_noise
        if generator is not None:
            draws = [torch.randn(z.shape, generator=generator, device=generator.device, dtype=z.dtype).to(z.device) for _ in range(K - 1)]
        else:
            draws = [torch.randn_like(z) for _ in range(K - 1)]
        return torch.stack(draws)

    def _dm_draws(self, what, z, num_scales, noise, indices, generator, gen_sigma, min_step_frac, max_step_frac):
        """-> (gen_sigma, indices, noise): sigma_G checked, then the draws of one generator step, indices before noise."""
        gen_sigma = float(self.sigma_max if gen_sigma is None else gen_sigma)
        if not (math.isfinite(gen_sigma) and gen_sigma > 0):
            raise ValueError(f"{what}: gen_sigma must be positive and finite, got {gen_sigma!r}")
        N = z.shape[0]
        if indices is None:
            lo, hi = dm_index_range(num_scales, min_step_frac, max_step_frac)
            if generator is not None:
                indices = torch.randint(lo, hi + 1, (N,), generator=generator, device=generator.device).to(z.device)
            else:
                indices = torch.randint(lo, hi + 1, (N,), device=z.device)
        if noise is None:
            if generator is not None:
                noise = torch.randn(z.shape, generator=generator, device=generator.device, dtype=z.dtype).to(z.device)
            else:
                noise = torch.randn_like(z)
        return gen_sigma, indices, noise

    @staticmethod
    def _dm_level_operands(what, z, noise, indices):
        """-> (noise fp32 contiguous, indices int64 [N] on z's device), checked against the latents z [N, C, H, W]."""
        noise = noise.detach().to(torch.float32).contiguous()
        indices = indices.detach().to(device=z.device, dtype=torch.int64).reshape(-1).contiguous()
        if noise.shape != z.shape or indices.numel() != z.shape[0] or z.dim() != 4:
            raise ValueError(f"{what}: noise {tuple(noise.shape)} must match z {tuple(z.shape)} [N, C, H, W] "
                             f"and indices ({indices.numel()}) hold one level per sample")
        return noise, indices

    def _dm_hip_operands(self, what, nets, z, num_scales, model_kwargs, real_diffusion, fake_diffusion, noise, indices, gen_sigma):
        """The checks of the device path -> the leading arguments of _dm_loss / _sid_loss, up to gen_sigma."""
        net, real, fake = nets
        if z.requires_grad or noise.requires_grad:
            raise NotImplementedError(f"{what} on the HIP U-Net differentiates the generator's parameters only: "
                                      "z and noise must not require grad")
        extra = set(model_kwargs) - {"y"}
        if extra:
            raise NotImplementedError(f"{what} on the HIP U-Net: model_kwargs {sorted(extra)} are not inputs of UNetModel")
        y = model_kwargs.get("y")
        for n in nets:
            if (y is not None) != (n.num_classes is not None):
                raise ValueError("must specify y if and only if the model is class-conditional")
        z = z.detach().to(torch.float32).contiguous()
        noise, indices = self._dm_level_operands(what, z, noise, indices)
        levels = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho)
        if _graph.capturing() and not levels.on_device(z.device):
            raise DxmiError(f"{what} inside a StepGraph capture: the {int(num_scales)}-level table is not on {z.device} "
                            "yet (cd_levels(...).device_table(device) before the capture: an upload cannot be captured)")
        tab = levels.device_table(z.device)
        return (self, net, real, real_diffusion, fake, fake_diffusion, z, noise, indices, tab, y, gen_sigma)

    def sid_generator_losses(self, model, z, num_scales=1000, real_model=None, real_diffusion=None, fake_model=None, fake_diffusion=None,
                             model_kwargs=None, noise=None, indices=None, generator=None, gen_sigma=None, alpha=1.2,
                             min_step_frac=0.02, max_step_frac=0.98, gen_sigmas=None):
        """Score identity Distillation loss of the one-step generator of dm_generator_losses (SiD, Zhou et al., ICML 2024: the fused
        loss L~^(alpha) up to the constant 1 / CHW; its released code's (y_real - y_fake) * ((y_real - y) - alpha (y_real - y_fake))
        / weight_factor) -> {"loss": [N], "x": [N, C, H, W] detached fp32, "dm_norm": [N]}.  With x, x_t, D_r, D_f as there,
        delta = D_r - D_f and s = mean|x - D_r| ("dm_norm") under stop-gradient:
            loss_n = ((1 - alpha) sum(delta^2) + sum(delta (D_f - x))) / (CHW s_n)
        differentiated through x AND through both denoisers with respect to their input x_t; no parameter of the real or the fake
        net receives a gradient (theirs stay None).  A sample with s == 0 gets loss = 0 and no gradient (SiD's code clips the
        normaliser at 1e-5 instead), and the mean over CHW stands where SiD sums.  alpha: finite, SiD's default 1.2, 1 its base
        form; alpha = 0.5 is NOT dm_generator_losses (that one has no Jacobian paths).  Checks, refusals and draws (indices, then
        noise) are dm_generator_losses's.  DESIGN 5.34.
        gen_sigmas: a one-level ladder stands for gen_sigma; a K-step generator (K > 1) is refused: backward simulation is built for
        dm_generator_losses alone."""
        what = "sid_generator_losses"
        if gen_sigmas is not None:
            if gen_sigma is not None:
                raise ValueError(f"{what}: gen_sigmas excludes gen_sigma: give one of them")
            ladder = gen_ladder(what, gen_sigmas)
            if len(ladder) > 1:
                raise NotImplementedError(f"{what}: a K-step generator (gen_sigmas of {len(ladder)} levels) is limited to "
                                          "dm_generator_losses: score identity distillation is built for K = 1 only")
            gen_sigma = ladder.sigmas[0]
        model_kwargs, fake_diffusion = self._dm_refusals(what, real_model, real_diffusion, fake_model, fake_diffusion, model_kwargs)
        alpha = float(alpha)
        if not math.isfinite(alpha):
            raise ValueError(f"sid_generator_losses: alpha must be finite, got {alpha!r}")
        gen_sigma, indices, noise = self._dm_draws(what, z, num_scales, noise, indices, generator, gen_sigma, min_step_frac, max_step_frac)
        nets = [_hip_unet(m) for m in (model, real_model, fake_model)]
        if all(n is not None for n in nets) and z.is_cuda:
            args = self._dm_hip_operands(what, nets, z, num_scales, model_kwargs, real_diffusion, fake_diffusion, noise, indices, gen_sigma)
            if torch.is_grad_enabled():
                loss, x, s = _SiDLossFn.apply(*args, alpha, *ops.fast_parameters(nets[0]))
            else:
                loss, x, s, _ = _sid_loss(*args, alpha, keep=False)
            return {"loss": loss, "x": x, "dm_norm": s}
        if z.requires_grad or noise.requires_grad:
            raise NotImplementedError("sid_generator_losses differentiates the generator's parameters only: z and noise must not "
                                      "require grad")
        N, dims = z.shape[0], z.ndim
        levels = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho).table.to(z.device)
        t = levels[indices.to(z.device)]
        sigma_g = torch.full((N,), gen_sigma, dtype=torch.float32, device=z.device)
        x = self.denoise(model, z * gen_sigma, sigma_g, **model_kwargs)[1]
        keep = torch.is_grad_enabled()
        # d loss / d x is taken here, by autograd.grad with respect to x alone: the denoisers' parameters see no backward at all
        with torch.enable_grad() if keep else torch.no_grad():
            xd = x.detach().requires_grad_(keep)
            x_t = xd + noise * append_dims(t, dims)
            d_real = real_diffusion.denoise(real_model, x_t, t, **model_kwargs)[1]
            d_fake = fake_diffusion.denoise(fake_model, x_t, t, **model_kwargs)[1]
            s = mean_flat(torch.abs(xd - d_real)).detach()
            delta = d_real - d_fake
            total = ((1 - alpha) * delta ** 2 + delta * (d_fake - xd)).flatten(1).sum(dim=1)
            live = s != 0
            loss = torch.where(live, total / (xd[0].numel() * torch.where(live, s, torch.ones_like(s))), torch.zeros_like(s))
            g = torch.autograd.grad(loss.sum(), xd)[0] * xd[0].numel() if keep else None
        loss = loss.detach()
        return {"loss": _SiDSurrogate.apply(x, g, loss) if keep else loss, "x": x.detach().float(), "dm_norm": s}

    def sida_generator_losses(self, model, z, num_scales=1000, real_model=None, real_diffusion=None, fake_model=None, fake_diffusion=None,
                              model_kwargs=None, noise=None, indices=None, generator=None, gen_sigma=None, alpha=1.2,
                              sida_gen_weight=0.01, min_step_frac=0.02, max_step_frac=0.98, gen_sigmas=None):
        """Adversarial Score identity Distillation loss of the one-step generator (SiDA, Zhou, Zheng et al. 2024): the loss of
        sid_generator_losses plus an adversarial term whose discriminator has no parameters of its own -> {"loss": [N], "x": [N, C, H,
        W] detached fp32, "dm_norm": [N], "adv_loss": [N], "adv_logit": [N, P]} (the last two detached).  With h the activation of
        fake_model after its middle block at the SAME point (c_in x_t, t) the SiD term evaluates it at, [N, Cb, hb, wb], P = hb wb:
            logit[n, p] = mean_c h[n, c, p],  adv_n = mean_p softplus(-logit[n, p]),  loss_n = sid_n + sida_gen_weight adv_n / s_n
        with sid_n and s_n ("dm_norm", stop-gradient) those of sid_generator_losses; s_n == 0 gives loss 0 and no gradient.  The
        gradient reaches the generator through x alone: no parameter of the real or the fake net receives one.  sida_gen_weight = 0
        is sid_generator_losses bit for bit.  On HIP UNetModels it is ONE node (_SiDALossFn) that adds no network pass to SiD's:
        the fake net's input_forward hands out h, and its one input_backward takes the cotangent of h at the bottleneck next to
        the one at the output.  Any other fake model must offer encode(x_in, t, **kw) -> [N, Cb, hb, wb] (two calls of it off the
        device).  Checks, refusals and draws (indices, then noise) are sid_generator_losses's; K > 1 is refused.  DESIGN 5.41."""
        what = "sida_generator_losses"
        if gen_sigmas is not None:
            if gen_sigma is not None:
                raise ValueError(f"{what}: gen_sigmas excludes gen_sigma: give one of them")
            ladder = gen_ladder(what, gen_sigmas)
            if len(ladder) > 1:
                raise NotImplementedError(f"{what}: a K-step generator (gen_sigmas of {len(ladder)} levels) is limited to "
                                          "dm_generator_losses: adversarial score identity distillation is built for K = 1 only")
            gen_sigma = ladder.sigmas[0]
        model_kwargs, fake_diffusion = self._dm_refusals(what, real_model, real_diffusion, fake_model, fake_diffusion, model_kwargs)
        alpha, weight = float(alpha), float(sida_gen_weight)
        if not math.isfinite(alpha):
            raise ValueError(f"{what}: alpha must be finite, got {alpha!r}")
        if not math.isfinite(weight):
            raise ValueError(f"{what}: sida_gen_weight must be finite, got {weight!r}")
        gen_sigma, indices, noise = self._dm_draws(what, z, num_scales, noise, indices, generator, gen_sigma, min_step_frac, max_step_frac)
        keys = ("loss", "x", "dm_norm", "adv_loss", "adv_logit")
        nets = [_hip_unet(m) for m in (model, real_model, fake_model)]
        if all(n is not None for n in nets) and z.is_cuda:
            args = self._dm_hip_operands(what, nets, z, num_scales, model_kwargs, real_diffusion, fake_diffusion, noise, indices, gen_sigma)
            if torch.is_grad_enabled():
                out = _SiDALossFn.apply(*args, alpha, weight, *ops.fast_parameters(nets[0]))
            else:
                loss, x, s, _, adv, logit = _sida_loss(*args, alpha, weight, keep=False)
                out = (loss, x, s, adv, logit)
            return dict(zip(keys, out))
        if z.requires_grad or noise.requires_grad:
            raise NotImplementedError(f"{what} differentiates the generator's parameters only: z and noise must not require grad")
        if not hasattr(fake_model, "encode"):
            raise NotImplementedError(f"{what}: the fake model must offer encode(x_in, t, **kw) -> [N, Cb, hb, wb], the bottleneck "
                                      f"features the discriminator reads; {type(fake_model).__name__} has no encode")
        N, dims = z.shape[0], z.ndim
        levels = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho).table.to(z.device)
        t = levels[indices.to(z.device)]
        sigma_g = torch.full((N,), gen_sigma, dtype=torch.float32, device=z.device)
        x = self.denoise(model, z * gen_sigma, sigma_g, **model_kwargs)[1]
        keep = torch.is_grad_enabled()
        # d loss / d x is taken here, by autograd.grad with respect to x alone: the denoisers' parameters see no backward at all
        with torch.enable_grad() if keep else torch.no_grad():
            xd = x.detach().requires_grad_(keep)
            x_t = xd + noise * append_dims(t, dims)
            d_real = real_diffusion.denoise(real_model, x_t, t, **model_kwargs)[1]
            d_fake = fake_diffusion.denoise(fake_model, x_t, t, **model_kwargs)[1]
            c_in = append_dims(fake_diffusion.get_scalings(t)[2], dims)
            h = fake_model.encode(c_in * x_t, 1000 * 0.25 * torch.log(t + 1e-44), **model_kwargs)
            logit = h.flatten(2).mean(dim=1)
            adv = torch.nn.functional.softplus(-logit).mean(dim=1)
            s = mean_flat(torch.abs(xd - d_real)).detach()
            delta = d_real - d_fake
            total = ((1 - alpha) * delta ** 2 + delta * (d_fake - xd)).flatten(1).sum(dim=1)
            live = s != 0
            safe = torch.where(live, s, torch.ones_like(s))
            loss = torch.where(live, total / (xd[0].numel() * safe) + weight * adv / safe, torch.zeros_like(s))
            g = torch.autograd.grad(loss.sum(), xd)[0] * xd[0].numel() if keep else None
        loss = loss.detach()
        return {"loss": _SiDSurrogate.apply(x, g, loss) if keep else loss, "x": x.detach().float(), "dm_norm": s,
                "adv_loss": adv.detach(), "adv_logit": logit.detach()}

    def sida_discriminator_losses(self, fake_model, x_fake, x_real, num_scales, model_kwargs=None, real_kwargs=None, noise=None,
                                  indices=None, generator=None, min_step_frac=0.0, max_step_frac=1.0):
        """SiDA's discriminator loss -> {"loss": [N], "logit_fake": [N, P], "logit_real": [N, P]} (logits detached).  `self` is the
        fake denoiser's diffusion.  The generated batch x_fake (model_kwargs) and the real batch x_real (real_kwargs) run as one batch
        of 2N, generated half first: indices [2N] are drawn uniformly over dm_index_range(num_scales, min_step_frac, max_step_frac)
        when None, then noise [2N, C, H, W]; x_t = x + noise t, h = the activation of fake_model after its middle block at
        (c_in x_t, t), logit = mean_c h, and with a_n(sign) = mean_p softplus(sign logit[n, p]):
            loss_n = a_n(+1) of the generated image + a_n(-1) of the real image.
        The discriminator has no parameters of its own: gradients go to the fake net's encoder, middle block and embedding
        parameters, its decoder gets none.  On the HIP U-Net it is one node (_SiDADisLossFn); any other fake model must offer
        encode(x_in, t, **kw).  DESIGN 5.41."""
        what = "sida_discriminator_losses"
        if tuple(x_fake.shape) != tuple(x_real.shape):
            raise ValueError(f"{what}: the generated batch {tuple(x_fake.shape)} and the real batch {tuple(x_real.shape)} must have one shape")
        model_kwargs, real_kwargs = model_kwargs or {}, real_kwargs or {}
        if set(model_kwargs) != set(real_kwargs):
            raise ValueError(f"{what}: model_kwargs {sorted(model_kwargs)} and real_kwargs {sorted(real_kwargs)} must name the same inputs")
        kw = {k: torch.cat([model_kwargs[k], real_kwargs[k].to(model_kwargs[k].device)]) for k in model_kwargs}
        net = _hip_unet(fake_model)
        x = torch.cat([x_fake.detach(), x_real.detach().to(x_fake.device)])
        if net is not None and x.is_cuda:
            x = x.float()
        _, indices, noise = self._dm_draws(what, x, num_scales, noise, indices, generator, 1.0, min_step_frac, max_step_frac)
        N = x_fake.shape[0]
        if tuple(noise.shape) != tuple(x.shape) or indices.numel() != 2 * N:
            raise ValueError(f"{what}: noise {tuple(noise.shape)} must match the stacked batch {tuple(x.shape)} and indices "
                             f"({indices.numel()}) hold one level per sample of it")
        if net is not None and x.is_cuda:
            extra = set(kw) - {"y"}
            if extra:
                raise NotImplementedError(f"{what} on the HIP U-Net: model_kwargs {sorted(extra)} are not inputs of UNetModel")
            y = kw.get("y")
            if (y is not None) != (net.num_classes is not None):
                raise ValueError("must specify y if and only if the model is class-conditional")
            x, noise = x.contiguous(), noise.detach().to(torch.float32).contiguous()
            indices = indices.detach().to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
            tab = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho).device_table(x.device)
            loss, lf, lr = _SiDADisLossFn.apply(self, net, x, noise, indices, tab, y, *ops.fast_parameters(net))
            return {"loss": loss, "logit_fake": lf, "logit_real": lr}
        if not hasattr(fake_model, "encode"):
            raise NotImplementedError(f"{what}: the fake model must offer encode(x_in, t, **kw) -> [N, Cb, hb, wb], the bottleneck "
                                      f"features the discriminator reads; {type(fake_model).__name__} has no encode")
        levels = cd_levels(num_scales, self.sigma_min, self.sigma_max, self.rho).table.to(x.device)
        t = levels[indices.to(x.device)]
        x_t = x + noise * append_dims(t, x.ndim)
        c_in = append_dims(self.get_scalings(t)[2], x.ndim)
        logit = fake_model.encode(c_in * x_t, 1000 * 0.25 * torch.log(t + 1e-44), **kw).flatten(2).mean(dim=1)
        sp = torch.nn.functional.softplus
        return {"loss": sp(logit[:N]).mean(dim=1) + sp(-logit[N:]).mean(dim=1), "logit_fake": logit[:N].detach(),
                "logit_real": logit[N:].detach()}

    def denoise(self, model, x_t, sigmas, **model_kwargs):
        scal = self.get_scalings_for_boundary_condition(sigmas) if self.distillation else self.get_scalings(sigmas)
        c_skip, c_out, c_in = [append_dims(s, x_t.ndim) for s in scal]
        rescaled_t = 1000 * 0.25 * torch.log(sigmas + 1e-44)
        model_output = model(c_in * x_t, rescaled_t, **model_kwargs)
        return model_output, c_out * model_output + c_skip * x_t


def get_sigmas_karras(n, sigma_min, sigma_max, rho=7.0, device="cpu"):
    ramp = torch.linspace(0, 1, n)
    min_inv_rho = sigma_min ** (1 / rho)
    max_inv_rho = sigma_max ** (1 / rho)
    sigmas = (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho
    return append_zero(sigmas).to(device)


def get_ancestral_step(sigma_from, sigma_to):
    sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


# ------------------------------------------------------------------------------------------------------------- Karras samplers
KARRAS_SAMPLERS = ("heun", "dpm", "euler", "ancestral")
CM_SAMPLERS = ("onestep", "multistep")
_GRAPHS = weakref.WeakKeyDictionary()       # model -> {graph key: StepGraph}
_SCHEDULES = {}


class KarrasDenoiserFn:
    """The reference's `denoiser(x_t, sigma)` closure of karras_sample (:404-410), as data: the device samplers fuse its
    arithmetic (scalings, clip) into their stage kernels and call only `model(c_in x, 250 ln(sigma + 1e-44), **model_kwargs)`."""

    def __init__(self, diffusion, model, clip_denoised=True, model_kwargs=None):
        self.diffusion, self.model = diffusion, model
        self.clip_denoised, self.model_kwargs = bool(clip_denoised), dict(model_kwargs or {})

    def __call__(self, *a, **k):
        raise TypeError("KarrasDenoiserFn is not called directly: pass it to sample_heun / sample_dpm / sample_euler / "
                        "sample_euler_ancestral, which fuse its arithmetic into dxmi_karras_stage, or to the consistency "
                        "samplers and editing loops, which fuse it into dxmi_cm_stage")


def _refuse_distillation(diffusion):
    if getattr(diffusion, "distillation", False):
        raise NotImplementedError("the EDM samplers on the device support distillation=False only: the boundary-condition "
                                  "scalings belong to consistency-distilled models, which sample with onestep / multistep")


class KarrasSchedule(_HostTable):
    """Host schedule of one sampler over a sigma ladder, in fp32 torch with the reference's expressions (:447-640).

    Per step i: gamma (python float, as the reference), sigma_hat, churn = (sigma_hat^2 - sigma^2)^0.5, and per sampler the
    step sizes (dt; dpm: sigma_mid, dt_1, dt_2; ancestral: sigma_down, sigma_up).  `launches` is the launch sequence of
    dxmi_karras_stage: launch 0 (FIRST) precedes evaluation 1 and launch k follows evaluation k; `table` holds one row per launch
    (include/dxmi_hip.h, DXMI_KT_*).  What _run_stages reads of a launch: `last`; `draw`, the draw a generator makes there (None:
    none) and `used`, whether its result reaches the kernel; `cb`, the callback's step index (None: no callback)."""

    def __init__(self, sigmas, sampler, diffusion, clip_denoised=True, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0,
                 x_scale=1.0):
        if sampler not in KARRAS_SAMPLERS:
            raise ValueError(f"unknown Karras sampler {sampler!r}; the device path runs {KARRAS_SAMPLERS}")
        sigmas = sigmas.detach().to("cpu", torch.float32)
        self.sampler, self.sigmas, self.sigma_data = sampler, sigmas, diffusion.sigma_data
        n = len(sigmas) - 1
        self.steps = n
        churned = sampler in ("heun", "dpm")
        self.gamma, sh, churn, dt, mid, dt2, down, up = [], [], [], [], [], [], [], []
        for i in range(n):
            gamma = (min(s_churn / (len(sigmas) - 1), 2 ** 0.5 - 1) if s_tmin <= sigmas[i] <= s_tmax else 0.0) if churned else 0.0
            sigma_hat = sigmas[i] * (gamma + 1)
            self.gamma.append(gamma)
            sh.append(sigma_hat)
            churn.append((sigma_hat ** 2 - sigmas[i] ** 2) ** 0.5)
            if sampler == "dpm":
                sigma_mid = ((sigma_hat ** (1 / 3) + sigmas[i + 1] ** (1 / 3)) / 2) ** 3
                mid.append(sigma_mid)
                dt.append(sigma_mid - sigma_hat)
                dt2.append(sigmas[i + 1] - sigma_hat)
            elif sampler == "ancestral":
                sigma_down, sigma_up = get_ancestral_step(sigmas[i], sigmas[i + 1])
                down.append(sigma_down)
                up.append(sigma_up)
                dt.append(sigma_down - sigmas[i])
            else:
                dt.append(sigmas[i + 1] - sigma_hat)
        st = lambda v: torch.stack(v) if v else None
        self.sigma_hat, self.churn, self.dt = st(sh), st(churn), st(dt)
        self.sigma_mid, self.dt_2, self.sigma_down, self.sigma_up = st(mid), st(dt2), st(down), st(up)

        z = torch.zeros((), dtype=torch.float32)
        L = []      # (mode, last, eval sigma, dt, sigma_up, next eval sigma, churn step, draw, callback step)

        def corr_tail(i):
            return dict(last=i == n - 1, nxt=None if i == n - 1 else sh[i + 1], churn_step=None if i == n - 1 else i + 1,
                        draw=None if i == n - 1 or not churned else ("eps", i + 1))
        L.append(dict(mode=ops.KARRAS_FIRST, last=False, sig=None, dt=z, up=z, nxt=sh[0], churn_step=0 if churned else None,
                      draw=("eps", 0) if churned else None, cb=None))
        for i in range(n):
            if sampler == "heun" and sigmas[i + 1] != 0:
                L.append(dict(mode=ops.KARRAS_PRED, last=False, sig=sh[i], dt=dt[i], up=z, nxt=sigmas[i + 1], churn_step=None,
                              draw=None, cb=i))
                L.append(dict(mode=ops.KARRAS_HEUN_CORR, sig=sigmas[i + 1], dt=dt[i], up=z, cb=None, **corr_tail(i)))
            elif sampler == "dpm":
                L.append(dict(mode=ops.KARRAS_PRED, last=False, sig=sh[i], dt=dt[i], up=z, nxt=mid[i], churn_step=None, draw=None,
                              cb=i))
                L.append(dict(mode=ops.KARRAS_DPM_CORR, sig=mid[i], dt=dt2[i], up=z, cb=None, **corr_tail(i)))
            elif sampler == "ancestral":
                L.append(dict(mode=ops.KARRAS_ANCESTRAL, last=i == n - 1, sig=sigmas[i], dt=dt[i], up=up[i],
                              nxt=None if i == n - 1 else sigmas[i + 1], churn_step=None, draw=("z", i), cb=i))
            else:   # euler, and heun's last step (sigma_{i+1} = 0: Euler, :537-539)
                L.append(dict(mode=ops.KARRAS_EULER, last=i == n - 1, sig=sh[i], dt=dt[i], up=z,
                              nxt=None if i == n - 1 else sigmas[i + 1], churn_step=None, draw=None, cb=i))
        for l in L:     # eps at gamma = 0 and a z at sigma_up = 0 (the last ancestral step) are drawn for the generator's sake alone
            kind, i = l["draw"] or (None, None)
            l["used"] = kind is not None and (self.gamma[i] > 0 if kind == "eps" else float(up[i]) != 0.0)
        self.launches = L
        self.scratch = ("x2", "d") if churned else ()       # state buffers next to x / x_in / t / out
        self.nfe = len(L) - 1
        self.eval_sigmas = torch.stack([l["nxt"] for l in L if l["nxt"] is not None])      # noise level of every evaluation

        tab = torch.zeros((len(L), ops.KT_COLS), dtype=torch.float32)
        for k, l in enumerate(L):
            if l["sig"] is not None:
                c_skip, c_out, _ = diffusion.get_scalings(l["sig"].reshape(1))
                tab[k, ops.KT_SIGMA], tab[k, ops.KT_CSKIP], tab[k, ops.KT_COUT] = l["sig"], c_skip[0], c_out[0]
            tab[k, ops.KT_DT], tab[k, ops.KT_SIGMA_UP] = l["dt"], l["up"]
            if l["churn_step"] is not None:
                tab[k, ops.KT_CHURN] = churn[l["churn_step"]]
            tab[k, ops.KT_SNOISE] = s_noise
            if l["nxt"] is not None:
                s = l["nxt"].reshape(1)
                tab[k, ops.KT_CIN] = diffusion.get_scalings(s)[2][0]
                tab[k, ops.KT_T] = (1000 * 0.25 * torch.log(s + 1e-44))[0]      # denoise() (:348)
            tab[k, ops.KT_XSCALE] = x_scale
            tab[k, ops.KT_CLIP] = 1.0 if clip_denoised else 0.0
        super().__init__(tab)

    def stage(self, k, bufs, F, noise, den):
        l = self.launches[k]
        last = l["last"]
        ops.karras_stage(l["mode"], last, bufs["tab"], k, bufs["x"], x2=bufs.get("x2"), d=bufs.get("d"), model_out=F, noise=noise,
                         x_in=None if last else bufs["x_in"], t=None if last else bufs["t"], out=bufs["out"] if last else None,
                         denoised=den)

    def callback_info(self, k, x, den):
        i = self.launches[k]["cb"]
        info = {"x": x, "i": i, "sigma": self.sigmas[i], "sigma_hat": self.sigma_hat[i], "denoised": den}
        if self.sampler == "euler":
            del info["sigma_hat"]          # the reference's euler callback has none (:566-574)
        return info


def _schedule(sigmas, sampler, denoiser, x_scale, s_churn, s_tmin, s_tmax, s_noise):
    key = (sampler, tuple(sigmas.detach().cpu().float().tolist()), float(denoiser.diffusion.sigma_data), denoiser.clip_denoised,
           float(s_churn), float(s_tmin), float(s_tmax), float(s_noise), float(x_scale))
    return _memo(_SCHEDULES, key, 64, lambda: KarrasSchedule(sigmas, sampler, denoiser.diffusion, denoiser.clip_denoised, s_churn,
                                                             s_tmin, s_tmax, s_noise, x_scale))


def _as_f32(v, device):
    v = v.to(device=device, dtype=torch.float32)
    return v if v.is_contiguous() else v.contiguous()


def _run_stages(sch, denoiser, x0, shape, device, generator, callback=None, progress=False, **edit):
    """The launch sequence of `sch` (a KarrasSchedule or a CMSchedule): FIRST, then per network evaluation one stage launch.  x0: the
    initial state (scaled by the table's XSCALE), or None to draw it (generator.randn, else on the device).  edit: what the editing
    loops hand to every dxmi_cm_stage launch after FIRST (edit, Q, ref, mask).  -> the output (a new tensor, static under graph
    capture)."""
    f32 = dict(dtype=torch.float32, device=device)
    bufs = dict(tab=sch.device_table(device), x=torch.empty(shape, **f32))
    x = bufs["x"]
    if x0 is not None:
        x.copy_(x0)
    elif generator is not None:
        x.copy_(generator.randn(*shape, device=device))
    else:
        x.normal_()
    bufs.update({k: torch.empty(shape, **f32) for k in sch.scratch + ("x_in",)}, t=torch.empty(shape[0], **f32),
                out=torch.empty(shape, **f32))
    noise_buf = None
    model, kw = denoiser.model, denoiser.model_kwargs
    launches = range(len(sch.launches))
    if progress:
        try:
            from tqdm.auto import tqdm
            launches = tqdm(launches)
        except ImportError:
            pass
    F = None
    for k in launches:
        l = sch.launches[k]
        if k > 0:
            F = model(bufs["x_in"], bufs["t"], **kw)
            if F.dtype != torch.float32 or not F.is_contiguous() or F.device != x.device:
                F = _as_f32(F, device)
            assert F.shape == x.shape, f"model output {tuple(F.shape)} != sample shape {tuple(x.shape)}"
        noise = None
        if l["draw"] is not None:
            if generator is not None:     # the reference's draws, in its order and number (:522, :603, :477, :681)
                draw = generator.randn_like(x)
                noise = _as_f32(draw, device) if l["used"] else None
            elif l["used"]:
                if noise_buf is None:
                    noise_buf = torch.empty(shape, **f32)
                noise = noise_buf.normal_()
        den, cb_x = None, None
        if callback is not None and l["cb"] is not None:
            den, cb_x = torch.empty(shape, **f32), x.clone()
        sch.stage(k, bufs, F, noise, den, **edit)
        if den is not None:
            callback(sch.callback_info(k, cb_x, den))
    return bufs["out"]


def _check_sampler_args(denoiser, x, edm=True):
    if not isinstance(denoiser, KarrasDenoiserFn):
        raise TypeError("the device Karras samplers take a KarrasDenoiserFn (diffusion, model, clip_denoised, model_kwargs): "
                        "they fuse the denoiser's arithmetic into dxmi_karras_stage / dxmi_cm_stage")
    if edm:
        _refuse_distillation(denoiser.diffusion)
    elif not getattr(denoiser.diffusion, "distillation", False):
        raise NotImplementedError("the consistency samplers on the device need a consistency-distilled model: a diffusion "
                                  "with distillation=True (boundary-condition scalings)")
    _check_device(x)


def _check_device(x):
    if not x.is_cuda:
        raise DxmiError("the Karras samplers run only on the HIP device path (no CPU fallback)")


@torch.no_grad()
def sample_euler_ancestral(model, x, sigmas, generator, progress=False, callback=None):
    """Ancestral sampling with Euler steps (reference :447-478).  model: a KarrasDenoiserFn; x: the initial state."""
    _check_sampler_args(model, x)
    sch = _schedule(sigmas, "ancestral", model, 1.0, 0.0, 0.0, float("inf"), 1.0)
    return _run_stages(sch, model, x, tuple(x.shape), x.device, generator, callback, progress)


@torch.no_grad()
def sample_heun(denoiser, x, sigmas, generator, progress=False, callback=None, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"),
                s_noise=1.0):
    """Algorithm 2 (Heun steps) of Karras et al. (2022) (reference :499-547).  NFE = 2 * steps - 1 (the last step is Euler)."""
    _check_sampler_args(denoiser, x)
    sch = _schedule(sigmas, "heun", denoiser, 1.0, s_churn, s_tmin, s_tmax, s_noise)
    return _run_stages(sch, denoiser, x, tuple(x.shape), x.device, generator, callback, progress)


@torch.no_grad()
def sample_euler(denoiser, x, sigmas, generator, progress=False, callback=None):
    """Euler steps (reference :550-578).  NFE = steps."""
    _check_sampler_args(denoiser, x)
    sch = _schedule(sigmas, "euler", denoiser, 1.0, 0.0, 0.0, float("inf"), 1.0)
    return _run_stages(sch, denoiser, x, tuple(x.shape), x.device, generator, callback, progress)


@torch.no_grad()
def sample_dpm(denoiser, x, sigmas, generator, progress=False, callback=None, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"),
               s_noise=1.0):
    """DPM-Solver-2-like midpoint steps, midpoint on a rho=3 Karras ladder (reference :581-621).  NFE = 2 * steps."""
    _check_sampler_args(denoiser, x)
    sch = _schedule(sigmas, "dpm", denoiser, 1.0, s_churn, s_tmin, s_tmax, s_noise)
    return _run_stages(sch, denoiser, x, tuple(x.shape), x.device, generator, callback, progress)


@torch.no_grad()
def sample_progdist(denoiser, x, sigmas, generator=None, progress=False, callback=None):
    """The sampler of a progressively distilled student (reference :685-719): the trailing zero of `sigmas` is dropped and every
    remaining interval is one Euler step, so it ends at the last non-zero sigma (sigma_min), not at 0.  NFE = len(sigmas) - 2.
    The launches are sample_euler's (DXMI_KARRAS_EULER rows) on the shortened ladder."""
    if len(sigmas) < 3:
        raise ValueError(f"sample_progdist needs at least one step: three sigmas with the trailing zero, got {len(sigmas)}")
    _check_sampler_args(denoiser, x)
    sch = _schedule(sigmas[:-1], "euler", denoiser, 1.0, 0.0, 0.0, float("inf"), 1.0)
    return _run_stages(sch, denoiser, x, tuple(x.shape), x.device, generator, callback, progress)


def karras_nfe(sampler, steps):
    """Network evaluations per image: heun 2 steps - 1, dpm 2 steps, euler / ancestral / progdist steps."""
    return {"heun": 2 * steps - 1, "dpm": 2 * steps, "euler": steps, "ancestral": steps, "progdist": steps}[sampler]


def karras_sample(diffusion, model, shape, steps, clip_denoised=True, progress=False, callback=None, model_kwargs=None,
                  device=None, sigma_min=0.002, sigma_max=80, rho=7.0, sampler="heun", s_churn=0.0, s_tmin=0.0,
                  s_tmax=float("inf"), s_noise=1.0, generator=None, ts=None, use_graph=False):
    """Sample the EDM teacher with a Karras sampler on the device (reference :354-420); returns clamp(x_0, -1, 1).

    model: any callable model(x_in, t, **model_kwargs) -> [B, C, H, W] (the HIP UNetModel, or a torch function).
    RNG: with generator=None every draw is made on the device and draws whose result is unused are skipped (eps when
    gamma = 0, the last ancestral z, whose sigma_up is 0), so the stream differs from the reference's.  With a generator its
    randn / randn_like are called in the reference's order and number (x_T, one eps per heun / dpm step even at gamma = 0, one z
    per ancestral step): a generator that replays recorded draws reproduces the reference's trajectory.
    use_graph: replay the whole loop of a key (sampler, steps, sigma and churn settings, shape, device, labels given) as one
    hipGraph: the first call of a key runs eagerly, the second is captured.  The returned tensor is then STATIC: the next call
    of the same key overwrites it.  Off with callback, progress or a generator, and for model_kwargs other than `y`.
    sampler onestep / multistep (ts: the multistep step indices in [0, steps - 1]): consistency-model sampling, only for a
    diffusion with distillation=True (see the module docstring); multistep uses diffusion.rho, as the reference does (:400).
    sampler progdist is not served here: this entry point keeps refusing it together with the consistency samplers on a plain
    diffusion (tests/test_karras_sample_host.py and tests/test_cm_sample_host.py pin that refusal); progdist_sample below is the
    entry point of that sampler."""
    denoiser = KarrasDenoiserFn(diffusion, model, clip_denoised, model_kwargs)
    if sampler in CM_SAMPLERS and getattr(diffusion, "distillation", False):
        # x_T = randn * sigma_max, clamp(x_0, -1, 1); the schedule (and so ts) is settled before the device is looked at
        if sampler == "onestep":
            sigma0 = float(get_sigmas_karras(steps, sigma_min, sigma_max, rho)[0])
            sch = _cm_schedule("onestep", diffusion, None, steps, sigma_min, sigma_max, rho, clip_denoised, sigma_max, True, sigma0)
        else:
            ts = _check_ts(ts, steps)
            sch = _cm_schedule("multistep", diffusion, ts, steps, sigma_min, sigma_max, diffusion.rho, clip_denoised, sigma_max,
                               True)
        key = (sampler, steps, ts, float(sigma_min), float(sigma_max), float(rho), float(diffusion.rho),
               bool(diffusion.distillation), bool(clip_denoised), float(diffusion.sigma_data))
        return _sample_on_device(lambda: sch, denoiser, shape, device, "cm_sample", key, use_graph, generator, callback, progress)
    if sampler == "progdist":
        raise NotImplementedError("karras_sample refuses sampler 'progdist' as it refuses the samplers of a consistency-distilled "
                                  "model on a plain diffusion: a progressively distilled student, which keeps the EDM scalings "
                                  "(distillation=False), samples through progdist_sample(diffusion, model, shape, steps, ...)")
    if sampler in CM_SAMPLERS:
        raise NotImplementedError(f"sampler {sampler!r} needs a consistency-distilled model (`ts`, boundary-condition scalings): a "
                                  "diffusion with distillation=True; a plain one samples with heun, dpm, euler and ancestral")
    if sampler not in KARRAS_SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r}")
    _refuse_distillation(diffusion)
    churned = sampler in ("heun", "dpm")
    schedule = lambda: _schedule(get_sigmas_karras(steps, sigma_min, sigma_max, rho, device="cpu"), sampler, denoiser, sigma_max,
                                 s_churn if churned else 0.0, s_tmin if churned else 0.0, s_tmax if churned else float("inf"),
                                 s_noise if churned else 1.0)
    key = (sampler, steps, float(sigma_min), float(sigma_max), float(rho), float(s_churn), float(s_tmin), float(s_tmax),
           float(s_noise), bool(clip_denoised), float(diffusion.sigma_data))
    return _sample_on_device(schedule, denoiser, shape, device, "karras_sample", key, use_graph, generator, callback, progress)


def progdist_sample(diffusion, model, shape, steps, clip_denoised=True, progress=False, callback=None, model_kwargs=None, device=None,
                    sigma_min=0.002, sigma_max=80, rho=7.0, generator=None, use_graph=False):
    """Sample a progressively distilled student on the device: what the reference's karras_sample(sampler="progdist") does
    (:378-379, sample_progdist :685-719); returns clamp(x, -1, 1).  The ladder is get_sigmas_karras(steps + 1) with the trailing zero
    dropped: `steps` Euler steps (NFE = steps) that end at sigma_min, not at 0.  distillation=False only: the student keeps the EDM
    scalings.  model, generator, callback (no sigma_hat in its dict, as the reference's), progress and use_graph as for
    karras_sample's euler; the launches are DXMI_KARRAS_EULER rows."""
    if getattr(diffusion, "distillation", False):
        raise NotImplementedError("progdist_sample runs a progressively distilled student, which keeps the EDM scalings "
                                  "(distillation=False); a consistency-distilled model samples with onestep / multistep")
    if steps < 1:
        raise ValueError(f"progdist_sample needs at least one step, got {steps}")
    denoiser = KarrasDenoiserFn(diffusion, model, clip_denoised, model_kwargs)
    schedule = lambda: _schedule(get_sigmas_karras(steps + 1, sigma_min, sigma_max, rho, device="cpu")[:-1], "euler", denoiser,
                                 sigma_max, 0.0, 0.0, float("inf"), 1.0)
    key = ("progdist", steps, float(sigma_min), float(sigma_max), float(rho), bool(clip_denoised), float(diffusion.sigma_data))
    return _sample_on_device(schedule, denoiser, shape, device, "progdist_sample", key, use_graph, generator, callback, progress)


def dm_sample(diffusion, model, shape, gen_sigma=None, clip_denoised=True, model_kwargs=None, generator=None, device=None,
              gen_sigmas=None):
    """Sample the one-step generator that dm_generator_losses trains: x = D_theta(sigma_G z, sigma_G) with the EDM scalings, NFE = 1
    (dxmi_dm_gen_in -> forward_inference -> dxmi_dm_gen_out); clamped to [-1, 1] when clip_denoised.  gen_sigma: None = sigma_max,
    and it must be the one the generator was trained at.  generator: as for karras_sample (its randn draws z: with a
    DeterministicGenerator image i gets the same latent whatever the batch size); None: drawn on the device.
    gen_sigmas (excludes gen_sigma): the ladder of a K-step generator (dm_generator_losses with gen_sigmas), NFE = K: dxmi_dmms_in,
    then K - 1 x (forward_inference, dxmi_dmms_stage: x' = G_j(x) + sigma_{j+1} eps, not clamped), forward_inference, dxmi_dmms_out.
    A DeterministicGenerator's stage noise is made inside the launch, with the draw numbers its randn would take; any other
    generator's randn, or torch, supplies it.  K = 1 is the one-step sampler at gen_sigmas[0]."""
    if getattr(diffusion, "distillation", False):
        raise NotImplementedError("dm_sample runs a distribution-matching generator, which keeps the EDM scalings (distillation=False); "
                                  "a consistency-distilled model samples in one step with --cm_sampler onestep")
    ladder = None
    if gen_sigmas is not None:
        if gen_sigma is not None:
            raise ValueError("dm_sample: gen_sigmas (the K-step ladder) excludes gen_sigma (the one-step level): give one of them")
        ladder = gen_ladder("dm_sample", gen_sigmas)
        if len(ladder) == 1:
            gen_sigma, ladder = ladder.sigmas[0], None
    device = _graph.indexed_device(torch.device("cuda") if device is None else device)
    if device.type != "cuda":
        raise DxmiError("dm_sample runs only on the HIP device path (no CPU fallback)")
    kw = {} if model_kwargs is None else model_kwargs
    shape = tuple(int(v) for v in shape)
    gen_sigma = float(diffusion.sigma_max if gen_sigma is None else gen_sigma)

    def evaluate(x_in, t):
        F = model(x_in, t, **kw)          # under no_grad the HIP UNetModel's forward is forward_inference
        if F.dtype != torch.float32 or not F.is_contiguous() or F.device != x_in.device:
            F = _as_f32(F, device)
        return F
    with torch.no_grad():
        if generator is not None:
            z = _as_f32(generator.randn(*shape, device=device), device)
        else:
            z = torch.randn(shape, dtype=torch.float32, device=device)
        if ladder is not None:
            tab, sd = ladder.device_table(device), diffusion.sigma_data
            x, x_in, t = ops.dmms_in(z, tab, sd)
            for j in range(len(ladder) - 1):
                F = evaluate(x_in, t)
                if isinstance(generator, DeterministicGenerator):
                    ops.dmms_stage(F, j, tab, x, x_in, t, sample_index=generator.get_indices(shape[0], device), seed=generator.seed,
                                   draw=generator._next_draw(), sigma_data=sd)
                else:
                    eps = _as_f32(generator.randn(*shape, device=device), device) if generator is not None else torch.randn_like(z)
                    ops.dmms_stage(F, j, tab, x, x_in, t, eps=eps, sigma_data=sd)
            return ops.dmms_out(evaluate(x_in, t), x, tab, sd, clip=clip_denoised, out=x)
        x_in, t = ops.dm_gen_in(z, gen_sigma, diffusion.sigma_data)
        return ops.dm_gen_out(evaluate(x_in, t), z, gen_sigma, diffusion.sigma_data, clip=clip_denoised)


def _sample_on_device(schedule, denoiser, shape, device, name, key, use_graph, generator, callback, progress):
    """karras_sample once the sampler is settled: resolve the device, build the schedule (schedule()), then run its launch
    sequence, eagerly or as the hipGraph of (key, shape, device, labels given) in the model's graphs."""
    device = _graph.indexed_device(torch.device("cuda") if device is None else device)
    if device.type != "cuda":
        raise DxmiError("karras_sample runs only on the HIP device path (no CPU fallback)")
    shape = tuple(int(s) for s in shape)
    sch = schedule()
    model, kw = denoiser.model, denoiser.model_kwargs
    with torch.no_grad():
        if not (use_graph and callback is None and not progress and generator is None and set(kw) <= {"y"}
                and not _graph.capturing()):
            return _run_stages(sch, denoiser, None, shape, device, generator, callback, progress)
        key = key + (shape, device.index, "y" in kw)
        try:
            graphs = _GRAPHS.setdefault(model, {})
        except TypeError:        # not weak-referenceable: no cache, so no replay
            graphs = {}
        g = graphs.get(key)
        if g is None:
            if "y" in kw:
                fn = lambda y: _run_stages(sch, KarrasDenoiserFn(denoiser.diffusion, model, denoiser.clip_denoised, {"y": y}), None,
                                           shape, device, None)
            else:
                fn = lambda: _run_stages(sch, denoiser, None, shape, device, None)
            g = graphs[key] = _graph.StepGraph(fn, device, modules=_graph.pack_modules(model), name=f"{name}{key}")
        return g(kw["y"]) if "y" in kw else g()


# ------------------------------------------------------------------------------------------------- consistency-model samplers
_CM_SCHEDULES = {}
_Q_CACHE = {}


def cm_nfe(sampler, ts=None):
    """Network evaluations per image: onestep 1, multistep len(ts) - 1."""
    return 1 if sampler == "onestep" else len(ts) - 1


def _check_ts(ts, steps):
    if ts is None or len(ts) < 2:
        raise ValueError("the multistep sampler needs ts: at least two step indices in [0, steps - 1]")
    for v in ts:
        if not 0 <= v <= steps - 1:
            raise ValueError(f"ts entry {v} outside [0, steps - 1] = [0, {steps - 1}]")
    return tuple(ts)


class CMSchedule(_HostTable):
    """Host table of the consistency-model samplers (reference :644-683) and editing loops (:722-951).

    onestep evaluates once at sigma0 (karras_sample: sigmas[0] = sigma_max of the fp32 Karras ladder).  multistep evaluates at
    t_i = (t_max^(1/rho) + ts[i] / (steps - 1) (t_min^(1/rho) - t_max^(1/rho)))^rho for i < len(ts) - 1, in float64 python as
    the reference, and after each evaluation adds z sqrt(next_t^2 - t_min^2) with next_t the next index's t clipped to
    [t_min, t_max] (np.clip / np.sqrt, float64; nonzero after the last evaluation unless ts[-1] = steps - 1).  The network sees
    fp32(t) (t * s_in); the scalings are the diffusion's boundary-condition ones when distillation is set, else the plain ones,
    evaluated on that fp32 sigma as denoise() does.  Row 0 is the FIRST launch, row k the launch after evaluation k
    (include/dxmi_hip.h, DXMI_CT_*); `launches` describes them to _run_stages as KarrasSchedule's do: one z per multistep
    evaluation, the last included, used unless its factor is 0; none for onestep; the callback fires after every evaluation."""

    scratch = ()

    def __init__(self, sampler, diffusion, ts=None, steps=40, t_min=0.002, t_max=80.0, rho=7.0, clip_denoised=True,
                 x_scale=1.0, out_clamp=False, sigma0=None):
        if sampler == "onestep":
            self.t = [float(sigma0)]
            self.noise = [0.0]
            self.ts = None
        elif sampler == "multistep":
            ts = self.ts = _check_ts(ts, steps)
            t_max_rho, t_min_rho = t_max ** (1 / rho), t_min ** (1 / rho)
            self.t, self.noise = [], []
            for i in range(len(ts) - 1):
                self.t.append((t_max_rho + ts[i] / (steps - 1) * (t_min_rho - t_max_rho)) ** rho)
                next_t = (t_max_rho + ts[i + 1] / (steps - 1) * (t_min_rho - t_max_rho)) ** rho
                next_t = np.clip(next_t, t_min, t_max)
                self.noise.append(np.sqrt(next_t ** 2 - t_min ** 2))
        else:
            raise ValueError(f"unknown consistency sampler {sampler!r}; the device path runs onestep and multistep")
        self.sampler, self.nfe = sampler, len(self.t)
        self.launches = [dict(mode=ops.CM_FIRST, last=False, draw=None, used=False, cb=None)]
        for k in range(1, self.nfe + 1):
            self.launches.append(dict(mode=ops.CM_STEP, last=k == self.nfe, draw=("z", k - 1) if sampler == "multistep" else None,
                                      used=sampler == "multistep" and float(self.noise[k - 1]) != 0.0, cb=k - 1))
        self.eval_sigmas = torch.stack([torch.tensor([t], dtype=torch.float32)[0] for t in self.t])   # fp32(t): t * s_in
        scal = diffusion.get_scalings_for_boundary_condition if diffusion.distillation else diffusion.get_scalings
        tab = torch.zeros((self.nfe + 1, ops.CT_COLS), dtype=torch.float32)
        for k in range(self.nfe + 1):
            if k > 0:
                c_skip, c_out, _ = scal(self.eval_sigmas[k - 1].reshape(1))
                tab[k, ops.CT_CSKIP], tab[k, ops.CT_COUT] = c_skip[0], c_out[0]
                tab[k, ops.CT_NOISE] = float(self.noise[k - 1])          # randn_like(x) * np.float64: fp32 multiplier
            if k < self.nfe:
                s = self.eval_sigmas[k].reshape(1)
                tab[k, ops.CT_CIN] = scal(s)[2][0]
                tab[k, ops.CT_T] = (1000 * 0.25 * torch.log(s + 1e-44))[0]    # denoise() (:348)
            tab[k, ops.CT_XSCALE] = x_scale
            tab[k, ops.CT_CLIP] = 1.0 if clip_denoised else 0.0
            tab[k, ops.CT_OUTCLAMP] = 1.0 if out_clamp else 0.0
        super().__init__(tab)

    def stage(self, k, bufs, F, noise, den, **edit):
        l = self.launches[k]
        last = l["last"]
        ops.cm_stage(l["mode"], last, bufs["tab"], k, bufs["x"], model_out=F, noise=noise, x_in=None if last else bufs["x_in"],
                     t=None if last else bufs["t"], out=bufs["out"] if last else None, denoised=den, **(edit if k > 0 else {}))

    def callback_info(self, k, x, den):
        return {"x": x, "i": k - 1, "sigma": self.eval_sigmas[k - 1], "denoised": den}


def _cm_schedule(sampler, diffusion, ts, steps, t_min, t_max, rho, clip, x_scale, out_clamp, sigma0=None):
    key = (sampler, None if ts is None else tuple(float(v) for v in ts), int(steps), float(t_min), float(t_max), float(rho),
           float(diffusion.sigma_data), float(diffusion.sigma_min), bool(diffusion.distillation), bool(clip), float(x_scale),
           bool(out_clamp), None if sigma0 is None else float(sigma0))
    return _memo(_CM_SCHEDULES, key, 64, lambda: CMSchedule(sampler, diffusion, ts, steps, t_min, t_max, rho, clip, x_scale, out_clamp,
                                                            sigma0))


def _orthogonal(vector):
    """The reference's basis of iterative_colorization / iterative_superres (:731-739, :850-858): QR of the identity whose first
    column is the normalised vector, sign-fixed so that column 0 sums positive; float64 numpy, then fp32."""
    vec = np.asarray(vector)
    vec = vec / np.linalg.norm(vec)
    m = np.eye(len(vec))
    m[:, 0] = vec
    m = np.linalg.qr(m)[0]
    if np.sum(m[:, 0]) < 0:
        m = -m
    return torch.from_numpy(m).to(torch.float32)


def colour_basis():
    """3x3 Q of iterative_colorization: column 0 along the luma weights (0.2989, 0.5870, 0.1140)."""
    if "colour" not in _Q_CACHE:
        _Q_CACHE["colour"] = _orthogonal([0.2989, 0.5870, 0.1140])
    return _Q_CACHE["colour"]


def patch_basis():
    """64x64 Q of iterative_superres: column 0 along the 8x8 patch mean."""
    if "patch" not in _Q_CACHE:
        _Q_CACHE["patch"] = _orthogonal([1] * 64)
    return _Q_CACHE["patch"]


def _check_cm_args(distiller, x):
    _check_sampler_args(distiller, x, edm=False)


@torch.no_grad()
def sample_onestep(distiller, x, sigmas, generator=None, progress=False, callback=None):
    """Single-step generation from a distilled model (reference :644-655): the denoiser at sigmas[0].  distiller: a
    KarrasDenoiserFn whose diffusion has distillation=True.  callback, if given, sees {x, i, sigma, denoised} once per
    evaluation (the reference accepts and ignores it)."""
    _check_cm_args(distiller, x)
    sch = _cm_schedule("onestep", distiller.diffusion, None, 1, 0.002, 80.0, 7.0, distiller.clip_denoised, 1.0, False,
                       sigma0=float(torch.as_tensor(sigmas[0], dtype=torch.float32)))
    return _run_stages(sch, distiller, x, tuple(x.shape), x.device, generator, callback, progress)


@torch.no_grad()
def stochastic_iterative_sampler(distiller, x, sigmas, generator, ts, progress=False, callback=None, t_min=0.002, t_max=80.0,
                                 rho=7.0, steps=40):
    """The multistep consistency sampler (reference :658-683).  NFE = len(ts) - 1; returns x after the last step's noise,
    unclamped.  generator: None draws on the device (skipping a draw whose factor is 0); else one randn_like per step."""
    _check_ts(ts, steps)
    _check_cm_args(distiller, x)
    sch = _cm_schedule("multistep", distiller.diffusion, ts, steps, t_min, t_max, rho, distiller.clip_denoised, 1.0, False)
    return _run_stages(sch, distiller, x, tuple(x.shape), x.device, generator, callback, progress)


# ------------------------------------------------------------------------------------------------------ zero-shot editing
def _patches(v):
    """[N, C, H, W] -> [N, C, H/8, W/8, 64] view order of the reference's permute(0, 1, 2, 4, 3, 5) flattening."""
    N, C, H, W = v.shape
    return v.reshape(N, C, H // 8, 8, W // 8, 8).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 8, W // 8, 64)


def _unpatches(p, shape):
    N, C, H, W = shape
    return p.reshape(N, C, H // 8, W // 8, 8, 8).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H, W)


def inpainting_mask(n, image_size, font_path=None):
    """The reference's inpainting mask (:781-801): the letter "S" drawn at (50, 0) in a 250-point TrueType font on a white
    image_size x image_size image; groups of 7 images alternate between keeping the letter's background and the letter
    itself.  -> fp32 [n, 3, image_size, image_size].  The reference hard-codes arial.ttf: pass the font file here."""
    import os
    if n % 7 != 0:
        raise ValueError(f"the letter mask alternates groups of 7 images: n ({n}) must be a multiple of 7 (or pass mask=)")
    if not font_path:
        raise ValueError("inpainting_mask needs font_path: a TrueType font file to draw the letter with (the reference uses "
                         "arial.ttf)")
    if not os.path.isfile(font_path):
        raise FileNotFoundError(f"inpainting_mask: font file {font_path!r} not found")
    from PIL import Image, ImageDraw, ImageFont
    img = Image.new("RGB", (image_size, image_size), color="white")
    ImageDraw.Draw(img).text((50, 0), "S", font=ImageFont.truetype(font_path, 250), fill=(0, 0, 0))
    img_th = torch.from_numpy(np.array(img).transpose(2, 0, 1).copy())
    mask = torch.zeros(n // 7, 7, 3, image_size, image_size)
    mask[::2, :, img_th > 0.5] = 1.0
    mask[1::2, :, img_th < 0.5] = 1.0
    return mask.reshape(n, 3, image_size, image_size)


def _edit_args(distiller, images, x, ts, steps, generator):
    ts = _check_ts(ts, steps)
    if images.shape != x.shape:
        raise ValueError(f"images {tuple(images.shape)} and x {tuple(x.shape)} differ in shape")
    return ts, _as_f32(images, x.device)


def _edit(distiller, x, ts, t_min, t_max, rho, steps, generator, edit, Q, ref, mask=None):
    # the editing loops clamp x0 themselves (:758, :819, :938): CLIP is on whatever clip_denoised says
    sch = _cm_schedule("multistep", distiller.diffusion, ts, steps, t_min, t_max, rho, True, 1.0, False)
    return _run_stages(sch, distiller, x, tuple(x.shape), x.device, generator, edit=edit, Q=Q, ref=ref, mask=mask)


@torch.no_grad()
def iterative_colorization(distiller, images, x, ts, t_min=0.002, t_max=80.0, rho=7.0, steps=40, generator=None):
    """Zero-shot colourisation (reference :722-771): keep the luma coefficient of `images`, let the model fill the two chroma
    coefficients.  -> (x, the greyscale view of images), unclamped.  generator=None draws on the device."""
    if x.shape[1] != 3:
        raise ValueError("iterative_colorization needs 3 channels")
    _check_cm_args(distiller, x)
    ts, images = _edit_args(distiller, images, x, ts, steps, generator)
    Q = colour_basis().to(x.device)
    y = torch.einsum("bchw,cd->bdhw", images, Q)
    y[:, 1:] = 0.0
    images = torch.einsum("bdhw,cd->bchw", y, Q).contiguous()          # replacement(images, 0)
    return _edit(distiller, x, ts, t_min, t_max, rho, steps, generator, ops.CM_EDIT_COLOUR, Q, images), images


@torch.no_grad()
def iterative_inpainting(distiller, images, x, ts, t_min=0.002, t_max=80.0, rho=7.0, steps=40, generator=None, mask=None,
                         font_path=None):
    """Zero-shot inpainting (reference :774-832): where mask = 1 keep `images`, elsewhere let the model fill.  mask: fp32
    [N, C, H, W]; without it the reference's letter mask (inpainting_mask, needs font_path and N % 7 == 0).
    -> (x, images with the masked-out part set to -1), unclamped."""
    ts = _check_ts(ts, steps)
    if mask is None:
        if x.shape[-1] != x.shape[-2] or x.shape[1] != 3:
            raise ValueError("the letter mask needs square 3-channel images; pass mask=")
        mask = inpainting_mask(x.shape[0], x.shape[-1], font_path)
    if tuple(mask.shape) != tuple(x.shape):
        raise ValueError(f"mask {tuple(mask.shape)} must have the images' shape {tuple(x.shape)}")
    _check_cm_args(distiller, x)
    ts, images = _edit_args(distiller, images, x, ts, steps, generator)
    mask = _as_f32(mask, x.device)
    images = (images * mask + (-torch.ones_like(images)) * (1 - mask)).contiguous()     # replacement(images, -1)
    return _edit(distiller, x, ts, t_min, t_max, rho, steps, generator, ops.CM_EDIT_MASK, None, images, mask), images


@torch.no_grad()
def iterative_superres(distiller, images, x, ts, t_min=0.002, t_max=80.0, rho=7.0, steps=40, generator=None):
    """Zero-shot 8x super-resolution (reference :835-951): keep each 8x8 patch's mean of `images`, let the model fill the other
    63 coefficients of the patch basis.  H and W must be multiples of 8.  -> (x, the patch-averaged images), unclamped."""
    if x.dim() != 4 or x.shape[-1] % 8 or x.shape[-2] % 8:
        raise ValueError(f"iterative_superres needs H and W multiples of 8 (got {tuple(x.shape)})")
    _check_cm_args(distiller, x)
    ts, images = _edit_args(distiller, images, x, ts, steps, generator)
    p = _patches(images)
    images = _unpatches(p.mean(dim=-1, keepdim=True).expand_as(p), images.shape).contiguous()   # average_image_patches
    Q = patch_basis().to(x.device)
    return _edit(distiller, x, ts, t_min, t_max, rho, steps, generator, ops.CM_EDIT_PATCH, Q, images), images
