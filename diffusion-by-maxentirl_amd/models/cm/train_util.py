"""Denoising score-matching training of the EDM U-Net (`models.cm.train_util.TrainLoop`; reference: models/cm/train_util.py:29-264).

Same keyword arguments and methods as the reference (run_loop, run_step, forward_backward with microbatches, _update_ema,
_anneal_lr, save; checkpoints model%06d.pt, ema_{rate}_%06d.pt, opt%06d.pt next to each other, resumed from the model file's
step).  What differs:
  * the loss is KarrasDenoiser.training_losses on the HIP U-Net (one autograd node around the network, models/cm/karras_diffusion.py);
  * the optimiser is dxmi_hip.optim.RAdam behind MixedPrecisionTrainer, and gradients are exchanged by the trainer's
    dxmi_hip.dist.FlatGradSync in optimize() (the reference wraps the model in DDP);
  * every EMA rate is updated by one dxmi_ema_update launch series that reads the master weights once (nn.update_ema_rates);
  * `schedule_sampler` is required (the reference's default UniformSampler needs a num_timesteps KarrasDenoiser lacks: use
    models.cm.resample.LogNormalSampler), and `log_dir` replaces blobfile's get_blob_logdir();
  * the logged terms are summed on the device and read back once per `log_interval` steps (dumpkvs), as their means.
The reference's bookkeeping is kept as it is: the step counter advances, and the EMA moves, only on steps the optimiser took
(an fp16 overflow skips both); after a resume `step` starts at the resumed step and _anneal_lr / save add resume_step to it.

CMTrainLoop (reference :267-566) trains a consistency model by distillation from an EDM teacher or by consistency training, with
KarrasDenoiser.consistency_losses.  It keeps the reference's own bookkeeping, which differs from TrainLoop's: `step` and
`global_step` advance AFTER the EMA updates of a step the optimiser took, the target network follows the masters by an EMA whose
rate comes from ema_scale_fn(global_step) (one dxmi_ema_update launch series on the device; rate 0, the stop-gradient student of
improved consistency training, is a copy bit for bit), checkpoints are named by
global_step, and target_model%06d.pt (plus, with the first save, teacher_model%06d.pt) is written next to TrainLoop's files and
read back on resume (a checkpoint later than the first finds the teacher under the first save's name in the same directory;
where there is none, the teacher the caller passed is kept).  An fp16 overflow step skips the target EMA on the host, from the
flag optimize() has already read back, so its eager launch passes no found_inf.

training_mode="progdist" (reference :305-318, :388-442, :456-476, :551-555) is progressive distillation with
KarrasDenoiser.progdist_losses: ema_scale_fn's ("fixed", "progdist") schedule halves num_scales; the first phase distils
teacher_model under teacher_diffusion, and after the step at which num_scales changes reset_training_for_progdist copies the student
into teacher_model (fresh RAdam, EMA series restarted from the masters, lr_anneal_steps doubled at num_scales 2, step = 0), so every
later phase distils the previous phase's student under the student's own diffusion.  teacher_model%06d.pt is written with EVERY
save and a resume reads the file of the resumed step.  target_model may be None; one that is given stays in eval mode, is saved,
and neither enters the loss nor is moved by an EMA.  `step` is the phase's own counter (the learning rate anneals on it alone).
use_graph=True is refused in this mode.  Where this differs from the reference's call site, which cannot run: DESIGN 5.28.

DMTrainLoop (not in the reference) distils the EDM teacher into a one-step generator by distribution matching
(KarrasDenoiser.dm_generator_losses): the generator and an online-trained fake denoiser have a trainer and an optimiser each and are
updated on two clocks; the data are latents.  It refuses use_graph=True.

use_graph=True (the first two loops; off by default) replays a whole step from hipGraphs (dxmi_hip/graph.py StepGraph): the first run_step
runs eagerly (weight packs, workspaces, optimiser state), the second is captured, later ones are host producers + one upload + the
graph launches.  Captured is everything run_step does on the device: zero_grad, every microbatch of forward_backward (sigma, index
and noise draws are torch device RNG), the gradient exchange (a cut: the collectives run eagerly between two graph launches), the
norm + RAdam launches (loss scale, RAdam scalars and lr are host inputs), every EMA launch series and, for CMTrainLoop, the target's
EMA and the refresh of its packed weights.  The batch and cond["y"] are the graph's tensor arguments.  Nothing on the host decides
per step: both EMA series take the device overflow flag of the iteration as found_inf; after the launches ONE read-back (norms, flag,
the logged terms of every microbatch) feeds MixedPrecisionTrainer.finish_replay, and the same flag advances or holds the counters.
What a capture freezes by value is the pair ema_scale_fn(global_step) = (target EMA rate, num_scales): the graph is keyed on it
(_KeyedStepGraph), a changed pair drops the graph (and its pool) and captures a new one at once, so only one graph is alive.  The
logged terms are summed in fp32 on the host in the order the eager loop sums them on the device, so the rows are the same.
Refused at construction: use_fp16 off or masters that are not device-aliased (the trainer's captured path), loss_norm="lpips", a
schedule_sampler that draws on the host; a CPU model runs eagerly.
"""
import json
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from dxmi_hip import graph as _graph
from dxmi_hip.dist import broadcast_parameters, is_distributed
from dxmi_hip.optim import RAdam

from .fp16_util import MixedPrecisionTrainer, get_param_groups_and_shapes, make_master_params, master_params_to_model_params
from .karras_diffusion import gen_ladder
from .nn import update_ema, update_ema_rates

INITIAL_LOG_LOSS_SCALE = 20.0


def _rank():
    return dist.get_rank() if is_distributed() else 0


def _world():
    return dist.get_world_size() if is_distributed() else 1


class _KeyedStepGraph:
    """At most ONE StepGraph, the one of the current key: graph(key) is built by build(key) on first use and whenever the key
    differs from the one held; the graph held before is dropped first (drop(): on_drop(), then its references, so that its pool is
    free before the next capture).  captures / replays count over every graph this object has held."""

    def __init__(self, build, on_drop=None):
        self.build, self.on_drop = build, on_drop
        self.key, self.graph = None, None
        self.captures = self.replays = self.builds = 0

    def drop(self):
        if self.graph is not None and self.on_drop is not None:
            self.on_drop()
        self.key, self.graph = None, None

    def __call__(self, key, *args):
        if self.graph is None or key != self.key:
            self.drop()
            self.graph, self.key = self.build(key), key
            self.builds += 1
        g = self.graph
        c0, r0 = g.captures, g.replays
        try:
            return g(*args)
        finally:
            self.captures += g.captures - c0
            self.replays += g.replays - r0


class TrainLoop:
    def __init__(self, *, model, diffusion, data, batch_size, microbatch, lr, ema_rate, log_interval, save_interval,
                 resume_checkpoint, use_fp16=False, fp16_scale_growth=1e-3, schedule_sampler=None, weight_decay=0.0,
                 lr_anneal_steps=0, log_dir=None, use_graph=False):
        if schedule_sampler is None:
            raise ValueError("TrainLoop: schedule_sampler is required (e.g. models.cm.resample.LogNormalSampler())")
        if use_graph:
            if not use_fp16:
                raise NotImplementedError("use_graph=True needs use_fp16=True: a captured step keeps the loss scale, the overflow flag and "
                                          "the RAdam scalars on the device, which only MixedPrecisionTrainer's fp16 path (flat masters "
                                          "aliased by the model parameters) does")
            if getattr(diffusion, "loss_norm", None) == "lpips":
                raise NotImplementedError("use_graph=True with loss_norm='lpips': LPIPS refuses a StepGraph capture (models/cm/lpips.py); "
                                          "train eagerly, or with l1 / l2 / l2-32")
            if getattr(schedule_sampler, "generator", None) is not None:
                raise NotImplementedError("use_graph=True needs a schedule_sampler that draws on the device (generator=None): with a "
                                          "generator the sampler draws on the host, which cannot be captured")
        self.model, self.diffusion, self.data = model, diffusion, data
        self.batch_size = batch_size
        self.microbatch = microbatch if microbatch > 0 else batch_size
        self.lr = lr
        self.ema_rate = [ema_rate] if isinstance(ema_rate, float) else [float(x) for x in str(ema_rate).split(",")]
        self.log_interval, self.save_interval = log_interval, save_interval
        self.resume_checkpoint = resume_checkpoint
        self.use_fp16, self.fp16_scale_growth = use_fp16, fp16_scale_growth
        self.schedule_sampler = schedule_sampler
        self.weight_decay, self.lr_anneal_steps = weight_decay, lr_anneal_steps
        self.log_dir = log_dir or os.getcwd()
        self.device = next(model.parameters()).device

        self.step = 0
        self.resume_step = 0
        self.global_batch = self.batch_size * _world()

        self._load_and_sync_parameters()
        self.mp_trainer = MixedPrecisionTrainer(model=self.model, use_fp16=self.use_fp16, fp16_scale_growth=fp16_scale_growth)
        self.opt = RAdam(self.mp_trainer.master_params, lr=self.lr, weight_decay=self.weight_decay)
        if self.resume_step:
            self._load_optimizer_state()
            self.ema_params = [self._load_ema_parameters(rate) for rate in self.ema_rate]
        else:
            self.ema_params = [[p.detach().clone() for p in self.mp_trainer.master_params] for _ in self.ema_rate]
        self.ddp_model = self.model
        self.step = self.resume_step
        self._log_sums, self._log_count, self.logged = {}, 0, []
        self.use_graph = bool(use_graph) and self.device.type == "cuda"      # a CPU model runs eagerly
        if self.use_graph and not self.mp_trainer._aliased:
            raise NotImplementedError("use_graph=True needs masters that the model parameters alias on the device (contiguous fp32 "
                                      "CUDA parameters): MixedPrecisionTrainer captures no other layout")
        self._graph = _KeyedStepGraph(self._build_graph, self._on_graph_drop) if self.use_graph else None
        self._graph_warm = False
        self._cap_log = self._cap_keys = None

    # ------------------------------------------------------------------ checkpoints
    def _load_and_sync_parameters(self):
        if self.resume_checkpoint:
            self.resume_step = parse_resume_step_from_filename(self.resume_checkpoint)
            self.model.load_state_dict(torch.load(self.resume_checkpoint, map_location=self.device))
        broadcast_parameters(self.model)

    def _load_ema_parameters(self, rate):
        ema_params = [p.detach().clone() for p in self.mp_trainer.master_params]
        ema_checkpoint = find_ema_checkpoint(self.resume_checkpoint, self.resume_step, rate)
        if ema_checkpoint:
            state_dict = torch.load(ema_checkpoint, map_location=self.device)
            ema_params = [p.detach().clone().contiguous() for p in self.mp_trainer.state_dict_to_master_params(state_dict)]
        if is_distributed():
            with torch.no_grad():
                for p in ema_params:
                    dist.broadcast(p, 0)
        return ema_params

    def _load_optimizer_state(self):
        opt_checkpoint = os.path.join(os.path.dirname(self.resume_checkpoint), f"opt{self.resume_step:06}.pt")
        if os.path.exists(opt_checkpoint):
            self.opt.load_state_dict(torch.load(opt_checkpoint, map_location=self.device))

    def save(self):
        def save_checkpoint(rate, params):
            state_dict = self.mp_trainer.master_params_to_state_dict(params)
            if _rank() == 0:
                name = f"model{(self.step + self.resume_step):06d}.pt" if not rate else f"ema_{rate}_{(self.step + self.resume_step):06d}.pt"
                torch.save({k: v.detach().clone() for k, v in state_dict.items()}, os.path.join(self.log_dir, name))

        os.makedirs(self.log_dir, exist_ok=True)
        for rate, params in zip(self.ema_rate, self.ema_params):
            save_checkpoint(rate, params)
        if _rank() == 0:
            torch.save(self.opt.state_dict(), os.path.join(self.log_dir, f"opt{(self.step + self.resume_step):06d}.pt"))
        save_checkpoint(0, self.mp_trainer.master_params)     # last: a restart never finds a model without its opt / EMA files
        if is_distributed():
            dist.barrier()

    # ------------------------------------------------------------------ loop
    def run_loop(self):
        while not self.lr_anneal_steps or self.step < self.lr_anneal_steps:
            batch, cond = next(self.data)
            self.run_step(batch, cond)
            if self.step % self.log_interval == 0:
                self.dumpkvs()
            if self.step % self.save_interval == 0:
                self.save()
                if os.environ.get("DIFFUSION_TRAINING_TEST", "") and self.step > 0:
                    return
        if (self.step - 1) % self.save_interval != 0:
            self.save()

    def run_step(self, batch, cond):
        took_step = self._step_replayed(batch, cond) if self.use_graph and self._graph_warm else self._step_on_device(batch, cond)
        self._graph_warm = True
        if took_step:
            self._count_step()
        self._anneal_lr()
        self.log_step()
        return took_step

    def _step_on_device(self, batch, cond):
        """The device work of an eager step -> took_step (read back by optimize()); the EMAs move only on a step that was taken."""
        self.forward_backward(batch, cond)
        took_step = self.mp_trainer.optimize(self.opt)
        if took_step:
            self._update_emas()
        return took_step

    def _count_step(self):
        self.step += 1

    def _update_emas(self, found_inf=None):
        self._update_ema(found_inf)

    def forward_backward(self, batch, cond):
        self.mp_trainer.zero_grad()
        for i in range(0, batch.shape[0], self.microbatch):
            micro = batch[i:i + self.microbatch].to(self.device)
            micro_cond = {k: v[i:i + self.microbatch].to(self.device) for k, v in cond.items()}
            sigmas, weights = self.schedule_sampler.sample(micro.shape[0], self.device)
            losses = self.diffusion.training_losses(self.ddp_model, micro, sigmas, model_kwargs=micro_cond)
            loss = (losses["loss"] * weights).mean()
            self._log_loss_dict({k: v * weights for k, v in losses.items()})
            self.mp_trainer.backward(loss)

    def _update_ema(self, found_inf=None):
        """found_inf: device fp32 flag (a captured step: the launches skip on it, as the optimiser's do)."""
        masters = self.mp_trainer.master_params
        if all(p.is_cuda for p in masters):
            update_ema_rates(self.ema_params, masters, self.ema_rate, found_inf=found_inf)
            return
        for rate, params in zip(self.ema_rate, self.ema_params):
            update_ema(params, masters, rate=rate, found_inf=found_inf)

    # ------------------------------------------------------------------ hipGraph replay of the step (use_graph=True)
    def _graph_key(self):
        """What the captured step freezes by value, beyond the shapes of its arguments."""
        return ()

    def _graph_modules(self):
        return _graph.pack_modules(self.model)

    def _before_capture(self, key):
        """Host work a capture cannot hold (uploads), for the graph of `key`."""

    def _build_graph(self, key):
        self._before_capture(key)
        return _graph.StepGraph(self._captured_step, self.device, warmup=0, modules=self._graph_modules(),
                                name=f"{type(self).__name__}.run_step{key}")

    def _on_graph_drop(self):
        self.mp_trainer.__dict__.pop("_cap_state", None)      # tensors of the dropped graph's pool
        self._cap_log = self._cap_keys = None

    def _captured_step(self, batch, *y):
        """The body of the StepGraph: the device work of run_step, with the device overflow flag where the eager step branches on
        the host -> fp32 [3 + terms]: (scaled gradient norm, parameter norm, overflow flag), then every logged term of every
        microbatch in the order _log_loss_dict met them."""
        self.mp_trainer.begin_captured(self.opt)
        self._cap_log = log = []
        try:
            self.forward_backward(batch, {"y": y[0]} if y else {})
        finally:
            self._cap_log = None                 # _log_loss_dict sums on the device again (a capture that failed included)
        self.mp_trainer.optimize(self.opt)
        self._update_emas(self.mp_trainer.captured_found_inf())
        self._cap_keys = [k for k, _ in log]
        return torch.cat([self.mp_trainer.captured_stats().reshape(-1)] + [m.reshape(1) for _, m in log])

    def _step_replayed(self, batch, cond):
        """run_step's device work from the graph of the current key (captured by this call if there is none) -> took_step."""
        extra = set(cond) - {"y"}
        if extra:
            raise NotImplementedError(f"use_graph=True: cond entries {sorted(extra)} are not inputs of the captured step (only 'y' is)")
        if any(torch.is_tensor(v) for v in self._log_sums.values()):      # sums an eager step left on the device: to the host
            keys = list(self._log_sums)
            vals = torch.stack([torch.as_tensor(self._log_sums[k], dtype=torch.float32, device=self.device) for k in keys]).tolist()
            self._log_sums = {k: np.float32(v) for k, v in zip(keys, vals)}
        args = [batch.to(self.device)] + ([cond["y"].to(self.device)] if "y" in cond else [])
        out = self._graph(self._graph_key(), *args).tolist()               # the step's ONE read-back
        took_step = self.mp_trainer.finish_replay(self.opt, [out[:3]]) == 1
        with np.errstate(over="ignore", invalid="ignore"):
            for k, v in zip(self._cap_keys, out[3:]):                        # fp32 sums in the eager loop's order
                self._log_sums[k] = self._log_sums[k] + np.float32(v) if k in self._log_sums else np.float32(v)
        self._log_count += len(self._cap_keys) // max(1, len(set(self._cap_keys)))
        return took_step

    def _anneal_lr(self):
        if not self.lr_anneal_steps:
            return
        frac_done = (self.step + self.resume_step) / self.lr_anneal_steps
        lr = self.lr * (1 - frac_done)
        for param_group in self.opt.param_groups:
            param_group["lr"] = lr

    # ------------------------------------------------------------------ logging
    def _log_loss_dict(self, losses):
        """Device sums of every term's batch mean (no host sync); dumpkvs() reads them."""
        if self._cap_log is not None:        # a step being captured: the means are outputs of the graph (_step_replayed sums them)
            self._cap_log += [(k, v.detach().float().mean()) for k, v in losses.items()]
            return
        for k, v in losses.items():
            m = v.detach().float().mean()
            self._log_sums[k] = self._log_sums[k] + m if k in self._log_sums else m
        self._log_count += 1

    def log_step(self):
        self._kv = {"step": self.step + self.resume_step, "samples": (self.step + self.resume_step + 1) * self.global_batch}

    def dumpkvs(self):
        """Means of the logged terms since the last dump: ONE device-to-host read.  Appended to self.logged, and written as a
        JSON line to log_dir/progress.jsonl on rank 0."""
        row = dict(getattr(self, "_kv", {}))
        if self._log_count:
            keys = sorted(self._log_sums)
            sums = [self._log_sums[k] for k in keys]           # device tensors (eager steps) or fp32 host sums (replayed steps)
            vals = torch.stack(sums).tolist() if all(torch.is_tensor(v) for v in sums) else [float(v) for v in sums]
            row.update({k: v / self._log_count for k, v in zip(keys, vals)})
        row.update({k: v for k, v in self.mp_trainer.log.items()})
        self._log_sums, self._log_count = {}, 0
        self.logged.append(row)
        if _rank() == 0:
            os.makedirs(self.log_dir, exist_ok=True)
            with open(os.path.join(self.log_dir, "progress.jsonl"), "a") as f:
                f.write(json.dumps(row) + "\n")
        return row


class CMTrainLoop(TrainLoop):
    def __init__(self, *, target_model, teacher_model, teacher_diffusion, training_mode, ema_scale_fn, total_training_steps,
                 index_sampler=None, **kwargs):
        """kwargs: TrainLoop's, use_graph among them.  index_sampler: what draws the ladder index of every sample in
        consistency_losses (models.cm.resample.DiscreteLogNormalSampler); None: the loss's own uniform randint."""
        progdist = training_mode == "progdist"
        if training_mode not in ("consistency_distillation", "consistency_training", "progdist"):
            raise ValueError(f"Unknown training mode {training_mode}")
        if progdist:
            if teacher_model is None or teacher_diffusion is None:
                raise NotImplementedError("CMTrainLoop: progdist must have a teacher_model and its teacher_diffusion")
            if kwargs.get("use_graph"):
                raise NotImplementedError("CMTrainLoop: use_graph=True with training_mode='progdist' is not supported: a phase change "
                                          "replaces the optimiser and the EMA buffers and rewrites the teacher under a live capture; "
                                          "train this mode eagerly")
        elif target_model is None:
            raise NotImplementedError("Must have a target model")
        if training_mode == "consistency_distillation" and (teacher_model is None or teacher_diffusion is None):
            raise ValueError("CMTrainLoop: consistency_distillation needs teacher_model and teacher_diffusion")
        if index_sampler is not None and progdist:
            raise NotImplementedError("CMTrainLoop: index_sampler belongs to consistency_losses; progdist_losses draws its own indices")
        if kwargs.get("schedule_sampler") is None:      # the losses draw their own levels: only `weights` is used
            kwargs["schedule_sampler"] = _UnitWeights()
        self.index_sampler = index_sampler
        super().__init__(**kwargs)
        self.training_mode, self.ema_scale_fn = training_mode, ema_scale_fn
        self.target_model, self.teacher_model, self.teacher_diffusion = target_model, teacher_model, teacher_diffusion
        self.total_training_steps = total_training_steps
        self._teacher_saved = False

        if self.target_model is not None:
            self._load_and_sync_side_model(self.target_model, "target_model")
            self.target_model.requires_grad_(False)
            self.target_model.train()
            if self.use_fp16:   # flat fp32 masters in the trainer's groups, the target parameters views of them on the device
                self.target_model_param_groups_and_shapes = get_param_groups_and_shapes(self.target_model.named_parameters())
                self.target_model_master_params = [p.detach().requires_grad_(False) for p in
                                                   make_master_params(self.target_model_param_groups_and_shapes)]
                _alias_params_into_masters(self.target_model_param_groups_and_shapes, self.target_model_master_params)
            else:               # the trainer's masters are the model parameters themselves: so are the target's
                self.target_model_param_groups_and_shapes = None
                self.target_model_master_params = [p.detach() for p in self.target_model.parameters()]
        if self.teacher_model is not None:
            self._load_and_sync_side_model(self.teacher_model, "teacher_model")
            self.teacher_model.requires_grad_(False)
            self.teacher_model.eval()
        self.global_step = self.step
        if progdist:        # reference :305-318: `step` counts within the phase of the resumed global_step
            if self.target_model is not None:
                self.target_model.eval()
            if self.lr_anneal_steps:
                _, scale = ema_scale_fn(self.global_step)
                if scale == 1 or scale == 2:
                    _, start_scale = ema_scale_fn(0)
                    n_normal_steps = int(np.log2(start_scale // 2)) * self.lr_anneal_steps
                    step = self.global_step - n_normal_steps
                    if step != 0:
                        self.lr_anneal_steps *= 2
                        self.step = step % self.lr_anneal_steps
                    else:
                        self.step = 0
                else:
                    self.step = self.global_step % self.lr_anneal_steps

    def _load_and_sync_side_model(self, net, prefix):
        if self.resume_checkpoint:
            path, name = os.path.split(self.resume_checkpoint)
            ckpt = os.path.join(path, name.replace("model", prefix))
            if not os.path.exists(ckpt) and prefix == "teacher_model" and self.training_mode == "progdist":
                # the teacher changes at every phase: only the file of the resumed step holds the one this step distils from
                raise FileNotFoundError(f"CMTrainLoop: resuming progdist needs {ckpt} (the teacher is written at every save)")
            if not os.path.exists(ckpt) and prefix == "teacher_model":
                # the teacher never changes and is written with the first save only: a later checkpoint resumes from that file
                found = sorted(f for f in os.listdir(path or ".") if f.startswith("teacher_model") and f.endswith(".pt"))
                if found:
                    ckpt = os.path.join(path, found[0])
            if os.path.exists(ckpt):
                net.load_state_dict(torch.load(ckpt, map_location=self.device))
        broadcast_parameters(net)
        if is_distributed():
            with torch.no_grad():
                for b in net.buffers():
                    dist.broadcast(b, 0)

    def run_loop(self):
        saved = False
        while not self.lr_anneal_steps or self.step < self.lr_anneal_steps or self.global_step < self.total_training_steps:
            batch, cond = next(self.data)
            self.run_step(batch, cond)
            saved = False
            if self.global_step and self.save_interval != -1 and self.global_step % self.save_interval == 0:
                self.save()
                saved = True
                if os.environ.get("DIFFUSION_TRAINING_TEST", "") and self.step > 0:
                    return
            if self.global_step % self.log_interval == 0:
                self.dumpkvs()
        if not saved:
            self.save()

    def _count_step(self):      # after the EMA updates of the step: _update_target_ema reads global_step before it moves
        self.step += 1
        self.global_step += 1

    def _update_emas(self, found_inf=None):
        """Eagerly only on a step the optimiser took (an fp16 overflow step moves neither EMA: optimize() has read the flag back
        already); in a captured step always, with the device flag."""
        self._update_ema(found_inf)
        if self.training_mode == "progdist":     # the target, if any, takes no part (rate 1.0: its EMA launch series is skipped)
            self.reset_training_for_progdist()
        else:
            self._update_target_ema(found_inf)

    def reset_training_for_progdist(self):
        """Reference :416-442, in its place: after the EMA updates of a step the optimiser took, before the counters advance.  When
        that step was the first of a new num_scales, the student becomes the teacher of the phase that has begun: its weights are
        copied into teacher_model (and the teacher's packed weights refreshed: forward_inference reads those), the optimiser is a
        fresh RAdam over the masters, every EMA series restarts from the masters, lr_anneal_steps doubles for num_scales 2, and
        `step` restarts."""
        assert self.training_mode == "progdist", "Training mode must be progdist"
        if self.global_step <= 0:
            return
        scales, scales2 = self.ema_scale_fn(self.global_step)[1], self.ema_scale_fn(self.global_step - 1)[1]
        if scales == scales2:
            return
        with torch.no_grad():
            for pt, ps in zip(self.teacher_model.parameters(), self.model.parameters()):
                pt.copy_(ps.detach())
        net = self.teacher_model.module if hasattr(self.teacher_model, "module") else self.teacher_model
        if hasattr(net, "refresh_packs") and next(net.parameters()).is_cuda:
            net.refresh_packs()
        # a fresh optimiser of the loop's own kind (RAdam; a host test stands torch's in for it), with no state
        self.opt = type(self.opt)(self.mp_trainer.master_params, lr=self.lr, weight_decay=self.weight_decay)
        self.ema_params = [[p.detach().clone() for p in self.mp_trainer.master_params] for _ in self.ema_rate]
        if scales == 2:
            self.lr_anneal_steps *= 2
        self.teacher_model.eval()
        self.step = 0

    def _anneal_lr(self):
        if self.training_mode != "progdist":
            return super()._anneal_lr()
        if not self.lr_anneal_steps:
            return
        lr = self.lr * (1 - self.step / self.lr_anneal_steps)      # `step` is the phase's own count here, after a resume too (:305-318)
        for param_group in self.opt.param_groups:
            param_group["lr"] = lr

    def _graph_key(self):
        return self.ema_scale_fn(self.global_step)

    def _graph_modules(self):
        nets = [n for n in (self.model, self.target_model, self.teacher_model) if n is not None]
        return [m for net in nets for m in _graph.pack_modules(net)]

    def _before_capture(self, key):
        d = self.diffusion
        if all(hasattr(d, a) for a in ("sigma_min", "sigma_max", "rho")):       # the level table of this key: uploaded, not captured
            from .karras_diffusion import cd_levels
            # held for as long as the graph lives: the graph has the table's address, the cache of level sets may be emptied
            self._cap_table = cd_levels(key[1], d.sigma_min, d.sigma_max, d.rho).device_table(self.device)
        if self.index_sampler is not None and hasattr(self.index_sampler, "cdf"):      # its CDF over the levels of this key, likewise
            self._cap_cdf = self.index_sampler.cdf(key[1]).device_table(self.device)

    def _on_graph_drop(self):
        super()._on_graph_drop()
        self._cap_table = self._cap_cdf = None

    def _update_target_ema(self, found_inf=None):
        target_ema, _ = self.ema_scale_fn(self.global_step)
        with torch.no_grad():
            update_ema(self.target_model_master_params, [p.detach() for p in self.mp_trainer.master_params], rate=target_ema,
                       found_inf=found_inf)
            if self.target_model_param_groups_and_shapes is not None:
                master_params_to_model_params(self.target_model_param_groups_and_shapes, self.target_model_master_params)
            else:
                torch.autograd.graph.increment_version(list(self.target_model.parameters()))
        net = self.target_model.module if hasattr(self.target_model, "module") else self.target_model
        if hasattr(net, "refresh_packs") and next(net.parameters()).is_cuda:
            net.refresh_packs()

    def forward_backward(self, batch, cond):
        self.mp_trainer.zero_grad()
        for i in range(0, batch.shape[0], self.microbatch):
            micro = batch[i:i + self.microbatch].to(self.device)
            micro_cond = {k: v[i:i + self.microbatch].to(self.device) for k, v in cond.items()}
            _, weights = self.schedule_sampler.sample(micro.shape[0], self.device)
            _, num_scales = self.ema_scale_fn(self.global_step)
            if self.training_mode == "progdist":
                # the first phase distils the given teacher under its own diffusion; every later one the previous phase's student,
                # which reset_training_for_progdist copied into teacher_model, under the student's diffusion (reference :456-476,
                # whose keyword names progdist_losses does not take: DESIGN 5.28)
                first = num_scales == self.ema_scale_fn(0)[1]
                losses = self.diffusion.progdist_losses(self.ddp_model, micro, num_scales, teacher_model=self.teacher_model,
                                                        teacher_diffusion=self.teacher_diffusion if first else self.diffusion,
                                                        model_kwargs=micro_cond)
                loss = (losses["loss"] * weights).mean()
                self._log_loss_dict({k: v * weights for k, v in losses.items()})
                self.mp_trainer.backward(loss)
                continue
            distill = self.training_mode == "consistency_distillation"
            losses = self.diffusion.consistency_losses(self.ddp_model, micro, num_scales, target_model=self.target_model,
                                                       teacher_model=self.teacher_model if distill else None,
                                                       teacher_diffusion=self.teacher_diffusion if distill else None,
                                                       model_kwargs=micro_cond,
                                                       **({} if self.index_sampler is None else {"index_sampler": self.index_sampler}))
            loss = (losses["loss"] * weights).mean()
            self._log_loss_dict({k: v * weights for k, v in losses.items()})
            self.mp_trainer.backward(loss)

    def save(self):
        step = self.global_step

        def save_checkpoint(rate, params):
            state_dict = self.mp_trainer.master_params_to_state_dict(params)
            if _rank() == 0:
                name = f"model{step:06d}.pt" if not rate else f"ema_{rate}_{step:06d}.pt"
                torch.save({k: v.detach().clone() for k, v in state_dict.items()}, os.path.join(self.log_dir, name))

        os.makedirs(self.log_dir, exist_ok=True)
        for rate, params in zip(self.ema_rate, self.ema_params):
            save_checkpoint(rate, params)
        if _rank() == 0:
            torch.save(self.opt.state_dict(), os.path.join(self.log_dir, f"opt{step:06d}.pt"))
            if self.target_model is not None:
                torch.save({k: v.detach().clone() for k, v in self.target_model.state_dict().items()},
                           os.path.join(self.log_dir, f"target_model{step:06d}.pt"))
            # the teacher of CD never changes: written once; the teacher of progdist changes at every phase: written with every save
            if self.teacher_model is not None and (not self._teacher_saved or self.training_mode == "progdist"):
                torch.save({k: v.detach().clone() for k, v in self.teacher_model.state_dict().items()},
                           os.path.join(self.log_dir, f"teacher_model{step:06d}.pt"))
        self._teacher_saved = True
        save_checkpoint(0, self.mp_trainer.master_params)
        if is_distributed():
            dist.barrier()

    def log_step(self):
        self._kv = {"step": self.global_step, "samples": (self.global_step + 1) * self.global_batch}


class _FakeWithHead(torch.nn.Module):
    """(fake denoiser, GAN head): the one module the fake clock's trainer and optimiser see.  It is never saved as such: the
    fake net and the head keep their own files and their own state-dict keys."""

    def __init__(self, net, head):
        super().__init__()
        self.net, self.head = net, head


class DMTrainLoop(TrainLoop):
    """Distribution matching distillation of an EDM teacher (`real_model` under `real_diffusion`, frozen) into the one-step
    generator `model` (KarrasDenoiser.dm_generator_losses; DMD2's two time-scale rule, its GAN term under gan_head below).  Two trainers on two
    clocks: the generator has TrainLoop's own mp_trainer / opt / EMA series and is updated when step % gen_update_every == 0; the
    fake denoiser `fake_model` has a MixedPrecisionTrainer and RAdam of its own (fake_lr, None = lr; its own loss scale and
    gradient exchange) and is updated at EVERY iteration by denoising score matching on that iteration's generated images, which
    were made before the generator moved.  data yields (z, cond): standard-normal latents of the image shape and {"y": labels}
    for a class-conditional net.  `step` counts iterations and names the checkpoints (no resume_step is added to it); an overflow
    in one trainer skips that trainer's update alone.  save() adds fake_model%06d.pt and fake_opt%06d.pt to TrainLoop's files; a
    resume reads all of them, and a missing fake_model file is an error.  use_graph=True is refused.
    objective: "dmd" (dm_generator_losses under `weighting`) or "sid" (sid_generator_losses at sid_alpha: score identity distillation,
    DESIGN 5.34); only the generator's loss differs, everything else of the loop is the same.  "sida" (sida_generator_losses at
    sid_alpha and sida_gen_weight: adversarial score identity distillation) adds a discriminator WITHOUT parameters,
    the channel mean of the fake net's bottleneck.  It needs real_data and takes no gan_head; on the fake clock every microbatch
    backpropagates (dsm weights).mean() + sida_dis_weight dis.mean(), dis being sida_discriminator_losses on the generated and the
    real microbatch.  The discriminator lives in the fake net: no checkpoint file is added.  One-step generators only.
    gan_head (models.cm.gan_head.GANHead; None: the loop without it): DMD2's GAN term.  It needs real_data, an iterator
    of (x_real NCHW fp32 in [-1, 1], cond).  The head trains with the fake denoiser on its clock: one trainer / RAdam / loss scale
    over (fake net, head), one backward per microbatch of (dsm weights).mean() + gan_dis_weight dis.mean(), dis being
    gan_discriminator_losses on the generated and the real microbatch; the generator's loss gains gan_gen_weight softplus(-logit).
    save() adds gan_head%06d.pt (fake_model%06d.pt stays the bare net's state dict); a resume with a head needs that file, and a
    fake_opt file whose parameter count does not match the run's is an error.
    gen_sigmas (excludes gen_sigma; None: the one-step generator): the ladder of a K-step generator trained by backward simulation
    (dm_generator_losses with gen_sigmas).  Objective "sid" takes one level only.  Checkpoints are unchanged: the ladder
    is an argument of the run, and of dm_sample afterwards."""

    def __init__(self, *, real_model, real_diffusion, fake_model, fake_diffusion=None, num_scales=1000, gen_update_every=5,
                 fake_lr=None, weighting="dmd", gen_sigma=None, min_step_frac=0.02, max_step_frac=0.98, generator=None, objective="dmd",
                 sid_alpha=1.2, gan_head=None, real_data=None, gan_gen_weight=3e-3, gan_dis_weight=1e-2, gan_min_step_frac=0.0,
                 gan_max_step_frac=1.0, gen_sigmas=None, sida_gen_weight=0.01, sida_dis_weight=1.0, **kwargs):
        if kwargs.get("use_graph"):
            raise NotImplementedError("DMTrainLoop: use_graph=True is not supported: the generator and the fake denoiser are updated "
                                      "on two clocks, which needs two captured steps and a graph key per clock; train this mode eagerly")
        if real_model is None or real_diffusion is None or fake_model is None:
            raise NotImplementedError("DMTrainLoop: must have a real_model with its real_diffusion and a fake_model")
        if int(gen_update_every) < 1:
            raise ValueError(f"DMTrainLoop: gen_update_every must be at least 1, got {gen_update_every}")
        if objective not in ("dmd", "sid", "sida"):
            raise ValueError(f"DMTrainLoop: objective {objective!r} is not one of ('dmd', 'sid', 'sida')")
        if objective in ("sid", "sida") and not math.isfinite(float(sid_alpha)):
            raise ValueError(f"DMTrainLoop: sid_alpha must be finite, got {sid_alpha!r}")
        if objective == "sida":
            if gan_head is not None:
                raise ValueError("DMTrainLoop: objective 'sida' takes no gan_head: its discriminator is the channel mean of the fake "
                                 "denoiser's bottleneck and has no parameters of its own")
            if real_data is None:
                raise ValueError("DMTrainLoop: objective 'sida' needs real_data, an iterator of (x_real NCHW fp32 in [-1, 1], cond)")
            for name, v in (("sida_gen_weight", sida_gen_weight), ("sida_dis_weight", sida_dis_weight)):
                if not math.isfinite(float(v)):
                    raise ValueError(f"DMTrainLoop: {name} must be finite, got {v!r}")
        if gan_head is not None and objective == "sid":
            raise NotImplementedError("DMTrainLoop: objective 'sid' takes no gan_head: a discriminator on score identity distillation "
                                      "is SiDA, a different recipe (its own loss weighting and schedule), which is not built here")
        if gan_head is not None and real_data is None:
            raise ValueError("DMTrainLoop: a gan_head needs real_data, an iterator of (x_real NCHW fp32 in [-1, 1], cond)")
        if gen_sigmas is not None:
            if gen_sigma is not None:
                raise ValueError("DMTrainLoop: gen_sigmas (the K-step ladder) excludes gen_sigma (the one-step level): give one of them")
            gen_sigmas = gen_ladder("DMTrainLoop", gen_sigmas).sigmas
            if objective in ("sid", "sida") and len(gen_sigmas) > 1:
                raise NotImplementedError(f"DMTrainLoop: objective {objective!r} is limited to a one-step generator, gen_sigmas has "
                                          f"{len(gen_sigmas)} levels: backward simulation is built for objective 'dmd' alone")
        super().__init__(**kwargs)
        self.gen_sigmas = gen_sigmas
        self.gan_head, self.real_data = gan_head, real_data
        self.gan_gen_weight, self.gan_dis_weight = float(gan_gen_weight), float(gan_dis_weight)
        self.gan_min_step_frac, self.gan_max_step_frac = gan_min_step_frac, gan_max_step_frac
        self.real_model, self.real_diffusion, self.fake_model = real_model, real_diffusion, fake_model
        self.fake_diffusion = real_diffusion if fake_diffusion is None else fake_diffusion
        self.num_scales, self.gen_update_every = int(num_scales), int(gen_update_every)
        self.fake_lr = self.lr if fake_lr is None else fake_lr
        self.weighting, self.gen_sigma, self.generator = weighting, gen_sigma, generator
        self.min_step_frac, self.max_step_frac = min_step_frac, max_step_frac
        self.objective, self.sid_alpha = objective, float(sid_alpha)
        self.sida_gen_weight, self.sida_dis_weight = float(sida_gen_weight), float(sida_dis_weight)
        self.real_model.requires_grad_(False)
        self.real_model.eval()
        if self.resume_checkpoint:      # never restart the fake denoiser from the teacher silently
            ckpt = self._side_file("fake_model")
            if not os.path.exists(ckpt):
                raise FileNotFoundError(f"DMTrainLoop: resuming needs {ckpt} (the fake denoiser is written at every save)")
            self.fake_model.load_state_dict(torch.load(ckpt, map_location=self.device))
            if self.gan_head is not None:
                ckpt = self._side_file("gan_head")
                if not os.path.exists(ckpt):
                    raise FileNotFoundError(f"DMTrainLoop: resuming with a gan_head needs {ckpt} (the head is written at every save)")
                self.gan_head.load_state_dict(torch.load(ckpt, map_location=self.device))
        broadcast_parameters(self.fake_model)
        fake_side = self.fake_model
        if self.gan_head is not None:
            self.gan_head.to(self.device)
            broadcast_parameters(self.gan_head)
            fake_side = _FakeWithHead(self.fake_model, self.gan_head)
        self.fake_trainer = MixedPrecisionTrainer(model=fake_side, use_fp16=self.use_fp16, fp16_scale_growth=self.fp16_scale_growth)
        self.fake_opt = RAdam(self.fake_trainer.master_params, lr=self.fake_lr, weight_decay=self.weight_decay)
        if self.resume_checkpoint and os.path.exists(self._side_file("fake_opt")):
            state = torch.load(self._side_file("fake_opt"), map_location=self.device)
            have = [st["exp_avg"].numel() for st in state["state"].values() if "exp_avg" in st]
            want = [p.numel() for p in self.fake_trainer.master_params]
            saved = sum(len(g["params"]) for g in state["param_groups"])
            if saved != len(want) or (len(have) == len(want) and have != want):
                raise ValueError(f"DMTrainLoop: {self._side_file('fake_opt')} holds the state of {saved} parameters "
                                 f"({sum(have)} elements), this run's fake clock trains {len(want)} ({sum(want)} elements): "
                                 "was the checkpoint written with / without a gan_head?")
            self.fake_opt.load_state_dict(state)
        self.resume_step = 0            # `step` already stands at the resumed step: nothing is added to it again

    def _side_file(self, prefix):
        path, name = os.path.split(self.resume_checkpoint)
        return os.path.join(path, f"{prefix}{parse_resume_step_from_filename(name):06d}.pt")

    def run_loop(self):
        while not self.lr_anneal_steps or self.step < self.lr_anneal_steps:
            batch, cond = next(self.data)
            self.run_step(batch, cond)
            if self.step % self.log_interval == 0:
                self.dumpkvs()
            if self.step % self.save_interval == 0:
                self.save()
                if os.environ.get("DIFFUSION_TRAINING_TEST", "") and self.step > 0:
                    return
        if self.step % self.save_interval != 0:
            self.save()

    def run_step(self, batch, cond):
        """One iteration -> (generator step taken, fake step taken)."""
        gen_turn = self.step % self.gen_update_every == 0
        self.forward_backward(batch, cond, gen_turn)
        took_gen = False
        if gen_turn:
            took_gen = bool(self.mp_trainer.optimize(self.opt))
            if took_gen:
                self._update_emas()
        took_fake = bool(self.fake_trainer.optimize(self.fake_opt))
        self.step += 1
        self._anneal_lr()
        self.log_step()
        return took_gen, took_fake

    def forward_backward(self, batch, cond, gen_turn=True):
        """Both losses of every microbatch, accumulated before either optimize(): the generator's (with grad on its turn, else under
        no_grad) and, on the images it returned, the fake denoiser's DSM loss as TrainLoop.forward_backward forms it."""
        if gen_turn:
            self.mp_trainer.zero_grad()
        self.fake_trainer.zero_grad()
        with_real = self.gan_head is not None or self.objective == "sida"
        if with_real:
            x_real, real_cond = next(self.real_data)
            if x_real.shape[0] != batch.shape[0]:
                raise ValueError(f"DMTrainLoop: real_data yields batches of {x_real.shape[0]} images, the latents come in {batch.shape[0]}")
            real_cond = {k: v for k, v in (real_cond or {}).items() if k in cond}
        for i in range(0, batch.shape[0], self.microbatch):
            z = batch[i:i + self.microbatch].to(self.device)
            micro_cond = {k: v[i:i + self.microbatch].to(self.device) for k, v in cond.items()}
            if self.objective == "sid":
                gen_loss, how = self.diffusion.sid_generator_losses, dict(alpha=self.sid_alpha)
            elif self.objective == "sida":
                gen_loss, how = self.diffusion.sida_generator_losses, dict(alpha=self.sid_alpha, sida_gen_weight=self.sida_gen_weight)
            else:
                gen_loss, how = self.diffusion.dm_generator_losses, dict(weighting=self.weighting)
                if self.gan_head is not None:
                    how.update(gan_head=self.gan_head, gan_gen_weight=self.gan_gen_weight, gan_min_step_frac=self.gan_min_step_frac,
                               gan_max_step_frac=self.gan_max_step_frac)
            with torch.enable_grad() if gen_turn else torch.no_grad():
                terms = gen_loss(
                    self.ddp_model, z, self.num_scales, real_model=self.real_model, real_diffusion=self.real_diffusion,
                    fake_model=self.fake_model, fake_diffusion=self.fake_diffusion, model_kwargs=micro_cond, generator=self.generator,
                    gen_sigma=self.gen_sigma, gen_sigmas=self.gen_sigmas, min_step_frac=self.min_step_frac,
                    max_step_frac=self.max_step_frac, **how)
            if gen_turn:
                self.mp_trainer.backward(terms["loss"].mean())
            x = terms["x"]
            sigmas, weights = self.schedule_sampler.sample(x.shape[0], self.device)
            losses = self.fake_diffusion.training_losses(self.fake_model, x, sigmas, model_kwargs=micro_cond)
            logs = {"loss": terms["loss"], "dm_norm": terms["dm_norm"], "fake_mse": losses["mse"] * weights,
                    "fake_xs_mse": losses["xs_mse"] * weights}
            fake_loss = (losses["loss"] * weights).mean()
            if self.gan_head is not None:
                dis = self.fake_diffusion.gan_discriminator_losses(
                    self.fake_model, self.gan_head, x, x_real[i:i + self.microbatch].to(self.device), self.num_scales,
                    model_kwargs=micro_cond, real_kwargs={k: v[i:i + self.microbatch].to(self.device) for k, v in real_cond.items()},
                    generator=self.generator, gan_min_step_frac=self.gan_min_step_frac, gan_max_step_frac=self.gan_max_step_frac)
                fake_loss = fake_loss + self.gan_dis_weight * dis["loss"].mean()
                logs.update(gan_gen=terms["gan_loss"], gan_dis=dis["loss"], logit_fake=dis["logit_fake"], logit_real=dis["logit_real"])
            if self.objective == "sida":
                dis = self.fake_diffusion.sida_discriminator_losses(
                    self.fake_model, x, x_real[i:i + self.microbatch].to(self.device), self.num_scales, model_kwargs=micro_cond,
                    real_kwargs={k: v[i:i + self.microbatch].to(self.device) for k, v in real_cond.items()}, generator=self.generator)
                fake_loss = fake_loss + self.sida_dis_weight * dis["loss"].mean()
                logs.update(sida_gen=terms["adv_loss"], sida_dis=dis["loss"], logit_fake=dis["logit_fake"].mean(dim=1),
                            logit_real=dis["logit_real"].mean(dim=1))
            self._log_loss_dict(logs)
            self.fake_trainer.backward(fake_loss)

    def _anneal_lr(self):
        if not self.lr_anneal_steps:
            return
        frac = 1 - self.step / self.lr_anneal_steps
        for opt, lr in ((self.opt, self.lr), (self.fake_opt, self.fake_lr)):
            for param_group in opt.param_groups:
                param_group["lr"] = lr * frac

    def log_step(self):
        self._kv = {"step": self.step, "samples": (self.step + 1) * self.global_batch}
        self._kv.update({f"fake_{k}": v for k, v in self.fake_trainer.log.items()})

    def save(self):
        os.makedirs(self.log_dir, exist_ok=True)
        if _rank() == 0:
            torch.save({k: v.detach().clone() for k, v in self.fake_model.state_dict().items()},
                       os.path.join(self.log_dir, f"fake_model{self.step:06d}.pt"))
            torch.save(self.fake_opt.state_dict(), os.path.join(self.log_dir, f"fake_opt{self.step:06d}.pt"))
            if self.gan_head is not None:
                torch.save({k: v.detach().clone() for k, v in self.gan_head.state_dict().items()},
                           os.path.join(self.log_dir, f"gan_head{self.step:06d}.pt"))
        super().save()                  # ema, opt, then the model file last


class _UnitWeights:
    """schedule_sampler of CMTrainLoop when none is given: unit loss weights (consistency_losses draws the levels itself)."""

    def sample(self, batch_size, device):
        return None, torch.ones(batch_size, dtype=torch.float32, device=device)


def _alias_params_into_masters(param_groups_and_shapes, master_params):
    """Device fp32 parameters become views of their slices of the flat masters (as MixedPrecisionTrainer does for the model it
    trains): the EMA of the masters then IS the update of the network, with nothing to copy."""
    params = [p for group, _ in param_groups_and_shapes for _, p in group]
    if not all(p.is_cuda and p.dtype == torch.float32 for p in params):
        return
    for master, (group, _) in zip(master_params, param_groups_and_shapes):
        flat, off = master.detach().view(-1), 0
        for _, p in group:
            p.data = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
    torch.autograd.graph.increment_version(params)


def parse_resume_step_from_filename(filename):
    """Parse filenames of the form path/to/modelNNNNNN.pt, where NNNNNN is the checkpoint's number of steps."""
    split = os.path.basename(filename).split("model")
    if len(split) < 2:
        return 0
    split1 = split[-1].split(".")[0]
    try:
        return int(split1)
    except ValueError:
        return 0


def find_ema_checkpoint(main_checkpoint, step, rate):
    if main_checkpoint is None:
        return None
    path = os.path.join(os.path.dirname(main_checkpoint), f"ema_{rate}_{step:06d}.pt")
    return path if os.path.exists(path) else None
