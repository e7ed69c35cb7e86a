"""Train a consistency model on the HIP U-Net: distillation from an EDM teacher, consistency training without one, or progressive
distillation of the teacher
(models.cm.train_util.CMTrainLoop over KarrasDenoiser.consistency_losses; reference: the consistency_models training entry point
over models/cm/script_util.py cm_train_defaults + model_and_diffusion_defaults).

    torchrun --nproc_per_node=8 cm_train.py --training_mode consistency_distillation --teacher_model_path edm_imagenet64.pt \\
        --synthetic_data True --batch_size 16 --log_dir results/cd
    python cm_train.py --training_mode consistency_training --synthetic_data True --max_iters 2

Every key of cm_train_defaults() and model_and_diffusion_defaults() is a flag, next to --synthetic_data, --batch_size, --microbatch,
--lr, --ema_rate, --log_dir, --max_iters, --use_fp16 and the loop's intervals.  For distillation the student and the target start
from the teacher's weights, the teacher's diffusion has distillation=False and the student's distillation=True.  The target_model
checkpoints it writes are what `generate_large.py --cm_sampler onestep --pretrained ...` reads.  Image folders are not read by
this package: --data_npz PATH trains on a uint8 image array file (dxmi_hip/data.py ImageStore, normalised as the reference's
image_datasets.py does; --data_resident auto|device|host), --synthetic_data True draws uniform images and labels; the two exclude
each other and one of them is required.  --training_mode progdist is progressive distillation (KarrasDenoiser.progdist_losses):
the student keeps distillation=False and starts from the teacher (--teacher_model_path), there is no target network, the schedule is
the reference's ("fixed", "progdist") pair (--start_scales halved every --distill_steps_per_iter steps; --scale_mode is set to progdist
unless given otherwise), a phase anneals the learning rate over --lr_anneal_steps (default: --distill_steps_per_iter) steps, and
--max_iters only bounds total_training_steps; its model%06d.pt is what `generate_large.py --karras_sampler progdist --pretrained ...`
reads.  CMTrainLoop.run_loop keeps the reference's condition, which
ends only when both lr_anneal_steps and total_training_steps are reached: --max_iters N (smoke runs) sets both to N, so the
learning rate anneals to zero over those N steps.  --loss_norm lpips needs the VGG16 and LPIPS linear weight files:
--lpips_vgg16 PATH --lpips_lin PATH, or DXMI_LPIPS_VGG16 / DXMI_LPIPS_LIN in the environment; without them it is refused.
--use_graph True replays the train step from hipGraphs (CMTrainLoop(use_graph=True): needs --use_fp16 True and a loss norm other than
lpips); DXMI_GRAPH=0 in the environment forces it off.
Improved consistency training (Song and Dhariwal 2023) needs neither LPIPS weights nor a teacher: --loss_norm pseudo-huber (--huber_c C,
0 = 0.00054 sqrt(C H W)), --weight_schedule ict (1 / (t - t2); with pseudo-huber only), --index_sampler lognormal (--p_mean, --p_std: the
discretised lognormal over the levels; uniform = the reference's randint), --scale_mode ict (num_scales doubles from --start_scales to
--end_scales over --total_training_steps) and --start_ema 0 (the target is the student of the step before).  --ict True sets all of these
at once (loss_norm, weight_schedule, scale_mode, target_ema_mode fixed, start_ema 0, start_scales 10, end_scales 1280, index_sampler
lognormal) and takes --training_mode consistency_training, which it also selects where no --training_mode is given; any other is an error.
--training_mode dm is distribution matching distillation of the teacher into a ONE-step generator (models.cm.train_util.DMTrainLoop over
KarrasDenoiser.dm_generator_losses; Diff-Instruct / DMD / DMD2, its GAN term with --dm_gan): generator and fake denoiser start from
--teacher_model_path, the data are latents and uniform labels from a device generator seeded seed + rank, so neither --data_npz (refused)
nor --synthetic_data is needed; --gen_update_every (5), --fake_lr (0 = --lr), --dm_weighting dmd|none, --dm_num_scales (1000).  The sigma
levels of the fake denoiser's loss are EDM's (LogNormalSampler's defaults, as train_edm.py draws them).  --ict, a --loss_norm other than the default and
--index_sampler lognormal are errors with it.  Its model%06d.pt is what `generate_large.py --karras_sampler dm --pretrained ...` reads.
--dm_objective sid trains the same generator by score identity distillation instead (KarrasDenoiser.sid_generator_losses; SiD, Zhou et
al. 2024: the loss is differentiated through both denoisers' inputs): --sid_alpha (1.2), and --gen_sigma, the generator's input level
(0 = sigma_max; SiD's runs use 2.5, and generate_large.py must then be given the same --gen_sigma).  --gen_sigmas 80,5,1,0.3 trains a
K-step generator on that ladder by backward simulation instead (DMD2 section 4.4-4.5; not with --gen_sigma or --dm_objective sid;
generate_large.py takes the same --gen_sigmas).  --dm_weighting none does not go
with it, and these flags are errors outside --training_mode dm.
--dm_gan True adds DMD2's GAN term (models.cm.gan_head.GANHead on the fake denoiser's bottleneck, sized from the net: its bottleneck
channels and image_size / 2^(levels - 1); KarrasDenoiser.gan_discriminator_losses on the fake clock, the generator's loss gains
--gan_gen_weight softplus(-logit)): it needs real images, --data_npz PATH or --synthetic_data True, and does not go with --dm_objective
sid; --gan_gen_weight (3e-3), --gan_dis_weight (1e-2), --gan_max_step_frac (1.0: the noise levels of the GAN term's inputs reach up to that
fraction of the ladder).  The gan_* flags are errors without --dm_gan.
--dm_objective sida is adversarial score identity distillation (KarrasDenoiser.sida_generator_losses / sida_discriminator_losses; SiDA,
Zhou, Zheng et al. 2024): SiD plus a discriminator WITHOUT parameters, the channel mean of the fake denoiser's bottleneck, read from the
evaluation SiD already makes.  It needs real images (--data_npz PATH or --synthetic_data True) and takes --sid_alpha (1.2),
--sida_gen_weight (0.01), --sida_dis_weight (1.0) and --gen_sigma; --dm_gan True, --dm_weighting none and a ladder of more than one level
are errors with it, and the sida_* flags are errors without it.  No file is added to the checkpoints: the discriminator is the fake net.
"""
import argparse
import math
import os
import sys

import torch

from dxmi_hip import dist as _dist
from dxmi_hip import graph as _graph
from models.cm.script_util import (add_dict_to_argparser, args_to_dict, cm_train_defaults, create_ema_and_scales_fn,
                                   create_model_and_diffusion, model_and_diffusion_defaults)
from models.cm.train_util import CMTrainLoop, DMTrainLoop


def print0(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print(*a, flush=True)


def synthetic_batches(batch_size, image_size, class_cond, device, seed):
    gen = torch.Generator(device=device).manual_seed(seed)
    while True:
        x = torch.rand(batch_size, 3, image_size, image_size, device=device, generator=gen) * 2 - 1
        cond = {"y": torch.randint(0, 1000, (batch_size,), device=device, generator=gen)} if class_cond else {}
        yield x, cond


def latent_batches(batch_size, image_size, class_cond, device, seed, num_classes=1000):
    """The `data=` iterator of DMTrainLoop: standard-normal latents of the image shape and uniform labels, from a device generator."""
    gen = torch.Generator(device=device).manual_seed(seed)
    while True:
        z = torch.randn(batch_size, 3, image_size, image_size, device=device, generator=gen)
        cond = {"y": torch.randint(0, num_classes, (batch_size,), device=device, generator=gen)} if class_cond else {}
        yield z, cond


REAL_SEED_OFFSET = 1 << 20      # --dm_gan: the synthetic real images are drawn from another stream than the latents


def make_loader(args, device, rank, world, seed_offset=0):
    """The `data=` iterator of CMTrainLoop for the parsed flags, and the ImageStore behind it (None for synthetic data).
    seed_offset: added to the synthetic stream's seed (two device generators of one seed would draw correlated values)."""
    if args.data_npz:
        from dxmi_hip.data import NORM_ADM, ImageStore
        store = ImageStore(args.data_npz, device, NORM_ADM, batch_size=args.batch_size, rank=rank, world=world, seed=args.seed,
                           class_cond=args.class_cond, resident=args.data_resident)
        return store.batches(), store
    if not args.synthetic_data:
        raise NotImplementedError("cm_train.py: image folders are not read by this package; run with --data_npz PATH (an uint8 array "
                                  "file, see make_npz.py) or --synthetic_data True")
    return synthetic_batches(args.batch_size, args.image_size, args.class_cond, device, args.seed + rank + seed_offset), None


# what --ict True sets: improved consistency training as its paper runs it
ICT_SETTINGS = dict(training_mode="consistency_training", loss_norm="pseudo-huber", weight_schedule="ict", scale_mode="ict",
                    target_ema_mode="fixed", start_ema=0.0, start_scales=10, end_scales=1280, index_sampler="lognormal")


def parse_gen_sigmas(text):
    """"80,5,1,0.3" -> the checked ladder of a K-step generator, fp32 values as python floats (ValueError with the reason)."""
    from models.cm.karras_diffusion import gen_ladder
    try:
        vals = [float(v) for v in str(text).split(",")]
    except ValueError:
        raise ValueError("comma-separated levels, largest first, e.g. 80,5,1,0.3") from None
    return gen_ladder("--gen_sigmas", vals).sigmas


def parse_args(argv=None):
    defaults = dict(model_and_diffusion_defaults())
    defaults.update(cm_train_defaults())
    defaults.update(synthetic_data=False, data_npz="", data_resident="auto", batch_size=16, microbatch=-1, lr=1e-4, ema_rate="0.9999",
                    log_dir="results/cm_train",
                    max_iters=0, weight_decay=0.0, lr_anneal_steps=0, log_interval=10, save_interval=10000, resume_checkpoint="",
                    fp16_scale_growth=1e-3, seed=42, batch_invariant=False, lpips_vgg16="", lpips_lin="", use_graph=False,
                    huber_c=0.0, index_sampler="uniform", p_mean=-1.1, p_std=2.0, ict=False, gen_update_every=5, fake_lr=0.0,
                    dm_weighting="dmd", dm_num_scales=1000, dm_objective="dmd", sid_alpha=1.2, gen_sigma=0.0, gen_sigmas="", dm_gan=False,
                    gan_gen_weight=3e-3, gan_dis_weight=1e-2, gan_max_step_frac=1.0, sida_gen_weight=0.01, sida_dis_weight=1.0)
    ap = argparse.ArgumentParser()
    add_dict_to_argparser(ap, defaults)
    args = ap.parse_args(argv)
    words = sys.argv[1:] if argv is None else argv
    given = lambda flag: any(a == flag or a.startswith(flag + "=") for a in words)
    if args.synthetic_data and args.data_npz:
        ap.error("--synthetic_data and --data_npz exclude each other")
    if args.training_mode == "dm":
        if args.dm_gan and not (args.data_npz or args.synthetic_data):
            ap.error("--dm_gan True needs real images: --data_npz PATH or --synthetic_data True")
        if args.dm_gan and args.dm_objective == "sid":
            ap.error("--dm_gan True does not go with --dm_objective sid: a discriminator on score identity distillation is SiDA, a "
                     "different recipe")
        if args.dm_gan and not (math.isfinite(args.gan_gen_weight) and math.isfinite(args.gan_dis_weight)
                                and 0.0 <= args.gan_max_step_frac <= 1.0):
            ap.error("--gan_gen_weight and --gan_dis_weight must be finite and --gan_max_step_frac lie in [0, 1]")
        if args.dm_objective == "sida":
            if args.dm_gan:
                ap.error("--dm_gan True does not go with --dm_objective sida: SiDA's discriminator has no head, it is the channel mean "
                         "of the fake denoiser's bottleneck")
            if not (args.data_npz or args.synthetic_data):
                ap.error("--dm_objective sida needs real images: --data_npz PATH or --synthetic_data True")
            if not (math.isfinite(args.sida_gen_weight) and math.isfinite(args.sida_dis_weight)):
                ap.error("--sida_gen_weight and --sida_dis_weight must be finite")
        if args.data_npz and not (args.dm_gan or args.dm_objective == "sida"):
            ap.error("--data_npz does not go with --training_mode dm: distribution matching trains on latents alone, it reads no images")
        if args.ict:
            ap.error("--ict True is improved consistency TRAINING: --training_mode dm does not go with it")
        if args.loss_norm != cm_train_defaults()["loss_norm"]:
            ap.error(f"--loss_norm {args.loss_norm} belongs to the consistency and progdist losses, not to --training_mode dm")
        if args.index_sampler == "lognormal":
            ap.error("--index_sampler lognormal belongs to the consistency losses, not to --training_mode dm")
        if args.dm_weighting not in ("dmd", "none"):
            ap.error(f"--dm_weighting {args.dm_weighting!r}: dmd or none")
        if args.gen_update_every < 1 or args.dm_num_scales < 2 or args.fake_lr < 0:
            ap.error("--gen_update_every must be >= 1, --dm_num_scales >= 2 and --fake_lr >= 0 (0: --lr)")
        if args.use_graph:
            ap.error("--use_graph True does not go with --training_mode dm (two update clocks; DMTrainLoop refuses it)")
        if args.dm_objective not in ("dmd", "sid", "sida"):
            ap.error(f"--dm_objective {args.dm_objective!r}: dmd, sid or sida")
        if args.dm_objective in ("sid", "sida") and args.dm_weighting == "none":
            ap.error("--dm_weighting none belongs to --dm_objective dmd: score identity distillation has its normaliser in the loss")
        if not math.isfinite(args.sid_alpha):
            ap.error(f"--sid_alpha {args.sid_alpha}: a finite number (SiD: 1.2; 1 is its base form)")
        if not (math.isfinite(args.gen_sigma) and args.gen_sigma >= 0):
            ap.error(f"--gen_sigma {args.gen_sigma}: a positive level, or 0 for sigma_max")
        if args.gen_sigmas:
            if given("--gen_sigma"):
                ap.error("--gen_sigmas (the ladder of a K-step generator) does not go with --gen_sigma (the one-step level)")
            try:
                args.gen_sigmas = parse_gen_sigmas(args.gen_sigmas)
            except ValueError as e:
                ap.error(f"--gen_sigmas {args.gen_sigmas}: {e}")
            if args.dm_objective in ("sid", "sida") and len(args.gen_sigmas) > 1:
                ap.error(f"--gen_sigmas with more than one level does not go with --dm_objective {args.dm_objective}: backward simulation is built for "
                         "--dm_objective dmd alone")
        else:
            args.gen_sigmas = None
    else:
        for flag in ("--dm_objective", "--sid_alpha", "--gen_sigma", "--gen_sigmas", "--dm_gan"):
            if given(flag):
                ap.error(f"{flag} belongs to --training_mode dm, not to --training_mode {args.training_mode}")
    if not (args.training_mode == "dm" and args.dm_objective == "sida"):
        for flag in ("--sida_gen_weight", "--sida_dis_weight"):
            if given(flag):
                ap.error(f"{flag} belongs to --training_mode dm --dm_objective sida")
    if not args.dm_gan:
        for flag in ("--gan_gen_weight", "--gan_dis_weight", "--gan_max_step_frac"):
            if given(flag):
                ap.error(f"{flag} belongs to --dm_gan True")
    if args.ict:
        if given("--training_mode") and args.training_mode != "consistency_training":
            ap.error(f"--ict True is improved consistency TRAINING: --training_mode {args.training_mode} does not go with it")
        for k, v in ICT_SETTINGS.items():
            setattr(args, k, v)
    if args.index_sampler not in ("uniform", "lognormal"):
        ap.error(f"--index_sampler {args.index_sampler!r}: uniform or lognormal")
    if args.huber_c < 0:
        ap.error(f"--huber_c {args.huber_c}: a positive constant, or 0 for 0.00054 sqrt(C H W)")
    if args.weight_schedule == "ict" and args.loss_norm != "pseudo-huber":
        ap.error(f"--weight_schedule ict goes with --loss_norm pseudo-huber only, not {args.loss_norm}")
    if args.loss_norm == "pseudo-huber" and args.training_mode == "progdist":
        ap.error("--loss_norm pseudo-huber belongs to the consistency losses, not to progdist")
    if args.index_sampler == "lognormal" and args.training_mode == "progdist":
        ap.error("--index_sampler lognormal belongs to the consistency losses, not to progdist")
    if args.training_mode == "progdist" and args.scale_mode == "fixed":
        args.scale_mode = "progdist"       # the reference's pair for this mode: target_ema_mode fixed, scale_mode progdist
    if args.data_resident not in ("auto", "device", "host"):
        ap.error(f"--data_resident {args.data_resident!r}: auto, device or host")
    return args


def main():
    args = parse_args()
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    device = _dist.rank_device(local_rank)
    torch.cuda.set_device(device)
    if not args.batch_invariant:
        from dxmi_hip import ops as _ops
        _ops.tune_for_throughput()
    torch.manual_seed(args.seed + local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend=_dist.dist_backend(), init_method="env://")   # RCCL
    if args.training_mode == "dm":
        return main_dm(args, device, local_rank, world)
    data, store = make_loader(args, device, local_rank, world)
    if store is not None:
        print0(store.describe())
    progdist = args.training_mode == "progdist"
    distill = args.training_mode == "consistency_distillation" or progdist      # the modes with a teacher
    if args.training_mode not in ("consistency_distillation", "consistency_training", "progdist"):
        raise NotImplementedError(f"training_mode {args.training_mode!r}: consistency_distillation, consistency_training or progdist")

    model_kw = args_to_dict(args, model_and_diffusion_defaults().keys())
    model, diffusion = create_model_and_diffusion(distillation=not progdist, **model_kw)     # a progdist student keeps EDM scalings
    diffusion.loss_norm = args.loss_norm
    diffusion.huber_c = args.huber_c or None       # 0: the paper's constant for the image size of a call
    if args.loss_norm == "lpips":      # refused here, before the target and the teacher are built, when no weights were named
        from models.cm.karras_diffusion import _NO_LPIPS
        from models.cm.lpips import ENV_LIN, ENV_VGG16, LPIPS
        vgg, lin = args.lpips_vgg16 or os.environ.get(ENV_VGG16), args.lpips_lin or os.environ.get(ENV_LIN)      # a flag wins
        if not vgg or not lin:
            raise NotImplementedError(_NO_LPIPS)
        diffusion.lpips_loss = LPIPS.from_files(vgg, lin)
    target_model = None if progdist else create_model_and_diffusion(distillation=True, **model_kw)[0]
    teacher_model = teacher_diffusion = None
    if distill:
        teacher_model, teacher_diffusion = create_model_and_diffusion(distillation=False, **dict(model_kw, dropout=args.teacher_dropout))
        if args.teacher_model_path:
            teacher_model.load_state_dict(torch.load(args.teacher_model_path, map_location="cpu"))
            print0(f"teacher loaded from {args.teacher_model_path}")
        else:
            print0("no --teacher_model_path: the teacher keeps its random initialisation (smoke runs)")
        model.load_state_dict(teacher_model.state_dict())      # student and target start from the teacher
        teacher_model.to(device).eval()
    model.to(device).train()
    if target_model is not None:
        target_model.load_state_dict(model.state_dict())
        target_model.to(device).train()

    ema_scale_fn = create_ema_and_scales_fn(target_ema_mode=args.target_ema_mode, start_ema=args.start_ema, scale_mode=args.scale_mode,
                                            start_scales=args.start_scales, end_scales=args.end_scales,
                                            total_steps=args.total_training_steps, distill_steps_per_iter=args.distill_steps_per_iter)
    total = args.max_iters if args.max_iters else args.total_training_steps
    lr_anneal_steps = args.lr_anneal_steps if not args.max_iters else args.max_iters
    if progdist:       # the loop's phase arithmetic takes lr_anneal_steps for the length of a phase (doubled for num_scales 2 and 1)
        lr_anneal_steps = args.lr_anneal_steps or args.distill_steps_per_iter
    index_sampler = None
    if args.index_sampler == "lognormal":
        from models.cm.resample import DiscreteLogNormalSampler
        index_sampler = DiscreteLogNormalSampler(diffusion.sigma_min, diffusion.sigma_max, diffusion.rho, args.p_mean, args.p_std)
    loop = CMTrainLoop(model=model, target_model=target_model, teacher_model=teacher_model, teacher_diffusion=teacher_diffusion,
                       training_mode=args.training_mode, ema_scale_fn=ema_scale_fn, total_training_steps=total, diffusion=diffusion,
                       data=data,
                       batch_size=args.batch_size, microbatch=args.microbatch, lr=args.lr, ema_rate=args.ema_rate,
                       log_interval=args.log_interval, save_interval=args.save_interval, resume_checkpoint=args.resume_checkpoint,
                       use_fp16=args.use_fp16, fp16_scale_growth=args.fp16_scale_growth, weight_decay=args.weight_decay,
                       lr_anneal_steps=lr_anneal_steps, log_dir=args.log_dir, index_sampler=index_sampler,
                       use_graph=args.use_graph and _graph.default_enabled())
    print0(f"{args.training_mode}: {sum(p.numel() for p in model.parameters()) / 1e6:.1f} M parameters, {world} rank(s), "
           f"{total} steps, loss_norm {args.loss_norm}")
    loop.run_loop()
    if loop.logged:
        print0("last log row:", loop.logged[-1])
    if store is not None:
        store.close()
    if world > 1:
        torch.distributed.destroy_process_group()


def main_dm(args, device, local_rank, world):
    """--training_mode dm: generator and fake denoiser start from the teacher, which stays frozen as the real denoiser."""
    from models.cm.resample import LogNormalSampler
    model_kw = args_to_dict(args, model_and_diffusion_defaults().keys())
    model, diffusion = create_model_and_diffusion(distillation=False, **model_kw)
    fake_model = create_model_and_diffusion(distillation=False, **model_kw)[0]
    real_model, real_diffusion = create_model_and_diffusion(distillation=False, **dict(model_kw, dropout=args.teacher_dropout))
    if args.teacher_model_path:
        real_model.load_state_dict(torch.load(args.teacher_model_path, map_location="cpu"))
        print0(f"teacher loaded from {args.teacher_model_path}")
    else:
        print0("no --teacher_model_path: the teacher keeps its random initialisation (smoke runs)")
    model.load_state_dict(real_model.state_dict())
    fake_model.load_state_dict(real_model.state_dict())
    real_model.to(device).eval()
    model.to(device).train()
    fake_model.to(device).train()
    data = latent_batches(args.batch_size, args.image_size, args.class_cond, device, args.seed + local_rank)
    gan, store = {}, None
    if args.dm_gan:
        from models.cm.gan_head import GANHead
        levels = len(fake_model.channel_mult)
        head = GANHead(int(fake_model.channel_mult[-1] * fake_model.model_channels), args.image_size // 2 ** (levels - 1))
        real_data, store = make_loader(args, device, local_rank, world, seed_offset=REAL_SEED_OFFSET)
        if store is not None:
            print0(store.describe())
        gan = dict(gan_head=head.to(device), real_data=real_data, gan_gen_weight=args.gan_gen_weight, gan_dis_weight=args.gan_dis_weight,
                   gan_max_step_frac=args.gan_max_step_frac)
    if args.dm_objective == "sida":
        real_data, store = make_loader(args, device, local_rank, world, seed_offset=REAL_SEED_OFFSET)
        if store is not None:
            print0(store.describe())
        gan = dict(real_data=real_data, sida_gen_weight=args.sida_gen_weight, sida_dis_weight=args.sida_dis_weight)
    loop = DMTrainLoop(**gan, model=model, diffusion=diffusion, real_model=real_model, real_diffusion=real_diffusion, fake_model=fake_model,
                       num_scales=args.dm_num_scales, gen_update_every=args.gen_update_every, fake_lr=args.fake_lr or None,
                       weighting=args.dm_weighting, objective=args.dm_objective, sid_alpha=args.sid_alpha,
                       gen_sigma=args.gen_sigma or None, gen_sigmas=args.gen_sigmas, data=data, batch_size=args.batch_size, microbatch=args.microbatch, lr=args.lr,
                       ema_rate=args.ema_rate, log_interval=args.log_interval, save_interval=args.save_interval,
                       resume_checkpoint=args.resume_checkpoint, use_fp16=args.use_fp16, fp16_scale_growth=args.fp16_scale_growth,
                       schedule_sampler=LogNormalSampler(), weight_decay=args.weight_decay,
                       lr_anneal_steps=args.max_iters if args.max_iters else args.lr_anneal_steps, log_dir=args.log_dir)
    print0(f"dm: {sum(p.numel() for p in model.parameters()) / 1e6:.1f} M parameters, {world} rank(s), "
           + (f"objective sid (alpha {args.sid_alpha}), " if args.dm_objective == "sid"
              else f"objective sida (alpha {args.sid_alpha}, generator weight {args.sida_gen_weight}, discriminator weight "
                   f"{args.sida_dis_weight}), " if args.dm_objective == "sida" else f"weighting {args.dm_weighting}, ")
           + (f"gen_sigmas {args.gen_sigmas} (K = {len(args.gen_sigmas)}), " if args.gen_sigmas
              else f"gen_sigma {args.gen_sigma or diffusion.sigma_max}, ")
           + f"generator update every {args.gen_update_every} iterations"
           + (f", GAN term (generator weight {args.gan_gen_weight}, discriminator weight {args.gan_dis_weight})" if args.dm_gan else ""))
    loop.run_loop()
    if loop.logged:
        print0("last log row:", loop.logged[-1])
    if store is not None:
        store.close()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
