"""Generate samples from an EDM-backbone DxMI sampler (ImageNet-64, LSUN-256) on MI355X; CLI-compatible with
the reference's generate_large.py:85-190 for the generation path.

    torchrun --nproc_per_node=N generate_large.py --log_dir results/imagenet64/T10/run --n_sample 50000 --batchsize 100

Reads `config.yaml` + `sampler.pth` from --log_dir, builds models.cm U-Net + OpenAIDiffusion, seeds every rank
with seed+rank (reference :103-114) and generates n_sample / batchsize / world batches per rank; --batchsize is
PER RANK, as in the reference.  Ranks never exchange data while sampling (the reference wraps the net in DDP
only to broadcast weights; here every rank loads the same checkpoint), so the only collective is the final
gather of uint8 images for the FID npz.  FID itself (pytorch_fid + Inception weights + dataset statistics) is
outside the accelerated path and runs only when those are present; --skip_fid writes PNGs as images are produced.
`--synthetic NAME` builds the net of a built-in config with random weights (benchmark / smoke use).

`--karras_sampler {heun,dpm,euler,ancestral,progdist}` samples the EDM teacher instead (progdist: a progressively distilled
student of it, `--pretrained` a model%06d.pt of `cm_train.py --training_mode progdist`, NFE = `--karras_steps`; `--karras_sampler dm`: a
one-step distribution-matching generator, `--pretrained` a model%06d.pt of `cm_train.py --training_mode dm`, NFE = 1,
`--gen_sigma` its input level (0 = sigma_max; the level it was trained at, 2.5 for score identity distillation as SiD runs it), or
`--gen_sigmas 80,5,1,0.3` the ladder of a K-step generator (the one given to `cm_train.py --gen_sigmas`; NFE = K; with `--generator
determ` / `determ-indiv` the noise between the steps is indexed per image, so samples_N.npz is the same whatever the batch size), and
`--karras_steps`, `--rho` and the churn and solver flags are refused with it) (models.cm.karras_diffusion.karras_sample,
reference models/cm/karras_diffusion.py:354-420): `--karras_steps` (40), `--rho`, `--s_churn`, `--s_tmin`, `--s_tmax`,
`--s_noise`.  Weights: `--pretrained [PATH]` loads a plain U-Net state dict (PATH, or the config's training.pretrained_path),
otherwise `sampler.pth` from --log_dir without its `log_betas` entry.  Class-conditional nets draw one label per image.

`--karras_sampler {dpmpp,sde-dpmpp}` samples the EDM teacher with multistep DPM-Solver++ (models.cm.dpm_sample.edm_dpm_sample; the
ODE solver and its SDE variant): NFE = `--karras_steps` (default 10), `--solver_order` (2; 3 with dpmpp only), `--solver_type
midpoint|exact`, `--skip_type karras|logsnr` (`--rho` with the karras ladder only), `--no_lower_order_final`; `--pretrained`,
`--generator`, `--seed` and `--no_graph` as above.  The churn flags do not apply.

`--cm_sampler {onestep,multistep}` samples a consistency-distilled model the same way (karras_sample's onestep /
multistep branch, reference :644-683): the diffusion is built with distillation=True; `--ts 0,22,39` (required for
multistep), `--cm_steps` (40); `--pretrained [PATH]` as above.  It excludes --karras_sampler and --guidance_scale.

`--generator {dummy,determ,determ-indiv}` (with --karras_sampler / --cm_sampler; reference models/cm/random_util.py): `dummy`, the
default, draws on the device as before.  `determ` / `determ-indiv` make image i of the run see the same noise and label whatever
--batchsize and the number of ranks are (models.cm.random_util): image i is row k of batch b on rank r with
i = b * batchsize * world + r + k * world, and samples_N.npz is written in that order.  `--seed` is the generator's seed (default:
the config's training.seed).

`--sampler_generator {dummy,determ,determ-indiv}` is the same choice for the DxMI sampler's own path (--guidance_scale included;
refused with --karras_sampler / --cm_sampler, which have --generator): labels and noise of image i then do not depend on --batchsize
or the number of ranks, every transition makes its draw inside its launch (dxmi_edm_step_fwd_indexed), `--seed` is accepted with it
and samples_N.npz is written in global-index order.
"""
import argparse
import math
import os
import random
import time

import numpy as np
import torch
from dxmi_hip import dist as _dist

import dxmi_config
from models.cm.script_util import create_model_and_diffusion
from models.DxMI.openai_diffusion import OpenAIDiffusion
from utils import mkdir_p, print0, to_uint8_nhwc, write_png_batch


KARRAS_FLAGS = ("karras_steps", "rho", "s_churn", "s_tmin", "s_tmax", "s_noise", "pretrained")
CM_FLAGS = ("ts", "cm_steps")
DPM_SAMPLERS = {"dpmpp": "dpmsolver++", "sde-dpmpp": "sde-dpmsolver++"}
DPM_FLAGS = ("solver_order", "solver_type", "skip_type", "no_lower_order_final")
CHURN_FLAGS = ("s_churn", "s_tmin", "s_tmax", "s_noise")


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log_dir", type=str, required=True, help="path to logdir")
    ap.add_argument("--n_sample", type=int, required=True)
    ap.add_argument("--batchsize", type=int, default=100)
    ap.add_argument("--guidance_scale", type=float, default=None)
    ap.add_argument("--skip_fid", action="store_true")
    ap.add_argument("--fid_extractor", type=str, default=None,
                    help="'module:attribute' of the feature extractor (the reference builds pytorch_fid's InceptionV3, whose "
                         "weights this image cannot download): callable(batch in [0,1]) -> [features [B, dims, h, w]]")
    ap.add_argument("--fid_stats", type=str, default=None, help="npz with the dataset's `mu` / `sigma` (reference: datasets/VIRTUAL_*.npz)")
    ap.add_argument("--fid_dims", type=int, default=2048)
    ap.add_argument("--synthetic", type=str, default=None, help="builtin config name, e.g. imagenet64_T10 (random weights)")
    ap.add_argument("--no_graph", action="store_true", help="issue every launch from python instead of replaying the T-step loop of a "
                                                           "batch as one hipGraph (dxmi_hip/graph.py; DXMI_GRAPH=0 does the same)")
    ap.add_argument("--karras_sampler", type=str, default=None, choices=("heun", "dpm", "euler", "ancestral", "progdist", "dpmpp", "sde-dpmpp", "dm"),
                    help="sample the EDM teacher with this Karras sampler, or with DPM-Solver++ (dpmpp: the ODE solver, sde-dpmpp: "
                         "its SDE variant), or a one-step distribution-matching generator distilled from it (dm), instead of the "
                         "DxMI sampler")
    ap.add_argument("--karras_steps", type=int, default=None, help="Karras sampler steps (default 40; dpmpp / sde-dpmpp: the number "
                                                                   "of network evaluations, default 10)")
    ap.add_argument("--solver_order", type=int, default=None, choices=(1, 2, 3), help="dpmpp / sde-dpmpp: the solver's order (default 2; "
                                                                                      "3 with dpmpp only)")
    ap.add_argument("--solver_type", type=str, default=None, choices=("midpoint", "exact"), help="dpmpp / sde-dpmpp: the second-order rows "
                                                                                                "(default midpoint)")
    ap.add_argument("--skip_type", type=str, default=None, choices=("karras", "logsnr"), help="dpmpp / sde-dpmpp: the sigma ladder "
                                                                                             "(default karras)")
    ap.add_argument("--no_lower_order_final", action="store_const", const=True, default=None,
                    help="dpmpp / sde-dpmpp: keep the full order on the last rows")
    ap.add_argument("--rho", type=float, default=None, help="Karras schedule rho (default 7.0)")
    ap.add_argument("--gen_sigma", type=float, default=None, help="--karras_sampler dm: the generator's input level, the one it was "
                                                                  "trained at (cm_train.py --gen_sigma; default 0 = sigma_max)")
    ap.add_argument("--gen_sigmas", type=str, default=None, help="--karras_sampler dm: the ladder of a K-step generator, largest level "
                                                                 "first, e.g. 80,5,1,0.3 (cm_train.py --gen_sigmas); not with --gen_sigma")
    ap.add_argument("--s_churn", type=float, default=None, help="Karras churn (default 0)")
    ap.add_argument("--s_tmin", type=float, default=None, help="churn window lower end (default 0)")
    ap.add_argument("--s_tmax", type=float, default=None, help="churn window upper end (default inf)")
    ap.add_argument("--s_noise", type=float, default=None, help="churn noise scale (default 1)")
    ap.add_argument("--pretrained", type=str, nargs="?", const="", default=None,
                    help="with --karras_sampler: load a plain U-Net state dict from PATH, or from the config's "
                         "training.pretrained_path when PATH is omitted")
    ap.add_argument("--cm_sampler", type=str, default=None, choices=("onestep", "multistep"),
                    help="sample a consistency-distilled model (distillation=True) with this sampler")
    ap.add_argument("--ts", type=str, default=None, help="multistep: comma-separated step indices, e.g. 0,22,39")
    ap.add_argument("--cm_steps", type=int, default=None, help="consistency sampler steps: the ts index range (default 40)")
    ap.add_argument("--generator", type=str, default="dummy", choices=("dummy", "determ", "determ-indiv"),
                    help="with --karras_sampler / --cm_sampler: determ / determ-indiv give image i of the run the same noise "
                         "whatever the batch size and the number of ranks (models/cm/random_util.py)")
    ap.add_argument("--sampler_generator", type=str, default="dummy", choices=("dummy", "determ", "determ-indiv"),
                    help="the DxMI sampler's draws (without --karras_sampler / --cm_sampler): determ / determ-indiv give image i of "
                         "the run the same labels and noise whatever the batch size and the number of ranks")
    ap.add_argument("--seed", type=int, default=None, help="seed of --generator / --sampler_generator determ / determ-indiv (default: the "
                                                           "config's training.seed)")
    return ap


def parse_args(argv=None):
    """-> (args, unknown); checks the Karras flags: they need --karras_sampler, which excludes --guidance_scale; and the
    consistency flags: they need --cm_sampler, which excludes --karras_sampler and --guidance_scale."""
    ap = build_parser()
    args, unknown = ap.parse_known_args(argv)
    if args.generator == "dummy" and args.sampler_generator == "dummy" and args.seed is not None:
        ap.error("--seed only applies with --generator / --sampler_generator determ / determ-indiv")
    if args.sampler_generator != "dummy" and (args.cm_sampler is not None or args.karras_sampler is not None):
        ap.error("--sampler_generator is the DxMI sampler's: with --karras_sampler / --cm_sampler use --generator")
    if args.generator != "dummy" and args.cm_sampler is None and args.karras_sampler is None:
        ap.error("--generator determ / determ-indiv only applies with --karras_sampler or --cm_sampler")
    if args.karras_sampler not in DPM_SAMPLERS:
        given = [f"--{k}" for k in DPM_FLAGS if getattr(args, k) is not None]
        if given:
            ap.error(f"{', '.join(given)} only apply with --karras_sampler dpmpp / sde-dpmpp")
    if args.gen_sigma is not None and args.karras_sampler != "dm":
        ap.error("--gen_sigma only applies with --karras_sampler dm")
    if args.gen_sigmas is not None and args.karras_sampler != "dm":
        ap.error("--gen_sigmas only applies with --karras_sampler dm")
    if args.cm_sampler is not None:
        return parse_cm_args(ap, args), unknown
    given = [f"--{k}" for k in CM_FLAGS if getattr(args, k) is not None]
    if given:
        ap.error(f"{', '.join(given)} only apply with --cm_sampler")
    if args.karras_sampler is None:
        given = [f"--{k}" for k in KARRAS_FLAGS if getattr(args, k) is not None]
        if given:
            ap.error(f"{', '.join(given)} only apply with --karras_sampler")
    else:
        if args.guidance_scale is not None:
            ap.error("--karras_sampler samples the EDM teacher: it cannot be combined with --guidance_scale")
        if args.karras_sampler in DPM_SAMPLERS:
            return parse_dpm_args(ap, args), unknown
        if args.karras_sampler == "dm":       # one evaluation at sigma_max: no ladder, no churn, no solver
            given = [f"--{k}" for k in ("karras_steps", "rho") + CHURN_FLAGS if getattr(args, k) is not None]
            if given:
                ap.error(f"{', '.join(given)}: --karras_sampler dm is one network evaluation at sigma_max, it has no steps, ladder or churn")
            if args.gen_sigmas is not None:
                if args.gen_sigma is not None:
                    ap.error("--gen_sigmas (the ladder of a K-step generator) does not go with --gen_sigma (the one-step level)")
                from cm_train import parse_gen_sigmas
                try:
                    args.gen_sigmas = parse_gen_sigmas(args.gen_sigmas)
                except ValueError as e:
                    ap.error(f"--gen_sigmas {args.gen_sigmas}: {e}")
            args.gen_sigma = 0.0 if args.gen_sigma is None else args.gen_sigma
            if not (math.isfinite(args.gen_sigma) and args.gen_sigma >= 0):
                ap.error(f"--gen_sigma {args.gen_sigma}: a positive level, or 0 for sigma_max")
            return args, unknown
        for k, v in (("karras_steps", 40), ("rho", 7.0), ("s_churn", 0.0), ("s_tmin", 0.0), ("s_tmax", float("inf")),
                     ("s_noise", 1.0)):
            if getattr(args, k) is None:
                setattr(args, k, v)
        if args.karras_steps < 1:
            ap.error("--karras_steps must be >= 1")
    return args, unknown


def parse_dpm_args(ap, args):
    """--karras_sampler dpmpp / sde-dpmpp: the defaults of the solver's flags and what they exclude."""
    given = [f"--{k}" for k in CHURN_FLAGS if getattr(args, k) is not None]
    if given:
        ap.error(f"{', '.join(given)}: --karras_sampler {args.karras_sampler} has no churn")
    for k, v in (("karras_steps", 10), ("solver_order", 2), ("solver_type", "midpoint"), ("skip_type", "karras")):
        if getattr(args, k) is None:
            setattr(args, k, v)
    args.no_lower_order_final = bool(args.no_lower_order_final)
    if args.karras_steps < 2:
        ap.error(f"--karras_steps must be >= 2 with --karras_sampler {args.karras_sampler}")
    if args.karras_sampler == "sde-dpmpp" and args.solver_order == 3:
        ap.error("--karras_sampler sde-dpmpp is defined for --solver_order 1 and 2")
    if args.rho is not None and args.skip_type == "logsnr":
        ap.error("--rho shapes the karras ladder: it does not apply with --skip_type logsnr")
    if args.rho is None:
        args.rho = 7.0
    return args


def parse_cm_args(ap, args):
    if args.karras_sampler is not None:
        ap.error("--cm_sampler and --karras_sampler exclude each other")
    if args.guidance_scale is not None:
        ap.error("--cm_sampler samples a consistency-distilled model: it cannot be combined with --guidance_scale")
    given = [f"--{k}" for k in KARRAS_FLAGS if k != "pretrained" and getattr(args, k) is not None]
    if given:
        ap.error(f"{', '.join(given)} only apply with --karras_sampler")
    if args.cm_steps is None:
        args.cm_steps = 40
    if args.cm_steps < 2:
        ap.error("--cm_steps must be >= 2")
    if args.cm_sampler == "onestep":
        if args.ts is not None:
            ap.error("--ts applies to --cm_sampler multistep only")
        return args
    if args.ts is None:
        ap.error("--cm_sampler multistep needs --ts, e.g. --ts 0,22,39")
    try:
        ts = tuple(int(v) for v in args.ts.split(","))
    except ValueError:
        ap.error(f"--ts {args.ts!r}: comma-separated integers expected")
    if len(ts) < 2 or any(not 0 <= v <= args.cm_steps - 1 for v in ts):
        ap.error(f"--ts needs at least two indices in [0, --cm_steps - 1] = [0, {args.cm_steps - 1}]")
    args.ts = ts
    return args


def resolve_weights(args, cfg):
    """Weights of the Karras path: -> (path, kind) with kind 'plain' (a U-Net state dict) or 'sampler' (sampler.pth), or
    (None, None) for --synthetic without --pretrained."""
    if args.pretrained is not None:
        path = args.pretrained or cfg.training.get("pretrained_path")
        if not path:
            raise ValueError("--pretrained without PATH needs training.pretrained_path in the config")
        return path, "plain"
    if args.synthetic:
        return None, None
    return os.path.join(args.log_dir, "sampler.pth"), "sampler"


def main():
    args, unknown = parse_args()

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    device = _dist.rank_device(local_rank)
    torch.cuda.set_device(device)
    if args.synthetic:
        import configs_builtin
        cfg = configs_builtin.get(args.synthetic)
    else:
        cfg = dxmi_config.load(os.path.join(args.log_dir, "config.yaml"))
    seed = cfg.training.seed
    torch.manual_seed(seed + local_rank)
    np.random.seed(seed + local_rank)
    torch.cuda.manual_seed_all(seed + local_rank)
    random.seed(seed + local_rank)

    unet, diffusion = create_model_and_diffusion(**cfg.diffusion)
    output_path = os.path.join(args.log_dir, "generated")
    mkdir_p(output_path)
    if args.karras_sampler is not None or args.cm_sampler is not None:
        return main_karras(args, cfg, unet, diffusion, device, local_rank, world, output_path)
    sampler = OpenAIDiffusion(unet, diffusion, **cfg.sampler)
    if not args.synthetic:
        ckpt_path = os.path.join(args.log_dir, "sampler.pth")
        ckpt = torch.load(ckpt_path, map_location="cpu")
        print0(f"checkpoint loaded from {ckpt_path} (FID {ckpt.get('fid')}, iter {ckpt.get('i_iter')})")
        sampler.net.load_state_dict(ckpt["state_dict"])
    sampler.net.to(device)
    if cfg.diffusion.use_fp16:
        unet.convert_to_fp16()
    sampler.eval()

    trainer = None
    if args.guidance_scale is not None:   # reference :132-148: value.pth + the trainer as the sampling driver
        v = dxmi_config.instantiate(cfg.value).to(device)
        if not args.synthetic:
            value_path = os.path.join(args.log_dir, "value.pth")
            if not os.path.exists(value_path):
                raise ValueError(f"Value ftn not found at {value_path}")
            v.load_state_dict(torch.load(value_path, map_location=device)["state_dict"])
        v.eval()
        trainer = dxmi_config.instantiate(cfg.trainer, batchsize=args.batchsize)
        trainer.set_models(v=v, sampler=sampler, optimizer=None, optimizer_v=None)

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend=_dist.dist_backend(), init_method="env://")  # RCCL

    from dxmi_hip import graph as hip_graph
    sampler.use_graph = hip_graph.default_enabled() and not args.no_graph        # second batch onwards: one hipGraphLaunch per batch
    n_batches = int(args.n_sample / args.batchsize / world)
    generator = None                            # dummy: every draw on the device with torch
    if args.sampler_generator != "dummy":       # after the process group is up: the generator reads its rank and world size
        from models.cm.random_util import get_generator
        generator = get_generator(args.sampler_generator, n_batches * args.batchsize * world,
                                  cfg.training.seed if args.seed is None else args.seed)
    l_sample, i_img = [], 0
    from dxmi_hip import ops
    from utils import ImageWriter
    writer = ImageWriter()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i_batch in range(n_batches):
        if generator is not None:               # the images all ranks have finished; the batch's draws count from 0 again
            generator.set_done_samples(i_batch * args.batchsize * world)
        if trainer is not None:
            d_sample = trainer.sample_guidance(n_sample=args.batchsize, device=device, guidance_scale=args.guidance_scale,
                                               generator=generator)
        else:
            d_sample = sampler.sample(args.batchsize, device=device, i_class=None, enable_grad=False, generator=generator)
        sample = d_sample["sample"]
        if args.skip_fid:
            # ((sample + 1) / 2).clamp(0, 1) -> save_image (:36-41) on the device, pinned copy on a side stream, PNG thread pool
            writer.submit(sample, [os.path.join(output_path, f"{local_rank}_{i_img + k}.png") for k in range(len(sample))])
            i_img += len(sample)
        else:
            l_sample.append(ops.quantize_u8(sample.contiguous().float(), mode=1, nhwc=False))      # ((x + 1) * 127.5).clamp.to(uint8), :43
    writer.close()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print0(f"generated {n_batches * args.batchsize} images/rank x {world} ranks, "
           f"{n_batches * args.batchsize / max(dt, 1e-9):.1f} images/s/rank")
    if args.skip_fid:
        return
    finish(args, l_sample, device, local_rank, world)


def index_order(gathered, batchsize):
    """The ranks' samples (each [n_batches * batchsize, ...], batch after batch) in the order of the deterministic generators'
    global index b * batchsize * world + r + k * world: batch, then row, then rank."""
    s = torch.stack(gathered)
    world, tail = s.shape[0], tuple(s.shape[2:])
    s = s.reshape((world, -1, batchsize) + tail)
    return s.permute(1, 2, 0, *range(3, s.dim())).reshape((-1,) + tail)


def finish(args, l_sample, device, local_rank, world):
    """All-gather of the uint8 batches, samples_N.npz on rank 0 and FID."""
    samples = torch.cat(l_sample)
    if world > 1:
        gathered = [torch.zeros_like(samples) for _ in range(world)]
        torch.distributed.all_gather(gathered, samples)
        indexed = args.generator != "dummy" or args.sampler_generator != "dummy"
        samples = index_order(gathered, args.batchsize) if indexed else torch.cat(gathered)
    if local_rank == 0:
        np.savez(os.path.join(args.log_dir, f"samples_{len(samples)}.npz"), samples.permute(0, 2, 3, 1).cpu().numpy())
    if args.fid_extractor is None or args.fid_stats is None:
        print0("samples saved as npz; FID needs --fid_extractor module:attr (an InceptionV3 pool3 extractor: its weights are not in "
               "this image) and --fid_stats <dataset statistics npz>")
        return
    # reference fid() (:57-74): this rank's strided share of ALL samples -> activations -> all_gather -> statistics -> distance;
    # the statistics (np.mean / np.cov on the host in the reference) run on the device
    from pytorch_fid.fid_score import fid_from_images, load_extractor, load_statistics
    extractor = load_extractor(args.fid_extractor)
    if hasattr(extractor, "to"):
        extractor = extractor.to(device)
    m2, s2 = load_statistics(args.fid_stats)
    fid = fid_from_images(samples[local_rank::world], extractor, m2, s2, batch_size=50, dims=args.fid_dims, device=device)
    print0(f"FID from {len(samples)} samples: {fid}")


def main_karras(args, cfg, unet, diffusion, device, local_rank, world, output_path):
    """--karras_sampler: the EDM teacher, no OpenAIDiffusion wrapper; the output stage is the DxMI path's.  --cm_sampler: a
    consistency-distilled model through the same path, with distillation=True."""
    from dxmi_hip import graph as hip_graph
    from dxmi_hip import ops
    from models.cm.dpm_sample import edm_dpm_sample
    from models.cm.karras_diffusion import cm_nfe, dm_sample, karras_nfe, karras_sample, progdist_sample
    from utils import ImageWriter
    path, kind = resolve_weights(args, cfg)
    if path is not None:
        sd = torch.load(path, map_location="cpu")
        if kind == "sampler":
            sd = {k: v for k, v in sd["state_dict"].items() if k != "log_betas"}
        unet.load_state_dict(sd)
        print0(f"EDM weights loaded from {path}")
    unet.to(device)
    if cfg.diffusion.use_fp16:
        unet.convert_to_fp16()
    unet.eval()
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend=_dist.dist_backend(), init_method="env://")  # RCCL
    shape = (args.batchsize,) + tuple(cfg.sampler.sample_shape)
    use_graph = hip_graph.default_enabled() and not args.no_graph
    if args.cm_sampler is not None:
        diffusion.distillation = True          # boundary-condition scalings (the diffusion block's distillation: True)
        sampler, steps, nfe = args.cm_sampler, args.cm_steps, cm_nfe(args.cm_sampler, args.ts)
        extra = dict(ts=args.ts)
    elif args.karras_sampler in DPM_SAMPLERS:      # one evaluation per step
        sampler, steps, nfe = args.karras_sampler, args.karras_steps, args.karras_steps
        extra = dict(algorithm=DPM_SAMPLERS[sampler], order=args.solver_order, solver_type=args.solver_type, skip_type=args.skip_type,
                     lower_order_final=not args.no_lower_order_final, rho=args.rho)
    elif args.karras_sampler == "dm":              # a distribution-matching generator: one evaluation at sigma_max
        sampler, steps, nfe, extra = "dm", len(args.gen_sigmas or (0,)), len(args.gen_sigmas or (0,)), {}
    else:
        sampler, steps, nfe = args.karras_sampler, args.karras_steps, karras_nfe(args.karras_sampler, args.karras_steps)
        extra = dict(rho=args.rho, s_churn=args.s_churn, s_tmin=args.s_tmin, s_tmax=args.s_tmax, s_noise=args.s_noise)
    n_batches = int(args.n_sample / args.batchsize / world)
    generator = None                            # dummy: every draw on the device, hipGraph replay allowed
    if args.generator != "dummy":
        from models.cm.random_util import get_generator
        generator = get_generator(args.generator, n_batches * args.batchsize * world,
                                  cfg.training.seed if args.seed is None else args.seed)
    l_sample, i_img = [], 0
    writer = ImageWriter()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i_batch in range(n_batches):
        kw = {}
        if generator is not None:               # the images all ranks have finished; the batch's draws count from 0 again
            generator.set_done_samples(i_batch * args.batchsize * world)
        if unet.num_classes is not None:        # one uniform label per image, as OpenAIDiffusion._sample draws them
            kw["y"] = (torch.randint(0, unet.num_classes, (args.batchsize,), device=device) if generator is None else
                       generator.randint(0, unet.num_classes, (args.batchsize,), device=device))
        if sampler in DPM_SAMPLERS:
            sample = edm_dpm_sample(diffusion, unet, shape, steps, model_kwargs=kw, device=device, sigma_min=diffusion.sigma_min,
                                    sigma_max=diffusion.sigma_max, use_graph=use_graph, generator=generator, **extra)
        elif sampler == "dm":
            sample = dm_sample(diffusion, unet, shape, gen_sigma=None if args.gen_sigmas else (args.gen_sigma or None), model_kwargs=kw,
                               device=device, generator=generator, gen_sigmas=args.gen_sigmas)
        elif sampler == "progdist":             # its own entry point: karras_sample keeps refusing this sampler
            sample = progdist_sample(diffusion, unet, shape, steps, model_kwargs=kw, device=device, sigma_min=diffusion.sigma_min,
                                     sigma_max=diffusion.sigma_max, rho=args.rho, use_graph=use_graph, generator=generator)
        else:
            sample = karras_sample(diffusion, unet, shape, steps, model_kwargs=kw, device=device, sigma_min=diffusion.sigma_min,
                                   sigma_max=diffusion.sigma_max, sampler=sampler, use_graph=use_graph, generator=generator, **extra)
        if args.skip_fid:
            writer.submit(sample, [os.path.join(output_path, f"{local_rank}_{i_img + k}.png") for k in range(len(sample))])
            i_img += len(sample)
        else:
            l_sample.append(ops.quantize_u8(sample, mode=1, nhwc=False))
    writer.close()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print0(f"generated {n_batches * args.batchsize} images/rank x {world} ranks, "
           f"{n_batches * args.batchsize / max(dt, 1e-9):.1f} images/s/rank, {nfe} NFE/image "
           f"({sampler}, {steps} steps{', order ' + str(args.solver_order) + ', ' + args.skip_type if sampler in DPM_SAMPLERS else ''}"
           f"{'' if args.cm_sampler is None or args.ts is None else ', ts ' + str(list(args.ts))})")
    if not args.skip_fid:
        finish(args, l_sample, device, local_rank, world)


if __name__ == "__main__":
    main()
