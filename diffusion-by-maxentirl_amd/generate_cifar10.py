"""Generate samples from a trained DxMI sampler on MI355X (CLI-compatible with the reference's
generate_cifar10.py:45-233 for the generation path).

    torchrun --nproc_per_node=N generate_cifar10.py --log_dir results/cifar10/T10/run -n 50000 --batchsize 100

Reads `config.yaml` + `sampler_{epoch}.pth` from --log_dir (as written by train_cifar10.py), shards the
images over ranks with seed+rank (reference :103-110, :193-204), runs the HIP sampler and writes
`{rank}_{i}.png` under <log_dir>/generated.  FID (pytorch_fid + Inception weights + the training PNGs)
is outside the accelerated path: it runs only when pytorch_fid and the dataset folder are present,
otherwise it is skipped with a message (`--skip_fid` forces that).  `--synthetic` builds the net from
the built-in config with random weights (benchmark / smoke use, no checkpoint needed).

    python generate_cifar10.py --log_dir out/ddim50 --config builtin:cifar10_T10 --teacher_ckpt .../ema_0.9999_800000.pt \\
        --ddpm_steps 50 --eta 0 -n 50000 --batchsize 500

`--teacher_ckpt PATH` samples the DDPM teacher itself (models/DxMI/ddpm_sample.py ddpm_sample: ancestral, DDIM and strided
schedules): PATH is a plain state dict of the bare network, train_ddpm.py's ema_*.pt / model*.pt.  With it: `--ddpm_steps S`
(1000), `--eta E` (1: ancestral, 0: DDIM), `--variance {small,large}`, `--skip_type {uniform,quad}`, `--no_clip`,
`--generator {dummy,determ,determ-indiv}` (the deterministic ones make a run's images independent of batch size and rank count;
`--seed` is their seed) and `--config builtin:NAME | PATH` for a --log_dir that holds no config.yaml.  The images go to
<log_dir>/generated and through the same FID flow.  It excludes --guidance_scale.

    python generate_cifar10.py --log_dir out/dpmpp10 --config builtin:cifar10_T10 --teacher_ckpt .../ema_0.9999_800000.pt \\
        --solver dpmpp --ddpm_steps 10 -n 50000 --batchsize 500

`--solver {ancestral,dpmpp,sde-dpmpp}` (with --teacher_ckpt; default ancestral, the path above) samples the teacher with multistep
DPM-Solver++ (models/DxMI/dpm_sample.py dpm_sample), the ODE solver or its SDE variant: `--ddpm_steps S` network evaluations (10),
`--solver_order {1,2,3}` (2; the SDE variant 1 or 2), `--solver_type {midpoint,exact}`, `--no_lower_order_final`, `--skip_type
{logsnr,uniform,quad}` (logsnr).  --eta and --variance belong to the ancestral path and are refused with these solvers.

`--sampler_generator {dummy,determ,determ-indiv}` is the DxMI sampler's own (--guidance_scale included; refused with --teacher_ckpt,
which has --generator): with determ / determ-indiv image i of the run sees the same noise whatever --batchsize and the number of
ranks are (models.cm.random_util with `--seed` as its seed), and the PNGs are named by that global index, `{i}.png` with
i = b * batchsize * world + rank + k * world for row k of batch b, so the folders of two runs compare file by file.
"""
import argparse
import os
import random
import time

import numpy as np
import torch
from dxmi_hip import dist as _dist

import cmd_utils as cmd  # noqa: F401  (kept for CLI parity: unknown --a.b overrides are parsed the same way)
import dxmi_config
from utils import mkdir_p, print0, to_uint8_nhwc, write_png_batch


def rescale(X):
    return (X - (-1)) / 2


def save_png(img_chw, path):
    """uint8 PNG of a [3,H,W] tensor in [0,1] (torchvision.utils.save_image rounding: x*255+0.5)."""
    write_png_batch(to_uint8_nhwc(img_chw[None]), [path], workers=1)


TEACHER_FLAGS = ("ddpm_steps", "eta", "variance", "skip_type", "generator", "config")
SOLVER_FLAGS = ("solver", "solver_order", "solver_type")         # DPM-Solver++; with --no_lower_order_final
SOLVERS = {"dpmpp": "dpmsolver++", "sde-dpmpp": "sde-dpmsolver++"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--log_dir", type=str, required=True)
    ap.add_argument("--batchsize", type=int, default=100)
    ap.add_argument("-n", "--n_generate", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epoch", type=str, default="best")
    ap.add_argument("-save", "--save_images", type=bool, default=True)
    ap.add_argument("--guidance_scale", type=float, default=None)
    ap.add_argument("--stat", type=str, default=None)
    ap.add_argument("--skip_fid", action="store_true")
    ap.add_argument("--fid_extractor", type=str, default=None,
                    help="'module:attribute' of the feature extractor the FID uses (the reference builds pytorch_fid's InceptionV3, "
                         "whose weights this image cannot download): callable(batch in [0,1]) -> [features [B, 2048, h, w]]")
    ap.add_argument("--fid_stats", type=str, default=None, help="statistics npz (`mu`, `sigma`) instead of the dataset's PNG folder")
    ap.add_argument("--synthetic", type=str, default=None, help="builtin config name, e.g. cifar10_T10 (random weights)")
    ap.add_argument("--no_graph", action="store_true", help="issue every launch from python instead of replaying the T-step loop of a "
                                                           "batch as one hipGraph (dxmi_hip/graph.py; DXMI_GRAPH=0 does the same)")
    ap.add_argument("--teacher_ckpt", type=str, default=None,
                    help="sample the DDPM teacher itself: a plain state dict of the bare network (train_ddpm.py's ema_*.pt / model*.pt)")
    ap.add_argument("--ddpm_steps", type=int, default=None, help="with --teacher_ckpt: transitions per image (default 1000)")
    ap.add_argument("--eta", type=float, default=None, help="with --teacher_ckpt: 1 ancestral (default), 0 DDIM")
    ap.add_argument("--variance", type=str, default=None, choices=("small", "large"),
                    help="with --teacher_ckpt: the posterior variance (default) or Ho et al.'s fixedlarge (needs --eta 1)")
    ap.add_argument("--skip_type", type=str, default=None, choices=("uniform", "quad", "logsnr"),
                    help="with --teacher_ckpt: spacing of the steps (logsnr: with --solver dpmpp / sde-dpmpp only, their default)")
    ap.add_argument("--no_clip", action="store_true", help="with --teacher_ckpt: do not clip the predicted x_0 to [-1, 1]")
    ap.add_argument("--generator", type=str, default=None, choices=("dummy", "determ", "determ-indiv"),
                    help="with --teacher_ckpt: dummy (default) draws on the device; determ / determ-indiv make image i independent "
                         "of batch size and rank count (models/cm/random_util.py)")
    ap.add_argument("--sampler_generator", type=str, default="dummy", choices=("dummy", "determ", "determ-indiv"),
                    help="the DxMI sampler's draws (without --teacher_ckpt): dummy draws on the device; determ / determ-indiv make "
                         "image i independent of batch size and rank count and name the PNGs by global index (--seed is their seed)")
    ap.add_argument("--config", type=str, default=None,
                    help="with --teacher_ckpt: builtin:NAME or a yaml path, for a --log_dir that holds no config.yaml")
    ap.add_argument("--solver", type=str, default=None, choices=("ancestral", "dpmpp", "sde-dpmpp"),
                    help="with --teacher_ckpt: ancestral (default: ddpm_sample, with --eta / --variance), or multistep DPM-Solver++ as "
                         "the ODE solver (dpmpp) or its SDE variant (sde-dpmpp); --ddpm_steps then defaults to 10")
    ap.add_argument("--solver_order", type=int, default=None, choices=(1, 2, 3), help="with --solver dpmpp (1-3) / sde-dpmpp (1-2): default 2")
    ap.add_argument("--solver_type", type=str, default=None, choices=("midpoint", "exact"),
                    help="with --solver dpmpp / sde-dpmpp: the second-order rows' weights (default midpoint)")
    ap.add_argument("--no_lower_order_final", action="store_true",
                    help="with --solver dpmpp / sde-dpmpp: keep the order up to the last transition")
    args, unknown = ap.parse_known_args(argv)
    given = [f"--{k}" for k in TEACHER_FLAGS if getattr(args, k) is not None] + (["--no_clip"] if args.no_clip else [])
    given += [f"--{k}" for k in SOLVER_FLAGS if getattr(args, k) is not None] + (["--no_lower_order_final"] if args.no_lower_order_final else [])
    if args.teacher_ckpt is None and given:
        ap.error(f"{', '.join(given)} only apply with --teacher_ckpt")
    if args.teacher_ckpt is not None and args.guidance_scale is not None:
        ap.error("--teacher_ckpt and --guidance_scale exclude each other")
    if args.teacher_ckpt is not None and args.sampler_generator != "dummy":
        ap.error("--sampler_generator is the DxMI sampler's: with --teacher_ckpt use --generator")
    if args.teacher_ckpt is not None and args.solver in SOLVERS:
        refused = [f"--{k}" for k in ("eta", "variance") if getattr(args, k) is not None]
        if refused:
            ap.error(f"{', '.join(refused)} belong to --solver ancestral, not to --solver {args.solver}")
        args.ddpm_steps = 10 if args.ddpm_steps is None else args.ddpm_steps
        args.solver_order = 2 if args.solver_order is None else args.solver_order
        args.solver_type, args.skip_type = args.solver_type or "midpoint", args.skip_type or "logsnr"
        args.generator = args.generator or "dummy"
        if args.solver == "sde-dpmpp" and args.solver_order == 3:
            ap.error("--solver sde-dpmpp is defined for --solver_order 1 and 2")
        from models.DxMI.dpm_sample import dpm_timesteps
        try:
            dpm_timesteps(args.ddpm_steps, skip_type=args.skip_type)
        except ValueError as e:
            ap.error(str(e))
    elif args.teacher_ckpt is not None:
        only = [f"--{k}" for k in SOLVER_FLAGS[1:] if getattr(args, k) is not None] + (["--no_lower_order_final"] if args.no_lower_order_final else [])
        only += ["--skip_type logsnr"] if args.skip_type == "logsnr" else []
        if only:
            ap.error(f"{', '.join(only)} only apply with --solver dpmpp or --solver sde-dpmpp")
        args.solver = "ancestral"
        args.ddpm_steps = 1000 if args.ddpm_steps is None else args.ddpm_steps
        args.eta = 1.0 if args.eta is None else args.eta
        args.variance, args.skip_type = args.variance or "small", args.skip_type or "uniform"
        args.generator = args.generator or "dummy"
        if args.variance == "large" and args.eta != 1.0:
            ap.error("--variance large is the ancestral sampler's: it needs --eta 1")
        if not 0.0 <= args.eta <= 1.0 or args.ddpm_steps < 1:
            ap.error("--eta must lie in [0, 1] and --ddpm_steps be at least 1")
    return args


def main(argv=None):
    args = parse_args(argv)

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    device = _dist.rank_device(local_rank)
    torch.cuda.set_device(device)
    seed = args.seed
    torch.manual_seed(seed + local_rank)
    np.random.seed(seed + local_rank)
    torch.cuda.manual_seed_all(seed + local_rank)
    random.seed(seed + local_rank)
    assert args.n_generate % args.batchsize == 0, "n_generate must be a multiple of batchsize"

    if args.config is not None:
        if args.config.startswith("builtin:"):
            import configs_builtin
            run_config = configs_builtin.get(args.config.split(":", 1)[1])
        else:
            run_config = dxmi_config.load(args.config)
    elif args.synthetic:
        import configs_builtin
        run_config = configs_builtin.get(args.synthetic)
    else:
        config_path = os.path.join(args.log_dir, "config.yaml")
        if not os.path.exists(config_path):
            raise ValueError(f"Config not found at {config_path}")
        run_config = dxmi_config.load(config_path)
    output_path = os.path.join(args.log_dir, "generated" if args.guidance_scale is None else f"generated_{args.guidance_scale}")
    mkdir_p(output_path)

    net = dxmi_config.instantiate(run_config.sampler_net)
    if args.teacher_ckpt is not None:
        return generate_teacher(args, run_config, net, device, local_rank, world, output_path)
    sampler = dxmi_config.instantiate(run_config.sampler, net=net).to(device)
    if not args.synthetic:
        sampler_path = os.path.join(args.log_dir, f"sampler_{args.epoch}.pth")
        if not os.path.exists(sampler_path) and os.path.exists(os.path.join(args.log_dir, "sampler.pth")):
            sampler_path = os.path.join(args.log_dir, "sampler.pth")
        if not os.path.exists(sampler_path):
            raise ValueError(f"Sampler not found at {sampler_path}")
        ckpt = torch.load(sampler_path, map_location=device)
        sampler.net.load_state_dict(ckpt["state_dict"])
        print0(f"Loaded sampler from {sampler_path} (epoch {ckpt.get('epoch')}, FID {ckpt.get('fid')})")
    sampler.eval()
    from dxmi_hip import graph as hip_graph
    sampler.use_graph = hip_graph.default_enabled() and not args.no_graph     # second batch onwards: one hipGraphLaunch per batch

    trainer = None
    if args.guidance_scale is not None:   # reference :160-191: value net from value_best.pth, trainer only as the sampling driver
        v = dxmi_config.instantiate(run_config.value).to(device)
        if not args.synthetic:
            value_path = os.path.join(args.log_dir, "value_best.pth")
            if not os.path.exists(value_path) and os.path.exists(os.path.join(args.log_dir, f"value_{args.epoch}.pth")):
                value_path = os.path.join(args.log_dir, f"value_{args.epoch}.pth")
            if not os.path.exists(value_path):
                raise ValueError(f"Value ftn not found at {value_path}")
            v.load_state_dict(torch.load(value_path, map_location=device)["state_dict"])
        v.eval()
        trainer = dxmi_config.instantiate(run_config.trainer, batchsize=args.batchsize)
        trainer.set_models(f=None, v=v, sampler=sampler, optimizer=None, optimizer_fstar=None, optimizer_v=None)

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend=_dist.dist_backend(), init_method="env://")  # RCCL; only the final barrier uses it

    generator = None
    if args.sampler_generator != "dummy":       # after the process group is up: the generator reads its rank and world size
        from models.cm.random_util import get_generator
        generator = get_generator(args.sampler_generator, int(args.n_generate / args.batchsize / world) * args.batchsize * world, args.seed)

    def batch(i_batch):
        if generator is not None:       # the images all ranks have finished; the batch's draws count from 0 again
            generator.set_done_samples(i_batch * args.batchsize * world)
        with torch.no_grad():
            if trainer is not None:
                return trainer.sample_guidance(n_sample=args.batchsize, device=device, guidance_scale=args.guidance_scale,
                                               generator=generator)["sample"]
            return sampler.sample(args.batchsize, device=device, generator=generator)["sample"]

    generate_and_score(args, run_config, batch, device, local_rank, world, output_path, by_global_index=generator is not None)


def generate_teacher(args, run_config, net, device, local_rank, world, output_path):
    """--teacher_ckpt: the DDPM teacher under ddpm_sample, through the output stage and the FID flow of the sampler path."""
    from dxmi_hip import graph as hip_graph
    from models.DxMI.ddpm_sample import ddpm_sample
    from models.DxMI.dpm_sample import dpm_sample
    from utils import fix_legacy_dict
    net = net.to(device)
    net.load_state_dict(fix_legacy_dict(torch.load(args.teacher_ckpt, map_location=device)))
    net.eval()
    if args.solver in SOLVERS:
        print0(f"Loaded the DDPM teacher from {args.teacher_ckpt}: DPM-Solver++ ({SOLVERS[args.solver]}), {args.ddpm_steps} "
               f"{args.skip_type} steps, order {args.solver_order}, {args.solver_type}, lower_order_final "
               f"{not args.no_lower_order_final}, clip_denoised {not args.no_clip}, generator {args.generator}")
    else:
        print0(f"Loaded the DDPM teacher from {args.teacher_ckpt}: {args.ddpm_steps} {args.skip_type} steps, eta {args.eta}, "
               f"variance {args.variance}, clip_denoised {not args.no_clip}, generator {args.generator}")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend=_dist.dist_backend(), init_method="env://")
    n_batches = int(args.n_generate / args.batchsize / world)
    generator = None
    if args.generator != "dummy":       # after the process group is up: the generator reads its rank and world size
        from models.cm.random_util import get_generator
        generator = get_generator(args.generator, n_batches * args.batchsize * world, args.seed)
    use_graph = hip_graph.default_enabled() and not args.no_graph
    shape = (args.batchsize,) + tuple(run_config.sampler.sample_shape)

    def batch(i_batch):
        if generator is not None:       # the images all ranks have finished; the batch's draws count from 0 again
            generator.set_done_samples(i_batch * args.batchsize * world)
        if args.solver in SOLVERS:
            return dpm_sample(net, shape, steps=args.ddpm_steps, order=args.solver_order, algorithm=SOLVERS[args.solver],
                              solver_type=args.solver_type, skip_type=args.skip_type, lower_order_final=not args.no_lower_order_final,
                              clip_denoised=not args.no_clip, device=device, generator=generator, use_graph=use_graph)
        return ddpm_sample(net, shape, steps=args.ddpm_steps, eta=args.eta, variance=args.variance, skip_type=args.skip_type,
                           clip_denoised=not args.no_clip, device=device, generator=generator, use_graph=use_graph)

    generate_and_score(args, run_config, batch, device, local_rank, world, output_path)


def generate_and_score(args, run_config, batch, device, local_rank, world, output_path, by_global_index=False):
    """batch(i) -> [batchsize, 3, H, W] in [-1, 1], n_batches times: PNGs under output_path, then the FID on rank 0.  The PNGs are
    `{rank}_{count}.png`, or with by_global_index `{i}.png` by the deterministic generators' global index of the row."""
    n_batches = int(args.n_generate / args.batchsize / world)
    i_img = 0
    from utils import ImageWriter
    writer = ImageWriter()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i_batch in range(n_batches):
        sample = batch(i_batch)
        if args.save_images:
            # rescale -> clamp -> save_image rounding on the device (dxmi_quantize_u8), pinned double-buffered copy on a side
            # stream, PNGs from a thread pool: the sampler never waits for the files
            n = sample.shape[0]
            names = [f"{i_batch * n * world + local_rank + k * world}.png" if by_global_index else f"{local_rank}_{i_img + k}.png" for k in range(n)]
            writer.submit(sample, [os.path.join(output_path, name) for name in names])
            i_img += n
    writer.close()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        torch.distributed.barrier()
    print0(f"Generated {args.n_generate} samples at {output_path} "
           f"({n_batches * args.batchsize / dt:.1f} images/s/rank incl. PNG writing)")

    data_path = args.fid_stats or os.path.join("datasets", f"{run_config.data.name}_train_png")
    if args.skip_fid or local_rank != 0:
        return
    if args.fid_extractor is None:
        print0("FID skipped: pass --fid_extractor module:attr (an InceptionV3 pool3 extractor; its weights are not in this image)")
        return
    if not os.path.exists(data_path):
        print0(f"Dataset not found at {data_path}: FID skipped")
        return
    # reference :212-216: FID of the generated PNG folder against the dataset; the activation statistics run on the device
    from pytorch_fid.fid_score import calculate_fid_given_paths, load_extractor
    extractor = load_extractor(args.fid_extractor)
    if hasattr(extractor, "to"):
        extractor = extractor.to(device)
    fid = calculate_fid_given_paths([output_path, data_path], batch_size=args.batchsize, device=device, dims=2048, extractor=extractor)
    print(f"FID score: {fid}")


if __name__ == "__main__":
    main()
