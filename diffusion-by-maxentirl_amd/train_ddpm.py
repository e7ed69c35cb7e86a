"""Train the CIFAR-10 DDPM U-Net with the noise-prediction loss: the teacher `train_cifar10.py` reads as `training.sampler_ckpt`
(models.DxMI.ddpm_train.DDPMTrainLoop over DDPMSchedule.training_losses; Ho et al. 2020 — the reference downloads this network and
has no code that trains it).

    torchrun --nproc_per_node=8 train_ddpm.py --config builtin:cifar10_T10 --data_npz cifar10_train.npz --run t0
    python train_ddpm.py --config builtin:cifar10_T10 --synthetic_data --max_iters 2 --run smoke
    python train_cifar10.py --config builtin:cifar10_T10 --dataset builtin --data_npz cifar10_train.npz --run r0 \\
        --training.sampler_ckpt results/cifar10/cifar10_T10_ddpm/t0/ema_0.9999_800000.pt

The network is the config's `sampler_net` block (dropout 0.1 included), the forward process the 1000-step linear-beta schedule
VARSampler is built on.  --batch_size is the global batch: a rank steps batch_size // world images.  --data_npz PATH trains on a
uint8 image array file (dxmi_hip/data.py ImageStore: ToTensor's scaling to [-1, 1], random horizontal flips, --data_resident
auto|device|host); --synthetic_data feeds uniform images (smoke runs); the two exclude each other and one of them is required.
Checkpoints go to results/<data name>/<config>_ddpm/<run>/: model%06d.pt, ema_{rate}_%06d.pt (plain state dicts of the bare network,
what `training.sampler_ckpt` takes) and opt%06d.pt; --resume PATH continues from a model file.  --max_iters N stops after N steps
(and saves).  The step is replayed from hipGraphs unless --no_graph or DXMI_GRAPH=0.
"""
import argparse
import os

import torch

import dxmi_config
from dxmi_hip import dist as _dist
from dxmi_hip import graph as _graph
from utils import mkdir_p, print0


def synthetic_batches(batch_size, shape, device, seed):
    gen = torch.Generator(device=device).manual_seed(seed)
    while True:
        yield torch.rand(batch_size, *shape, device=device, generator=gen) * 2 - 1, {}


def make_loader(args, batch_size, shape, device, rank, world, seed):
    """The `data=` iterator of DDPMTrainLoop for the parsed flags, and the ImageStore behind it (None for synthetic data)."""
    if args.data_npz:
        from dxmi_hip.data import NORM_TOTENSOR, ImageStore
        store = ImageStore(args.data_npz, device, NORM_TOTENSOR, batch_size=batch_size, rank=rank, world=world, seed=seed,
                           random_flip=True, resident=args.data_resident)
        return store.batches(), store
    if not args.synthetic_data:
        raise NotImplementedError("train_ddpm.py: image folders are not read by this package; run with --data_npz PATH (an uint8 array "
                                  "file, see make_npz.py) or --synthetic_data")
    return synthetic_batches(batch_size, shape, device, seed + rank), None


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--dataset", type=str, default="builtin")
    ap.add_argument("--run", type=str, default="run")
    ap.add_argument("--synthetic_data", action="store_true")
    ap.add_argument("--data_npz", type=str, default="", help="uint8 image array file: .npz with arr_0 [M, 32, 32, 3], or .npy")
    ap.add_argument("--data_resident", choices=("auto", "device", "host"), default="auto",
                    help="keep the array in device memory, or on the host behind a prefetch thread (auto: by its size)")
    ap.add_argument("--batch_size", type=int, default=128, help="global batch: a rank steps batch_size // world images")
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--warmup_steps", type=int, default=5000)
    ap.add_argument("--ema_rate", type=str, default="0.9999", help="comma-separated EMA rates")
    ap.add_argument("--grad_clip", type=float, default=1.0)
    ap.add_argument("--total_steps", type=int, default=800000)
    ap.add_argument("--save_interval", type=int, default=10000)
    ap.add_argument("--log_interval", type=int, default=100)
    ap.add_argument("--max_iters", type=int, default=None, help="stop after this many steps (smoke runs)")
    ap.add_argument("--resume", type=str, default="", help="a model%%06d.pt file: its step, opt and EMA files are read next to it")
    ap.add_argument("--seed", type=int, default=None, help="default: the config's training.seed")
    ap.add_argument("--batch_invariant", action="store_true",
                    help="keep one conv kernel per layer shape whatever the batch size instead of routing under-filled grids to "
                         "smaller tiles (dxmi_hip.ops.tune_for_throughput)")
    ap.add_argument("--no_graph", action="store_true",
                    help="issue every kernel launch from python instead of replaying the step from hipGraphs (DXMI_GRAPH=0 does the same)")
    args = ap.parse_args(argv)
    if args.synthetic_data and args.data_npz:
        ap.error("--synthetic_data and --data_npz exclude each other")
    if args.batch_size < 1:
        ap.error("--batch_size must be at least 1")
    return args


def log_dir_of(args, cfg):
    name = os.path.basename(args.config).split(".")[0].replace("builtin:", "")
    return os.path.join(f"results/{cfg.data.name}/{name}_ddpm", args.run)


def main(argv=None):
    args = parse_args(argv)
    from train_cifar10 import load_config
    cfg = load_config(args.config, args.dataset)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    batch_size = args.batch_size // world
    if batch_size < 1:
        raise ValueError(f"--batch_size {args.batch_size} leaves no image for each of {world} ranks")
    seed = cfg.training.seed if args.seed is None else args.seed
    shape = tuple(cfg.sampler.sample_shape)
    logdir = log_dir_of(args, cfg)
    if not args.data_npz and not args.synthetic_data:
        make_loader(args, batch_size, shape, "cpu", local_rank, world, seed)       # refused before the device is touched

    device = _dist.rank_device(local_rank)
    torch.cuda.set_device(device)
    if not args.batch_invariant:
        from dxmi_hip import ops as _ops
        _ops.tune_for_throughput()
    torch.manual_seed(seed + local_rank)
    torch.cuda.manual_seed_all(seed + local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend=_dist.dist_backend(), init_method="env://")   # RCCL

    from models.DxMI.ddpm_train import DDPMSchedule, DDPMTrainLoop
    net = dxmi_config.instantiate(cfg.sampler_net).to(device).train()
    data, store = make_loader(args, batch_size, shape, device, local_rank, world, seed)
    if store is not None:
        print0(store.describe())
    if local_rank == 0:
        mkdir_p(logdir)
    total = args.max_iters if args.max_iters is not None else args.total_steps
    loop = DDPMTrainLoop(model=net, schedule=DDPMSchedule(), data=data, batch_size=batch_size, lr=args.lr, warmup_steps=args.warmup_steps,
                         grad_clip=args.grad_clip, ema_rate=args.ema_rate, log_interval=args.log_interval,
                         save_interval=args.save_interval, resume_checkpoint=args.resume, log_dir=logdir,
                         total_steps=total + (0 if args.max_iters is None else _resume_step(args.resume)),
                         use_graph=_graph.default_enabled() and not args.no_graph)
    print0(f"DDPM noise-prediction training: {sum(p.numel() for p in net.parameters()) / 1e6:.1f} M parameters, {world} rank(s) x "
           f"{batch_size} images, steps {loop.step} -> {loop.total_steps}, checkpoints in {logdir}")
    loop.run_loop()
    if loop.logged:
        print0("last log row:", loop.logged[-1])
    print0(f"saved {logdir}/ema_{loop.ema_rate[0]}_{loop.step:06d}.pt (training.sampler_ckpt of train_cifar10.py)")
    if store is not None:
        store.close()
    if world > 1:
        torch.distributed.destroy_process_group()


def _resume_step(path):
    from models.cm.train_util import parse_resume_step_from_filename
    return parse_resume_step_from_filename(path) if path else 0


if __name__ == "__main__":
    main()
