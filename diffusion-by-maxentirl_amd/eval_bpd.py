"""Bits per dimension of a uint8 image array under an EDM net or the DDPM teacher: the test-set likelihood of the probability-flow
ODE (models/cm/likelihood.py, models/DxMI/likelihood.py), on MI355X.  The reference has no such program.

    python eval_bpd.py --data_npz test.npz --pretrained edm.pt [--config builtin:imagenet64_T10] [--steps 40]
    python eval_bpd.py --data_npz test.npz --teacher_ckpt ema.pt [--config builtin:cifar10_T10] [--steps 40] [--skip_type uniform]

`--pretrained PATH`: a plain state dict of the EDM U-Net (the config's `diffusion:` block builds it; class-conditional nets take the
labels from the file's arr_1).  `--teacher_ckpt PATH`: a plain state dict of the bare DDPM network (train_ddpm.py's ema_*.pt), the
config's `sampler_net:`; `--skip_type` spaces its integer steps (uniform, the default, accepts any --steps below T; logsnr at most 37).
`--n_images N` scores the file's first N images (default: all), `--batchsize` is per rank.  Image i is row k of batch b on rank r
with i = b * batchsize * world + r + k * world (generate_large.py's order); the per-image values are gathered and written as
`bpd_N.npz` (arr_0 in global-index order) next to the data file, or under --out_dir.  `--repeats R` averages R probe (and
dequantisation) draws per image; the printed standard error is over the images.  `--generator determ` (the default) makes image i's
probe and dequantisation noise independent of --batchsize and of the number of ranks; `dummy` draws with torch.
"""
import argparse
import math
import os

import numpy as np
import torch

PROBES = ("rademacher", "gaussian")
DEQUANTIZE = ("uniform", "center")
GENERATORS = ("determ", "determ-indiv", "dummy")
SKIP_TYPES = ("uniform", "logsnr", "quad")


def build_parser():
    ap = argparse.ArgumentParser(description="bits/dim of a uint8 image array under an EDM net or the DDPM teacher")
    ap.add_argument("--data_npz", type=str, required=True, help="uint8 images [M, H, W, C] (.npz arr_0, labels arr_1; or .npy)")
    ap.add_argument("--pretrained", type=str, default=None, help="plain state dict of the EDM U-Net")
    ap.add_argument("--teacher_ckpt", type=str, default=None, help="plain state dict of the bare DDPM network")
    ap.add_argument("--config", type=str, default=None, help="builtin:NAME or a yaml path (default builtin:imagenet64_T10 with "
                                                             "--pretrained, builtin:cifar10_T10 with --teacher_ckpt)")
    ap.add_argument("--steps", type=int, default=40, help="Heun steps: 2 * steps network evaluations per image")
    ap.add_argument("--skip_type", type=str, default=None, choices=SKIP_TYPES, help="with --teacher_ckpt: spacing of the integer steps")
    ap.add_argument("--rho", type=float, default=None, help="with --pretrained: the Karras ladder's rho (default 7)")
    ap.add_argument("--batchsize", type=int, default=64)
    ap.add_argument("--n_images", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--probe", type=str, default="rademacher", choices=PROBES)
    ap.add_argument("--dequantize", type=str, default="uniform", choices=DEQUANTIZE)
    ap.add_argument("--generator", type=str, default="determ", choices=GENERATORS)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out_dir", type=str, default=None, help="where bpd_N.npz goes (default: the data file's directory)")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if (args.pretrained is None) == (args.teacher_ckpt is None):
        ap.error("exactly one of --pretrained (an EDM net) and --teacher_ckpt (the DDPM teacher) is needed")
    if args.teacher_ckpt is not None:
        if args.rho is not None:
            ap.error("--rho shapes the EDM nets' Karras ladder: it does not apply with --teacher_ckpt")
        args.skip_type = args.skip_type or "uniform"
        args.config = args.config or "builtin:cifar10_T10"
    else:
        if args.skip_type is not None:
            ap.error("--skip_type spaces the DDPM teacher's integer steps: it does not apply with --pretrained")
        args.rho = 7.0 if args.rho is None else args.rho
        args.config = args.config or "builtin:imagenet64_T10"
    if args.steps < 1 or args.batchsize < 1 or args.repeats < 1 or (args.n_images is not None and args.n_images < 1):
        ap.error("--steps, --batchsize, --repeats and --n_images must be at least 1")
    return args


def shard_rows(n, batchsize, rank, world):
    """The global indices of this rank's batches, in order: image i is row k of batch b on rank r with
    i = b * batchsize * world + r + k * world; the last batch holds what is left below n."""
    out, per = [], batchsize * world
    for done in range(0, n, per):
        rows = torch.arange(done + rank, min(done + per, n), world, dtype=torch.int64)
        out.append((done, rows))
    return out


def merge(n, parts):
    """parts: (global indices, values [len, ...]) of every rank -> the values in global-index order; every index in [0, n) must be
    covered exactly once."""
    idx = torch.cat([p[0] for p in parts])
    vals = torch.cat([p[1] for p in parts])
    if sorted(idx.tolist()) != list(range(n)):
        raise RuntimeError(f"the ranks' shards do not cover the {n} images exactly once")
    out = torch.empty((n,) + tuple(vals.shape[1:]), dtype=vals.dtype)
    out[idx] = vals
    return out


def score_rank(score, raw, n, batchsize, rank, world, repeats=1, dequantize="uniform", generator="determ", seed=0):
    """This rank's share: score(x0, labels, generator) -> bpd [B] over its batches -> (global indices, bpd [len, repeats]).  raw(rows)
    -> (uint8 [B, C, H, W], labels or None).  generator: one of GENERATORS; repeat j draws with seed + j."""
    from models.cm.likelihood import dequantize_u8
    from models.cm.random_util import DeterministicGenerator
    shards = shard_rows(n, batchsize, rank, world)
    cols = []
    for j in range(repeats):
        g = DeterministicGenerator(n, seed + j, rank=rank, world_size=world) if generator != "dummy" else None
        vals = []
        for done, rows in shards:
            if not len(rows):
                continue
            if g is not None:       # the images all ranks have finished; the batch's draws count from 0 again
                g.set_done_samples(done)
            u8, y = raw(rows)
            vals.append(score(dequantize_u8(u8, dequantize, g), y, g).detach().float().cpu())
        cols.append(torch.cat(vals) if vals else torch.empty(0))
    idx = torch.cat([rows for _, rows in shards]) if shards else torch.empty(0, dtype=torch.int64)
    return idx, torch.stack(cols, dim=1)


def summary(bpd, repeats, nfe):
    n = len(bpd)
    mean = float(bpd.double().mean())
    se = float(bpd.double().std(unbiased=True) / math.sqrt(n)) if n > 1 else float("nan")
    return f"bits/dim: {mean:.4f} ± {se:.4f} over {n} images ({repeats} repeat{'s' if repeats != 1 else ''}), NFE {nfe}"


def load_config(name):
    import dxmi_config
    if name.startswith("builtin:"):
        import configs_builtin
        return configs_builtin.get(name.split(":", 1)[1])
    return dxmi_config.load(name)


def build_scorer(args, cfg, device):
    """-> (score(x0, labels, generator) -> bpd [B], class_cond)."""
    import dxmi_config
    from utils import fix_legacy_dict, print0
    if args.teacher_ckpt is not None:
        from models.DxMI.likelihood import ddpm_log_likelihood
        net = dxmi_config.instantiate(cfg.sampler_net).to(device)
        net.load_state_dict(fix_legacy_dict(torch.load(args.teacher_ckpt, map_location=device)))
        net.eval()
        print0(f"Loaded the DDPM teacher from {args.teacher_ckpt}: {args.steps} {args.skip_type} Heun steps, probe {args.probe}")
        return (lambda x0, y, g: ddpm_log_likelihood(net, x0, steps=args.steps, skip_type=args.skip_type, probe=args.probe,
                                                     generator=g)["bpd"]), False
    from models.cm.likelihood import edm_log_likelihood
    from models.cm.script_util import create_model_and_diffusion
    unet, diffusion = create_model_and_diffusion(**cfg.diffusion)
    unet.load_state_dict(torch.load(args.pretrained, map_location="cpu"))
    unet.to(device)
    if cfg.diffusion.get("use_fp16"):
        unet.convert_to_fp16()
    unet.eval()
    cond = unet.num_classes is not None
    print0(f"EDM weights loaded from {args.pretrained}: {args.steps} Heun steps on the Karras ladder (rho {args.rho}), probe {args.probe}")
    return (lambda x0, y, g: edm_log_likelihood(diffusion, unet, x0, steps=args.steps, rho=args.rho, probe=args.probe,
                                                model_kwargs={"y": y} if cond else None, generator=g)["bpd"]), cond


def main(argv=None):
    args = parse_args(argv)
    from dxmi_hip import dist as _dist
    from dxmi_hip.data import ImageStore
    from utils import mkdir_p, print0
    local_rank, world = int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    device = _dist.rank_device(local_rank)
    torch.cuda.set_device(device)
    torch.manual_seed(args.seed + local_rank)
    torch.cuda.manual_seed_all(args.seed + local_rank)
    cfg = load_config(args.config)
    score, cond = build_scorer(args, cfg, device)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend=_dist.dist_backend(), init_method="env://")
    store = ImageStore(args.data_npz, device, "adm", batch_size=1, random_flip=False, class_cond=cond)
    n = store.M if args.n_images is None else min(args.n_images, store.M)
    idx, vals = score_rank(score, store.raw, n, args.batchsize, local_rank, world, args.repeats, args.dequantize, args.generator, args.seed)
    parts = [(idx, vals)]
    if world > 1:       # shards differ in length by at most one batch tail: gathered as python objects
        parts = [None] * world
        torch.distributed.all_gather_object(parts, (idx, vals))
    if local_rank == 0:
        per_repeat = merge(n, parts)
        bpd = per_repeat.double().mean(dim=1)
        out_dir = args.out_dir or os.path.dirname(os.path.abspath(args.data_npz))
        mkdir_p(out_dir)
        np.savez(os.path.join(out_dir, f"bpd_{n}.npz"), bpd.numpy().astype(np.float32))
        print0(summary(bpd, args.repeats, 2 * args.steps))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
