"""DxMI training for CIFAR-10 on MI355X (CLI-compatible with the reference's train_cifar10.py:208-462
for the training path).

    torchrun --nproc_per_node=N train_cifar10.py --config configs/cifar10/T10.yaml \
        --dataset configs/cifar10/cifar10.yaml --run myrun [--training.lr 1e-7 ...]
    (or --config builtin:cifar10_T10 --dataset builtin --synthetic_data for a self-contained run)

Same flow as the reference: config merge + `--a.b.c v` overrides, seeding with seed+rank, instantiate
net / sampler / value from `_target_`, Adam with the log_betas / rest split (reference :283-296),
per-rank batch = batchsize // world, epoch loop of `train_one_epoch` (:141-205), checkpoints with the
reference's file names and state-dict keys (:58-78, :459-462).  Differences, all outside the
accelerated path: gradients are exchanged by one flat RCCL all-reduce per backward instead of DDP
buckets (dxmi_hip/dist.py); wandb / tensorboard logging is skipped; the in-training FID (training.fid_epoch / training.fid_every,
best sampler kept as sampler.pth / value.pth) runs on the device from `--fid_extractor module:attr --fid_stats stats.npz`
(FidEvaluator; without the two flags no FID is computed) instead of from PNG folders; `--data_npz PATH` trains on a uint8 image
array file (dxmi_hip/data.py ImageStore: ToTensor's scaling, random horizontal flips, `--data_resident auto|device|host`); `--synthetic_data` feeds uniform images (benchmarks, smoke runs).
"""
import argparse
import os
import random

import numpy as np
import torch
from dxmi_hip import dist as _dist

import cmd_utils as cmd
import dxmi_config
from dxmi_hip.dist import broadcast_parameters
from dxmi_hip.optim import Adam          # torch.optim.Adam subclass: step() is one multi-tensor HIP kernel series
from models.DxMI.replay import TransitionRing
from models.DxMI.trainer import append_buffer, reset_buffer
from utils import fix_legacy_dict, mkdir_p, print0


def save_model(trainer, logdir, postfix, d_other_info=None):
    """sampler_{postfix}.pth / value_{postfix}.pth with reference key names (train_cifar10.py:58-78)."""
    d = {"state_dict": trainer.sampler.net.state_dict()}
    d.update(d_other_info or {})
    torch.save(d, os.path.join(logdir, f"sampler_{postfix}.pth"))
    if trainer.v is not None:
        torch.save({"state_dict": trainer.v.state_dict()}, os.path.join(logdir, f"value_{postfix}.pth"))


def synthetic_loader(batchsize, n_batches, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    for _ in range(n_batches):
        yield torch.rand(batchsize, 3, 32, 32, device=device, generator=g), None


def make_store(args, cfg, device, rank, world):
    """The ImageStore of --data_npz (None without the flag): ToTensor's normalisation with the `2 * images - 1` of train_one_epoch
    applied in the same launch, the per-rank batch, and the seed and rank the synthetic loader gets."""
    if not args.data_npz:
        return None
    from dxmi_hip.data import NORM_TOTENSOR, ImageStore
    return ImageStore(args.data_npz, device, NORM_TOTENSOR, batch_size=cfg.training.batchsize // world, rank=rank, world=world,
                      seed=cfg.training.seed, resident=args.data_resident)


def make_loader(args, cfg, device, rank, world, epoch, store=None):
    """One epoch's (images, labels) iterable: the ImageStore's epoch, the synthetic loader, or the reference's pipeline."""
    batchsize = cfg.training.batchsize // world
    if store is not None:
        return store.epoch(epoch)
    if args.synthetic_data:
        return synthetic_loader(batchsize, args.max_iters or 100, device, cfg.training.seed + rank + epoch)
    import loader as ref_loader  # the reference's torchvision CIFAR-10 pipeline (out of scope here)
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    train_set = ref_loader.get_dataset(cfg.data.name, cfg.data.data_dir)
    ds = DistributedSampler(train_set) if world > 1 else None
    return DataLoader(train_set, batch_size=batchsize, shuffle=ds is None, sampler=ds, num_workers=4, pin_memory=True, drop_last=True)


class FidEvaluator:
    """The reference's in-training FID (train_cifar10.py:81-139, :384-442) on the device: int(n_fid_samples / sampling_batchsize /
    world) batches per rank from the sampler in eval(), each quantised to uint8 as save_image would store it before the next
    sample() call (with use_graph the returned tensors are the graph's static outputs), activations gathered over RCCL, statistics
    by dxmi_fid_stats, the distance by `distance` ("device": fp64 MFMA Newton-Schulz, "host": scipy's sqrtm).  Every rank computes
    the same value; rank 0 keeps the best-scoring sampler as sampler.pth / value.pth, which is what generate_cifar10.py loads.
    The samples go to no replay ring, and the sampler's train() / eval() flag is put back.
    --fid_generator determ: every evaluation samples the same n_fid_samples noise streams (a DeterministicGenerator seeded with
    training.seed, set_done_samples before each batch), so the FID of two checkpoints differs by the weights alone."""

    def __init__(self, args, cfg, trainer, sampler, logdir, device, rank, world):
        from pytorch_fid.fid_score import load_extractor, load_statistics
        extractor = load_extractor(args.fid_extractor)
        self.extractor = extractor.to(device) if hasattr(extractor, "to") else extractor
        self.m2, self.s2 = load_statistics(args.fid_stats)
        self.dims, self.distance = args.fid_dims, args.fid_distance
        self.n_batches = int(cfg.training.n_fid_samples / cfg.training.sampling_batchsize / world)
        self.sampling_batchsize = cfg.training.sampling_batchsize
        self.trainer, self.sampler, self.logdir, self.device, self.rank = trainer, sampler, logdir, device, rank
        self.best_fid = float("inf")
        self.world, self.generator = world, None
        if getattr(args, "fid_generator", "dummy") != "dummy":      # built after the process group: it reads its rank and world size
            from models.cm.random_util import get_generator
            self.generator = get_generator(args.fid_generator, self.n_batches * self.sampling_batchsize * world, cfg.training.seed)

    def _batch(self, i_batch):
        if self.generator is not None:
            self.generator.set_done_samples(i_batch * self.sampling_batchsize * self.world)
            return self.sampler.sample(self.sampling_batchsize, device=self.device, generator=self.generator)["sample"]
        return self.sampler.sample(self.sampling_batchsize, device=self.device)["sample"]

    def __call__(self, epoch, i_iter):
        from dxmi_hip import ops
        from pytorch_fid.fid_score import fid_from_images
        was_training = self.sampler.training
        print0("generating images for FID evaluation")
        self.sampler.eval()
        images = torch.cat([ops.quantize_u8(self._batch(i), mode=0, nhwc=False) for i in range(self.n_batches)])
        print0("calculating FID score")
        fid = fid_from_images(images, self.extractor, self.m2, self.s2, batch_size=50, dims=self.dims, device=self.device,
                              distance=self.distance)
        if self.rank == 0 and fid < self.best_fid:
            self.best_fid = fid
            path = os.path.join(self.logdir, "sampler.pth")
            torch.save({"state_dict": self.trainer.sampler.net.state_dict(), "fid": fid, "epoch": epoch, "iter": i_iter}, path)
            if self.trainer.v is not None:
                torch.save({"state_dict": self.trainer.v.state_dict()}, os.path.join(self.logdir, "value.pth"))
            print0(f"best FID: sampler saved at {path}")
        print0(f"FID score: {fid}")
        self.sampler.train(was_training)
        return fid


def check_fid_schedule(cfg):
    """(fid_every, fid_epoch) of cfg.training; setting both is refused as the reference refuses it (:251-253)."""
    fid_every, fid_epoch = cfg.training.get("fid_every"), cfg.training.get("fid_epoch")
    if fid_every is not None and fid_epoch is not None:
        raise ValueError("cannot set both fid_epoch and fid_every")
    return fid_every, fid_epoch


def train_one_epoch(trainer, sampler, dataloader, n_critic, n_generator, device, log_every, state, normalised=False, max_iters=None,
                    fid_every=None, evaluate=None):
    """reference train_one_epoch (:141-205) without the logging side paths.  normalised: the loader's images are already in
    [-1, 1] (ImageStore); max_iters: stop inside the epoch once state['i_iter'] reaches it; evaluate(i_iter): called at the top of
    every iteration with i_iter % fid_every == 0, iteration 0 included (reference :165-167)."""
    # device-resident replay ring: n_critic trajectories of T transitions each, generated in place by the sampler
    buf = TransitionRing(n_critic, trainer.n_timesteps, trainer.batchsize, sampler.sample_shape, device)
    for step, (images, _) in enumerate(dataloader):
        if evaluate is not None and fid_every is not None and state["i_iter"] % fid_every == 0:
            evaluate(state["i_iter"])
        sampler.eval()
        images = images.to(device) if normalised else (2 * images - 1).to(device)
        in_ring = len(images) == trainer.batchsize
        d_sample = sampler.sample(len(images), device=device, out=buf.next_slot() if in_ring else None)
        append_buffer(buf, d_sample)
        d_energy = trainer.update_f_v(images, d_sample, buf)
        if (step + 1) % n_critic == 0:
            d_sampler = trainer.update_sampler(buf, n_generator)
            buf = reset_buffer(device, ring=buf)
            if (step + 1) % log_every == 0:
                print0(f"iter {state['i_iter']}: d_loss {d_energy['ebm/d_loss_']:.4f} v_loss {d_energy['ebm/v_loss_']:.4f} "
                       f"sampler_loss {d_sampler['sampler/sampler_loss_']:.4f}")
        state["i_iter"] += 1
        if max_iters is not None and state["i_iter"] >= max_iters:
            break


def load_config(config, dataset, overrides=None):
    """--config / --dataset / `--a.b.c v` overrides -> merged Cfg (reference :228-233: OmegaConf.load x 2 + merge)."""
    if config.startswith("builtin:"):
        import configs_builtin
        cfg = configs_builtin.get(config.split(":", 1)[1])
    else:
        cfg = dxmi_config.merge(dxmi_config.load(config), dxmi_config.load(dataset))
    return dxmi_config.merge(cfg, overrides or {})


def build_optimizers(cfg, net, sampler, v):
    """Adam with the log_betas / rest learning-rate split, Adam for the value net (reference :283-296)."""
    tune_beta = bool(sampler.trainable_beta) and cfg.training.get("beta_lr") is not None
    if tune_beta:
        not_beta = [p for n, p in net.named_parameters() if "log_betas" not in n]
        optimizer = Adam([{"params": net.log_betas, "lr": cfg.training.beta_lr},
                          {"params": not_beta, "lr": cfg.training.lr}])
    else:
        optimizer = Adam(net.parameters(), lr=cfg.training.lr)
    return optimizer, Adam(v.parameters(), lr=cfg.training.v_lr)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--dataset", type=str, required=True)
    ap.add_argument("--run", type=str, default="run")
    ap.add_argument("--synthetic_data", action="store_true")
    ap.add_argument("--data_npz", type=str, default="", help="uint8 image array file: .npz with arr_0 [M, 32, 32, 3], or .npy")
    ap.add_argument("--data_resident", choices=("auto", "device", "host"), default="auto",
                    help="keep the array in device memory, or on the host behind a prefetch thread (auto: by its size)")
    ap.add_argument("--max_iters", type=int, default=None, help="stop after this many iterations (smoke runs)")
    ap.add_argument("--batch_invariant", action="store_true",
                    help="keep one conv kernel per layer shape whatever the batch size (bitwise batch-independent results) instead of "
                         "routing under-filled grids to smaller tiles (dxmi_hip.ops.tune_for_throughput)")
    ap.add_argument("--no_graph", action="store_true",
                    help="issue every kernel launch from python instead of replaying the generation call and the two updates as hipGraphs "
                         "(dxmi_hip/graph.py; DXMI_GRAPH=0 does the same)")
    ap.add_argument("--fid_extractor", type=str, default=None,
                    help="'module:attribute' of the FID feature extractor (the reference builds pytorch_fid's InceptionV3, whose weights "
                         "this image cannot download); with --fid_stats it enables the FID of training.fid_epoch / training.fid_every")
    ap.add_argument("--fid_stats", type=str, default=None, help="dataset statistics npz (`mu`, `sigma`)")
    ap.add_argument("--fid_dims", type=int, default=2048)
    ap.add_argument("--fid_distance", choices=("device", "host"), default="device",
                    help="the Frechet distance of an evaluation: fp64 MFMA Newton-Schulz on the device, or scipy's sqrtm on the host")
    ap.add_argument("--fid_generator", choices=("dummy", "determ"), default="dummy",
                    help="the noise of the in-training FID: dummy draws afresh at every evaluation; determ gives every evaluation the "
                         "same n_fid_samples noise streams (models/cm/random_util.py, seeded with training.seed)")
    args, unknown = ap.parse_known_args(argv)
    if args.synthetic_data and args.data_npz:
        ap.error("--synthetic_data and --data_npz exclude each other")
    return args, unknown


def main():
    args, unknown = parse_args()
    d_cmd_cfg = cmd.parse_nested_args(cmd.parse_unknown_args(unknown))
    print0("Overriding", d_cmd_cfg)

    cfg = load_config(args.config, args.dataset, d_cmd_cfg)

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    device = _dist.rank_device(local_rank)
    torch.cuda.set_device(device)
    if not args.batch_invariant:
        from dxmi_hip import ops as _ops
        _ops.tune_for_throughput()
    seed = cfg.training.seed
    torch.manual_seed(seed + local_rank)
    np.random.seed(seed + local_rank)
    torch.cuda.manual_seed_all(seed + local_rank)
    random.seed(seed + local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend=_dist.dist_backend(), init_method="env://")   # RCCL

    net = dxmi_config.instantiate(cfg.sampler_net)
    sampler = dxmi_config.instantiate(cfg.sampler, net=net).to(device)
    if cfg.training.sampler_ckpt and os.path.exists(cfg.training.sampler_ckpt):
        net.load_state_dict(fix_legacy_dict(torch.load(cfg.training.sampler_ckpt, map_location="cpu")), strict=False)
        print0(f"Sampler checkpoint loaded from {cfg.training.sampler_ckpt}")
    else:
        print0("no sampler checkpoint found: random initialisation")
    v = dxmi_config.instantiate(cfg.value).to(device)
    if cfg.training.get("value_ckpt") is not None:
        v.load_pretrained(torch.load(cfg.training.value_ckpt, map_location="cpu"))
    broadcast_parameters(net)
    broadcast_parameters(v)

    optimizer, optimizer_v = build_optimizers(cfg, net, sampler, v)

    batchsize = cfg.training.batchsize // world     # the reference divides by the visible device count (:298-301)
    trainer = dxmi_config.instantiate(cfg.trainer, batchsize=batchsize)
    trainer.set_models(f=None, v=v, sampler=sampler, optimizer=optimizer, optimizer_fstar=None, optimizer_v=optimizer_v)
    # per-rank batches of a multi-GPU run are small (batchsize // world): the step is replayed from hipGraphs so that the host does not
    # bound it; gradient exchanges stay eager RCCL calls at graph cuts (dxmi_hip/dist.py)
    from dxmi_hip import graph as hip_graph
    trainer.use_graphs = sampler.use_graph = hip_graph.default_enabled() and not args.no_graph

    model_cfg_name = os.path.basename(args.config).split(".")[0].replace("builtin:", "")
    logdir = os.path.join(f"results/{cfg.data.name}/{model_cfg_name}", args.run)
    if local_rank == 0:
        mkdir_p(logdir)
        dxmi_config.save(cfg, os.path.join(logdir, "config.yaml"))

    store = make_store(args, cfg, device, local_rank, world)
    if store is not None:
        print0(store.describe())
    # in-training FID (reference :81-139, :384-442): on with --fid_extractor and --fid_stats, scheduled by the config
    fid_every = fid_epoch = evaluator = None
    if args.fid_extractor is not None and args.fid_stats is not None:
        fid_every, fid_epoch = check_fid_schedule(cfg)
        evaluator = FidEvaluator(args, cfg, trainer, sampler, logdir, device, local_rank, world)
    state = {"i_iter": 0}
    for epoch in range(cfg.training.n_epochs):
        loader = make_loader(args, cfg, device, local_rank, world, epoch, store)
        train_one_epoch(trainer, sampler, loader, cfg.training.n_critic, cfg.training.n_generator, device,
                        cfg.training.log_every, state, normalised=store is not None,
                        max_iters=args.max_iters if store is not None else None,
                        fid_every=fid_every, evaluate=None if evaluator is None else (lambda it, e=epoch: evaluator(e, it)))
        if evaluator is not None and fid_epoch is not None and epoch % fid_epoch == 0:
            evaluator(epoch, state["i_iter"])           # the sampler as it stands after this epoch
        if args.max_iters is not None and state["i_iter"] >= args.max_iters:
            break
    if store is not None:
        store.close()
    if local_rank == 0:
        save_model(trainer, logdir, "last", d_other_info={"epoch": epoch, "iter": state["i_iter"], "fid": None})
        print0(f"saved {logdir}/sampler_last.pth and value_last.pth after {state['i_iter']} iterations")


if __name__ == "__main__":
    main()
