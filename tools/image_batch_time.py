"""Time the batch launch of the real-image dataset (dxmi_image_batch) at the shapes the programs run, on one GPU.

    python tools/image_batch_time.py [--reps 200] [--host_batches 40]

For 256 x 32 x 32 x 3 (train_cifar10.py), 16 x 64 x 64 x 3 (ImageNet-64) and 8 x 256 x 256 x 3 (LSUN): the mean of --reps back-to-back
ops.image_batch calls (device events around the series) next to its floor, B*H*W*C*5 bytes / 8 TB/s, and next to the same batch
formed by the torch sequence a user would write on the device (index_select, flip of the chosen rows, permute, float, div, sub).
Then what a training step sees of its loader, host time included: us per next() of a device-resident ImageStore with labels against
us per next() of the scripts' synthetic loader (torch.rand * 2 - 1 and torch.randint on the device) at the same batch; the rest of a
step is the same work in both legs.  Then the host-resident mode at the LSUN shape: ms per batch of the background thread's gather
into pinned memory plus the copy, from an ImageStore(resident="host") over a scratch .npy file that the page cache holds (a cold disk
is slower), with the consumer doing nothing else.  Prints one JSON line per shape, per loader comparison and for the host leg."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 8e12
SHAPES = [(256, 32, 32, 3, 1), (16, 64, 64, 3, 0), (8, 256, 256, 3, 0)]      # B, H, W, C, norm (1: TOTENSOR, 0: ADM)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def torch_batch(store, idx, flip, norm):
    u8 = store.index_select(0, idx)
    u8 = torch.where(flip.bool().view(-1, 1, 1, 1), u8.flip(2), u8)
    x = u8.permute(0, 3, 1, 2).float()
    return (x.div(127.5).sub(1) if norm == 0 else x.div(255).mul(2).sub(1)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host_batches", type=int, default=40)
    args = ap.parse_args()
    from dxmi_hip import ops
    from dxmi_hip.data import NORM_ADM, ImageStore
    ops.device_check()
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    for B, H, W, C, norm in SHAPES:
        rows = max(4 * B, 1024)
        store = torch.randint(0, 256, (rows, H, W, C), dtype=torch.uint8, generator=gen).to(dev)
        idx = torch.randperm(rows, generator=gen)[:B].to(dev)
        flip = (torch.rand(B, generator=gen) < 0.5).to(torch.uint8).to(dev)
        out = torch.empty(B, C, H, W, device=dev)
        us = timed(lambda: ops.image_batch(store, idx, flip, norm, out=out), args.reps)
        us_torch = timed(lambda: torch_batch(store, idx, flip, norm), args.reps)
        print(json.dumps({"shape": [B, H, W, C], "norm": "totensor" if norm else "adm", "image_batch_us": round(us, 2),
                          "floor_us": round(B * H * W * C * 5 / HBM * 1e6, 3), "torch_sequence_us": round(us_torch, 2)}), flush=True)

    for B, H, W, C, norm in SHAPES[:2]:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "a.npz")
            rng = np.random.default_rng(1)
            np.savez(path, rng.integers(0, 256, (8 * B, H, W, C), dtype=np.uint8), rng.integers(0, 1000, 8 * B).astype(np.int64))
            st = ImageStore(path, dev, norm, batch_size=B, class_cond=True, resident="device")
        it = st.batches()
        g = torch.Generator(device=dev).manual_seed(0)

        def synthetic():
            return torch.rand(B, C, H, W, device=dev, generator=g) * 2 - 1, torch.randint(0, 1000, (B,), device=dev, generator=g)

        legs = {"store": [], "synthetic": []}
        for _ in range(5):                               # alternating legs, wall clock with a synchronise at each leg's end
            for name, fn in (("store", lambda: next(it)), ("synthetic", synthetic)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                legs[name].append((time.perf_counter() - t0) * 1e6 / args.reps)
        print(json.dumps({"loader_next_us": [B, H, W, C], **{k: [round(v, 1) for v in sorted(vs[2:])] for k, vs in legs.items()}}),
              flush=True)

    B, H, W, C, _ = SHAPES[2]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "lsun.npy")
        np.save(path, np.random.default_rng(0).integers(0, 256, (2048, H, W, C), dtype=np.uint8))
        store = ImageStore(path, dev, NORM_ADM, batch_size=B, resident="host")
        it = store.batches()
        for _ in range(4):
            next(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.host_batches):
            next(it)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.host_batches
        store.close()
    print(json.dumps({"host_resident": [B, H, W, C], "ms_per_batch_gather_copy_launch": round(ms, 3),
                      "bytes_per_batch": B * H * W * C}), flush=True)


if __name__ == "__main__":
    main()
