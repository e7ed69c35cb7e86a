"""Time one draw of the deterministic generators (dxmi_randn_indexed) against the draw it replaces, on one GPU.

    python tools/randn_indexed_time.py [--batch 100] [--calls 200] [--timeout 60]

At [batch, 3, 64, 64], the mean of --calls back-to-back calls after 20 warm-up calls (device events, a synchronise at the end):
  launch      ops.randn_indexed into a given buffer: the kernel and its ctypes call
  generator   DeterministicIndividualGenerator.randn_like: the same plus the index cache, the draw counter and the allocation
  randint     ops.randint_indexed of [batch] labels
  torch       x.normal_() on the implicit device generator: what generator=None (the `dummy` path) does per draw
A draw sits between two network evaluations of ~8 ms at this shape; no floor is quoted, the kernel is ALU-bound.  Every timing
runs under its own time limit, kept by a watchdog thread: an overrun ends the script with status 124.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))

import torch  # noqa: E402


def _overrun():
    sys.stderr.write("randn_indexed_time: a timing overran its time limit\n")
    sys.stderr.flush()
    os._exit(124)


def timed(fn, limit, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dog = threading.Timer(limit, _overrun)
    dog.daemon = True
    dog.start()
    try:
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
    finally:
        dog.cancel()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)      # generate_large.py's default per-rank batch
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=60)
    args = ap.parse_args()
    from dxmi_hip import ops
    from models.cm.random_util import get_generator
    ops.device_check()
    dev, B = "cuda:0", args.batch
    shape = (B, 3, 64, 64)
    x = torch.empty(shape, device=dev)
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    gen = get_generator("determ-indiv", 50000, seed=0)
    draw = [0]

    def launch():
        draw[0] += 1
        ops.randn_indexed(idx, shape[1:], 0, draw[0], out=x)

    def labels():
        draw[0] += 1
        ops.randint_indexed(idx, (), 0, 1000, 0, draw[0])
    legs = {"launch": launch, "generator": lambda: gen.randn_like(x), "randint": labels, "torch": lambda: x.normal_()}
    out = {"batch": B, "shape": list(shape), "calls": args.calls}
    for k, fn in legs.items():
        timed(fn, args.timeout, 20)
        out[f"{k}_us"] = round(timed(fn, args.timeout, args.calls) * 1e3, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
