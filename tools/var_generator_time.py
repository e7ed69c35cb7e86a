"""Time VARSampler.sample with batch- and rank-invariant noise on the CIFAR-10 T = 10 sampler (synthetic weights), on one
GPU, in one process:

    python tools/var_generator_time.py [--batch 256] [--calls 20] [--warmup 3] [--out FILE]

  generator   sample(B, generator=g), g a DeterministicGenerator: the draws are made inside the transition launches
              (dxmi_var_step_fwd_indexed) and the whole T-step loop replays from one hipGraph;
  injected    the only way to the same images without generator=: Z = [g.randn(size)] x (T + 1) (dxmi_randn_indexed launches), then
              sample(B, noise=Z), which no graph replays (noise= runs eagerly);
  default     sample(B): torch's device draws, the loop replayed from one hipGraph.
Every mode runs --warmup calls (a replayed mode's include its eager call and its capture), then the modes ALTERNATE call by call for
--calls timed calls each; a call is timed by the host clock with a synchronise at both ends and set_done_samples(0) before it.
Reported: ms per call as the median with the min and max.  Every call runs under a watchdog (status 124 on an overrun).  Prints one
JSON line."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))

import torch  # noqa: E402


def _overrun():
    sys.stderr.write("var_generator_time: a call overran its time limit\n")
    sys.stderr.flush()
    os._exit(124)


def guarded(fn, limit):
    dog = threading.Timer(limit, _overrun)
    dog.daemon = True
    dog.start()
    try:
        return fn()
    finally:
        dog.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--call_timeout", type=int, default=120)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import configs_builtin
    import dxmi_config
    from dxmi_hip import ops
    from models.cm.random_util import get_generator
    ops.device_check()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = configs_builtin.get("cifar10_T10")
    sampler = dxmi_config.instantiate(cfg.sampler, net=dxmi_config.instantiate(cfg.sampler_net)).to(dev).eval()
    B, T = args.batch, sampler.n_timesteps
    size = (B,) + tuple(sampler.sample_shape)
    gen = get_generator("determ", 1 << 20, 0)

    def generator():
        sampler.use_graph = True
        gen.set_done_samples(0)
        return sampler.sample(B, device=dev, generator=gen)["sample"]

    def injected():
        sampler.use_graph = False
        gen.set_done_samples(0)
        return sampler.sample(B, device=dev, noise=[gen.randn(size, device=dev) for _ in range(T + 1)])["sample"]

    def default():
        sampler.use_graph = True
        return sampler.sample(B, device=dev)["sample"]

    modes = {"generator": generator, "injected": injected, "default": default}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for fn in modes.values():
        for _ in range(args.warmup):
            guarded(lambda: timed(fn), args.call_timeout)
    with torch.no_grad():
        same = torch.equal(generator().clone(), injected())
    ms = {k: [] for k in modes}
    for _ in range(args.calls):
        for k, fn in modes.items():
            ms[k].append(guarded(lambda: timed(fn), args.call_timeout))
    out = {"batch": B, "T": T, "calls": args.calls, "device": torch.cuda.get_device_name(0), "generator_equals_injected": same,
           "captures": {str(k): g.captures for k, g in sampler._graphs.items()}}
    for k, v in ms.items():
        out[f"{k}_ms"] = round(statistics.median(v), 4)
        out[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
