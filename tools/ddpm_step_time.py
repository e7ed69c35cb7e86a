"""Time DDPMTrainLoop.run_step eagerly and replayed from hipGraphs (use_graph=True) on the full CIFAR-10 DDPM U-Net (35.7 M
parameters, dropout 0.1, synthetic images), on one GPU, in one process; and the three dxmi_ddpm_* launches beside a plain copy of the
same bytes.

    python tools/ddpm_step_time.py [--batches 128,32] [--steps 8] [--windows 5] [--warmup 3] [--out FILE]

Per batch size two loops are built from the same seed, one eager and one with use_graph=True.  Both run --warmup steps (the replayed
loop's include its eager call and its capture), then --windows timed windows of --steps run_step calls each, the two loops
ALTERNATING window by window; a window is timed by the host clock with a synchronise at both ends (run_step reads nothing back).
Reported: steps/s of either loop as the median over windows with the min and max, replay over eager and the per-step time the replay
removes.  The launches: device time by events around --reps back-to-back calls (median of 5 such rounds, after a warm-up round), for
[B, 3, 32, 32]; `copy` is x.copy_(y) of one such tensor (one read, one write: prep reads two tensors and writes one, loss_fwd reads
two, loss_bwd reads two and writes one).  Every window runs under a watchdog (status 124 on an overrun).  Prints one JSON line.
"""
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

NET = dict(ch=128, out_ch=3, ch_mult=(1, 2, 2, 2), num_res_blocks=2, attn_resolutions=[16], dropout=0.1, in_channels=3, resolution=32)


def _overrun():
    sys.stderr.write("ddpm_step_time: a window overran its time limit\n")
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


def build_loop(use_graph, B, dev):
    from models.DxMI.ddpm_train import DDPMSchedule, DDPMTrainLoop
    from models.DxMI.unet_small import Model
    torch.manual_seed(0)
    net = Model(**NET).to(dev).train()
    return DDPMTrainLoop(model=net, schedule=DDPMSchedule(), data=None, batch_size=B, log_interval=10 ** 9, save_interval=10 ** 9,
                         log_dir=os.path.join(ROOT, "results", "ddpm_step_time"), use_graph=use_graph)


def window(loop, x0, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loop.run_step(x0)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def measure_steps(B, args, dev):
    x0 = torch.rand(B, 3, 32, 32, device=dev) * 2 - 1
    loops = {"eager": build_loop(False, B, dev), "replay": build_loop(True, B, dev)}
    for loop in loops.values():
        guarded(lambda: window(loop, x0, args.warmup), args.window_timeout)
    rates = {k: [] for k in loops}
    for _ in range(args.windows):
        for k, loop in loops.items():
            rates[k].append(guarded(lambda: window(loop, x0, args.steps), args.window_timeout))
    out = {"captures": loops["replay"].captures, "replays": loops["replay"].replays}
    for k, v in rates.items():
        out[f"{k}_steps_per_s"] = round(statistics.median(v), 3)
        out[f"{k}_steps_per_s_min_max"] = [round(min(v), 3), round(max(v), 3)]
        out[f"{k}_ms_per_step"] = round(1e3 / statistics.median(v), 3)
    e, r = statistics.median(rates["eager"]), statistics.median(rates["replay"])
    out["replay_over_eager"] = round(r / e, 4)
    out["ms_per_step_removed"] = round(1e3 / e - 1e3 / r, 3)
    return out


def measure_launches(B, reps, dev):
    from dxmi_hip import ops
    from models.DxMI.ddpm_train import DDPMSchedule
    tab = DDPMSchedule().device_table(torch.device(dev))
    x0, noise, eps = (torch.randn(B, 3, 32, 32, device=dev) for _ in range(3))
    out_buf, g = torch.empty_like(x0), torch.rand(B, device=dev)
    t = torch.randint(0, 1000, (B,), device=dev)
    calls = {"ddpm_prep": lambda: ops.ddpm_prep(x0, noise, t, tab, out=out_buf), "ddpm_loss_fwd": lambda: ops.ddpm_loss_fwd(eps, noise),
             "ddpm_loss_bwd": lambda: ops.ddpm_loss_bwd(g, eps, noise, out=out_buf), "copy": lambda: out_buf.copy_(x0)}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"bytes_per_tensor": x0.numel() * 4}
    for name, fn in calls.items():
        rounds = []
        for r in range(6):
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                rounds.append(a.elapsed_time(b) * 1e3 / reps)
        res[f"{name}_us"] = round(statistics.median(rounds), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,32")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--window_timeout", type=int, default=180)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from dxmi_hip import ops
    ops.device_check()
    ops.tune_for_throughput()            # as train_ddpm.py runs
    dev = "cuda:0"
    out = {"steps_per_window": args.steps, "windows": args.windows, "device": torch.cuda.get_device_name(0)}
    for B in [int(v) for v in args.batches.split(",")]:
        out[f"launches_b{B}"] = guarded(lambda: measure_launches(B, args.reps, dev), args.window_timeout)
        out[f"b{B}"] = measure_steps(B, args, dev)
        sys.stderr.write(f"ddpm_step_time: B={B} {json.dumps(out[f'b{B}'])} {json.dumps(out[f'launches_b{B}'])}\n")
        sys.stderr.flush()
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
