"""Time run_step of the consistency and DSM training loops eagerly and replayed from hipGraphs (use_graph=True), on one GPU, in one
process: the full-size ImageNet-64 U-Net (295.9 M parameters, synthetic weights) at the per-rank batch of an 8-GPU run.

    python tools/cm_step_time.py [--batch 16] [--steps 8] [--windows 5] [--warmup 3] [--kinds cd,ct,dsm] [--out profiles/cm_step_time.json]

Per kind (cd: CMTrainLoop consistency_distillation, l2; ct: consistency_training, l2; dsm: TrainLoop) two loops are built from the
same seed, one eager and one with use_graph=True.  Both run --warmup steps (the replayed loop's include its eager call and its
capture), then --windows timed windows of --steps run_step calls each, the two loops ALTERNATING window by window; a window is
timed by the host clock around calls that each end in the step's device read-back, with a synchronise at both ends.  Reported per
kind: steps/s of either loop as the median over windows with the min and max (the spread), replay over eager, the per-step time
the replay removes, and `eager_issue_ms`: the host time the eager loop needs to ISSUE forward_backward (the call returns before
the device has finished: no synchronise inside), next to `eager_fb_device_ms`, the device time of the same launches (events).  Where
the first exceeds the second the step is bound by the host.  Every window runs under a watchdog (status 124 on an overrun).
Prints one JSON line; --out also writes it to a file.
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

MODEL = dict(image_size=64, class_cond=True, learn_sigma=False, num_channels=192, num_res_blocks=3, channel_mult="", num_heads=4,
             num_head_channels=64, num_heads_upsample=-1, attention_resolutions="32,16,8", dropout=0.0, use_checkpoint=False,
             use_scale_shift_norm=True, resblock_updown=True, use_fp16=True, use_new_attention_order=False, weight_schedule="uniform")
MODES = {"cd": "consistency_distillation", "ct": "consistency_training"}


def _overrun():
    sys.stderr.write("cm_step_time: a window overran its time limit\n")
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


def build_loop(kind, use_graph, B, dev, dropout):
    from models.cm.resample import LogNormalSampler
    from models.cm.script_util import create_ema_and_scales_fn, create_model_and_diffusion
    from models.cm.train_util import CMTrainLoop, TrainLoop
    torch.manual_seed(0)

    def net(distillation=False, p=dropout):
        m, d = create_model_and_diffusion(**dict(MODEL, distillation=distillation, dropout=p))
        return m.to(dev), d

    common = dict(data=None, batch_size=B, microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=10 ** 9, save_interval=10 ** 9,
                  resume_checkpoint="", use_fp16=True, log_dir=os.path.join(ROOT, "results", "cm_step_time"), use_graph=use_graph)
    if kind == "dsm":
        m, d = net()
        return TrainLoop(model=m.train(), diffusion=d, schedule_sampler=LogNormalSampler(), **common)
    online, student = net(True)
    target, _ = net(True)
    student.loss_norm = "l2"
    teacher, teacher_diffusion = net(False, 0.0) if kind == "cd" else (None, None)
    return CMTrainLoop(model=online.train(), diffusion=student, target_model=target, teacher_model=teacher,
                       teacher_diffusion=teacher_diffusion, training_mode=MODES[kind],
                       ema_scale_fn=create_ema_and_scales_fn("fixed", 0.95, "fixed", 40, 40, 10 ** 6, 50000),
                       total_training_steps=10 ** 6, **common)


def window(loop, x0, cond, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loop.run_step(x0, cond)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def issue_time(loop, x0, cond, reps):
    """(host ms to issue forward_backward, device ms of its launches), medians over `reps` eager steps."""
    host, device = [], []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        torch.cuda.synchronize()
        a.record()
        t0 = time.perf_counter()
        loop.forward_backward(x0, cond)
        host.append((time.perf_counter() - t0) * 1e3)
        b.record()
        torch.cuda.synchronize()
        device.append(a.elapsed_time(b))
        loop.mp_trainer.optimize(loop.opt)
    return statistics.median(host), statistics.median(device)


def measure(kind, args, dev):
    B = args.batch
    x0 = torch.rand(B, 3, 64, 64, device=dev) * 2 - 1
    cond = {"y": torch.randint(0, 1000, (B,), device=dev)}
    loops = {"eager": build_loop(kind, False, B, dev, args.dropout), "replay": build_loop(kind, True, B, dev, args.dropout)}
    for loop in loops.values():
        guarded(lambda: window(loop, x0, cond, args.warmup), args.window_timeout)
    rates = {k: [] for k in loops}
    for _ in range(args.windows):
        for k, loop in loops.items():
            rates[k].append(guarded(lambda: window(loop, x0, cond, args.steps), args.window_timeout))
    g = loops["replay"]._graph
    out = {"captures": g.captures, "replays": g.replays}
    for k, v in rates.items():
        out[f"{k}_steps_per_s"] = round(statistics.median(v), 4)
        out[f"{k}_steps_per_s_min_max"] = [round(min(v), 4), round(max(v), 4)]
    e, r = statistics.median(rates["eager"]), statistics.median(rates["replay"])
    out["replay_over_eager"] = round(r / e, 4)
    out["ms_per_step_removed"] = round(1e3 / e - 1e3 / r, 3)
    host, device = guarded(lambda: issue_time(loops["eager"], x0, cond, 5), args.window_timeout)
    out["eager_issue_ms"], out["eager_fb_device_ms"] = round(host, 3), round(device, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)        # cm_train.py's per-rank default
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--kinds", default="cd,ct,dsm")
    ap.add_argument("--window_timeout", type=int, default=180)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from dxmi_hip import ops
    ops.device_check()
    dev = "cuda:0"
    out = {"batch": args.batch, "steps_per_window": args.steps, "windows": args.windows, "dropout": args.dropout,
           "device": torch.cuda.get_device_name(0)}
    for kind in args.kinds.split(","):
        if kind not in ("cd", "ct", "dsm"):
            ap.error(f"--kinds: cd, ct, dsm (got {kind!r})")
        out[kind] = measure(kind, args, dev)
        sys.stderr.write(f"cm_step_time: {kind} {json.dumps(out[kind])}\n")      # progress: the result line comes at the end
        sys.stderr.flush()
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
