"""Time a consistency-distillation (CD) and a consistency-training (CT) step of the full-size ImageNet-64 U-Net (295.9 M
parameters, synthetic weights) against the sum of their parts, on one GPU, in one process.

    python tools/cm_train_time.py [--batch 16] [--reps 3] [--warmup 2] [--leg_timeout 120] [--launches_only]

Legs, alternating, median of --reps after --warmup rounds (device events around each leg, a synchronise at its end):
  cd    one CMTrainLoop.run_step, consistency_distillation: online forward + backward, two teacher and one target evaluation
  ct    one CMTrainLoop.run_step, consistency_training: online forward + backward, one target evaluation
  dsm   one TrainLoop.run_step (the DSM step of the EDM teacher), same net and batch
  inf   one forward_inference of the same net and batch
Ratios: cd / (dsm + 3 inf) and ct / (dsm + inf): the consistency launches and the target EMA are all a step adds to its parts.
Then every consistency launch alone at the same batch (mean of 200 back-to-back launches) next to its HBM floor, bytes / 8 TB/s.
Every leg runs under its own time limit, kept by a watchdog thread that needs no turn of the interpreter's main thread (a leg
stuck inside a device call is ended too): an overrun ends the script with status 124, and any failure ends it at once.  Prints
one JSON line for the legs and one for the launches.
"""
import argparse
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))

import torch  # noqa: E402

MODEL = dict(image_size=64, class_cond=True, learn_sigma=False, num_channels=192, num_res_blocks=3, channel_mult="", num_heads=4,
             num_head_channels=64, num_heads_upsample=-1, attention_resolutions="32,16,8", dropout=0.0, use_checkpoint=False,
             use_scale_shift_norm=True, resblock_updown=True, use_fp16=True, use_new_attention_order=False, weight_schedule="uniform")


def _overrun():
    sys.stderr.write("cm_train_time: a leg overran its time limit\n")
    sys.stderr.flush()
    os._exit(124)


def timed(fn, limit, reps=1):
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


def launch_times(ops, B, dev, limit):
    """us per launch of every consistency kernel at [B, 3, 64, 64], with its HBM floor (bytes / 8 TB/s)."""
    from models.cm.karras_diffusion import cd_levels
    shape, n = (B, 3, 64, 64), B * 3 * 64 * 64
    r = lambda: torch.randn(shape, device=dev)
    x0, noise, F1, F2, Fs, Ft = r(), r(), r(), r(), r(), r()
    tab = cd_levels(40, 0.002, 80.0, 7.0).device_table(dev)
    idx = torch.randint(0, 39, (B,), device=dev)
    g = torch.ones(B, device=dev)
    x_t, _, _, _ = ops.cd_prep(x0, noise, idx, tab)
    d, smp, _, _ = ops.cd_solver(ops.CD_HEUN_PRED, x_t, idx, tab, model_out=F1)
    x_t2, _, _ = ops.cd_solver(ops.CD_HEUN_CORR, x_t, idx, tab, model_out=F2, d=d, samples=smp)
    cases = {"prep": (16, lambda: ops.cd_prep(x0, noise, idx, tab)),
             "solver_euler_x0": (16, lambda: ops.cd_solver(ops.CD_EULER_X0, x_t, idx, tab, x_start=x0)),
             "solver_heun_pred": (20, lambda: ops.cd_solver(ops.CD_HEUN_PRED, x_t, idx, tab, model_out=F1)),
             "solver_heun_corr": (24, lambda: ops.cd_solver(ops.CD_HEUN_CORR, x_t, idx, tab, model_out=F2, d=d, samples=smp))}
    for norm in ("l1", "l2", "l2-32"):
        cases[f"loss_fwd_{norm}"] = (16, lambda norm=norm: ops.cd_loss_fwd(Fs, Ft, x_t, x_t2, idx, tab, norm, "uniform", distillation=True))
        cases[f"loss_bwd_{norm}"] = (20, lambda norm=norm: ops.cd_loss_bwd(g, Fs, Ft, x_t, x_t2, idx, tab, norm, "uniform", distillation=True))
    # the pseudo-Huber pair of improved consistency training: the l2 stream plus one [B] vector (ssq) written / read
    hc = 0.00054 * (3 * 64 * 64) ** 0.5
    _, ssq = ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx, tab, hc, "ict", distillation=True)
    cases["huber_fwd"] = (16, lambda: ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx, tab, hc, "ict", distillation=True))
    cases["huber_bwd"] = (20, lambda: ops.cd_huber_bwd(g, ssq, Fs, Ft, x_t, x_t2, idx, tab, hc, "ict", distillation=True))
    out = {}
    for k, (bytes_per, fn) in cases.items():
        timed(fn, limit, 20)
        out[k] = {"us": round(timed(fn, limit, 200) * 1e3, 2), "floor_us": round(bytes_per * n / 8e12 * 1e6, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)      # train_image_large.py's per-rank batch at 8 GPUs
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg_timeout", type=int, default=120)
    ap.add_argument("--launches_only", action="store_true", help="skip the step legs: only the per-launch times")
    args = ap.parse_args()
    from dxmi_hip import ops
    if args.launches_only:
        ops.device_check()
        print(json.dumps({"launches_us": launch_times(ops, args.batch, "cuda:0", args.leg_timeout)}), flush=True)
        return
    from models.cm.resample import LogNormalSampler
    from models.cm.script_util import create_ema_and_scales_fn, create_model_and_diffusion
    from models.cm.train_util import CMTrainLoop, TrainLoop
    ops.device_check()
    dev, B = "cuda:0", args.batch
    torch.manual_seed(0)

    def net(distillation=False):
        m, d = create_model_and_diffusion(**dict(MODEL, distillation=distillation))
        return m.to(dev), d

    common = dict(data=None, batch_size=B, microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=10 ** 9, save_interval=10 ** 9,
                  resume_checkpoint="", use_fp16=True, log_dir=os.path.join(ROOT, "results", "cm_train_time"))
    scales = create_ema_and_scales_fn("fixed", 0.95, "fixed", 40, 40, 10 ** 6, 50000)
    teacher, teacher_diffusion = net()
    loops = {}
    for mode, key in (("consistency_distillation", "cd"), ("consistency_training", "ct")):
        online, student = net(True)
        target, _ = net(True)
        student.loss_norm = "l2"
        loops[key] = CMTrainLoop(model=online.train(), diffusion=student, target_model=target, teacher_model=teacher if key == "cd" else None,
                                 teacher_diffusion=teacher_diffusion if key == "cd" else None, training_mode=mode, ema_scale_fn=scales,
                                 total_training_steps=10 ** 6, **common)
    dsm_net, dsm_diffusion = net()
    loops["dsm"] = TrainLoop(model=dsm_net.train(), diffusion=dsm_diffusion, schedule_sampler=LogNormalSampler(), **common)
    x0 = torch.rand(B, 3, 64, 64, device=dev) * 2 - 1
    cond = {"y": torch.randint(0, 1000, (B,), device=dev)}
    t_in = torch.full((B,), 100.0, device=dev)
    legs = {"cd": lambda: loops["cd"].run_step(x0, cond), "ct": lambda: loops["ct"].run_step(x0, cond),
            "dsm": lambda: loops["dsm"].run_step(x0, cond), "inf": lambda: teacher.forward_inference(x0, t_in, cond["y"])}
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.reps):
        for k, fn in legs.items():
            ms = timed(fn, args.leg_timeout)
            if r >= args.warmup:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"batch": B, "reps": args.reps}
    out.update({f"{k}_ms": round(v, 3) for k, v in med.items()})
    out.update({f"{k}_ms_all": [round(x, 3) for x in v] for k, v in times.items()})
    out["cd_over_parts"] = round(med["cd"] / (med["dsm"] + 3 * med["inf"]), 4)
    out["ct_over_parts"] = round(med["ct"] / (med["dsm"] + med["inf"]), 4)
    print(json.dumps(out), flush=True)
    print(json.dumps({"batch": B, "launches": launch_times(ops, B, dev, args.leg_timeout)}), flush=True)


if __name__ == "__main__":
    main()
