"""Time what a progressive-distillation (PD) loss step spends outside its network evaluations, on one GPU, in one process.

    python tools/pd_step_time.py [--batch 16] [--reps 5] [--warmup 2] [--leg_timeout 120]

Two measurements at [batch, 3, 64, 64], num_scales 40, norm l2:
  launches  the four non-network launches of the forward of a step (dxmi_cd_prep on the coarse ladder, dxmi_pd_solver MID and END,
            dxmi_pd_loss_fwd), each the mean of 200 back-to-back launches between two device events, next to the reference's torch
            expressions for the same four stages on the same operands, timed the same way (the torch fallback of progdist_losses
            runs exactly these between its network calls);
  step      progdist_losses + backward of loss.mean() on the full-size ImageNet-64 U-Net (295.9 M parameters, synthetic weights,
            dropout 0) as student and as teacher: the device path (one autograd node around the student) against the torch
            fallback on the SAME two HIP nets, which a thin callable around each net selects.  Both run the same network programs
            (training forward + backward of the student, two inference forwards of the teacher); legs alternate, median of --reps
            after --warmup rounds, device events around each leg and a synchronise at its end.
Every timed piece runs under its own time limit, kept by a watchdog thread: an overrun ends the script with status 124.  Prints
one JSON line per measurement.
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
             use_scale_shift_norm=True, resblock_updown=True, use_fp16=True, use_new_attention_order=False, weight_schedule="karras")
S = 40


def _overrun():
    sys.stderr.write("pd_step_time: a timed piece overran its time limit\n")
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


def launch_times(ops, diffusion, B, dev, limit):
    """us per stage at [B, 3, 64, 64]: the HIP launch and the reference's torch expressions for it."""
    from models.cm.karras_diffusion import pd_levels
    from models.cm.nn import append_dims, mean_flat
    shape = (B, 3, 64, 64)
    r = lambda: torch.randn(shape, device=dev)
    x0, noise, F1, F2, Fs = r(), r(), r(), r(), r()
    lv = pd_levels(S, 0.002, 80.0, 7.0)
    tab = lv.device_table(torch.device(dev))
    idx = torch.randint(0, S, (B,), device=dev)
    t, t2, t3 = lv.levels(idx)
    e = lambda v: append_dims(v, 4)
    x_t, _, _, _ = ops.cd_prep(x0, noise, idx, tab[:S + 1])
    x_t2, _, _ = ops.pd_solver(ops.PD_MID, x_t, F1, idx, tab)
    target = ops.pd_solver(ops.PD_END, x_t, F2, idx, tab, x_t2=x_t2)
    d = diffusion

    def torch_prep():
        xt = x0 + noise * e(t)
        return e(d.get_scalings(t)[2]) * xt, 1000 * 0.25 * torch.log(t + 1e-44)

    def torch_euler(x, F, s, nxt):
        c_skip, c_out, _ = [e(v) for v in d.get_scalings(s)]
        den = c_out * F + c_skip * x
        return x + (x - den) / e(s) * e(nxt - s)

    def torch_mid():
        x2 = torch_euler(x_t, F1, t, t2)
        return e(d.get_scalings(t2)[2]) * x2, 1000 * 0.25 * torch.log(t2 + 1e-44)

    def torch_end():
        x3 = torch_euler(x_t2, F2, t2, t3)
        return x_t - e(t) * (x3 - x_t) / e(t3 - t)

    def torch_loss():
        c_skip, c_out, _ = [e(v) for v in d.get_scalings(t)]
        return mean_flat((c_out * Fs + c_skip * x_t - target) ** 2) * (t ** -2 + 1.0 / d.sigma_data ** 2)

    cases = {"prep": (lambda: ops.cd_prep(x0, noise, idx, tab[:S + 1]), torch_prep),
             "solver_mid": (lambda: ops.pd_solver(ops.PD_MID, x_t, F1, idx, tab), torch_mid),
             "solver_end": (lambda: ops.pd_solver(ops.PD_END, x_t, F2, idx, tab, x_t2=x_t2), torch_end),
             "loss_fwd": (lambda: ops.pd_loss_fwd(Fs, x_t, target, idx, tab, "l2", "karras"), torch_loss)}
    out = {}
    for name, (hip, th) in cases.items():
        for fn in (hip, th):
            timed(fn, limit, 20)
        out[name] = {"hip_us": round(timed(hip, limit, 200) * 1e3, 2), "torch_us": round(timed(th, limit, 200) * 1e3, 2)}
    out["sum"] = {k: round(sum(v[k] for v in out.values()), 2) for k in ("hip_us", "torch_us")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)      # the per-rank batch of the ImageNet-64 runs at 8 GPUs
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg_timeout", type=int, default=120)
    args = ap.parse_args()
    from dxmi_hip import ops
    from models.cm.script_util import create_model_and_diffusion
    ops.device_check()
    dev, B = "cuda:0", args.batch
    torch.manual_seed(0)
    online, student = create_model_and_diffusion(**MODEL)
    teacher, teacher_diffusion = create_model_and_diffusion(**MODEL)
    online, teacher = online.to(dev).train(), teacher.to(dev).eval().requires_grad_(False)
    student.loss_norm = "l2"
    print(json.dumps({"batch": B, "num_scales": S, "launches": launch_times(ops, student, B, dev, args.leg_timeout)}), flush=True)

    x0 = torch.rand(B, 3, 64, 64, device=dev) * 2 - 1
    noise = torch.randn(B, 3, 64, 64, device=dev)
    idx = torch.randint(0, S, (B,), device=dev)
    kw = {"y": torch.randint(0, 1000, (B,), device=dev)}
    as_callable = lambda net: (lambda x, t, **k: net(x, t, **k))      # no UNetModel: progdist_losses takes its torch path

    def leg(model, tch):
        def run():
            for p in online.parameters():
                p.grad = None
            loss = student.progdist_losses(model, x0, S, model_kwargs=kw, teacher_model=tch, teacher_diffusion=teacher_diffusion,
                                           noise=noise, indices=idx)["loss"]
            loss.mean().backward()
            return loss
        return run
    legs = {"device": leg(online, teacher), "torch": leg(as_callable(online), as_callable(teacher))}
    times = {k: [] for k in legs}
    losses = {}
    for r in range(args.warmup + args.reps):
        for k, fn in legs.items():
            ms = timed(lambda: losses.__setitem__(k, fn()), args.leg_timeout)
            if r >= args.warmup:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    rel = ((losses["device"].detach() - losses["torch"].detach()).abs() / losses["torch"].detach().abs()).max().item()
    out = {"batch": B, "reps": args.reps, "num_scales": S}
    out.update({f"{k}_ms": round(v, 3) for k, v in med.items()})
    out.update({f"{k}_ms_all": [round(x, 3) for x in v] for k, v in times.items()})
    out["torch_minus_device_ms"] = round(med["torch"] - med["device"], 3)
    out["loss_worst_rel_diff"] = rel
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
