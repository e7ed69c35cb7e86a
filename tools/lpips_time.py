"""Time the LPIPS loss norm on one GPU: every LPIPS launch at the shapes of a B = 16, 64 -> 224 step next to its floor, LPIPS forward
+ backward alone, and the consistency-distillation (CD) / consistency-training (CT) steps of the full-size ImageNet-64 U-Net with
`lpips` next to `l2` (tools/cm_train_time.py's set-up; He-scaled random VGG weights: timing does not depend on their values).

    python tools/lpips_time.py [--batch 16] [--reps 3] [--warmup 2] [--leg_timeout 120] [--no_steps]

Floors: convolutions 2 N h w Cout Cin 9 FLOP over the 2.5 PFLOP/s dense bf16 MFMA peak; every other launch its bytes over 8 TB/s.
A launch row is the mean of 10 back-to-back calls of the Python wrapper between two device events: the wrapper's output allocation
is host work that overlaps the device, so the figure is the device time wherever a launch takes longer than its call (about 10 us);
the smallest rows are bounded by the call, not by the kernel.  Every leg runs under its own time limit (the watchdog of
tools/cm_train_time.py).  Prints one JSON line per table; the first also sums the rows by kind.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
from cm_train_time import MODEL, timed  # noqa: E402

PEAK_FLOPS, HBM = 2.5e15, 8e12


def random_lpips(seed=0):
    from models.cm.lpips import CONV_INDICES, CONV_WIDTHS, TAP_WIDTHS, LPIPS
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for idx, cout in zip(CONV_INDICES, CONV_WIDTHS):
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[f"features.{idx}.bias"] = 0.05 * torch.randn(cout, generator=g)
        cin = cout
    return LPIPS(sd, [0.1 + torch.rand(1, c, 1, 1, generator=g) for c in TAP_WIDTHS])


def launch_table(lp, B, dev, limit):
    from dxmi_hip import lpips_ops as lo
    from dxmi_hip import ops
    from models.cm.lpips import GROUPS
    fw = [ops.gconv_pack(w.to(dev), bias=b) for w, b in lp.convs]
    bw = [ops.gconv_pack(w.to(dev).transpose(0, 1).flip(2, 3)) for w, _ in lp.convs]
    lin = [w.to(dev) for w in lp.lin]
    rows = {}

    def row(name, fn, flops=0.0, nbytes=0.0):
        if name in rows:      # a second layer of the same shape: timed once, counted twice
            rows[name]["per_step"] += 1
            return
        timed(fn, limit, 3)
        us = timed(fn, limit, 10) * 1e3
        floor = max(flops / PEAK_FLOPS, nbytes / HBM) * 1e6
        rows[name] = {"us": round(us, 1), "floor_us": round(floor, 2), "fraction": round(floor / us, 4), "per_step": 1}

    xy = torch.rand(2 * B, 3, 64, 64, device=dev)
    row("front_fwd", lambda: lo.front_fwd(xy, 224), nbytes=xy.numel() * 4 + 2 * B * 224 * 224 * 32)
    h = lo.front_fwd(xy, 224)
    for gi, group in enumerate(GROUPS):
        for l in group:
            pk, hin = fw[l], h
            n, hh, ww, _ = hin.shape
            fl = 2.0 * n * hh * ww * pk.Cout * pk.Cin * 9
            row(f"conv{l}_fwd_{hh}x{pk.Cin}->{pk.Cout}", lambda: ops.gconv(hin, pk, pad=(1, 1), relu=True), flops=fl)
            h = ops.gconv(hin, pk, pad=(1, 1), relu=True)
            gm, pb = h[:B].contiguous(), bw[l]
            out = torch.zeros(B, hh, ww, 16, dtype=torch.bfloat16, device=dev) if l == 0 else None
            row(f"conv{l}_bwd_{hh}x{pk.Cout}->{pk.Cin}", lambda: ops.gconv(gm, pb, pad=(1, 1), relu=False, out=out), flops=fl / 2)
            tap = l == group[-1]      # at a tap the tap gradient is a third stream read
            ga, gb = torch.zeros_like(gm), torch.zeros_like(gm) if tap else None
            row(f"mask_acc_{hh}x{pk.Cout}" + ("_tap" if tap else ""), lambda: lo.relu_mask_acc(ga, gb, gm), nbytes=gm.numel() * (8 if tap else 6))
        a, b, w = h[:B], h[B:], lin[gi]
        row(f"tap{gi}_fwd_{h.shape[1]}x{h.shape[3]}", lambda: lo.tap_fwd(a, b, w), nbytes=h.numel() * 2)
        row(f"tap{gi}_bwd_{h.shape[1]}x{h.shape[3]}", lambda: lo.tap_bwd(None, a, b, w), nbytes=h.numel() * 2 + a.numel() * 2)
        if gi < len(GROUPS) - 1:
            hp = h
            row(f"pool{gi}_fwd_{h.shape[1]}x{h.shape[3]}", lambda: lo.avgpool2x2(hp), nbytes=hp.numel() * 2.5)
            h = lo.avgpool2x2(hp)
            go = h[:B].contiguous()
            row(f"pool{gi}_bwd_{hp.shape[1]}x{h.shape[3]}", lambda: lo.avgpool2x2_bwd(go, hp.shape[1], hp.shape[2]), nbytes=go.numel() * 2 * 5)
    gz = torch.zeros(B, 224, 224, 16, dtype=torch.bfloat16, device=dev)
    row("front_bwd", lambda: lo.front_bwd(gz, 64, 64), nbytes=gz.numel() * 2 + B * 3 * 64 * 64 * 4)
    kinds = {}
    for name, r in rows.items():
        kind = "conv_fwd" if "_fwd_" in name and name.startswith("conv") else "conv_bwd" if name.startswith("conv") else "other"
        kinds[kind] = round(kinds.get(kind, 0.0) + r["us"] * r["per_step"] / 1e3, 3)
    return rows, kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg_timeout", type=int, default=120)
    ap.add_argument("--no_steps", action="store_true")
    args = ap.parse_args()
    from dxmi_hip import ops
    ops.device_check()
    dev, B = "cuda:0", args.batch
    torch.manual_seed(0)
    lp = random_lpips()
    rows, kinds = launch_table(lp, B, dev, args.leg_timeout)
    print(json.dumps({"batch": B, "launches": rows, "sum_ms": kinds}), flush=True)

    x = torch.rand(B, 3, 64, 64, device=dev, requires_grad=True)
    y = torch.rand(B, 3, 64, 64, device=dev)

    def fwd_bwd():
        x.grad = None
        lp(x, y, resize=224).sum().backward()

    legs = {"lpips_fwd": lambda: lp(x.detach(), y, resize=224), "lpips_fwd_bwd": fwd_bwd}
    if not args.no_steps:
        from models.cm.script_util import create_ema_and_scales_fn, create_model_and_diffusion
        from models.cm.train_util import CMTrainLoop

        def net(distillation=False):
            m, d = create_model_and_diffusion(**dict(MODEL, distillation=distillation))
            return m.to(dev), d

        common = dict(data=None, batch_size=B, microbatch=-1, lr=1e-4, ema_rate="0.9999", log_interval=10 ** 9, save_interval=10 ** 9,
                      resume_checkpoint="", use_fp16=True, log_dir=os.path.join(ROOT, "results", "lpips_time"))
        scales = create_ema_and_scales_fn("fixed", 0.95, "fixed", 40, 40, 10 ** 6, 50000)
        teacher, teacher_diffusion = net()
        x0 = torch.rand(B, 3, 64, 64, device=dev) * 2 - 1
        cond = {"y": torch.randint(0, 1000, (B,), device=dev)}
        for mode, key in (("consistency_distillation", "cd"), ("consistency_training", "ct")):
            for norm in ("l2", "lpips"):
                online, student = net(True)
                target, _ = net(True)
                student.loss_norm, student.lpips_loss = norm, lp
                loop = CMTrainLoop(model=online.train(), diffusion=student, target_model=target, teacher_model=teacher if key == "cd" else None,
                                   teacher_diffusion=teacher_diffusion if key == "cd" else None, training_mode=mode, ema_scale_fn=scales,
                                   total_training_steps=10 ** 6, **common)
                legs[f"{key}_{norm}"] = lambda loop=loop: loop.run_step(x0, cond)
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.reps):
        for k, fn in legs.items():
            ms = timed(fn, args.leg_timeout)
            if r >= args.warmup:
                times[k].append(ms)
    out = {"batch": B, "reps": args.reps}
    out.update({f"{k}_ms": round(statistics.median(v), 3) for k, v in times.items()})
    out.update({f"{k}_ms_all": [round(t, 3) for t in v] for k, v in times.items()})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
