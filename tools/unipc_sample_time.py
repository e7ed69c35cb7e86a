"""Time dxmi_unipc_stage and dxmi_edm_unipc_stage (UniPC, models/DxMI/unipc_sample.py and models/cm/unipc_sample.py) beside
dxmi_dpm_stage and dxmi_edm_dpm_stage, and one replayed unipc_sample / edm_unipc_sample call beside the DPM-Solver++ call at equal
steps, on one GPU, in one process.

    python tools/unipc_sample_time.py [--shapes 256x32,100x64,16x256] [--reps 200] [--rounds 5] [--steps 10] [--windows 3]
                                      [--warmup 2] [--no_loop] [--out FILE]

The launches, for every N x size in --shapes on fp32 [N, 3, size, size]: device time by events around --reps back-to-back calls, the
four launches ALTERNATING round by round, the median of --rounds rounds after a warm-up round, with min - max.  Every launch runs
row 5 of a 10-step order-3 schedule.  Bytes are counted from the shapes:
  unipc_stage      an order-3 row with an order-3 corrector: reads x, eps, xc, D1, D2, D3, writes x, xc and one slot     36 B per element
  dpm_stage        an order-3 ODE row: reads x, eps, D1, D2, writes x and one slot                                       24 B per element
  edm_unipc_stage  the same with the second output stream x_in                                                           40 B per element
  edm_dpm_stage    an order-3 ODE row: reads x, F, D1, D2, writes x, x_in and one slot                                   28 B per element
Reported per launch: microseconds, achieved bytes/s and, for the two new launches, their time over their DPM-Solver++ neighbour's
next to the byte ratios 1.5 and 1.43.  The loops (--no_loop skips them): the CIFAR-10 teacher U-Net at batch 256 (synthetic
weights) with unipc_sample and dpm_sample(order 3), and the ImageNet-64 U-Net of configs_builtin (synthetic weights, fp16 as the
config says) at batch 100, labels given, with edm_unipc_sample and edm_dpm_sample(order 3); all at --steps steps, use_graph=True,
--warmup calls each (captures included), then --windows timed calls each, alternating; a call is timed by the host clock with a
synchronise at both ends.  Every round and window runs under a watchdog (status 124 on an overrun).  Prints one JSON line.
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

BYTES = {"unipc_stage": 36, "dpm_stage": 24, "edm_unipc_stage": 40, "edm_dpm_stage": 28}
NET = dict(ch=128, out_ch=3, ch_mult=(1, 2, 2, 2), num_res_blocks=2, attn_resolutions=[16], dropout=0.1, in_channels=3, resolution=32)
ROW = 5


def _overrun():
    sys.stderr.write("unipc_sample_time: a window overran its time limit\n")
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


def measure_launches(N, size, reps, rounds, dev):
    from dxmi_hip import ops
    from models.cm.dpm_sample import edm_dpm_schedule
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.unipc_sample import edm_unipc_schedule
    from models.DxMI.dpm_sample import dpm_sample_schedule
    from models.DxMI.unipc_sample import unipc_sample_schedule
    device = torch.device(dev)
    diffusion = KarrasDenoiser()
    uni, dpm = unipc_sample_schedule(10, 3), dpm_sample_schedule(10, 3)
    euni, edm = edm_unipc_schedule(diffusion, 10, 3), edm_dpm_schedule(diffusion, 10, 3)
    assert uni.table[ROW, ops.UT_ORDER] == 3 and uni.table[ROW, ops.UT_CORDER] == 3 and uni.table[ROW, ops.UT_CV3] != 0
    assert euni.table[ROW, ops.EUT_ORDER] == 3 and euni.table[ROW, ops.EUT_CORDER] == 3 and euni.table[ROW, ops.EUT_CV3] != 0
    assert dpm.table[ROW, ops.MT_ORDER] == 3 and dpm.table[ROW, ops.MT_S] == 0 and edm.table[ROW, ops.ET_ORDER] == 3
    utab, dtab, eutab, etab = (s.device_table(device) for s in (uni, dpm, euni, edm))
    shape = (N, 3, size, size)
    x, F, y, xc = (torch.randn(shape, device=dev) for _ in range(4))
    hist = torch.randn((4,) + shape, device=dev).clamp_(-1, 1)
    out, x_in, t = torch.empty_like(x), torch.empty_like(x), torch.empty(N, device=dev)
    calls = {"unipc_stage": lambda: ops.unipc_stage(ops.UNIPC_STEP, utab, t, row=ROW, x=x, xc=xc, eps=F, hist=hist, out=out),
             "dpm_stage": lambda: ops.dpm_stage(ops.DPM_STEP, dtab, t, row=ROW, x=x, eps=F, hist=hist[:3], out=out),
             "edm_unipc_stage": lambda: ops.edm_unipc_stage(ops.EDM_UNIPC_STEP, eutab, t, row=ROW, x=x, xc=xc, model_out=F, hist=hist,
                                                            x_in=x_in, out=out),
             "edm_dpm_stage": lambda: ops.edm_dpm_stage(ops.EDM_DPM_STEP, etab, t, row=ROW, x=x, model_out=F, hist=hist[:3], x_in=x_in,
                                                        out=out)}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {k: [] for k in calls}
    for r in range(rounds + 1):
        for name, fn in calls.items():
            x.copy_(y)                       # the stages update x and xc in place: every round starts from the same state
            xc.copy_(y)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                us[name].append(a.elapsed_time(b) * 1e3 / reps)
    elements = x.numel()
    res = {"elements": elements}
    for name, v in us.items():
        m = statistics.median(v)
        res[f"{name}_us"] = round(m, 3)
        res[f"{name}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        res[f"{name}_GBps"] = round(BYTES[name] * elements / (m * 1e-6) / 1e9, 1)
    for new, old in (("unipc_stage", "dpm_stage"), ("edm_unipc_stage", "edm_dpm_stage")):
        res[f"{new}_over_{old}_time"] = round(res[f"{new}_us"] / res[f"{old}_us"], 3)
        res[f"{new}_over_{old}_bytes"] = round(BYTES[new] / BYTES[old], 3)
    return res


def measure_loops(args, dev):
    import configs_builtin
    from models.cm.dpm_sample import edm_dpm_sample
    from models.cm.script_util import create_model_and_diffusion
    from models.cm.unipc_sample import edm_unipc_sample
    from models.DxMI.dpm_sample import dpm_sample
    from models.DxMI.unet_small import Model
    from models.DxMI.unipc_sample import unipc_sample
    torch.manual_seed(0)
    teacher = Model(**NET).to(dev).eval()
    cfg = configs_builtin.get("imagenet64_T10")
    net, diffusion = create_model_and_diffusion(**cfg.diffusion)
    net.to(dev)
    if cfg.diffusion.use_fp16:
        net.convert_to_fp16()
    net.eval()
    small, large = (256, 3, 32, 32), (100, 3, 64, 64)
    y = torch.randint(0, net.num_classes, (large[0],), device=dev)
    edm_kw = dict(steps=args.steps, order=3, model_kwargs={"y": y}, device=dev, sigma_min=diffusion.sigma_min,
                  sigma_max=diffusion.sigma_max, use_graph=True)
    runs = {"unipc_sample": lambda: unipc_sample(teacher, small, steps=args.steps, order=3, device=dev, use_graph=True),
            "dpm_sample": lambda: dpm_sample(teacher, small, steps=args.steps, order=3, device=dev, use_graph=True),
            "edm_unipc_sample": lambda: edm_unipc_sample(diffusion, net, large, **edm_kw),
            "edm_dpm_sample": lambda: edm_dpm_sample(diffusion, net, large, **edm_kw)}

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for fn in runs.values():
        for _ in range(args.warmup):
            guarded(lambda: window(fn), args.window_timeout)
    ms = {k: [] for k in runs}
    for _ in range(args.windows):
        for k, fn in runs.items():
            ms[k].append(guarded(lambda: window(fn), args.window_timeout))
    out = {"teacher_shape": list(small), "edm_shape": list(large), "nfe": args.steps}
    for k, v in ms.items():
        out[f"{k}_ms_per_call"] = round(statistics.median(v), 2)
        out[f"{k}_ms_per_call_min_max"] = [round(min(v), 2), round(max(v), 2)]
    out["unipc_over_dpm_sample"] = round(out["unipc_sample_ms_per_call"] / out["dpm_sample_ms_per_call"], 4)
    out["edm_unipc_over_edm_dpm_sample"] = round(out["edm_unipc_sample_ms_per_call"] / out["edm_dpm_sample_ms_per_call"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x32,100x64,16x256")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no_loop", action="store_true")
    ap.add_argument("--window_timeout", type=int, default=180)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from dxmi_hip import ops
    ops.device_check()
    dev = "cuda:0"
    out = {"reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for spec in args.shapes.split(","):
        N, size = (int(v) for v in spec.split("x"))
        out[f"launches_{spec}"] = guarded(lambda: measure_launches(N, size, args.reps, args.rounds, dev), args.window_timeout)
        sys.stderr.write(f"unipc_sample_time: {spec} {json.dumps(out[f'launches_{spec}'])}\n")
        sys.stderr.flush()
        torch.cuda.empty_cache()
    if not args.no_loop:
        out["loops"] = measure_loops(args, dev)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
