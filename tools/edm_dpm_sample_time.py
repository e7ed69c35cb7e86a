"""Time dxmi_edm_dpm_stage (DPM-Solver++ on the EDM nets, models/cm/dpm_sample.py) beside dxmi_dpm_stage and the Euler row of
dxmi_karras_stage, and one replayed edm_dpm_sample call beside karras_sample's Heun, on one GPU, in one process.

    python tools/edm_dpm_sample_time.py [--shapes 100x64,16x256] [--reps 200] [--rounds 5] [--steps 10] [--heun_steps 5]
                                        [--windows 3] [--warmup 2] [--no_loop] [--out FILE]

The launches, for every N x size in --shapes on fp32 [N, 3, size, size] (100 x 64 and 16 x 256 are the per-call shapes of the
benchmark's ImageNet-64 and LSUN-256 legs): device time by events around --reps back-to-back calls, the three launches ALTERNATING
round by round, the median of --rounds rounds after a warm-up round.  Bytes are counted from the shapes:
  edm_dpm_stage   an order-2 ODE row: reads x, F, D1, writes x, x_in and one history slot   24 B per element
  dpm_stage       an order-2 ODE row: reads x, eps, D1, writes x and one history slot       20 B per element
  karras_euler    a DXMI_KARRAS_EULER row that is not last: reads x, F, writes x and x_in    16 B per element
Reported per launch: microseconds, achieved bytes/s and, for the new launch, its time over dxmi_dpm_stage's next to the byte ratio
1.2.  The loop (--no_loop skips it): the ImageNet-64 U-Net of configs_builtin (synthetic weights, fp16 as the config says), batch
100, labels given; edm_dpm_sample(steps = --steps, order 2, use_graph=True) and karras_sample(heun, --heun_steps steps: 2 steps - 1
evaluations, use_graph=True) run --warmup calls each (captures included), then --windows timed calls each, alternating; a call is
timed by the host clock with a synchronise at both ends.  Every round and window runs under a watchdog (status 124 on an overrun).
Prints one JSON line.
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

BYTES = {"edm_dpm_stage": 24, "dpm_stage": 20, "karras_euler": 16}


def _overrun():
    sys.stderr.write("edm_dpm_sample_time: a window overran its time limit\n")
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
    from models.cm.karras_diffusion import KarrasDenoiser, KarrasSchedule, get_sigmas_karras
    from models.DxMI.dpm_sample import dpm_sample_schedule
    device = torch.device(dev)
    diffusion = KarrasDenoiser()
    edm, dpm = edm_dpm_schedule(diffusion, 10, 2), dpm_sample_schedule(10, 2)
    euler = KarrasSchedule(get_sigmas_karras(10, 0.002, 80.0), "euler", diffusion)
    row = 4
    assert edm.table[row, ops.ET_ORDER] == 2 and edm.table[row, ops.ET_W2] == 0 and edm.table[row, ops.ET_S] == 0
    assert dpm.table[row, ops.MT_ORDER] == 2 and dpm.table[row, ops.MT_W2] == 0 and dpm.table[row, ops.MT_S] == 0
    assert euler.launches[row + 1]["mode"] == ops.KARRAS_EULER and not euler.launches[row + 1]["last"]
    etab, dtab, ktab = edm.device_table(device), dpm.device_table(device), euler.device_table(device)
    shape = (N, 3, size, size)
    x, F, y = (torch.randn(shape, device=dev) for _ in range(3))
    hist = torch.randn((3,) + shape, device=dev).clamp_(-1, 1)
    out, x_in, t = torch.empty_like(x), torch.empty_like(x), torch.empty(N, device=dev)
    calls = {"edm_dpm_stage": lambda: ops.edm_dpm_stage(ops.EDM_DPM_STEP, etab, t, row=row, x=x, model_out=F, hist=hist, x_in=x_in, out=out),
             "dpm_stage": lambda: ops.dpm_stage(ops.DPM_STEP, dtab, t, row=row, x=x, eps=F, hist=hist, out=out),
             "karras_euler": lambda: ops.karras_stage(ops.KARRAS_EULER, False, ktab, row + 1, x, model_out=F, x_in=x_in, t=t)}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {k: [] for k in calls}
    for r in range(rounds + 1):
        for name, fn in calls.items():
            x.copy_(y)                       # the stages update x in place: every round starts from the same state
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
    res["edm_over_dpm_stage_time"] = round(res["edm_dpm_stage_us"] / res["dpm_stage_us"], 3)
    res["edm_over_dpm_stage_bytes"] = BYTES["edm_dpm_stage"] / BYTES["dpm_stage"]
    return res


def measure_loop(args, dev):
    import configs_builtin
    from models.cm.dpm_sample import edm_dpm_sample, replay_graphs
    from models.cm.karras_diffusion import karras_nfe, karras_sample
    from models.cm.script_util import create_model_and_diffusion
    cfg = configs_builtin.get("imagenet64_T10")
    torch.manual_seed(0)
    net, diffusion = create_model_and_diffusion(**cfg.diffusion)
    net.to(dev)
    if cfg.diffusion.use_fp16:
        net.convert_to_fp16()
    net.eval()
    shape = (100, 3, 64, 64)
    y = torch.randint(0, net.num_classes, (shape[0],), device=dev)
    runs = {"edm_dpm_sample": lambda: edm_dpm_sample(diffusion, net, shape, steps=args.steps, order=2, model_kwargs={"y": y}, device=dev,
                                                     sigma_min=diffusion.sigma_min, sigma_max=diffusion.sigma_max, use_graph=True),
            "karras_heun": lambda: karras_sample(diffusion, net, shape, args.heun_steps, model_kwargs={"y": y}, device=dev,
                                                 sigma_min=diffusion.sigma_min, sigma_max=diffusion.sigma_max, sampler="heun",
                                                 use_graph=True)}

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
    graphs = replay_graphs(net)
    out = {"shape": list(shape), "edm_dpm_nfe": args.steps, "heun_nfe": karras_nfe("heun", args.heun_steps),
           "edm_dpm_captures": sum(g.captures for g in graphs), "edm_dpm_replays": sum(g.replays for g in graphs)}
    for k, v in ms.items():
        out[f"{k}_ms_per_call"] = round(statistics.median(v), 2)
        out[f"{k}_ms_per_call_min_max"] = [round(min(v), 2), round(max(v), 2)]
    out["edm_dpm_ms_per_nfe"] = round(out["edm_dpm_sample_ms_per_call"] / args.steps, 2)
    out["heun_ms_per_nfe"] = round(out["karras_heun_ms_per_call"] / out["heun_nfe"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100x64,16x256")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--heun_steps", type=int, default=5)
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
        sys.stderr.write(f"edm_dpm_sample_time: {spec} {json.dumps(out[f'launches_{spec}'])}\n")
        sys.stderr.flush()
        torch.cuda.empty_cache()
    if not args.no_loop:
        out["loop"] = measure_loop(args, dev)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
