"""Time the probability-flow likelihood (models/cm/likelihood.py, models/DxMI/likelihood.py) on one GPU, in one process.

    python tools/nll_step_time.py [--reps 5] [--warmup 2] [--leg_timeout 120] [--out profiles/nll_step_time.json]

Two measurements per case, at [16, 3, 64, 64] on the full ImageNet-64 EDM net and at [256, 3, 32, 32] on the CIFAR-10 DDPM net
(synthetic weights, dropout off):
  launches  the three modes of dxmi_pf_ll_stage (FIRST, PREDICT, CORRECT on the last row, given probe), each the mean of 200
            back-to-back launches between two device events, next to the torch expressions of the fallback loop for the same stage on
            the same operands, timed the same way;
  vjp       one input_vjp (forward + input-only backward, what one network evaluation of the likelihood costs) against one full
            forward_with_grad + backward on the same net, input and probe: what the input-only switch saves.  Legs alternate, median
            of --reps after --warmup rounds, device events around each leg and a synchronise at its end.
From the CIFAR figures: the projected wall time of 10 000 test images at steps = 40 on one GPU, (10 000 / 256 batches) x 40 steps x
(2 input_vjp + PREDICT + CORRECT).  Every timed piece runs under its own time limit, kept by a watchdog thread: an overrun ends the
script with status 124.  Prints one JSON line per case and writes them to --out.
"""
import argparse
import json
import math
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))

import torch  # noqa: E402

EDM_MODEL = dict(image_size=64, class_cond=True, learn_sigma=False, num_channels=192, num_res_blocks=3, channel_mult="", num_heads=4,
                 num_head_channels=64, num_heads_upsample=-1, attention_resolutions="32,16,8", dropout=0.0, use_checkpoint=False,
                 use_scale_shift_norm=True, resblock_updown=True, use_fp16=True, use_new_attention_order=False, weight_schedule="karras")
DDPM_MODEL = dict(ch=128, out_ch=3, ch_mult=(1, 2, 2, 2), num_res_blocks=2, attn_resolutions=[16], dropout=0.1, in_channels=3,
                  resolution=32)
STEPS = 40


def _overrun():
    sys.stderr.write("nll_step_time: a timed piece overran its time limit\n")
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


def launch_times(ops, sch, shape, dev, limit):
    """us per mode at `shape`: the HIP launch and the fallback's torch expressions for it (models.cm.likelihood.pf_ll_*)."""
    from models.cm import likelihood as ll
    N = shape[0]
    r = lambda: torch.randn(shape, device=dev)
    x, F, g, e, k1, x_in = r(), r(), r(), r(), r(), r()
    t, div1, ell, prior, logp, bpd = (torch.zeros(N, device=dev) for _ in range(6))
    tab, last = sch.device_table(torch.device(dev)), sch.steps - 1
    row = tab[last]
    x_first, x_corr = x.clone(), x.clone()

    def torch_first():
        xs = x * tab[0, ops.PL_XSCALE]
        return xs, tab[0, ops.PL_CIN] * xs, torch.full((N,), float(tab[0, ops.PL_T]), device=dev), torch.full((N,), float(tab[0, ops.PL_LOGDET0]), device=dev)

    def torch_predict():
        kk, xt, d1 = ll.pf_ll_predict(row, x, F, g, e)
        return kk, xt, row[ops.PL_CIN_NEXT] * xt, d1

    def torch_correct():
        xn, el = ll.pf_ll_correct(row, x, k1, F, g, e, div1, ell)
        return (xn, el) + tuple(ll.pf_ll_finish(row, xn, el))

    cases = {"first": (lambda: ops.pf_ll_stage(ops.PF_LL_FIRST, tab, t, row=0, x=x_first, x_in=x_in, ell=ell), torch_first),
             "predict": (lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, row=last, x=x, model_out=F, vjp=g, eps=e, k1=k1, x_in=x_in,
                                                 div1=div1), torch_predict),
             "correct": (lambda: ops.pf_ll_stage(ops.PF_LL_CORRECT, tab, t, row=last, x=x_corr, model_out=F, vjp=g, eps=e, k1=k1, x_in=x_in,
                                                 div1=div1, ell=ell, prior=prior, logp=logp, bpd=bpd), torch_correct)}
    out = {}
    for name, (hip, th) in cases.items():
        for fn in (hip, th):
            timed(fn, limit, 20)
        out[name] = {"hip_us": round(timed(hip, limit, 200) * 1e3, 2), "torch_us": round(timed(th, limit, 200) * 1e3, 2)}
    out["sum"] = {k: round(sum(v[k] for v in out.values()), 2) for k in ("hip_us", "torch_us")}
    return out


def vjp_times(vjp, full, args):
    legs = {"input_vjp": vjp, "full_backward": full}
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.reps):
        for k, fn in legs.items():
            ms = timed(fn, args.leg_timeout)
            if r >= args.warmup:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {f"{k}_ms": round(v, 3) for k, v in med.items()}
    out.update({f"{k}_ms_all": [round(x, 3) for x in v] for k, v in times.items()})
    out["saved_ms"] = round(med["full_backward"] - med["input_vjp"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg_timeout", type=int, default=120)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nll_step_time.json"))
    args = ap.parse_args()
    from dxmi_hip import ops
    from models.cm import unet_train
    from models.cm.likelihood import edm_ll_schedule
    from models.cm.script_util import create_model_and_diffusion
    from models.DxMI import unet_small_train
    from models.DxMI.likelihood import ddpm_ll_schedule
    from models.DxMI.unet_small import Model
    ops.device_check()
    dev = "cuda:0"
    torch.manual_seed(0)
    rows = []

    # ---- the ImageNet-64 EDM net at [16, 3, 64, 64]
    shape = (16, 3, 64, 64)
    net, diffusion = create_model_and_diffusion(**EDM_MODEL)
    with torch.no_grad():       # the constructor zeroes the output convolution
        net.out[2].weight.normal_(0.0, 0.05, generator=torch.Generator().manual_seed(1))
    net = net.to(dev).eval()
    sch = edm_ll_schedule(diffusion, 3 * 64 * 64, STEPS)
    x, v = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
    t = torch.full((shape[0],), 250 * math.log(2.0), device=dev)
    y = torch.randint(0, 1000, (shape[0],), device=dev)

    def edm_full():
        for p in net.parameters():
            p.grad = None
        unet_train.forward_with_grad(net, x.clone().requires_grad_(True), t, y).backward(v)
    row = {"case": "imagenet64_edm", "shape": list(shape), "launches": launch_times(ops, sch, shape, dev, args.leg_timeout)}
    row.update(vjp_times(lambda: unet_train.input_vjp(net, x, t, v, y), edm_full, args))
    rows.append(row)
    print(json.dumps(row), flush=True)
    del net
    torch.cuda.empty_cache()

    # ---- the CIFAR-10 DDPM net at [256, 3, 32, 32]
    shape = (256, 3, 32, 32)
    net = Model(**DDPM_MODEL).to(dev).eval()
    sch = ddpm_ll_schedule(3 * 32 * 32, STEPS, "uniform")
    x, v = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
    t = torch.full((shape[0],), 500.0, device=dev)

    def ddpm_full():
        for p in net.parameters():
            p.grad = None
        unet_small_train.forward_with_grad(net, x.clone().requires_grad_(True), t).backward(v)
    row = {"case": "cifar10_ddpm", "shape": list(shape), "launches": launch_times(ops, sch, shape, dev, args.leg_timeout)}
    row.update(vjp_times(lambda: unet_small_train.input_vjp(net, x, t, v), ddpm_full, args))
    per_step_ms = 2 * row["input_vjp_ms"] + (row["launches"]["predict"]["hip_us"] + row["launches"]["correct"]["hip_us"]) / 1e3
    row["projected_10000_images_steps40_s"] = round(math.ceil(10000 / shape[0]) * STEPS * per_step_ms / 1e3, 1)
    rows.append(row)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
