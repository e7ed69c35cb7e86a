"""Time what score identity distillation (SiD) adds to a distribution-matching generator turn, on one GPU, in one process.

    python tools/sid_step_time.py [--batch 16] [--reps 5] [--warmup 2] [--leg_timeout 120] [--out profiles/sid_step_time.json]

Three measurements at [batch, 3, 64, 64], num_scales 1000:
  launches  the two new launches (dxmi_sid_grad_fwd, dxmi_sid_join), each the mean of 200 back-to-back launches between two device
            events, next to the torch expressions of the fallback of sid_generator_losses for the same stages on the same operands
            (the fallback leaves the gradient to autograd, so its expressions for the cotangents are written out here), timed the
            same way;
  nets      one forward_inference and one input_vjp (input_forward + input_backward) of the full-size real net: what each of the two
            denoisers costs a DMD turn and a SiD turn;
  turn      one generator turn, the loss and its backward through the generator (no optimiser, no fake-denoiser step, which are the
            same in both): DMTrainLoop's objective "sid" (sid_generator_losses, alpha 1.2) against objective "dmd"
            (dm_generator_losses, weighting dmd), on three full-size ImageNet-64 U-Nets (295.9 M parameters each, synthetic weights,
            dropout 0); legs alternate, median of --reps after --warmup rounds, device events around each leg and a synchronise at
            its end.
Every timed piece runs under its own time limit, kept by a watchdog thread: an overrun ends the script with status 124.  Prints one
JSON line per measurement and writes them to --out.  The figures are stated as measured; no test or threshold rests on them.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from dm_step_time import GEN_SIGMA, MODEL, S, timed  # noqa: E402

ALPHA = 1.2


def launch_times(ops, d, B, dev, limit):
    """us per stage at [B, 3, 64, 64]: the HIP launch and torch expressions for it."""
    from models.cm.karras_diffusion import cd_levels
    from models.cm.nn import append_dims, mean_flat
    shape = (B, 3, 64, 64)
    r = lambda: torch.randn(shape, device=dev)
    Fr, Ff, x, x_t, g_r, g_f = r(), r(), r(), r(), r(), r()
    tab = cd_levels(S, 0.002, 80.0, 7.0).device_table(torch.device(dev))
    idx = torch.randint(20, 980, (B,), device=dev)
    t = tab[idx]
    e = lambda v: append_dims(v, 4)
    _, _, d_dir, _, s = ops.sid_grad_fwd(Fr, Ff, x, x_t, idx, tab, ALPHA)

    def torch_grad():
        c_skip, c_out, _ = [e(v) for v in d.get_scalings(t)]
        d_r, d_f = c_out * Fr + c_skip * x_t, c_out * Ff + c_skip * x_t
        ss = mean_flat(torch.abs(x - d_r))
        delta, ex = d_r - d_f, d_f - x
        a_r, a_f = 2 * (1 - ALPHA) * delta + ex, (2 * ALPHA - 1) * delta - ex
        total = ((1 - ALPHA) * delta ** 2 + delta * ex).flatten(1).sum(dim=1)
        loss = torch.where(ss == 0, torch.zeros_like(ss), total / (x[0].numel() * ss))
        return c_out * a_r, c_out * a_f, c_skip * a_r + c_skip * a_f - delta, loss, ss

    def torch_join():
        c_in = e(d.get_scalings(t)[2])
        g = (d_dir + c_in * g_r + c_in * g_f) / e(s)
        return torch.where(e(s) == 0, torch.zeros_like(g), g)

    cases = {"sid_grad_fwd": (lambda: ops.sid_grad_fwd(Fr, Ff, x, x_t, idx, tab, ALPHA), torch_grad),
             "sid_join": (lambda: ops.sid_join(d_dir, g_r, g_f, s, idx, tab), torch_join)}
    out = {}
    for name, (hip, th) in cases.items():
        for fn in (hip, th):
            timed(fn, limit, 20)
        out[name] = {"hip_us": round(timed(hip, limit, 200) * 1e3, 2), "torch_us": round(timed(th, limit, 200) * 1e3, 2)}
    out["sum"] = {k: round(sum(v[k] for v in out.values()), 2) for k in ("hip_us", "torch_us")}
    return out


def alternating(legs, warmup, reps, limit):
    times = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            ms = timed(fn, limit)
            if r >= warmup:
                times[k].append(ms)
    out = {f"{k}_ms": round(statistics.median(v), 3) for k, v in times.items()}
    out.update({f"{k}_ms_all": [round(x, 3) for x in v] for k, v in times.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)      # the per-rank batch of the ImageNet-64 runs at 8 GPUs
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg_timeout", type=int, default=120)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sid_step_time.json"))
    args = ap.parse_args()
    from dxmi_hip import ops
    from models.cm.script_util import create_model_and_diffusion
    from models.cm.unet_train import input_vjp
    ops.device_check()
    dev, B = "cuda:0", args.batch
    torch.manual_seed(0)
    gen_net, diffusion = create_model_and_diffusion(**MODEL)
    fake, fake_diffusion = create_model_and_diffusion(**MODEL)
    real, real_diffusion = create_model_and_diffusion(**MODEL)
    with torch.no_grad():       # the constructor zeroes the output convolution: with it every denoiser would be c_skip x_t and delta = 0
        for net, seed in ((gen_net, 1), (fake, 2)):
            net.out[2].weight.normal_(0.0, 0.05, generator=torch.Generator().manual_seed(seed))
    real.load_state_dict(gen_net.state_dict())               # the generator starts from the teacher; the fake net has moved on
    gen_net, fake, real = gen_net.to(dev).train(), fake.to(dev).train(), real.to(dev).eval().requires_grad_(False)
    rows = [{"batch": B, "num_scales": S, "alpha": ALPHA, "launches": launch_times(ops, diffusion, B, dev, args.leg_timeout)}]
    print(json.dumps(rows[0]), flush=True)

    z = torch.randn(B, 3, 64, 64, device=dev)
    noise = torch.randn(B, 3, 64, 64, device=dev)
    idx = torch.randint(20, 980, (B,), device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)
    tm = 250 * torch.log(torch.rand(B, device=dev) * 5 + 0.1)
    with torch.no_grad():
        nets = alternating({"forward_inference": lambda: real.forward_inference(z, tm, y), "input_vjp": lambda: input_vjp(real, z, tm, noise, y)},
                           args.warmup, args.reps, args.leg_timeout)
    nets["input_vjp_minus_forward_ms"] = round(nets["input_vjp_ms"] - nets["forward_inference_ms"], 3)
    rows.append(dict({"batch": B, "reps": args.reps}, **nets))
    print(json.dumps(rows[-1]), flush=True)

    kw = dict(real_model=real, real_diffusion=real_diffusion, fake_model=fake, fake_diffusion=fake_diffusion, model_kwargs={"y": y},
              noise=noise, indices=idx, gen_sigma=GEN_SIGMA)

    def leg(loss_fn, **how):
        def run():
            for p in gen_net.parameters():
                p.grad = None
            loss_fn(gen_net, z, S, **kw, **how)["loss"].mean().backward()
        return run
    out = {"batch": B, "reps": args.reps, "num_scales": S, "alpha": ALPHA}
    out.update(alternating({"sid": leg(diffusion.sid_generator_losses, alpha=ALPHA), "dmd": leg(diffusion.dm_generator_losses, weighting="dmd")},
                           args.warmup, args.reps, args.leg_timeout))
    out["sid_minus_dmd_ms"] = round(out["sid_ms"] - out["dmd_ms"], 3)
    out["sid_over_dmd"] = round(out["sid_ms"] / out["dmd_ms"], 4)
    out["two_input_vjp_minus_forward_ms"] = round(2 * nets["input_vjp_minus_forward_ms"], 3)
    rows.append(out)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
