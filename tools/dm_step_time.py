"""Time what a distribution-matching (DM) generator step spends outside its network evaluations, on one GPU, in one process.

    python tools/dm_step_time.py [--batch 16] [--reps 5] [--warmup 2] [--leg_timeout 120] [--out profiles/dm_step_time.json]

Two measurements at [batch, 3, 64, 64], num_scales 1000, weighting dmd:
  launches  the four non-network launches of a generator step (dxmi_dm_gen_in, dxmi_dm_gen_prep, dxmi_dm_grad_fwd, dxmi_dm_gen_bwd),
            each the mean of 200 back-to-back launches between two device events, next to the torch expressions of the fallback of
            dm_generator_losses for the same four stages on the same operands, timed the same way;
  step      one full iteration without the optimiser launches: dm_generator_losses + backward of loss.mean() through the generator,
            then the fake denoiser's training_losses on the returned images + backward, on three full-size ImageNet-64 U-Nets (295.9 M
            parameters each, synthetic weights, dropout 0): the device path (one autograd node around the generator) against the torch
            fallback on the SAME HIP nets, which a thin callable around each net selects.  Both run the same network programs; legs
            alternate, median of --reps after --warmup rounds, device events around each leg and a synchronise at its end.
Every timed piece runs under its own time limit, kept by a watchdog thread: an overrun ends the script with status 124.  Prints one
JSON line per measurement and writes both to --out.

    python tools/dm_step_time.py --gen_sigmas 80,5,1,0.3 [--out profiles/dmms_step_time.json]

times the K-step generator of DMD2's backward simulation instead, device path only:
  launches  dxmi_dmms_stage (noise given, and made in the launch) and the four non-network launches of a K-step generator step
            (dxmi_dmms_in, dxmi_dmms_prep, dxmi_dm_grad_fwd, dxmi_dmms_bwd) at the same shape, steps cycling through 0 .. K-1;
  step      the same full iteration with gen_sigmas (steps drawn once, uniform over 0 .. K-1, and injected with the simulation noise)
            next to the K = 1 leg (gen_sigma = gen_sigmas[0]) of the same run, alternating.  The expected difference is K - 1
            inference forwards of the generator.
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
S = 1000
GEN_SIGMA = 80.0


def _overrun():
    sys.stderr.write("dm_step_time: a timed piece overran its time limit\n")
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


def launch_times(ops, d, B, dev, limit):
    """us per stage at [B, 3, 64, 64]: the HIP launch and the fallback's torch expressions for it."""
    from models.cm.karras_diffusion import cd_levels
    from models.cm.nn import append_dims, mean_flat
    shape = (B, 3, 64, 64)
    r = lambda: torch.randn(shape, device=dev)
    z, noise, Fg, Fr, Ff = r(), r(), r(), r(), r()
    tab = cd_levels(S, 0.002, 80.0, 7.0).device_table(torch.device(dev))
    idx = torch.randint(20, 980, (B,), device=dev)
    t = tab[idx]
    up = torch.rand(B, device=dev)
    sg = torch.full((B,), GEN_SIGMA, device=dev)
    e = lambda v: append_dims(v, 4)
    x, x_t, _, _, _ = ops.dm_gen_prep(Fg, z, noise, idx, tab, GEN_SIGMA)
    g, _, _ = ops.dm_grad_fwd(Fr, Ff, x, x_t, idx, tab, "dmd")

    def torch_in():
        return e(d.get_scalings(sg)[2]) * (z * GEN_SIGMA), 1000 * 0.25 * torch.log(sg + 1e-44)

    def torch_prep():
        c_skip, c_out, _ = [e(v) for v in d.get_scalings(sg)]
        xx = c_out * Fg + c_skip * (z * GEN_SIGMA)
        xt = xx + noise * e(t)
        return xx, xt, e(d.get_scalings(t)[2]) * xt, 1000 * 0.25 * torch.log(t + 1e-44)

    def torch_grad():
        c_skip, c_out, _ = [e(v) for v in d.get_scalings(t)]
        d_r, d_f = c_out * Fr + c_skip * x_t, c_out * Ff + c_skip * x_t
        s = mean_flat(torch.abs(x - d_r))
        gg = (d_f - d_r) / e(s)
        gg = torch.where(e(s) == 0, torch.zeros_like(gg), gg)
        return gg, 0.5 * mean_flat(gg ** 2), s

    def torch_bwd():
        return (e(up) * g / g[0].numel()) * e(d.get_scalings(sg)[1])

    cases = {"gen_in": (lambda: ops.dm_gen_in(z, GEN_SIGMA), torch_in),
             "gen_prep": (lambda: ops.dm_gen_prep(Fg, z, noise, idx, tab, GEN_SIGMA), torch_prep),
             "grad_fwd": (lambda: ops.dm_grad_fwd(Fr, Ff, x, x_t, idx, tab, "dmd"), torch_grad),
             "gen_bwd": (lambda: ops.dm_gen_bwd(up, g, GEN_SIGMA), torch_bwd)}
    out = {}
    for name, (hip, th) in cases.items():
        for fn in (hip, th):
            timed(fn, limit, 20)
        out[name] = {"hip_us": round(timed(hip, limit, 200) * 1e3, 2), "torch_us": round(timed(th, limit, 200) * 1e3, 2)}
    out["sum"] = {k: round(sum(v[k] for v in out.values()), 2) for k in ("hip_us", "torch_us")}
    return out


def ms_launch_times(ops, ladder, B, dev, limit):
    """us per launch of the K-step generator at [B, 3, 64, 64]."""
    from models.cm.karras_diffusion import cd_levels
    K = len(ladder)
    r = lambda: torch.randn((B, 3, 64, 64), device=dev)
    z, noise, eps, Fg, Fr, Ff = r(), r(), r(), r(), r(), r()
    tab = cd_levels(S, 0.002, 80.0, 7.0).device_table(torch.device(dev))
    sig = torch.tensor(ladder, dtype=torch.float32, device=dev)
    idx = torch.randint(20, 980, (B,), device=dev)
    steps = (torch.arange(B, device=dev) % K).contiguous()
    live = steps.clamp(min=1)                                     # stage 0 with every image live: the launch's full traffic
    index = torch.arange(B, device=dev)
    up = torch.rand(B, device=dev)
    x_k, x_in, tm = ops.dmms_in(z, sig)
    x, x_t, _, _, _ = ops.dmms_prep(Fg, x_k, noise, steps, sig, idx, tab)
    g, _, _ = ops.dm_grad_fwd(Fr, Ff, x, x_t, idx, tab, "dmd")
    cases = {"dmms_in": lambda: ops.dmms_in(z, sig),
             "dmms_prep": lambda: ops.dmms_prep(Fg, x_k, noise, steps, sig, idx, tab),
             "grad_fwd": lambda: ops.dm_grad_fwd(Fr, Ff, x, x_t, idx, tab, "dmd"),
             "dmms_bwd": lambda: ops.dmms_bwd(up, g, steps, sig)}
    if K > 1:
        cases.update({"dmms_stage": lambda: ops.dmms_stage(Fg, 0, sig, x_k, x_in, tm, steps=live, eps=eps),
                      "dmms_stage_own_noise": lambda: ops.dmms_stage(Fg, 0, sig, x_k, x_in, tm, steps=live, sample_index=index, seed=1, draw=0),
                      "dmms_stage_mixed_steps": lambda: ops.dmms_stage(Fg, 0, sig, x_k, x_in, tm, steps=steps, eps=eps)})
    out = {}
    for name, fn in cases.items():
        timed(fn, limit, 20)
        out[name] = {"hip_us": round(timed(fn, limit, 200) * 1e3, 2)}
    out["sum_of_a_step"] = {"hip_us": round(sum(out[k]["hip_us"] for k in ("dmms_in", "dmms_prep", "grad_fwd", "dmms_bwd")), 2)}
    return out


def main_ms(args, ladder):
    from dxmi_hip import ops
    from models.cm.script_util import create_model_and_diffusion
    ops.device_check()
    dev, B, K = "cuda:0", args.batch, len(ladder)
    torch.manual_seed(0)
    gen_net, diffusion = create_model_and_diffusion(**MODEL)
    fake, fake_diffusion = create_model_and_diffusion(**MODEL)
    real, real_diffusion = create_model_and_diffusion(**MODEL)
    with torch.no_grad():
        for net, seed in ((gen_net, 1), (fake, 2)):
            net.out[2].weight.normal_(0.0, 0.05, generator=torch.Generator().manual_seed(seed))
    real.load_state_dict(gen_net.state_dict())
    gen_net, fake, real = gen_net.to(dev).train(), fake.to(dev).train(), real.to(dev).eval().requires_grad_(False)
    rows = [{"batch": B, "num_scales": S, "gen_sigmas": list(ladder), "launches": ms_launch_times(ops, ladder, B, dev, args.leg_timeout)}]
    print(json.dumps(rows[0]), flush=True)
    r = lambda: torch.randn(B, 3, 64, 64, device=dev)
    z, noise, dsm_noise = r(), r(), r()
    sim = torch.randn(K - 1, B, 3, 64, 64, device=dev)
    steps = torch.randint(0, K, (B,), device=dev)
    sigmas = (torch.randn(B, device=dev) * 1.2 - 1.2).exp()
    idx = torch.randint(20, 980, (B,), device=dev)
    kw = {"y": torch.randint(0, 1000, (B,), device=dev)}

    def leg(**how):
        def run():
            for p in list(gen_net.parameters()) + list(fake.parameters()):
                p.grad = None
            terms = diffusion.dm_generator_losses(gen_net, z, S, real_model=real, real_diffusion=real_diffusion, fake_model=fake,
                                                  fake_diffusion=fake_diffusion, model_kwargs=kw, noise=noise, indices=idx, **how)
            terms["loss"].mean().backward()
            fake_diffusion.training_losses(fake, terms["x"], sigmas, model_kwargs=kw, noise=dsm_noise)["loss"].mean().backward()
        return run
    legs = {"one_step": leg(gen_sigma=ladder[0]), "k_step": leg(gen_sigmas=ladder, steps=steps, sim_noise=sim)}
    times = {k: [] for k in legs}
    for rnd in range(args.warmup + args.reps):
        for k, fn in legs.items():
            ms = timed(fn, args.leg_timeout)
            if rnd >= args.warmup:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    x_in, t_g = ops.dm_gen_in(z, ladder[0])
    fwd = lambda: gen_net.forward_inference(x_in, t_g, kw["y"])
    timed(fwd, args.leg_timeout, 2)
    out = {"batch": B, "reps": args.reps, "num_scales": S, "K": K, "steps": steps.tolist()}
    out.update({f"{k}_ms": round(v, 3) for k, v in med.items()})
    out.update({f"{k}_ms_all": [round(x, 3) for x in v] for k, v in times.items()})
    out["k_step_minus_one_step_ms"] = round(med["k_step"] - med["one_step"], 3)
    out["generator_forward_inference_ms"] = round(timed(fwd, args.leg_timeout, 5), 3)
    rows.append(out)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)      # the per-rank batch of the ImageNet-64 runs at 8 GPUs
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg_timeout", type=int, default=120)
    ap.add_argument("--gen_sigmas", type=str, default="")  # the ladder of a K-step generator, e.g. 80,5,1,0.3: time that instead
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "dmms_step_time.json" if args.gen_sigmas else "dm_step_time.json")
    if args.gen_sigmas:
        from models.cm.karras_diffusion import gen_ladder
        return main_ms(args, gen_ladder("--gen_sigmas", [float(v) for v in args.gen_sigmas.split(",")]).sigmas)
    from dxmi_hip import ops
    from models.cm.script_util import create_model_and_diffusion
    ops.device_check()
    dev, B = "cuda:0", args.batch
    torch.manual_seed(0)
    gen_net, diffusion = create_model_and_diffusion(**MODEL)
    fake, fake_diffusion = create_model_and_diffusion(**MODEL)
    real, real_diffusion = create_model_and_diffusion(**MODEL)
    with torch.no_grad():       # the constructor zeroes the output convolution: with it every denoiser would be c_skip x_t and g = 0
        for net, seed in ((gen_net, 1), (fake, 2)):
            net.out[2].weight.normal_(0.0, 0.05, generator=torch.Generator().manual_seed(seed))
    real.load_state_dict(gen_net.state_dict())               # the generator starts from the teacher; the fake net has moved on
    gen_net, fake, real = gen_net.to(dev).train(), fake.to(dev).train(), real.to(dev).eval().requires_grad_(False)
    rows = [{"batch": B, "num_scales": S, "launches": launch_times(ops, diffusion, B, dev, args.leg_timeout)}]
    print(json.dumps(rows[0]), flush=True)

    z = torch.randn(B, 3, 64, 64, device=dev)
    noise = torch.randn(B, 3, 64, 64, device=dev)
    dsm_noise = torch.randn(B, 3, 64, 64, device=dev)
    sigmas = (torch.randn(B, device=dev) * 1.2 - 1.2).exp()
    idx = torch.randint(20, 980, (B,), device=dev)
    kw = {"y": torch.randint(0, 1000, (B,), device=dev)}
    as_callable = lambda net: (lambda x, t, **k: net(x, t, **k))      # no UNetModel: the losses take their torch paths

    def leg(g_model, r_model, f_model):
        def run():
            for p in list(gen_net.parameters()) + list(fake.parameters()):
                p.grad = None
            terms = diffusion.dm_generator_losses(g_model, z, S, real_model=r_model, real_diffusion=real_diffusion, fake_model=f_model,
                                                  fake_diffusion=fake_diffusion, model_kwargs=kw, noise=noise, indices=idx)
            terms["loss"].mean().backward()
            fake_diffusion.training_losses(f_model, terms["x"], sigmas, model_kwargs=kw, noise=dsm_noise)["loss"].mean().backward()
            return terms["loss"]
        return run
    legs = {"device": leg(gen_net, real, fake), "torch": leg(as_callable(gen_net), as_callable(real), as_callable(fake))}
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
    rows.append(out)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
