"""Time what adversarial score identity distillation (SiDA) adds to a SiD generator turn, on one GPU, in one process.

    python tools/sida_step_time.py [--batch 16] [--reps 5] [--warmup 2] [--leg_timeout 120] [--out profiles/sida_step_time.json]

Three measurements, num_scales 1000:
  launches  the two new launches (dxmi_sida_map_fwd, dxmi_sida_map_bwd) at the full-size net's bottleneck [batch, 64, 768], each the
            mean of 200 back-to-back launches between two device events, next to the torch expressions of the fallback for the same
            stage on the same operand, timed the same way;
  encoder   encoder_input_forward + encoder_input_backward of the full-size fake net: the separate encoder pass a discriminator on
            its own evaluation would pay per generator turn (DMD2's GAN term pays it), re-measured here, in this process;
  turn      one generator turn, the loss and its backward through the generator (no optimiser, no fake-denoiser step): objective
            "sida" (sida_generator_losses, alpha 1.2, sida_gen_weight 0.01) against objective "sid" (sid_generator_losses), on three
            full-size ImageNet-64 U-Nets (synthetic weights, dropout 0); legs alternate, median of --reps after --warmup rounds.
The claim to read off: sida_minus_sid_ms against encoder_pass_ms.  Every timed piece runs under its own time limit, kept by a
watchdog thread: an overrun ends the script with status 124.  Prints one JSON line per measurement and writes them to --out.  The
figures are stated as measured; no test or threshold rests on them.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from dm_step_time import GEN_SIGMA, MODEL, S, timed  # noqa: E402
from sid_step_time import ALPHA, alternating  # noqa: E402

WEIGHT = 0.01
P, CB = 64, 768


def launch_times(ops, B, dev, limit):
    """us per launch at [B, 64, 768]: the HIP launch and the torch expressions for it."""
    h = torch.randn(B, P, CB, device=dev).to(torch.bfloat16)
    logit, _ = ops.sida_map_fwd(h, -1)

    def torch_fwd():
        lg = h.float().mean(dim=2)
        return lg, torch.nn.functional.softplus(-lg).mean(dim=1)

    def torch_bwd():
        return (-(WEIGHT * 12288.0 / (P * CB)) * torch.sigmoid(-logit))[:, :, None].expand(B, P, CB).to(torch.bfloat16).contiguous()

    cases = {"sida_map_fwd": (lambda: ops.sida_map_fwd(h, -1), torch_fwd),
             "sida_map_bwd": (lambda: ops.sida_map_bwd(logit, -1, WEIGHT * 12288.0, CB), torch_bwd)}
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
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sida_step_time.json"))
    args = ap.parse_args()
    from dxmi_hip import ops
    from models.cm.script_util import create_model_and_diffusion
    from models.cm.unet_train import encoder_input_backward, encoder_input_forward
    ops.device_check()
    dev, B = "cuda:0", args.batch
    torch.manual_seed(0)
    rows = [{"batch": B, "shape": [B, P, CB], "launches": launch_times(ops, B, dev, args.leg_timeout)}]
    print(json.dumps(rows[0]), flush=True)

    gen_net, diffusion = create_model_and_diffusion(**MODEL)
    fake, fake_diffusion = create_model_and_diffusion(**MODEL)
    real, real_diffusion = create_model_and_diffusion(**MODEL)
    with torch.no_grad():       # the constructor zeroes the output convolution: with it every denoiser would be c_skip x_t and delta = 0
        for net, seed in ((gen_net, 1), (fake, 2)):
            net.out[2].weight.normal_(0.0, 0.05, generator=torch.Generator().manual_seed(seed))
    real.load_state_dict(gen_net.state_dict())
    gen_net, fake, real = gen_net.to(dev).train(), fake.to(dev).train(), real.to(dev).eval().requires_grad_(False)
    z = torch.randn(B, 3, 64, 64, device=dev)
    noise = torch.randn(B, 3, 64, 64, device=dev)
    idx = torch.randint(20, 980, (B,), device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)
    tm = 250 * torch.log(torch.rand(B, device=dev) * 5 + 0.1)
    h0, _ = encoder_input_forward(fake, z, tm, y)
    assert tuple(h0.shape) == (B, 8, 8, CB), tuple(h0.shape)
    d_h = torch.randn(h0.shape, device=dev).to(torch.bfloat16)

    def encoder_pass():
        _, tape = encoder_input_forward(fake, z, tm, y)
        encoder_input_backward(tape, d_h)
    enc = alternating({"encoder_pass": encoder_pass}, args.warmup, args.reps, args.leg_timeout)
    rows.append(dict({"batch": B, "reps": args.reps}, **enc))
    print(json.dumps(rows[-1]), flush=True)

    kw = dict(real_model=real, real_diffusion=real_diffusion, fake_model=fake, fake_diffusion=fake_diffusion, model_kwargs={"y": y},
              noise=noise, indices=idx, gen_sigma=GEN_SIGMA, alpha=ALPHA)

    def leg(loss_fn, **how):
        def run():
            for p in gen_net.parameters():
                p.grad = None
            loss_fn(gen_net, z, S, **kw, **how)["loss"].mean().backward()
        return run
    out = {"batch": B, "reps": args.reps, "num_scales": S, "alpha": ALPHA, "sida_gen_weight": WEIGHT}
    out.update(alternating({"sida": leg(diffusion.sida_generator_losses, sida_gen_weight=WEIGHT), "sid": leg(diffusion.sid_generator_losses)},
                           args.warmup, args.reps, args.leg_timeout))
    out["sida_minus_sid_ms"] = round(out["sida_ms"] - out["sid_ms"], 3)
    out["sida_over_sid"] = round(out["sida_ms"] / out["sid_ms"], 4)
    out["encoder_pass_ms"] = enc["encoder_pass_ms"]
    out["saved_against_a_separate_encoder_pass_ms"] = round(enc["encoder_pass_ms"] - out["sida_minus_sid_ms"], 3)
    rows.append(out)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
