"""Time one DSM training step of the full-size ImageNet-64 EDM U-Net (295.9 M parameters) per phase, on one GPU.

    python tools/edm_dsm_time.py [--batches 16,32] [--steps 5] [--warmup 2]

Phases (device events, each window ends in a synchronise): U-Net forward incl. the DSM prep and loss launches
(training_losses), backward incl. dxmi_edm_dsm_loss_bwd, MixedPrecisionTrainer.optimize (norms + RAdam, fp16 bookkeeping),
the EMA (nn.update_ema_rates, one rate), and the loss kernels alone.  Achieved GB/s of dxmi_ema_update = 12 bytes per parameter
and rate (read source, read + write EMA) over its time.  Prints one JSON line per batch size.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))

import torch  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,32")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from dxmi_hip import ops
    from dxmi_hip.optim import RAdam
    from models.cm.fp16_util import MixedPrecisionTrainer
    from models.cm.nn import update_ema_rates
    from models.cm.resample import LogNormalSampler
    from models.cm.script_util import create_model_and_diffusion
    ops.device_check()
    dev = "cuda:0"
    torch.manual_seed(0)
    net, diffusion = create_model_and_diffusion(
        image_size=64, class_cond=True, learn_sigma=False, num_channels=192, num_res_blocks=3, channel_mult="", num_heads=4,
        num_head_channels=64, num_heads_upsample=-1, attention_resolutions="32,16,8", dropout=0.0, use_checkpoint=False,
        use_scale_shift_norm=True, resblock_updown=True, use_fp16=True, use_new_attention_order=False, weight_schedule="karras")
    net = net.to(dev).train()
    n_params = sum(p.numel() for p in net.parameters())
    mp = MixedPrecisionTrainer(model=net, use_fp16=True)
    opt = RAdam(mp.master_params, lr=1e-4)
    ema = [[p.detach().clone() for p in mp.master_params]]
    sampler = LogNormalSampler()
    for B in [int(b) for b in args.batches.split(",")]:
        x0 = torch.rand(B, 3, 64, 64, device=dev) * 2 - 1
        y = torch.randint(0, 1000, (B,), device=dev)
        noise = torch.randn_like(x0)
        sig, w = sampler.sample(B, dev)
        state = {}

        def fwd():
            mp.zero_grad()
            t = diffusion.training_losses(net, x0, sig, model_kwargs={"y": y}, noise=noise)
            state["loss"] = (t["loss"] * w).mean()

        def bwd():
            mp.backward(state["loss"])

        def step():
            fwd()
            bwd()
            mp.optimize(opt)
            update_ema_rates(ema, mp.master_params, [0.9999])

        for _ in range(args.warmup):
            step()
        t_fwd = t_bwd = 0.0
        for _ in range(args.steps):
            t_fwd += timed(fwd, 1)
            t_bwd += timed(bwd, 1)
            mp.optimize(opt)
        t_fwd, t_bwd = t_fwd / args.steps, t_bwd / args.steps
        t_opt = timed(lambda: (fwd(), bwd(), mp.optimize(opt)), args.steps) - t_fwd - t_bwd
        t_ema = timed(lambda: update_ema_rates(ema, mp.master_params, [0.9999]), args.steps * 4)
        F = torch.randn_like(x0)
        g = torch.ones(B, device=dev)
        t_loss = timed(lambda: (ops.edm_dsm_prep(x0, noise, sig), ops.edm_dsm_loss_fwd(F, x0, noise, sig, "karras"),
                                ops.edm_dsm_loss_bwd(g, None, F, x0, noise, sig, "karras")), args.steps * 4)
        t_step = timed(step, args.steps)
        print(json.dumps({"batch": B, "params": n_params, "step_ms": round(t_step, 3), "unet_fwd_ms": round(t_fwd, 3),
                          "unet_bwd_ms": round(t_bwd, 3), "optimize_ms": round(t_opt, 3), "ema_ms": round(t_ema, 3),
                          "ema_GBps": round(12.0 * n_params / (t_ema * 1e-3) / 1e9, 1), "loss_kernels_ms": round(t_loss, 4),
                          "images_per_s": round(B / (t_step * 1e-3), 1)}), flush=True)


if __name__ == "__main__":
    main()
