"""Generate tests/golden/edm_dsm.npz by running the REFERENCE's KarrasDenoiser.training_losses (models/cm/karras_diffusion.py:82-106,
get_weightings :18-31) and update_ema (models/cm/nn.py:57-67).

Runs ONLY in the build container, next to make_golden.py (same reference checkout and import stubs, same formula weights):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dsm.py

Fixed x_start / noise [N, 3, 16, 16] and sigmas spanning 0.002 .. 80.  Per weight schedule ws in (snr, snr+1, karras, truncated-snr,
uniform) the fixture holds, as arrays only:
  analytic.<ws>.xs_mse / .mse      terms of the analytic model tanh(0.7 x_in + 1e-3 t) (a CPU test restates it in torch);
  analytic_distill.karras.*        the same with distillation=True (boundary-condition scalings);
  <net>.<ws>.xs_mse / .mse         terms of the shrunken U-Nets (net = unet: class-conditional imagenet64 topology, unet_plain);
  <net>.grad.<param>               fp16 gradients of (loss * w).mean() (karras schedule, w = `loss_w`) for the parameters listed in
                                   <net>.grad_names (every tensor of <= 4096 elements and a few weights, so the file stays small);
  ema.*                            two-rate EMA: sources and targets before / after three update_ema calls per rate.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference first on sys.path and installs its import stubs)
import models.cm.karras_diffusion as ref_kd  # noqa: E402
import models.cm.nn as ref_nn  # noqa: E402

SCHEDULES = ("snr", "snr+1", "karras", "truncated-snr", "uniform")
SIGMAS = [0.002, 0.02, 0.25, 1.0, 6.0, 80.0]
BIG_PICK = ("input_blocks.0.0.weight", "out.2.weight", "input_blocks.3.1.proj_out.weight", "output_blocks.3.0.skip_connection.weight")
EMA_RATES = (0.999, 0.9)


def analytic(x_in, t, **kw):
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


def main():
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(2024)
    N = len(SIGMAS)
    x_start = torch.rand(N, 3, 16, 16, generator=g) * 2 - 1
    noise = torch.randn(N, 3, 16, 16, generator=g)
    sigmas = torch.tensor(SIGMAS, dtype=torch.float32)
    loss_w = torch.rand(N, generator=g) + 0.5
    y = torch.tensor([3, 977, 0, 511, 42, 999])
    out = dict(x_start=x_start, noise=noise, sigmas=sigmas, loss_w=loss_w, y=y)

    for ws in SCHEDULES:
        d = ref_kd.KarrasDenoiser(sigma_data=0.5, weight_schedule=ws)
        t = d.training_losses(analytic, x_start, sigmas, noise=noise)
        out[f"analytic.{ws}.xs_mse"], out[f"analytic.{ws}.mse"] = t["xs_mse"], t["mse"]
    d = ref_kd.KarrasDenoiser(sigma_data=0.5, weight_schedule="karras", distillation=True)
    t = d.training_losses(analytic, x_start, sigmas, noise=noise)
    out["analytic_distill.karras.xs_mse"], out["analytic_distill.karras.mse"] = t["xs_mse"], t["mse"]

    for tag, over in (("unet", {}), ("unet_plain", dict(class_cond=False, use_scale_shift_norm=False, resblock_updown=False))):
        net, _ = mg.build_edm(**over)
        kw = dict(y=y) if over.get("class_cond", True) else {}
        with torch.no_grad():
            for ws in SCHEDULES:
                d = ref_kd.KarrasDenoiser(sigma_data=0.5, weight_schedule=ws)
                t = d.training_losses(net, x_start, sigmas, model_kwargs=kw, noise=noise)
                out[f"{tag}.{ws}.xs_mse"], out[f"{tag}.{ws}.mse"] = t["xs_mse"], t["mse"]
        d = ref_kd.KarrasDenoiser(sigma_data=0.5, weight_schedule="karras")
        net.zero_grad()
        t = d.training_losses(net, x_start, sigmas, model_kwargs=kw, noise=noise)
        (t["loss"] * loss_w).mean().backward()
        names = [n for n, p in net.named_parameters() if p.numel() <= 4096 or n in BIG_PICK]
        params = dict(net.named_parameters())
        for n in names:
            out[f"{tag}.grad.{n}"] = params[n].grad.detach().to(torch.float16)
        out[f"{tag}.grad_names"] = np.array(names)

    ge = torch.Generator().manual_seed(7)
    shapes = [(1000,), (37,), (64, 3, 3, 3), (4097,)]
    src = [[torch.randn(s, generator=ge) for s in shapes] for _ in range(3)]
    for k, rate in enumerate(EMA_RATES):
        tgt = [torch.randn(s, generator=ge) for s in shapes]
        for i, s in enumerate(tgt):
            out[f"ema.{k}.before.{i}"] = s.clone()
        for it in range(3):
            ref_nn.update_ema(tgt, src[it], rate=rate)
        for i, s in enumerate(tgt):
            out[f"ema.{k}.after.{i}"] = s.clone()
    for it in range(3):
        for i, s in enumerate(src[it]):
            out[f"ema.src.{it}.{i}"] = s
    out["ema.rates"] = np.array(EMA_RATES)
    mg.save("edm_dsm", **out)


if __name__ == "__main__":
    main()
