"""Generate tests/golden/karras_sample.npz by running the REFERENCE's karras_sample (models/cm/karras_diffusion.py:354-640).

Runs ONLY in the build container, next to make_golden.py (same reference checkout and import stubs, same formula weights):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_karras.py

Every Gaussian draw goes through a recording generator (randn / randn_like, in the reference's order), so a test that replays the
stored draws reproduces the trajectory.  Per case (sampler and settings) the fixture holds, as arrays only:
  <case>.sigmas, .sigma_hat (per step, from the callback), .eval_sigma / .eval_t (noise level and time input of every network
  evaluation, recorded at denoise()), .sigma_down / .sigma_up (ancestral);
  per model m in (analytic, unet, unet_plain): <case>.<m>.x / .denoised [steps, B, C, H, W] (callback values) and
  <case>.<m>.sample (karras_sample's result); <case>.analytic.draws and <case>.draws (the two U-Nets) [K, B, C, H, W];
  <case>.y: the label of the class-conditional U-Net.
The analytic model is tanh(0.7 x_in + 1e-3 t) in fp32 on 2 x 3 x 8 x 8: a test restates it in torch on the device, which
isolates the sampler from the bf16 network; its values are stored in fp32.  The U-Nets run on 1 x 3 x 16 x 16 and their per-step
values are stored in fp16 (a relative rounding of 2^-11, against the 3e-2 bound their bf16 device run is held to), so the
fixture stays small.  Case heun40 (steps 40, rho 7) holds the tables only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference first on sys.path and installs its import stubs)
import models.cm.karras_diffusion as ref_kd  # noqa: E402

ANALYTIC_SHAPE, UNET_SHAPE = (2, 3, 8, 8), (1, 3, 16, 16)
CASES = {
    "heun6": dict(sampler="heun", steps=6),
    "heun6_churn": dict(sampler="heun", steps=6, s_churn=10.0, s_tmin=0.05, s_tmax=10.0, s_noise=1.007),
    "dpm4_churn": dict(sampler="dpm", steps=4, s_churn=2.0, s_noise=1.007),
    "euler8": dict(sampler="euler", steps=8),
    "ancestral8": dict(sampler="ancestral", steps=8),
}


class RecordingGenerator:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.draws = []

    def randn(self, *shape, device=None):
        v = torch.randn(*shape, generator=self.g)
        self.draws.append(v.clone())
        return v.to(device)

    def randn_like(self, x):
        v = torch.randn(x.shape, generator=self.g, dtype=x.dtype)
        self.draws.append(v.clone())
        return v.to(x.device)


def analytic(x_in, t, **kw):
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


def run(diffusion, model, kw, case, seed, shape):
    evals, ts, cb = [], [], []
    orig = diffusion.denoise

    def denoise(model_, x_t, sigmas, **mk):
        evals.append(sigmas[0].clone())
        ts.append((1000 * 0.25 * torch.log(sigmas + 1e-44))[0].clone())
        return orig(model_, x_t, sigmas, **mk)
    diffusion.denoise = denoise
    gen = RecordingGenerator(seed)
    p = dict(case)
    steps, sampler = p.pop("steps"), p.pop("sampler")
    with torch.no_grad():
        x0 = ref_kd.karras_sample(diffusion, model, shape, steps, sampler=sampler, model_kwargs=kw, device="cpu", generator=gen,
                                  callback=lambda d: cb.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}),
                                  **p)
    diffusion.denoise = orig
    return dict(sample=x0, draws=torch.stack(gen.draws), evals=torch.stack(evals), ts=torch.stack(ts), cb=cb)


def main():
    torch.set_num_threads(8)
    out = {}
    analytic_diff = ref_kd.KarrasDenoiser(sigma_data=0.5, sigma_max=80.0, sigma_min=0.002, weight_schedule="uniform")
    nets = {"unet": mg.build_edm(), "unet_plain": mg.build_edm(class_cond=False, use_scale_shift_norm=False, resblock_updown=False)}
    y = torch.tensor([871])
    for ci, (name, case) in enumerate(CASES.items()):
        seed = 1000 + ci
        res = {"analytic": run(analytic_diff, analytic, {}, case, seed, ANALYTIC_SHAPE)}
        res["unet"] = run(nets["unet"][1], nets["unet"][0], {"y": y}, case, seed, UNET_SHAPE)
        res["unet_plain"] = run(nets["unet_plain"][1], nets["unet_plain"][0], {}, case, seed, UNET_SHAPE)
        r0 = res["analytic"]
        sig = ref_kd.get_sigmas_karras(case["steps"], 0.002, 80.0, 7.0)
        out[f"{name}.sigmas"] = sig
        out[f"{name}.sigma_hat"] = torch.stack([torch.as_tensor(d.get("sigma_hat", d["sigma"])) for d in r0["cb"]])
        out[f"{name}.eval_sigma"], out[f"{name}.eval_t"] = r0["evals"], r0["ts"]
        out[f"{name}.analytic.draws"], out[f"{name}.draws"] = r0["draws"], res["unet"]["draws"]
        out[f"{name}.y"] = y
        if case["sampler"] == "ancestral":
            dn, up = ref_kd.get_ancestral_step(sig[:-1], sig[1:])
            out[f"{name}.sigma_down"], out[f"{name}.sigma_up"] = dn, up
        for m, r in res.items():
            assert len(r["draws"]) == len(r0["draws"]) and torch.equal(r["evals"], r0["evals"])
            store = torch.float32 if m == "analytic" else torch.float16
            out[f"{name}.{m}.x"] = torch.stack([d["x"] for d in r["cb"]]).to(store)
            out[f"{name}.{m}.denoised"] = torch.stack([d["denoised"] for d in r["cb"]]).to(store)
            out[f"{name}.{m}.sample"] = r["sample"]
        print(name, "NFE", len(r0["evals"]), "draws", len(r0["draws"]))
    r = run(analytic_diff, analytic, {}, dict(sampler="heun", steps=40, s_churn=40.0, s_tmin=0.05, s_tmax=50.0), 7, shape=(1, 1, 2, 2))
    out["heun40.sigmas"] = ref_kd.get_sigmas_karras(40, 0.002, 80.0, 7.0)
    out["heun40.sigma_hat"] = torch.stack([torch.as_tensor(d["sigma_hat"]) for d in r["cb"]])
    out["heun40.eval_sigma"], out["heun40.eval_t"] = r["evals"], r["ts"]
    path = os.path.join(HERE, "karras_sample.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
