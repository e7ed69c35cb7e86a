"""Generate tests/golden/cm_sample.npz by running the REFERENCE's consistency-model samplers and editing loops
(models/cm/karras_diffusion.py: karras_sample :354-420 with sample_onestep / stochastic_iterative_sampler :644-683;
iterative_colorization / iterative_inpainting / iterative_superres :722-951).

Runs ONLY in the build container, next to make_golden.py (same reference checkout and import stubs, same formula weights) and
make_golden_karras.py (same recording generator and analytic model):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cm.py

Two reference defects are worked around here:
  * the iterative_* loops call dist_util.dev(), but the module's `from . import dist_util` is commented out (:12): a CPU
    stand-in is set as the module's dist_util attribute;
  * iterative_inpainting hard-codes ImageFont.truetype("arial.ttf", 250): truetype is patched to the TrueType font FONT, which
    exists in the build container; the fixture records the font's file name (`font`, as uint8 codes).

Every Gaussian draw goes through the recording generator.  Every network evaluation goes through a wrapping distiller, which
records its input x, sigma, the time input 250 ln(sigma + 1e-44) and the denoised output it returns.  Per case and model m the
fixture holds, as arrays only:
  <case>.eval_sigma / .eval_t (per evaluation); <case>.<m>.denoised [nfe, B, C, H, W]; <case>.<m>.out (the sampler's return:
  karras_sample's clamped sample, or the editing loop's x); <case>.y (class-conditional U-Net label);
  for m = analytic (tanh(0.7 x_in + 1e-3 t), 2 x 3 x 8 x 8, superres 2 x 3 x 16 x 16, inpainting 14 x 3 x 8 x 8; fp32):
  also .x_eval (the distiller's input x per evaluation), .draws, and for the editing cases .images_in (the input images) and
  .images (the returned degraded view);
  for the two shrunken U-Nets with distillation=True (unet: class-conditional, unet_plain; 1 x 3 x 16 x 16, inpainting
  14 x 3 x 16 x 16): .denoised and .out in fp16, and, shared by both, <case>.draws (fp32), <case>.images_in / .images (fp16).  Also: Q3 / Q64 (the reference's colour and patch bases,
fp32) and mask256.g0 / .g1 (the two groups of the 256x256 letter mask, np.packbits of the [3, 256, 256] booleans), derived
from the returned images of one inpainting run at 256 with images = 1 and a single evaluation.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference first on sys.path and installs its import stubs)
import make_golden_karras as mk  # noqa: E402  (RecordingGenerator, analytic)
import models.cm.karras_diffusion as ref_kd  # noqa: E402

FONT = "/usr/share/fonts/truetype/dejavu/DejaVuSans.ttf"
ANALYTIC_SHAPE, ANALYTIC_SUPERRES_SHAPE, UNET_SHAPE = (2, 3, 8, 8), (2, 3, 16, 16), (1, 3, 16, 16)
CASES = {   # name: (kind, ts, steps)
    "onestep": ("onestep", None, 40),
    "multistep_0_22_39": ("multistep", (0, 22, 39), 40),
    "multistep_0_10_20": ("multistep", (0, 10, 20), 40),
    "colorization": ("colorization", (0, 22, 39), 40),
    "superres": ("superres", (0, 22, 39), 40),
    "inpainting": ("inpainting", (0, 10, 20), 40),
}


def install_workarounds():
    ref_kd.dist_util = types.SimpleNamespace(dev=lambda: "cpu")
    from PIL import ImageFont
    orig = ImageFont.truetype
    ImageFont.truetype = lambda font=None, size=10, *a, **k: orig(FONT if font == "arial.ttf" else font, size, *a, **k)


def make_distiller(diffusion, model, kw, rec):
    def distiller(x_t, sigma):
        rec["x"].append(x_t.clone())
        rec["sigma"].append(sigma[0].clone())
        rec["t"].append((1000 * 0.25 * torch.log(sigma + 1e-44))[0].clone())
        _, den = diffusion.denoise(model, x_t, sigma, **kw)
        den = den.clamp(-1, 1)                 # karras_sample's denoiser with clip_denoised=True (:404-410)
        rec["den"].append(den.clone())
        return den
    return distiller


def run(diffusion, model, kw, case, seed, shape):
    kind, ts, steps = CASES[case]
    if kind == "inpainting":
        shape = (14,) + tuple(shape[1:])
    rec = {"x": [], "sigma": [], "t": [], "den": []}
    gen = mk.RecordingGenerator(seed)
    res = {}
    with torch.no_grad():
        if kind in ("onestep", "multistep"):
            orig = diffusion.denoise

            def denoise(model_, x_t, sigmas, **mk_):      # karras_sample's own closure calls this; record through it
                rec["x"].append(x_t.clone())
                rec["sigma"].append(sigmas[0].clone())
                rec["t"].append((1000 * 0.25 * torch.log(sigmas + 1e-44))[0].clone())
                r = orig(model_, x_t, sigmas, **mk_)
                rec["den"].append(r[1].clamp(-1, 1).clone())
                return r
            diffusion.denoise = denoise
            res["out"] = ref_kd.karras_sample(diffusion, model, shape, steps, model_kwargs=kw, device="cpu", generator=gen,
                                              sampler=kind, ts=ts)
            diffusion.denoise = orig
        else:
            g = torch.Generator().manual_seed(seed + 500)
            images = (torch.rand(shape, generator=g) * 2 - 1)
            x = gen.randn(*shape) * 80.0
            fn = {"colorization": ref_kd.iterative_colorization, "superres": ref_kd.iterative_superres,
                  "inpainting": ref_kd.iterative_inpainting}[kind]
            out, imgs = fn(make_distiller(diffusion, model, kw, rec), images, x, ts, steps=steps, generator=gen)
            res.update(out=out, images=imgs, images_in=images)
    res.update(draws=torch.stack(gen.draws), x_eval=torch.stack(rec["x"]), denoised=torch.stack(rec["den"]),
               sigma=torch.stack(rec["sigma"]), t=torch.stack(rec["t"]))
    return res


def letter_mask():
    diff = ref_kd.KarrasDenoiser(sigma_data=0.5, sigma_max=80.0, sigma_min=0.002, weight_schedule="uniform", distillation=True)
    shape = (14, 3, 256, 256)
    distiller = make_distiller(diff, mk.analytic, {}, {"x": [], "sigma": [], "t": [], "den": []})
    with torch.no_grad():
        _, imgs = ref_kd.iterative_inpainting(distiller, torch.ones(shape), torch.zeros(shape), (0, 39), steps=40,
                                              generator=mk.RecordingGenerator(5))
    m = (imgs + 1) / 2
    assert torch.equal(m, m.round())
    g0, g1 = m[0] > 0.5, m[7] > 0.5
    for i in range(14):
        assert torch.equal(m[i] > 0.5, g0 if i < 7 else g1)
    return np.packbits(g0.numpy()), np.packbits(g1.numpy())


def main():
    torch.set_num_threads(8)
    install_workarounds()
    out = {}
    analytic_diff = ref_kd.KarrasDenoiser(sigma_data=0.5, sigma_max=80.0, sigma_min=0.002, weight_schedule="uniform",
                                          distillation=True)
    nets = {"unet": mg.build_edm(distillation=True),
            "unet_plain": mg.build_edm(class_cond=False, use_scale_shift_norm=False, resblock_updown=False, distillation=True)}
    for ci, case in enumerate(CASES):
        seed = 2000 + ci
        res = {"analytic": run(analytic_diff, mk.analytic, {}, case, seed,
                               ANALYTIC_SUPERRES_SHAPE if case == "superres" else ANALYTIC_SHAPE)}
        y = torch.tensor([871] * (14 if CASES[case][0] == "inpainting" else 1))
        res["unet"] = run(nets["unet"][1], nets["unet"][0], {"y": y}, case, seed, UNET_SHAPE)
        res["unet_plain"] = run(nets["unet_plain"][1], nets["unet_plain"][0], {}, case, seed, UNET_SHAPE)
        r0 = res["analytic"]
        out[f"{case}.eval_sigma"], out[f"{case}.eval_t"] = r0["sigma"], r0["t"]
        out[f"{case}.y"] = y
        for m, r in res.items():
            assert torch.equal(r["sigma"], r0["sigma"]) and len(r["draws"]) == len(r0["draws"])
            if m == "analytic":
                for k in ("x_eval", "denoised", "draws", "out", "images", "images_in"):
                    if k in r:
                        out[f"{case}.analytic.{k}"] = r[k]
            else:
                out[f"{case}.{m}.denoised"], out[f"{case}.{m}.out"] = r["denoised"].half(), r["out"].half()
        ru = res["unet"]       # the two U-Nets share the draws, input images and degraded view (same seed and shape)
        for k in ("draws", "images", "images_in"):
            if k in ru:
                assert torch.equal(ru[k], res["unet_plain"][k])
                out[f"{case}.{k}"] = ru[k] if k == "draws" else ru[k].half()
        print(case, "NFE", len(r0["sigma"]), "draws", len(r0["draws"]))
    out["Q3"], out["Q64"] = reference_bases()
    out["mask256.g0"], out["mask256.g1"] = letter_mask()
    out["font"] = np.frombuffer(os.path.basename(FONT).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "cm_sample.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def reference_bases():
    """The reference's Q matrices, captured from its own runs: the einsum calls of iterative_colorization and iterative_superres
    see Q as their second operand."""
    seen = {}
    orig = torch.einsum

    def spy(eq, *ops):
        if eq in ("bchw,cd->bdhw", "bcnd,de->bcne"):
            seen.setdefault(eq, ops[1].clone())
        return orig(eq, *ops)
    diff = ref_kd.KarrasDenoiser(sigma_data=0.5, distillation=True)
    ref_kd.th.einsum = spy
    try:
        shape = (1, 3, 8, 8)
        for fn in (ref_kd.iterative_colorization, ref_kd.iterative_superres):
            d = make_distiller(diff, mk.analytic, {}, {"x": [], "sigma": [], "t": [], "den": []})
            with torch.no_grad():
                fn(d, torch.zeros(shape), torch.zeros(shape), (0, 39), steps=40, generator=mk.RecordingGenerator(1))
    finally:
        ref_kd.th.einsum = orig
    return seen["bchw,cd->bdhw"], seen["bcnd,de->bcne"]


if __name__ == "__main__":
    main()
