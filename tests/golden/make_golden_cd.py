"""Generate tests/golden/cm_train.npz and cm_train_plain.npz (the unet_plain.* arrays) by running the REFERENCE's KarrasDenoiser.consistency_losses (models/cm/karras_diffusion.py:
108-241) and create_ema_and_scales_fn (models/cm/script_util.py:161-219).

Runs ONLY in the build container, next to make_golden.py (same reference checkout and import stubs, same formula weights):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cd.py

Fixed x_start / noise [6, 3, 16, 16]; ladders of num_scales 6 and 18.  The reference draws its indices inside the call
(th.randint(0, num_scales - 1, (N,))): `indices.<S>` is that draw, recorded by seeding torch with `seed.<S>` and drawing the same
way first.  The student diffusion has distillation=True (boundary-condition scalings), the teacher's has not; weight schedule karras.
Modes: cd (teacher given: Heun) and ct (no teacher: Euler on x_start).  Arrays only:
  analytic.<mode>.<norm>.<S>.loss / .t / .t2 / .x_t2     three different analytic callables as online / target / teacher;
  <net>.<mode>.<norm>.loss                                the shrunken U-Nets (net = unet: class-conditional imagenet64 topology,
                                                          unet_plain) on the coarse ladder S = 6, three distinct formula-weight
                                                          sets: formula_tensor(salt + name) with salt "", "target:", "teacher:";
  <net>.<mode>.<norm>.sep                                 (rms(distiller - target), rms distiller, rms target) of that case;
  <net>.<mode>.<norm>.grad.<param>                        fp16 gradients of (loss * loss_w).mean() for the parameters listed in
                                                          <net>.grad_names (the pick of edm_dsm.npz);
  <net>.target_out_scale                                  factor on the target net's output layer (1 unless the formula weights
                                                          alone did not separate distiller and target);
  ema_scales.<pair>.ema / .scales / ema_scales.steps      ema_and_scales_fn of the four mode pairs.
Conditions asserted here (and again by the tests from the stored arrays): every U-Net case has rms(distiller - target) >= 0.5 x
max(rms distiller, rms target) — the loss is a difference of two network outputs and must not sit in their bf16 noise — and every
case has at least one sample whose t2 is the last ladder level (the boundary, where the target is x_t2 up to c_out ~ 0).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference first on sys.path and installs its import stubs)
import models.cm.karras_diffusion as ref_kd  # noqa: E402
import models.cm.script_util as ref_su  # noqa: E402
from oracle.weights import formula_tensor  # noqa: E402

NORMS = ("l1", "l2", "l2-32")
MODES = ("cd", "ct")
SCALES = (6, 18)
N = 6
BIG_PICK = ("input_blocks.0.0.weight", "out.2.weight", "input_blocks.3.1.proj_out.weight", "output_blocks.3.0.skip_connection.weight")
EMA_PAIRS = {"fixed_fixed": dict(target_ema_mode="fixed", start_ema=0.95, scale_mode="fixed", start_scales=40, end_scales=40),
             "fixed_progressive": dict(target_ema_mode="fixed", start_ema=0.9, scale_mode="progressive", start_scales=2, end_scales=150),
             "adaptive_progressive": dict(target_ema_mode="adaptive", start_ema=0.95, scale_mode="progressive", start_scales=2,
                                          end_scales=150),
             "fixed_progdist": dict(target_ema_mode="fixed", start_ema=0.0, scale_mode="progdist", start_scales=16, end_scales=16)}
EMA_STEPS = [0, 1, 2, 5, 10, 49, 50, 51, 99, 100, 149, 150, 199, 200, 250, 299, 300, 400, 500, 750, 999, 1000]
EMA_TOTAL, EMA_PER_ITER = 1000, 50


def online_fn(x_in, t, **kw):
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


def target_fn(x_in, t, **kw):
    return torch.tanh(0.5 * x_in - 2e-3 * t[:, None, None, None] + 0.1)


def teacher_fn(x_in, t, **kw):
    return 0.8 * torch.tanh(0.9 * x_in + 5e-4 * t[:, None, None, None])


class Recording(ref_kd.KarrasDenoiser):
    """The reference's diffusion with its denoise() calls recorded: the first is the online net at (x_t, t), the last the
    target at (x_t2, t2)."""

    def denoise(self, model, x_t, sigmas, **kw):
        out = super().denoise(model, x_t, sigmas, **kw)
        self.calls.append((x_t.detach().clone(), sigmas.detach().clone(), out[1].detach().clone()))
        return out


def find_seed(S):
    """The first seed whose draw has a sample at the last usable index (t2 = the last ladder level) and one at index 0."""
    for seed in range(1000):
        torch.manual_seed(seed)
        idx = torch.randint(0, S - 1, (N,))
        if (idx == S - 2).any() and (idx == 0).any():
            return seed, idx
    raise RuntimeError("no seed found")


def run(student, mode, S, seed, online, target, teacher, teacher_diffusion, x_start, noise, kw):
    student.calls = []
    torch.manual_seed(seed)
    terms = student.consistency_losses(online, x_start, S, model_kwargs=kw, target_model=target,
                                       teacher_model=teacher if mode == "cd" else None,
                                       teacher_diffusion=teacher_diffusion if mode == "cd" else None, noise=noise)
    (x_t, t, distiller), (x_t2, t2, tgt) = student.calls[0], student.calls[-1]
    return terms["loss"], dict(t=t, t2=t2, x_t2=x_t2, distiller=distiller, target=tgt)


def rms(v):
    return float(v.double().pow(2).mean().sqrt())


def salted(net, salt, out_scale=1.0):
    sd = {k: formula_tensor(salt + k, v.shape).to(v.dtype) if torch.is_floating_point(v) else v.clone() for k, v in net.state_dict().items()}
    for k in ("out.2.weight", "out.2.bias"):
        sd[k] = sd[k] * out_scale
    net.load_state_dict(sd)
    return net


def main():
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(2025)
    x_start = torch.rand(N, 3, 16, 16, generator=g) * 2 - 1
    noise = torch.randn(N, 3, 16, 16, generator=g)
    loss_w = torch.rand(N, generator=g) + 0.5
    y = torch.tensor([3, 977, 0, 511, 42, 999])
    out = dict(x_start=x_start, noise=noise, loss_w=loss_w, y=y, num_scales=np.array(SCALES))
    seeds = {}
    for S in SCALES:
        seeds[S], idx = find_seed(S)
        out[f"seed.{S}"], out[f"indices.{S}"] = np.array(seeds[S]), idx
    teacher_diffusion = ref_kd.KarrasDenoiser(sigma_data=0.5, weight_schedule="karras", distillation=False)

    def student(norm):
        return Recording(sigma_data=0.5, weight_schedule="karras", distillation=True, loss_norm=norm)

    for mode in MODES:
        for norm in NORMS:
            for S in SCALES:
                loss, rec = run(student(norm), mode, S, seeds[S], online_fn, target_fn, teacher_fn, teacher_diffusion, x_start, noise, {})
                pre = f"analytic.{mode}.{norm}.{S}"
                out[pre + ".loss"], out[pre + ".t"], out[pre + ".t2"], out[pre + ".x_t2"] = loss, rec["t"], rec["t2"], rec["x_t2"]
                # the table the package builds (arange over the ladder, then the gather) is the reference's per-sample expression
                idx = out[f"indices.{S}"]
                ar = torch.arange(S)
                tab = (80.0 ** (1 / 7.0) + ar / (S - 1) * (0.002 ** (1 / 7.0) - 80.0 ** (1 / 7.0))) ** 7.0
                assert torch.equal(tab[idx], rec["t"]) and torch.equal(tab[idx + 1], rec["t2"]), "ladder table differs from the draw"
                assert (rec["t2"] == tab[S - 1]).any()

    S = SCALES[0]
    for tag, over in (("unet", {}), ("unet_plain", dict(class_cond=False, use_scale_shift_norm=False, resblock_updown=False))):
        kw = dict(y=y) if over.get("class_cond", True) else {}
        online = salted(mg.build_edm(**over)[0], "")
        teacher = salted(mg.build_edm(**over)[0], "teacher:")
        for p in teacher.parameters():
            p.requires_grad_(False)
        names = [n for n, p in online.named_parameters() if p.numel() <= 4096 or n in BIG_PICK]
        out[f"{tag}.grad_names"] = np.array(names)
        scale = 1.0
        while True:
            target = salted(mg.build_edm(**over)[0], "target:", scale)
            for p in target.parameters():
                p.requires_grad_(False)
            res, ok = {}, True
            for mode in MODES:
                for norm in NORMS:
                    online.zero_grad()
                    loss, rec = run(student(norm), mode, S, seeds[S], online, target, teacher, teacher_diffusion, x_start, noise, kw)
                    (loss * loss_w).mean().backward()
                    sep = (rms(rec["distiller"] - rec["target"]), rms(rec["distiller"]), rms(rec["target"]))
                    ok = ok and sep[0] >= 0.5 * max(sep[1], sep[2])
                    grads = {n: p.grad.detach().clone() for n, p in online.named_parameters() if n in names}
                    res[mode, norm] = (loss.detach(), sep, grads, rec)
            if ok:
                break
            scale *= 2.0
            assert scale <= 16.0, "the target's output layer scale did not separate distiller and target"
        out[f"{tag}.target_out_scale"] = np.array(scale)
        for (mode, norm), (loss, sep, grads, rec) in res.items():
            pre = f"{tag}.{mode}.{norm}"
            out[pre + ".loss"], out[pre + ".sep"] = loss, np.array(sep)
            assert (rec["t2"] == rec["t2"].min()).any() and abs(float(rec["t2"].min()) - 0.002) < 1e-6      # the boundary level
            for n in names:
                g16 = grads[n].to(torch.float16)
                assert torch.isfinite(g16).all(), (pre, n)
                out[f"{pre}.grad.{n}"] = g16
            print(f"{pre}: loss {loss.tolist()}  sep {sep[0]:.3f} vs max {max(sep[1], sep[2]):.3f}")

    steps = np.array(EMA_STEPS)
    out["ema_scales.steps"] = steps
    for name, kw in EMA_PAIRS.items():
        fn = ref_su.create_ema_and_scales_fn(total_steps=EMA_TOTAL, distill_steps_per_iter=EMA_PER_ITER, **kw)
        vals = [fn(int(s)) for s in steps]
        out[f"ema_scales.{name}.ema"] = np.array([v[0] for v in vals], dtype=np.float64)
        out[f"ema_scales.{name}.scales"] = np.array([v[1] for v in vals], dtype=np.int64)
    # two files, each under the size limit of a committed file: the plain U-Net's arrays go to cm_train_plain.npz
    plain = {k: v for k, v in out.items() if k.startswith("unet_plain.")}
    mg.save("cm_train", **{k: v for k, v in out.items() if k not in plain})
    mg.save("cm_train_plain", **plain)


if __name__ == "__main__":
    main()
