"""Generate tests/golden/pd_train.npz by running the REFERENCE's KarrasDenoiser.progdist_losses (models/cm/karras_diffusion.py:243-335)
and karras_sample(sampler="progdist") (:354-420, sample_progdist :685-719).

Runs ONLY in the build container, next to make_golden.py (same reference checkout and import stubs, same formula weights):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pd.py

Fixed x_start / noise [6, 3, 16, 16] (the draws of make_golden_cd.py); num_scales S = 1, 2 and 6.  The reference draws its indices
inside the call (th.randint(0, num_scales, (N,))): `indices.<S>` is that draw, recorded by seeding torch with `seed.<S>` and drawing
the same way first.  Student and teacher diffusion both have distillation=False (the student of this mode keeps the EDM scalings);
weight schedule karras.  Arrays only:
  analytic.<norm>.<S>.loss / .t / .t2 / .t3 / .target_x   two different analytic callables as student / teacher, norm l1 and l2;
  <net>.<norm>.loss                                        the shrunken U-Nets (net = unet: class-conditional imagenet64 topology,
                                                           unet_plain) at S = 6, two distinct formula-weight sets:
                                                           formula_tensor(salt + name) with salt "" and "teacher:";
  <net>.<norm>.sep                                         (rms(denoised - target_x), rms denoised, rms target_x) of that case;
  <net>.<norm>.grad.<param>                                fp16 gradients of (loss * loss_w).mean() for the parameters listed in
                                                           <net>.grad_names (the pick of cm_train.npz);
  <net>.teacher_out_scale                                  factor on the teacher net's output layer (1 unless the formula weights
                                                           alone did not separate denoised and target_x);
  amp.<S>                                                  max over the ladder of (t / t2) |t3 - t2| / |t3 - t|: the factor by which
                                                           an error of the teacher's SECOND evaluation enters target_x;
  sample.<steps>.sigmas, sample.<steps>.<m>.x_T / .x / .denoised / .sample   karras_sample(sampler="progdist") from the recorded x_T
                                                           (generator.randn) at steps 1 and 3, m = analytic ([2, 3, 8, 8], fp32)
                                                           and unet ([1, 3, 16, 16]; callback values in fp16), sample.y its label.
target_x is a local of the reference's call: it is restated here from the recorded teacher evaluations with the reference's own
expressions (:271-272, :278-280), and the restatement is checked bit for bit against the loss the reference returned.
Conditions asserted here (and again by the tests from the stored arrays): every S = 6 draw has a sample at index 0 and one at index
S - 1 (t3 reaches sigma_min); every U-Net case has rms(denoised - target_x) >= 0.5 x max(rms denoised, rms target_x); amp.<S> <= 1.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference first on sys.path and installs its import stubs)
import models.cm.karras_diffusion as ref_kd  # noqa: E402
from oracle.weights import formula_tensor  # noqa: E402

NORMS = ("l1", "l2")
SCALES = (1, 2, 6)
N = 6
BIG_PICK = ("input_blocks.0.0.weight", "out.2.weight", "input_blocks.3.1.proj_out.weight", "output_blocks.3.0.skip_connection.weight")
SAMPLE_STEPS = (1, 3)
ANALYTIC_SHAPE, UNET_SHAPE = (2, 3, 8, 8), (1, 3, 16, 16)


def online_fn(x_in, t, **kw):
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


def teacher_fn(x_in, t, **kw):
    return 0.8 * torch.tanh(0.9 * x_in + 5e-4 * t[:, None, None, None])


class Recording(ref_kd.KarrasDenoiser):
    """The reference's diffusion with its denoise() calls recorded into a list shared by the student's and the teacher's object:
    the student at (x_t, t), then the teacher at (x_t, t) and at (x_t2, t2)."""
    calls = None

    def denoise(self, model, x_t, sigmas, **kw):
        out = super().denoise(model, x_t, sigmas, **kw)
        self.calls.append((x_t.detach().clone(), sigmas.detach().clone(), out[1].detach().clone()))
        return out


def find_seed(S):
    """The first seed whose draw has a sample at the last index (t3 = sigma_min) and one at index 0."""
    for seed in range(1000):
        torch.manual_seed(seed)
        idx = torch.randint(0, S, (N,))
        if (idx == S - 1).any() and (idx == 0).any():
            return seed, idx
    raise RuntimeError("no seed found")


def levels(idx, S, d):
    a, delta = d.sigma_max ** (1 / d.rho), d.sigma_min ** (1 / d.rho) - d.sigma_max ** (1 / d.rho)
    return (a + idx / S * delta) ** d.rho, (a + (idx + 0.5) / S * delta) ** d.rho, (a + (idx + 1) / S * delta) ** d.rho


def run(norm, S, seed, idx, online, teacher, x_start, noise, kw):
    calls = []
    student = Recording(sigma_data=0.5, weight_schedule="karras", distillation=False, loss_norm=norm)
    teacher_diffusion = Recording(sigma_data=0.5, weight_schedule="karras", distillation=False)
    student.calls = teacher_diffusion.calls = calls
    torch.manual_seed(seed)
    loss = student.progdist_losses(online, x_start, S, model_kwargs=kw, teacher_model=teacher, teacher_diffusion=teacher_diffusion,
                                   noise=noise)["loss"]
    assert len(calls) == 3
    (x_t, t, denoised), (x_t_b, t_b, _), (x_t2, t2, den2) = calls
    tt, tt2, tt3 = levels(idx, S, student)
    assert torch.equal(t, tt) and torch.equal(t_b, tt) and torch.equal(t2, tt2) and torch.equal(x_t, x_t_b), "levels differ from the draw"
    e = lambda v: v[:, None, None, None]
    with torch.no_grad():
        x_t3 = x_t2 + (x_t2 - den2) / e(t2) * e(tt3 - t2)
        target_x = x_t - e(t) * (x_t3 - x_t) / e(tt3 - t)
        diffs = (denoised - target_x).abs() if norm == "l1" else (denoised - target_x) ** 2
        again = diffs.mean(dim=[1, 2, 3]) * (t ** -2 + 1.0 / 0.5 ** 2)
    assert torch.equal(again, loss.detach()), "the restated target_x is not the reference's"
    return loss, dict(t=t, t2=t2, t3=tt3, target_x=target_x, denoised=denoised)


def rms(v):
    return float(v.double().pow(2).mean().sqrt())


def salted(net, salt, out_scale=1.0):
    sd = {k: formula_tensor(salt + k, v.shape).to(v.dtype) if torch.is_floating_point(v) else v.clone() for k, v in net.state_dict().items()}
    for k in ("out.2.weight", "out.2.bias"):
        sd[k] = sd[k] * out_scale
    net.load_state_dict(sd)
    return net


class RecordingGenerator:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.draws = []

    def randn(self, *shape, device=None):
        v = torch.randn(*shape, generator=self.g)
        self.draws.append(v.clone())
        return v.to(device)

    def randn_like(self, x):
        raise AssertionError("sample_progdist draws nothing after x_T")


def sample(diffusion, model, kw, steps, seed, shape):
    cb = []
    gen = RecordingGenerator(seed)
    with torch.no_grad():
        x0 = ref_kd.karras_sample(diffusion, model, shape, steps, sampler="progdist", model_kwargs=kw, device="cpu", generator=gen,
                                  callback=lambda d: cb.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}))
    assert len(gen.draws) == 1 and len(cb) == steps and all("sigma_hat" not in d for d in cb)
    return dict(sample=x0, x_T=gen.draws[0], cb=cb)


def main():
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(2025)
    x_start = torch.rand(N, 3, 16, 16, generator=g) * 2 - 1
    noise = torch.randn(N, 3, 16, 16, generator=g)
    loss_w = torch.rand(N, generator=g) + 0.5
    y = torch.tensor([3, 977, 0, 511, 42, 999])
    out = dict(x_start=x_start, noise=noise, loss_w=loss_w, y=y, num_scales=np.array(SCALES))
    seeds, draws = {}, {}
    plain_d = ref_kd.KarrasDenoiser(sigma_data=0.5)
    for S in SCALES:
        seeds[S], draws[S] = find_seed(S)
        out[f"seed.{S}"], out[f"indices.{S}"] = np.array(seeds[S]), draws[S]
        t, t2, t3 = levels(torch.arange(S), S, plain_d)
        amp = float(((t / t2) * (t3 - t2).abs() / (t3 - t).abs()).max())
        assert amp <= 1.0, (S, amp)
        out[f"amp.{S}"] = np.array(amp)
        assert abs(float(t3[-1]) - 0.002) < 1e-6
        print(f"S = {S}: seed {seeds[S]}, indices {draws[S].tolist()}, teacher amplification {amp:.3f}")

    for norm in NORMS:
        for S in SCALES:
            loss, rec = run(norm, S, seeds[S], draws[S], online_fn, teacher_fn, x_start, noise, {})
            pre = f"analytic.{norm}.{S}"
            out[pre + ".loss"] = loss
            for k in ("t", "t2", "t3", "target_x"):
                out[f"{pre}.{k}"] = rec[k]

    S = 6
    for tag, over in (("unet", {}), ("unet_plain", dict(class_cond=False, use_scale_shift_norm=False, resblock_updown=False))):
        kw = dict(y=y) if over.get("class_cond", True) else {}
        online = salted(mg.build_edm(**over)[0], "")
        names = [n for n, p in online.named_parameters() if p.numel() <= 4096 or n in BIG_PICK]
        out[f"{tag}.grad_names"] = np.array(names)
        scale = 1.0
        while True:
            teacher = salted(mg.build_edm(**over)[0], "teacher:", scale)
            for p in teacher.parameters():
                p.requires_grad_(False)
            res, ok = {}, True
            for norm in NORMS:
                online.zero_grad()
                loss, rec = run(norm, S, seeds[S], draws[S], online, teacher, x_start, noise, kw)
                (loss * loss_w).mean().backward()
                sep = (rms(rec["denoised"] - rec["target_x"]), rms(rec["denoised"]), rms(rec["target_x"]))
                ok = ok and sep[0] >= 0.5 * max(sep[1], sep[2])
                grads = {n: p.grad.detach().clone() for n, p in online.named_parameters() if n in names}
                res[norm] = (loss.detach(), sep, grads, rec)
            if ok:
                break
            scale *= 2.0
            assert scale <= 16.0, "the teacher's output layer scale did not separate denoised and target_x"
        out[f"{tag}.teacher_out_scale"] = np.array(scale)
        for norm, (loss, sep, grads, rec) in res.items():
            pre = f"{tag}.{norm}"
            out[pre + ".loss"], out[pre + ".sep"] = loss, np.array(sep)
            assert (rec["t3"] == rec["t3"].min()).any() and abs(float(rec["t3"].min()) - 0.002) < 1e-6      # t3 reaches sigma_min
            for n in names:
                g16 = grads[n].to(torch.float16)
                assert torch.isfinite(g16).all(), (pre, n)
                out[f"{pre}.grad.{n}"] = g16
            print(f"{pre}: teacher_out_scale {scale}  loss {loss.tolist()}  sep {sep[0]:.3f} vs max {max(sep[1], sep[2]):.3f}")

    analytic_diff = ref_kd.KarrasDenoiser(sigma_data=0.5, sigma_max=80.0, sigma_min=0.002, weight_schedule="uniform")
    unet, unet_diff = mg.build_edm()
    ys = torch.tensor([871])
    out["sample.y"] = ys
    for si, steps in enumerate(SAMPLE_STEPS):
        out[f"sample.{steps}.sigmas"] = ref_kd.get_sigmas_karras(steps + 1, 0.002, 80.0, 7.0)
        for m, r in (("analytic", sample(analytic_diff, online_fn, {}, steps, 3000 + si, ANALYTIC_SHAPE)),
                     ("unet", sample(unet_diff, unet, {"y": ys}, steps, 3000 + si, UNET_SHAPE))):
            store = torch.float32 if m == "analytic" else torch.float16
            pre = f"sample.{steps}.{m}"
            out[pre + ".x_T"], out[pre + ".sample"] = r["x_T"], r["sample"]
            out[pre + ".x"] = torch.stack([d["x"] for d in r["cb"]]).to(store)
            out[pre + ".denoised"] = torch.stack([d["denoised"] for d in r["cb"]]).to(store)
            assert [float(d["sigma"]) for d in r["cb"]] == [float(s) for s in out[f"sample.{steps}.sigmas"][:steps]]
    mg.save("pd_train", **out)
    assert os.path.getsize(os.path.join(HERE, "pd_train.npz")) < (1 << 20), "pd_train.npz exceeds the size limit of a committed file"


if __name__ == "__main__":
    main()
