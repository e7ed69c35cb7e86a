"""EDM denoising score-matching training on the GPU: the four kernels of csrc/edm_dsm.hip against float64 on the same fp32
operands, run-to-run bits, training_losses on the shrunken U-Nets against the reference (tests/golden/edm_dsm.npz), ResBlock
dropout against torch autograd through the pinned oracle with the same masks, and TrainLoop (EMA, lr anneal, overflow, resume).

Bounds: elementwise kernel results within 16 u M of float64 (u = 2^-24, M = the magnitude of the operands that meet in the
result); per-sample sums within 64 u of their magnitude; the network terms within the 1.5e-2 the shrunken net's forward is held
to (test_hip_edm.py); parameter gradients cosine >= 0.995 and norm within 5 % (test_edm_trainer.py).
"""
import math
import os

import numpy as np
import pytest
import torch

from ew_shapes import SECOND_TRIP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SCHEDULES = ("snr", "snr+1", "karras", "truncated-snr", "uniform")
TINY_KW = dict(image_size=16, class_cond=True, learn_sigma=False, num_channels=64, num_res_blocks=1, channel_mult="1,2",
               num_heads=4, num_head_channels=64, num_heads_upsample=-1, attention_resolutions="8", dropout=0.0,
               use_checkpoint=False, use_scale_shift_norm=True, resblock_updown=True, use_fp16=False,
               use_new_attention_order=False, weight_schedule="karras")
PLAIN = dict(class_cond=False, use_scale_shift_norm=False, resblock_updown=False)


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "edm_dsm.npz"), allow_pickle=False)


def build(over=None, **kw2):
    from models.cm.script_util import create_model_and_diffusion
    from oracle.weights import formula_tensor
    kw = dict(TINY_KW)
    kw.update(over or {})
    kw.update(kw2)
    net, diffusion = create_model_and_diffusion(**kw)
    sd = {k: formula_tensor(k, v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    return net.to(DEV).eval(), diffusion, sd


def scalings64(s, sd=0.5, smin=float(np.float32(0.002)), distill=False):      # sigma_min as the fp32 scalar torch subtracts
    s = s.double()
    if distill:
        c_skip = sd ** 2 / ((s - smin) ** 2 + sd ** 2)
        c_out = (s - smin) * sd / (s ** 2 + sd ** 2) ** 0.5
    else:
        c_skip = sd ** 2 / (s ** 2 + sd ** 2)
        c_out = s * sd / (s ** 2 + sd ** 2) ** 0.5
    return c_skip, c_out, 1 / (s ** 2 + sd ** 2) ** 0.5


def weights64(ws, s, sd=0.5):
    snr = s.double() ** -2
    return {"snr": snr, "snr+1": snr + 1, "karras": snr + 1 / sd ** 2, "truncated-snr": snr.clamp(min=1.0),
            "uniform": torch.ones_like(snr)}[ws]


def operands(N, CHW, seed):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(N, CHW, generator=gen) * 2 - 1
    noise = torch.randn(N, CHW, generator=gen)
    F = torch.randn(N, CHW, generator=gen)
    sig = torch.exp(torch.linspace(math.log(0.002), math.log(80.0), N))
    return x0, noise, F, sig


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("CHW", [3 * 16 * 16, 3 * 64 * 64, 4 * 3 * 33, math.prod(SECOND_TRIP)])
@pytest.mark.parametrize("distill", [False, True])
def test_dsm_kernels_vs_fp64(ops, CHW, distill):
    N = 1 if CHW == math.prod(SECOND_TRIP) else 7
    x0, noise, F, sig = operands(N, CHW, 5 + CHW)
    d = lambda t: t.to(DEV).contiguous()
    x_in, t = ops.edm_dsm_prep(d(x0), d(noise), d(sig))
    c_skip, c_out, c_in = [v[:, None] for v in scalings64(sig, distill=distill)]
    xt = x0.double() + noise.double() * sig.double()[:, None]
    ref = c_in * xt
    M = c_in * (x0.double().abs() + (noise.double() * sig.double()[:, None]).abs())
    assert ((x_in.cpu().double() - ref).abs() <= 16 * U * M + 1e-30).all()
    assert ((t.cpu().double() - 250 * torch.log(sig.double())).abs() <= 16 * U * 250 * torch.log(sig.double()).abs() + 1e-4).all()
    gm, gx = torch.randn(N), torch.randn(N)
    worst = 0.0
    for ws in SCHEDULES:
        w = weights64(ws, sig)[:, None]
        xs, mse = ops.edm_dsm_loss_fwd(d(F), d(x0), d(noise), d(sig), ws, distillation=distill)
        den = c_out * F.double() + c_skip * xt
        e = den - x0.double()
        Me = (c_out * F.double()).abs() + (c_skip * xt).abs() + x0.double().abs()
        ref_xs, ref_mse = (e ** 2).mean(1), (w * e ** 2).mean(1)
        bound_xs = 64 * U * (Me * (e.abs() + 16 * U * Me)).mean(1) * 2 + 1e-30
        assert ((xs.cpu().double() - ref_xs).abs() <= bound_xs).all(), ws
        assert ((mse.cpu().double() - ref_mse).abs() <= w[:, 0] * bound_xs).all(), ws
        worst = max(worst, ((xs.cpu().double() - ref_xs).abs() / bound_xs).max().item())
        for gm_, gx_ in ((gm, gx), (gm, None), (None, gx)):
            dF = ops.edm_dsm_loss_bwd(None if gm_ is None else d(gm_), None if gx_ is None else d(gx_), d(F), d(x0), d(noise), d(sig),
                                      ws, distillation=distill)
            a = (0 if gm_ is None else gm_.double()[:, None] / CHW * w) + (0 if gx_ is None else gx_.double()[:, None] / CHW)
            ref_dF = 2 * e * a * c_out
            Ma = ((0 if gm_ is None else gm_.double().abs()[:, None] / CHW * w) + (0 if gx_ is None else gx_.double().abs()[:, None] / CHW))
            bound = 16 * U * 2 * Me * Ma * c_out.abs() + 1e-38
            assert ((dF.cpu().double() - ref_dF).abs() <= bound).all(), (ws, gm_ is None, gx_ is None)
    print(f"dsm loss_fwd worst |err| / bound = {worst:.3e} (CHW {CHW}, distill {distill})")


def test_dsm_kernels_reproducible(ops):
    x0, noise, F, sig = [t.to(DEV) for t in operands(16, 3 * 64 * 64, 3)]
    gm = torch.rand(16, device=DEV)
    a = ops.edm_dsm_loss_fwd(F, x0, noise, sig, "karras")
    b = ops.edm_dsm_loss_fwd(F, x0, noise, sig, "karras")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops.edm_dsm_loss_bwd(gm, gm, F, x0, noise, sig, "snr"), ops.edm_dsm_loss_bwd(gm, gm, F, x0, noise, sig, "snr"))


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_ema_update_vs_fp64_and_torch(ops, K):
    from models.cm.nn import update_ema_rates
    gen = torch.Generator().manual_seed(K)
    shapes = [(4096 * 3,), (37,), (192, 192, 3, 3), (5,), (4097,)] + [(64 + i,) for i in range(70)]   # > DXMI_MT_MAX tensors
    src = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
    base = torch.randn(4098 * 2, generator=gen).to(DEV)
    src.append(base[1:4098])            # 4-byte aligned only: the dword path
    rates = [0.9999, 0.999, 0.99, 0.5][:K]
    tg = [[torch.randn(s.shape, generator=gen).to(DEV) for s in src] for _ in rates]
    before = [[t.clone() for t in ts] for ts in tg]
    flag = torch.ones(1, device=DEV)
    update_ema_rates(tg, src, rates, found_inf=flag)         # overflow step: untouched
    for ts, bs in zip(tg, before):
        assert all(torch.equal(a, b) for a, b in zip(ts, bs))
    flag.zero_()
    update_ema_rates(tg, src, rates, found_inf=flag)
    for k, r in enumerate(rates):
        for t, b, s in zip(tg[k], before[k], src):
            ref64 = np.float32(r).astype(np.float64) * b.double().cpu() + np.float32(1 - r).astype(np.float64) * s.double().cpu()
            M = b.double().cpu().abs() * r + s.double().cpu().abs() * (1 - r)
            assert ((t.cpu().double() - ref64).abs() <= 4 * U * M + 1e-38).all()
            tt = b.clone().mul_(r).add_(s, alpha=1 - r)
            assert ((t - tt).abs() <= 2 * U * M.to(DEV).float() + 1e-38).all()


def test_update_ema_two_rates_vs_reference(ops, g):
    from models.cm.nn import update_ema
    for k, rate in enumerate(g["ema.rates"]):
        tgt = [torch.from_numpy(g[f"ema.{k}.before.{i}"]).to(DEV) for i in range(4)]
        for it in range(3):
            update_ema(tgt, [torch.from_numpy(g[f"ema.src.{it}.{i}"]).to(DEV) for i in range(4)], rate=float(rate))
        for i in range(4):
            ref = torch.from_numpy(g[f"ema.{k}.after.{i}"])
            assert ((tgt[i].cpu() - ref).abs() <= 8 * U * ref.abs() + 1e-6 * U).all()


# ------------------------------------------------------------------------------------------ training_losses
def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(a @ b / (a.norm() * b.norm() + 1e-300))


@pytest.mark.parametrize("tag", ["unet", "unet_plain"])
def test_training_losses_vs_reference(ops, g, tag):
    from models.cm.karras_diffusion import KarrasDenoiser
    net, _, _ = build(PLAIN if tag == "unet_plain" else None)
    kw = {"y": torch.from_numpy(g["y"]).to(DEV)} if tag == "unet" else {}
    x0, noise, sig = (torch.from_numpy(g[k]).to(DEV) for k in ("x_start", "noise", "sigmas"))
    worst = 0.0
    with torch.no_grad():
        for ws in SCHEDULES:
            t = KarrasDenoiser(sigma_data=0.5, weight_schedule=ws).training_losses(net, x0, sig, model_kwargs=kw, noise=noise)
            for term in ("xs_mse", "mse"):
                ref = torch.from_numpy(g[f"{tag}.{ws}.{term}"]).double()
                r = ((t[term].cpu().double() - ref).norm() / ref.norm()).item()
                worst = max(worst, r)
                assert r < 1.5e-2, (ws, term, r)
    for p in net.parameters():
        p.requires_grad_(True)
    d = KarrasDenoiser(sigma_data=0.5, weight_schedule="karras")
    t = d.training_losses(net, x0, sig, model_kwargs=kw, noise=noise)
    assert t["loss"].requires_grad
    (t["loss"] * torch.from_numpy(g["loss_w"]).to(DEV)).mean().backward()
    P = dict(net.named_parameters())
    wc, wn = ("", 1.0), ("", 0.0)
    for n in g[f"{tag}.grad_names"]:
        ref = torch.from_numpy(g[f"{tag}.grad.{n}"]).float()
        got = P[str(n)].grad.cpu()
        assert got.shape == ref.shape
        if ref.norm() < 1e-6 * max(1.0, got.norm().item()):
            continue
        c, nr = _cos(got, ref), (got.norm() / ref.norm()).item()
        wc = min(wc, (str(n), c), key=lambda v: v[1])
        wn = max(wn, (str(n), abs(nr - 1)), key=lambda v: v[1])
        assert c >= 0.995 and abs(nr - 1) <= 0.05, (n, c, nr)
    print(f"{tag}: terms worst rel-L2 {worst:.3e} (bound 1.5e-2); gradient worst cosine {wc[1]:.5f} ({wc[0]}), "
          f"worst norm ratio deviation {wn[1]:.4f} ({wn[0]})")


def test_training_losses_refuses_grad_inputs(ops):
    from models.cm.karras_diffusion import KarrasDenoiser
    net, _, _ = build(PLAIN)
    x0 = torch.zeros(2, 3, 16, 16, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError):
        KarrasDenoiser().training_losses(net, x0, torch.ones(2, device=DEV))


# ------------------------------------------------------------------------------------------ dropout
def test_dropout_zero_train_equals_eval(ops):
    """p = 0 in train mode runs no dropout launch and gives the eval-mode bits (the tape holds no (seed, p) entry)."""
    from models.cm.unet_train import forward_with_grad
    outs = []
    for p, train in ((0.0, True), (0.0, False)):
        net, _, _ = build(PLAIN, dropout=p)
        net.train(train)
        x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
        t = torch.tensor([100.0, -300.0], device=DEV)
        y = forward_with_grad(net, x, t)
        (y * 0.5).sum().backward()
        outs.append((y.detach(), [q.grad.clone() for q in net.parameters()]))
        assert net.dropout_seeds_used == []
    assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


@pytest.mark.parametrize("tag", ["", "_plain"])
def test_dropout_gradients_vs_oracle_with_same_masks(ops, tag):
    from oracle import Precision, edm
    p = 0.3
    net, _, sd = build(PLAIN if tag else None, dropout=p)
    net.train()
    cc = not tag
    cfg = edm.EDMConfig(image_size=16, model_channels=64, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                        **(dict(num_classes=None, use_scale_shift_norm=False, resblock_updown=False) if tag else {}))
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(2, 3, 16, 16, generator=gen)
    t = torch.tensor([700.0, -900.0])
    y = torch.tensor([5, 321])
    w_out = torch.randn(2, 3, 16, 16, generator=gen)
    for q in net.parameters():
        q.requires_grad_(True)
    out = net(x.to(DEV), t.to(DEV), **({"y": y.to(DEV)} if cc else {}))
    (out * w_out.to(DEV)).sum().backward()
    seeds = list(net.dropout_seeds_used)
    assert len(seeds) == sum(1 for k in sd if k.endswith("out_layers.3.weight"))
    orig = edm._conv
    ref = {}
    try:
        for mode in ("fp32", "bf16"):
            it = iter(seeds)

            def conv(sd_, name, xin, prec, **kw):
                if name.endswith(".out_layers.3"):       # conv2 of a ResBlock: its input through the recorded mask
                    N, C, H, W = xin.shape
                    ones = torch.ones(N, H, W, C, dtype=torch.bfloat16, device=DEV)
                    mask = ops.dropout(ones, p, next(it)).float().permute(0, 3, 1, 2).cpu()
                    xin = xin * mask
                return orig(sd_, name, xin, prec, **kw)
            edm._conv = conv
            leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
            yo = edm.unet_forward(leaves, cfg, x, t, prec=Precision(mode), **({"y": y} if cc else {}))
            (yo * w_out).sum().backward()
            ref[mode] = {k: leaves[k].grad for k in leaves}
            assert next(it, None) is None
    finally:
        edm._conv = orig
    worst = ("", 0.0)
    for k, q in net.named_parameters():
        r = ((q.grad.cpu().double() - ref["fp32"][k].double()).norm() / (ref["fp32"][k].double().norm() + 1e-30)).item()
        fl = ((ref["bf16"][k].double() - ref["fp32"][k].double()).norm() / (ref["fp32"][k].double().norm() + 1e-30)).item()
        assert r < 2.0 * fl + 1.5e-2, (k, r, fl)
        worst = max(worst, (k, r), key=lambda v: v[1])
    print(f"dropout p={p}{tag}: worst gradient rel-L2 vs oracle {worst[1]:.3e} ({worst[0]})")


# ------------------------------------------------------------------------------------------ TrainLoop
def _loop(tmp, use_fp16, resume="", anneal=10):
    from models.cm.resample import LogNormalSampler
    from models.cm.train_util import TrainLoop
    net, diffusion, _ = build(PLAIN)
    net.train()
    return TrainLoop(model=net, diffusion=diffusion, data=None, batch_size=4, microbatch=2, lr=1e-4, ema_rate="0.999,0.9",
                     log_interval=3, save_interval=100, resume_checkpoint=resume, use_fp16=use_fp16,
                     schedule_sampler=LogNormalSampler(), lr_anneal_steps=anneal, log_dir=str(tmp))


def _batch(k):
    gen = torch.Generator().manual_seed(50 + k)
    return torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1, {}


@pytest.mark.parametrize("use_fp16", [False, True])
def test_trainloop_ema_anneal_overflow_resume(ops, tmp_path, use_fp16):
    tl = _loop(tmp_path, use_fp16)
    ema0 = [[p.detach().clone() for p in ps] for ps in tl.ema_params]
    masters, lrs = [], []
    for k in range(3):
        torch.manual_seed(100 + k)
        assert tl.run_step(*_batch(k))
        masters.append([p.detach().clone() for p in tl.mp_trainer.master_params])
        lrs.append(tl.opt.param_groups[0]["lr"])
        if k == 1:
            tl.save()
            lg_at_2 = tl.mp_trainer.lg_loss_scale
    assert tl.step == 3
    assert lrs == [pytest.approx(1e-4 * (1 - s / 10), rel=1e-12) for s in (1, 2, 3)]
    for ps in tl.ema_params + [tl.mp_trainer.master_params]:
        for p in ps:
            assert torch.isfinite(p).all()
    for k, rate in enumerate(tl.ema_rate):      # the reference's loop replayed on the recorded master weights
        rep = [t.clone() for t in ema0[k]]
        for m in masters:
            for a, b in zip(rep, m):
                a.mul_(rate).add_(b, alpha=1 - rate)
        for a, b in zip(tl.ema_params[k], rep):
            assert ((a - b).abs() <= 8 * U * b.abs() + 1e-30).all()
    row = tl.dumpkvs()
    assert {"loss", "mse", "xs_mse", "step"} <= set(row) and math.isfinite(row["loss"])
    assert sorted(os.listdir(tmp_path)) == sorted(["ema_0.999_000002.pt", "ema_0.9_000002.pt", "model000002.pt", "opt000002.pt",
                                                   "progress.jsonl"])

    if use_fp16:                                # an overflow step: no optimiser step, no EMA move, no step count
        ema_before = [[p.clone() for p in ps] for ps in tl.ema_params]
        m_before = [p.clone() for p in tl.mp_trainer.master_params]
        tl.mp_trainer.lg_loss_scale = 400.0
        torch.manual_seed(7)
        assert not tl.run_step(*_batch(9))
        assert tl.step == 3 and tl.mp_trainer.lg_loss_scale == 399.0
        for a, b in zip([p for ps in tl.ema_params for p in ps], [p for ps in ema_before for p in ps]):
            assert torch.equal(a, b)
        assert all(torch.equal(a, b) for a, b in zip(tl.mp_trainer.master_params, m_before))

    tr = _loop(tmp_path, use_fp16, resume=str(tmp_path / "model000002.pt"))
    assert tr.step == 2 and tr.resume_step == 2
    tr.mp_trainer.lg_loss_scale = lg_at_2       # the reference does not checkpoint the loss scale
    torch.manual_seed(102)
    assert tr.run_step(*_batch(2))
    for a, b in zip(tr.mp_trainer.master_params, masters[2]):
        assert torch.equal(a.detach(), b)
    for ka, kb in zip(tl.ema_params, tr.ema_params):           # the overflow step above left tl's EMA at step 3
        assert all(torch.equal(a, b) for a, b in zip(ka, kb))
    assert tr.opt.param_groups[0]["lr"] == pytest.approx(1e-4 * (1 - (3 + 2) / 10), rel=1e-12)   # the reference's step + resume_step


def test_imagenet64_full_size_dsm_step(ops):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.script_util import create_model_and_diffusion
    from backward_census import EDM_DSM_MODEL as kw              # the set-up the launch censuses record (dropout 0.1, fp16)
    torch.manual_seed(0)
    net, diffusion = create_model_and_diffusion(**kw)
    net = net.to(DEV).train()
    n = sum(p.numel() for p in net.parameters())
    assert 290e6 < n < 300e6
    from models.cm.resample import LogNormalSampler
    x0 = torch.rand(8, 3, 64, 64, device=DEV) * 2 - 1
    sig, w = LogNormalSampler().sample(8, DEV)
    t = diffusion.training_losses(net, x0, sig, model_kwargs={"y": torch.arange(8, device=DEV)})
    (t["loss"] * w).mean().backward()
    assert torch.isfinite(t["loss"]).all() and t["loss"].shape == (8,)
    for p in net.parameters():
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all()
    print(f"imagenet64 DSM step at 8 images: loss {t['loss'].tolist()}")


def test_dsm_wrappers_check_shapes(ops):
    from dxmi_hip import DxmiError
    from models.cm.karras_diffusion import KarrasDenoiser
    x0, noise, F, sig = [t.to(DEV) for t in operands(4, 3 * 16 * 16, 9)]
    with pytest.raises(DxmiError):
        ops.edm_dsm_prep(x0, noise[:2], sig)
    with pytest.raises(DxmiError):
        ops.edm_dsm_prep(x0, noise, sig[:3])
    with pytest.raises(DxmiError):
        ops.edm_dsm_loss_fwd(torch.cat([F, F], 1), x0, noise, sig, "karras")
    with pytest.raises(DxmiError):
        ops.edm_dsm_loss_bwd(torch.ones(3, device=DEV), None, F, x0, noise, sig, "karras")
    net, _, _ = build(PLAIN)
    with pytest.raises(ValueError):
        KarrasDenoiser().training_losses(net, torch.zeros(2, 3, 16, 16, device=DEV), torch.ones(1, device=DEV))
    with pytest.raises(ValueError):
        KarrasDenoiser().training_losses(net, torch.zeros(2, 3, 16, 16, device=DEV), torch.ones(2, device=DEV),
                                         noise=torch.zeros(1, 3, 16, 16, device=DEV))


def test_no_grad_training_losses_applies_dropout_in_train_mode(ops):
    """With grad disabled a train-mode net with dropout > 0 still drops (the training forward runs); eval mode does not."""
    from models.cm.karras_diffusion import KarrasDenoiser
    net, _, _ = build(PLAIN, dropout=0.3)
    x0, noise, _, sig = [t.to(DEV) for t in operands(2, 3 * 16 * 16, 4)]
    x0, noise = x0.view(2, 3, 16, 16), noise.view(2, 3, 16, 16)
    d = KarrasDenoiser()
    with torch.no_grad():
        ev = d.training_losses(net, x0, sig, noise=noise)["loss"]
        net.train()
        net.dropout_seed = 5
        tr = d.training_losses(net, x0, sig, noise=noise)["loss"]
        assert len(net.dropout_seeds_used) > 0
    net.dropout_seed, net._dropout_calls = 5, 0
    tg = d.training_losses(net, x0, sig, noise=noise)["loss"]      # grad path, same seeds
    assert not torch.equal(ev, tr)
    assert torch.equal(tr, tg.detach())


# ------------------------------------------------------------------------------------------ TrainLoop at world size 2
class _FixedDiffusion:
    """KarrasDenoiser whose training_losses takes the noise of each call from a fixed list (the test's stand-in for randn_like,
    so two ranks and one process see the same draws)."""

    def __init__(self, noises, start=0):
        from models.cm.karras_diffusion import KarrasDenoiser
        self.d, self.noises, self.i = KarrasDenoiser(sigma_data=0.5, weight_schedule="karras"), noises, start

    def training_losses(self, model, x_start, sigmas, model_kwargs=None, noise=None):
        n = self.noises[self.i].to(x_start.device)
        self.i += 1
        return self.d.training_losses(model, x_start, sigmas, model_kwargs=model_kwargs, noise=n)


class _FixedSampler:
    def __init__(self, sigmas):
        self.sigmas, self.i = sigmas, 0

    def sample(self, n, device):
        s = self.sigmas[self.i].to(device)
        self.i += 1
        assert s.numel() == n
        return s, torch.ones_like(s)


def _w2_data():
    gen = torch.Generator().manual_seed(321)
    steps = 3
    x = [torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1 for _ in range(steps)]
    sig = [torch.exp(torch.randn(4, generator=gen) * 1.2 - 1.2) for _ in range(steps)]
    noise = [torch.randn(4, 3, 16, 16, generator=gen) for _ in range(steps)]
    return x, sig, noise


def _w2_run(rank, world, log_dir):
    """Three TrainLoop steps on this rank's share of the fixed global batch of 4 (microbatch = batch_size), a save after step 2,
    and a second loop resumed from that save that runs step 3 again.  -> numpy copies of the masters / EMAs."""
    from models.cm.train_util import TrainLoop
    x, sig, noise = _w2_data()
    bs = 4 // world
    sl = slice(rank * bs, (rank + 1) * bs)
    net, _, _ = build(PLAIN)
    net.train()
    if rank == 1:                              # rank 1 starts from other weights: the load-time broadcast must replace them
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.25)

    def loop(resume, start):
        return TrainLoop(model=net, diffusion=_FixedDiffusion([n[sl] for n in noise], start),
                         data=None, batch_size=bs, microbatch=bs, lr=1e-4, ema_rate="0.999,0.9", log_interval=10, save_interval=100,
                         resume_checkpoint=resume, schedule_sampler=_FixedSampler([s[sl] for s in sig]), log_dir=log_dir)
    tl = loop("", 0)
    assert tl.global_batch == 4
    w0 = [p.detach().cpu().numpy().copy() for p in tl.mp_trainer.master_params]
    snap = lambda t: ([p.detach().cpu().numpy().copy() for p in t.mp_trainer.master_params],
                      [[p.detach().cpu().numpy().copy() for p in ps] for ps in t.ema_params])
    out = {"w0": w0}
    for k in range(2):
        assert tl.run_step(x[k][sl], {})
    out["step2"] = snap(tl)
    tl.save()
    assert tl.run_step(x[2][sl], {})
    out["step3"] = snap(tl)
    net2, _, _ = build(PLAIN)
    net2.train()
    net = net2
    tr = loop(os.path.join(log_dir, "model000002.pt"), 2)
    tr.schedule_sampler.i = 2
    assert tr.resume_step == 2
    assert tr.run_step(x[2][sl], {})
    out["resumed3"] = snap(tr)
    return out


def _w2_worker(rank, world, port, q, log_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = _w2_run(rank, world, log_dir)
    except Exception as e:       # reported to the parent, which stops the other rank (it may wait in a collective)
        q.put((rank, repr(e)))
        raise
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def _rel(a, b):
    a = np.concatenate([np.ravel(v) for v in a]).astype(np.float64)
    b = np.concatenate([np.ravel(v) for v in b]).astype(np.float64)
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300)


def test_trainloop_world_size_2_gloo_matches_one_process(ops, tmp_path):
    """Two ranks on cuda:0 over gloo, each with half of the batch, against one process on the whole batch: load-time broadcast,
    gradient exchange, EMA, rank-0 checkpoint writes + barrier, and the resume (EMA broadcast) all take part."""
    import socket
    import torch.multiprocessing as mp
    single = _w2_run(0, 1, str(tmp_path / "single"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.makedirs(tmp_path / "w2", exist_ok=True)
    procs = [ctx.Process(target=_w2_worker, args=(r, 2, port, q, str(tmp_path / "w2"))) for r in range(2)]
    res = {}
    try:
        for p in procs:
            p.start()
        for _ in procs:
            r, v = q.get(timeout=600)
            res[r] = v
            assert not isinstance(v, str), (r, v)
        for p in procs:
            p.join(120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(30)
    a, b = res[0], res[1]
    assert all(np.array_equal(u, v) for u, v in zip(a["w0"], b["w0"]))                        # broadcast at load
    assert all(np.array_equal(u, v) for u, v in zip(a["w0"], single["w0"]))
    for key in ("step2", "step3", "resumed3"):
        (ma, ea), (mb, eb) = a[key], b[key]
        assert all(np.array_equal(u, v) for u, v in zip(ma, mb)), key                        # ranks agree bit for bit
        assert all(np.array_equal(u, v) for x_, y_ in zip(ea, eb) for u, v in zip(x_, y_)), key
    for rk in (a, b):                                                                         # resume reproduces step 3
        assert all(np.array_equal(u, v) for u, v in zip(rk["step3"][0], rk["resumed3"][0]))
        assert all(np.array_equal(u, v) for x_, y_ in zip(rk["step3"][1], rk["resumed3"][1]) for u, v in zip(x_, y_))
    worst = 0.0
    for key in ("step2", "step3"):                       # against one process: the weight UPDATES agree to bf16-level noise
        (m2, e2), (m1, e1) = a[key], single[key]
        d2 = [u - w for u, w in zip(m2, a["w0"])]
        d1 = [u - w for u, w in zip(m1, single["w0"])]
        r = _rel(d2, d1)
        worst = max(worst, r)
        assert r < 2e-2, (key, r)
        for k in range(2):
            de2 = [u - w for u, w in zip(e2[k], a["w0"])]
            de1 = [u - w for u, w in zip(e1[k], single["w0"])]
            assert _rel(de2, de1) < 2e-2, (key, k)
    print(f"world size 2 vs one process: worst rel-L2 of the weight update {worst:.3e} (bound 2e-2)")
