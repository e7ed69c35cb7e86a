"""Host side of adversarial score identity distillation (SiDA): the torch paths of KarrasDenoiser.sida_generator_losses
and sida_discriminator_losses on float64 analytic callables against an independent float64 statement of the issue's formulas that
torch.autograd differentiates as a whole, a negative control without the adversarial path, the s == 0 convention, sida_gen_weight = 0
against sid_generator_losses, the draw order, every refusal of the loop and of the parser, DMTrainLoop(objective="sida") on the CPU
with save / resume, and the C entry points of csrc/sida_train.hip under the host sanitizers.  No GPU."""
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_dm_host import EVERY, ITERS, LR, _diffusion, _flat, _latents, _t4
from test_sid_host import D64, N, S, SHAPE, _Dense, _operands, _rel, _scal32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dxmi_sida_map_fwd", "dxmi_sida_map_bwd")
CB, HB = 6, 2                 # the analytic bottleneck: [N, 6, 2, 2]
WEIGHTS = (0.01, 0.7)


class _DenseEnc(_Dense):
    """_Dense with a bottleneck: encode(x_in, t) = tanh(E x_in + 2e-3 t) reshaped [N, CB, HB, HB], E dense, so the logits depend on every
    pixel.  E is a parameter: the generator path must leave its grad None, the discriminator path must fill it."""

    def __init__(self, seed, scale, bias=True):
        super().__init__(seed, scale, bias)
        gen = torch.Generator().manual_seed(seed + 100)
        n = math.prod(SHAPE)
        self.E = torch.nn.Parameter(torch.randn(CB * HB * HB, n, generator=gen, dtype=D64) * 2.0 / math.sqrt(n))

    def encode(self, x_in, t, **kw):
        return torch.tanh(x_in.flatten(1) @ self.E.T + 2e-3 * t[:, None]).view(-1, CB, HB, HB)


def _nets(bias=True):
    return _Dense(1, 0.8, bias), _Dense(2, 1.1, bias), _DenseEnc(3, 0.6, bias)


def _softplus(v):
    return torch.clamp(v, min=0) + torch.log1p(torch.exp(-v.abs()))          # the form of the issue


def _a(h, sign):
    """a_n(sign) of the issue from h [N, CB, HB, HB]: logit = channel mean, mean over the positions of softplus(sign logit)."""
    logit = h.sum(dim=1).flatten(1) / h.shape[1]
    return _softplus(sign * logit).sum(dim=1) / logit.shape[1], logit


def _statement(gen, real, fake, z, noise, idx, alpha, weight, gen_sigma=80.0, sd_f=0.5, adversarial=True, skip=()):
    """loss_n = sid_n + weight a_n(-1) / sg(s_n) as ONE expression of the generator's parameters, differentiated by autograd as a whole
    (through x, both denoisers' inputs and the encoder).  adversarial=False: the encoder sees x_t.detach() (the negative control)."""
    from models.cm.karras_diffusion import cd_levels
    t = cd_levels(S, 0.002, 80.0, 7.0).table[idx]
    sg = torch.full((N,), gen_sigma, dtype=torch.float32)

    def denoise(net, x_t, sigma, sd):
        c_skip, c_out, c_in = (_t4(c) for c in _scal32(sigma, sd))
        return c_out * net(c_in * x_t, 250 * torch.log(sigma + 1e-44)) + c_skip * x_t
    x = denoise(gen, z * gen_sigma, sg, 0.5)
    x_t = x + noise * _t4(t)
    D_r, D_f = denoise(real, x_t, t, 0.5), denoise(fake, x_t, t, sd_f)
    s = (x - D_r).abs().flatten(1).mean(dim=1).detach()
    delta = D_r - D_f
    total = ((1 - alpha) * delta ** 2 + delta * (D_f - x)).flatten(1).sum(dim=1)
    c_in_f = _t4(_scal32(t, sd_f)[2])
    adv, logit = _a(fake.encode(c_in_f * (x_t if adversarial else x_t.detach()), 250 * torch.log(t + 1e-44)), -1.0)
    keep = torch.tensor([n not in skip for n in range(N)])
    safe = torch.where(keep, s, torch.ones_like(s))
    loss = torch.where(keep, total / (math.prod(SHAPE) * safe) + weight * adv / safe, torch.zeros_like(s))
    params = list(gen.parameters())
    grads = torch.autograd.grad(loss.sum(), params)
    return loss.detach(), s, adv.detach(), logit.detach(), dict(zip(params, grads))


def _call(gen, real, fake, z, noise, idx, **kw):
    return _diffusion().sida_generator_losses(gen, z, S, real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise,
                                              indices=idx, **kw)


# ------------------------------------------------------------------------------------------ wiring
def test_entry_points_are_declared_everywhere():
    from dxmi_hip import _lib, ops
    header = open(os.path.join(ROOT, "include", "dxmi_hip.h")).read()
    makefile = open(os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc", "Makefile")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header) and sym in _lib.SIGNATURES
        assert hasattr(ops, sym[len("dxmi_"):])
    assert "sida_train.hip" in re.search(r"^SRCS = (.*)$", makefile, flags=re.M).group(1).split()
    assert "asan_sida" in makefile


# ------------------------------------------------------------------------------------------ the generator's torch path
@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("alpha,sd_f", [(1.2, 0.5), (1.0, 0.25)])
def test_generator_torch_path_against_autograd_of_the_whole_loss(alpha, sd_f, weight):
    z, noise, idx = _operands()
    gen, real, fake = _nets()
    terms = _call(gen, real, fake, z, noise, idx, fake_diffusion=_diffusion(sigma_data=sd_f), alpha=alpha, sida_gen_weight=weight)
    assert set(terms) == {"loss", "x", "dm_norm", "adv_loss", "adv_logit"}
    assert terms["loss"].shape == (N,) and terms["adv_loss"].shape == (N,) and terms["adv_logit"].shape == (N, HB * HB)
    assert terms["loss"].requires_grad and not any(terms[k].requires_grad for k in ("x", "dm_norm", "adv_loss", "adv_logit"))
    terms["loss"].sum().backward()
    ref_loss, ref_s, ref_adv, ref_logit, ref_grads = _statement(gen, real, fake, z, noise, idx, alpha, weight, sd_f=sd_f)
    errs = dict(loss=_rel(terms["loss"].detach(), ref_loss), dm_norm=_rel(terms["dm_norm"], ref_s), adv=_rel(terms["adv_loss"], ref_adv),
                logit=_rel(terms["adv_logit"], ref_logit), grads=max(_rel(p.grad, g) for p, g in ref_grads.items()))
    print(f"sida torch path vs autograd (alpha {alpha}, fake sigma_data {sd_f}, weight {weight}): relative errors {errs}")
    assert all(v <= 1e-12 for v in errs.values()), errs
    # the gradient reaches the generator through x alone
    assert all(p.grad is None for net in (real, fake) for p in net.parameters())
    # negative control: without the adversarial path (the encoder fed x_t.detach()) the gradient is another one
    *_, twin = _statement(gen, real, fake, z, noise, idx, alpha, weight, sd_f=sd_f, adversarial=False)
    apart = min(_rel(p.grad, g) for p, g in twin.items())
    print(f"  the twin without the adversarial path differs by at least {apart:.3e} (relative, per parameter)")
    assert apart >= (1e-2 if weight == 0.7 else 1e-4)


def test_weight_zero_is_sid_generator_losses_and_no_grad_forms_everything():
    z, noise, idx = _operands()
    gen, real, fake = _nets()
    a = _call(gen, real, fake, z, noise, idx, sida_gen_weight=0.0)
    a["loss"].sum().backward()
    ga = [p.grad.clone() for p in gen.parameters()]
    gen.zero_grad()
    b = _diffusion().sid_generator_losses(gen, z, S, real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx)
    b["loss"].sum().backward()
    for k in ("loss", "x", "dm_norm"):
        assert torch.equal(a[k].detach(), b[k].detach()), k
    assert all(torch.equal(u, p.grad) for u, p in zip(ga, gen.parameters()))
    assert float(a["adv_loss"].min()) > 0                                   # the term is formed, it only has no weight
    c = _call(gen, real, fake, z, noise, idx)                               # the default weight changes the loss, not dm_norm
    assert not torch.equal(c["loss"].detach(), a["loss"].detach()) and torch.equal(c["dm_norm"], a["dm_norm"])
    with torch.no_grad():
        v = _call(gen, real, fake, z, noise, idx)
    assert not v["loss"].requires_grad
    for k in ("loss", "x", "dm_norm", "adv_loss", "adv_logit"):
        assert torch.equal(c[k].detach(), v[k]), k
    assert all(p.grad is None for net in (real, fake) for p in net.parameters())


@pytest.mark.parametrize("weight", WEIGHTS)
def test_zero_normaliser_gives_zero_loss_and_no_gradient(weight):
    """Sample 1: z = 0 and noise = 0 through nets without bias give x = 0 = x_t = D_r, so s == 0 exactly: loss 0 although its
    adversarial term is log 2 > 0, and that sample adds nothing to the gradient (the statement leaves it out of its sum)."""
    z, noise, idx = _operands()
    z[1], noise[1] = 0, 0
    gen, real, fake = _nets(bias=False)
    terms = _call(gen, real, fake, z, noise, idx, sida_gen_weight=weight)
    assert float(terms["dm_norm"][1]) == 0 and float(terms["loss"].detach()[1]) == 0 and float(terms["adv_loss"][1]) > 0
    assert torch.isfinite(terms["loss"]).all()
    terms["loss"].sum().backward()
    ref_loss, _, _, _, ref_grads = _statement(gen, real, fake, z, noise, idx, 1.2, weight, skip=(1,))
    assert _rel(terms["loss"].detach(), ref_loss) <= 1e-12
    for p, g in ref_grads.items():
        assert torch.isfinite(p.grad).all() and float(g.abs().max()) > 0 and _rel(p.grad, g) <= 1e-12


def test_generator_refusals():
    z, noise, idx = _operands()
    gen, real, fake = _nets()
    with pytest.raises(NotImplementedError, match="K = 1 only"):
        _call(gen, real, fake, z, noise, idx, gen_sigmas=(80.0, 2.5))
    assert torch.equal(_call(gen, real, fake, z, noise, idx, gen_sigmas=(2.5,))["x"], _call(gen, real, fake, z, noise, idx, gen_sigma=2.5)["x"])
    with pytest.raises(ValueError, match="excludes gen_sigma"):
        _call(gen, real, fake, z, noise, idx, gen_sigmas=(2.5,), gen_sigma=2.5)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sida_gen_weight"):
            _call(gen, real, fake, z, noise, idx, sida_gen_weight=bad)
        with pytest.raises(ValueError, match="alpha"):
            _call(gen, real, fake, z, noise, idx, alpha=bad)
    with pytest.raises(NotImplementedError, match="encode"):
        _call(gen, real, _Dense(3, 0.6), z, noise, idx)
    with pytest.raises(NotImplementedError, match="distillation=False"):
        _diffusion(distillation=True).sida_generator_losses(gen, z, S, real_model=real, real_diffusion=_diffusion(), fake_model=fake)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        _call(gen, real, fake, z.clone().requires_grad_(True), noise, idx)
    with pytest.raises(NotImplementedError, match="real_model"):
        _diffusion().sida_generator_losses(gen, z, S, fake_model=fake)


# ------------------------------------------------------------------------------------------ the discriminator's torch path
def _dis_operands():
    gen = torch.Generator().manual_seed(23)
    x_fake, x_real = torch.randn(N, *SHAPE, generator=gen, dtype=D64), torch.rand(N, *SHAPE, generator=gen, dtype=D64) * 2 - 1
    noise = torch.randn(2 * N, *SHAPE, generator=gen, dtype=D64)
    idx = torch.tensor([0, S - 1, 7, 9, 12, 3, 3, 16, 1, 10])
    return x_fake, x_real, noise, idx


@pytest.mark.parametrize("sd", [0.5, 0.25])
def test_discriminator_torch_path_against_the_statement(sd):
    from models.cm.karras_diffusion import cd_levels
    x_fake, x_real, noise, idx = _dis_operands()
    fake = _DenseEnc(3, 0.6)
    terms = _diffusion(sigma_data=sd).sida_discriminator_losses(fake, x_fake, x_real, S, noise=noise, indices=idx)
    assert set(terms) == {"loss", "logit_fake", "logit_real"} and terms["loss"].shape == (N,)
    assert terms["logit_fake"].shape == (N, HB * HB) == terms["logit_real"].shape and not terms["logit_fake"].requires_grad
    terms["loss"].sum().backward()
    got = fake.E.grad.clone()
    assert fake.A.grad is None and fake.b.grad is None              # nothing downstream of the bottleneck takes part
    # the statement: one batch of 2N, generated half first
    t = cd_levels(S, 0.002, 80.0, 7.0).table[idx]
    x = torch.cat([x_fake, x_real])
    h = fake.encode(_t4(_scal32(t, sd)[2]) * (x + noise * _t4(t)), 250 * torch.log(t + 1e-44))
    a_plus, logit = _a(h[:N], 1.0)
    a_minus, logit_r = _a(h[N:], -1.0)
    ref = a_plus + a_minus
    g, = torch.autograd.grad(ref.sum(), fake.E)
    assert _rel(terms["loss"].detach(), ref.detach()) <= 1e-12 and _rel(got, g) <= 1e-12 and float(g.abs().max()) > 0
    assert _rel(terms["logit_fake"], logit.detach()) <= 1e-12 and _rel(terms["logit_real"], logit_r.detach()) <= 1e-12
    with pytest.raises(ValueError, match="one shape"):
        _diffusion().sida_discriminator_losses(fake, x_fake, x_real[:2], S)
    with pytest.raises(ValueError, match="name the same inputs"):
        _diffusion().sida_discriminator_losses(fake, x_fake, x_real, S, model_kwargs={"y": torch.zeros(N)})
    with pytest.raises(ValueError, match="stacked batch"):
        _diffusion().sida_discriminator_losses(fake, x_fake, x_real, S, noise=noise[:N], indices=idx)
    with pytest.raises(NotImplementedError, match="encode"):
        _diffusion().sida_discriminator_losses(_Dense(3, 0.6), x_fake, x_real, S)


def test_draw_order():
    """The generator: indices, then noise, as sid_generator_losses draws them.  The discriminator: ONE draw of indices [2N], then
    noise [2N, ...], as gan_discriminator_losses draws them (restated here with the generator's own calls)."""
    from models.cm.karras_diffusion import cd_levels, dm_index_range
    seen = {}

    def spy(name):
        def real(x_in, t, **kw):
            seen[name] = (x_in.clone(), t.clone())
            return torch.zeros_like(x_in)
        return real
    z = torch.randn(64, *SHAPE, generator=torch.Generator().manual_seed(1), dtype=D64)
    gen, _, fake = _nets()
    state = torch.get_rng_state()
    for name in ("sid", "sida"):
        fn = getattr(_diffusion(), f"{name}_generator_losses")
        fn(gen, z, S, real_model=spy(name), real_diffusion=_diffusion(), fake_model=fake, generator=torch.Generator().manual_seed(11))
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(seen["sid"][0], seen["sida"][0]) and torch.equal(seen["sid"][1], seen["sida"][1])
    x_fake, x_real, _, _ = _dis_operands()
    g = torch.Generator().manual_seed(31)
    lo, hi = dm_index_range(S, 0.0, 1.0)
    idx = torch.randint(lo, hi + 1, (2 * N,), generator=g)
    noise = torch.randn((2 * N,) + SHAPE, generator=g, dtype=D64)
    drawn = _diffusion().sida_discriminator_losses(fake, x_fake, x_real, S, generator=torch.Generator().manual_seed(31))
    given = _diffusion().sida_discriminator_losses(fake, x_fake, x_real, S, noise=noise, indices=idx)
    assert torch.equal(torch.get_rng_state(), state)
    assert (lo, hi) == (0, S - 1) and all(torch.equal(drawn[k].detach(), given[k].detach()) for k in drawn)
    assert float(cd_levels(S, 0.002, 80.0, 7.0).table[idx].max()) > 1.0      # the draw reaches the high levels


# ------------------------------------------------------------------------------------------ loop and parser
class _TinyEnc(torch.nn.Module):
    """test_dm_host._Tiny with a bottleneck on the same parameters: encode = the 2x2 mean pool of tanh(a x + b), [N, 3, 4, 4]."""

    def __init__(self, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(3, 3, generator=gen) * 0.3)
        self.b = torch.nn.Parameter(torch.randn(3, generator=gen) * 0.1)

    def _mix(self, x, t):
        return torch.tanh(torch.einsum("oc,nchw->nohw", self.a, x) + self.b[None, :, None, None] + 1e-3 * _t4(t))

    def forward(self, x, t):
        return self._mix(x, t)

    def encode(self, x, t):
        return torch.nn.functional.avg_pool2d(self._mix(x, t), 2)


def _reals(seed=77):
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand(4, 3, 8, 8, generator=gen) * 2 - 1 for _ in range(ITERS)]


def _loop(tmp, resume="", reals=None, start=0, **over):
    from models.cm.resample import LogNormalSampler
    from models.cm.train_util import DMTrainLoop
    from test_dm_host import _Tiny
    kw = dict(model=_Tiny(1), diffusion=_diffusion(), real_model=_Tiny(3), real_diffusion=_diffusion(), fake_model=_TinyEnc(2), num_scales=18,
              gen_update_every=EVERY, fake_lr=2 * LR, data=None, batch_size=4, microbatch=2, lr=LR, ema_rate="0.9,0.5", log_interval=2,
              save_interval=100, resume_checkpoint=resume, schedule_sampler=LogNormalSampler(), log_dir=str(tmp), objective="sida",
              real_data=iter([(r, {}) for r in (reals or _reals())[start:]]))
    kw.update(over)
    tl = DMTrainLoop(**kw)
    for name, trainer, lr in (("opt", tl.mp_trainer, LR), ("fake_opt", tl.fake_trainer, 2 * LR)):
        opt = torch.optim.RAdam(trainer.master_params, lr=lr)
        if resume:
            opt.load_state_dict(getattr(tl, name).state_dict())
        setattr(tl, name, opt)
    return tl


def _run(tl, k, z):
    torch.manual_seed(1000 + k)
    return tl.run_step(z[k], {})


def test_dmtrainloop_sida_two_clocks_save_resume(tmp_path):
    z = _latents()
    tl = _loop(tmp_path, sid_alpha=1.2, sida_gen_weight=0.5, sida_dis_weight=2.0)
    assert (tl.objective, tl.sid_alpha, tl.sida_gen_weight, tl.sida_dis_weight) == ("sida", 1.2, 0.5, 2.0)
    real0 = _flat(tl.real_model.parameters()).clone()
    gens, fakes = {}, {}
    g_prev, f_prev = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
    for k in range(ITERS):
        took_gen, took_fake = _run(tl, k, z)
        gens[k], fakes[k] = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
        on = k % EVERY == 0
        assert took_gen == on and took_fake
        assert torch.equal(gens[k], g_prev) != on and not torch.equal(fakes[k], f_prev), k
        assert torch.equal(_flat(tl.real_model.parameters()), real0) and all(p.grad is None for p in tl.real_model.parameters())
        g_prev, f_prev = gens[k], fakes[k]
        if tl.step == 4:
            tl.save()
    row = tl.dumpkvs()
    assert {"loss", "dm_norm", "fake_mse", "sida_gen", "sida_dis", "logit_fake", "logit_real", "step"} <= set(row)
    assert all(math.isfinite(row[k]) for k in ("loss", "sida_gen", "sida_dis"))
    files = set(os.listdir(tmp_path))
    assert {"model000004.pt", "opt000004.pt", "fake_model000004.pt", "fake_opt000004.pt"} <= files
    assert not any(f.startswith(("gan_head", "sida")) for f in files)        # the discriminator lives in fake_model%06d.pt
    tr = _loop(tmp_path, resume=str(tmp_path / "model000004.pt"), start=4, sid_alpha=1.2, sida_gen_weight=0.5, sida_dis_weight=2.0)
    assert tr.step == 4 and torch.equal(_flat(tr.fake_model.parameters()), fakes[3])
    for k in (4, 5, 6):
        _run(tr, k, z)
        assert torch.equal(_flat(tr.model.parameters()), gens[k]) and torch.equal(_flat(tr.fake_model.parameters()), fakes[k]), k
    # both weights are live: another discriminator weight moves the fake net elsewhere at once, another generator weight the generator
    other = _loop(tmp_path / "dis", sida_gen_weight=0.5, sida_dis_weight=0.0)
    _run(other, 0, z)
    assert torch.equal(_flat(other.model.parameters()), gens[0]) and not torch.equal(_flat(other.fake_model.parameters()), fakes[0])
    other = _loop(tmp_path / "gen", sida_gen_weight=0.0, sida_dis_weight=2.0)
    _run(other, 0, z)
    assert not torch.equal(_flat(other.model.parameters()), gens[0]) and torch.equal(_flat(other.fake_model.parameters()), fakes[0])
    # and with both at zero the generator's step is objective "sid"'s
    from test_dm_host import _loop as sid_loop
    # (one microbatch: the discriminator's draws come after the generator's and the DSM loss's, so the streams agree up to there)
    zero = _loop(tmp_path / "zero", sida_gen_weight=0.0, sida_dis_weight=0.0, microbatch=4)
    sid = sid_loop(tmp_path / "sid", objective="sid", microbatch=4)
    sid.fake_model.load_state_dict({k: v for k, v in zero.fake_model.state_dict().items()})
    _run(zero, 0, z), _run(sid, 0, z)
    assert torch.equal(_flat(zero.model.parameters()), _flat(sid.model.parameters()))


def test_dmtrainloop_refusals(tmp_path):
    from models.cm.gan_head import GANHead
    with pytest.raises(ValueError, match="needs real_data"):
        _loop(tmp_path, real_data=None)
    with pytest.raises(ValueError, match="takes no gan_head"):
        _loop(tmp_path, gan_head=GANHead(128, 8))
    with pytest.raises(NotImplementedError, match="limited to a one-step generator"):
        _loop(tmp_path, gen_sigmas=(80.0, 2.5))
    assert len(_loop(tmp_path, gen_sigmas=(2.5,)).gen_sigmas) == 1         # a one-level ladder stands for gen_sigma
    with pytest.raises(NotImplementedError, match="use_graph"):
        _loop(tmp_path, use_graph=True)
    for bad in (dict(sida_gen_weight=float("nan")), dict(sida_dis_weight=float("inf")), dict(sid_alpha=float("nan"))):
        with pytest.raises(ValueError, match="sida_gen_weight|sida_dis_weight|sid_alpha"):
            _loop(tmp_path, **bad)
    # objective "sid" with a head keeps its refusal and its words
    with pytest.raises(NotImplementedError, match="SiDA"):
        _loop(tmp_path, objective="sid", gan_head=GANHead(128, 8))
    with pytest.raises(ValueError, match="objective"):
        _loop(tmp_path, objective="sida2")
    tl = _loop(tmp_path)
    with pytest.raises(ValueError, match="real_data yields batches of 4 images"):
        tl.run_step(torch.zeros(2, 3, 8, 8), {})


def test_command_line_flags_and_refusals(capsys):
    import cm_train
    dm = ["--training_mode", "dm"]
    a = cm_train.parse_args(dm)
    assert (a.dm_objective, a.sida_gen_weight, a.sida_dis_weight) == ("dmd", 0.01, 1.0)
    a = cm_train.parse_args(dm + ["--dm_objective", "sida", "--synthetic_data", "True"])
    assert (a.dm_objective, a.sid_alpha, a.sida_gen_weight, a.sida_dis_weight, a.gen_sigma) == ("sida", 1.2, 0.01, 1.0, 0.0)
    a = cm_train.parse_args(dm + ["--dm_objective=sida", "--data_npz", "x.npz", "--sid_alpha", "1.0", "--sida_gen_weight", "0.1",
                                  "--sida_dis_weight=0.5", "--gen_sigma", "2.5"])
    assert (a.sid_alpha, a.sida_gen_weight, a.sida_dis_weight, a.gen_sigma, a.data_npz) == (1.0, 0.1, 0.5, 2.5, "x.npz")
    sida = dm + ["--dm_objective", "sida", "--synthetic_data", "True"]
    for argv, msg in ((dm + ["--dm_objective", "sida"], "needs real images"),
                      (sida + ["--dm_gan", "True"], "--dm_gan True does not go with --dm_objective sida"),
                      (sida + ["--dm_weighting", "none"], "--dm_weighting none"),
                      (sida + ["--sida_gen_weight", "nan"], "--sida_gen_weight"),
                      (sida + ["--sida_dis_weight", "inf"], "--sida_dis_weight"),
                      (sida + ["--sid_alpha", "nan"], "--sid_alpha"),
                      (sida + ["--gen_sigmas", "80,2.5"], "--gen_sigmas with more than one level"),
                      (sida + ["--use_graph", "True"], "--use_graph"),
                      (dm + ["--sida_gen_weight", "0.1"], "--sida_gen_weight belongs to --training_mode dm --dm_objective sida"),
                      (dm + ["--dm_objective", "sid", "--sida_dis_weight=2"], "--sida_dis_weight belongs to"),
                      (["--training_mode", "consistency_training", "--synthetic_data", "True", "--sida_gen_weight", "0.1"],
                       "--sida_gen_weight belongs to"),
                      (["--training_mode", "progdist", "--synthetic_data", "True", "--dm_objective", "sida"],
                       "--dm_objective belongs to --training_mode dm"),
                      # every present error stays
                      (dm + ["--dm_objective", "dmd2"], "--dm_objective"),
                      (dm + ["--dm_objective", "sid", "--dm_gan", "True", "--synthetic_data", "True"], "is SiDA"),
                      (dm + ["--data_npz", "x.npz"], "--data_npz does not go with --training_mode dm"),
                      (dm + ["--dm_objective", "sid", "--data_npz", "x.npz"], "--data_npz does not go with --training_mode dm")):
        with pytest.raises(SystemExit):
            cm_train.parse_args(argv)
        assert msg in capsys.readouterr().err, argv


# ------------------------------------------------------------------------------------------ host sanitizers
def test_sida_entry_points_under_address_and_ub_sanitizers():
    """`make asan_sida` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_sida.c, a program with its own main, against it and a no-device HIP runtime stub.  Null and misaligned
    pointers, sizes out of range, a Cb that is no multiple of 8, a sign that is not -1 / +1 and a non-finite coef (in the first and in
    a later launch's chunk of the host arrays, which are allocated at exactly N values) must each come back as DXMI_EINVAL with the
    message of their check: no crash, no sanitizer report.  The program runs as a child process; nothing is loaded into python.  A
    host-only build: machines without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_sida"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_sida")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") == 51        # every case of the driver
