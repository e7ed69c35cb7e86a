"""Host side of distribution matching distillation: the torch path of KarrasDenoiser.dm_generator_losses against a float64
restatement written here, its fixed points, the index draw, the refusals, DMTrainLoop's two clocks and its save / resume on small
nn.Modules, the command-line refusals, and the C entry points of csrc/dm_train.hip under the host sanitizers.  No GPU."""
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SYMBOLS = ("dxmi_dm_gen_in", "dxmi_dm_gen_out", "dxmi_dm_gen_prep", "dxmi_dm_grad_fwd", "dxmi_dm_gen_bwd")


def _diffusion(**kw):
    from models.cm.karras_diffusion import KarrasDenoiser
    return KarrasDenoiser(**dict(dict(sigma_data=0.5, weight_schedule="karras", distillation=False), **kw))


def _t4(t):
    return t[:, None, None, None]


class _Tanh(torch.nn.Module):
    """F = a tanh(w x_in + 1e-3 t) with parameters w and a (the analytic style of test_pd_host.py)."""

    def __init__(self, w, a=1.0, dtype=torch.float32):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(w, dtype=dtype))
        self.a = torch.nn.Parameter(torch.tensor(a, dtype=dtype))

    def forward(self, x_in, t, **kw):
        return self.a * torch.tanh(self.w * x_in + 1e-3 * _t4(t))


def _operands(N=6, shape=(3, 8, 8), S=18, seed=5):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(N, *shape, generator=gen)
    noise = torch.randn(N, *shape, generator=gen)
    idx = torch.randint(0, S, (N,), generator=gen)
    idx[0], idx[1] = 0, S - 1
    return z, noise, idx


def _restate64(gen, real, fake, z, noise, idx, S, weighting, gen_sigma=80.0, sd=0.5, sd_r=0.5, sd_f=0.5):
    """dm_generator_losses in float64 -> dict: x, s, g, loss, surrogate = 0.5 mean((x - sg(x - g))^2), and the magnitudes the fp32
    path's rounding errors scale with (the form of test_hip_pd_train.py: an elementwise result is held to 16 u M, M the magnitude
    of the operands that meet in it; a per-sample mean to 64 u of the mean of its terms' magnitudes):
      M_x   = |c_out F_g| + |c_skip sigma_G z| + c_out |a| (|w x_in| + 1e-3 |time|) (the last term: the rounding of tanh's argument,
              which reaches the output whatever the size of F), M_xt = M_x + |noise t|
      M_r   = |c_out_r F_r| + |c_skip_r x_t| + the same argument term + L_r M_xt, L_r = c_out_r |a w| c_in_r + c_skip_r the denoiser's Lipschitz constant in
              x_t (the fp32 path evaluates it at its own rounded x_t); M_f likewise
      s_mag = mean(M_x + M_r): |s - s64| <= 64 u s_mag
      M_g   = M_r + M_f ("none"); (M_r + M_f) / s + 4 |g| s_mag / s ("dmd": g carries the relative error of s)
      l_mag = mean(M_g (|g| + 16 u M_g)): |loss - loss64| <= 64 u l_mag."""
    from models.cm.karras_diffusion import cd_levels
    d = torch.float64
    z, noise = z.to(d), noise.to(d)
    t = cd_levels(S, 0.002, 80.0, 7.0).table.to(d)[idx]

    def scal(sigma, sd):
        return (sd ** 2 / (sigma ** 2 + sd ** 2), sigma * sd / (sigma ** 2 + sd ** 2) ** 0.5, 1 / (sigma ** 2 + sd ** 2) ** 0.5)

    def denoise(net, x_t, sigma, sd):
        c_skip, c_out, c_in = scal(sigma, sd)
        x_in, tm = _t4(c_in) * x_t, 250 * torch.log(sigma)
        F = net(x_in, tm)
        a, w = abs(float(net.a.detach())), abs(float(net.w.detach()))
        lip = c_out * a * w * c_in + c_skip
        arg = _t4(c_out) * a * (w * x_in.abs() + 1e-3 * _t4(tm.abs()))      # tanh is 1-Lipschitz: the rounding of its argument
        return _t4(c_out) * F + _t4(c_skip) * x_t, (_t4(c_out) * F).abs() + (_t4(c_skip) * x_t).abs() + arg.detach(), _t4(lip)
    sg = torch.full((z.shape[0],), gen_sigma, dtype=d)
    x, M_x, _ = denoise(gen, z * gen_sigma, sg, sd)
    with torch.no_grad():
        x_t = x + noise * _t4(t)
        M_xt = M_x + (noise * _t4(t)).abs()
        d_r, M_r, L_r = denoise(real, x_t, t, sd_r)
        d_f, M_f, L_f = denoise(fake, x_t, t, sd_f)
        M_r, M_f = M_r + L_r * M_xt, M_f + L_f * M_xt
        s = (x - d_r).abs().mean(dim=[1, 2, 3])
        s_mag = (M_x + M_r).mean(dim=[1, 2, 3])
        g, M_g = d_f - d_r, M_r + M_f
        if weighting == "dmd":
            g = g / _t4(s)
            M_g = M_g / _t4(s) + 4 * g.abs() * _t4(s_mag / s)
        l_mag = (M_g * (g.abs() + 16 * U * M_g)).mean(dim=[1, 2, 3])
    loss = 0.5 * (g ** 2).mean(dim=[1, 2, 3])
    surrogate = 0.5 * ((x - (x - g).detach()) ** 2).mean(dim=[1, 2, 3])
    return dict(x=x, s=s, g=g, loss=loss, surrogate=surrogate, M_x=M_x.detach(), s_mag=s_mag, M_g=M_g, l_mag=l_mag,
                c_out_g=scal(sg, sd)[1], x_in_g=_t4(scal(sg, sd)[2]) * z * gen_sigma)


# ------------------------------------------------------------------------------------------ wiring
def test_entry_points_are_declared_everywhere():
    from dxmi_hip import _lib, ops
    header = open(os.path.join(ROOT, "include", "dxmi_hip.h")).read()
    makefile = open(os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc", "Makefile")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header) and sym in _lib.SIGNATURES
        assert hasattr(ops, sym[len("dxmi_"):])
    assert "dm_train.hip" in re.search(r"^SRCS = (.*)$", makefile, flags=re.M).group(1).split()
    assert "asan_dm" in makefile and "DXMI_DM_W_DMD" in header and "DXMI_DM_W_NONE" in header
    assert ops.DM_WEIGHTINGS == {"dmd": 0, "none": 1}


# ------------------------------------------------------------------------------------------ torch path against float64
@pytest.mark.parametrize("weighting", ["dmd", "none"])
@pytest.mark.parametrize("sd_f", [0.5, 0.25])
def test_torch_path_against_float64(weighting, sd_f):
    S = 18
    z, noise, idx = _operands(S=S)
    gen, real, fake = _Tanh(0.7), _Tanh(0.9, 0.8), _Tanh(0.5, 0.6)
    terms = _diffusion().dm_generator_losses(gen, z, S, real_model=real, real_diffusion=_diffusion(), fake_model=fake,
                                             fake_diffusion=_diffusion(sigma_data=sd_f), noise=noise, indices=idx, weighting=weighting)
    assert set(terms) == {"loss", "x", "dm_norm"}
    assert terms["loss"].shape == (6,) and terms["dm_norm"].shape == (6,) and terms["x"].shape == z.shape
    assert terms["x"].dtype == torch.float32 and not terms["x"].requires_grad and not terms["dm_norm"].requires_grad
    g64, r64, f64 = _Tanh(0.7, dtype=torch.float64), _Tanh(0.9, 0.8, torch.float64), _Tanh(0.5, 0.6, torch.float64)
    r = _restate64(g64, r64, f64, z, noise, idx, S, weighting, sd_f=sd_f)
    ex = float(((terms["x"].double() - r["x"].detach()).abs() / (16 * U * r["M_x"])).max())
    es = float(((terms["dm_norm"].double() - r["s"]).abs() / (64 * U * r["s_mag"])).max())
    el = float(((terms["loss"].detach().double() - r["loss"].detach()).abs() / (64 * U * r["l_mag"])).max())
    print(f"torch path vs fp64 ({weighting}, fake sigma_data {sd_f}): |err| / bound: x {ex:.3f}, dm_norm {es:.3f}, loss {el:.3f}")
    assert ex <= 1 and es <= 1 and el <= 1
    # the gradient: float64 autograd of the surrogate 0.5 mean((x - sg(x - g))^2).  d x / d w = c_out a sech^2(.) x_in and
    # d x / d a = c_out tanh(.), so |d x / d w| <= c_out |a x_in| and |d x / d a| <= c_out; an element's contribution g dx / CHW
    # carries g's error 16 u M_g and 16 u of its own magnitude
    terms["loss"].sum().backward()
    r["surrogate"].sum().backward()
    per_elem = (16 * U * r["M_g"] + 16 * U * r["g"].abs()) * _t4(r["c_out_g"]) / z[0].numel()
    for p, q, dx in ((gen.w, g64.w, abs(float(g64.a.detach())) * r["x_in_g"].abs()), (gen.a, g64.a, torch.ones_like(z, dtype=torch.float64))):
        assert p.grad is not None and float(q.grad) != 0
        err, bound = abs(float(p.grad) - float(q.grad)), float((per_elem * dx).sum())
        print(f"  d loss / d {'w' if p is gen.w else 'a'}: {float(p.grad):.6g} vs {float(q.grad):.6g}, |err| / bound {err / bound:.3f}")
        assert err <= bound
    for net in (real, fake):
        assert all(p.grad is None for p in net.parameters())


def test_no_grad_call_returns_the_same_values():
    S = 18
    z, noise, idx = _operands(S=S)
    nets = _Tanh(0.7), _Tanh(0.9, 0.8), _Tanh(0.5, 0.6)
    kw = dict(real_model=nets[1], real_diffusion=_diffusion(), fake_model=nets[2], noise=noise, indices=idx)
    a = _diffusion().dm_generator_losses(nets[0], z, S, **kw)
    with torch.no_grad():
        b = _diffusion().dm_generator_losses(nets[0], z, S, **kw)
    assert a["loss"].requires_grad and not b["loss"].requires_grad
    for k in ("loss", "x", "dm_norm"):
        assert torch.equal(a[k].detach(), b[k])


# ------------------------------------------------------------------------------------------ fixed points
def test_fake_identical_to_real_is_a_fixed_point():
    z, noise, idx = _operands()
    gen, real = _Tanh(0.7), _Tanh(0.9, 0.8)
    for weighting in ("dmd", "none"):
        gen.zero_grad()
        terms = _diffusion().dm_generator_losses(gen, z, 18, real_model=real, real_diffusion=_diffusion(), fake_model=real, noise=noise,
                                                 indices=idx, weighting=weighting)
        assert torch.equal(terms["loss"], torch.zeros(6))
        terms["loss"].sum().backward()
        assert float(gen.w.grad) == 0.0 and float(gen.a.grad) == 0.0
        assert (terms["dm_norm"] > 0).all()


class _Posterior(torch.nn.Module):
    """The network whose denoiser under KarrasDenoiser.denoise is the posterior mean of N(mu, v): D(x, s) = (v x + s^2 mu) / (v + s^2)."""

    def __init__(self, mu, v, sd=0.5):
        super().__init__()
        self.mu, self.v, self.sd = mu, v, sd

    def forward(self, x_in, t, **kw):
        s = _t4(torch.exp(t / 250))
        c_in = 1 / (s ** 2 + self.sd ** 2) ** 0.5
        c_skip, c_out = self.sd ** 2 / (s ** 2 + self.sd ** 2), s * self.sd / (s ** 2 + self.sd ** 2) ** 0.5
        x_t = x_in / c_in
        return ((self.v * x_t + s ** 2 * self.mu) / (self.v + s ** 2) - c_skip * x_t) / c_out


class _ConstImage(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.theta = torch.nn.Parameter(torch.full((1, 3, 8, 8), -0.8))

    def forward(self, x_in, t, **kw):
        return self.theta.expand(x_in.shape[0], -1, -1, -1)


@pytest.mark.parametrize("weighting", ["dmd", "none"])
def test_one_sgd_step_moves_a_constant_generator_towards_the_real_mean(weighting):
    z, noise, idx = _operands()
    d = _diffusion()
    gen = _ConstImage()
    mu_r = torch.full((1, 3, 8, 8), 0.3)

    def output():      # the generator's image for z = 0: c_out(sigma_max) theta
        with torch.no_grad():
            return d.denoise(gen, torch.zeros(1, 3, 8, 8), torch.tensor([80.0]))[1]
    before = output()
    real, fake = _Posterior(mu_r, 0.01), _Posterior(before.clone(), 0.01)     # the fake denoiser knows the generator's mean
    terms = d.dm_generator_losses(gen, z, 18, real_model=real, real_diffusion=d, fake_model=fake, noise=noise, indices=idx,
                                  weighting=weighting)
    assert (terms["loss"] > 0).all()
    terms["loss"].sum().backward()
    with torch.no_grad():
        gen.theta -= 0.5 * gen.theta.grad
    after = output()
    assert ((after - mu_r).abs() < (before - mu_r).abs()).all()
    assert float((after - mu_r).abs().mean()) < float((before - mu_r).abs().mean())


# ------------------------------------------------------------------------------------------ index draw
def test_index_range():
    from models.cm.karras_diffusion import dm_index_range
    assert dm_index_range(1000) == (math.ceil(0.02 * 999), math.floor(0.98 * 999)) == (20, 979)
    assert dm_index_range(2, 0.0, 1.0) == (0, 1)
    assert dm_index_range(18, 0.0, 1.0) == (0, 17)
    with pytest.raises(ValueError, match="min_step_frac"):
        dm_index_range(1000, 0.9, 0.1)
    with pytest.raises(ValueError, match="no ladder index"):
        dm_index_range(2, 0.4, 0.6)


@pytest.mark.parametrize("S,lo,hi,fracs", [(1000, 20, 979, {}), (2, 0, 1, dict(min_step_frac=0.0, max_step_frac=1.0))])
def test_index_draw_covers_exactly_the_range_and_uses_the_generator(S, lo, hi, fracs):
    from models.cm.karras_diffusion import cd_levels
    tab = cd_levels(S, 0.002, 80.0, 7.0).table
    seen = []

    def real(x_in, t, **kw):
        seen.append(t.clone())
        return torch.zeros_like(x_in)
    N = 20000 if S == 1000 else 64
    z = torch.zeros(N, 1, 2, 2)
    call = lambda gen: _diffusion().dm_generator_losses(_Tanh(0.7), z, S, real_model=real, real_diffusion=_diffusion(), fake_model=_Tanh(0.5),
                                                        generator=gen, **fracs)
    state = torch.get_rng_state()
    a = call(torch.Generator().manual_seed(11))
    b = call(torch.Generator().manual_seed(11))
    c = call(torch.Generator().manual_seed(12))
    assert torch.equal(torch.get_rng_state(), state)              # indices and noise both came from the generator
    assert torch.equal(a["loss"], b["loss"]) and not torch.equal(a["loss"], c["loss"])
    # the levels met: every one inside the range, both ends reached (sigma falls with the index)
    t = seen[0]
    levels = 250 * torch.log(tab[lo:hi + 1])
    assert float(t.max()) == pytest.approx(float(levels[0]), rel=1e-6) and float(t.min()) == pytest.approx(float(levels[-1]), rel=1e-6)
    nearest = (t[:, None] - levels[None, :]).abs().min(dim=1).values
    assert float(nearest.max()) <= 1e-3
    torch.manual_seed(3)
    d1 = call(None)
    torch.manual_seed(3)
    d2 = call(None)
    assert torch.equal(d1["loss"], d2["loss"])                    # without a generator: the global stream


# ------------------------------------------------------------------------------------------ refusals
def test_loss_refusals():
    z, noise, idx = _operands()
    gen, real, fake = _Tanh(0.7), _Tanh(0.9, 0.8), _Tanh(0.5, 0.6)
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx)
    with pytest.raises(NotImplementedError, match="distillation=False"):
        _diffusion(distillation=True).dm_generator_losses(gen, z, 18, **kw)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        _diffusion().dm_generator_losses(gen, z.clone().requires_grad_(True), 18, **kw)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        _diffusion().dm_generator_losses(gen, z, 18, **dict(kw, noise=noise.clone().requires_grad_(True)))
    with pytest.raises(NotImplementedError, match="real_model"):
        _diffusion().dm_generator_losses(gen, z, 18, fake_model=fake)
    with pytest.raises(ValueError, match="weighting"):
        _diffusion().dm_generator_losses(gen, z, 18, weighting="snr", **kw)
    with pytest.raises(ValueError, match="gen_sigma"):
        _diffusion().dm_generator_losses(gen, z, 18, gen_sigma=0.0, **kw)


def test_dm_sample_refusals():
    from dxmi_hip._lib import DxmiError
    from models.cm import karras_diffusion as kd
    with pytest.raises(NotImplementedError, match="--cm_sampler onestep"):
        kd.dm_sample(_diffusion(distillation=True), _Tanh(0.7), (1, 3, 8, 8))
    with pytest.raises(DxmiError, match="HIP device path"):
        kd.dm_sample(_diffusion(), _Tanh(0.7), (1, 3, 8, 8), device="cpu")


def test_command_line_refusals(capsys):
    import cm_train
    import generate_large
    a = cm_train.parse_args(["--training_mode", "dm", "--teacher_model_path", "edm.pt"])         # no data flag is needed
    assert (a.gen_update_every, a.fake_lr, a.dm_weighting, a.dm_num_scales) == (5, 0.0, "dmd", 1000)
    a = cm_train.parse_args(["--training_mode", "dm", "--gen_update_every", "2", "--fake_lr", "2e-4", "--dm_weighting", "none",
                             "--dm_num_scales", "40"])
    assert (a.gen_update_every, a.fake_lr, a.dm_weighting, a.dm_num_scales) == (2, 2e-4, "none", 40)
    for argv, msg in ((["--data_npz", "x.npz"], "--data_npz does not go with --training_mode dm"),
                      (["--ict", "True"], "--ict True"),
                      (["--loss_norm", "l1"], "--loss_norm l1"),
                      (["--loss_norm", "pseudo-huber"], "--loss_norm pseudo-huber"),
                      (["--index_sampler", "lognormal"], "--index_sampler lognormal"),
                      (["--dm_weighting", "snr"], "--dm_weighting"),
                      (["--gen_update_every", "0"], "--gen_update_every"),
                      (["--use_graph", "True"], "--use_graph")):
        with pytest.raises(SystemExit):
            cm_train.parse_args(["--training_mode", "dm"] + argv)
        assert msg in capsys.readouterr().err, argv
    args, _ = generate_large.parse_args(["--log_dir", "x", "--n_sample", "4", "--karras_sampler", "dm", "--pretrained", "model.pt"])
    assert args.karras_sampler == "dm" and args.karras_steps is None and args.pretrained == "model.pt"
    for flag, v in (("--karras_steps", "4"), ("--s_churn", "1.0"), ("--rho", "7"), ("--solver_order", "2"), ("--cm_steps", "3")):
        with pytest.raises(SystemExit):
            generate_large.parse_args(["--log_dir", "x", "--n_sample", "4", "--karras_sampler", "dm", flag, v])
        assert flag in capsys.readouterr().err


# ------------------------------------------------------------------------------------------ DMTrainLoop on the torch path
class _Tiny(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(3, 3, generator=gen) * 0.3)
        self.b = torch.nn.Parameter(torch.randn(3, generator=gen) * 0.1)

    def forward(self, x, t):
        return torch.tanh(torch.einsum("oc,nchw->nohw", self.a, x) + self.b[None, :, None, None] + 1e-3 * _t4(t))


ITERS, EVERY, LR = 7, 3, 1e-2


def _latents():
    gen = torch.Generator().manual_seed(99)
    return [torch.randn(4, 3, 8, 8, generator=gen) for _ in range(ITERS)]


def _loop(tmp, resume="", **over):
    from models.cm.resample import LogNormalSampler
    from models.cm.train_util import DMTrainLoop
    fake = _Tiny(2)
    kw = dict(model=_Tiny(1), diffusion=_diffusion(), real_model=_Tiny(3), real_diffusion=_diffusion(), fake_model=fake, num_scales=18,
              gen_update_every=EVERY, fake_lr=2 * LR, data=None, batch_size=4, microbatch=2, lr=LR, ema_rate="0.9,0.5", log_interval=2,
              save_interval=100, resume_checkpoint=resume, schedule_sampler=LogNormalSampler(), log_dir=str(tmp))
    kw.update(over)
    tl = DMTrainLoop(**kw)
    # the loop's optimisers are the device RAdam; on the CPU torch's own RAdam (its base class, same state dict) stands in
    for name, trainer, lr in (("opt", tl.mp_trainer, LR), ("fake_opt", tl.fake_trainer, 2 * LR)):
        opt = torch.optim.RAdam(trainer.master_params, lr=lr)
        if resume:
            opt.load_state_dict(getattr(tl, name).state_dict())
        setattr(tl, name, opt)
    return tl


def _flat(ps):
    return torch.cat([p.detach().reshape(-1) for p in ps])


def _run(tl, k, z):
    torch.manual_seed(1000 + k)          # the draws of iteration k: indices, noise, sigmas and the DSM noise, from the global stream
    return tl.run_step(z[k], {})


def test_dmtrainloop_two_clocks_save_resume(tmp_path):
    z = _latents()
    tl = _loop(tmp_path)
    assert not tl.real_model.training and not any(p.requires_grad for p in tl.real_model.parameters())
    assert tl.fake_opt.param_groups[0]["lr"] == 2 * LR and tl.opt.param_groups[0]["lr"] == LR
    real0 = _flat(tl.real_model.parameters()).clone()
    gens, fakes, emas = {}, {}, {}
    g_prev, f_prev, e_prev = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone(), _flat(tl.ema_params[0]).clone()
    for k in range(ITERS):
        assert tl.step == k
        took_gen, took_fake = _run(tl, k, z)
        gens[k], fakes[k] = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
        emas[k] = torch.cat([_flat(e) for e in tl.ema_params]).clone()
        on = k % EVERY == 0
        assert took_gen == on and took_fake
        assert torch.equal(gens[k], g_prev) != on, k                        # the generator moves on iterations 0, 3, 6 only
        assert not torch.equal(fakes[k], f_prev), k                         # the fake denoiser on every one
        assert torch.equal(_flat(tl.ema_params[0]), e_prev) != on, k       # the EMAs with the generator
        assert torch.equal(_flat(tl.real_model.parameters()), real0)
        g_prev, f_prev, e_prev = gens[k], fakes[k], _flat(tl.ema_params[0]).clone()
        if tl.step == 4:
            tl.save()
    assert tl.step == ITERS
    row = tl.dumpkvs()
    assert {"loss", "dm_norm", "fake_mse", "fake_xs_mse", "step"} <= set(row)
    files = set(os.listdir(tmp_path))
    assert {"model000004.pt", "opt000004.pt", "ema_0.9_000004.pt", "ema_0.5_000004.pt", "fake_model000004.pt", "fake_opt000004.pt"} <= files
    sd = torch.load(tmp_path / "fake_model000004.pt")
    assert torch.equal(torch.cat([sd["a"].reshape(-1), sd["b"].reshape(-1)]), fakes[3])

    tr = _loop(tmp_path, resume=str(tmp_path / "model000004.pt"))
    assert tr.step == 4
    assert torch.equal(_flat(tr.model.parameters()), gens[3]) and torch.equal(_flat(tr.fake_model.parameters()), fakes[3])
    for k in (4, 5, 6):
        _run(tr, k, z)
        assert torch.equal(_flat(tr.model.parameters()), gens[k]), k
        assert torch.equal(_flat(tr.fake_model.parameters()), fakes[k]), k
        assert torch.equal(torch.cat([_flat(e) for e in tr.ema_params]), emas[k]), k
    assert tr.step == ITERS

    os.remove(tmp_path / "fake_model000004.pt")
    with pytest.raises(FileNotFoundError, match="fake_model000004"):
        _loop(tmp_path, resume=str(tmp_path / "model000004.pt"))


def test_dmtrainloop_refusals(tmp_path):
    with pytest.raises(NotImplementedError, match="use_graph"):
        _loop(tmp_path, use_graph=True)
    with pytest.raises(NotImplementedError, match="fake_model"):
        _loop(tmp_path, fake_model=None)
    with pytest.raises(ValueError, match="gen_update_every"):
        _loop(tmp_path, gen_update_every=0)


# ------------------------------------------------------------------------------------------ host sanitizers
def test_dm_entry_points_under_address_and_ub_sanitizers():
    """`make asan_dm` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_dm.c, a program with its own main, against it and a no-device HIP runtime stub.  Null, misaligned and
    out-of-range arguments of the five dxmi_dm_* entry points must each come back as DXMI_EINVAL with the message of their check: no
    crash, no sanitizer report.  The program runs as a child process; nothing is loaded into python.  A host-only build: machines
    without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_dm"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_dm")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") == 77        # every case of the driver
