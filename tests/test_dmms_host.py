"""Host side of the K-step distribution-matching generator (DMD2's backward simulation): the wiring of the five
dxmi_dmms_* entry points, K = 1 against the one-step call, the torch path of dm_generator_losses(gen_sigmas=...) against a float64
restatement with a linear generator, the stop-gradient around the simulation, the draws and their order, the refusals, the
command lines, DMTrainLoop at K = 3 on small nn.Modules, and the C entry points under the host sanitizers.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_dm_host import _Tanh, _diffusion, _flat, _latents, _loop, _operands, _run, _t4, EVERY, ITERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SYMBOLS = ("dxmi_dmms_in", "dxmi_dmms_stage", "dxmi_dmms_prep", "dxmi_dmms_out", "dxmi_dmms_bwd")
LADDER = (80.0, 5.0, 0.5)


# ------------------------------------------------------------------------------------------ wiring
def test_entry_points_are_declared_everywhere():
    from dxmi_hip import _lib, ops
    header = open(os.path.join(ROOT, "include", "dxmi_hip.h")).read()
    makefile = open(os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc", "Makefile")).read()
    lib = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "dxmi_hip", "libdxmi_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header) and sym in _lib.SIGNATURES
        assert hasattr(ops, sym[len("dxmi_"):])
        assert re.search(r"\bT %s$" % sym, exported, flags=re.M), sym
    assert "asan_dmms" in makefile and "section 4.4" in header
    # the ctypes table has one entry per parameter of the header's declaration
    for sym in SYMBOLS:
        decl = re.search(r"\bint %s\(([^;]*)\);" % sym, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[sym][1]), sym


def test_dm_step_sigmas():
    from models.cm.karras_diffusion import dm_step_sigmas
    s = dm_step_sigmas(4, 80.0, 0.3)
    assert len(s) == 4 and s[0] == 80.0 and s[-1] == float(torch.tensor(0.3, dtype=torch.float32))
    assert all(a > b for a, b in zip(s, s[1:])) and all(float(torch.tensor(v, dtype=torch.float32)) == v for v in s)
    rho = 7.0
    mid = (80.0 ** (1 / rho) + (1 / 3) * (0.3 ** (1 / rho) - 80.0 ** (1 / rho))) ** rho
    assert s[1] == pytest.approx(mid, rel=1e-6)
    assert dm_step_sigmas(1, 80.0, 0.3) == (80.0,)
    for bad in ((0, 80.0, 0.3), (3, 0.3, 80.0), (3, 80.0, 0.0), (3, float("inf"), 1.0), (2, 5.0, 5.0)):
        with pytest.raises(ValueError):
            dm_step_sigmas(*bad)


# ------------------------------------------------------------------------------------------ K = 1 is the one-step path
@pytest.mark.parametrize("sigma", [80.0, 2.5])
def test_one_level_is_the_one_step_call(sigma):
    z, _, _ = _operands()
    real, fake = _Tanh(0.9, 0.8), _Tanh(0.5, 0.6)
    out, grads, states = [], [], []
    for how in (dict(gen_sigma=sigma), dict(gen_sigmas=[sigma])):
        gen = _Tanh(0.7)
        rng = torch.Generator().manual_seed(17)
        t = _diffusion().dm_generator_losses(gen, z, 18, real_model=real, real_diffusion=_diffusion(), fake_model=fake, generator=rng, **how)
        t["loss"].sum().backward()
        out.append(t)
        grads.append([p.grad.clone() for p in gen.parameters()])
        states.append(rng.get_state())
    assert set(out[0]) == {"loss", "x", "dm_norm"} and set(out[1]) == {"loss", "x", "dm_norm", "steps"}
    for k in ("loss", "x", "dm_norm"):
        assert torch.equal(out[0][k].detach(), out[1][k].detach()), k
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert torch.equal(states[0], states[1])                    # no extra draw was made
    assert torch.equal(out[1]["steps"], torch.zeros(6, dtype=torch.int64))


# ------------------------------------------------------------------------------------------ the simulation against float64
class _Linear(torch.nn.Module):
    """F = a x_in + b: every G_j is affine in x, so x_j has the closed form of a product of affine maps."""

    def __init__(self, a, b, dtype=torch.float32):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(a, dtype=dtype))
        self.b = torch.nn.Parameter(torch.tensor(b, dtype=dtype))

    def forward(self, x_in, t, **kw):
        return self.a * x_in + self.b


def _scal(sigma, sd=0.5):
    return (sd ** 2 / (sigma ** 2 + sd ** 2), sigma * sd / (sigma ** 2 + sd ** 2) ** 0.5, 1 / (sigma ** 2 + sd ** 2) ** 0.5)


def _sim_operands(N=5, shape=(3, 8, 8), K=3, S=18, seed=9):
    gen = torch.Generator().manual_seed(seed)
    z, noise = torch.randn(N, *shape, generator=gen), torch.randn(N, *shape, generator=gen)
    sim = torch.randn(K - 1, N, *shape, generator=gen)
    idx = torch.randint(0, S, (N,), generator=gen)
    idx[0], idx[1] = 0, S - 1
    steps = torch.tensor([0, 1, 2, 2, 1])[:N]
    return z, noise, sim, idx, steps


def _restate64(gen, real, fake, z, noise, sim, idx, steps, S, ladder=LADDER, weighting="dmd", sd=0.5):
    """dm_generator_losses(gen_sigmas=ladder) in float64 with the linear generator `gen` -> the values and the magnitudes of
    test_dm_host._restate64, with M_x grown through the simulation: a stage's rounding error (16 u of the magnitudes that meet in
    x') is carried through every later G_j by its slope |A_j| = |c_skip + c_out a c_in|."""
    from models.cm.karras_diffusion import cd_levels
    d = torch.float64
    z, noise, sim = z.to(d), noise.to(d), sim.to(d)
    sig = torch.tensor(ladder, dtype=torch.float32).to(d)
    t = cd_levels(S, 0.002, 80.0, 7.0).table.to(d)[idx]
    a, b = float(gen.a.detach()), float(gen.b.detach())
    x_k = z * sig[0]
    M_k = x_k.abs()
    for j in range(len(ladder) - 1):
        cs, co, ci = _scal(sig[j], sd)
        D = (cs + co * a * ci) * x_k + co * b                                   # the closed form of G_j
        nxt = D + sim[j] * sig[j + 1]
        own = co * (abs(a) * ci * x_k.abs() + abs(b)) + (cs * x_k).abs() + (sim[j] * sig[j + 1]).abs()
        live = _t4(steps > j)
        M_k = torch.where(live, (cs + co * a * ci).abs() * M_k + own, M_k)
        x_k = torch.where(live, nxt, x_k)
    sk = sig[steps]
    cs, co, ci = (_t4(v) for v in _scal(sk, sd))
    x_in = ci * x_k
    x = co * gen(x_in, None) + cs * x_k
    M_x = ((cs + co * a * ci).abs() * M_k + co * (abs(a) * x_in.abs() + abs(b)) + (cs * x_k).abs()).detach()

    def denoise(net, x_t, sigma, sd):
        c_skip, c_out, c_in = _scal(sigma, sd)
        xi, tm = _t4(c_in) * x_t, 250 * torch.log(sigma)
        F = net(xi, tm)
        na, nw = abs(float(net.a.detach())), abs(float(net.w.detach()))
        arg = _t4(c_out) * na * (nw * xi.abs() + 1e-3 * _t4(tm.abs()))
        return _t4(c_out) * F + _t4(c_skip) * x_t, (_t4(c_out) * F).abs() + (_t4(c_skip) * x_t).abs() + arg, _t4(c_out * na * nw * c_in + c_skip)
    with torch.no_grad():
        x_t = x + noise * _t4(t)
        M_xt = M_x + (noise * _t4(t)).abs()
        d_r, M_r, L_r = denoise(real, x_t, t, sd)
        d_f, M_f, L_f = denoise(fake, x_t, t, sd)
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
    return dict(x=x, x_k=x_k, s=s, g=g, loss=loss, surrogate=surrogate, M_x=M_x, M_k=M_k, s_mag=s_mag, M_g=M_g, l_mag=l_mag, c_out=co,
                c_in=ci, x_in=x_in.detach())


@pytest.mark.parametrize("weighting", ["dmd", "none"])
def test_simulation_against_float64(weighting):
    S = 18
    z, noise, sim, idx, steps = _sim_operands()
    assert set(steps.tolist()) == {0, 1, 2}
    gen, real, fake = _Linear(0.6, 0.05), _Tanh(0.9, 0.8), _Tanh(0.5, 0.6)
    terms = _diffusion().dm_generator_losses(gen, z, S, real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise,
                                             indices=idx, weighting=weighting, gen_sigmas=LADDER, steps=steps, sim_noise=sim)
    assert set(terms) == {"loss", "x", "dm_norm", "steps"} and torch.equal(terms["steps"], steps)
    assert terms["x"].dtype == torch.float32 and not terms["x"].requires_grad
    g64 = _Linear(0.6, 0.05, torch.float64)
    r = _restate64(g64, _Tanh(0.9, 0.8, torch.float64), _Tanh(0.5, 0.6, torch.float64), z, noise, sim, idx, steps, S, weighting=weighting)
    ex = float(((terms["x"].double() - r["x"].detach()).abs() / (16 * U * r["M_x"])).max())
    es = float(((terms["dm_norm"].double() - r["s"]).abs() / (64 * U * r["s_mag"])).max())
    el = float(((terms["loss"].detach().double() - r["loss"].detach()).abs() / (64 * U * r["l_mag"])).max())
    print(f"K = 3 torch path vs fp64 ({weighting}): |err| / bound: x {ex:.3f}, dm_norm {es:.3f}, loss {el:.3f}")
    assert ex <= 1 and es <= 1 and el <= 1
    # the gradient: d x / d a = c_out x_in, d x / d b = c_out, both of the GRADED evaluation alone; the fp32 x_in carries the
    # simulation's error c_in 16 u M_k
    terms["loss"].sum().backward()
    r["surrogate"].sum().backward()
    CHW = z[0].numel()
    per_elem = (16 * U * r["M_g"] + 16 * U * r["g"].abs()) * r["c_out"] / CHW
    extra = r["g"].abs() * r["c_out"] * r["c_in"] * 16 * U * r["M_k"] / CHW
    for name, p, q, bound in (("a", gen.a, g64.a, float((per_elem * r["x_in"].abs() + extra).sum())), ("b", gen.b, g64.b, float(per_elem.sum()))):
        assert p.grad is not None and float(q.grad) != 0
        err = abs(float(p.grad) - float(q.grad))
        print(f"  d loss / d {name}: {float(p.grad):.6g} vs {float(q.grad):.6g}, |err| / bound {err / bound:.3f}")
        assert err <= bound
    for net in (real, fake):
        assert all(p.grad is None for p in net.parameters())


def test_no_gradient_through_the_simulation():
    from models.cm import karras_diffusion as kd
    S = 18
    z, noise, sim, idx, steps = _sim_operands()
    real, fake, d = _Tanh(0.9, 0.8), _Tanh(0.5, 0.6), _diffusion()
    gen = _Tanh(0.7)
    terms = d.dm_generator_losses(gen, z, S, real_model=real, real_diffusion=d, fake_model=fake, noise=noise, indices=idx,
                                  gen_sigmas=LADDER, steps=steps, sim_noise=sim)
    terms["loss"].sum().backward()
    # the one-step expressions on the precomputed, detached x_k
    ref = _Tanh(0.7)
    sig = torch.tensor(LADDER, dtype=torch.float32)
    with torch.no_grad():
        x_k = z * LADDER[0]
        for j in range(2):
            nxt = d.denoise(ref, x_k, sig[j].expand(5))[1] + sim[j] * LADDER[j + 1]
            x_k = torch.where(_t4(steps > j), nxt, x_k)
    x = d.denoise(ref, x_k.detach(), sig[steps])[1]
    with torch.no_grad():
        t = kd.cd_levels(S, 0.002, 80.0, 7.0).table[idx]
        x_t = x + noise * _t4(t)
        d_r, d_f = d.denoise(real, x_t, t)[1], d.denoise(fake, x_t, t)[1]
        s = (x - d_r).abs().flatten(1).mean(1)
        g = (d_f - d_r) / _t4(s)
    loss = kd._DMSurrogate.apply(x, g)
    loss.sum().backward()
    assert torch.equal(terms["x"], x.detach()) and torch.equal(terms["loss"].detach(), loss.detach())
    for p, q in zip(gen.parameters(), ref.parameters()):
        assert torch.equal(p.grad, q.grad)
    # and the no-grad call returns the same values
    with torch.no_grad():
        again = d.dm_generator_losses(gen, z, S, real_model=real, real_diffusion=d, fake_model=fake, noise=noise, indices=idx,
                                      gen_sigmas=LADDER, steps=steps, sim_noise=sim)
    assert all(torch.equal(again[k], terms[k].detach()) for k in ("loss", "x", "dm_norm"))


# ------------------------------------------------------------------------------------------ draws
def test_step_draws_cover_the_ladder_and_use_the_generator():
    z = torch.zeros(64, 1, 2, 2)
    nets = dict(real_model=_Tanh(0.9, 0.8), real_diffusion=_diffusion(), fake_model=_Tanh(0.5))
    call = lambda gen: _diffusion().dm_generator_losses(_Tanh(0.7), z, 18, generator=gen, gen_sigmas=LADDER, **nets)
    state = torch.get_rng_state()
    a, b, c = call(torch.Generator().manual_seed(11)), call(torch.Generator().manual_seed(11)), call(torch.Generator().manual_seed(12))
    assert torch.equal(torch.get_rng_state(), state)                          # every draw came from the generator
    assert a["steps"].dtype == torch.int64 and set(a["steps"].tolist()) == {0, 1, 2}
    assert torch.equal(a["steps"], b["steps"]) and torch.equal(a["loss"], b["loss"]) and not torch.equal(a["steps"], c["steps"])
    torch.manual_seed(3)
    d1 = call(None)
    torch.manual_seed(3)
    d2 = call(None)
    assert torch.equal(d1["steps"], d2["steps"]) and torch.equal(d1["loss"], d2["loss"])     # without one: the global stream


def test_draw_order():
    """steps, then indices, noise (5.32's draws), then one simulation noise per stage in stage order."""
    from models.cm.karras_diffusion import dm_index_range
    N, S, K = 6, 18, 3
    z, _, _ = _operands(N=N)
    nets = dict(real_model=_Tanh(0.9, 0.8), real_diffusion=_diffusion(), fake_model=_Tanh(0.5, 0.6))
    drawn = _diffusion().dm_generator_losses(_Tanh(0.7), z, S, generator=torch.Generator().manual_seed(23), gen_sigmas=LADDER, **nets)
    rng = torch.Generator().manual_seed(23)
    steps = torch.randint(0, K, (N,), generator=rng)
    lo, hi = dm_index_range(S)
    idx = torch.randint(lo, hi + 1, (N,), generator=rng)
    noise = torch.randn(z.shape, generator=rng)
    sim = torch.stack([torch.randn(z.shape, generator=rng) for _ in range(K - 1)])
    given = _diffusion().dm_generator_losses(_Tanh(0.7), z, S, gen_sigmas=LADDER, steps=steps, indices=idx, noise=noise, sim_noise=sim, **nets)
    assert torch.equal(drawn["steps"], steps)
    assert all(torch.equal(drawn[k].detach(), given[k].detach()) for k in ("loss", "x", "dm_norm"))


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    z, noise, idx = _operands()
    gen, real, fake, d = _Tanh(0.7), _Tanh(0.9, 0.8), _Tanh(0.5, 0.6), _diffusion()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx)
    nan, inf = float("nan"), float("inf")
    for ladder in ((5.0, 80.0), (80.0, 80.0), (80.0, 5.0, 5.0), (80.0, 0.0), (80.0, -1.0), (nan, 1.0), (inf, 1.0), (80.0, nan), (),
                   (1.0, 1.0 + 1e-9)):
        with pytest.raises(ValueError, match="gen_sigmas"):
            d.dm_generator_losses(gen, z, 18, gen_sigmas=ladder, **kw)
    with pytest.raises(ValueError, match="excludes gen_sigma"):
        d.dm_generator_losses(gen, z, 18, gen_sigma=80.0, gen_sigmas=LADDER, **kw)
    with pytest.raises(NotImplementedError, match="K = 1 only"):
        d.sid_generator_losses(gen, z, 18, gen_sigmas=LADDER, **kw)
    with pytest.raises(ValueError, match="excludes gen_sigma"):
        d.sid_generator_losses(gen, z, 18, gen_sigma=2.5, gen_sigmas=[2.5], **kw)
    one = d.sid_generator_losses(gen, z, 18, gen_sigmas=[2.5], **kw)            # one level is SiD's one-step generator
    assert torch.equal(one["loss"].detach(), d.sid_generator_losses(gen, z, 18, gen_sigma=2.5, **kw)["loss"].detach())
    good = torch.tensor([0, 1, 2, 2, 1, 0])
    for steps in (torch.tensor([0, 1, 2, 3, 1, 0]), torch.tensor([0, -1, 2, 2, 1, 0]), good[:5], good.to(torch.int32), good.reshape(2, 3),
                  [0, 1, 2, 2, 1, 0]):
        with pytest.raises(ValueError, match="steps"):
            d.dm_generator_losses(gen, z, 18, gen_sigmas=LADDER, steps=steps, **kw)
    for shape in ((3, 6, 3, 8, 8), (2, 5, 3, 8, 8), (2, 6, 3, 8, 4), (6, 3, 8, 8)):
        with pytest.raises(ValueError, match="sim_noise"):
            d.dm_generator_losses(gen, z, 18, gen_sigmas=LADDER, steps=good, sim_noise=torch.zeros(shape), **kw)
    with pytest.raises(ValueError, match="give gen_sigmas"):
        d.dm_generator_losses(gen, z, 18, steps=good, **kw)
    with pytest.raises(ValueError, match="give gen_sigmas"):
        d.dm_generator_losses(gen, z, 18, sim_noise=torch.zeros(2, 6, 3, 8, 8), **kw)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        d.dm_generator_losses(gen, z, 18, gen_sigmas=LADDER, sim_noise=torch.zeros(2, 6, 3, 8, 8, requires_grad=True), **kw)


def test_dm_sample_refusals():
    from dxmi_hip._lib import DxmiError
    from models.cm import karras_diffusion as kd
    with pytest.raises(ValueError, match="excludes gen_sigma"):
        kd.dm_sample(_diffusion(), _Tanh(0.7), (1, 3, 8, 8), gen_sigma=80.0, gen_sigmas=LADDER, device="cpu")
    with pytest.raises(ValueError, match="gen_sigmas"):
        kd.dm_sample(_diffusion(), _Tanh(0.7), (1, 3, 8, 8), gen_sigmas=(1.0, 2.0), device="cpu")
    with pytest.raises(DxmiError, match="HIP device path"):
        kd.dm_sample(_diffusion(), _Tanh(0.7), (1, 3, 8, 8), gen_sigmas=LADDER, device="cpu")


def test_command_line(capsys):
    import cm_train
    import generate_large
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    a = cm_train.parse_args(["--training_mode", "dm", "--gen_sigmas", "80,5,1,0.3"])
    assert a.gen_sigmas == (80.0, 5.0, 1.0, f32(0.3)) and a.gen_sigma == 0.0
    assert cm_train.parse_args(["--training_mode", "dm"]).gen_sigmas is None
    assert cm_train.parse_args(["--training_mode", "dm", "--dm_objective", "sid", "--gen_sigmas", "2.5"]).gen_sigmas == (2.5,)
    for argv, msg in ((["--training_mode", "dm", "--gen_sigmas", "80,5", "--gen_sigma", "80"], "does not go with --gen_sigma"),
                      (["--training_mode", "dm", "--gen_sigmas", "80,5", "--dm_objective", "sid"], "--dm_objective sid"),
                      (["--training_mode", "dm", "--gen_sigmas", "5,80"], "decrease strictly"),
                      (["--training_mode", "dm", "--gen_sigmas", "80,x"], "comma-separated"),
                      (["--training_mode", "dm", "--gen_sigmas", "80,0"], "positive and finite"),
                      (["--training_mode", "consistency_distillation", "--gen_sigmas", "80,5"], "belongs to --training_mode dm")):
        with pytest.raises(SystemExit):
            cm_train.parse_args(argv)
        assert msg in capsys.readouterr().err, argv
    base = ["--log_dir", "x", "--n_sample", "4", "--pretrained", "model.pt"]
    args, _ = generate_large.parse_args(base + ["--karras_sampler", "dm", "--gen_sigmas", "80,5,1,0.3", "--generator", "determ"])
    assert args.gen_sigmas == (80.0, 5.0, 1.0, f32(0.3)) and args.generator == "determ"
    args, _ = generate_large.parse_args(base + ["--karras_sampler", "dm"])
    assert args.gen_sigmas is None and args.gen_sigma == 0.0
    for argv, msg in ((["--karras_sampler", "dm", "--gen_sigmas", "80,5", "--gen_sigma", "80"], "does not go with --gen_sigma"),
                      (["--karras_sampler", "heun", "--gen_sigmas", "80,5"], "only applies with --karras_sampler dm"),
                      (["--karras_sampler", "dm", "--gen_sigmas", "1,2"], "decrease strictly")):
        with pytest.raises(SystemExit):
            generate_large.parse_args(base + argv)
        assert msg in capsys.readouterr().err, argv


# ------------------------------------------------------------------------------------------ DMTrainLoop on the torch path
def test_dmtrainloop_three_steps_two_clocks_save_resume(tmp_path):
    z = _latents()
    tl = _loop(tmp_path, gen_sigmas=LADDER)
    assert tl.gen_sigmas == LADDER and tl.gen_sigma is None
    gens, fakes, emas = {}, {}, {}
    g_prev, f_prev = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
    for k in range(ITERS):
        took_gen, took_fake = _run(tl, k, z)
        gens[k], fakes[k] = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
        emas[k] = torch.cat([_flat(e) for e in tl.ema_params]).clone()
        on = k % EVERY == 0
        assert took_gen == on and took_fake
        assert torch.equal(gens[k], g_prev) != on, k                         # the generator moves on its turns only
        assert not torch.equal(fakes[k], f_prev), k
        g_prev, f_prev = gens[k], fakes[k]
        if tl.step == 4:
            tl.save()
    files = set(os.listdir(tmp_path))                                        # the checkpoint's files are the one-step loop's
    assert {"model000004.pt", "opt000004.pt", "ema_0.9_000004.pt", "ema_0.5_000004.pt", "fake_model000004.pt", "fake_opt000004.pt"} == \
        {f for f in files if f.endswith(".pt")}
    one = _loop(tmp_path / "one")                                            # the ladder changes what is trained
    _run(one, 0, z)
    assert not torch.equal(_flat(one.model.parameters()), gens[0])
    tr = _loop(tmp_path, resume=str(tmp_path / "model000004.pt"), gen_sigmas=LADDER)
    assert tr.step == 4 and torch.equal(_flat(tr.model.parameters()), gens[3])
    for k in (4, 5, 6):
        _run(tr, k, z)
        assert torch.equal(_flat(tr.model.parameters()), gens[k]), k
        assert torch.equal(_flat(tr.fake_model.parameters()), fakes[k]), k
        assert torch.equal(torch.cat([_flat(e) for e in tr.ema_params]), emas[k]), k


def test_dmtrainloop_refusals(tmp_path):
    with pytest.raises(NotImplementedError, match="one-step generator"):
        _loop(tmp_path, gen_sigmas=LADDER, objective="sid")
    with pytest.raises(ValueError, match="excludes gen_sigma"):
        _loop(tmp_path, gen_sigmas=LADDER, gen_sigma=80.0)
    with pytest.raises(ValueError, match="gen_sigmas"):
        _loop(tmp_path, gen_sigmas=(1.0, 2.0))
    assert _loop(tmp_path, gen_sigmas=[2.5], objective="sid").gen_sigmas == (2.5,)


# ------------------------------------------------------------------------------------------ host sanitizers
def test_dmms_entry_points_under_address_and_ub_sanitizers():
    """`make asan_dmms` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_dmms.c, a program with its own main, against it and a no-device HIP runtime stub.  Null, misaligned and
    out-of-range arguments of the five dxmi_dmms_* entry points must each come back as DXMI_EINVAL with the message of their check: no
    crash, no sanitizer report.  The program runs as a child process; nothing is loaded into python.  A host-only build: machines
    without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_dmms"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_dmms")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") == 83        # every case of the driver
