"""Host side of score identity distillation: the torch path of KarrasDenoiser.sid_generator_losses on float64 analytic
denoisers against an independent statement of the loss that torch.autograd differentiates as a whole (the denoisers' Jacobians
included), a negative control without those Jacobians, the s == 0 convention, DMTrainLoop(objective="sid") on the CPU with save /
resume, objective="dmd" against a loop built without the argument, the new command-line flags, and the C entry points of
csrc/sid_train.hip under the host sanitizers.  No GPU.

models.cm.unet_train.input_vjp has no CPU path (it walks the HIP U-Net's tape), so its equality with input_forward followed by
input_backward is asserted in tests/test_hip_sid_train.py."""
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_dm_host import EVERY, ITERS, _diffusion, _flat, _latents, _loop, _run, _t4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dxmi_sid_grad_fwd", "dxmi_sid_join")
D64 = torch.float64
SHAPE, N, S = (3, 4, 4), 5, 18
ALPHAS = (1.0, 1.2)


class _Dense(torch.nn.Module):
    """F(x_in, t) = A x_in + b + c t on the flattened image, A dense (48 x 48): a denoiser D = c_out F + c_skip x_t whose Jacobian
    in x_t couples every pixel with every other.  float64 parameters."""

    def __init__(self, seed, scale, bias=True):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        n = math.prod(SHAPE)
        self.A = torch.nn.Parameter(torch.randn(n, n, generator=gen, dtype=D64) * scale / math.sqrt(n))
        self.b = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=D64) * (0.3 if bias else 0.0))
        self.c = 1e-3 if bias else 0.0

    def forward(self, x_in, t, **kw):
        flat = x_in.flatten(1) @ self.A.T + self.b + self.c * t[:, None]
        return flat.view(x_in.shape)


def _operands(seed=5):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(N, *SHAPE, generator=gen, dtype=D64)
    noise = torch.randn(N, *SHAPE, generator=gen, dtype=D64)
    idx = torch.tensor([0, S - 1, 7, 9, 12])
    return z, noise, idx


def _nets(bias=True):
    return _Dense(1, 0.8, bias), _Dense(2, 1.1, bias), _Dense(3, 0.6, bias)


def _scal32(sigma, sd, distill=False, smin=0.002):
    """The scalings on the fp32 level, as KarrasDenoiser forms them (restated: the float64 comparison below needs the same fp32
    coefficients, not float64 ones)."""
    den = sigma ** 2 + sd ** 2
    if distill:
        return sd ** 2 / ((sigma - smin) ** 2 + sd ** 2), (sigma - smin) * sd / den ** 0.5, 1 / den ** 0.5
    return sd ** 2 / den, sigma * sd / den ** 0.5, 1 / den ** 0.5


def _statement(gen, real, fake, z, noise, idx, alpha, gen_sigma=80.0, sd_f=0.5, dist_f=False, jacobians=True, skip=()):
    """The loss of the issue, written as ONE expression of the generator's parameters and differentiated by autograd as a whole:
    loss_n = ((1 - alpha) sum(delta^2) + sum(delta (D_f - x))) / (CHW sg(s_n)), delta = D_r - D_f, s = mean|x - D_r|.
    jacobians=False: the denoisers see x_t.detach() (the negative control).  skip: samples left out of the sum (s == 0 there).
    -> (loss [N], s [N], {generator parameter: gradient of loss.sum()})."""
    from models.cm.karras_diffusion import cd_levels
    t = cd_levels(S, 0.002, 80.0, 7.0).table[idx]                       # fp32 levels
    sg = torch.full((N,), gen_sigma, dtype=torch.float32)

    def denoise(net, x_t, sigma, sd, distill=False):
        c_skip, c_out, c_in = (_t4(c) for c in _scal32(sigma, sd, distill))
        return c_out * net(c_in * x_t, 250 * torch.log(sigma + 1e-44)) + c_skip * x_t
    x = denoise(gen, z * gen_sigma, sg, 0.5)
    x_t = x + noise * _t4(t)
    fed = x_t if jacobians else x_t.detach()
    D_r, D_f = denoise(real, fed, t, 0.5), denoise(fake, fed, t, sd_f, dist_f)
    s = (x - D_r).abs().flatten(1).mean(dim=1).detach()
    delta = D_r - D_f
    total = ((1 - alpha) * delta ** 2 + delta * (D_f - x)).flatten(1).sum(dim=1)
    keep = torch.tensor([n not in skip for n in range(N)])
    loss = torch.where(keep, total / (math.prod(SHAPE) * torch.where(keep, s, torch.ones_like(s))), torch.zeros_like(s))
    params = list(gen.parameters())
    grads = torch.autograd.grad(loss.sum(), params)
    return loss.detach(), s, dict(zip(params, grads))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ------------------------------------------------------------------------------------------ wiring
def test_entry_points_are_declared_everywhere():
    from dxmi_hip import _lib, ops
    header = open(os.path.join(ROOT, "include", "dxmi_hip.h")).read()
    makefile = open(os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc", "Makefile")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header) and sym in _lib.SIGNATURES
        assert hasattr(ops, sym[len("dxmi_"):])
    assert "sid_train.hip" in re.search(r"^SRCS = (.*)$", makefile, flags=re.M).group(1).split()
    assert "asan_sid" in makefile


# ------------------------------------------------------------------------------------------ torch path against autograd
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("sd_f,dist_f", [(0.5, False), (0.25, False), (0.5, True)])
def test_torch_path_against_autograd_of_the_whole_loss(alpha, sd_f, dist_f):
    z, noise, idx = _operands()
    gen, real, fake = _nets()
    terms = _diffusion().sid_generator_losses(gen, z, S, real_model=real, real_diffusion=_diffusion(), fake_model=fake,
                                              fake_diffusion=_diffusion(sigma_data=sd_f, distillation=dist_f), noise=noise, indices=idx,
                                              alpha=alpha)
    assert set(terms) == {"loss", "x", "dm_norm"}
    assert terms["loss"].shape == (N,) and terms["dm_norm"].shape == (N,) and terms["x"].shape == z.shape
    assert terms["loss"].requires_grad and not terms["x"].requires_grad and not terms["dm_norm"].requires_grad
    assert terms["x"].dtype == torch.float32
    terms["loss"].sum().backward()
    ref_loss, ref_s, ref_grads = _statement(gen, real, fake, z, noise, idx, alpha, sd_f=sd_f, dist_f=dist_f)
    el, es = _rel(terms["loss"].detach(), ref_loss), _rel(terms["dm_norm"], ref_s)
    eg = max(_rel(p.grad, g) for p, g in ref_grads.items())
    print(f"sid torch path vs autograd (alpha {alpha}, fake sigma_data {sd_f}, distillation {dist_f}): relative error loss {el:.2e}, "
          f"dm_norm {es:.2e}, generator gradients {eg:.2e}")
    assert el <= 1e-12 and es <= 1e-12 and eg <= 1e-12
    assert all(float(g.abs().max()) > 0 for g in ref_grads.values())
    for net in (real, fake):
        assert all(p.grad is None for p in net.parameters())
    # negative control: without the Jacobian paths (the denoisers fed x_t.detach()) the gradient is another one
    _, _, twin = _statement(gen, real, fake, z, noise, idx, alpha, sd_f=sd_f, dist_f=dist_f, jacobians=False)
    apart = min(_rel(p.grad, g) for p, g in twin.items())
    print(f"  the twin without Jacobian paths differs from the path's gradients by at least {apart:.3f} (relative, per parameter)")
    assert apart >= 1e-2


def test_alpha_changes_the_loss_and_no_grad_returns_the_same_values():
    z, noise, idx = _operands()
    gen, real, fake = _nets()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx)
    a = _diffusion().sid_generator_losses(gen, z, S, **kw)                       # alpha = 1.2 by default
    b = _diffusion().sid_generator_losses(gen, z, S, alpha=1.2, **kw)
    c = _diffusion().sid_generator_losses(gen, z, S, alpha=1.0, **kw)
    assert torch.equal(a["loss"], b["loss"]) and not torch.equal(a["loss"], c["loss"]) and torch.equal(a["dm_norm"], c["dm_norm"])
    with torch.no_grad():
        v = _diffusion().sid_generator_losses(gen, z, S, **kw)
    assert a["loss"].requires_grad and not v["loss"].requires_grad
    for k in ("loss", "x", "dm_norm"):
        assert torch.equal(a[k].detach(), v[k])
    assert all(p.grad is None for net in (real, fake) for p in net.parameters())


@pytest.mark.parametrize("alpha", ALPHAS)
def test_zero_normaliser_gives_zeros_and_no_nan(alpha):
    """Sample 1: z = 0 and noise = 0 through nets without bias give x = 0 = x_t = D_r, so s == 0 exactly: loss 0, and that
    sample adds nothing to the gradient (the statement leaves it out of its sum)."""
    z, noise, idx = _operands()
    z[1], noise[1] = 0, 0
    gen, real, fake = _nets(bias=False)
    terms = _diffusion().sid_generator_losses(gen, z, S, real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise,
                                              indices=idx, alpha=alpha)
    assert float(terms["dm_norm"][1]) == 0 and float(terms["loss"].detach()[1]) == 0
    assert torch.isfinite(terms["loss"]).all() and (terms["dm_norm"][[0, 2, 3, 4]] > 0).all()
    terms["loss"].sum().backward()
    ref_loss, _, ref_grads = _statement(gen, real, fake, z, noise, idx, alpha, skip=(1,))
    assert _rel(terms["loss"].detach(), ref_loss) <= 1e-12
    for p, g in ref_grads.items():
        assert torch.isfinite(p.grad).all() and float(g.abs().max()) > 0 and _rel(p.grad, g) <= 1e-12


def test_loss_refusals():
    z, noise, idx = _operands()
    gen, real, fake = _nets()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx)
    with pytest.raises(NotImplementedError, match="distillation=False"):
        _diffusion(distillation=True).sid_generator_losses(gen, z, S, **kw)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        _diffusion().sid_generator_losses(gen, z.clone().requires_grad_(True), S, **kw)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        _diffusion().sid_generator_losses(gen, z, S, **dict(kw, noise=noise.clone().requires_grad_(True)))
    with pytest.raises(NotImplementedError, match="real_model"):
        _diffusion().sid_generator_losses(gen, z, S, fake_model=fake)
    with pytest.raises(ValueError, match="gen_sigma"):
        _diffusion().sid_generator_losses(gen, z, S, gen_sigma=0.0, **kw)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            _diffusion().sid_generator_losses(gen, z, S, alpha=bad, **kw)


def test_draw_order_is_that_of_dm_generator_losses():
    """indices, then noise, both from `generator`: the same generator state gives both losses the same x_t."""
    seen = {}

    def spy(name):
        def real(x_in, t, **kw):
            seen[name] = (x_in.clone(), t.clone())
            return torch.zeros_like(x_in)
        return real
    z = torch.randn(64, *SHAPE, generator=torch.Generator().manual_seed(1), dtype=D64)
    gen, _, fake = _nets()
    state = torch.get_rng_state()
    for name in ("dm", "sid"):
        fn = getattr(_diffusion(), f"{name}_generator_losses")
        fn(gen, z, S, real_model=spy(name), real_diffusion=_diffusion(), fake_model=fake, generator=torch.Generator().manual_seed(11))
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(seen["dm"][0], seen["sid"][0]) and torch.equal(seen["dm"][1], seen["sid"][1])


# ------------------------------------------------------------------------------------------ loop and parser
def test_dmtrainloop_sid_two_clocks_save_resume(tmp_path):
    z = _latents()
    tl = _loop(tmp_path, objective="sid", sid_alpha=1.2)
    assert tl.objective == "sid" and tl.sid_alpha == 1.2
    real0 = _flat(tl.real_model.parameters()).clone()
    gens, fakes, emas = {}, {}, {}
    g_prev, f_prev = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
    for k in range(ITERS):
        took_gen, took_fake = _run(tl, k, z)
        gens[k], fakes[k] = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
        emas[k] = torch.cat([_flat(e) for e in tl.ema_params]).clone()
        on = k % EVERY == 0
        assert took_gen == on and took_fake
        assert torch.equal(gens[k], g_prev) != on, k
        assert not torch.equal(fakes[k], f_prev), k
        assert torch.equal(_flat(tl.real_model.parameters()), real0)
        assert all(p.grad is None for p in tl.real_model.parameters())
        g_prev, f_prev = gens[k], fakes[k]
        if tl.step == 4:
            tl.save()
    row = tl.dumpkvs()
    assert {"loss", "dm_norm", "fake_mse", "fake_xs_mse", "step"} <= set(row) and math.isfinite(row["loss"])
    files = set(os.listdir(tmp_path))
    assert {"model000004.pt", "opt000004.pt", "ema_0.9_000004.pt", "ema_0.5_000004.pt", "fake_model000004.pt", "fake_opt000004.pt"} <= files
    tr = _loop(tmp_path, resume=str(tmp_path / "model000004.pt"), objective="sid", sid_alpha=1.2)
    assert tr.step == 4 and torch.equal(_flat(tr.model.parameters()), gens[3]) and torch.equal(_flat(tr.fake_model.parameters()), fakes[3])
    for k in (4, 5, 6):
        _run(tr, k, z)
        assert torch.equal(_flat(tr.model.parameters()), gens[k]), k
        assert torch.equal(_flat(tr.fake_model.parameters()), fakes[k]), k
        assert torch.equal(torch.cat([_flat(e) for e in tr.ema_params]), emas[k]), k
    # the objective is what moved the generator: the dmd loop's first step is another one
    other = _loop(tmp_path / "dmd")
    _run(other, 0, z)
    assert not torch.equal(_flat(other.model.parameters()), gens[0])


def test_dmtrainloop_dmd_objective_is_todays_step(tmp_path):
    z = _latents()
    plain, named = _loop(tmp_path / "a"), _loop(tmp_path / "b", objective="dmd", sid_alpha=7.0)
    assert plain.objective == "dmd"
    for k in range(4):
        assert _run(plain, k, z) == _run(named, k, z)
        assert torch.equal(_flat(plain.model.parameters()), _flat(named.model.parameters())), k
        assert torch.equal(_flat(plain.fake_model.parameters()), _flat(named.fake_model.parameters())), k
    for bad in (dict(objective="dmd2"), dict(objective="sid", sid_alpha=float("nan"))):
        with pytest.raises(ValueError, match="objective|sid_alpha"):
            _loop(tmp_path / "c", **bad)


def test_command_line_flags_and_refusals(capsys):
    import cm_train
    import generate_large
    a = cm_train.parse_args(["--training_mode", "dm"])
    assert (a.dm_objective, a.sid_alpha, a.gen_sigma, a.dm_weighting) == ("dmd", 1.2, 0.0, "dmd")
    a = cm_train.parse_args(["--training_mode", "dm", "--dm_objective", "sid", "--sid_alpha", "1.0", "--gen_sigma", "2.5"])
    assert (a.dm_objective, a.sid_alpha, a.gen_sigma) == ("sid", 1.0, 2.5)
    a = cm_train.parse_args(["--training_mode", "dm", "--dm_objective=sid", "--dm_weighting", "dmd"])
    assert a.dm_objective == "sid" and a.sid_alpha == 1.2
    for argv, msg in ((["--dm_objective", "dmd2"], "--dm_objective"),
                      (["--dm_objective", "sid", "--dm_weighting", "none"], "--dm_weighting none"),
                      (["--sid_alpha", "nan"], "--sid_alpha"),
                      (["--sid_alpha", "inf"], "--sid_alpha"),
                      (["--gen_sigma", "-1"], "--gen_sigma"),
                      (["--gen_sigma", "inf"], "--gen_sigma")):
        with pytest.raises(SystemExit):
            cm_train.parse_args(["--training_mode", "dm"] + argv)
        assert msg in capsys.readouterr().err, argv
    for mode in ("consistency_training", "consistency_distillation", "progdist"):
        for argv in (["--dm_objective", "sid"], ["--dm_objective=dmd"], ["--sid_alpha", "1.2"], ["--gen_sigma", "2.5"]):
            with pytest.raises(SystemExit):
                cm_train.parse_args(["--training_mode", mode, "--synthetic_data", "True"] + argv)
            assert argv[0].split("=")[0] + " belongs to --training_mode dm" in capsys.readouterr().err, (mode, argv)
    base = ["--log_dir", "x", "--n_sample", "4"]
    args, _ = generate_large.parse_args(base + ["--karras_sampler", "dm", "--pretrained", "model.pt"])
    assert args.gen_sigma == 0.0
    args, _ = generate_large.parse_args(base + ["--karras_sampler", "dm", "--pretrained", "model.pt", "--gen_sigma", "2.5"])
    assert args.gen_sigma == 2.5
    for argv in (["--karras_sampler", "heun", "--gen_sigma", "2.5"], ["--gen_sigma", "2.5"], ["--cm_sampler", "onestep", "--gen_sigma", "2.5"],
                 ["--karras_sampler", "dm", "--gen_sigma", "-2"], ["--karras_sampler", "dm", "--gen_sigma", "nan"]):
        with pytest.raises(SystemExit):
            generate_large.parse_args(base + argv)
        assert "--gen_sigma" in capsys.readouterr().err, argv


# ------------------------------------------------------------------------------------------ host sanitizers
def test_sid_entry_points_under_address_and_ub_sanitizers():
    """`make asan_sid` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_sid.c, a program with its own main, against it and a no-device HIP runtime stub.  Null, misaligned,
    out-of-range and wrongly aliased arguments of dxmi_sid_grad_fwd and dxmi_sid_join must each come back as DXMI_EINVAL with the
    message of their check: no crash, no sanitizer report.  The program runs as a child process; nothing is loaded into python.  A
    host-only build: machines without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_sid"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_sid")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") == 58        # every case of the driver
