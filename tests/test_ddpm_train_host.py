"""DDPM noise-prediction training on the host: the schedule table, the torch path of DDPMSchedule.training_losses against float64,
DDPMTrainLoop's bookkeeping (warm-up, EMA, checkpoints, resume) on a tiny torch module, the refusals and train_ddpm.py's arguments.
No GPU.  u = 2^-24; a per-sample sum is held within 64 u of the magnitude of its terms, as the DSM tests hold theirs."""
import json
import os

import numpy as np
import pytest
import torch

U = 2.0 ** -24


def test_schedule_table_is_var_samplers_alpha_bar():
    from models.DxMI.ddpm_train import DDPMSchedule
    from models.DxMI.var_sampler import calc_diffusion_hyperparams
    ab = calc_diffusion_hyperparams(1000, 1e-4, 0.02)["Alpha_bar"]
    tab = DDPMSchedule().table
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (2, 1000) and tab.is_contiguous()
    assert torch.equal(tab[0], torch.sqrt(ab)) and torch.equal(tab[1], torch.sqrt(1 - ab))
    assert DDPMSchedule(T=10, beta_0=1e-3, beta_T=0.5).table.shape == (2, 10)
    with pytest.raises(ValueError):
        DDPMSchedule(T=0)


class _Linear:
    """A fixed linear "network": eps = W x_t over channels + c t; keeps its output for the gradient check."""

    def __init__(self):
        gen = torch.Generator().manual_seed(3)
        self.W = torch.randn(3, 3, generator=gen) * 0.5
        self.c = 1e-3

    def __call__(self, x, t):
        self.out = torch.einsum("oc,nchw->nohw", self.W, x) + self.c * t[:, None, None, None]
        if self.out.requires_grad:
            self.out.retain_grad()
        return self.out


def _operands():
    gen = torch.Generator().manual_seed(11)
    x0 = torch.rand(5, 3, 8, 8, generator=gen) * 2 - 1
    noise = torch.randn(5, 3, 8, 8, generator=gen)
    t = torch.tensor([0, 1, 499, 999, 999])
    return x0, noise, t


def test_torch_path_vs_fp64_and_autograd_order():
    from models.DxMI.ddpm_train import DDPMSchedule
    sch, net = DDPMSchedule(), _Linear()
    x0, noise, t = _operands()
    out = sch.training_losses(net, x0, t=t, noise=noise)
    assert out["loss"].shape == (5,) and torch.equal(out["loss"], out["mse"])
    # float64 on the same fp32 operands
    a, b = sch.table[0][t].double()[:, None, None, None], sch.table[1][t].double()[:, None, None, None]
    xt = a * x0.double() + b * noise.double()
    Mxt = (a * x0.double()).abs() + (b * noise.double()).abs()
    tt = t.double()[:, None, None, None]
    eps = torch.einsum("oc,nchw->nohw", net.W.double(), xt) + net.c * tt
    Meps = torch.einsum("oc,nchw->nohw", net.W.double().abs(), Mxt) + net.c * tt
    e = eps - noise.double()
    Me = Meps + noise.double().abs()
    ref = (e ** 2).mean(dim=(1, 2, 3))
    bound = 64 * U * 2 * (Me * (e.abs() + 16 * U * Me)).mean(dim=(1, 2, 3)) + 1e-30
    err = (out["loss"].double() - ref).abs()
    print("torch path |err| / bound:", (err / bound).tolist())
    assert (err <= bound).all()

    # d loss / d eps_pred: torch autograd's own order, (g / D) * (2 (eps - noise)), exactly
    x0g = x0.clone().requires_grad_(True)          # (the torch path differentiates whatever asks for it)
    out = sch.training_losses(net, x0g, t=t, noise=noise)
    g = torch.tensor([1.0, -0.37, 2.5, 1e-3, 7.0])
    out["loss"].backward(g)
    D = 3 * 8 * 8
    want = (g / D)[:, None, None, None] * (2 * (net.out.detach() - noise))
    assert torch.equal(net.out.grad, want)

    # draws of its own: t in [0, T), standard normal noise, from torch's generator
    torch.manual_seed(5)
    l1 = sch.training_losses(net, x0)["loss"]
    torch.manual_seed(5)
    tt = torch.randint(0, 1000, (5,))
    nn_ = torch.randn_like(x0)
    assert torch.equal(l1, sch.training_losses(net, x0, t=tt, noise=nn_)["loss"])


class _Tiny(torch.nn.Module):
    def __init__(self, seed=1):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(3, 3, generator=gen) * 0.3)
        self.b = torch.nn.Parameter(torch.randn(3, generator=gen) * 0.1)

    def forward(self, x, t):
        return torch.tanh(torch.einsum("oc,nchw->nohw", self.a, x) + self.b[None, :, None, None] + 1e-3 * t[:, None, None, None])


def _batches(n=8):
    gen = torch.Generator().manual_seed(99)
    return [torch.rand(4, 3, 8, 8, generator=gen) * 2 - 1 for _ in range(n)]


def _loop(tmp, resume="", **kw):
    from models.DxMI.ddpm_train import DDPMSchedule, DDPMTrainLoop
    args = dict(model=_Tiny(), schedule=DDPMSchedule(), data=None, batch_size=4, lr=1e-2, warmup_steps=8, grad_clip=1.0,
                ema_rate="0.9999", log_interval=2, save_interval=4, resume_checkpoint=resume, log_dir=str(tmp), total_steps=4)
    args.update(kw)
    return DDPMTrainLoop(**args)


def _flat(ps):
    return torch.cat([p.detach().reshape(-1) for p in ps]).double()


def test_loop_warmup_ema_checkpoints_resume(tmp_path):
    xs = _batches()
    tl = _loop(tmp_path, data=iter([(x, {}) for x in xs[:4]]))
    assert isinstance(tl.opt, torch.optim.Adam) and tl.opt.defaults["betas"] == (0.9, 0.999) and tl.opt.defaults["eps"] == 1e-8
    seen, step0 = [], tl.opt.step
    tl.opt.step = lambda *a, **k: (seen.append(tl.opt.param_groups[0]["lr"]), step0(*a, **k))[1]
    rate = 0.9999
    p0 = _flat(tl.params)
    masters = []
    update0 = tl._update_ema
    tl._update_ema = lambda: (update0(), masters.append(_flat(tl.params)))[0]
    torch.manual_seed(0)
    tl.run_loop()
    assert tl.step == 4
    assert seen == [1e-2 * (k / 8) for k in (1, 2, 3, 4)]
    # EMA, closed form: r^4 p0 + (1 - r) sum_k r^(4 - k) p_k with the fp32 rate and 1 - rate torch rounds them to
    r, a = float(np.float32(rate)), float(np.float32(1 - rate))
    want = r ** 4 * p0 + sum(a * r ** (4 - k) * masters[k - 1] for k in (1, 2, 3, 4))
    mag = r ** 4 * p0.abs() + sum(a * r ** (4 - k) * masters[k - 1].abs() for k in (1, 2, 3, 4))
    assert ((_flat(tl.ema_params[0]) - want).abs() <= 12 * U * mag + 1e-30).all()
    assert not torch.equal(_flat(tl.ema_params[0]), p0)
    files = sorted(os.listdir(tmp_path))
    assert files == ["ema_0.9999_000004.pt", "model000004.pt", "opt000004.pt", "progress.jsonl"]
    rows = [json.loads(line) for line in open(tmp_path / "progress.jsonl")]
    assert [r_["step"] for r_ in rows] == [2, 4] and all(np.isfinite(r_["loss"]) and r_["grad_norm"] > 0 for r_ in rows)
    assert rows == tl.logged and rows[1]["samples"] == 16 and rows[1]["lr"] == 1e-2 * (4 / 8)
    sd = torch.load(tmp_path / "model000004.pt")
    assert sorted(sd) == ["a", "b"] and torch.equal(sd["a"], tl.model.a.detach())
    assert torch.equal(torch.load(tmp_path / "ema_0.9999_000004.pt")["b"], tl.ema_params[0][1])

    # resumed: step 4, optimiser moments and EMA restored; the next step is the step the first loop takes next
    t2 = _loop(tmp_path, resume=str(tmp_path / "model000004.pt"))
    assert t2.step == 4 and t2.current_lr() == 1e-2 * (5 / 8)
    assert torch.equal(_flat(t2.params), _flat(tl.params)) and torch.equal(_flat(t2.ema_params[0]), _flat(tl.ema_params[0]))
    for p, q in zip(tl.params, t2.params):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(tl.opt.state[p][k], t2.opt.state[q][k])
        assert float(t2.opt.state[q]["step"]) == 4
    for loop in (tl, t2):
        torch.manual_seed(7)
        loop.run_step(xs[4])
    assert t2.step == 5 and torch.equal(_flat(t2.params), _flat(tl.params))
    assert torch.equal(_flat(t2.ema_params[0]), _flat(tl.ema_params[0]))


def test_checkpoints_load_into_the_bare_model(tmp_path):
    from models.DxMI.unet_small import Model
    from utils import fix_legacy_dict
    kw = dict(ch=32, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[16], dropout=0.1, in_channels=3, resolution=32)
    torch.manual_seed(1)
    tl = _loop(tmp_path, model=Model(**kw), ema_rate="0.9999,0.999")
    assert tl.ema_rate == [0.9999, 0.999]
    tl.save()
    torch.manual_seed(2)
    for name in ("model000000.pt", "ema_0.9999_000000.pt", "ema_0.999_000000.pt"):
        fresh = Model(**kw)
        sd = fix_legacy_dict(torch.load(tmp_path / name, map_location="cpu"))
        fresh.load_state_dict(sd, strict=True)
        assert list(sd) == list(tl.model.state_dict())
        for (k, v), (_, w) in zip(fresh.state_dict().items(), tl.model.state_dict().items()):
            assert torch.equal(v, w), (name, k)


def test_refusals(tmp_path):
    from models.DxMI.ddpm_train import DDPMSchedule
    from models.DxMI.unet_small import Model
    with pytest.raises(NotImplementedError, match="use_graph"):
        _loop(tmp_path, use_graph=True)
    net = Model(ch=32, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[16], dropout=0.1, in_channels=3, resolution=32)
    x0, noise, t = _operands()
    sch = DDPMSchedule()
    with pytest.raises(NotImplementedError, match="require grad"):
        sch._training_losses_hip(net, x0.clone().requires_grad_(True), t, noise)
    with pytest.raises(NotImplementedError, match="require grad"):
        sch._training_losses_hip(net, x0, t, noise.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        sch._training_losses_hip(net, x0, t[:3], noise)


def test_ops_refuse_cpu_tensors():
    from dxmi_hip import DxmiError, ops
    x0, noise, t = _operands()
    tab = torch.ones(2, 1000)
    with pytest.raises(DxmiError):
        ops.ddpm_prep(x0, noise, t, tab)
    with pytest.raises(DxmiError):
        ops.ddpm_loss_fwd(x0, noise)
    with pytest.raises(DxmiError):
        ops.ddpm_loss_bwd(torch.ones(5), x0, noise)


def test_train_ddpm_arguments_and_no_data_refusal():
    import train_ddpm
    a = train_ddpm.parse_args(["--config", "builtin:cifar10_T10", "--run", "t0", "--synthetic_data"])
    assert (a.batch_size, a.lr, a.warmup_steps, a.ema_rate, a.grad_clip) == (128, 2e-4, 5000, "0.9999", 1.0)
    assert a.synthetic_data and not a.no_graph and a.resume == "" and a.max_iters is None and a.data_resident == "auto"
    a = train_ddpm.parse_args(["--config", "builtin:cifar10_T10", "--data_npz", "x.npz", "--data_resident", "host", "--batch_size", "32",
                               "--lr", "1e-4", "--warmup_steps", "10", "--ema_rate", "0.999,0.9999", "--grad_clip", "0.5",
                               "--total_steps", "100", "--save_interval", "50", "--log_interval", "5", "--max_iters", "2", "--no_graph",
                               "--resume", "results/model000010.pt", "--batch_invariant"])
    assert (a.data_npz, a.data_resident, a.batch_size, a.lr, a.max_iters) == ("x.npz", "host", 32, 1e-4, 2)
    assert a.no_graph and a.batch_invariant and a.resume.endswith("model000010.pt") and a.total_steps == 100
    from train_cifar10 import load_config
    assert train_ddpm.log_dir_of(a, load_config("builtin:cifar10_T10", "builtin")) == "results/cifar10/cifar10_T10_ddpm/run"
    with pytest.raises(SystemExit):
        train_ddpm.parse_args(["--config", "builtin:cifar10_T10", "--synthetic_data", "--data_npz", "x.npz"])
    with pytest.raises(NotImplementedError, match="image folders are not read by this package"):
        train_ddpm.main(["--config", "builtin:cifar10_T10", "--run", "t0"])
