"""DDPM noise-prediction training on the device: the three dxmi_ddpm_* launches against float64, the loss node against torch
autograd over the same network kernels, DDPMTrainLoop replayed from hipGraphs against its eager self, two ranks on one GPU, and the
hand-over of train_ddpm.py's EMA file to the train_cifar10.py loading path.

Bounds (u = 2^-24): x_t within 16 u (|a x0| + |b noise|) of float64 on the fp32 table values; t_out exact; a per-sample loss within
64 u of the magnitude of its summed terms (the DSM tests' form: 2 mean(M (|e| + 16 u M)), M = |eps| + |noise|); d_eps within 16 u of
its magnitude |g / D| 2 (|eps| + |noise|).

Node against torch: see test_node_vs_torch_autograd."""
import json
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

from ew_shapes import SECOND_TRIP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "diffusion-by-maxentirl_amd")


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


@pytest.fixture(scope="module")
def table():
    from models.DxMI.ddpm_train import DDPMSchedule
    return DDPMSchedule().table


def operands(N, CHW, seed):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(N, CHW, generator=gen) * 2 - 1
    noise = torch.randn(N, CHW, generator=gen)
    eps = torch.randn(N, CHW, generator=gen)
    g = torch.randn(N, generator=gen)
    return x0, noise, eps, g


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("CHW", [3 * 8 * 8, 4 * 3 * 33, 3 * 20 * 20, 3 * 32 * 32, math.prod(SECOND_TRIP)])
def test_ddpm_kernels_vs_fp64(ops, table, CHW):
    N = 1 if CHW == math.prod(SECOND_TRIP) else 7
    x0, noise, eps, g = operands(N, CHW, 5 + CHW)
    t = torch.tensor([0, 1, 2, 499, 998, 999, 999])[-N:]
    d = lambda v: v.to(DEV).contiguous()
    x_t, t_out = ops.ddpm_prep(d(x0), d(noise), d(t), d(table))
    a, b = table[0][t].double()[:, None], table[1][t].double()[:, None]
    ref = a * x0.double() + b * noise.double()
    M = (a * x0.double()).abs() + (b * noise.double()).abs()
    err = (x_t.cpu().double() - ref).abs()
    print(f"CHW {CHW}: x_t worst |err| / bound = {(err / (16 * U * M + 1e-30)).max().item():.3e}")
    assert x_t.shape == x0.shape and (err <= 16 * U * M + 1e-30).all()
    assert t_out.dtype == torch.float32 and torch.equal(t_out.cpu(), t.float())

    loss = ops.ddpm_loss_fwd(d(eps), d(noise))
    e = eps.double() - noise.double()
    Me = eps.double().abs() + noise.double().abs()
    bound = 64 * U * 2 * (Me * (e.abs() + 16 * U * Me)).mean(1) + 1e-30
    err = (loss.cpu().double() - (e ** 2).mean(1)).abs()
    print(f"CHW {CHW}: loss worst |err| / bound = {(err / bound).max().item():.3e}")
    assert loss.shape == (N,) and (err <= bound).all()

    d_eps = ops.ddpm_loss_bwd(d(g), d(eps), d(noise))
    ref = (g.double()[:, None] / CHW) * (2 * e)
    Md = (g.double().abs()[:, None] / CHW) * 2 * Me
    err = (d_eps.cpu().double() - ref).abs()
    print(f"CHW {CHW}: d_eps worst |err| / bound = {(err / (16 * U * Md + 1e-38)).max().item():.3e}")
    assert (err <= 16 * U * Md + 1e-38).all()
    # the stated operation order, one fp32 rounding per operation (a true division by CHW, no reciprocal)
    want = (g / torch.full_like(g, CHW))[:, None] * (2 * (eps - noise))
    assert torch.equal(d_eps.cpu(), want)


def test_ddpm_kernels_reproducible(ops, table):
    N = 16
    x0, noise, eps, g = [v.to(DEV) for v in operands(N, 3 * 32 * 32, 3)]
    x0, noise, eps = [v.view(N, 3, 32, 32) for v in (x0, noise, eps)]
    t = torch.randint(0, 1000, (N,), generator=torch.Generator().manual_seed(1)).to(DEV)
    tab = table.to(DEV)
    a, b = ops.ddpm_prep(x0, noise, t, tab), ops.ddpm_prep(x0, noise, t, tab)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape == (N, 3, 32, 32)
    assert torch.equal(ops.ddpm_loss_fwd(eps, noise), ops.ddpm_loss_fwd(eps, noise))
    assert torch.equal(ops.ddpm_loss_bwd(g, eps, noise), ops.ddpm_loss_bwd(g, eps, noise))


def test_ddpm_prep_out_of_range_t(ops, table):
    x0, noise, _, _ = [v.to(DEV) for v in operands(3, 3 * 8 * 8, 8)]
    tab = table.to(DEV)
    x_t, t_out = ops.ddpm_prep(x0, noise, torch.tensor([-1, 1000, 5], device=DEV), tab)
    clean, _ = ops.ddpm_prep(x0, noise, torch.tensor([7, 3, 5], device=DEV), tab)
    torch.cuda.synchronize()
    assert torch.isnan(x_t[0]).all() and torch.isnan(x_t[1]).all()
    assert torch.equal(x_t[2], clean[2]) and torch.isfinite(clean).all()
    assert t_out.tolist() == [-1.0, 1000.0, 5.0]


def test_ddpm_malformed_calls(ops, table):
    from dxmi_hip import DxmiError
    x0, noise, eps, g = [v.to(DEV) for v in operands(4, 768, 2)]
    tab, t = table.to(DEV), torch.tensor([0, 1, 2, 3], device=DEV)
    bad = [lambda: ops.ddpm_prep(x0, noise[:3], t, tab), lambda: ops.ddpm_prep(x0, noise, t[:3], tab),
           lambda: ops.ddpm_prep(x0, noise, t.int(), tab), lambda: ops.ddpm_prep(x0, noise, t, tab[0]),
           lambda: ops.ddpm_prep(x0.cpu(), noise, t, tab), lambda: ops.ddpm_prep(x0.double(), noise, t, tab),
           lambda: ops.ddpm_prep(x0[:, :6].contiguous(), noise[:, :6].contiguous(), t, tab),
           lambda: ops.ddpm_loss_fwd(eps, noise.cpu()), lambda: ops.ddpm_loss_fwd(eps[:, ::2], noise[:, ::2]),
           lambda: ops.ddpm_loss_bwd(g[:3], eps, noise), lambda: ops.ddpm_loss_bwd(g.double(), eps, noise)]
    for i, call in enumerate(bad):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"malformed call {i} was accepted")
    # the C entry points themselves: a status and a message, no launch
    lib = ops.load()
    p = lambda v: v.data_ptr()
    out, tf, l4 = torch.empty_like(x0), torch.empty(4, device=DEV), torch.empty(4, device=DEV)
    prep = lambda x=p(x0), T=1000, N=4, CHW=768: lib.dxmi_ddpm_prep(x, p(noise), p(t), p(tab), T, p(out), p(tf), N, CHW, None)
    fwd = lambda e=p(eps), N=4, CHW=768: lib.dxmi_ddpm_loss_fwd(e, p(noise), p(l4), N, CHW, None)
    bwd = lambda gg=p(g), N=4, CHW=768: lib.dxmi_ddpm_loss_bwd(gg, p(eps), p(noise), p(out), N, CHW, None)
    for entry in (prep, fwd, bwd):
        assert entry(None) != 0 and b"null pointer" in lib.dxmi_last_error()
        assert entry(N=0) != 0 and b"N (0)" in lib.dxmi_last_error()
        assert entry(CHW=6) != 0 and b"CHW (6)" in lib.dxmi_last_error()
        assert entry(CHW=0) != 0
    assert prep(T=0) != 0 and b"T (0)" in lib.dxmi_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the loss node on the U-Net
NET_KW = dict(ch=64, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[8], dropout=0.1, in_channels=3, resolution=16)


def small_unet():
    from models.DxMI.unet_small import Model
    from oracle.weights import formula_tensor
    net = Model(**NET_KW)
    net.load_state_dict({k: formula_tensor(k, v.shape) for k, v in net.state_dict().items()})
    net.dropout_seed = 4321
    return net.to(DEV).train()


def test_node_vs_torch_autograd(ops):
    """The node against forward_with_grad + the torch expressions, same dropout seeds, same network launches: only the loss
    arithmetic differs, and d_eps keeps torch's operation order.  Measured on one MI355X: every parameter gradient is bitwise equal
    to the torch path's (worst per-tensor relative L2 difference 0.0), under the training loop's upstream gradient (loss.mean()) and
    under a per-sample weighting that is no power of two; the loss differs from torch's fp32 mean by at most 1.2e-7 (one ulp: the
    two sum in different orders) and lies within 0.7 % of its 64 u bound against float64.  Asserted with torch.equal."""
    from models.DxMI.ddpm_train import DDPMSchedule
    from models.DxMI.unet_small_train import forward_with_grad
    sch = DDPMSchedule()
    net = small_unet()
    gen = torch.Generator().manual_seed(17)
    x0 = (torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1).to(DEV)
    noise = torch.randn(4, 3, 16, 16, generator=gen).to(DEV)
    t = torch.tensor([3, 250, 640, 999], device=DEV)
    w = torch.tensor([0.37, 1.0, -2.3, 0.71], device=DEV)
    names = [n for n, _ in net.named_parameters()]

    def both(reduce):
        net.zero_grad(set_to_none=True)
        net._dropout_calls = 0
        node = sch.training_losses(net, x0, t=t, noise=noise)["loss"]
        reduce(node).backward()
        g_node = [p.grad.clone() for p in net.parameters()]
        seeds_node = list(net.dropout_seeds_used)
        net.zero_grad(set_to_none=True)
        net._dropout_calls = 0
        x_t, tf = ops.ddpm_prep(x0, noise, t, sch.device_table(x0.device))
        eps = forward_with_grad(net, x_t, tf)
        ref = ((eps - noise) ** 2).mean(dim=(1, 2, 3))
        reduce(ref).backward()
        g_ref = [p.grad.clone() for p in net.parameters()]
        assert seeds_node == list(net.dropout_seeds_used) and len(seeds_node) > 0
        torch.cuda.synchronize()
        assert all(torch.isfinite(a).all() and a.abs().max() > 0 for a in g_ref)
        rels = [((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item() for a, b in zip(g_node, g_ref)]
        return node.detach(), ref.detach(), eps.detach(), g_node, g_ref, rels

    node, ref, eps, g_node, g_ref, rels = both(lambda v: v.mean())
    e = eps.double() - noise.double()
    Me = eps.double().abs() + noise.double().abs()
    bound = 64 * U * 2 * (Me * (e.abs() + 16 * U * Me)).mean(dim=(1, 2, 3)) + 1e-30
    err = (node.double() - (e ** 2).mean(dim=(1, 2, 3))).abs()
    print("node loss |err| / bound:", (err / bound).tolist(), "vs torch fp32 mean:", (node - ref).abs().tolist())
    print(f"node vs torch parameter gradients, loss.mean(): worst relative L2 difference {max(rels):.3e}")
    assert (err <= bound).all()
    for n, a, b in zip(names, g_node, g_ref):
        assert torch.equal(a, b), n

    _, _, _, g_node, g_ref, rels = both(lambda v: (v * w).sum())
    k = max(range(len(rels)), key=lambda i: rels[i])
    print(f"node vs torch parameter gradients, weighted sum: worst relative L2 difference {rels[k]:.3e} ({names[k]})")
    for n, a, b in zip(names, g_node, g_ref):
        assert torch.equal(a, b), n
    with pytest.raises(NotImplementedError):
        sch.training_losses(net, x0.clone().requires_grad_(True), t=t, noise=noise)


# ------------------------------------------------------------------------------------------ the loop: replay equals eager
def run_loop(use_graph, steps, tmp, seed=0, rates="0.9999,0.99", counter=None):
    """`steps` steps of DDPMTrainLoop on the small net from fixed weights, data and seeds -> (loop, collectives per step)."""
    from models.DxMI.ddpm_train import DDPMSchedule, DDPMTrainLoop
    net = small_unet()
    gen = torch.Generator().manual_seed(seed)
    xs = [(torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1).to(DEV) for _ in range(steps)]
    loop = DDPMTrainLoop(model=net, schedule=DDPMSchedule(), data=None, batch_size=4, lr=1e-3, warmup_steps=3, grad_clip=1.0,
                         ema_rate=rates, log_interval=1, save_interval=10 ** 9, log_dir=tmp, total_steps=steps, use_graph=use_graph)
    torch.manual_seed(1000 + seed)
    per_step = []
    for x in xs:
        c0 = counter[0] if counter is not None else 0
        loop.run_step(x)
        per_step.append((counter[0] if counter is not None else 0) - c0)
        loop.dumpkvs()
    torch.cuda.synchronize()
    return loop, per_step


def test_replay_equals_eager(ops, tmp_path):
    (le, _), (lg, _) = run_loop(False, 5, str(tmp_path / "e")), run_loop(True, 5, str(tmp_path / "g"))
    assert le.step == lg.step == 5 and le.captures == 0
    assert (lg.captures, lg.replays) == (1, 3)
    assert [r["lr"] for r in lg.logged] == [1e-3 * min(1.0, k / 3) for k in (1, 2, 3, 4, 5)]
    assert all(r["loss"] > 0 and r["grad_norm"] > 0 for r in le.logged)
    assert le.logged == lg.logged, (le.logged, lg.logged)
    moved = False
    for k, (a, b) in enumerate(zip(le.params, lg.params)):
        assert torch.equal(a, b), k
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(le.opt.state[a][key], lg.opt.state[b][key]), (k, key)
        assert float(le.opt.state[a]["step"]) == float(lg.opt.state[b]["step"]) == 5
        for r in range(2):
            assert torch.equal(le.ema_params[r][k], lg.ema_params[r][k]), (k, r)
        moved = moved or not torch.equal(le.ema_params[0][k], le.ema_params[1][k])
    assert moved and le.model._dropout_calls == lg.model._dropout_calls > 0


def test_two_ranks_on_one_gpu():
    """Two fresh child processes share cuda:0 and all-reduce their (different) gradients over gloo, at a graph cut when replayed; each
    child runs under its own time limit."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "_ddpm_rank_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate() for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-3000:]
    line = json.loads([ln for ln in outs[0][0].splitlines() if ln.startswith("{")][-1])
    assert line["world"] == 2 and (line["captures"], line["replays"]) == (1, 3) and line["cuts"] == 1
    assert line["eager_collectives"] == line["graph_collectives"] and min(line["eager_collectives"]) >= 1
    assert line["params_equal"] and line["ranks_identical"] and line["losses_differ"]


def test_teacher_hand_over_to_train_cifar10(tmp_path):
    """train_ddpm.py on the builtin config (the full-size net: its first pack and one capture, hence the time limit) in a child
    process; its EMA file through train_cifar10.py's loading path, then one VARSampler call."""
    import dxmi_config
    from train_cifar10 import load_config
    from utils import fix_legacy_dict
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(PKG, "train_ddpm.py"), "--config", "builtin:cifar10_T10",
                        "--synthetic_data", "--max_iters", "2", "--batch_size", "8", "--run", "t0"], cwd=tmp_path, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logdir = tmp_path / "results" / "cifar10" / "cifar10_T10_ddpm" / "t0"
    assert sorted(os.listdir(logdir)) == ["ema_0.9999_000002.pt", "model000002.pt", "opt000002.pt", "progress.jsonl"]
    cfg = load_config("builtin:cifar10_T10", "builtin")
    net = dxmi_config.instantiate(cfg.sampler_net)
    sampler = dxmi_config.instantiate(cfg.sampler, net=net).to(DEV)
    res = net.load_state_dict(fix_legacy_dict(torch.load(logdir / "ema_0.9999_000002.pt", map_location="cpu")), strict=False)
    assert set(res.missing_keys) <= {"log_betas", "std"} and not res.unexpected_keys
    model = torch.load(logdir / "model000002.pt", map_location="cpu")
    loaded = net.state_dict()
    assert any(not torch.equal(v, loaded[k].cpu()) for k, v in model.items())      # the EMA trails the weights
    sampler.eval()
    torch.manual_seed(0)
    out = sampler.sample(2, device=DEV)["sample"]
    assert out.shape == (2, 3, 32, 32) and torch.isfinite(out).all()
