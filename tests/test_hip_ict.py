"""Improved consistency training (Song and Dhariwal 2023) on the GPU: dxmi_cd_huber_fwd / _bwd (csrc/cm_train.hip) against float64
on the same fp32 operands, run-to-run bits, the index guard, malformed arguments; KarrasDenoiser.consistency_losses with
loss_norm="pseudo-huber" on the shrunken U-Nets against the l2 / uniform path of the same nets (which tests/test_hip_cm_train.py
pins to the reference); and six steps of CMTrainLoop with the ("fixed", "ict") curriculum, target EMA 0 and the discretised lognormal
level sampler, eagerly and replayed from hipGraphs.

Bounds (the convention of tests/test_hip_cm_train.py): u = 2^-24, elementwise results within 16 u M of float64 (M = the magnitude of
the operands that meet in the result), per-sample sums within 64 u of their magnitude.  With df = distiller - target, M_e the sum
of the magnitudes of the four products that meet in df, ssq = sum(df^2), c = huber_c, L = ssq / (sqrt(ssq + c^2) + c):
  ssq   within dS = sum(2 |df| 16 u M_e) + 64 u ssq
  loss  within w (dS / (2 sqrt(ssq + c^2)) + 8 u L) + 4 u w L          (dL/dssq = 1 / (2 sqrt(ssq + c^2)))
  dF    within 16 u M of (g w / sqrt(ssq32 + c^2)) df c_out(t), M = |g| w / sqrt(ssq32 + c^2) M_e |c_out(t)|, at the fp32 ssq32 the
        forward wrote.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ew_shapes import n_by_shape
from test_hip_cm_train import PLAIN, TINY_KW, _cos, build, scal64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SCHEDULES = ("ict", "karras", "uniform")
SHAPES = [(3, 16, 16), (3, 64, 64), (3, 12, 11)]


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


@pytest.fixture(scope="module")
def g(golden_dir):
    a = dict(np.load(os.path.join(golden_dir, "cm_train.npz"), allow_pickle=False))
    a.update(np.load(os.path.join(golden_dir, "cm_train_plain.npz"), allow_pickle=False))
    return a


def huber_c_of(shape):
    return 0.00054 * math.sqrt(shape[0] * shape[1] * shape[2])


def loss_operands(N, shape, seed, S, small=False):
    """The operand builder of tests/test_hip_cm_train.py (operands / _loss_operands) for an S-level ladder: idx[0] = S - 2, the
    boundary level, idx[1] = 0.  small: x_t = x_t2 = 0 and both network outputs 1e-5 randn, so that ssq is about 1e-4 c^2."""
    from models.cm.karras_diffusion import cd_levels
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(N, *shape, generator=gen) * 2 - 1
    noise = torch.randn(N, *shape, generator=gen)
    F1, F2, Fs, Ft = (torch.randn(N, *shape, generator=gen) for _ in range(4))
    idx = torch.randint(0, S - 1, (N,), generator=gen)
    idx[0] = S - 2
    if N > 1:
        idx[1] = 0
    tab = cd_levels(S, 0.002, 80.0, 7.0).table
    if small:
        z = torch.zeros(N, *shape)
        return 1e-5 * Fs, 1e-5 * Ft, z, z.clone(), idx, tab
    x_t = x0 + noise * tab[idx][:, None, None, None]
    x_t2 = x0 + F1 * tab[idx + 1][:, None, None, None]
    return Fs, Ft, x_t, x_t2, idx, tab


def w64(ws, t, t2, sd=0.5):
    t, t2 = t.double(), t2.double()
    return {"ict": 1 / (t - t2), "karras": t ** -2 + 1 / sd ** 2, "uniform": torch.ones_like(t)}[ws]


def check_huber_kernels(ops, cpu, ws, distill, c, gl):
    """One forward and one backward launch against float64 -> the worst |err| / bound of (ssq, loss, dF) and the worst relative
    error of the loss."""
    Fs, Ft, x_t, x_t2, idx, tab = cpu
    dev = [v.to(DEV).contiguous() for v in cpu]
    kw = dict(sigma_data=0.5, sigma_min=0.002, distillation=distill)
    loss, ssq = ops.cd_huber_fwd(*dev, c, ws, **kw)
    dF = ops.cd_huber_bwd(gl.to(DEV), ssq, *dev, c, ws, **kw)
    t, t2 = tab[idx], tab[idx + 1]
    cs_s, cs_o, _ = scal64(t, distill)
    ct_s, ct_o, _ = scal64(t2, distill)
    w = w64(ws, t, t2)
    df = (cs_o * Fs.double() + cs_s * x_t.double()) - (ct_o * Ft.double() + ct_s * x_t2.double())
    Me = (cs_o * Fs.double()).abs() + (cs_s * x_t.double()).abs() + (ct_o * Ft.double()).abs() + (ct_s * x_t2.double()).abs()
    s = (df ** 2).sum((1, 2, 3))
    root = torch.sqrt(s + c ** 2)
    L = s / (root + c)
    dS = (2 * df.abs() * 16 * U * Me).sum((1, 2, 3)) + 64 * U * s
    s_err = (ssq.cpu().double() - s).abs()
    bound = w * (dS / (2 * root) + 8 * U * L) + 4 * U * w * L
    l_err = (loss.cpu().double() - w * L).abs()
    # the gradient at the fp32 ssq the forward wrote
    gs = (gl.double() * w / torch.sqrt(ssq.cpu().double() + c ** 2))[:, None, None, None]
    ref_dF = gs * df * cs_o
    M = gs.abs() * Me * cs_o.abs()
    d_err = (dF.cpu().double() - ref_dF).abs()
    tiny = 1e-300
    worst = (float((s_err / (dS + tiny)).max()), float((l_err / (bound + tiny)).max()), float((d_err / (16 * U * M + 1e-38)).max()))
    rel = float((l_err / (w * L)).max())
    print(f"  huber {ws} distill {distill} S {tab.numel()} c {c:.4g}: |err| / bound ssq {worst[0]:.3e} loss {worst[1]:.3e} dF {worst[2]:.3e}; "
          f"loss worst relative error {rel:.3e}, ssq / c^2 in [{float((s / c ** 2).min()):.3e}, {float((s / c ** 2).max()):.3e}]")
    assert (s_err <= dS + tiny).all(), (ws, s_err / dS)
    assert (l_err <= bound + tiny).all(), (ws, l_err / bound)
    assert (d_err <= 16 * U * M + 1e-38).all(), (ws, float((d_err / (16 * U * M + 1e-38)).max()))
    return worst, rel


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("N,shape", n_by_shape(SHAPES))
@pytest.mark.parametrize("distill", [False, True])
def test_huber_kernels_vs_fp64(ops, shape, N, distill):
    gl = torch.randn(N, generator=torch.Generator().manual_seed(N))
    for S in (18, 1281):
        cpu = loss_operands(N, shape, 23 + N + shape[1] + S, S)
        for ws in SCHEDULES:
            check_huber_kernels(ops, cpu, ws, distill, huber_c_of(shape), gl)
    check_huber_kernels(ops, loss_operands(N, shape, 5, 18), "ict", distill, 37.5, gl)       # a given constant, ssq of its size


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("distill", [False, True])
def test_huber_small_difference_keeps_its_digits(ops, shape, distill):
    """x_t = x_t2 = 0 and f_online, f_target = 1e-5 randn: ssq is about 1e-4 c^2 and less, where a converged model lives.  There the
    loss bound is about 6.5e-6 relative.  w ssq / (sqrt(ssq + c^2) + c), the form the kernel must use, sits at about 2e-7; the
    mathematically equal sqrt(ssq + c^2) - c loses the digits of ssq below c^2 and is off by about 3e-4 in fp32 (both measured on
    the CPU), so this case fails a kernel that subtracts."""
    c = huber_c_of(shape)
    gl = torch.randn(7, generator=torch.Generator().manual_seed(3))
    for S in (18, 1281):
        cpu = loss_operands(7, shape, 41 + shape[1] + S, S, small=True)
        for ws in SCHEDULES:
            check_huber_kernels(ops, cpu, ws, distill, c, gl)
    # the premise, in fp32 on the host: the subtracting form misses this bound by far
    Fs, Ft, _, _, idx, tab = loss_operands(7, shape, 41 + shape[1] + 18, 18, small=True)
    _, cs_o, _ = scal64(tab[idx], distill)
    _, ct_o, _ = scal64(tab[idx + 1], distill)
    s = ((cs_o * Fs.double() - ct_o * Ft.double()) ** 2).sum((1, 2, 3))
    L = s / (torch.sqrt(s + c ** 2) + c)
    sub = (torch.sqrt(s.float() + np.float32(c) ** 2) - np.float32(c)).double()
    assert float(((sub - L).abs() / L).max()) > 1e-5


def test_huber_reproducible_and_index_guard(ops):
    cpu = loss_operands(16, (3, 64, 64), 3, 18)
    Fs, Ft, x_t, x_t2, idx, tab = dev = [v.to(DEV) for v in cpu]
    gl = torch.rand(16, device=DEV)
    c = huber_c_of((3, 64, 64))
    for ws in SCHEDULES:
        a, b = (ops.cd_huber_fwd(*dev, c, ws, distillation=True) for _ in range(2))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        p, q = (ops.cd_huber_bwd(gl, a[1], *dev, c, ws, distillation=True) for _ in range(2))
        assert torch.equal(p, q)
    bad = idx.clone()
    bad[3], bad[5] = tab.numel() - 1, -1                    # t2 / t outside the table: NaN for those samples only, nothing read
    loss, ssq = ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, bad, tab, c, "ict")
    assert torch.isnan(loss[[3, 5]]).all() and torch.isfinite(loss[[0, 1, 2, 4]]).all()
    dF = ops.cd_huber_bwd(gl, ssq, Fs, Ft, x_t, x_t2, bad, tab, c, "ict")
    assert torch.isnan(dF[[3, 5]]).all() and torch.isfinite(dF[[0, 1, 2, 4]]).all()
    # the sum is the l2 kernel's, in its order: ssq / CHW is what dxmi_cd_loss_fwd writes for l2 / uniform, to the rounding of the division
    l2 = ops.cd_loss_fwd(*dev, "l2", "uniform", distillation=True)
    _, ssq = ops.cd_huber_fwd(*dev, c, "uniform", distillation=True)
    assert np.array_equal(ssq.cpu().numpy() / np.float32(3 * 64 * 64), l2.cpu().numpy())       # numpy: a true fp32 division, as the kernel's


def test_huber_refuses_malformed_arguments(ops):
    from dxmi_hip import DxmiError
    Fs, Ft, x_t, x_t2, idx, tab = [v.to(DEV) for v in loss_operands(4, (3, 16, 16), 9, 18)]
    g1 = torch.ones(4, device=DEV)
    s1 = torch.ones(4, device=DEV)
    bad_calls = [
        lambda: ops.cd_huber_fwd(Fs, Ft[:2], x_t, x_t2, idx, tab, 0.1, "ict"),
        lambda: ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx[:3], tab, 0.1, "ict"),
        lambda: ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx.int(), tab, 0.1, "ict"),
        lambda: ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx, tab[:1], 0.1, "ict"),
        lambda: ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx, tab.double(), 0.1, "ict"),
        lambda: ops.cd_huber_fwd(Fs.cpu(), Ft, x_t, x_t2, idx, tab, 0.1, "ict"),
        lambda: ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx, tab, 0.0, "ict"),
        lambda: ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx, tab, -1.0, "ict"),
        lambda: ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx, tab, float("nan"), "ict"),
        lambda: ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx, tab, float("inf"), "ict"),
        lambda: ops.cd_huber_fwd(*(v.view(4, -1)[:, :766].contiguous() for v in (Fs, Ft, x_t, x_t2)), idx, tab, 0.1, "ict"),   # CHW % 4
        lambda: ops.cd_huber_bwd(g1[:3], s1, Fs, Ft, x_t, x_t2, idx, tab, 0.1, "ict"),
        lambda: ops.cd_huber_bwd(g1, s1[:3], Fs, Ft, x_t, x_t2, idx, tab, 0.1, "ict"),
        lambda: ops.cd_huber_bwd(None, s1, Fs, Ft, x_t, x_t2, idx, tab, 0.1, "ict"),
        lambda: ops.cd_huber_bwd(g1, None, Fs, Ft, x_t, x_t2, idx, tab, 0.1, "ict"),
        lambda: ops.cd_huber_bwd(g1, s1, Fs, Ft, x_t, x_t2, idx, tab, 0.0, "ict"),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"malformed call {i} was accepted")
    with pytest.raises(NotImplementedError):
        ops.cd_huber_fwd(Fs, Ft, x_t, x_t2, idx, tab, 0.1, "no-such-schedule")
    # "ict" is reachable through the two pseudo-Huber launches only
    for call in (lambda: ops.cd_loss_fwd(Fs, Ft, x_t, x_t2, idx, tab, "l2", "ict"),
                 lambda: ops.cd_loss_bwd(g1, Fs, Ft, x_t, x_t2, idx, tab, "l2", "ict"),
                 lambda: ops.edm_dsm_loss_fwd(Fs, x_t, x_t2, g1, "ict")):
        with pytest.raises(NotImplementedError):
            call()
    # the C entry points themselves: a status and a message, no launch
    lib = ops.load()
    p = lambda t: None if t is None else t.data_ptr()
    good_f = [p(Fs), p(Ft), p(x_t), p(x_t2), p(idx), p(tab), 18, p(g1), p(s1), 4, 768, 0.1, 0.5, 0.002, 0, 5, None]
    dbuf = torch.empty_like(Fs)
    good_b = [p(g1), p(s1), p(Fs), p(Ft), p(x_t), p(x_t2), p(idx), p(tab), 18, p(dbuf), 4, 768, 0.1, 0.5, 0.002, 0, 5, None]
    inf, nan = float("inf"), float("nan")

    def refused(fn, good, at, value, word):
        a = list(good)
        a[at] = value
        assert fn(*a) != 0, (at, value)
        assert word in lib.dxmi_last_error(), (at, value, lib.dxmi_last_error())

    for at in (0, 1, 2, 3, 4, 5, 7, 8):
        refused(lib.dxmi_cd_huber_fwd, good_f, at, None, b"null pointer")
    for at in (0, 1, 2, 3, 4, 5, 6, 7, 9):
        refused(lib.dxmi_cd_huber_bwd, good_b, at, None, b"null pointer")
    for fn, good, (i_S, i_chw, i_c, i_ws) in ((lib.dxmi_cd_huber_fwd, good_f, (6, 10, 11, 15)), (lib.dxmi_cd_huber_bwd, good_b, (8, 11, 12, 16))):
        for c in (0.0, -0.1, inf, -inf, nan):
            refused(fn, good, i_c, c, b"huber_c")
        for chw in (766, 0, -4):
            refused(fn, good, i_chw, chw, b"CHW")
        for S in (1, 0, -3):
            refused(fn, good, i_S, S, b"num_scales")
        for ws in (6, -1, 99):
            refused(fn, good, i_ws, ws, b"weight schedule")
        refused(fn, good, i_chw - 1, 0, b"N (")
    # every other entry point keeps its range: schedule 5 is unknown to it
    assert lib.dxmi_cd_loss_fwd(p(Fs), p(Ft), p(x_t), p(x_t2), p(idx), p(tab), 18, p(g1), 4, 3, 16, 16, 1, 0.5, 0.002, 0, 5, None) != 0
    assert b"weight schedule" in lib.dxmi_last_error()
    assert lib.dxmi_cd_loss_bwd(p(g1), p(Fs), p(Ft), p(x_t), p(x_t2), p(idx), p(tab), 18, p(dbuf), 4, 3, 16, 16, 1, 0.5, 0.002, 0, 5,
                                None) != 0
    assert b"weight schedule" in lib.dxmi_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ consistency_losses on the U-Nets
def _diffusion(norm, ws, huber_c=None):
    from models.cm.karras_diffusion import KarrasDenoiser
    return KarrasDenoiser(sigma_data=0.5, weight_schedule=ws, distillation=True, loss_norm=norm, huber_c=huber_c)


@pytest.fixture(scope="module")
def l2_runs(ops, g):
    """The l2 / uniform loss of every (net, mode), computed once: per-sample values and a closure that backpropagates an upstream."""
    from models.cm.karras_diffusion import KarrasDenoiser
    runs = {}
    for tag in ("unet", "unet_plain"):
        over = PLAIN if tag == "unet_plain" else None
        scale = float(g[f"{tag}.target_out_scale"])
        online, target, teacher = build(over), build(over, "target:", scale), build(over, "teacher:")
        for p in online.parameters():
            p.requires_grad_(True)
        kw = {"y": torch.from_numpy(g["y"]).to(DEV)} if tag == "unet" else {}
        runs[tag] = (online, target, teacher, kw, KarrasDenoiser(sigma_data=0.5, weight_schedule="uniform", distillation=False))
    return runs


@pytest.mark.parametrize("tag", ["unet", "unet_plain"])
@pytest.mark.parametrize("mode", ["cd", "ct"])
def test_consistency_losses_pseudo_huber_vs_l2_path(ops, g, l2_runs, tag, mode):
    from models.cm.karras_diffusion import cd_levels
    online, target, teacher, kw, td = l2_runs[tag]
    x0, noise, idx = (torch.from_numpy(g[k]).to(DEV) for k in ("x_start", "noise", "indices.6"))
    up = torch.from_numpy(g["loss_w"]).to(DEV).double()
    CHW = x0[0].numel()
    tab = cd_levels(6, 0.002, 80.0, 7.0).table.double()
    t, t2 = tab[idx.cpu()], tab[idx.cpu() + 1]
    P = dict(online.named_parameters())
    call = dict(model_kwargs=kw, target_model=target, teacher_model=teacher if mode == "cd" else None,
                teacher_diffusion=td if mode == "cd" else None, noise=noise, indices=idx)

    def grads(diffusion, upstream):
        online.zero_grad()
        out = diffusion.consistency_losses(online, x0, 6, **call)
        assert set(out) == {"loss"} and out["loss"].requires_grad and out["loss"].dtype == torch.float32
        (out["loss"] * upstream.to(DEV).float()).sum().backward()
        return out["loss"].detach().double().cpu(), {n: p.grad.detach().clone() for n, p in P.items()}

    l2, _ = grads(_diffusion("l2", "uniform"), up)
    S_n = CHW * l2
    for ws, c in (("ict", None), ("karras", None), ("uniform", 2.5)):
        cc = 0.00054 * math.sqrt(CHW) if c is None else c
        w = w64(ws, t, t2)
        root = torch.sqrt(S_n + cc ** 2)
        want = w * S_n / (root + cc)
        got, gh = grads(_diffusion("pseudo-huber", ws, c), up)
        rel = float(((got - want).abs() / want).max())
        print(f"{tag} {mode} {ws} c {cc:.4g}: pseudo-huber against the l2 path, worst relative error {rel:.3e} (bound {128 * U:.3e})")
        assert rel <= 128 * U
        _, gl2 = grads(_diffusion("l2", "uniform"), up.cpu() * w * CHW / (2 * root))
        seen = 0
        for n in P:
            a, b = gh[n], gl2[n]
            if b.norm() < 1e-6 * max(1.0, a.norm().item()):
                continue
            cos, nr = _cos(a, b), (a.norm() / b.norm()).item()
            assert cos >= 0.995 and abs(nr - 1) <= 0.05, (tag, mode, ws, n, cos, nr)
            seen += 1
        assert seen >= 20
    with torch.no_grad():                                   # the no-grad call is the same launch sequence without the node
        a = _diffusion("pseudo-huber", "ict").consistency_losses(online, x0, 6, **call)["loss"]
    assert not a.requires_grad and torch.equal(a.double().cpu(), grads(_diffusion("pseudo-huber", "ict"), up)[0])


def test_device_refusals_and_sampler_on_the_device(ops, g):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.resample import DiscreteLogNormalSampler
    online, target = build(PLAIN), build(PLAIN, "target:")
    x0, noise, idx = (torch.from_numpy(g[k]).to(DEV) for k in ("x_start", "noise", "indices.6"))
    for norm in ("l1", "l2", "l2-32"):
        with pytest.raises(NotImplementedError, match="pseudo-huber"):
            _diffusion(norm, "ict").consistency_losses(online, x0, 6, target_model=target, noise=noise, indices=idx)
    with pytest.raises(NotImplementedError, match="pseudo-huber"):
        KarrasDenoiser(weight_schedule="ict").training_losses(online, x0, torch.ones(6, device=DEV))
    with pytest.raises(ValueError, match="Unknown loss norm"):
        _diffusion("pseudo-huber", "karras").progdist_losses(online, x0, 4, teacher_model=target, teacher_diffusion=KarrasDenoiser())
    smp = DiscreteLogNormalSampler(0.002, 80.0, 7.0)
    for S in (3, 11, 1281):
        cdf = smp.cdf(S).table.numpy()
        dgen = torch.Generator(device=DEV).manual_seed(S)
        got = smp.sample_indices(S, 4096, DEV, dgen)
        u = torch.rand(4096, generator=torch.Generator(device=DEV).manual_seed(S), device=DEV)
        assert got.dtype == torch.int64 and got.device.type == "cuda"
        assert np.array_equal(got.cpu().numpy(), np.searchsorted(cdf, u.cpu().numpy(), side="right"))
        edge = torch.tensor([0.0, float(np.nextafter(np.float32(1), np.float32(0)))] + cdf[:64].tolist(), device=DEV)
        edge[edge >= 1] = 0.5
        assert np.array_equal(smp.indices_from_uniform(S, edge).cpu().numpy(), np.searchsorted(cdf, edge.cpu().numpy(), side="right"))
        host = smp.sample_indices(S, 64, DEV, torch.Generator().manual_seed(2))       # a host generator: drawn there, then moved
        assert host.device.type == "cuda" and torch.equal(host.cpu(), smp.sample_indices(S, 64, "cpu", torch.Generator().manual_seed(2)))
    a = _diffusion("pseudo-huber", "ict").consistency_losses(online, x0, 11, target_model=target, noise=noise, index_sampler=smp,
                                                              generator=torch.Generator(device=DEV).manual_seed(1))["loss"]
    idx11 = smp.sample_indices(11, 6, DEV, torch.Generator(device=DEV).manual_seed(1))
    b = _diffusion("pseudo-huber", "ict").consistency_losses(online, x0, 11, target_model=target, noise=noise, indices=idx11)["loss"]
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_ema_rate_zero_is_a_copy_on_the_device(ops):
    """dxmi_ema_update at rate 0: the targets become the sources bit for bit (-0 stays -0; inf and NaN in the old target do not
    leak), a chunk on the 16-byte path and a tail off it; and a set overflow flag still leaves the targets alone."""
    from models.cm.nn import update_ema
    gen = torch.Generator().manual_seed(0)
    src = [torch.randn(4096 + 37, generator=gen), torch.randn(5, generator=gen)]
    src[0][:4], src[1][0] = torch.tensor([-0.0, 0.0, 1e-40, -1e-40]), -0.0
    tgt = [torch.randn(4096 + 37, generator=gen), torch.randn(5, generator=gen)]
    tgt[0][:4], tgt[0][4100], tgt[1][0] = torch.tensor([1.0, -0.0, float("inf"), float("nan")]), float("-inf"), float("nan")
    src, tgt = [v.to(DEV) for v in src], [v.to(DEV) for v in tgt]
    before = [v.clone() for v in tgt]
    update_ema(tgt, src, rate=0.0, found_inf=torch.ones(1, device=DEV))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(tgt, before))
    update_ema(tgt, src, rate=0.0, found_inf=torch.zeros(1, device=DEV))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(tgt, src))


# ------------------------------------------------------------------------------------------ CMTrainLoop
def make_ict_loop(tmp, use_graph, dev=DEV):
    """Consistency training of the shrunken plain U-Net as --ict runs it, on a six-step curriculum: num_scales 3, 3, 5, 5, 9, 9."""
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.resample import DiscreteLogNormalSampler
    from models.cm.script_util import create_ema_and_scales_fn
    from models.cm.train_util import CMTrainLoop
    fn = create_ema_and_scales_fn(target_ema_mode="fixed", start_ema=0.0, scale_mode="ict", start_scales=2, end_scales=8, total_steps=6,
                                  distill_steps_per_iter=0)
    assert [fn(k) for k in range(6)] == [(0.0, 3), (0.0, 3), (0.0, 5), (0.0, 5), (0.0, 9), (0.0, 9)]
    online = build(PLAIN).to(dev).train()
    diffusion = KarrasDenoiser(sigma_data=0.5, weight_schedule="ict", distillation=True, loss_norm="pseudo-huber")
    return CMTrainLoop(model=online, target_model=build(PLAIN, "target:").to(dev), teacher_model=None, teacher_diffusion=None,
                       training_mode="consistency_training", ema_scale_fn=fn, total_training_steps=6, diffusion=diffusion,
                       index_sampler=DiscreteLogNormalSampler(diffusion.sigma_min, diffusion.sigma_max, diffusion.rho), data=None,
                       batch_size=4, microbatch=2, lr=1e-4, ema_rate="0.999,0.9", log_interval=2, save_interval=100, resume_checkpoint="",
                       use_fp16=True, log_dir=str(tmp), use_graph=use_graph)


def _same_packs(a, b):
    """The forward packed-weight sets of two nets of one architecture, entry by entry in build order (the keys of the entries of a
    block carry the block's id(), so they differ between the nets)."""
    from dxmi_hip.ops import PackedConvWeight
    va, vb = ([net.packed()[k] for k in net.packed() if k in net._packs.planned] for net in (a, b))
    assert len(va) == len(vb) >= 10
    packed = 0
    for u, v in zip(va, vb):
        if isinstance(u, PackedConvWeight):
            assert isinstance(v, PackedConvWeight) and torch.equal(u.buf, v.buf)
            packed += 1
        elif torch.is_tensor(u):
            assert torch.equal(u, v)
        else:
            assert u == v
    assert packed >= 10


def test_cmtrainloop_ict_six_steps(ops, tmp_path):
    from models.cm.karras_diffusion import KarrasDenoiser, karras_sample
    from test_hip_cm_graph import _batches
    batches = _batches(6, False)
    tl = make_ict_loop(tmp_path, False)
    assert not all(torch.equal(a, b) for a, b in zip(tl.target_model.parameters(), tl.model.parameters()))
    torch.manual_seed(5)
    moved = []
    for k, (x, cond) in enumerate(batches):
        before = [p.detach().clone() for p in tl.model.parameters()]
        assert tl.run_step(x, cond)
        assert tl.global_step == k + 1
        moved.append(not all(torch.equal(a, b) for a, b in zip(before, tl.model.parameters())))
        # target EMA 0: the target IS the student of this step, parameters, masters and packed weights, bit for bit
        for a, b in zip(tl.target_model.parameters(), tl.model.parameters()):
            assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
        for a, b in zip(tl.target_model_master_params, tl.mp_trainer.master_params):
            assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
        assert tl.target_model._packed_key == tl.target_model._param_key()
        _same_packs(tl.target_model, tl.model)
        if (k + 1) % 2 == 0:
            row = tl.dumpkvs()
            assert row["step"] == k + 1 and math.isfinite(row["loss"]) and row["loss"] > 0
    assert all(moved)
    tl.save()
    fresh = build(PLAIN, "other:")
    fresh.load_state_dict(torch.load(tmp_path / "target_model000006.pt", map_location=DEV))
    for a, b in zip(fresh.parameters(), tl.model.parameters()):
        assert torch.equal(a, b.detach())
    out = karras_sample(KarrasDenoiser(sigma_data=0.5, distillation=True), fresh, (2, 3, 16, 16), steps=9, device=DEV, sampler="onestep",
                        generator=None)
    assert out.shape == (2, 3, 16, 16) and torch.isfinite(out).all() and out.min() >= -1 and out.max() <= 1


def test_cmtrainloop_ict_replayed_equals_eager(ops, tmp_path):
    """The same six steps eagerly and with use_graph=True, in a fresh interpreter under its own time limit (tests/_ict_graph_worker.py):
    the warm-up step, then three captures (num_scales 3, 5 and 9: two re-captures) and two replays, on bitwise the eager state."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(here, "_ict_graph_worker.py"), str(tmp_path)],
                       capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["captures"] == 3 and line["builds"] == 3 and line["replays"] == 2, line
    assert line["global_step"] == 6 and line["key"] == [0.0, 9]
    assert line["graph_equals_eager"] and line["target_is_online"], line


def test_cli_cm_train_ict_then_onestep_sample(ops, tmp_path):
    """cm_train.py --ict True, 2 synthetic iterations on a shrunken config; the target_model file it writes is the student, loads
    into a fresh UNetModel and samples in one step."""
    from models.cm.karras_diffusion import KarrasDenoiser, karras_sample
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusion-by-maxentirl_amd")
    shrunk = dict(image_size=16, num_channels=64, num_res_blocks=1, channel_mult="1,2", attention_resolutions="8", num_head_channels=64,
                  class_cond=True, resblock_updown=True)
    args = [a for k, v in shrunk.items() for a in (f"--{k}", str(v))]
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1", RANK="0")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "cm_train.py", "--ict", "True", "--synthetic_data", "True",
                        "--max_iters", "2", "--batch_size", "4", "--microbatch", "2", "--use_fp16", "True", "--save_interval", "2",
                        "--log_interval", "1", "--ema_rate", "0.999", "--log_dir", str(tmp_path / "run")] + args, cwd=pkg, env=env,
                       capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "consistency_training" in r.stdout and "pseudo-huber" in r.stdout
    files = set(os.listdir(tmp_path / "run"))
    assert {"model000002.pt", "target_model000002.pt", "opt000002.pt", "ema_0.999_000002.pt", "progress.jsonl"} <= files, files
    rows = [json.loads(ln) for ln in open(tmp_path / "run" / "progress.jsonl")]
    assert rows and all(math.isfinite(row["loss"]) and row["loss"] > 0 for row in rows if "loss" in row)
    sd = torch.load(tmp_path / "run" / "target_model000002.pt", map_location=DEV)
    student = torch.load(tmp_path / "run" / "model000002.pt", map_location=DEV)
    assert all(torch.equal(sd[k], student[k]) for k in student)             # start_ema 0: the target is the student
    fresh = build(dict(TINY_KW, **shrunk), "other:")
    fresh.load_state_dict(sd)
    out = karras_sample(KarrasDenoiser(sigma_data=0.5, distillation=True), fresh, (2, 3, 16, 16), steps=11, device=DEV, sampler="onestep",
                        model_kwargs={"y": torch.tensor([1, 2], device=DEV)})
    assert torch.isfinite(out).all() and out.min() >= -1 and out.max() <= 1
