"""Progressive distillation on the GPU: the kernels of csrc/pd_train.hip against float64 on the same fp32 operands, run-to-run
bits, the index guard, malformed arguments, progdist_losses on the shrunken U-Nets against the reference (tests/golden/pd_train.npz),
its torch path with analytic callables, the lpips norm against the fp64 restatement of tests/lpips_ref.py, CMTrainLoop in progdist
mode across two phase changes (teacher copy, packs, optimiser, EMA, counters, save / resume), the progdist sampler (golden
trajectories, hipGraph replay, NFE) and the two command-line programs.

Bounds: elementwise kernel results within 16 u M of float64 (u = 2^-24, M = the magnitude of the operands that meet in the result;
for target_x = x_t - t (x_t3 - x_t) / (t3 - t), whose x_t3 = x_t2 + d2 (t3 - t2) is formed in registers, M = |x_t| + t (M3 + |x_t|) /
|t3 - t| with M3 = |x_t2| + |d2|-magnitude |t3 - t2|); per-sample sums within 64 u of their magnitude; parameter gradients cosine >=
0.995 and norm within 5 % (test_hip_cm_train.py).  Per-sample loss of the shrunken nets against the reference: PD_LOSS_REL_BOUND,
twice the worst value measured on an MI355X (PD_LOSS_REL_MEASURED = 1.834e-3: unet, l2; unet l1 9.726e-4, unet_plain l1 4.676e-4,
l2 8.328e-4; printed by the test); it may not exceed 0.18 = 3 network operands x 2 x 1.5e-2 (the bound the shrunken
net's forward is held to) / 0.5 (the fixture's separation ratio).  The lpips norm: the bounds of test_hip_lpips.py (the device value
against the bf16 storage model within PD_LPIPS_STORAGE_REL, twice the 5.584e-4 measured; against exact fp64 within twice the storage
model's own gap; d F cosine >= 0.995 and norm within 5 %).
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ew_shapes import n_by_shape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
NORMS = ("l1", "l2")
PD_LOSS_REL_MEASURED = 1.834e-3     # worst per-sample relative error measured on an MI355X (unet, l2)
PD_LOSS_REL_BOUND = 2 * PD_LOSS_REL_MEASURED
assert PD_LOSS_REL_BOUND <= 0.18
PD_LPIPS_STORAGE_REL = 1.12e-3      # device value against the bf16 storage model: twice the 5.584e-4 measured on an MI355X
SMIN = float(np.float32(0.002))      # sigma_min as the fp32 scalar the kernels subtract
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffusion-by-maxentirl_amd")


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


@pytest.fixture(scope="module")
def g(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "pd_train.npz"), allow_pickle=False))


def build(over=None, salt="", out_scale=1.0, **kw2):
    from test_hip_cm_train import build as b
    return b(over, salt, out_scale, **kw2)


def scal64(s, distill, sd=0.5):
    s = s.double()
    if distill:
        c_skip = sd ** 2 / ((s - SMIN) ** 2 + sd ** 2)
        c_out = (s - SMIN) * sd / (s ** 2 + sd ** 2) ** 0.5
    else:
        c_skip = sd ** 2 / (s ** 2 + sd ** 2)
        c_out = s * sd / (s ** 2 + sd ** 2) ** 0.5
    e = lambda v: v[:, None, None, None]
    return e(c_skip), e(c_out), e(1 / (s ** 2 + sd ** 2) ** 0.5)


def operands(N, shape, seed, S):
    from models.cm.karras_diffusion import pd_levels
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(N, *shape, generator=gen) * 2 - 1
    noise = torch.randn(N, *shape, generator=gen)
    F1, F2, Fs = (torch.randn(N, *shape, generator=gen) for _ in range(3))
    idx = torch.randint(0, S, (N,), generator=gen)
    idx[0] = S - 1                       # t3 = sigma_min
    if N > 1:
        idx[1] = 0
    tab = pd_levels(S, 0.002, 80.0, 7.0).table
    return x0, noise, F1, F2, Fs, idx, tab


def lv(tab, idx, S):
    return tab[idx], tab[S + 1 + idx], tab[idx + 1]


def close(got, ref, M, k=16, floor=1e-30):
    return ((got.cpu().double() - ref).abs() <= k * U * M + floor).all()


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("S", [1, 18])
@pytest.mark.parametrize("N,shape", n_by_shape([(3, 16, 16), (3, 64, 64), (3, 12, 11)]))
@pytest.mark.parametrize("distill", [False, True])
def test_solver_vs_fp64(ops, shape, N, distill, S):
    x0, noise, F1, F2, _, idx, tab = operands(N, shape, 11 + N + shape[1] + S, S)
    d = lambda t: t.to(DEV).contiguous()
    t, t2, t3 = lv(tab, idx, S)
    e = lambda v: v.double()[:, None, None, None]
    # prep: dxmi_cd_prep on the coarse ladder (the first S + 1 entries) gives x_t at t = tab[index]
    x_t, x_in, tm, _ = ops.cd_prep(d(x0), d(noise), d(idx), d(tab)[:S + 1], 0.5, 0.5)
    _, _, c_in = scal64(t, False)
    assert close(x_t, x0.double() + noise.double() * e(t), x0.double().abs() + (noise.double() * e(t)).abs())
    assert close(x_in, c_in * x_t.cpu().double(), c_in * x_t.cpu().double().abs(), k=8)
    assert ((tm.cpu().double() - 250 * torch.log(t.double())).abs() <= 16 * U * 250 * torch.log(t.double()).abs() + 1e-4).all()

    xt = x_t.cpu().double()
    kw = dict(sigma_data=0.5, sigma_min=0.002, distillation=distill, next_sigma_data=0.25)
    # MID with the solver diffusion's scalings; the next input under next_sigma_data
    c_skip, c_out, _ = scal64(t, distill)
    _, _, c_in2 = scal64(t2, False, sd=0.25)
    x_t2, nx, nt = ops.pd_solver(ops.PD_MID, x_t, d(F1), d(idx), d(tab), **kw)
    den = c_out * F1.double() + c_skip * xt
    Md = (xt.abs() + (c_out * F1.double()).abs() + (c_skip * xt).abs()) / e(t)
    dt = e(t2) - e(t)
    assert close(x_t2, xt + (xt - den) / e(t) * dt, xt.abs() + Md * dt.abs())
    assert close(nx, c_in2 * x_t2.cpu().double(), c_in2 * x_t2.cpu().double().abs(), k=8)
    assert ((nt.cpu().double() - 250 * torch.log(t2.double())).abs() <= 16 * U * 250 * torch.log(t2.double()).abs() + 1e-4).all()
    # END on the fp32 x_t2 the kernel wrote
    c_skip2, c_out2, _ = scal64(t2, distill)
    s64 = x_t2.cpu().double()
    target = ops.pd_solver(ops.PD_END, x_t, d(F2), d(idx), d(tab), x_t2=x_t2, **kw)
    den2 = c_out2 * F2.double() + c_skip2 * s64
    d2 = (s64 - den2) / e(t2)
    M2 = (s64.abs() + (c_out2 * F2.double()).abs() + (c_skip2 * s64).abs()) / e(t2)
    dt2, dt3 = e(t3) - e(t2), e(t3) - e(t)
    x_t3 = s64 + d2 * dt2
    M3 = s64.abs() + M2 * dt2.abs()
    ref = xt - e(t) * (x_t3 - xt) / dt3
    M = xt.abs() + e(t) * (M3 + xt.abs()) / dt3.abs()
    err = ((target.cpu().double() - ref).abs() / (U * M)).max().item()
    print(f"pd_solver END worst |err| / (u M) = {err:.2f} of 16 (shape {shape}, N {N}, distill {distill}, S {S})")
    assert close(target, ref, M)


def _loss_operands(N, shape, seed, S=18):
    x0, noise, F1, F2, Fs, idx, tab = operands(N, shape, seed, S)
    x_t = x0 + noise * tab[idx][:, None, None, None]
    target = x0 + 0.3 * F2
    return Fs, x_t, target, idx, tab


def _w64(ws, t, sd=0.5):
    snr = t.double() ** -2
    return {"karras": snr + 1 / sd ** 2, "uniform": torch.ones_like(snr), "snr": snr}[ws]


@pytest.mark.parametrize("S", [1, 18])
@pytest.mark.parametrize("N,shape", n_by_shape([(3, 16, 16), (3, 64, 64), (3, 12, 11)]))
@pytest.mark.parametrize("distill", [False, True])
def test_loss_kernels_vs_fp64(ops, shape, N, distill, S):
    from dxmi_hip import lpips_ops
    Fs, x_t, target, idx, tab = _loss_operands(N, shape, 23 + N + shape[1] + S, S)
    d = lambda t: t.to(DEV).contiguous()
    dev = [d(v) for v in (Fs, x_t, target, idx, tab)]
    t = tab[idx]
    cs_s, cs_o, _ = scal64(t, distill)
    gl = torch.randn(N, generator=torch.Generator().manual_seed(N))
    kw = dict(sigma_data=0.5, sigma_min=0.002, distillation=distill)
    worst = 0.0
    for ws in ("karras", "uniform"):
        w = _w64(ws, t)
        for norm in NORMS:
            loss = ops.pd_loss_fwd(*dev, norm, ws, **kw)
            dF = ops.pd_loss_bwd(d(gl), *dev, norm, ws, **kw)
            F64 = Fs.double().requires_grad_(True)
            ds = cs_o * F64 + cs_s * x_t.double()
            Me = (cs_o * Fs.double()).abs() + (cs_s * x_t.double()).abs() + target.double().abs()
            e = ds - target.double()
            diffs = e.abs() if norm == "l1" else e ** 2
            ref = diffs.mean((1, 2, 3)) * w
            (ref * gl.double()).sum().backward()
            ed = e.detach()
            if norm == "l1":
                bound = 64 * U * Me.mean((1, 2, 3)) * w + 1e-30
            else:
                bound = 64 * U * (Me * (ed.abs() + 16 * U * Me)).mean((1, 2, 3)) * 2 * w + 1e-30
            err = (loss.cpu().double() - ref.detach()).abs()
            assert (err <= bound).all(), (ws, norm, err / bound)
            worst = max(worst, (err / bound).max().item())
            gs = (gl.double().abs() * w / diffs[0].numel())[:, None, None, None]
            if norm == "l1":
                ok = ed.abs() > 32 * U * Me                # sign() of a difference inside its rounding error is not determined
                assert ok.float().mean() > 0.99
                assert (((dF.cpu().double() - F64.grad).abs() <= 16 * U * gs * cs_o.abs() + 1e-38) | ~ok).all(), (ws, norm)
            else:
                assert close(dF, F64.grad, gs * 2 * Me * cs_o.abs(), floor=1e-38), (ws, norm)
        # the stacked lpips images and the per-sample weights
        x01, wt = lpips_ops.pd_lpips_images(*dev, ws, **kw)
        assert x01.shape == (2 * N,) + shape
        den = (cs_o * Fs.double() + cs_s * x_t.double()).detach()
        assert close(x01[:N], (den + 1) / 2, ((cs_o * Fs.double()).abs() + (cs_s * x_t.double()).abs() + 1) / 2)
        assert close(x01[N:], (target.double() + 1) / 2, (target.double().abs() + 1) / 2)
        assert ((wt.cpu().double() - w).abs() <= 8 * U * w).all()
    print(f"pd loss_fwd worst |err| / bound = {worst:.3e} (shape {shape}, N {N}, distill {distill}, S {S})")


def test_l1_sign_of_zero_is_zero(ops):
    z = torch.zeros(2, 3, 16, 16, device=DEV)
    idx, tab = torch.tensor([0, 1], device=DEV), torch.tensor([80.0, 1.0, 0.002, 20.0, 0.5], device=DEV)
    dF = ops.pd_loss_bwd(torch.ones(2, device=DEV), z, z, z, idx, tab, "l1", "uniform")
    assert torch.equal(dF, z)
    assert torch.equal(ops.pd_loss_fwd(z, z, z, idx, tab, "l1", "uniform"), torch.zeros(2, device=DEV))


def test_kernels_reproducible_and_index_guard(ops):
    from dxmi_hip import lpips_ops
    S = 18
    Fs, x_t, target, idx, tab = [v.to(DEV) for v in _loss_operands(16, (3, 64, 64), 3, S)]
    F1 = torch.randn(16, 3, 64, 64, device=DEV)
    gl = torch.rand(16, device=DEV)
    same = lambda a, b: all(torch.equal(u, v) for u, v in zip(a, b))
    for norm in NORMS:
        a, b = (ops.pd_loss_fwd(Fs, x_t, target, idx, tab, norm, "karras") for _ in range(2))
        assert torch.equal(a, b)
        a, b = (ops.pd_loss_bwd(gl, Fs, x_t, target, idx, tab, norm, "karras") for _ in range(2))
        assert torch.equal(a, b)
    m1, m2 = (ops.pd_solver(ops.PD_MID, x_t, F1, idx, tab) for _ in range(2))
    assert same(m1, m2)
    assert torch.equal(*(ops.pd_solver(ops.PD_END, x_t, Fs, idx, tab, x_t2=m1[0]) for _ in range(2)))
    assert same(*(lpips_ops.pd_lpips_images(Fs, x_t, target, idx, tab, "karras") for _ in range(2)))
    bad = idx.clone()
    bad[3], bad[5] = S, -1                              # outside [0, S - 1]: NaN for those samples only, nothing read
    rows = [0, 1, 2, 4]
    loss = ops.pd_loss_fwd(Fs, x_t, target, bad, tab, "l2", "karras")
    assert torch.isnan(loss[[3, 5]]).all() and torch.isfinite(loss[rows]).all()
    x_t2, nx, nt = ops.pd_solver(ops.PD_MID, x_t, F1, bad, tab)
    assert torch.isnan(x_t2[[3, 5]]).all() and torch.isnan(nt[[3, 5]]).all() and torch.isfinite(x_t2[rows]).all()
    tg = ops.pd_solver(ops.PD_END, x_t, Fs, bad, tab, x_t2=m1[0])
    assert torch.isnan(tg[[3, 5]]).all() and torch.isfinite(tg[rows]).all()
    dF = ops.pd_loss_bwd(gl, Fs, x_t, target, bad, tab, "l2", "karras")
    assert torch.isnan(dF[[3, 5]]).all() and torch.isfinite(dF[rows]).all()
    torch.cuda.synchronize()


def test_wrappers_refuse_malformed_arguments(ops):
    from dxmi_hip import DxmiError, lpips_ops
    Fs, x_t, target, idx, tab = [v.to(DEV) for v in _loss_operands(4, (3, 16, 16), 9, 6)]
    g1 = torch.ones(4, device=DEV)
    bad_calls = [
        lambda: ops.pd_solver(ops.PD_MID, x_t, None, idx, tab),
        lambda: ops.pd_solver(ops.PD_END, x_t, Fs, idx, tab),
        lambda: ops.pd_solver(5, x_t, Fs, idx, tab),
        lambda: ops.pd_solver(ops.PD_MID, x_t, Fs[:2], idx, tab),
        lambda: ops.pd_solver(ops.PD_MID, x_t, Fs, idx[:3], tab),
        lambda: ops.pd_solver(ops.PD_MID, x_t, Fs, idx.int(), tab),
        lambda: ops.pd_solver(ops.PD_MID, x_t, Fs, idx, tab[:12]),            # an even number of levels is no 2 S + 1 table
        lambda: ops.pd_solver(ops.PD_MID, x_t, Fs, idx, tab[:1]),
        lambda: ops.pd_solver(ops.PD_MID, x_t, Fs, idx, tab.double()),
        lambda: ops.pd_solver(ops.PD_MID, x_t.cpu(), Fs, idx, tab),
        lambda: ops.pd_solver(ops.PD_MID, x_t.view(4, 768)[:, :766].contiguous(), Fs.view(4, 768)[:, :766].contiguous(), idx, tab),
        lambda: ops.pd_solver(ops.PD_MID, x_t.view(-1)[1:1 + 4 * 764].view(4, 764), Fs.view(4, 768)[:, :764].contiguous(), idx, tab),
        lambda: ops.pd_loss_fwd(Fs, x_t, target, idx, tab, "l2-32", "karras"),
        lambda: ops.pd_loss_fwd(Fs, x_t, target, idx, tab, "lpips", "karras"),
        lambda: ops.pd_loss_fwd(Fs, x_t[:, :, :8], target, idx, tab, "l2", "karras"),
        lambda: ops.pd_loss_bwd(g1[:3], Fs, x_t, target, idx, tab, "l2", "karras"),
        lambda: ops.pd_loss_bwd(None, Fs, x_t, target, idx, tab, "l2", "karras"),
        lambda: lpips_ops.pd_lpips_images(Fs.view(4, -1), x_t.view(4, -1), target.view(4, -1), idx, tab, "karras"),
        lambda: lpips_ops.pd_lpips_images(Fs, x_t, target[:2], idx, tab, "karras"),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"malformed call {i} was accepted")
    with pytest.raises(NotImplementedError):
        ops.pd_loss_fwd(Fs, x_t, target, idx, tab, "l2", "no-such-schedule")
    # the C entry points themselves: a status and a message, no launch
    lib = ops.load()
    p = lambda t: t.data_ptr()
    assert lib.dxmi_pd_solver(2, p(x_t), None, p(Fs), p(idx), p(tab), 6, p(target), p(Fs), p(g1), 4, 768, 0.5, 0.002, 0, 0.5, None) != 0
    assert b"unknown mode" in lib.dxmi_last_error()
    assert lib.dxmi_pd_solver(1, p(x_t), None, p(Fs), p(idx), p(tab), 6, p(target), None, None, 4, 768, 0.5, 0.002, 0, 0.5, None) != 0
    assert b"END needs" in lib.dxmi_last_error()
    assert lib.dxmi_pd_loss_fwd(p(Fs), p(x_t), p(target), p(idx), p(tab), 0, p(g1), 4, 768, 1, 0.5, 0.002, 0, 2, None) != 0
    assert b"num_scales" in lib.dxmi_last_error()
    assert lib.dxmi_pd_loss_bwd(p(g1), p(Fs), p(x_t), p(target), p(idx), p(tab), 6, p(Fs), 4, 768, 2, 0.5, 0.002, 0, 2, None) != 0
    assert b"loss norm" in lib.dxmi_last_error()
    assert lib.dxmi_pd_lpips_images(p(Fs), p(x_t), p(target), p(idx), p(tab), 6, None, p(g1), 4, 768, 0.5, 0.002, 0, 2, None) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ progdist_losses on the U-Nets
def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(a @ b / (a.norm() * b.norm() + 1e-300))


def _diffusions(norm, ws="karras"):
    from models.cm.karras_diffusion import KarrasDenoiser
    return (KarrasDenoiser(sigma_data=0.5, weight_schedule=ws, distillation=False, loss_norm=norm),
            KarrasDenoiser(sigma_data=0.5, weight_schedule=ws, distillation=False))


@pytest.mark.parametrize("tag", ["unet", "unet_plain"])
def test_progdist_losses_vs_reference(ops, g, tag):
    from test_hip_cm_train import PLAIN
    over = PLAIN if tag == "unet_plain" else None
    for norm in NORMS:                                   # the fixture's conditions, again
        sep = g[f"{tag}.{norm}.sep"]
        assert sep[0] >= 0.5 * max(sep[1], sep[2])
    assert float(g["amp.6"]) <= 1.0 and (g["indices.6"] == 0).any() and (g["indices.6"] == 5).any()
    online, teacher = build(over), build(over, "teacher:", float(g[f"{tag}.teacher_out_scale"]))
    for p in online.parameters():
        p.requires_grad_(True)
    kw = {"y": torch.from_numpy(g["y"]).to(DEV)} if tag == "unet" else {}
    x0, noise, idx = (torch.from_numpy(g[k]).to(DEV) for k in ("x_start", "noise", "indices.6"))
    loss_w = torch.from_numpy(g["loss_w"]).to(DEV)
    P = dict(online.named_parameters())
    worst, wc, wn = 0.0, ("", 1.0), ("", 0.0)
    for norm in NORMS:
        student, teacher_diffusion = _diffusions(norm)
        online.zero_grad()
        t = student.progdist_losses(online, x0, 6, model_kwargs=kw, teacher_model=teacher, teacher_diffusion=teacher_diffusion,
                                    noise=noise, indices=idx)
        assert set(t) == {"loss"} and t["loss"].requires_grad
        (t["loss"] * loss_w).mean().backward()
        ref = torch.from_numpy(g[f"{tag}.{norm}.loss"]).double()
        rel = ((t["loss"].detach().cpu().double() - ref).abs() / ref.abs()).max().item()
        print(f"{tag} {norm}: per-sample loss worst relative error {rel:.3e}")
        worst = max(worst, rel)
        for n in g[f"{tag}.grad_names"]:
            rg = torch.from_numpy(g[f"{tag}.{norm}.grad.{n}"]).float()
            got = P[str(n)].grad.cpu()
            assert got.shape == rg.shape
            if rg.norm() < 1e-6 * max(1.0, got.norm().item()):
                continue
            c, nr = _cos(got, rg), (got.norm() / rg.norm()).item()
            wc = min(wc, (f"{norm}.{n}", c), key=lambda v: v[1])
            wn = max(wn, (f"{norm}.{n}", abs(nr - 1)), key=lambda v: v[1])
            assert c >= 0.995 and abs(nr - 1) <= 0.05, (norm, n, c, nr)
        with torch.no_grad():                            # the same plain function with nothing kept
            again = student.progdist_losses(online, x0, 6, model_kwargs=kw, teacher_model=teacher, teacher_diffusion=teacher_diffusion,
                                            noise=noise, indices=idx)["loss"]
        assert torch.equal(again, t["loss"].detach()) and not again.requires_grad
    print(f"{tag}: per-sample loss worst relative error {worst:.3e} (bound {PD_LOSS_REL_BOUND}); gradient worst cosine {wc[1]:.5f} "
          f"({wc[0]}), worst norm ratio deviation {wn[1]:.4f} ({wn[0]})")
    assert worst <= PD_LOSS_REL_BOUND


def test_refusals_and_num_scales_one_on_hip_unets(ops, g):
    from test_hip_cm_train import PLAIN
    online, teacher = build(PLAIN), build(PLAIN, "teacher:")
    student, td = _diffusions("l2")
    x0, noise = (torch.from_numpy(g[k]).to(DEV) for k in ("x_start", "noise"))
    idx = torch.from_numpy(g["indices.6"]).to(DEV)
    with pytest.raises(NotImplementedError):
        student.progdist_losses(online, x0.clone().requires_grad_(True), 6, teacher_model=teacher, teacher_diffusion=td, noise=noise)
    with pytest.raises(NotImplementedError):
        student.progdist_losses(online, x0, 6, teacher_model=teacher, teacher_diffusion=td, noise=noise, model_kwargs={"z": 1})
    with pytest.raises(NotImplementedError, match="teacher"):
        student.progdist_losses(online, x0, 6, noise=noise)
    student.loss_norm = "l2-32"
    with pytest.raises(ValueError, match="Unknown loss norm"):
        student.progdist_losses(online, x0, 6, teacher_model=teacher, teacher_diffusion=td, noise=noise, indices=idx)
    student.loss_norm = "l2"
    # num_scales = 1: one interval from sigma_max to sigma_min; the index draw inside the call
    one = student.progdist_losses(online, x0, 1, teacher_model=teacher, teacher_diffusion=td, noise=noise)["loss"]
    assert one.shape == (6,) and torch.isfinite(one).all()
    # a mix of HIP and non-HIP models takes the torch path
    fn = lambda x_in, t, **kw: torch.tanh(x_in)
    c = student.progdist_losses(online, x0, 6, teacher_model=fn, teacher_diffusion=td, noise=noise, indices=idx)["loss"]
    assert c.shape == (6,) and torch.isfinite(c).all()


@pytest.mark.parametrize("S", [1, 2, 6])
@pytest.mark.parametrize("norm", NORMS)
def test_analytic_callables_on_the_device_torch_path(ops, g, norm, S):
    """Analytic callables are no HIP U-Nets: the reference's expressions run in torch on the device.  Against the CPU golden to fp32
    rounding: about 40 fp32 operations per element between the operands and the loss, device tanh / log / pow within 2 ulp of the
    host's, and the ladder's t / |t3 - t| <= 2 on the levels used: 40 x 2 x 2^-24 x 2 = 1e-5."""
    online_fn = lambda x_in, t, **kw: torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])
    teacher_fn = lambda x_in, t, **kw: 0.8 * torch.tanh(0.9 * x_in + 5e-4 * t[:, None, None, None])
    student, td = _diffusions(norm)
    x0, noise, idx = (torch.from_numpy(g[k]).to(DEV) for k in ("x_start", "noise", f"indices.{S}"))
    loss = student.progdist_losses(online_fn, x0, S, teacher_model=teacher_fn, teacher_diffusion=td, noise=noise, indices=idx)["loss"]
    np.testing.assert_allclose(loss.cpu().numpy(), g[f"analytic.{norm}.{S}.loss"], rtol=1e-5, atol=0)


def test_progdist_losses_lpips_on_hip_unets(ops, monkeypatch):
    import lpips_ref as R
    from dxmi_hip import lpips_ops as lo
    from models.cm.karras_diffusion import KarrasDenoiser, pd_levels
    from models.cm.lpips import LPIPS
    from test_hip_cm_train import PLAIN
    from test_hip_lpips import _grad_close, _value_close
    lp = LPIPS(*R.formula_weights())
    online, teacher = build(PLAIN), build(PLAIN, "teacher:", 8.0)
    for p in online.parameters():
        p.requires_grad_(True)
    student = KarrasDenoiser(distillation=False, loss_norm="lpips", lpips_loss=lp)
    td = KarrasDenoiser(distillation=False)
    gen = torch.Generator().manual_seed(11)
    N, S = 2, 6
    x0 = (torch.rand(N, 3, 16, 16, generator=gen) * 2 - 1).to(DEV)
    noise = torch.randn(N, 3, 16, 16, generator=gen).to(DEV)
    idx = torch.tensor([3, 5], device=DEV)
    rec = {}
    images, bwd = lo.pd_lpips_images, lo.cd_lpips_bwd

    def rec_images(F, x_t, target_x, *a, **k):
        rec.update(F=F, x_t=x_t, target_x=target_x)
        return images(F, x_t, target_x, *a, **k)

    def rec_bwd(*a, **k):
        rec["dF"] = bwd(*a, **k)
        return rec["dF"]

    monkeypatch.setattr(lo, "pd_lpips_images", rec_images)
    monkeypatch.setattr(lo, "cd_lpips_bwd", rec_bwd)
    call = lambda: student.progdist_losses(online, x0, S, teacher_model=teacher, teacher_diffusion=td, noise=noise, indices=idx)["loss"]
    loss = call()
    gu = torch.tensor([0.75, 1.25], device=DEV)
    (loss * gu).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in online.parameters())
    t = pd_levels(S, student.sigma_min, student.sigma_max, student.rho).table[idx.cpu()]
    F, x_t, target_x = (rec[k].detach().cpu().double() for k in ("F", "x_t", "target_x"))
    c_skip, c_out, _ = scal64(t, False)
    w = t.double() ** -2 + 1.0 / 0.5 ** 2

    def ref(**kw):       # the lpips branch of progdist_losses (reference :317-327) in fp64 from the network output and the PD target
        r = R.lpips_ref((c_out * F + c_skip * x_t + 1) / 2.0, (target_x + 1) / 2.0, resize=224, **kw)
        return r["value"] * w, (r["dx"] * (w.view(-1, 1, 1, 1) * 0.5 * c_out) if kw.get("grad") else None)
    exact, dF = ref(grad=True)
    model, _ = ref(storage=True)
    _value_close(loss, exact, model, "progdist_losses lpips", PD_LPIPS_STORAGE_REL)
    _grad_close(rec["dF"], dF * gu.cpu().double().view(N, 1, 1, 1), "progdist_losses lpips d F")
    with torch.no_grad():
        again = call()
    assert torch.equal(again, loss.detach()) and not again.requires_grad


# ------------------------------------------------------------------------------------------ CMTrainLoop
class _FixedDraws:
    def __init__(self, noises, indices, start=0):
        from models.cm.karras_diffusion import KarrasDenoiser
        self.d = KarrasDenoiser(sigma_data=0.5, weight_schedule="uniform", distillation=False, loss_norm="l2")
        self.noises, self.indices, self.i = noises, indices, start

    def __getattr__(self, name):
        return getattr(self.d, name)

    def progdist_losses(self, model, x_start, num_scales, **kw):
        n, idx = self.noises[self.i % 16].to(x_start.device), (self.indices[self.i % 16] % num_scales).to(x_start.device)
        self.i += 1
        return self.d.progdist_losses(model, x_start, num_scales, noise=n, indices=idx, **kw)


LR = 1e-4


def _data():
    gen = torch.Generator().manual_seed(99)
    x = [torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1 for _ in range(8)]
    noise = [torch.randn(2, 3, 16, 16, generator=gen) for _ in range(16)]
    idx = [torch.randint(0, 4, (2,), generator=gen) for _ in range(16)]
    return x, noise, idx


def _loop(tmp, resume="", start=0, **over):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.script_util import create_ema_and_scales_fn
    from models.cm.train_util import CMTrainLoop
    from test_hip_cm_train import PLAIN
    _, noise, idx = _data()
    online = build(PLAIN)
    online.train()
    fn = create_ema_and_scales_fn(target_ema_mode="fixed", start_ema=0.0, scale_mode="progdist", start_scales=4, end_scales=4,
                                  total_steps=100, distill_steps_per_iter=2)
    kw = dict(model=online, target_model=None, teacher_model=build(PLAIN, "teacher:"),
              teacher_diffusion=KarrasDenoiser(weight_schedule="uniform"), training_mode="progdist", ema_scale_fn=fn,
              total_training_steps=8, diffusion=_FixedDraws(noise, idx, 2 * start), data=None, batch_size=4, microbatch=2, lr=LR,
              ema_rate="0.999,0.9", log_interval=2, save_interval=100, resume_checkpoint=resume, use_fp16=True, lr_anneal_steps=2,
              log_dir=str(tmp))
    kw.update(over)
    return CMTrainLoop(**kw)


def test_cmtrainloop_progdist_on_the_device(ops, tmp_path):
    """Two phase changes (num_scales 4 -> 2 at global step 2, 2 -> 1 at 6); the reset follows the first step at the new num_scales."""
    from dxmi_hip.optim import RAdam
    x, _, _ = _data()
    tl = _loop(tmp_path)
    want = [(1, 1, 2), (2, 2, 2), (1, 3, 4), (2, 4, 4), (3, 5, 4), (4, 6, 4), (1, 7, 4), (2, 8, 4)]
    probe = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    pt = torch.tensor([1.5, -2.0], device=DEV)
    masters = {}
    for k in range(8):
        opt_before = tl.opt
        assert tl.run_step(x[k], {})
        assert (tl.step, tl.global_step, tl.lr_anneal_steps) == want[k], k
        assert tl.opt.param_groups[0]["lr"] == pytest.approx(LR * (1 - tl.step / tl.lr_anneal_steps))
        masters[k] = [p.detach().clone() for p in tl.mp_trainer.master_params]
        if k in (2, 6):
            for a, b in zip(tl.teacher_model.parameters(), tl.model.parameters()):
                assert torch.equal(a.detach(), b.detach())
            # the teacher's packed weights followed the copy: its inference forward is the student's in eval mode, bit for bit
            assert tl.teacher_model._packed_key == tl.teacher_model._param_key()
            tl.model.eval()
            with torch.no_grad():
                assert torch.equal(tl.teacher_model.forward_inference(probe, pt), tl.model.forward_inference(probe, pt))
            tl.model.train()
            assert tl.opt is not opt_before and isinstance(tl.opt, RAdam) and len(tl.opt.state) == 0
            for ema in tl.ema_params:
                assert all(torch.equal(e, m) and e.data_ptr() != m.data_ptr() for e, m in zip(ema, tl.mp_trainer.master_params))
            assert not tl.teacher_model.training
        else:
            assert tl.opt is opt_before
        if tl.global_step == 4:
            tl.save()
            lg = tl.mp_trainer.lg_loss_scale
    assert any(not torch.equal(a, b) for a, b in zip(masters[3], masters[2]))          # the student trains
    row = tl.dumpkvs()
    assert row["step"] == 8 and math.isfinite(row["loss"])
    files = set(os.listdir(tmp_path))
    assert {"ema_0.999_000004.pt", "ema_0.9_000004.pt", "model000004.pt", "opt000004.pt", "teacher_model000004.pt"} <= files
    assert not any(f.startswith("target_model") for f in files)

    # resume in the second phase (num_scales 2) from the save after step 3: the teacher of that phase comes back and steps 4, 5
    # are the uninterrupted run's, bit for bit
    tr = _loop(tmp_path, resume=str(tmp_path / "model000004.pt"), start=4)
    assert (tr.global_step, tr.step, tr.lr_anneal_steps) == (4, 2, 4)
    te = torch.load(tmp_path / "teacher_model000004.pt", map_location=DEV)
    assert all(torch.equal(v, te[k]) for k, v in tr.teacher_model.state_dict().items())
    assert all(torch.equal(a, b) for a, b in zip(tr.mp_trainer.master_params, masters[3]))
    tr.mp_trainer.lg_loss_scale = lg                # the reference does not checkpoint the loss scale
    for k in (4, 5):
        assert tr.run_step(x[k], {})
        assert (tr.step, tr.global_step, tr.lr_anneal_steps) == want[k]
        assert all(torch.equal(a.detach(), b) for a, b in zip(tr.mp_trainer.master_params, masters[k])), k
    with pytest.raises(NotImplementedError, match="use_graph"):
        _loop(tmp_path / "g", use_graph=True)


# ------------------------------------------------------------------------------------------ sampler
def _analytic(x_in, t, **kw):
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


def _rel_l2(got, want):
    want = torch.from_numpy(np.asarray(want, dtype=np.float32)).double()
    return ((got.detach().cpu().double() - want).norm() / want.norm()).item()


class _Replay:
    """A generator that hands back the recorded x_T."""

    def __init__(self, x_T):
        self.x_T, self.calls = x_T, 0

    def randn(self, *shape, device=None):
        self.calls += 1
        assert tuple(shape) == tuple(self.x_T.shape)
        return self.x_T.to(device)

    def randn_like(self, x):
        raise AssertionError("the progdist sampler draws nothing after x_T")


@pytest.mark.parametrize("steps", [1, 3])
def test_sampler_golden_trajectories(ops, g, steps):
    from models.cm.karras_diffusion import KarrasDenoiser, karras_nfe, progdist_sample
    analytic_diff = KarrasDenoiser(sigma_data=0.5, sigma_max=80.0, sigma_min=0.002, weight_schedule="uniform")
    unet = build()
    y = torch.from_numpy(g["sample.y"]).to(DEV)
    sig = torch.from_numpy(g[f"sample.{steps}.sigmas"])
    # rel-L2 bounds of test_hip_karras_sample.py: 1e-5 for the analytic model in fp32, 3e-2 for the bf16 U-Net against its fp32 run
    for m, model, kw, tol in (("analytic", _analytic, {}, 1e-5), ("unet", unet, {"y": y}, 3e-2)):
        pre = f"sample.{steps}.{m}"
        nfe, cb = [0], []

        def counted(x_in, t, **k):
            nfe[0] += 1
            return model(x_in, t, **k)
        gen = _Replay(torch.from_numpy(g[pre + ".x_T"]))
        out = progdist_sample(analytic_diff, counted, g[pre + ".x_T"].shape, steps, model_kwargs=kw, device=DEV,
                            generator=gen, callback=lambda d: cb.append(d))
        assert gen.calls == 1 and nfe[0] == steps == karras_nfe("progdist", steps) and len(cb) == steps
        assert out.min() >= -1 and out.max() <= 1
        r = _rel_l2(out, g[pre + ".sample"])
        assert r <= tol, (m, steps, r)
        for i, d in enumerate(cb):      # the reference's callback dict of this sampler has no sigma_hat
            assert set(d) == {"x", "i", "sigma", "denoised"} and d["i"] == i and float(d["sigma"]) == pytest.approx(float(sig[i]), rel=1e-6)
            for key in ("x", "denoised"):
                rk = _rel_l2(d[key], g[f"{pre}.{key}"][i])
                assert rk <= tol, (m, steps, i, key, rk)
        print(f"progdist sampler {m} steps {steps}: sample rel-L2 {r:.2e}")


def test_sampler_graph_replay_equals_eager(ops):
    from models.cm.karras_diffusion import _GRAPHS, KarrasDenoiser, karras_sample, progdist_sample
    diff = KarrasDenoiser()
    unet = build()
    y = torch.tensor([3, 871], device=DEV)
    shape = (2, 3, 16, 16)
    outs = []
    for use_graph in (False, True, True, True):          # eager; the key's first call (eager), its capture, a replay
        torch.manual_seed(1234)
        outs.append(progdist_sample(diff, unet, shape, 3, model_kwargs={"y": y}, device=DEV, use_graph=use_graph).clone())
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    (gr,) = _GRAPHS[unet].values()
    assert gr.captures == 1 and gr.replays == 1
    assert torch.isfinite(outs[0]).all() and outs[0].min() >= -1 and outs[0].max() <= 1
    # the ladder ends at sigma_min: one step is not the one-step Euler sampler over [sigma_max, 0]
    torch.manual_seed(1234)
    e = karras_sample(diff, unet, shape, 2, model_kwargs={"y": y}, device=DEV, sampler="euler")
    torch.manual_seed(1234)
    p = progdist_sample(diff, unet, shape, 1, model_kwargs={"y": y}, device=DEV)
    assert not torch.equal(e, p)
    with pytest.raises(NotImplementedError, match="distillation=False"):
        progdist_sample(KarrasDenoiser(distillation=True), unet, shape, 3, model_kwargs={"y": y}, device=DEV)


# ------------------------------------------------------------------------------------------ command line
def test_cli_cm_train_progdist_then_sample(ops, tmp_path):
    """cm_train.py --training_mode progdist on a shrunken config across one halving (num_scales 4 -> 2 at step 2; the run ends with
    the save at step 3, after the reset), then generate_large.py --karras_sampler progdist on the student it wrote."""
    from test_hip_cm_train import TINY_KW
    shrunk = dict(image_size=16, num_channels=64, num_res_blocks=1, channel_mult="1,2", attention_resolutions="8", num_head_channels=64,
                  class_cond=True, resblock_updown=True)
    args = [a for k, v in shrunk.items() for a in (f"--{k}", str(v))]
    over = dict(TINY_KW, **shrunk)
    teacher = build(over, "teacher:")
    torch.save(teacher.state_dict(), tmp_path / "teacher.pt")
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1", RANK="0", DIFFUSION_TRAINING_TEST="1")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "cm_train.py", "--training_mode", "progdist", "--synthetic_data",
                        "True", "--teacher_model_path", str(tmp_path / "teacher.pt"), "--max_iters", "3", "--batch_size", "4",
                        "--microbatch", "2", "--use_fp16", "True", "--start_scales", "4", "--distill_steps_per_iter", "2",
                        "--save_interval", "3", "--log_interval", "1", "--ema_rate", "0.999,0.9", "--lr", "1e-4",
                        "--log_dir", str(tmp_path / "run")] + args, cwd=PKG, env=env, capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = set(os.listdir(tmp_path / "run"))
    want = {"model000003.pt", "teacher_model000003.pt", "opt000003.pt", "ema_0.999_000003.pt", "ema_0.9_000003.pt", "progress.jsonl"}
    assert want <= files and not any(f.startswith("target_model") for f in files), files
    student = torch.load(tmp_path / "run" / "model000003.pt", map_location=DEV)
    saved_te = torch.load(tmp_path / "run" / "teacher_model000003.pt", map_location=DEV)
    te = teacher.state_dict()
    assert all(torch.isfinite(v).all() for v in student.values())
    # step 2 met num_scales 2: the student of that moment became the teacher, and it is no longer the teacher the run started from
    assert all(torch.equal(saved_te[k], student[k]) for k in te) and any(not torch.equal(saved_te[k], te[k]) for k in te)
    fresh = build(over, "other:")
    fresh.load_state_dict(student)

    # a log dir whose config.yaml describes the shrunken net (distillation False: the student keeps the EDM scalings)
    import dxmi_config
    os.makedirs(tmp_path / "gen")
    samp = dict(sample_shape=[3, 16, 16], n_timesteps=4, class_cond=True, num_classes=1000, trainable_beta="fix_last",
                stochastic_last=True, rho=4.0)
    dxmi_config.save(dxmi_config.Cfg({"diffusion": dict(over, distillation=False), "sampler": samp, "training": {"seed": 42}}),
                     os.path.join(tmp_path / "gen", "config.yaml"))
    gen_args = ["--log_dir", str(tmp_path / "gen"), "--karras_sampler", "progdist", "--karras_steps", "2", "--pretrained",
                str(tmp_path / "run" / "model000003.pt"), "--n_sample", "4", "--batchsize", "2"]
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "generate_large.py"] + gen_args, cwd=PKG, env=env,
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "2 NFE/image (progdist, 2 steps)" in r.stdout, r.stdout[-2000:]
    npz = np.load(tmp_path / "gen" / "samples_4.npz")["arr_0"]
    assert npz.shape == (4, 16, 16, 3) and npz.dtype == np.uint8
