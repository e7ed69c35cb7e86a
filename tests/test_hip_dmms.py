"""The K-step distribution-matching generator on the GPU (DMD2's backward simulation): the five dxmi_dmms_* launches of
csrc/dm_train.hip against float64 on the same fp32 operands, the frozen rows of dxmi_dmms_stage, its step guard and its in-launch
noise, K = 1 against the one-step node, KarrasDenoiser.dm_generator_losses(gen_sigmas=...) at K = 3 on the shrunken HIP U-Nets
against float64 oracle nets, dm_sample at K = 3, DMTrainLoop at K = 2 with save / resume, and the two command lines.

Bounds: test_hip_dm_train.py's.  An elementwise result within 16 u M of float64 on the operands the launch read (u = 2^-24, M the
magnitude of what meets in it).  Per-sample loss of the shrunken nets against the oracle: DMMS_LOSS_REL_BOUND, twice the worst value
measured on an MI355X (DMMS_LOSS_REL_MEASURED; printed by the test), under the cap of 5.32 with every simulated
evaluation counted as one more network operand: 2 x (5 + K - 1) x 1.5e-2 / 0.5 = 0.42 at K = 3; dm_norm likewise, (2 + K - 1)
operands and no square."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ew_shapes import n_by_shape
from test_hip_dm_train import (DEV, FAKE_SCALE, GEN_SCALE, NET_Y, PKG, S_NET, U, WEIGHTINGS, _Analytic, _cos, _diffusion, _flat,
                               _latents, _loop, _net_operands, _oracle64, _Replay, _run, build, close, e, grad_ref64, ratio, scal64)

pytestmark = pytest.mark.gpu
LADDERS = {1: (80.0,), 2: (80.0, 0.5), 3: (80.0, 10.0, 2.0), 4: (80.0, 5.0, 1.0, 0.3)}
K_NET = 3
NET_STEPS = (0, 1, 2, 2)
DMMS_LOSS_REL_MEASURED = 3.603e-3   # worst per-sample relative error of loss measured on an MI355X at K = 3 (none; dmd 3.041e-3)
DMMS_NORM_REL_MEASURED = 8.528e-4   # the same of dm_norm
DMMS_LOSS_REL_BOUND, DMMS_NORM_REL_BOUND = 2 * DMMS_LOSS_REL_MEASURED, 2 * DMMS_NORM_REL_MEASURED
DMMS_LOSS_REL_CAP = 2 * (5 + K_NET - 1) * 1.5e-2 / 0.5
DMMS_NORM_REL_CAP = (2 + K_NET - 1) * 1.5e-2 / 0.5
assert DMMS_LOSS_REL_BOUND <= DMMS_LOSS_REL_CAP and DMMS_NORM_REL_BOUND <= DMMS_NORM_REL_CAP


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def d(v):
    return v.to(DEV).contiguous()


def ladder_tab(K):
    return torch.tensor(LADDERS[K], dtype=torch.float32)


def step_vectors(N, K):
    """all zero, all K - 1, and mixed: cycling through 0 .. K-1, so that (N >= K) every stage has frozen and live images."""
    mixed = torch.arange(N) % K
    return {"zero": torch.zeros(N, dtype=torch.int64), "last": torch.full((N,), K - 1, dtype=torch.int64), "mixed": mixed.flip(0).contiguous()}


def bits(v):
    return v.contiguous().view(torch.int32)


def time_close(tm, sigma):
    ref = 250 * torch.log(sigma.double())
    return ((tm.cpu().double() - ref).abs() <= 16 * U * ref.abs() + 1e-4).all()


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("N,shape", n_by_shape([(3, 16, 16), (3, 12, 11), (3, 64, 64)]))
@pytest.mark.parametrize("sd_f", [0.5, 0.25])
def test_kernels_vs_fp64(ops, shape, N, K, sd_f):
    from models.cm.karras_diffusion import cd_levels
    S = 18
    gen = torch.Generator().manual_seed(101 + N + shape[1] + K)
    z, noise, Fg = (torch.randn(N, *shape, generator=gen) for _ in range(3))
    Fs, eps = torch.randn(max(K - 1, 1), N, *shape, generator=gen), torch.randn(max(K - 1, 1), N, *shape, generator=gen)
    idx = torch.randint(0, S, (N,), generator=gen)
    up = torch.randn(N, generator=gen)
    ttab = cd_levels(S, 0.002, 80.0, 7.0).table
    t = ttab[idx]
    sig = ladder_tab(K)
    tab = d(sig)
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)
    for name, steps in step_vectors(N, K).items():
        # dmms_in
        x, x_in, tm = ops.dmms_in(d(z), tab, 0.5)
        s0 = sig[0].expand(N)
        x0 = z.double() * float(sig[0])
        ci0 = scal64(s0)[2]
        assert close(x, x0, x0.abs()) and close(x_in, ci0 * x.cpu().double(), (ci0 * x0).abs()) and time_close(tm, s0)
        note("in", ratio(x_in, ci0 * x.cpu().double(), (ci0 * x0).abs()))
        # the stages, each against float64 on the fp32 state it read; frozen rows must keep their bits
        for j in range(K - 1):
            before = [v.clone() for v in (x, x_in, tm)]
            ops.dmms_stage(d(Fs[j]), j, tab, x, x_in, tm, steps=d(steps), eps=d(eps[j]), sigma_data=0.5)
            live = steps > j
            cs, co, _ = scal64(sig[j].expand(N))
            sn = sig[j + 1].expand(N)
            xb = before[0].cpu().double()
            a, b, c = co * Fs[j].double(), cs * xb, eps[j].double() * e(sn)
            ref, M = a + b + c, a.abs() + b.abs() + c.abs()
            cin = scal64(sn)[2]
            got_x = x.cpu().double()
            if live.any():
                assert close(x[d(live)], ref[live], M[live])
                assert close(x_in[d(live)], (cin * got_x)[live], (cin * got_x).abs()[live]) and time_close(tm[d(live)], sn[live])
                note("stage", ratio(x[d(live)], ref[live], M[live]))
            fz = d(~live)
            for now, was in zip((x, x_in, tm), before):
                assert torch.equal(bits(now[fz]), bits(was[fz])), (name, j)
        x_k = x.clone()
        # dmms_prep at every image's own level
        sk = sig[steps]
        cs, co, _ = scal64(sk)
        xkd = x_k.cpu().double()
        ref_x, M_x = co * Fg.double() + cs * xkd, (co * Fg.double()).abs() + (cs * xkd).abs()
        xo, x_t, xr_in, tm2, xf_in = ops.dmms_prep(d(Fg), x_k, d(noise), d(steps), tab, d(idx), d(ttab), 0.5, 0.5, sd_f)
        assert torch.equal(x_k, x)                                     # x_k is only read
        assert close(xo, ref_x, M_x) and (xf_in is None) == (sd_f == 0.5)
        note("prep.x", ratio(xo, ref_x, M_x))
        xd = xo.cpu().double()
        nt = noise.double() * e(t)
        assert close(x_t, xd + nt, xd.abs() + nt.abs())
        xtd = x_t.cpu().double()
        ci_r = scal64(t, 0.5)[2]
        assert close(xr_in, ci_r * xtd, ci_r * xtd.abs()) and time_close(tm2, t)
        if xf_in is not None:
            ci_f = scal64(t, sd_f)[2]
            assert close(xf_in, ci_f * xtd, ci_f * xtd.abs()) and not torch.equal(xf_in, xr_in)
        # dmms_out: G_{K-1} whatever the steps
        cs_l, co_l, _ = scal64(sig[K - 1].expand(N))
        ref_o, M_o = co_l * Fg.double() + cs_l * xkd, (co_l * Fg.double()).abs() + (cs_l * xkd).abs()
        plain, clip = ops.dmms_out(d(Fg), x_k, tab, 0.5, clip=False), ops.dmms_out(d(Fg), x_k, tab, 0.5, clip=True)
        assert close(plain, ref_o, M_o) and torch.equal(clip, plain.clamp(-1, 1)) and (ref_o.abs() > 1).any()
        note("out", ratio(plain, ref_o, M_o))
        xc = x_k.clone()
        assert ops.dmms_out(d(Fg), xc, tab, 0.5, clip=True, out=xc) is xc and torch.equal(xc, clip)      # x may be x_k
        # dmms_bwd
        g = xo                                                          # any image-sized operand
        dF = ops.dmms_bwd(d(up), g, d(steps), tab, 0.5)
        gd = g.cpu().double()
        ref_dF = e(up) / gd[0].numel() * gd * co
        assert close(dF, ref_dF, ref_dF.abs(), floor=1e-38)
        note("bwd", ratio(dF, ref_dF, ref_dF.abs(), floor=1e-38))
        if K == 1:                                                      # one level: the bits of the one-step launches
            s1 = LADDERS[1][0]
            x_in1, tm1 = ops.dm_gen_in(d(z), s1, 0.5)
            assert torch.equal(x_in1, x_in) and torch.equal(tm1, tm)
            one = ops.dm_gen_prep(d(Fg), d(z), d(noise), d(idx), d(ttab), s1, 0.5, 0.5, sd_f)
            for a, b in zip(one, (xo, x_t, xr_in, tm2, xf_in)):
                assert (a is None and b is None) or torch.equal(a, b)
            assert torch.equal(ops.dm_gen_out(d(Fg), d(z), s1, 0.5, clip=True), clip)
            assert torch.equal(ops.dm_gen_bwd(d(up), g, s1, 0.5), dF)
    print(f"dmms kernels worst |err| / bound (shape {shape}, N {N}, K {K}, fake sigma_data {sd_f}): "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 12, 11), (3, 64, 64)])
def test_frozen_rows_keep_a_bit_pattern(ops, shape):
    """x, x_in and t_out of the frozen images hold a NaN bit pattern no arithmetic would give back: after every stage it is intact."""
    N, K = 7, 4
    gen = torch.Generator().manual_seed(5 + shape[1])
    steps = torch.tensor([0, 3, 1, 2, 0, 3, 1])
    tab = d(ladder_tab(K))
    x, x_in, tm = ops.dmms_in(d(torch.randn(N, *shape, generator=gen)), tab, 0.5)
    pattern = torch.tensor(0x7FC12345, dtype=torch.int32, device=DEV)
    for j in range(K - 1):
        fz = d(steps <= j)
        for v in (x, x_in, tm):
            bits(v)[fz] = pattern
        ops.dmms_stage(d(torch.randn(N, *shape, generator=gen)), j, tab, x, x_in, tm, steps=d(steps), eps=d(torch.randn(N, *shape, generator=gen)))
        for v in (x, x_in, tm):
            assert (bits(v)[fz] == pattern).all(), j
            assert torch.isfinite(v[~fz]).all(), j
    # steps None: nothing is frozen
    ops.dmms_stage(d(torch.randn(N, *shape, generator=gen)), 0, tab, x, x_in, tm, eps=d(torch.randn(N, *shape, generator=gen)))
    assert torch.isnan(x[d(steps <= K - 2)]).all() and torch.isfinite(x[d(steps > K - 2)]).all() and torch.isfinite(tm).all()


def test_step_guard_and_reproducibility(ops):
    from models.cm.karras_diffusion import cd_levels
    N, K, shape, S = 5, 3, (3, 16, 16), 18
    gen = torch.Generator().manual_seed(77)
    z, F0, F1, Fg, e0, e1, noise = (d(torch.randn(N, *shape, generator=gen)) for _ in range(7))
    up, idx, ttab = d(torch.randn(N, generator=gen)), d(torch.randint(0, S, (N,), generator=gen)), d(cd_levels(S, 0.002, 80.0, 7.0).table)
    tab = d(ladder_tab(K))

    def run(steps):
        steps = d(steps)
        x, x_in, tm = ops.dmms_in(z, tab, 0.5)
        ops.dmms_stage(F0, 0, tab, x, x_in, tm, steps=steps, eps=e0)
        ops.dmms_stage(F1, 1, tab, x, x_in, tm, steps=steps, eps=e1)
        xo, x_t, xr_in, _, xf_in = ops.dmms_prep(Fg, x, noise, steps, tab, idx, ttab, 0.5, 0.5, 0.25)     # its time is the denoisers'
        return x, x_in, tm, xo, x_t, xr_in, xf_in, ops.dmms_bwd(up, xo, steps, tab, 0.5)
    good = torch.tensor([2, 1, 2, 0, 2])
    ref = run(good)
    assert all(torch.isfinite(v).all() for v in ref)
    for bad_value in (K, -1, 1 << 40, -(1 << 40)):
        bad = good.clone()
        bad[2] = bad_value
        a, b = run(bad), run(bad)
        for va, vb, vr in zip(a, b, ref):
            assert torch.equal(bits(va), bits(vb))                          # two runs: the same bits
            assert torch.isnan(va[2]).all(), bad_value                      # NaN in that image, in every output
            keep = [0, 1, 3, 4]
            assert torch.equal(va[keep], vr[keep]), bad_value               # and in that image only


@pytest.mark.parametrize("shape", [(3, 12, 11), (3, 64, 64)])
def test_in_launch_noise_is_randn_indexed(ops, shape):
    N, K = 7, 4
    gen = torch.Generator().manual_seed(3 + shape[1])
    seed = (1 << 35) + 11
    index = d(torch.tensor([0, 5, 1 << 33, 49999, 7, 7, 123456789]))
    steps = d(torch.arange(N) % K)
    tab = d(ladder_tab(K))
    z = d(torch.randn(N, *shape, generator=gen))
    a, b = ops.dmms_in(z, tab, 0.5), ops.dmms_in(z, tab, 0.5)
    for j in range(K - 1):
        F = d(torch.randn(N, *shape, generator=gen))
        draw = 3 * j + 1
        ops.dmms_stage(F, j, tab, *a, steps=steps, sample_index=index, seed=seed, draw=draw)
        ops.dmms_stage(F, j, tab, *b, steps=steps, eps=ops.randn_indexed(index, shape, seed, draw))
        for va, vb in zip(a, b):
            assert torch.equal(va, vb), j
    from dxmi_hip._lib import DxmiError
    with pytest.raises(DxmiError, match="exactly one"):
        ops.dmms_stage(z, 0, tab, *a, sample_index=index, eps=z)
    with pytest.raises(DxmiError, match="exactly one"):
        ops.dmms_stage(z, 0, tab, *a)
    with pytest.raises(DxmiError, match="stage"):
        ops.dmms_stage(z, K - 1, tab, *a, eps=z)
    with pytest.raises(DxmiError, match="steps"):
        ops.dmms_stage(z, 0, tab, *a, eps=z, steps=steps[:3])
    with pytest.raises(DxmiError, match="gen_sigmas"):
        ops.dmms_in(z, tab.double(), 0.5)


# ------------------------------------------------------------------------------------------ K = 1 is the one-step node
@pytest.mark.parametrize("gan", [False, True])
def test_one_level_is_the_one_step_node(ops, gan):
    real, fake = build(None, "", GEN_SCALE), build(None, "fake:", FAKE_SCALE)
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, model_kwargs={"y": y}, noise=noise, indices=idx)
    if gan:
        from test_hip_gan import _head
        g = torch.Generator().manual_seed(4)
        kw.update(gan_head=_head(128, 8).to(DEV), gan_gen_weight=1e-2, gan_noise=torch.randn(z.shape, generator=g).to(DEV),
                  gan_indices=torch.randint(0, S_NET, (len(z),), generator=g).to(DEV))
    out, grads = [], []
    for how in (dict(gen_sigma=80.0), dict(gen_sigmas=[80.0])):
        net = build(None, "", GEN_SCALE)
        for p in net.parameters():
            p.requires_grad_(True)
        t = _diffusion().dm_generator_losses(net, z, S_NET, **kw, **how)
        t["loss"].sum().backward()
        out.append(t)
        grads.append({n: p.grad.clone() for n, p in net.named_parameters()})
    assert set(out[1]) == set(out[0]) | {"steps"} and torch.equal(out[1]["steps"], torch.zeros(len(z), dtype=torch.int64, device=DEV))
    for k in ("loss", "x", "dm_norm") + (("gan_loss", "gan_logit") if gan else ()):
        assert torch.equal(out[0][k].detach(), out[1][k].detach()), k
    assert grads[0].keys() == grads[1].keys() and all(torch.equal(grads[0][n], grads[1][n]) for n in grads[0])
    assert any(float(v.abs().max()) > 0 for v in grads[0].values())


# ------------------------------------------------------------------------------------------ the loss on the shrunken nets
def _sim_operands():
    gen = torch.Generator().manual_seed(13)
    return torch.randn(K_NET - 1, 4, 3, 16, 16, generator=gen), torch.tensor(NET_STEPS)


def _oracle_dmms(gen_sd, fake_sd, z, noise, sim, idx, steps, y, weighting, ladder=LADDERS[K_NET]):
    """dm_generator_losses(gen_sigmas=ladder) on float64 oracle nets (test_hip_dm_train._oracle_dm with the backward simulation in
    front: the states x_k come from the generator's own weights, detached) -> loss, s, parameter gradients, the two separations."""
    from models.cm.karras_diffusion import cd_levels
    t = cd_levels(S_NET, 0.002, 80.0, 7.0).table.double()[idx]
    sig = torch.tensor(ladder, dtype=torch.float32).double()
    N = len(z)
    with _oracle64() as edm:
        from oracle import Precision
        cfg = edm.EDMConfig(image_size=16, model_channels=64, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2))

        def den(sd, x_t, s):
            cs, co, ci = scal64(s)
            return co * edm.unet_forward(sd, cfg, ci * x_t, 250 * torch.log(s), y=y, prec=Precision("fp32")) + cs * x_t
        leaves = {k: v.double().requires_grad_(True) for k, v in gen_sd.items()}
        real = {k: v.double() for k, v in gen_sd.items()}
        fake = {k: v.double() for k, v in fake_sd.items()}
        with torch.no_grad():
            x_k = z.double() * sig[0]
            for j in range(len(ladder) - 1):
                nxt = den(real, x_k, sig[j].expand(N)) + sim[j].double() * sig[j + 1]
                x_k = torch.where(e(steps > j).bool(), nxt, x_k)
        x = den(leaves, x_k, sig[steps])
        with torch.no_grad():
            x_t = x + noise.double() * e(t)
            D_r, D_f = den(real, x_t, t), den(fake, x_t, t)
            s = (x - D_r).abs().mean(dim=[1, 2, 3])
            g = D_f - D_r
            if weighting == "dmd":
                g = g / e(s)
        loss = 0.5 * ((x - (x - g).detach()) ** 2).mean(dim=[1, 2, 3])
        loss.sum().backward()
    rms = lambda v: v.detach().pow(2).mean(dim=[1, 2, 3]).sqrt()
    sep_g = (rms(D_f - D_r) / torch.maximum(rms(D_f), rms(D_r))).min().item()
    sep_s = (s / torch.maximum(rms(x), rms(D_r))).min().item()
    value = 0.5 * (g ** 2).mean(dim=[1, 2, 3])
    return value, s, {k: v.grad for k, v in leaves.items()}, sep_g, sep_s


def test_dm_generator_losses_k3_vs_fp64_oracle(ops):
    """Per-sample relative error against the float64 oracle nets, measured on an MI355X at K = 3, N = 4, steps (0, 1, 2, 2):
    loss DMMS_LOSS_REL_MEASURED, dm_norm DMMS_NORM_REL_MEASURED; the bounds are twice those."""
    gen_net, real, fake = build(None, "", GEN_SCALE), build(None, "", GEN_SCALE), build(None, "fake:", FAKE_SCALE)
    for p in gen_net.parameters():
        p.requires_grad_(True)
    z, noise, idx, y = _net_operands()
    sim, steps = _sim_operands()
    gen_sd = {k: v.detach().cpu() for k, v in gen_net.state_dict().items()}
    fake_sd = {k: v.detach().cpu() for k, v in fake.state_dict().items()}
    dd = _diffusion()
    P = dict(gen_net.named_parameters())
    worst, worst_s, wc, wn = 0.0, 0.0, ("", 1.0), ("", 0.0)
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, model_kwargs={"y": y.to(DEV)}, noise=noise.to(DEV),
              indices=idx.to(DEV), gen_sigmas=LADDERS[K_NET], steps=steps.to(DEV), sim_noise=sim.to(DEV))
    for weighting in WEIGHTINGS:
        ref_loss, ref_s, ref_grads, sep_g, sep_s = _oracle_dmms(gen_sd, fake_sd, z, noise, sim, idx, steps, y, weighting)
        print(f"{weighting}: rms(D_f - D_r) / max(rms D_f, rms D_r) >= {sep_g:.3f}, mean|x - D_r| / max(rms x, rms D_r) >= {sep_s:.3f}")
        assert sep_g >= 0.5 and sep_s >= 0.5
        gen_net.zero_grad()
        t = dd.dm_generator_losses(gen_net, z.to(DEV), S_NET, weighting=weighting, **kw)
        assert set(t) == {"loss", "x", "dm_norm", "steps"} and t["loss"].requires_grad and not t["x"].requires_grad
        assert torch.equal(t["steps"].cpu(), steps)
        t["loss"].sum().backward()
        rel = ((t["loss"].detach().cpu().double() - ref_loss).abs() / ref_loss.abs()).max().item()
        rel_s = ((t["dm_norm"].cpu().double() - ref_s).abs() / ref_s).max().item()
        print(f"{weighting}: K = {K_NET} per-sample loss worst relative error {rel:.3e}, dm_norm {rel_s:.3e}")
        worst, worst_s = max(worst, rel), max(worst_s, rel_s)
        for n, rg in ref_grads.items():
            got = P[n].grad.cpu()
            if rg.norm() < 1e-6 * max(1.0, got.norm().item()):
                continue
            c, nr = _cos(got, rg), (got.double().norm() / rg.norm()).item()
            wc = min(wc, (f"{weighting}.{n}", c), key=lambda v: v[1])
            wn = max(wn, (f"{weighting}.{n}", abs(nr - 1)), key=lambda v: v[1])
        assert all(p.grad is None for net in (real, fake) for p in net.parameters())
        with torch.no_grad():
            again = dd.dm_generator_losses(gen_net, z.to(DEV), S_NET, weighting=weighting, **kw)
        assert not again["loss"].requires_grad and torch.equal(again["x"], t["x"]) and torch.equal(again["loss"], t["loss"].detach())
    print(f"dm_generator_losses K = {K_NET}: per-sample loss worst relative error {worst:.3e} (bound {DMMS_LOSS_REL_BOUND}, cap "
          f"{DMMS_LOSS_REL_CAP}); dm_norm {worst_s:.3e} (bound {DMMS_NORM_REL_BOUND}, cap {DMMS_NORM_REL_CAP}); gradient worst cosine "
          f"{wc[1]:.5f} ({wc[0]}), worst norm ratio deviation {wn[1]:.4f} ({wn[0]})")
    assert DMMS_LOSS_REL_BOUND <= DMMS_LOSS_REL_CAP and DMMS_NORM_REL_BOUND <= DMMS_NORM_REL_CAP
    assert wc[1] >= 0.995 and wn[1] <= 0.05
    assert worst <= DMMS_LOSS_REL_BOUND and worst_s <= DMMS_NORM_REL_BOUND


@pytest.mark.parametrize("sd_f", [0.5, 0.25])
def test_device_node_vs_torch_fallback_on_the_same_nets(ops, sd_f):
    """Wrapped in plain callables the same HIP nets take the torch fallback.  The node's launch chain is run here by hand too, which
    exposes its operands: both paths are held to the kernel bounds against float64 on those operands."""
    from models.cm.karras_diffusion import cd_levels
    gen_net, real, fake = build(None, "", GEN_SCALE), build(None, "", GEN_SCALE), build(None, "fake:", FAKE_SCALE)
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    sim, steps = (v.to(DEV) for v in _sim_operands())
    dd, fd = _diffusion(), _diffusion(sigma_data=sd_f)
    ttab = cd_levels(S_NET, 0.002, 80.0, 7.0).device_table(torch.device(DEV))
    tab = d(ladder_tab(K_NET))
    wrap = lambda net: (lambda x_in, t, **kw: net(x_in, t, **kw))
    for weighting in WEIGHTINGS:
        kw = dict(real_diffusion=_diffusion(), fake_diffusion=fd, model_kwargs={"y": y}, noise=noise, indices=idx, weighting=weighting,
                  gen_sigmas=LADDERS[K_NET], steps=steps, sim_noise=sim)
        with torch.no_grad():
            node = dd.dm_generator_losses(gen_net, z, S_NET, real_model=real, fake_model=fake, **kw)
            fb = dd.dm_generator_losses(wrap(gen_net), z, S_NET, real_model=wrap(real), fake_model=wrap(fake), **kw)
            x_k, x_in, tg = ops.dmms_in(z, tab, 0.5)
            for j in range(K_NET - 1):
                ops.dmms_stage(gen_net.forward_inference(x_in, tg, y), j, tab, x_k, x_in, tg, steps=steps, eps=sim[j])
            x, x_t, xr, tm, xf = ops.dmms_prep(gen_net.forward_inference(x_in, tg, y), x_k, noise, steps, tab, idx, ttab, 0.5, 0.5, sd_f)
            F_r, F_f = real.forward_inference(xr, tm, y), fake.forward_inference(xr if xf is None else xf, tm, y)
            g, loss, s = ops.dm_grad_fwd(F_r, F_f, x, x_t, idx, ttab, weighting, fake=dict(sigma_data=sd_f, sigma_min=0.002, distillation=False))
        assert torch.equal(node["loss"], loss) and torch.equal(node["dm_norm"], s) and torch.equal(node["x"], x)
        assert torch.equal(fb["steps"], steps) and torch.equal(node["steps"], steps)
        _, rl, rs, _, b_l, b_s = grad_ref64(F_r, F_f, x, x_t, ttab.cpu()[idx.cpu()], weighting, 0.5, sd_f)
        for name, t in (("node", node), ("fallback", fb)):
            el = ((t["loss"].cpu().double() - rl).abs() / b_l).max().item()
            es = ((t["dm_norm"].cpu().double() - rs).abs() / b_s).max().item()
            print(f"{name} ({weighting}, fake sigma_data {sd_f}) |err| / kernel bound: loss {el:.3f}, dm_norm {es:.3f}; x equal bits: "
                  f"{torch.equal(t['x'], x)}")
            assert el <= 1 and es <= 1, (name, weighting, el, es)


def test_hip_refusals(ops):
    gen_net, real, fake = build(), build(), build(None, "fake:")
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    sim, steps = (v.to(DEV) for v in _sim_operands())
    dd = _diffusion()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx, model_kwargs={"y": y})
    with pytest.raises(NotImplementedError, match="K = 1 only"):
        dd.sid_generator_losses(gen_net, z, S_NET, gen_sigmas=LADDERS[3], **kw)
    with pytest.raises(ValueError, match="steps"):
        dd.dm_generator_losses(gen_net, z, S_NET, gen_sigmas=LADDERS[3], steps=steps + 1, sim_noise=sim, **kw)
    with pytest.raises(ValueError, match="sim_noise"):
        dd.dm_generator_losses(gen_net, z, S_NET, gen_sigmas=LADDERS[3], steps=steps, sim_noise=sim[:1], **kw)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        dd.dm_generator_losses(gen_net, z, S_NET, gen_sigmas=LADDERS[3], steps=steps, sim_noise=sim.clone().requires_grad_(True), **kw)
    with pytest.raises(ValueError, match="excludes gen_sigma"):
        dd.dm_generator_losses(gen_net, z, S_NET, gen_sigmas=LADDERS[3], gen_sigma=80.0, **kw)


# ------------------------------------------------------------------------------------------ sampler
def test_dm_sample_k3_vs_fp64_and_nfe(ops):
    from models.cm.karras_diffusion import dm_sample
    K, N = 3, 4
    sig = ladder_tab(K)
    gen = torch.Generator().manual_seed(21)
    draws = [torch.randn(N, 3, 16, 16, generator=gen) for _ in range(K)]

    class Replay:
        def __init__(self):
            self.left = list(draws)

        def randn(self, *shape, device=None):
            return self.left.pop(0).to(device)
    net = _Analytic()
    calls = []
    hook = net.register_forward_hook(lambda m, a, out: calls.append(1))
    try:
        outs = {clip: dm_sample(_diffusion(), net, (N, 3, 16, 16), clip_denoised=clip, generator=Replay(), device=DEV, gen_sigmas=LADDERS[K])
                for clip in (True, False)}
    finally:
        hook.remove()
    assert len(calls) == 2 * K                                              # NFE = K per call
    x = draws[0].double() * float(sig[0])
    M = x.abs()
    for j in range(K):
        s = sig[j].expand(N)
        cs, co, ci = scal64(s)
        arg = 0.7 * ci * x + 1e-3 * e(250 * torch.log(s.double()))
        F = 4.0 * torch.tanh(arg)
        D = co * F + cs * x
        # the error carried into G_j by x (slope <= c_skip + 2.8 c_out c_in), the rounding of tanh's argument, and this stage's own
        M = (cs + 2.8 * co * ci) * M + co * 4.0 * arg.abs() + (co * F).abs() + (cs * x).abs()
        if j < K - 1:
            n = draws[j + 1].double() * float(sig[j + 1])
            x, M = D + n, M + n.abs()
    assert close(outs[False], D, M) and close(outs[True], D.clamp(-1, 1), M)
    assert torch.equal(outs[True], outs[False].clamp(-1, 1)) and outs[False].abs().max() > 1
    drawn = dm_sample(_diffusion(), net, (N, 3, 16, 16), device=DEV, gen_sigmas=LADDERS[K])
    assert torch.isfinite(drawn).all() and drawn.std() > 0
    one = dm_sample(_diffusion(), net, (N, 3, 16, 16), generator=_Replay(draws[0]), device=DEV, gen_sigmas=[80.0])
    assert torch.equal(one, dm_sample(_diffusion(), net, (N, 3, 16, 16), generator=_Replay(draws[0]), device=DEV, gen_sigma=80.0))


@pytest.mark.parametrize("kind", ["determ", "determ-indiv"])
def test_dm_sample_k3_batch_invariance(ops, kind):
    from models.cm.karras_diffusion import dm_sample
    from models.cm.random_util import get_generator
    net = build(None, "", GEN_SCALE)
    y = torch.tensor([3, 871, 40, 999, 7, 512], device=DEV)
    gen = get_generator(kind, 6, seed=(1 << 35) + 3)

    def run(done, rows):
        gen.set_done_samples(done)
        out = dm_sample(_diffusion(), net, (rows.stop - rows.start, 3, 16, 16), model_kwargs={"y": y[rows]}, generator=gen, device=DEV,
                        gen_sigmas=LADDERS[3])
        assert gen.draw == 3                                              # z and one draw number per stage, as randn would take them
        return out.clone()
    whole = run(0, slice(0, 6))
    parts = torch.cat([run(0, slice(0, 3)), run(3, slice(3, 6))])
    assert torch.equal(whole, parts) and not torch.equal(whole[0], whole[1])
    # the launch's own noise is the generator's: the same images from randn draws handed over as eps
    gen.set_done_samples(0)
    zs = [gen.randn(6, 3, 16, 16, device=DEV) for _ in range(3)]

    class Replay:
        def randn(self, *shape, device=None):
            return zs.pop(0)
    assert torch.equal(dm_sample(_diffusion(), net, (6, 3, 16, 16), model_kwargs={"y": y}, generator=Replay(), device=DEV,
                                 gen_sigmas=LADDERS[3]), whole)


# ------------------------------------------------------------------------------------------ DMTrainLoop
@pytest.mark.parametrize("use_fp16", [True, False])
def test_dmtrainloop_k2_on_the_device(ops, tmp_path, use_fp16):
    ITERS, EVERY = 5, 2
    z = _latents()
    tl = _loop(tmp_path, use_fp16, gen_sigmas=LADDERS[2])
    assert tl.gen_sigmas == LADDERS[2]
    probe = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    pt = torch.tensor([1.5, -2.0], device=DEV)
    infer = lambda net: net.forward_inference(probe, pt).clone()
    gens, fakes, emas, lg = {}, {}, {}, None
    g_prev, f_prev, out_prev = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone(), infer(tl.model)
    for k in range(ITERS):
        took_gen, took_fake = _run(tl, k, z)
        on = k % EVERY == 0
        assert took_gen == on and took_fake, k
        gens[k], fakes[k] = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
        emas[k] = torch.cat([_flat(p) for p in tl.ema_params]).clone()
        assert torch.equal(gens[k], g_prev) != on and not torch.equal(fakes[k], f_prev), k
        out = infer(tl.model)
        assert torch.equal(out, out_prev) != on, k                   # the packed weights change exactly on the generator's turns
        assert tl.model._packed_key == tl.model._param_key()
        g_prev, f_prev, out_prev = gens[k], fakes[k], out
        if tl.step == 2:
            tl.save()
            lg = (tl.mp_trainer.lg_loss_scale, tl.fake_trainer.lg_loss_scale)
    row = tl.dumpkvs()
    assert all(math.isfinite(row[k]) for k in ("loss", "dm_norm", "fake_mse"))
    tr = _loop(tmp_path, use_fp16, resume=str(tmp_path / "model000002.pt"), gen_sigmas=LADDERS[2])
    assert tr.step == 2 and torch.equal(_flat(tr.model.parameters()), gens[1])
    tr.mp_trainer.lg_loss_scale, tr.fake_trainer.lg_loss_scale = lg          # the loss scales are not checkpointed
    for k in (2, 3, 4):
        _run(tr, k, z)
        assert torch.equal(_flat(tr.model.parameters()), gens[k]), k
        assert torch.equal(_flat(tr.fake_model.parameters()), fakes[k]), k
        assert torch.equal(torch.cat([_flat(p) for p in tr.ema_params]), emas[k]), k
    with pytest.raises(NotImplementedError, match="one-step generator"):
        _loop(tmp_path / "s", use_fp16, gen_sigmas=LADDERS[2], objective="sid")


# ------------------------------------------------------------------------------------------ command line
def test_cli_cm_train_gen_sigmas_then_sample(ops, tmp_path):
    """cm_train.py --training_mode dm --gen_sigmas, 3 iterations on a shrunken config; then generate_large.py --karras_sampler dm
    --gen_sigmas on the generator it wrote, with --generator determ."""
    from test_hip_cm_train import TINY_KW
    shrunk = dict(image_size=16, num_channels=64, num_res_blocks=1, channel_mult="1,2", attention_resolutions="8", num_head_channels=64,
                  class_cond=True, resblock_updown=True)
    args = [a for k, v in shrunk.items() for a in (f"--{k}", str(v))]
    over = dict(TINY_KW, **shrunk)
    teacher = build(over, "teacher:", GEN_SCALE)
    torch.save(teacher.state_dict(), tmp_path / "teacher.pt")
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1", RANK="0")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "cm_train.py", "--training_mode", "dm", "--teacher_model_path",
                        str(tmp_path / "teacher.pt"), "--max_iters", "3", "--batch_size", "4", "--microbatch", "2", "--use_fp16", "True",
                        "--gen_update_every", "2", "--dm_num_scales", "18", "--save_interval", "2", "--log_interval", "1",
                        "--ema_rate", "0.999,0.9", "--lr", "1e-4", "--gen_sigmas", "80,5,0.5", "--log_dir", str(tmp_path / "run")] + args,
                       cwd=PKG, env=env, capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "gen_sigmas (80.0, 5.0, 0.5) (K = 3)" in r.stdout, r.stdout[-2000:]
    files = set(os.listdir(tmp_path / "run"))
    assert {"model000002.pt", "fake_model000002.pt", "fake_opt000002.pt", "model000003.pt", "progress.jsonl"} <= files, files
    rows = [json.loads(l) for l in open(tmp_path / "run" / "progress.jsonl")]
    assert len(rows) == 3 and all(math.isfinite(r_[k]) for r_ in rows for k in ("loss", "dm_norm", "fake_mse"))

    import dxmi_config
    os.makedirs(tmp_path / "gen")
    samp = dict(sample_shape=[3, 16, 16], n_timesteps=4, class_cond=True, num_classes=1000, trainable_beta="fix_last",
                stochastic_last=True, rho=4.0)
    dxmi_config.save(dxmi_config.Cfg({"diffusion": dict(over, distillation=False), "sampler": samp, "training": {"seed": 42}}),
                     os.path.join(tmp_path / "gen", "config.yaml"))
    gen_args = ["--log_dir", str(tmp_path / "gen"), "--karras_sampler", "dm", "--pretrained", str(tmp_path / "run" / "model000002.pt"),
                "--n_sample", "4", "--batchsize", "2", "--gen_sigmas", "80,5,0.5", "--generator", "determ"]
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "generate_large.py"] + gen_args, cwd=PKG, env=env,
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "3 NFE/image (dm, 3 steps)" in r.stdout, r.stdout[-2000:]
    npz = np.load(tmp_path / "gen" / "samples_4.npz")["arr_0"]
    assert npz.shape == (4, 16, 16, 3) and npz.dtype == np.uint8 and npz.std() > 0
