"""Adversarial score identity distillation on the device (SiDA): the two map launches of csrc/sida_train.hip against
float64 on the same bf16 operands, the bottleneck tap of input_forward / input_backward, KarrasDenoiser.sida_generator_losses and
sida_discriminator_losses against float64 oracle nets, DMTrainLoop(objective="sida") and the command line.

Bounds of the map launches, from the summation order the kernel implements (u = 2^-24):
  logit   a lane adds the 8 channels of each of its ceil(Cb / 512) 16-byte vectors in order, the wave's xor-shuffle tree adds 6
          levels, one division by Cb follows: depth = 8 ceil(Cb / 512) + 6 + 1 roundings on sums of |h| (bf16 -> fp32 is exact), so
          |logit - logit64| <= depth u mean_c|h|
  a       softplus is 1-Lipschitz, so the logit bound passes through it and through the mean over the positions unchanged; the
          softplus itself (expf, log1pf: a few ulp), the at most ceil(P / 4) + 2 additions of positive terms and the division by P
          stay inside 64 u |a|
  d_h     one rounding to bf16 (relative 2^-8) of the fp32 value, whose own error (a product, expf, two divisions, a product) stays
          inside 16 u |v|
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from backward_bounds import U16
from test_hip_cm_train import PLAIN
from test_hip_dm_train import DEV, FAKE_SCALE, GEN_SCALE, NET_Y, N_NET, PKG, S_NET, U, _cos, _diffusion, _flat, _oracle64, build, e, scal64
from test_hip_gan import BOTTLENECK_MEASURED, CAP, ENC_Y, N_ENC, _cfg, _enc_operands, _grad_report, _is_decoder
from test_hip_sid_train import GEN_SIGMAS, NET_IDX, SID_LOSS_REL_CAP, _net_operands

pytestmark = pytest.mark.gpu
SENTINEL, PAD = -12288.0, 64      # (exact in bf16)
LEVELS = (0.0, 30.0, -30.0, 0.5, -3.0)      # logits around 0 and at +-30: both branches of max(v, 0) + log1p(exp(-|v|)) at both signs
ALPHA = 1.2
# sida_gen_weight of the oracle test per gen_sigma, chosen on the CPU oracle (indices NET_IDX) so that the adversarial part of the
# generator's gradient has about the norm of the SiD part (|grad sid| / |grad adv| = 1.628 and 1.634 there, and the twin without the
# adversarial cotangent then has per-parameter cosines of at most 0.83 and 0.73); asserted on the oracle in every run
SIDA_TEST_WEIGHT = {80.0: 1.6, 2.5: 1.6}
# worst per-sample relative errors against the float64 oracle, measured on an MI355X: loss 1.887e-3 at gen_sigma 80 and 2.053e-3 at 2.5,
# adv_loss 6.808e-4 and 5.755e-4 (its cap, derived in the test from the bottleneck's standing cap, is 2.06e-2)
SIDA_LOSS_REL_MEASURED = 2.053e-3
SIDA_ADV_REL_MEASURED = 6.808e-4
SIDA_LOSS_REL_BOUND, SIDA_ADV_REL_BOUND = 2 * SIDA_LOSS_REL_MEASURED, 2 * SIDA_ADV_REL_MEASURED


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


# ------------------------------------------------------------------------------------------ the map launches
def _softplus64(v):
    return torch.clamp(v, min=0) + torch.log1p(torch.exp(-v.abs()))


def _sigmoid64(v):
    return 1 / (1 + torch.exp(-v))


def _map_operands(N, P, Cb, seed):
    """h bf16 [N, P, Cb] whose channel means sit at LEVELS (cycling over image + position) with unit noise around them, mixed signs,
    coefficients of both signs."""
    gen = torch.Generator().manual_seed(seed)
    level = torch.tensor([[LEVELS[(n + p) % len(LEVELS)] for p in range(P)] for n in range(N)])
    h = (level[:, :, None] + torch.randn(N, P, Cb, generator=gen)).to(torch.bfloat16)
    sign = [1 if (n * 7 + 3) % 3 else -1 for n in range(N)]
    coef = [(-1.0) ** n * (0.5 + 1.7 * n) for n in range(N)]
    up = torch.rand(N, generator=gen) + 0.5
    return h, sign, coef, up


def _logit_depth(Cb):
    return 8 * math.ceil(Cb / 512) + 6 + 1


def _guard(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
    return buf[PAD:PAD + n].view(*shape), buf


def _untouched(buf):
    return bool((buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all())


def _map_with_guards(ops, h, sign, coef, up):
    """Both launches through the C entry points with sentinels around every buffer they write (and around h) -> (logit, a, d_h)."""
    import ctypes
    from dxmi_hip import _lib
    N, P, Cb = h.shape
    (hg, hb), (lg, lb), (ag, ab), (dg, db) = (_guard((N, P, Cb), torch.bfloat16), _guard((N, P), torch.float32), _guard((N,), torch.float32),
                                              _guard((N, P, Cb), torch.bfloat16))
    hg.copy_(h)
    sg, cf = (ctypes.c_int32 * N)(*sign), (ctypes.c_float * N)(*coef)
    lib, st = _lib.load(), ops._stream()
    ops.check(lib.dxmi_sida_map_fwd(ops._ptr(hg), sg, ops._ptr(lg), ops._ptr(ag), N, P, Cb, st), "dxmi_sida_map_fwd")
    ops.check(lib.dxmi_sida_map_bwd(ops._ptr(lg), sg, cf, ops._ptr(up), ops._ptr(dg), N, P, Cb, st), "dxmi_sida_map_bwd")
    torch.cuda.synchronize()
    assert all(_untouched(b) for b in (hb, lb, ab, db)) and torch.equal(hg, h)
    return lg.clone(), ag.clone(), dg.clone()


MAP_SHAPES = [(N, P, Cb) for N in (1, 7) for P in (1, 16, 64) for Cb in (128, 192, 768)] + \
             [(2, 3, 8), (2, 5, 4096), (3, 7, 520), (65, 4, 128), (130, 1, 64)]      # one lane; two trips of the vector loop; a ragged
                                                                                       # last vector row; two and three launches


@pytest.mark.parametrize("N,P,Cb", MAP_SHAPES)
def test_map_launches_vs_fp64(ops, N, P, Cb):
    h, sign, coef, up = _map_operands(N, P, Cb, seed=N * 1000 + P * 10 + Cb)
    hd, upd = h.to(DEV), up.to(DEV)
    logit, a = ops.sida_map_fwd(hd, sign)
    assert logit.shape == (N, P) and a.shape == (N,) and logit.dtype == torch.float32
    h64, s64 = h.double(), torch.tensor(sign, dtype=torch.float64)
    logit64 = h64.sum(dim=2) / Cb
    b_logit = _logit_depth(Cb) * U * h64.abs().mean(dim=2)
    f_logit = ((logit.cpu().double() - logit64).abs() / b_logit).max().item()
    a64 = _softplus64(s64[:, None] * logit64).mean(dim=1)
    b_a = b_logit.mean(dim=1) + 64 * U * a64.abs()
    f_a = ((a.cpu().double() - a64).abs() / b_a).max().item()
    # the backward on the device's own logits (the same operands), with and without the upstream
    fr = []
    for u_dev, u64 in ((None, torch.ones(N, dtype=torch.float64)), (upd, up.double())):
        d_h = ops.sida_map_bwd(logit, sign, coef, Cb, upstream=u_dev)
        assert d_h.shape == (N, P, Cb) and d_h.dtype == torch.bfloat16
        c64 = torch.tensor(np.asarray(coef, dtype=np.float32).astype(np.float64)) * u64
        v64 = (c64 * s64)[:, None] * _sigmoid64(s64[:, None] * logit.cpu().double()) / (P * Cb)
        got = d_h.cpu().double()
        assert (got == got[:, :, :1]).all()                      # one value per position
        fr.append(((got[:, :, 0] - v64).abs() / (U16 * v64.abs() + 16 * U * v64.abs() + 1e-300)).max().item())
    print(f"sida map [{N}, {P}, {Cb}] |err| / bound: logit {f_logit:.3f} (depth {_logit_depth(Cb)}), a {f_a:.3f}, d_h {fr[0]:.3f} / {fr[1]:.3f}")
    assert f_logit <= 1 and f_a <= 1 and max(fr) <= 1
    assert torch.isfinite(a).all() and (a > 0).all()
    # two runs give the same bits, and the entry points write nothing outside their buffers
    lg, ag, dg = _map_with_guards(ops, hd, sign, coef, upd)
    assert torch.equal(lg, logit) and torch.equal(ag, a) and torch.equal(dg, ops.sida_map_bwd(logit, sign, coef, Cb, upstream=upd))
    if N == 7:                                                   # seven images are three plus four, bitwise
        for r in (slice(0, 3), slice(3, 7)):
            l2, a2 = ops.sida_map_fwd(hd[r].contiguous(), sign[r])
            assert torch.equal(l2, logit[r]) and torch.equal(a2, a[r])
            d2 = ops.sida_map_bwd(l2, sign[r], coef[r], Cb, upstream=upd[r].contiguous())
            assert torch.equal(d2, dg[r])
    if N >= 65:                                                  # an image of the second launch's chunk is itself alone
        l2, a2 = ops.sida_map_fwd(hd[64:65].contiguous(), sign[64:65])
        assert torch.equal(l2, logit[64:65]) and torch.equal(a2, a[64:65])


def test_map_softplus_branches_and_scalar_operands(ops):
    """softplus(+-30) and softplus(-+30) to their float64 values (no overflow, no cancellation), and a scalar sign / coef stands for
    every image."""
    h = torch.full((2, 4, 128), 30.0).to(torch.bfloat16)
    h[1] = -30.0
    for sign in (1, -1):
        logit, a = ops.sida_map_fwd(h.to(DEV), sign)
        assert torch.equal(logit.cpu(), torch.tensor([[30.0] * 4, [-30.0] * 4]))
        ref = _softplus64(sign * torch.tensor([30.0, -30.0], dtype=torch.float64))
        assert ((a.cpu().double() - ref).abs() <= 64 * U * ref).all(), (a, ref)
        d_h = ops.sida_map_bwd(logit, sign, 2.0, 128, shape=(2, 2, 2, 128))
        assert d_h.shape == (2, 2, 2, 128)
        v = 2.0 * sign * _sigmoid64(sign * torch.tensor([30.0, -30.0], dtype=torch.float64)) / (4 * 128)
        assert ((d_h.cpu().double()[:, 0, 0, 0] - v).abs() <= (U16 + 16 * U) * v.abs()).all()
        assert torch.equal(d_h, ops.sida_map_bwd(logit, [sign] * 2, [2.0, 2.0], 128, shape=(2, 2, 2, 128)))


def test_map_wrappers_refuse_malformed_arguments(ops):
    from dxmi_hip import DxmiError
    h = torch.zeros(4, 16, 128, dtype=torch.bfloat16, device=DEV)
    logit, _ = ops.sida_map_fwd(h, 1)
    off = torch.zeros(4 * 16 * 128 + 1, dtype=torch.bfloat16, device=DEV)[1:].view(4, 16, 128)
    bad_calls = [
        lambda: ops.sida_map_fwd(h, 0),
        lambda: ops.sida_map_fwd(h, [1, 1, 2, 1]),
        lambda: ops.sida_map_fwd(h, [1, -1]),
        lambda: ops.sida_map_fwd(h, torch.ones(4, device=DEV)),
        lambda: ops.sida_map_fwd(h.float(), 1),
        lambda: ops.sida_map_fwd(h.cpu(), 1),
        lambda: ops.sida_map_fwd(h[:, :, :100], 1),
        lambda: ops.sida_map_fwd(torch.zeros(4, 16, 100, dtype=torch.bfloat16, device=DEV), 1),
        lambda: ops.sida_map_fwd(off, 1),
        lambda: ops.sida_map_bwd(logit, 1, float("nan"), 128),
        lambda: ops.sida_map_bwd(logit, 1, [1.0, 1.0, float("inf"), 1.0], 128),
        lambda: ops.sida_map_bwd(logit, 3, 1.0, 128),
        lambda: ops.sida_map_bwd(logit, 1, 1.0, 100),
        lambda: ops.sida_map_bwd(logit, 1, 1.0, 128, upstream=torch.ones(3, device=DEV)),
        lambda: ops.sida_map_bwd(logit, 1, 1.0, 128, upstream=torch.ones(4)),
        lambda: ops.sida_map_bwd(logit, 1, 1.0, 128, shape=(4, 4, 4, 64)),
        lambda: ops.sida_map_bwd(logit.double(), 1, 1.0, 128),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"call {i} was accepted")


# ------------------------------------------------------------------------------------------ the tap
def _walk_roundings(tape):
    """bf16 tensors written on the walk from the bottleneck to the stem: per residual block conv2's data gradient, GroupNorm 2, conv1's
    data gradient, the resampling, GroupNorm 1 and the shortcut (6); per attention block proj, attention, qkv, GroupNorm (4); one per
    downsample and one per skip-connection add."""
    upto = next(i for i, en in enumerate(tape) if en[0] == "tap")
    kinds = [en[0] for en in tape[:upto]]
    return 6 * kinds.count("res") + 4 * kinds.count("attn") + kinds.count("down") + kinds.count("push")


@pytest.mark.parametrize("plain", [False, True])
def test_bottleneck_tap(ops, plain):
    """input_forward(tap=True) / input_backward(d_tap=...) on the shrunken net.

    The cross-check's bound.  With a = input_backward(v) and b = encoder_input_backward(d_tap), the joint walk differs from a + b by
    the one extra rounding of the add at the bottleneck and by where the D bf16 roundings of the encoder's walk fall: on the sum in the
    joint walk (D + 1 roundings of tensors the size of a + b), on the two parts in the separate ones (D each).  A rounding to bf16 moves
    an element by at most half a unit in the last place, 2^-8 relative, and as an error uniform over that interval by 2^-8 / sqrt(3)
    relative in the root mean square; the 3 D + 1 roundings fall on different tensors and are taken as independent, so their L2
    contributions add in quadrature:
        || joint - (a + b) || <= 2 (2^-8 / sqrt 3) sqrt((D + 1) ||a + b||^2 + D ||a||^2 + D ||b||^2)
    the factor 2 allowing for a layer of the walk passing an error on up to twice as large, relative to its result, as it came in.  D
    is counted from the tape (_walk_roundings).  At D = 41 and ||a|| = ||b|| that is 0.03 (||a|| + ||b||): a tap cotangent wrong by
    a few per cent fails it, a dropped one by a factor of 15.  The cotangents are scaled (on the oracle, by a power of two) so that
    ||a|| and ||b|| are of one size."""
    from models.cm import unet_train as ut
    from oracle import Precision
    net = build(PLAIN if plain else None, "", GEN_SCALE).train()
    x, t, d_tap = _enc_operands()
    v = torch.randn(N_ENC, 3, 16, 16, generator=torch.Generator().manual_seed(43))
    y = None if plain else torch.tensor(ENC_Y)
    yd = None if plain else y.to(DEV)
    sd = {k: p.detach().cpu() for k, p in net.state_dict().items()}
    with _oracle64() as edm:
        x64 = x.double().requires_grad_(True)
        trace = []
        F64 = edm.unet_forward({k: p.double() for k, p in sd.items()}, _cfg(edm, plain), x64, t.double(), y=y, prec=Precision("fp32"), trace=trace)
        mid = dict(trace)["middle_block"]
        g_v, = torch.autograd.grad((F64 * v.double()).sum(), x64, retain_graph=True)
        g_t, = torch.autograd.grad((mid * d_tap.double().permute(0, 3, 1, 2)).sum(), x64)
    scale = 2.0 ** round(math.log2(float(g_v.norm() / g_t.norm())))
    d_tap, g_t = (d_tap.float() * scale).to(torch.bfloat16), g_t * scale
    ratio = float(g_t.norm() / g_v.norm())
    print(f"tap ({'plain' if plain else 'tiny'}): oracle |J^T v| {float(g_v.norm()):.3e}, |J_enc^T d_tap| {float(g_t.norm()):.3e} (d_tap x {scale})")
    assert 0.7 <= ratio <= 1.5
    xd, td, vd, dd = x.to(DEV), t.to(DEV), v.to(DEV), d_tap.to(DEV)
    F0, tape0 = ut.input_forward(net, xd, td, yd)
    F1, tape1 = ut.input_forward(net, xd, td, yd, tap=True)
    F2, tape2 = ut.input_forward(net, xd, td, yd, tap=True)
    h, etape = ut.encoder_input_forward(net, xd, td, yd)
    assert net.training and not hasattr(tape0, "bottleneck") and not any(en[0] == "tap" for en in tape0.tape)
    assert torch.equal(F1, F0) and torch.equal(tape1.bottleneck, h) and h.dtype == torch.bfloat16
    g0 = ut.input_backward(tape0, vd)
    g1 = ut.input_backward(tape1, vd, None)
    assert torch.equal(g1, g0)                                                  # no cotangent: today's walk, bit for bit
    D = _walk_roundings(tape2.tape)
    g2 = ut.input_backward(tape2, vd, dd)
    worst = [(1.0, ""), (0.0, "")]
    _grad_report("dx", g2, g_v + g_t, worst)
    b = ut.encoder_input_backward(etape, dd)
    na, nb = float(g0.double().norm()), float(b.double().norm())
    diff = float((g2.double() - (g0.double() + b.double())).norm())
    nab = float((g0.double() + b.double()).norm())
    bound = 2 * (U16 / math.sqrt(3)) * math.sqrt((D + 1) * nab ** 2 + D * na ** 2 + D * nb ** 2)
    print(f"tap ({'plain' if plain else 'tiny'}): joint walk vs oracle: cosine {worst[0][0]:.5f}, norm deviation {worst[1][0]:.4f}; "
          f"joint - (a + b): {diff:.3e} = {diff / bound:.3f} of the bound (D = {D}, |a| {na:.3e}, |b| {nb:.3e})")
    assert worst[0][0] >= 0.995 and worst[1][0] <= 0.05
    assert diff <= bound < 0.1 * nb
    assert all(p.grad is None for p in net.parameters())
    with pytest.raises(ValueError, match="tap=True"):
        ut.input_backward(ut.input_forward(net, xd, td, yd)[1], vd, dd)
    with pytest.raises(ValueError, match="tap cotangent"):
        ut.input_backward(ut.input_forward(net, xd, td, yd, tap=True)[1], vd, dd[:, :4])


# ------------------------------------------------------------------------------------------ the generator's loss on the shrunken nets
def _oracle_sida(gen_sd, fake_sd, z, noise, idx, y, alpha, gen_sigma):
    """sida_generator_losses on float64 oracle nets (the real net shares the generator's weights, as constants): the SiD part
    sid_n and the adversarial part adv_n / s_n, each differentiated by autograd through x and through everything x_t feeds ->
    dict(sid, adv, s, logit, mid, g_sid, g_adv): loss = sid + w adv / s and its gradient g_sid + w g_adv for any weight w."""
    from models.cm.karras_diffusion import cd_levels
    from oracle import Precision
    t = cd_levels(S_NET, 0.002, 80.0, 7.0).table.double()[idx]
    with _oracle64() as edm:
        cfg = _cfg(edm, False)
        trace = []

        def den(sd, x_t, s, trace=None):
            cs, co, ci = scal64(s)
            return co * edm.unet_forward(sd, cfg, ci * x_t, 250 * torch.log(s), y=y, prec=Precision("fp32"), trace=trace) + cs * x_t
        leaves = {k: v.double().requires_grad_(True) for k, v in gen_sd.items()}
        real = {k: v.double() for k, v in gen_sd.items()}
        fake = {k: v.double() for k, v in fake_sd.items()}
        x = den(leaves, z.double() * gen_sigma, torch.full((len(z),), gen_sigma, dtype=torch.float64))
        x_t = x + noise.double() * e(t)
        D_r, D_f = den(real, x_t, t), den(fake, x_t, t, trace)
        mid = dict(trace)["middle_block"]                                    # the SAME evaluation of the fake net
        s = (x - D_r).abs().mean(dim=[1, 2, 3]).detach()
        delta = D_r - D_f
        isum = lambda v: v.sum(dim=[1, 2, 3])
        sid = ((1 - alpha) * isum(delta ** 2) + isum(delta * (D_f - x))) / (x[0].numel() * s)
        logit = mid.mean(dim=1).flatten(1)
        adv = _softplus64(-logit).mean(dim=1)
        g_sid = torch.autograd.grad(sid.sum(), list(leaves.values()), retain_graph=True)
        g_adv = torch.autograd.grad((adv / s).sum(), list(leaves.values()))
    return dict(sid=sid.detach(), adv=adv.detach(), s=s, logit=logit.detach(), mid=mid.detach(), g_sid=dict(zip(leaves, g_sid)),
                g_adv=dict(zip(leaves, g_adv)))


def _norm(gs):
    return math.sqrt(sum(float(v.double().pow(2).sum()) for v in gs.values()))


@pytest.fixture(scope="module")
def nets():
    gen_net, real, fake = build(None, "", GEN_SCALE), build(None, "", GEN_SCALE), build(None, "fake:", FAKE_SCALE)
    for p in gen_net.parameters():
        p.requires_grad_(True)
    return gen_net, real, fake


@pytest.fixture(scope="module")
def oracle(nets):
    """One float64 oracle pass per gen_sigma, shared by the tests below and left unchanged."""
    gen_net, _, fake = nets
    z, noise, idx, y = _net_operands()
    gen_sd = {k: v.detach().cpu() for k, v in gen_net.state_dict().items()}
    fake_sd = {k: v.detach().cpu() for k, v in fake.state_dict().items()}
    return {gs: _oracle_sida(gen_sd, fake_sd, z, noise, idx, y, ALPHA, gs) for gs in GEN_SIGMAS}


@pytest.mark.parametrize("gen_sigma", GEN_SIGMAS)
def test_sida_generator_losses_vs_fp64_oracle(ops, nets, oracle, gen_sigma):
    """Figures measured on an MI355X (gen_sigma 80 / 2.5): see SIDA_LOSS_REL_MEASURED and SIDA_ADV_REL_MEASURED above."""
    gen_net, real, fake = nets
    z, noise, idx, y = _net_operands()
    ref, w = oracle[gen_sigma], SIDA_TEST_WEIGHT[gen_sigma]
    n_sid, n_adv = _norm(ref["g_sid"]), w * _norm(ref["g_adv"])
    true = {n: ref["g_sid"][n] + w * ref["g_adv"][n] for n in ref["g_sid"]}
    compared = [n for n, rg in true.items() if rg.norm() >= 1e-6 * max(1.0, ref["g_sid"][n].norm().item())]
    twin = [_cos(ref["g_sid"][n], true[n]) for n in compared]             # the twin without the adversarial cotangent IS the SiD part
    print(f"gen_sigma {gen_sigma}: oracle: |grad sid| {n_sid:.4e}, sida_gen_weight {w} x |grad adv| = {n_adv:.4e} (ratio {n_adv / n_sid:.3f}); "
          f"the twin without the adversarial cotangent has per-parameter cosine in [{min(twin):.3f}, {max(twin):.3f}]")
    assert 0.3 <= n_adv / n_sid <= 3.0
    assert max(twin) <= 0.95                                              # no parameter's gradient passes without the adversarial path
    d = _diffusion()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, model_kwargs={"y": y.to(DEV)}, noise=noise.to(DEV),
              indices=idx.to(DEV), gen_sigma=gen_sigma, alpha=ALPHA, sida_gen_weight=w)
    gen_net.zero_grad()
    t = d.sida_generator_losses(gen_net, z.to(DEV), S_NET, **kw)
    assert set(t) == {"loss", "x", "dm_norm", "adv_loss", "adv_logit"} and t["loss"].requires_grad
    assert not any(t[k].requires_grad for k in ("x", "dm_norm", "adv_loss", "adv_logit")) and t["adv_logit"].shape == (N_NET, 64)
    t["loss"].sum().backward()
    loss64 = ref["sid"] + w * ref["adv"] / ref["s"]
    rel = ((t["loss"].detach().cpu().double() - loss64).abs() / loss64.abs()).max().item()
    rel_adv = ((t["adv_loss"].cpu().double() - ref["adv"]).abs() / ref["adv"]).max().item()
    # the cap of adv_loss: |d adv_n| <= mean_p |d logit| <= ||d h_n||_2 / sqrt(P Cb) <= CAP rms(h_n), CAP test_hip_gan's cap of the
    # bottleneck's relative L2 error
    adv_cap = (CAP * ref["mid"].pow(2).mean(dim=[1, 2, 3]).sqrt() / ref["adv"]).min().item()
    P = dict(gen_net.named_parameters())
    worst = [(1.0, ""), (0.0, "")]
    for n in compared:
        _grad_report(n, P[n].grad, true[n], worst)
    twin_dev = min(_cos(P[n].grad.cpu(), ref["g_sid"][n]) for n in compared)
    print(f"gen_sigma {gen_sigma}: device: per-sample loss worst relative error {rel:.3e} (bound {SIDA_LOSS_REL_BOUND:.3e}, cap {SID_LOSS_REL_CAP}); "
          f"adv_loss {rel_adv:.3e} (bound {SIDA_ADV_REL_BOUND:.3e}, cap {adv_cap:.3e}); gradient worst cosine {worst[0][0]:.5f} "
          f"({worst[0][1]}), worst norm deviation {worst[1][0]:.4f} ({worst[1][1]}); worst cosine to the SiD part alone {twin_dev:.3f}")
    assert all(p.grad is None for net in (real, fake) for p in net.parameters())
    assert worst[0][0] >= 0.995 and worst[1][0] <= 0.05
    assert SIDA_LOSS_REL_BOUND <= SID_LOSS_REL_CAP and SIDA_ADV_REL_BOUND <= adv_cap
    assert rel <= SIDA_LOSS_REL_BOUND and rel_adv <= SIDA_ADV_REL_BOUND
    assert torch.allclose(t["adv_loss"].cpu().double(), _softplus64(-t["adv_logit"].cpu().double()).mean(dim=1), rtol=1e-5)
    with torch.no_grad():                            # no node: everything is still formed, from the same evaluations
        again = d.sida_generator_losses(gen_net, z.to(DEV), S_NET, **kw)
    assert set(again) == set(t) and not again["loss"].requires_grad
    for k in t:
        assert torch.equal(again[k], t[k].detach()), k


def test_weight_zero_is_sid_generator_losses_bitwise(ops, nets):
    gen_net, real, fake = nets
    z, noise, idx, y = _net_operands()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, model_kwargs={"y": y.to(DEV)}, noise=noise.to(DEV),
              indices=idx.to(DEV), gen_sigma=2.5, alpha=ALPHA)
    gen_net.zero_grad()
    a = _diffusion().sida_generator_losses(gen_net, z.to(DEV), S_NET, sida_gen_weight=0.0, **kw)
    a["loss"].sum().backward()
    ga = {n: p.grad.clone() for n, p in gen_net.named_parameters()}
    gen_net.zero_grad()
    b = _diffusion().sid_generator_losses(gen_net, z.to(DEV), S_NET, **kw)
    b["loss"].sum().backward()
    assert torch.equal(a["loss"].detach(), b["loss"].detach()) and torch.equal(a["x"], b["x"]) and torch.equal(a["dm_norm"], b["dm_norm"])
    assert all(torch.equal(ga[n], p.grad) for n, p in gen_net.named_parameters())
    assert float(a["adv_loss"].min()) > 0
    gen_net.zero_grad()


class _Wrapped:
    """A HIP net behind a plain callable with encode: the loss then takes its torch fallback."""

    def __init__(self, net):
        self.net = net

    def __call__(self, x_in, t, **kw):
        return self.net(x_in, t, **kw)

    def encode(self, x_in, t, **kw):
        return self.net.encode(x_in, t, **kw)


def test_device_node_vs_torch_fallback_on_the_same_nets(ops, nets):
    """x is bitwise equal; adv_logit and adv_loss agree to the rounding of two mean orders (the fallback's mean over channels is
    torch's), dm_norm and loss to fp32 roundings of the same expressions."""
    gen_net, real, fake = nets
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    kw = dict(real_diffusion=_diffusion(), model_kwargs={"y": y}, noise=noise, indices=idx, alpha=ALPHA, sida_gen_weight=0.3)
    with torch.no_grad():
        node = _diffusion().sida_generator_losses(gen_net, z, S_NET, real_model=real, fake_model=fake, **kw)
        fb = _diffusion().sida_generator_losses(_Wrapped(gen_net), z, S_NET, real_model=_Wrapped(real), fake_model=_Wrapped(fake), **kw)
    assert torch.equal(node["x"], fb["x"])
    assert set(node) == set(fb) and all(node[k].shape == fb[k].shape for k in node)
    h_abs = fake.encode(*_fake_point(z, noise, idx, node["x"]), y).abs().mean(dim=1).flatten(1)
    # (both read bitwise the same h: the kernel's order of depth _logit_depth, torch's mean over 128 channels of depth <= 128)
    assert ((node["adv_logit"] - fb["adv_logit"]).abs() <= (_logit_depth(128) + 128) * U * h_abs + 1e-30).all()
    assert torch.allclose(node["adv_loss"], fb["adv_loss"], rtol=1e-4) and torch.allclose(node["dm_norm"], fb["dm_norm"], rtol=1e-4)
    assert torch.allclose(node["loss"], fb["loss"], rtol=1e-2)


def _fake_point(z, noise, idx, x):
    from models.cm.karras_diffusion import cd_levels
    t = cd_levels(S_NET, 0.002, 80.0, 7.0).device_table(torch.device(DEV))[idx]
    c_in = _diffusion().get_scalings(t)[2]
    return c_in[:, None, None, None] * (x + noise * t[:, None, None, None]), 1000 * 0.25 * torch.log(t + 1e-44)


def test_generator_refusals_on_the_device(ops, nets):
    gen_net, real, fake = nets
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx, model_kwargs={"y": y})
    with pytest.raises(NotImplementedError, match="K = 1 only"):
        _diffusion().sida_generator_losses(gen_net, z, S_NET, gen_sigmas=(80.0, 2.5), **kw)
    with pytest.raises(ValueError, match="sida_gen_weight"):
        _diffusion().sida_generator_losses(gen_net, z, S_NET, sida_gen_weight=float("nan"), **kw)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        _diffusion().sida_generator_losses(gen_net, z.clone().requires_grad_(True), S_NET, **kw)
    with pytest.raises(ValueError, match="class-conditional"):
        _diffusion().sida_generator_losses(gen_net, z, S_NET, **dict(kw, model_kwargs={}))


# ------------------------------------------------------------------------------------------ the discriminator's loss
def test_sida_discriminator_losses_vs_fp64_oracle(ops, nets):
    from models.cm.karras_diffusion import cd_levels
    from oracle import Precision
    _, _, fake = nets
    gen = torch.Generator().manual_seed(19)
    x_fake = torch.randn(N_NET, 3, 16, 16, generator=gen) * 0.5
    x_real = torch.rand(N_NET, 3, 16, 16, generator=gen) * 2 - 1
    noise = torch.randn(2 * N_NET, 3, 16, 16, generator=gen)
    didx = torch.tensor(NET_IDX + (9, 3, 14, 6))
    y = torch.tensor(NET_Y)
    yy = torch.cat([y, y.flip(0)])
    t = cd_levels(S_NET, 0.002, 80.0, 7.0).table.double()[didx]
    with _oracle64() as edm:
        leaves = {k: v.detach().cpu().double().requires_grad_(True) for k, v in fake.state_dict().items()}
        xs = torch.cat([x_fake, x_real]).double()
        trace = []
        edm.unet_forward(leaves, _cfg(edm, False), scal64(t)[2] * (xs + noise.double() * e(t)), 250 * torch.log(t), y=yy, prec=Precision("fp32"),
                         trace=trace)
        mid = dict(trace)["middle_block"]
        logit = mid.mean(dim=1).flatten(1)
        loss64 = _softplus64(logit[:N_NET]).mean(dim=1) + _softplus64(-logit[N_NET:]).mean(dim=1)
        g64 = dict(zip(leaves, torch.autograd.grad(loss64.sum(), list(leaves.values()), allow_unused=True)))
    for p in fake.parameters():
        p.requires_grad_(True)
        p.grad = None
    try:
        terms = _diffusion().sida_discriminator_losses(fake, x_fake.to(DEV), x_real.to(DEV), S_NET, model_kwargs={"y": y.to(DEV)},
                                                       real_kwargs={"y": y.flip(0).to(DEV)}, noise=noise.to(DEV), indices=didx.to(DEV))
        assert set(terms) == {"loss", "logit_fake", "logit_real"} and terms["loss"].shape == (N_NET,)
        assert terms["logit_fake"].shape == (N_NET, 64) == terms["logit_real"].shape and not terms["logit_fake"].requires_grad
        terms["loss"].sum().backward()
        # per image: ||d logit_n||_2 <= ||d h_n||_2 / sqrt(Cb) <= CAP ||h_n||_2 / sqrt(Cb), CAP the standing cap of the bottleneck's
        # relative L2 error (test_hip_gan.py); softplus is 1-Lipschitz, so |d a_n| <= mean_p |d logit| <= ||d logit_n||_2 / sqrt(P)
        got = torch.cat([terms["logit_fake"], terms["logit_real"]]).double().cpu()
        err = (got - logit.detach()).norm(dim=1)
        bound = CAP * mid.detach().flatten(1).norm(dim=1) / math.sqrt(mid.shape[1])
        print(f"sida discriminator: per-image |logit error|_2 / bound {float((err / bound).max()):.3f} "
              f"(2 x the measured bottleneck error would be {2 * BOTTLENECK_MEASURED / CAP:.3f})")
        assert (err <= bound).all()
        b_loss = (bound[:N_NET] + bound[N_NET:]) / math.sqrt(logit.shape[1]) + 1e-6
        assert ((terms["loss"].detach().double().cpu() - loss64.detach()).abs() <= b_loss).all()
        worst, seen = [(1.0, ""), (0.0, "")], 0
        for name, p in fake.named_parameters():
            if _is_decoder(name):
                assert p.grad is None or not p.grad.any(), name
                assert ".emb_layers." in name or p.grad is None, name
                continue
            assert p.grad is not None and g64[name] is not None and float(g64[name].norm()) > 0, name
            _grad_report(name, p.grad, g64[name], worst)
            seen += 1
        print(f"sida discriminator: {seen} parameter gradients, worst cosine {worst[0][0]:.5f} ({worst[0][1]}), worst norm deviation "
              f"{worst[1][0]:.4f} ({worst[1][1]})")
        assert worst[0][0] >= 0.995 and worst[1][0] <= 0.05
        with pytest.raises(ValueError, match="one shape"):
            _diffusion().sida_discriminator_losses(fake, x_fake.to(DEV), x_real[:2].to(DEV), S_NET)
    finally:
        for p in fake.parameters():
            p.requires_grad_(False)
            p.grad = None


# ------------------------------------------------------------------------------------------ DMTrainLoop
LOOP_ITERS, LOOP_EVERY = 3, 2


def _run(tl, k, z):
    torch.manual_seed(1000 + k)
    return tl.run_step(z[k].to(DEV), {})


@pytest.mark.parametrize("use_fp16", [True, False])
def test_dmtrainloop_sida_on_the_device(ops, tmp_path, use_fp16):
    """Three iterations, generator turns at 0 and 2: the generator moves on its turns only, the fake net at every iteration, the teacher
    stays bitwise, the logs carry both adversarial terms, no file is added to the checkpoint, and a loop resumed from the save after
    iteration 1 repeats iteration 2 bit for bit."""
    from test_hip_dm_train import _loop
    gen = torch.Generator().manual_seed(99)
    z = [torch.randn(4, 3, 16, 16, generator=gen) for _ in range(LOOP_ITERS)]
    reals = [(torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1, {}) for _ in range(LOOP_ITERS)]
    over = dict(objective="sida", sid_alpha=1.2, gen_sigma=2.5, gen_update_every=LOOP_EVERY, sida_gen_weight=0.05, sida_dis_weight=0.5)
    tl = _loop(tmp_path, use_fp16, real_data=iter(reals), **over)
    teacher_w = _flat(tl.real_model.parameters()).clone()
    gens, fakes, lg = {}, {}, None
    g_prev, f_prev = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
    for k in range(LOOP_ITERS):
        took_gen, took_fake = _run(tl, k, z)
        on = k % LOOP_EVERY == 0
        assert took_gen == on and took_fake, k
        gens[k], fakes[k] = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
        assert torch.equal(gens[k], g_prev) != on and not torch.equal(fakes[k], f_prev), k
        assert torch.isfinite(gens[k]).all() and torch.isfinite(fakes[k]).all()
        assert torch.equal(_flat(tl.real_model.parameters()), teacher_w) and all(p.grad is None for p in tl.real_model.parameters()), k
        assert tl.fake_model.training and tl.model.training
        g_prev, f_prev = gens[k], fakes[k]
        if tl.step == 2:
            tl.save()
            lg = (tl.mp_trainer.lg_loss_scale, tl.fake_trainer.lg_loss_scale)
    row = tl.dumpkvs()
    assert all(math.isfinite(row[k]) for k in ("loss", "dm_norm", "fake_mse", "sida_gen", "sida_dis", "logit_fake", "logit_real"))
    files = set(os.listdir(tmp_path))
    assert {"model000002.pt", "fake_model000002.pt", "fake_opt000002.pt"} <= files and not any(f.startswith(("gan_head", "sida")) for f in files)
    tr = _loop(tmp_path, use_fp16, resume=str(tmp_path / "model000002.pt"), real_data=iter(reals[2:]), **over)
    assert tr.step == 2 and torch.equal(_flat(tr.model.parameters()), gens[1]) and torch.equal(_flat(tr.fake_model.parameters()), fakes[1])
    tr.mp_trainer.lg_loss_scale, tr.fake_trainer.lg_loss_scale = lg          # the loss scales are not checkpointed
    _run(tr, 2, z)
    assert torch.equal(_flat(tr.model.parameters()), gens[2]) and torch.equal(_flat(tr.fake_model.parameters()), fakes[2])
    from models.cm.train_util import DMTrainLoop
    with pytest.raises(ValueError, match="needs real_data"):
        _loop(tmp_path / "x", use_fp16, **over)
    assert isinstance(tl, DMTrainLoop)


# ------------------------------------------------------------------------------------------ command line
def test_cli_cm_train_sida_then_sample(ops, tmp_path):
    """cm_train.py --training_mode dm --dm_objective sida --synthetic_data True for 2 iterations on a shrunken config, then
    generate_large.py --karras_sampler dm on the generator it wrote: NFE = 1."""
    from test_hip_cm_train import TINY_KW
    shrunk = dict(image_size=16, num_channels=64, num_res_blocks=1, channel_mult="1,2", attention_resolutions="8", num_head_channels=64,
                  class_cond=True, resblock_updown=True)
    args = [a for k, v in shrunk.items() for a in (f"--{k}", str(v))]
    over = dict(TINY_KW, **shrunk)
    teacher = build(over, "teacher:", GEN_SCALE)
    torch.save(teacher.state_dict(), tmp_path / "teacher.pt")
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1", RANK="0")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "cm_train.py", "--training_mode", "dm", "--dm_objective", "sida",
                        "--synthetic_data", "True", "--gen_sigma", "2.5", "--sida_gen_weight", "0.05", "--teacher_model_path",
                        str(tmp_path / "teacher.pt"), "--max_iters", "2", "--batch_size", "4", "--microbatch", "2", "--use_fp16", "True",
                        "--gen_update_every", "1", "--dm_num_scales", "18", "--save_interval", "2", "--log_interval", "1", "--ema_rate",
                        "0.999", "--lr", "1e-4", "--log_dir", str(tmp_path / "run")] + args,
                       cwd=PKG, env=env, capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "objective sida (alpha 1.2, generator weight 0.05, discriminator weight 1.0), gen_sigma 2.5" in r.stdout, r.stdout[-2000:]
    files = set(os.listdir(tmp_path / "run"))
    assert {"model000002.pt", "ema_0.999_000002.pt", "opt000002.pt", "fake_model000002.pt", "fake_opt000002.pt", "progress.jsonl"} <= files, files
    assert not any(f.startswith("gan_head") for f in files)
    student = torch.load(tmp_path / "run" / "model000002.pt", map_location=DEV)
    te = teacher.state_dict()
    assert all(torch.isfinite(v).all() for v in student.values())
    assert any(not torch.equal(student[k], te[k]) for k in te)
    rows = [json.loads(l) for l in open(tmp_path / "run" / "progress.jsonl")]
    assert len(rows) == 2 and all(math.isfinite(r_[k]) for r_ in rows for k in ("loss", "dm_norm", "fake_mse", "sida_gen", "sida_dis"))
    # iteration 0 meets fake == real: the SiD part is 0 and the loss is the adversarial term alone, sida_gen_weight adv / s > 0
    assert rows[0]["loss"] > 0 and all(r_["dm_norm"] > 0 and r_["sida_gen"] > 0 for r_ in rows)

    import dxmi_config
    os.makedirs(tmp_path / "gen")
    samp = dict(sample_shape=[3, 16, 16], n_timesteps=4, class_cond=True, num_classes=1000, trainable_beta="fix_last",
                stochastic_last=True, rho=4.0)
    dxmi_config.save(dxmi_config.Cfg({"diffusion": dict(over, distillation=False), "sampler": samp, "training": {"seed": 42}}),
                     os.path.join(tmp_path / "gen", "config.yaml"))
    gen_args = ["--log_dir", str(tmp_path / "gen"), "--karras_sampler", "dm", "--gen_sigma", "2.5", "--pretrained",
                str(tmp_path / "run" / "model000002.pt"), "--n_sample", "4", "--batchsize", "2"]
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "generate_large.py"] + gen_args, cwd=PKG, env=env,
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "1 NFE/image (dm, 1 steps)" in r.stdout, r.stdout[-2000:]
    npz = np.load(tmp_path / "gen" / "samples_4.npz")["arr_0"]
    assert npz.shape == (4, 16, 16, 3) and npz.dtype == np.uint8 and npz.std() > 0
