"""Score identity distillation on the GPU: the two launches of csrc/sid_train.hip against float64 on the same fp32
operands, input_vjp against its two halves, KarrasDenoiser.sid_generator_losses on the shrunken HIP U-Nets against float64 oracle
nets differentiated through the denoisers' inputs, the device node against the torch fallback, DMTrainLoop(objective="sid"), and
the two command lines.

Bounds (the project's, as test_hip_dm_train.py writes them out; u = 2^-24): an elementwise result within 16 u M of float64, M the
magnitude of the operands that meet in it.  With M_r = |c_out_r F_r| + |c_skip_r x_t| (M_f likewise): delta = D_r - D_f has M_d =
M_r + M_f, e = D_f - x has M_e = M_f + |x|, a_r = k_r delta + e has M_ar = |k_r| M_d + M_e (a_f likewise), v_r: c_out_r M_ar, d_dir:
c_skip_r M_ar + c_skip_f M_af + M_d.  s within 64 u of the mean of |x| + M_r.  loss = mean(T) / s with T = (1 - alpha) delta^2 +
delta e, whose error per element is that of delta (16 u M_d) times its partners 2 |1 - alpha| |delta| + |e|, plus that of e
(16 u M_e) times |delta|: the magnitude of T is M_T = |1 - alpha| M_d (|delta| + 16 u M_d) + M_d (|e| + 16 u M_e) + M_e |delta|,
and loss is within (64 u mean(M_T) + |loss| 64 u mean(|x| + M_r)) / s, the second term being the relative error of s.  g of the
join within 16 u M / s + 64 u |g|, M = |d_dir| + |c_in_r g_r| + |c_in_f g_f|.  alpha is the fp32 operand the launch receives.
Parameter gradients of the shrunken nets: cosine >= 0.995 and norm within 5 %.  Per-sample loss of the shrunken nets against the
oracle: SID_LOSS_REL_BOUND, twice the worst value measured on an MI355X (SID_LOSS_REL_MEASURED; printed by the test), which may not
exceed the cap 0.30 (the accounting of test_hip_dm_train.py: each term a product of two differences of network outputs, over s).
dm_norm within 0.06."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ew_shapes import n_by_shape
from test_hip_dm_train import (DEV, FAKE_SCALE, GEN_SCALE, NET_Y, N_NET, PKG, S_NET, U, _cos, _diffusion, _flat, _oracle64, build, e,
                               scal64)

pytestmark = pytest.mark.gpu
ALPHAS = (1.0, 1.2)
SID_LOSS_REL_MEASURED = 2.786e-3    # worst per-sample relative error measured on an MI355X (alpha 1.2, gen_sigma 80; alpha 1.0: 2.767e-3;
                                    # gen_sigma 2.5: 1.342e-3 and 1.340e-3; dm_norm 4.525e-4 and 3.993e-4)
SID_LOSS_REL_BOUND = 2 * SID_LOSS_REL_MEASURED
SID_LOSS_REL_CAP = 0.30
SID_NORM_REL_BOUND = 0.06
# ladder indices of the oracle test: at the high levels test_hip_dm_train.py uses (1 and 4) the Jacobian paths contribute nothing
# measurable (cosine of the full gradient to the one without them 1.000 and 0.998); here the twin is far off (asserted below)
NET_IDX = (8, 9, 11, 12)
GEN_SIGMAS = (80.0, 2.5)
SENTINEL, PAD = -12345.5, 64


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def f32(v):
    return float(np.float32(v))


def operands(N, shape, seed, S):
    from models.cm.karras_diffusion import cd_levels
    gen = torch.Generator().manual_seed(seed)
    Fr, Ff, x, x_t, g_r, g_f = (torch.randn(N, *shape, generator=gen) for _ in range(6))
    idx = torch.randint(0, S, (N,), generator=gen)
    idx[0] = S - 1
    if N > 1:
        idx[1] = 0
    return Fr, Ff, x, x_t, g_r, g_f, idx, cd_levels(S, 0.002, 80.0, 7.0).table


def grad_ref64(Fr, Ff, x, x_t, t, alpha, sd_f=0.5, dist_f=False):
    """dxmi_sid_grad_fwd in float64 on fp32 operands -> {name: (value, bound)} (the bounds of the module docstring)."""
    a = f32(alpha)
    k_r, k_f = 2 * (1 - a), 2 * a - 1
    cs_r, co_r, _ = scal64(t, 0.5, False)
    cs_f, co_f, _ = scal64(t, sd_f, dist_f)
    Fr, Ff, x, x_t = (v.cpu().double() for v in (Fr, Ff, x, x_t))
    D_r, D_f = co_r * Fr + cs_r * x_t, co_f * Ff + cs_f * x_t
    M_r, M_f = (co_r * Fr).abs() + (cs_r * x_t).abs(), (co_f * Ff).abs() + (cs_f * x_t).abs()
    delta, M_d = D_r - D_f, M_r + M_f
    ex, M_e = D_f - x, M_f + x.abs()
    a_r, M_ar = k_r * delta + ex, abs(k_r) * M_d + M_e
    a_f, M_af = k_f * delta - ex, abs(k_f) * M_d + M_e
    mean = lambda v: v.mean(dim=[1, 2, 3])
    s, s_mag = mean((x - D_r).abs()), mean(x.abs() + M_r)
    T = (1 - a) * delta ** 2 + delta * ex
    M_T = abs(1 - a) * M_d * (delta.abs() + 16 * U * M_d) + M_d * (ex.abs() + 16 * U * M_e) + M_e * delta.abs()
    loss = mean(T) / s
    return {"v_r": (co_r * a_r, 16 * U * co_r.abs() * M_ar), "v_f": (co_f * a_f, 16 * U * co_f.abs() * M_af),
            "d_dir": (cs_r * a_r + cs_f * a_f - delta, 16 * U * (cs_r * M_ar + cs_f * M_af + M_d)),
            "s": (s, 64 * U * s_mag), "loss": (loss, (64 * U * mean(M_T) + loss.abs() * 64 * U * s_mag) / s)}


def join_ref64(d_dir, g_r, g_f, s, t, sd_f=0.5):
    ci_r, ci_f = scal64(t, 0.5)[2], scal64(t, sd_f)[2]
    d_dir, g_r, g_f = (v.cpu().double() for v in (d_dir, g_r, g_f))
    sd = e(s.cpu())
    g = (d_dir + ci_r * g_r + ci_f * g_f) / sd
    return g, 16 * U * (d_dir.abs() + (ci_r * g_r).abs() + (ci_f * g_f).abs()) / sd + 64 * U * g.abs()


def frac(got, ref, bound):
    return ((got.cpu().double() - ref).abs() / (bound + 1e-30)).max().item()


def kw_fake(sd_f, dist_f):
    return dict(sigma_data=sd_f, sigma_min=0.002, distillation=dist_f)


FAKES = ((0.5, False), (0.25, False), (0.5, True))


# ------------------------------------------------------------------------------------------ launches
@pytest.mark.parametrize("S", [2, 18])
@pytest.mark.parametrize("N,shape", n_by_shape([(3, 16, 16), (3, 12, 11), (3, 64, 64), (3, 80, 80)]))
def test_launches_vs_fp64(ops, shape, N, S):
    """3 x 64 x 64 is the largest image of the programs here, 3 x 80 x 80 lies above it (where dxmi_dm_grad_fwd changes kernels;
    the launch here is one pass at every size), 3 x 12 x 11 = 396 elements leaves a partly filled trip."""
    Fr, Ff, x, x_t, g_r, g_f, idx, tab = operands(N, shape, 41 + N + shape[1] + S, S)
    dev = [v.to(DEV).contiguous() for v in (Fr, Ff, x, x_t, idx, tab)]
    gr_d, gf_d = g_r.to(DEV), g_f.to(DEV)
    t = tab[idx]
    worst = {}
    for sd_f, dist_f in FAKES:
        for alpha in ALPHAS:
            v_r, v_f, d_dir, loss, s = ops.sid_grad_fwd(*dev, alpha, fake=kw_fake(sd_f, dist_f))
            ref = grad_ref64(Fr, Ff, x, x_t, t, alpha, sd_f, dist_f)
            for name, got in (("v_r", v_r), ("v_f", v_f), ("d_dir", d_dir), ("s", s), ("loss", loss)):
                f = frac(got, *ref[name])
                worst[name] = max(worst.get(name, 0.0), f)
                assert f <= 1, (name, sd_f, dist_f, alpha, f)
            g = ops.sid_join(d_dir, gr_d, gf_d, s, dev[4], dev[5], 0.5, sd_f)
            f = frac(g, *join_ref64(d_dir, g_r, g_f, s, t, sd_f))
            worst["g"] = max(worst.get("g", 0.0), f)
            assert f <= 1, ("g", sd_f, dist_f, alpha, f)
            before = d_dir.clone()
            assert ops.sid_join(d_dir, gr_d, gf_d, s, dev[4], dev[5], 0.5, sd_f, out=d_dir) is d_dir
            assert torch.equal(d_dir, g) and not torch.equal(before, g)                 # g aliasing d_dir: the same bits
    print(f"sid launches worst |err| / bound (shape {shape}, N {N}, S {S}): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def guarded(N, shape):
    n = N * int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf[PAD:PAD + n].view(N, *shape), buf


def untouched(buf):
    return bool((buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all())


@pytest.mark.parametrize("shape", [(3, 12, 11), (3, 64, 64), (3, 80, 80)])
def test_poisoned_index_sentinels_batch_split_and_reproducibility(ops, shape):
    N, S = 7, 18
    Fr, Ff, x, x_t, g_r, g_f, idx, tab = [v.to(DEV) for v in operands(N, shape, 3, S)]
    # the table sits at the start of a buffer of finite sentinels: a read past it would bring 1e30 into the result, not NaN
    wide = torch.full((S + 64,), 1e30, dtype=torch.float32, device=DEV)
    wide[:S] = tab
    tab = wide[:S]
    bad = idx.clone()
    bad[2], bad[5] = -1, S
    ok = torch.ones(N, dtype=torch.bool, device=DEV)
    ok[2] = ok[5] = False
    fake = kw_fake(0.25, False)
    clean = ops.sid_grad_fwd(Fr, Ff, x, x_t, idx, tab, 1.2, fake=fake)
    again = ops.sid_grad_fwd(Fr, Ff, x, x_t, idx, tab, 1.2, fake=fake)
    assert all(torch.equal(a, b) for a, b in zip(clean, again))                          # two runs, identical bits
    outs, bufs = zip(*[guarded(N, shape) for _ in range(3)] + [guarded(N, ()) for _ in range(2)])
    got = ops.sid_grad_fwd(Fr, Ff, x, x_t, bad, tab, 1.2, fake=fake, outs=outs)
    torch.cuda.synchronize()
    assert all(untouched(b) for b in bufs)
    for a, b in zip(got, clean):
        assert torch.isnan(a[~ok]).all() and torch.equal(a[ok], b[ok])
    # seven images in one launch are launches of three and four
    parts = [ops.sid_grad_fwd(Fr[r], Ff[r], x[r], x_t[r], idx[r].contiguous(), tab, 1.2, fake=fake) for r in (slice(0, 3), slice(3, 7))]
    assert all(torch.equal(torch.cat([p[k] for p in parts]), clean[k]) for k in range(5))
    # the join
    _, _, d_dir, _, s = clean
    g = ops.sid_join(d_dir, g_r, g_f, s, idx, tab, 0.5, 0.25)
    assert torch.equal(g, ops.sid_join(d_dir, g_r, g_f, s, idx, tab, 0.5, 0.25))
    gv, gb = guarded(N, shape)
    ops.sid_join(d_dir, g_r, g_f, s, bad, tab, 0.5, 0.25, out=gv)
    torch.cuda.synchronize()
    assert untouched(gb) and torch.isnan(gv[~ok]).all() and torch.equal(gv[ok], g[ok])
    parts = [ops.sid_join(d_dir[r], g_r[r], g_f[r], s[r].clone(), idx[r].contiguous(), tab, 0.5, 0.25) for r in (slice(0, 3), slice(3, 7))]
    assert torch.equal(torch.cat(parts), g)


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 64, 64), (3, 80, 80)])
def test_zero_normaliser_gives_zero_not_nan(ops, shape):
    N, S = 3, 18
    Fr, Ff, x, x_t, g_r, g_f, idx, tab = operands(N, shape, 5, S)
    Fr[1], x[1], x_t[1] = 0, 0, 0                # D_r = 0 = x: s == 0 for this sample alone
    dev = [v.to(DEV).contiguous() for v in (Fr, Ff, x, x_t, idx, tab)]
    for alpha in ALPHAS:
        v_r, v_f, d_dir, loss, s = ops.sid_grad_fwd(*dev, alpha)
        assert float(s[1]) == 0 and float(loss[1]) == 0 and (s[[0, 2]] > 0).all()
        assert all(torch.isfinite(v).all() for v in (v_r, v_f, d_dir, loss, s))
        g = ops.sid_join(d_dir, g_r.to(DEV), g_f.to(DEV), s, dev[4], dev[5])
        assert (g[1] == 0).all() and torch.isfinite(g).all() and (g[[0, 2]] != 0).any()


def test_wrappers_refuse_malformed_arguments(ops):
    from dxmi_hip import DxmiError
    Fr, Ff, x, x_t, g_r, g_f, idx, tab = [v.to(DEV) for v in operands(4, (3, 16, 16), 9, 18)]
    _, _, d_dir, _, s = ops.sid_grad_fwd(Fr, Ff, x, x_t, idx, tab)
    odd = torch.zeros(4, 3, 5, 5, device=DEV)
    off = torch.zeros(4 * 768 + 1, device=DEV)[1:].view(4, 3, 16, 16)
    bad_calls = [
        lambda: ops.sid_grad_fwd(Fr, Ff, x, x_t, idx, tab, float("nan")),
        lambda: ops.sid_grad_fwd(Fr, Ff, x, x_t, idx, tab, float("inf")),
        lambda: ops.sid_grad_fwd(Fr, Ff[:2], x, x_t, idx, tab),
        lambda: ops.sid_grad_fwd(Fr, Ff, x, None, idx, tab),
        lambda: ops.sid_grad_fwd(Fr, Ff, x, x_t, idx.cpu(), tab),
        lambda: ops.sid_grad_fwd(Fr, Ff, x, x_t, idx.int(), tab),
        lambda: ops.sid_grad_fwd(Fr, Ff, x, x_t, idx, tab[:1]),
        lambda: ops.sid_grad_fwd(Fr, Ff, x, off, idx, tab),
        lambda: ops.sid_grad_fwd(Fr.double(), Ff, x, x_t, idx, tab),
        lambda: ops.sid_grad_fwd(Fr, Ff, x, x_t, idx, tab, real=dict(sigma_data=0.0, sigma_min=0.002, distillation=False)),
        lambda: ops.sid_grad_fwd(odd, odd, odd, odd, idx, tab),
        lambda: ops.sid_join(d_dir, g_r, g_f, None, idx, tab),
        lambda: ops.sid_join(d_dir, g_r, g_f, s[:3], idx, tab),
        lambda: ops.sid_join(d_dir, g_r[:2], g_f, s, idx, tab),
        lambda: ops.sid_join(d_dir, g_r, g_f, s, idx, tab, fake_sigma_data=-0.5),
        lambda: ops.sid_join(d_dir, g_r, g_f, s, idx, tab, out=g_r),
        lambda: ops.sid_join(d_dir, g_r, g_f, s, idx, tab, out=off),
        lambda: ops.sid_join(odd, odd, odd, s, idx, tab),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"call {i} was accepted")


@pytest.mark.parametrize("plain", [False, True])
def test_input_vjp_is_input_forward_then_input_backward(ops, plain):
    from models.cm.unet_train import input_backward, input_forward, input_vjp
    from test_hip_cm_train import PLAIN
    net = build(PLAIN if plain else None, "", GEN_SCALE)
    net.train()
    gen = torch.Generator().manual_seed(17)
    x, v = torch.randn(2, 3, 16, 16, generator=gen).to(DEV), torch.randn(2, 3, 16, 16, generator=gen).to(DEV)
    t = torch.tensor([250 * math.log(0.7), 250 * math.log(9.0)], dtype=torch.float32, device=DEV)
    y = None if plain else torch.tensor([3, 871], device=DEV)
    F, g = input_vjp(net, x, t, v, y)
    F2, tape = input_forward(net, x, t, y)
    assert net.training                                            # the mode is restored between the halves
    g2 = input_backward(tape, v)
    assert torch.equal(F, F2) and torch.equal(g, g2) and g.abs().max() > 0
    assert all(p.grad is None for p in net.parameters())


# ------------------------------------------------------------------------------------------ the loss on the shrunken nets
def _net_operands():
    gen = torch.Generator().manual_seed(7)
    z, noise = torch.randn(N_NET, 3, 16, 16, generator=gen), torch.randn(N_NET, 3, 16, 16, generator=gen)
    return z, noise, torch.tensor(NET_IDX), torch.tensor(NET_Y)


def _oracle_sid(gen_sd, fake_sd, z, noise, idx, y, alpha, gen_sigma, jacobians=True):
    """sid_generator_losses on float64 oracle nets (the real net shares the generator's weights, as constants), the loss
    differentiated by autograd through x and, with jacobians=True, through both denoisers' inputs -> dict(loss, s, grads of
    loss.sum(), and the per-sample conditioning figures of the module docstring)."""
    from models.cm.karras_diffusion import cd_levels
    t = cd_levels(S_NET, 0.002, 80.0, 7.0).table.double()[idx]
    with _oracle64() as edm:
        from oracle import Precision
        cfg = edm.EDMConfig(image_size=16, model_channels=64, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2))

        def den(sd, x_t, s):
            cs, co, ci = scal64(s)
            return co * edm.unet_forward(sd, cfg, ci * x_t, 250 * torch.log(s), y=y, prec=Precision("fp32")) + cs * x_t
        leaves = {k: v.double().requires_grad_(True) for k, v in gen_sd.items()}
        real = {k: v.double() for k, v in gen_sd.items()}
        fake = {k: v.double() for k, v in fake_sd.items()}
        x = den(leaves, z.double() * gen_sigma, torch.full((len(z),), gen_sigma, dtype=torch.float64))
        x_t = x + noise.double() * e(t)
        fed = x_t if jacobians else x_t.detach()
        D_r, D_f = den(real, fed, t), den(fake, fed, t)
        s = (x - D_r).abs().mean(dim=[1, 2, 3]).detach()
        delta = D_r - D_f
        isum = lambda v: v.sum(dim=[1, 2, 3])
        A, B = (1 - alpha) * isum(delta ** 2), isum(delta * (D_f - x))
        loss = (A + B) / (x[0].numel() * s)
        grads = torch.autograd.grad(loss.sum(), list(leaves.values()))
    rms = lambda v: v.detach().pow(2).mean(dim=[1, 2, 3]).sqrt()
    return dict(loss=loss.detach(), s=s, grads=dict(zip(leaves, grads)),
                sep_g=(rms(D_f - D_r) / torch.maximum(rms(D_f), rms(D_r))).min().item(),
                sep_s=(s / torch.maximum(rms(x), rms(D_r))).min().item(),
                sep_x=(rms(D_f - x) / torch.maximum(rms(D_f), rms(x))).min().item(),
                no_cancel=((A + B).abs() / (A.abs() + isum((delta * (D_f - x)).abs()))).detach().min().item())


@pytest.fixture(scope="module")
def nets():
    gen_net, real, fake = build(None, "", GEN_SCALE), build(None, "", GEN_SCALE), build(None, "fake:", FAKE_SCALE)
    for p in gen_net.parameters():
        p.requires_grad_(True)
    return gen_net, real, fake


@pytest.mark.parametrize("gen_sigma", GEN_SIGMAS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_sid_generator_losses_vs_fp64_oracle(ops, nets, alpha, gen_sigma):
    gen_net, real, fake = nets
    z, noise, idx, y = _net_operands()
    gen_sd = {k: v.detach().cpu() for k, v in gen_net.state_dict().items()}
    fake_sd = {k: v.detach().cpu() for k, v in fake.state_dict().items()}
    ref = _oracle_sid(gen_sd, fake_sd, z, noise, idx, y, alpha, gen_sigma)
    twin = _oracle_sid(gen_sd, fake_sd, z, noise, idx, y, alpha, gen_sigma, jacobians=False)
    compared = [n for n, rg in ref["grads"].items() if rg.norm() >= 1e-6 * max(1.0, twin["grads"][n].norm().item())]
    twin_cos = max(_cos(twin["grads"][n], ref["grads"][n]) for n in compared)
    print(f"alpha {alpha}, gen_sigma {gen_sigma}: oracle: the twin without Jacobian paths has per-parameter cosine <= {twin_cos:.3f}; "
          f"rms(D_f - D_r) / max rms >= {ref['sep_g']:.3f}, mean|x - D_r| / max rms >= {ref['sep_s']:.3f}, rms(D_f - x) / max rms >= "
          f"{ref['sep_x']:.3f}, |A + B| / (|A| + sum|delta (D_f - x)|) >= {ref['no_cancel']:.3f}")
    # on the oracle alone: the test cannot pass without the Jacobian paths, and the loss is no small difference of large numbers
    assert twin_cos <= 0.95
    assert ref["sep_g"] >= 0.5 and ref["sep_s"] >= 0.5 and ref["sep_x"] >= 0.5 and ref["no_cancel"] >= 0.5
    d = _diffusion()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, model_kwargs={"y": y.to(DEV)}, noise=noise.to(DEV),
              indices=idx.to(DEV), gen_sigma=gen_sigma, alpha=alpha)
    gen_net.zero_grad()
    t = d.sid_generator_losses(gen_net, z.to(DEV), S_NET, **kw)
    assert set(t) == {"loss", "x", "dm_norm"} and t["loss"].requires_grad and not t["x"].requires_grad
    t["loss"].sum().backward()
    rel = ((t["loss"].detach().cpu().double() - ref["loss"]).abs() / ref["loss"].abs()).max().item()
    rel_s = ((t["dm_norm"].cpu().double() - ref["s"]).abs() / ref["s"]).max().item()
    P = dict(gen_net.named_parameters())
    wc, wn = ("", 1.0), ("", 0.0)
    for n in compared:
        got, rg = P[n].grad.cpu(), ref["grads"][n]
        wc = min(wc, (n, _cos(got, rg)), key=lambda v: v[1])
        wn = max(wn, (n, abs((got.double().norm() / rg.norm()).item() - 1)), key=lambda v: v[1])
    print(f"alpha {alpha}, gen_sigma {gen_sigma}: device: per-sample loss worst relative error {rel:.3e} (bound {SID_LOSS_REL_BOUND}, cap "
          f"{SID_LOSS_REL_CAP}); dm_norm {rel_s:.3e} (bound {SID_NORM_REL_BOUND}); gradient worst cosine {wc[1]:.5f} ({wc[0]}), worst "
          f"norm ratio deviation {wn[1]:.4f} ({wn[0]})")
    assert all(p.grad is None for net in (real, fake) for p in net.parameters())
    with torch.no_grad():                            # no node: forward_inference everywhere, only loss, x and s
        again = d.sid_generator_losses(gen_net, z.to(DEV), S_NET, **kw)
    assert not again["loss"].requires_grad and torch.equal(again["x"], t["x"]) and torch.equal(again["dm_norm"], t["dm_norm"])
    assert wc[1] >= 0.995 and wn[1] <= 0.05
    assert SID_LOSS_REL_BOUND <= SID_LOSS_REL_CAP
    assert rel <= SID_LOSS_REL_BOUND and rel_s <= SID_NORM_REL_BOUND


@pytest.mark.parametrize("sd_f", [0.5, 0.25])
def test_device_node_vs_torch_fallback_on_the_same_nets(ops, nets, sd_f):
    """Wrapped in plain callables the same HIP nets take the torch fallback.  The launch chain of the no-grad path is run here by
    hand too, which exposes its operands: both paths are held to the launch bounds against float64 on those operands, and they
    agree in x bitwise.

    The node gives both denoisers the time 250 ln(t + 1e-44) by the torch expression of denoise() on the device (it does not take
    the one dxmi_dm_gen_prep writes: that logf and torch.log differ in the last bit at the ladder indices 9, 11 and 12, and the
    bf16 nets turn one ulp of time into 6e-4 of the loss, 28 times the launch bound, measured before the node did so); the hand
    chain below does the same, so the networks of both paths see bitwise the same inputs."""
    from models.cm.karras_diffusion import cd_levels
    gen_net, real, fake = nets
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    d, fd = _diffusion(), _diffusion(sigma_data=sd_f)
    tab = cd_levels(S_NET, 0.002, 80.0, 7.0).device_table(torch.device(DEV))
    wrap = lambda net: (lambda x_in, t, **kw: net(x_in, t, **kw))
    figures = []
    for alpha in ALPHAS:
        kw = dict(real_diffusion=_diffusion(), fake_diffusion=fd, model_kwargs={"y": y}, noise=noise, indices=idx, alpha=alpha)
        with torch.no_grad():
            node = d.sid_generator_losses(gen_net, z, S_NET, real_model=real, fake_model=fake, **kw)
            fb = d.sid_generator_losses(wrap(gen_net), z, S_NET, real_model=wrap(real), fake_model=wrap(fake), **kw)
            x_in, tg = ops.dm_gen_in(z, 80.0, 0.5)
            x, x_t, xr, _, xf = ops.dm_gen_prep(gen_net.forward_inference(x_in, tg, y), z, noise, idx, tab, 80.0, 0.5, 0.5, sd_f)
            tm = 1000 * 0.25 * torch.log(tab[idx] + 1e-44)
            F_r, F_f = real.forward_inference(xr, tm, y), fake.forward_inference(xr if xf is None else xf, tm, y)
            _, _, _, loss, s = ops.sid_grad_fwd(F_r, F_f, x, x_t, idx, tab, alpha, fake=kw_fake(sd_f, False))
        assert torch.equal(node["loss"], loss) and torch.equal(node["dm_norm"], s) and torch.equal(node["x"], x)
        assert torch.equal(fb["x"], x)                               # the two paths agree in x bitwise
        ref = grad_ref64(F_r, F_f, x, x_t, tab.cpu()[idx.cpu()], alpha, sd_f)
        rel = ((fb["loss"] - node["loss"]).abs() / node["loss"].abs()).max().item()
        for name, t in (("node", node), ("fallback", fb)):
            el, es = frac(t["loss"], *ref["loss"]), frac(t["dm_norm"], *ref["s"])
            print(f"{name} (alpha {alpha}, fake sigma_data {sd_f}) |err| / launch bound: loss {el:.3f}, dm_norm {es:.3f}; "
                  f"fallback against node, relative: {rel:.2e}")
            figures.append((name, alpha, el, es))
    assert all(el <= 1 and es <= 1 for _, _, el, es in figures), figures


@pytest.mark.parametrize("sd_f", [0.5, 0.25])
def test_torch_fallback_vs_fp64_on_its_own_operands(ops, nets, sd_f):
    """The torch fallback on the HIP nets, with hooks on the three nets that keep what each was given and what it returned: x, the
    networks' inputs, dm_norm and loss are held to the launch bounds against float64 on the network outputs the fallback itself
    received, whichever time its networks were given (the test above relies on both paths forming it alike)."""
    from models.cm.karras_diffusion import cd_levels
    gen_net, real, fake = nets
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    d, fd = _diffusion(), _diffusion(sigma_data=sd_f)
    tab = cd_levels(S_NET, 0.002, 80.0, 7.0).device_table(torch.device(DEV))
    t = tab.cpu()[idx.cpu()]
    seen = {}
    hooks = [net.register_forward_hook(lambda m, a, kw, out, k=k: seen.__setitem__(k, (a[0].clone(), a[1].clone(), out.clone())), with_kwargs=True)
             for k, net in (("gen", gen_net), ("real", real), ("fake", fake))]
    wrap = lambda net: (lambda x_in, tt, **kw: net(x_in, tt, **kw))
    try:
        for alpha in ALPHAS:
            with torch.no_grad():
                fb = d.sid_generator_losses(wrap(gen_net), z, S_NET, real_model=wrap(real), real_diffusion=_diffusion(), fake_model=wrap(fake),
                                            fake_diffusion=fd, model_kwargs={"y": y}, noise=noise, indices=idx, alpha=alpha)
                x, x_t, xr, tm, xf = ops.dm_gen_prep(seen["gen"][2], z, noise, idx, tab, 80.0, 0.5, 0.5, sd_f)
            assert torch.equal(fb["x"], x) and torch.equal(seen["real"][0], xr) and torch.equal(seen["fake"][0], xr if xf is None else xf)
            assert torch.equal(seen["real"][1], seen["fake"][1]) and ((seen["real"][1] - tm).abs() <= 16 * U * tm.abs()).all()
            ref = grad_ref64(seen["real"][2], seen["fake"][2], x, x_t, t, alpha, sd_f)
            el, es = frac(fb["loss"], *ref["loss"]), frac(fb["dm_norm"], *ref["s"])
            _, _, _, loss, s = ops.sid_grad_fwd(seen["real"][2], seen["fake"][2], x, x_t, idx, tab, alpha, fake=kw_fake(sd_f, False))
            print(f"fallback on its own operands (alpha {alpha}, fake sigma_data {sd_f}) |err| / launch bound: loss {el:.3f}, dm_norm {es:.3f}; "
                  f"the launch on the same operands: loss {frac(loss, *ref['loss']):.3f}, dm_norm {frac(s, *ref['s']):.3f}")
            assert el <= 1 and es <= 1, (alpha, el, es)
            assert frac(loss, *ref["loss"]) <= 1 and frac(s, *ref["s"]) <= 1
    finally:
        for h in hooks:
            h.remove()


def test_hip_refusals(ops):
    gen_net, real, fake = build(), build(), build(None, "fake:")
    plain = build(dict(class_cond=False))
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    d = _diffusion()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        d.sid_generator_losses(gen_net, z.clone().requires_grad_(True), S_NET, model_kwargs={"y": y}, **kw)
    with pytest.raises(NotImplementedError, match="not inputs of UNetModel"):
        d.sid_generator_losses(gen_net, z, S_NET, model_kwargs={"y": y, "w": 1}, **kw)
    with pytest.raises(ValueError, match="class-conditional"):
        d.sid_generator_losses(gen_net, z, S_NET, **kw)
    with pytest.raises(ValueError, match="class-conditional"):
        d.sid_generator_losses(gen_net, z, S_NET, model_kwargs={"y": y}, **dict(kw, fake_model=plain))
    with pytest.raises(NotImplementedError, match="distillation=False"):
        _diffusion(distillation=True).sid_generator_losses(gen_net, z, S_NET, model_kwargs={"y": y}, **kw)
    with pytest.raises(ValueError, match="alpha"):
        d.sid_generator_losses(gen_net, z, S_NET, model_kwargs={"y": y}, alpha=float("nan"), **kw)


# ------------------------------------------------------------------------------------------ DMTrainLoop
LOOP_ITERS, LOOP_EVERY = 3, 2


def _run(tl, k, z):
    torch.manual_seed(1000 + k)
    return tl.run_step(z[k].to(DEV), {})


@pytest.mark.parametrize("use_fp16", [True, False])
def test_dmtrainloop_sid_on_the_device(ops, tmp_path, use_fp16):
    """Three iterations, generator turns at 0 and 2: the generator moves on its turns only, the teacher stays bitwise and is left
    without gradients, and a loop resumed from the save after iteration 1 repeats iteration 2 bit for bit."""
    from test_hip_dm_train import _loop
    gen = torch.Generator().manual_seed(99)
    z = [torch.randn(4, 3, 16, 16, generator=gen) for _ in range(LOOP_ITERS)]
    over = dict(objective="sid", sid_alpha=1.2, gen_sigma=2.5, gen_update_every=LOOP_EVERY)
    tl = _loop(tmp_path, use_fp16, **over)
    probe = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    pt = torch.tensor([1.5, -2.0], device=DEV)
    teacher_out = tl.real_model.forward_inference(probe, pt).clone()
    teacher_w = _flat(tl.real_model.parameters()).clone()
    gens, fakes, lg = {}, {}, None
    g_prev, f_prev = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
    for k in range(LOOP_ITERS):
        took_gen, took_fake = _run(tl, k, z)
        on = k % LOOP_EVERY == 0
        assert took_gen == on and took_fake, k
        gens[k], fakes[k] = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
        assert torch.equal(gens[k], g_prev) != on and not torch.equal(fakes[k], f_prev), k
        assert torch.equal(_flat(tl.real_model.parameters()), teacher_w), k
        assert torch.equal(tl.real_model.forward_inference(probe, pt), teacher_out), k
        assert all(p.grad is None for p in tl.real_model.parameters()), k
        assert tl.fake_model.training and tl.model.training                     # input_forward restored the fake net's mode
        g_prev, f_prev = gens[k], fakes[k]
        if tl.step == 2:
            tl.save()
            lg = (tl.mp_trainer.lg_loss_scale, tl.fake_trainer.lg_loss_scale)
    row = tl.dumpkvs()
    assert all(math.isfinite(row[k]) for k in ("loss", "dm_norm", "fake_mse"))
    tr = _loop(tmp_path, use_fp16, resume=str(tmp_path / "model000002.pt"), **over)
    assert tr.step == 2 and torch.equal(_flat(tr.model.parameters()), gens[1]) and torch.equal(_flat(tr.fake_model.parameters()), fakes[1])
    tr.mp_trainer.lg_loss_scale, tr.fake_trainer.lg_loss_scale = lg          # the loss scales are not checkpointed
    _run(tr, 2, z)
    assert torch.equal(_flat(tr.model.parameters()), gens[2]) and torch.equal(_flat(tr.fake_model.parameters()), fakes[2])


# ------------------------------------------------------------------------------------------ command line
def test_cli_cm_train_sid_then_sample(ops, tmp_path):
    """cm_train.py --training_mode dm --dm_objective sid --gen_sigma 2.5 for 2 iterations on a shrunken config, then
    generate_large.py --karras_sampler dm --gen_sigma 2.5 on the generator it wrote: NFE = 1."""
    from test_hip_cm_train import TINY_KW
    shrunk = dict(image_size=16, num_channels=64, num_res_blocks=1, channel_mult="1,2", attention_resolutions="8", num_head_channels=64,
                  class_cond=True, resblock_updown=True)
    args = [a for k, v in shrunk.items() for a in (f"--{k}", str(v))]
    over = dict(TINY_KW, **shrunk)
    teacher = build(over, "teacher:", GEN_SCALE)
    torch.save(teacher.state_dict(), tmp_path / "teacher.pt")
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1", RANK="0")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "cm_train.py", "--training_mode", "dm", "--dm_objective", "sid",
                        "--gen_sigma", "2.5", "--teacher_model_path", str(tmp_path / "teacher.pt"), "--max_iters", "2", "--batch_size", "4",
                        "--microbatch", "2", "--use_fp16", "True", "--gen_update_every", "1", "--dm_num_scales", "18", "--save_interval",
                        "2", "--log_interval", "1", "--ema_rate", "0.999", "--lr", "1e-4", "--log_dir", str(tmp_path / "run")] + args,
                       cwd=PKG, env=env, capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "objective sid (alpha 1.2), gen_sigma 2.5" in r.stdout, r.stdout[-2000:]
    files = set(os.listdir(tmp_path / "run"))
    assert {"model000002.pt", "ema_0.999_000002.pt", "opt000002.pt", "fake_model000002.pt", "fake_opt000002.pt", "progress.jsonl"} <= files, files
    student = torch.load(tmp_path / "run" / "model000002.pt", map_location=DEV)
    te = teacher.state_dict()
    assert all(torch.isfinite(v).all() for v in student.values())
    # iteration 0 meets fake == real (delta = 0: no gradient, loss 0); iteration 1 meets a trained fake net and moves the generator
    assert any(not torch.equal(student[k], te[k]) for k in te)
    rows = [json.loads(l) for l in open(tmp_path / "run" / "progress.jsonl")]
    assert len(rows) == 2 and all(math.isfinite(r_[k]) for r_ in rows for k in ("loss", "dm_norm", "fake_mse"))
    assert rows[0]["loss"] == 0 and rows[1]["loss"] != 0 and all(r_["dm_norm"] > 0 for r_ in rows)

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
