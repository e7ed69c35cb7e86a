"""Distribution matching distillation on the GPU: the five launches of csrc/dm_train.hip against float64 on the same fp32 operands,
KarrasDenoiser.dm_generator_losses on the shrunken HIP U-Nets against float64 oracle nets, DMTrainLoop's two clocks with save /
resume, dm_sample, and the two command lines.

Bounds (the project's, as test_hip_pd_train.py writes them out): an elementwise result within 16 u M of float64 (u = 2^-24, M the
magnitude of the operands that meet in it); s and loss within 64 u of the mean of their terms' magnitudes; g under the "dmd"
weighting additionally carries the relative error of s: 16 u M_g / s + 64 u |g|.  Parameter gradients of the shrunken nets: cosine >=
0.995 and norm within 5 %.  Per-sample loss of the shrunken nets against the oracle: DM_LOSS_REL_BOUND, twice the worst value
measured on an MI355X (DM_LOSS_REL_MEASURED; printed by the test); it may not exceed the cap 0.30 = 2 (the square) x 5
network operands (three in D_f - D_r, two in s) x 1.5e-2 (the bound the shrunken net's forward is held to) / 0.5 (the separation
ratio asserted below).  dm_norm = s has two network operands and no square: within 2 x 1.5e-2 / 0.5 = 0.06."""
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
SMIN = float(np.float32(0.002))
DM_LOSS_REL_MEASURED = 3.517e-3     # worst per-sample relative error measured on an MI355X (dmd; none 3.458e-3; dm_norm 8.528e-4)
DM_LOSS_REL_BOUND = 2 * DM_LOSS_REL_MEASURED
DM_LOSS_REL_CAP = 2 * 5 * 1.5e-2 / 0.5
DM_NORM_REL_BOUND = 2 * 1.5e-2 / 0.5
assert DM_LOSS_REL_BOUND <= DM_LOSS_REL_CAP == 0.30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffusion-by-maxentirl_amd")
WEIGHTINGS = ("dmd", "none")
GEN_SIGMA = 80.0


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def build(over=None, salt="", out_scale=1.0, **kw2):
    from test_hip_cm_train import build as b
    return b(over, salt, out_scale, **kw2)


def e(v):
    return v.double()[:, None, None, None]


def scal64(s, sd=0.5, distill=False):
    s = s.double()
    if distill:
        c_skip, c_out = sd ** 2 / ((s - SMIN) ** 2 + sd ** 2), (s - SMIN) * sd / (s ** 2 + sd ** 2) ** 0.5
    else:
        c_skip, c_out = sd ** 2 / (s ** 2 + sd ** 2), s * sd / (s ** 2 + sd ** 2) ** 0.5
    return e(c_skip), e(c_out), e(1 / (s ** 2 + sd ** 2) ** 0.5)


def close(got, ref, M, k=16, floor=1e-30):
    return ((got.cpu().double() - ref).abs() <= k * U * M + floor).all()


def ratio(got, ref, M, k=16, floor=1e-30):
    return ((got.cpu().double() - ref).abs() / (k * U * M + floor)).max().item()


def operands(N, shape, seed, S):
    from models.cm.karras_diffusion import cd_levels
    gen = torch.Generator().manual_seed(seed)
    z, noise, Fg, Fr, Ff = (torch.randn(N, *shape, generator=gen) for _ in range(5))
    idx = torch.randint(0, S, (N,), generator=gen)
    idx[0] = S - 1                       # legal here: only t is gathered
    if N > 1:
        idx[1] = 0
    return z, noise, Fg, Fr, Ff, idx, cd_levels(S, 0.002, 80.0, 7.0).table


def grad_ref64(Fr, Ff, x, x_t, t, weighting, sd_r=0.5, sd_f=0.5, dist_r=False, dist_f=False):
    """dxmi_dm_grad_fwd in float64 on fp32 operands -> (g, loss, s, bound of g, bound of loss, bound of s)."""
    cs_r, co_r, _ = scal64(t, sd_r, dist_r)
    cs_f, co_f, _ = scal64(t, sd_f, dist_f)
    Fr, Ff, x, x_t = (v.cpu().double() for v in (Fr, Ff, x, x_t))
    D_r, D_f = co_r * Fr + cs_r * x_t, co_f * Ff + cs_f * x_t
    M_r, M_f = (co_r * Fr).abs() + (cs_r * x_t).abs(), (co_f * Ff).abs() + (cs_f * x_t).abs()
    s = (x - D_r).abs().mean(dim=[1, 2, 3])
    b_s = 64 * U * (x.abs() + M_r).mean(dim=[1, 2, 3])
    g, M_g = D_f - D_r, M_r + M_f
    if weighting == "dmd":
        g = g / e(s)
        b_g = 16 * U * M_g / e(s) + 64 * U * g.abs()
    else:
        b_g = 16 * U * M_g
    g = torch.where(e(s) == 0, torch.zeros_like(g), g)
    loss = 0.5 * (g ** 2).mean(dim=[1, 2, 3])
    b_l = 64 * U * ((b_g / (16 * U)) * (g.abs() + b_g)).mean(dim=[1, 2, 3])
    return g, loss, s, b_g, b_l, b_s


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("S", [2, 18])
@pytest.mark.parametrize("N,shape", n_by_shape([(3, 16, 16), (3, 12, 11), (3, 64, 64)]))
@pytest.mark.parametrize("sd_f", [0.5, 0.25])
def test_kernels_vs_fp64(ops, shape, N, S, sd_f):
    z, noise, Fg, Fr, Ff, idx, tab = operands(N, shape, 31 + N + shape[1] + S, S)
    d = lambda v: v.to(DEV).contiguous()
    t = tab[idx]
    sg = torch.full((N,), GEN_SIGMA)
    cs_g, co_g, ci_g = scal64(sg)
    xT = z.double() * GEN_SIGMA
    worst = {}
    # gen_in
    x_in, tm = ops.dm_gen_in(d(z), GEN_SIGMA, 0.5)
    worst["gen_in"] = ratio(x_in, ci_g * xT, ci_g * xT.abs())
    assert close(x_in, ci_g * xT, ci_g * xT.abs())
    assert ((tm.cpu().double() - 250 * math.log(GEN_SIGMA)).abs() <= 16 * U * 250 * math.log(GEN_SIGMA) + 1e-4).all()
    # gen_out
    ref_x, M_x = co_g * Fg.double() + cs_g * xT, (co_g * Fg.double()).abs() + (cs_g * xT).abs()
    x_plain = ops.dm_gen_out(d(Fg), d(z), GEN_SIGMA, 0.5, clip=False)
    x_clip = ops.dm_gen_out(d(Fg), d(z), GEN_SIGMA, 0.5, clip=True)
    worst["gen_out"] = ratio(x_plain, ref_x, M_x)
    assert close(x_plain, ref_x, M_x) and close(x_clip, ref_x.clamp(-1, 1), M_x)
    assert x_clip.min() >= -1 and x_clip.max() <= 1 and (ref_x.abs() > 1).any()         # the clamp had something to do
    assert torch.equal(x_clip, x_plain.clamp(-1, 1))
    # gen_prep
    x, x_t, xr_in, tm, xf_in = ops.dm_gen_prep(d(Fg), d(z), d(noise), d(idx), d(tab), GEN_SIGMA, 0.5, 0.5, sd_f)
    assert torch.equal(x, x_plain)
    assert (xf_in is None) == (sd_f == 0.5)
    xd, xtd = x.cpu().double(), x_t.cpu().double()
    worst["x_t"] = ratio(x_t, xd + noise.double() * e(t), xd.abs() + (noise.double() * e(t)).abs())
    assert close(x_t, xd + noise.double() * e(t), xd.abs() + (noise.double() * e(t)).abs())
    ci_r = scal64(t, 0.5)[2]
    assert close(xr_in, ci_r * xtd, ci_r * xtd.abs())
    if xf_in is not None:
        ci_f = scal64(t, sd_f)[2]
        assert close(xf_in, ci_f * xtd, ci_f * xtd.abs()) and not torch.equal(xf_in, xr_in)
    assert ((tm.cpu().double() - 250 * torch.log(t.double())).abs() <= 16 * U * 250 * torch.log(t.double()).abs() + 1e-4).all()
    # grad_fwd and gen_bwd on the x, x_t the kernel wrote
    up = torch.randn(N, generator=torch.Generator().manual_seed(N + S))
    for weighting in WEIGHTINGS:
        for dist_f in (False, True):
            g, loss, s = ops.dm_grad_fwd(d(Fr), d(Ff), x, x_t, d(idx), d(tab), weighting, real=dict(sigma_data=0.5, sigma_min=0.002, distillation=False),
                                         fake=dict(sigma_data=sd_f, sigma_min=0.002, distillation=dist_f))
            rg, rl, rs, b_g, b_l, b_s = grad_ref64(Fr, Ff, x, x_t, t, weighting, 0.5, sd_f, False, dist_f)
            eg = ((g.cpu().double() - rg).abs() / (b_g + 1e-30)).max().item()
            el = ((loss.cpu().double() - rl).abs() / (b_l + 1e-30)).max().item()
            es = ((s.cpu().double() - rs).abs() / (b_s + 1e-30)).max().item()
            for k, v in ((f"g.{weighting}", eg), (f"loss.{weighting}", el), ("s", es)):
                worst[k] = max(worst.get(k, 0.0), v)
            assert eg <= 1 and el <= 1 and es <= 1, (weighting, dist_f, eg, el, es)
        dF = ops.dm_gen_bwd(d(up), g, GEN_SIGMA, 0.5)
        gd = g.cpu().double()
        ref_dF = e(up) / gd[0].numel() * gd * co_g
        worst["gen_bwd"] = max(worst.get("gen_bwd", 0.0), ratio(dF, ref_dF, ref_dF.abs(), floor=1e-38))
        assert close(dF, ref_dF, ref_dF.abs(), floor=1e-38)
    print(f"dm kernels worst |err| / bound (shape {shape}, N {N}, S {S}, fake sigma_data {sd_f}): "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_grad_fwd_above_the_register_budget(ops, weighting):
    """3 x 80 x 80 = 19200 elements per image: above the 12288 the one-pass kernel keeps in registers, so the two-pass kernel runs;
    3 x 64 x 64 and 3 x 16 x 16 above are the two one-pass instantiations."""
    shape, N, S = (3, 80, 80), 2, 18
    assert 3 * 80 * 80 > ops.DM_REG_CHW >= 3 * 64 * 64
    z, noise, Fg, Fr, Ff, idx, tab = operands(N, shape, 77, S)
    d = lambda v: v.to(DEV).contiguous()
    x, x_t, _, _, _ = ops.dm_gen_prep(d(Fg), d(z), d(noise), d(idx), d(tab), GEN_SIGMA, 0.5, 0.5, 0.25)
    g, loss, s = ops.dm_grad_fwd(d(Fr), d(Ff), x, x_t, d(idx), d(tab), weighting, fake=dict(sigma_data=0.25, sigma_min=0.002, distillation=False))
    rg, rl, rs, b_g, b_l, b_s = grad_ref64(Fr, Ff, x, x_t, tab[idx], weighting, 0.5, 0.25)
    eg = ((g.cpu().double() - rg).abs() / b_g).max().item()
    el, es = ((loss.cpu().double() - rl).abs() / b_l).max().item(), ((s.cpu().double() - rs).abs() / b_s).max().item()
    print(f"dm grad_fwd two-pass ({weighting}) worst |err| / bound: g {eg:.3f}, loss {el:.3f}, s {es:.3f}")
    assert eg <= 1 and el <= 1 and es <= 1
    g2, loss2, s2 = ops.dm_grad_fwd(d(Fr), d(Ff), x, x_t, d(idx), d(tab), weighting, fake=dict(sigma_data=0.25, sigma_min=0.002, distillation=False))
    assert torch.equal(g, g2) and torch.equal(loss, loss2) and torch.equal(s, s2)


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 64, 64), (3, 80, 80)])
def test_zero_normaliser_gives_zero_not_nan(ops, shape):
    N, S = 3, 18
    _, _, _, Fr, Ff, idx, tab = operands(N, shape, 5, S)
    x, x_t = torch.randn(N, *shape), torch.randn(N, *shape)
    Fr[1], x[1], x_t[1] = 0, 0, 0                # D_r = 0 = x: s == 0 for this sample alone
    dev = [v.to(DEV).contiguous() for v in (Fr, Ff, x, x_t, idx, tab)]
    for weighting in WEIGHTINGS:
        g, loss, s = ops.dm_grad_fwd(*dev, weighting)
        assert float(s[1]) == 0 and float(loss[1]) == 0 and (g[1] == 0).all()
        assert torch.isfinite(g).all() and torch.isfinite(loss).all() and torch.isfinite(s).all()
        assert (s[[0, 2]] > 0).all() and (loss[[0, 2]] > 0).all()


def test_index_guard_reproducibility(ops):
    N, S, shape = 16, 18, (3, 64, 64)
    z, noise, Fg, Fr, Ff, idx, tab = [v.to(DEV) for v in operands(N, shape, 3, S)]
    bad = idx.clone()
    bad[3], bad[9] = -1, S
    ok = torch.ones(N, dtype=torch.bool, device=DEV)
    ok[3] = ok[9] = False
    clean = ops.dm_gen_prep(Fg, z, noise, idx, tab, GEN_SIGMA, 0.5, 0.5, 0.25)
    again = ops.dm_gen_prep(Fg, z, noise, idx, tab, GEN_SIGMA, 0.5, 0.5, 0.25)
    assert all(torch.equal(a, b) for a, b in zip(clean, again))                    # two calls, identical bits
    guarded = ops.dm_gen_prep(Fg, z, noise, bad, tab, GEN_SIGMA, 0.5, 0.5, 0.25)
    assert torch.equal(guarded[0], clean[0])                                       # x needs no level
    for a, b in zip(guarded[1:], clean[1:]):
        assert torch.isnan(a[~ok]).all() and torch.equal(a[ok], b[ok])
    x, x_t = clean[0], clean[1]
    for weighting in WEIGHTINGS:
        c = ops.dm_grad_fwd(Fr, Ff, x, x_t, idx, tab, weighting)
        c2 = ops.dm_grad_fwd(Fr, Ff, x, x_t, idx, tab, weighting)
        assert all(torch.equal(a, b) for a, b in zip(c, c2))
        gd = ops.dm_grad_fwd(Fr, Ff, x, x_t, bad, tab, weighting)
        for a, b in zip(gd, c):
            assert torch.isnan(a[~ok]).all() and torch.equal(a[ok], b[ok])
        up = torch.rand(N, device=DEV)
        assert torch.equal(ops.dm_gen_bwd(up, c[0], GEN_SIGMA), ops.dm_gen_bwd(up, c[0], GEN_SIGMA))
    assert all(torch.equal(a, b) for a, b in zip(ops.dm_gen_in(z, GEN_SIGMA), ops.dm_gen_in(z, GEN_SIGMA)))


def test_wrappers_refuse_malformed_arguments(ops):
    from dxmi_hip import DxmiError
    z, noise, Fg, Fr, Ff, idx, tab = [v.to(DEV) for v in operands(4, (3, 16, 16), 9, 18)]
    x, x_t = ops.dm_gen_prep(Fg, z, noise, idx, tab, GEN_SIGMA)[:2]
    up = torch.ones(4, device=DEV)
    odd = torch.zeros(4, 3, 5, 5, device=DEV)                       # 75 elements per sample: no multiple of 4
    off = torch.zeros(4 * 768 + 1, device=DEV)[1:].view(4, 3, 16, 16)      # 4 bytes past a 16-byte boundary
    bad_calls = [
        lambda: ops.dm_gen_in(z.double(), GEN_SIGMA),
        lambda: ops.dm_gen_in(z.cpu(), GEN_SIGMA),
        lambda: ops.dm_gen_in(odd, GEN_SIGMA),
        lambda: ops.dm_gen_in(off, GEN_SIGMA),
        lambda: ops.dm_gen_in(z, 0.0),
        lambda: ops.dm_gen_in(z, GEN_SIGMA, sigma_data=-0.5),
        lambda: ops.dm_gen_in(None, GEN_SIGMA),
        lambda: ops.dm_gen_out(Fg, z[:2], GEN_SIGMA),
        lambda: ops.dm_gen_out(Fg, None, GEN_SIGMA),
        lambda: ops.dm_gen_out(Fg, z, float("nan")),
        lambda: ops.dm_gen_out(Fg.permute(0, 1, 3, 2), z, GEN_SIGMA),
        lambda: ops.dm_gen_prep(Fg, z, noise[:3], idx, tab, GEN_SIGMA),
        lambda: ops.dm_gen_prep(Fg, z, None, idx, tab, GEN_SIGMA),
        lambda: ops.dm_gen_prep(Fg, z, noise, idx.int(), tab, GEN_SIGMA),
        lambda: ops.dm_gen_prep(Fg, z, noise, idx[:3], tab, GEN_SIGMA),
        lambda: ops.dm_gen_prep(Fg, z, noise, idx, tab[:1], GEN_SIGMA),
        lambda: ops.dm_gen_prep(Fg, z, noise, idx, tab.double(), GEN_SIGMA),
        lambda: ops.dm_gen_prep(Fg, z, noise, idx, tab, GEN_SIGMA, fake_sigma_data=0.0),
        lambda: ops.dm_gen_prep(odd, odd, odd, idx, tab, GEN_SIGMA),
        lambda: ops.dm_grad_fwd(Fr, Ff, x, x_t, idx, tab, "snr"),
        lambda: ops.dm_grad_fwd(Fr, Ff[:2], x, x_t, idx, tab),
        lambda: ops.dm_grad_fwd(Fr, Ff, x, None, idx, tab),
        lambda: ops.dm_grad_fwd(Fr, Ff, x, x_t, idx.cpu(), tab),
        lambda: ops.dm_grad_fwd(Fr, Ff, x, x_t, idx, tab, real=dict(sigma_data=0.0, sigma_min=0.002, distillation=False)),
        lambda: ops.dm_grad_fwd(odd, odd, odd, odd, idx, tab),
        lambda: ops.dm_gen_bwd(None, x, GEN_SIGMA),
        lambda: ops.dm_gen_bwd(up[:3], x, GEN_SIGMA),
        lambda: ops.dm_gen_bwd(up, off, GEN_SIGMA),
        lambda: ops.dm_gen_bwd(up, x, -1.0),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"call {i} was accepted")


# ------------------------------------------------------------------------------------------ the loss on the shrunken nets
N_NET, S_NET = 4, 18
GEN_SCALE, FAKE_SCALE = 8.0, 32.0          # output-layer scales at which the separations below hold (checked on the CPU oracle first)
NET_IDX = (1, 4, 8, 12)
NET_Y = (3, 871, 40, 999)


class _oracle64:
    """oracle.edm.unet_forward in float64: its three fp32-only pieces (the timestep embedding's .float(), GroupNorm's .float(), the
    legacy attention's fp16 einsums) are replaced, for the duration of the block, by the same expressions in the input's dtype."""

    def __enter__(self):
        import torch.nn.functional as Fn
        from oracle import edm
        self.edm, self.saved = edm, (edm.timestep_embedding, edm._gn, edm.attention_block)

        def te(t, dim, max_period=10000):
            half = dim // 2
            freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
            a = t[:, None].double() * freqs[None]
            return torch.cat([torch.cos(a), torch.sin(a)], dim=-1)

        def gn(sd, name, x):
            return Fn.group_norm(x, 32, sd[name + ".weight"], sd[name + ".bias"], 1e-5)

        def attn(sd, pre, x, heads, prec):
            b, c, hh, ww = x.shape
            L, ch = hh * ww, c // heads
            qkv = edm._conv(sd, pre + ".qkv", gn(sd, pre + ".norm", x), prec).reshape(b, 3 * c, L)
            q, k, v = [u.reshape(b * heads, ch, L) for u in qkv.reshape(b, 3, heads, ch, L).unbind(1)]
            w = torch.softmax(torch.einsum("bct,bcs->bts", q, k) / math.sqrt(ch), dim=-1)
            return x + edm._conv(sd, pre + ".proj_out", torch.einsum("bts,bcs->bct", w, v).reshape(b, c, hh, ww), prec)
        edm.timestep_embedding, edm._gn, edm.attention_block = te, gn, attn
        return edm

    def __exit__(self, *a):
        self.edm.timestep_embedding, self.edm._gn, self.edm.attention_block = self.saved


def _oracle_dm(gen_sd, fake_sd, z, noise, idx, y, weighting):
    """dm_generator_losses on float64 oracle nets (the real net shares the generator's weights, detached) -> loss, s, parameter
    gradients of loss.sum(), and the two separations."""
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
        x = den(leaves, z.double() * GEN_SIGMA, torch.full((len(z),), GEN_SIGMA, dtype=torch.float64))
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


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(a @ b / (a.norm() * b.norm() + 1e-300))


def _net_operands():
    gen = torch.Generator().manual_seed(7)
    z, noise = torch.randn(N_NET, 3, 16, 16, generator=gen), torch.randn(N_NET, 3, 16, 16, generator=gen)
    return z, noise, torch.tensor(NET_IDX), torch.tensor(NET_Y)


def _diffusion(**kw):
    from models.cm.karras_diffusion import KarrasDenoiser
    return KarrasDenoiser(**dict(dict(sigma_data=0.5, weight_schedule="karras", distillation=False), **kw))


def test_dm_generator_losses_vs_fp64_oracle(ops):
    gen_net, real, fake = build(None, "", GEN_SCALE), build(None, "", GEN_SCALE), build(None, "fake:", FAKE_SCALE)
    for p in gen_net.parameters():
        p.requires_grad_(True)
    z, noise, idx, y = _net_operands()
    gen_sd = {k: v.detach().cpu() for k, v in gen_net.state_dict().items()}
    fake_sd = {k: v.detach().cpu() for k, v in fake.state_dict().items()}
    d = _diffusion()
    P = dict(gen_net.named_parameters())
    worst, worst_s, wc, wn = 0.0, 0.0, ("", 1.0), ("", 0.0)
    for weighting in WEIGHTINGS:
        ref_loss, ref_s, ref_grads, sep_g, sep_s = _oracle_dm(gen_sd, fake_sd, z, noise, idx, y, weighting)
        # the separations, per sample, on the oracle: the loss is no small difference of large network outputs
        print(f"{weighting}: rms(D_f - D_r) / max(rms D_f, rms D_r) >= {sep_g:.3f}, mean|x - D_r| / max(rms x, rms D_r) >= {sep_s:.3f}")
        assert sep_g >= 0.5 and sep_s >= 0.5
        gen_net.zero_grad()
        t = d.dm_generator_losses(gen_net, z.to(DEV), S_NET, real_model=real, real_diffusion=_diffusion(), fake_model=fake,
                                  model_kwargs={"y": y.to(DEV)}, noise=noise.to(DEV), indices=idx.to(DEV), weighting=weighting)
        assert set(t) == {"loss", "x", "dm_norm"} and t["loss"].requires_grad and not t["x"].requires_grad
        t["loss"].sum().backward()
        rel = ((t["loss"].detach().cpu().double() - ref_loss).abs() / ref_loss.abs()).max().item()
        rel_s = ((t["dm_norm"].cpu().double() - ref_s).abs() / ref_s).max().item()
        print(f"{weighting}: per-sample loss worst relative error {rel:.3e}, dm_norm {rel_s:.3e}")
        worst, worst_s = max(worst, rel), max(worst_s, rel_s)
        for n, rg in ref_grads.items():
            got = P[n].grad.cpu()
            if rg.norm() < 1e-6 * max(1.0, got.norm().item()):
                continue
            c, nr = _cos(got, rg), (got.double().norm() / rg.norm()).item()
            wc = min(wc, (f"{weighting}.{n}", c), key=lambda v: v[1])
            wn = max(wn, (f"{weighting}.{n}", abs(nr - 1)), key=lambda v: v[1])
        assert all(p.grad is None for net in (real, fake) for p in net.parameters())
        with torch.no_grad():                            # no node: the values of a forward_inference generator
            again = d.dm_generator_losses(gen_net, z.to(DEV), S_NET, real_model=real, real_diffusion=_diffusion(), fake_model=fake,
                                          model_kwargs={"y": y.to(DEV)}, noise=noise.to(DEV), indices=idx.to(DEV), weighting=weighting)
        assert not again["loss"].requires_grad and again["x"].shape == z.shape and torch.isfinite(again["loss"]).all()
    print(f"dm_generator_losses: per-sample loss worst relative error {worst:.3e} (bound {DM_LOSS_REL_BOUND}, cap {DM_LOSS_REL_CAP}); "
          f"dm_norm {worst_s:.3e} (bound {DM_NORM_REL_BOUND}); gradient worst cosine {wc[1]:.5f} ({wc[0]}), worst norm ratio deviation "
          f"{wn[1]:.4f} ({wn[0]})")
    assert DM_LOSS_REL_BOUND <= DM_LOSS_REL_CAP
    assert wc[1] >= 0.995 and wn[1] <= 0.05
    assert worst <= DM_LOSS_REL_BOUND and worst_s <= DM_NORM_REL_BOUND


@pytest.mark.parametrize("sd_f", [0.5, 0.25])
def test_device_node_vs_torch_fallback_on_the_same_nets(ops, sd_f):
    """Wrapped in plain callables the same HIP nets take the torch fallback.  The launch chain of the node is run here by hand too,
    which exposes its operands: both paths are held to the kernel bounds against float64 on those operands."""
    from models.cm.karras_diffusion import cd_levels
    gen_net, real, fake = build(None, "", GEN_SCALE), build(None, "", GEN_SCALE), build(None, "fake:", FAKE_SCALE)
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    d, fd = _diffusion(), _diffusion(sigma_data=sd_f)
    tab = cd_levels(S_NET, 0.002, 80.0, 7.0).device_table(torch.device(DEV))
    wrap = lambda net: (lambda x_in, t, **kw: net(x_in, t, **kw))
    for weighting in WEIGHTINGS:
        kw = dict(real_diffusion=_diffusion(), fake_diffusion=fd, model_kwargs={"y": y}, noise=noise, indices=idx, weighting=weighting)
        with torch.no_grad():
            node = d.dm_generator_losses(gen_net, z, S_NET, real_model=real, fake_model=fake, **kw)
            fb = d.dm_generator_losses(wrap(gen_net), z, S_NET, real_model=wrap(real), fake_model=wrap(fake), **kw)
            x_in, tg = ops.dm_gen_in(z, GEN_SIGMA, 0.5)
            x, x_t, xr, tm, xf = ops.dm_gen_prep(gen_net.forward_inference(x_in, tg, y), z, noise, idx, tab, GEN_SIGMA, 0.5, 0.5, sd_f)
            F_r, F_f = real.forward_inference(xr, tm, y), fake.forward_inference(xr if xf is None else xf, tm, y)
            g, loss, s = ops.dm_grad_fwd(F_r, F_f, x, x_t, idx, tab, weighting, fake=dict(sigma_data=sd_f, sigma_min=0.002, distillation=False))
        assert torch.equal(node["loss"], loss) and torch.equal(node["dm_norm"], s) and torch.equal(node["x"], x)
        _, rl, rs, _, b_l, b_s = grad_ref64(F_r, F_f, x, x_t, tab.cpu()[idx.cpu()], weighting, 0.5, sd_f)
        for name, t in (("node", node), ("fallback", fb)):
            el = ((t["loss"].cpu().double() - rl).abs() / b_l).max().item()
            es = ((t["dm_norm"].cpu().double() - rs).abs() / b_s).max().item()
            print(f"{name} ({weighting}, fake sigma_data {sd_f}) |err| / kernel bound: loss {el:.3f}, dm_norm {es:.3f}; x equal bits: "
                  f"{torch.equal(t['x'], x)}")
            assert el <= 1 and es <= 1, (name, weighting, el, es)


def test_hip_refusals(ops):
    gen_net, real, fake = build(), build(), build(None, "fake:")
    plain = build(dict(class_cond=False))
    z, noise, idx, y = (v.to(DEV) for v in _net_operands())
    d = _diffusion()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx)
    with pytest.raises(NotImplementedError, match="must not require grad"):
        d.dm_generator_losses(gen_net, z.clone().requires_grad_(True), S_NET, model_kwargs={"y": y}, **kw)
    with pytest.raises(NotImplementedError, match="not inputs of UNetModel"):
        d.dm_generator_losses(gen_net, z, S_NET, model_kwargs={"y": y, "w": 1}, **kw)
    with pytest.raises(ValueError, match="class-conditional"):
        d.dm_generator_losses(gen_net, z, S_NET, **kw)
    with pytest.raises(ValueError, match="class-conditional"):
        d.dm_generator_losses(gen_net, z, S_NET, model_kwargs={"y": y}, **dict(kw, fake_model=plain))
    with pytest.raises(NotImplementedError, match="distillation=False"):
        _diffusion(distillation=True).dm_generator_losses(gen_net, z, S_NET, model_kwargs={"y": y}, **kw)


# ------------------------------------------------------------------------------------------ DMTrainLoop
ITERS, EVERY, LR = 5, 2, 1e-4


def _latents():
    gen = torch.Generator().manual_seed(99)
    return [torch.randn(4, 3, 16, 16, generator=gen) for _ in range(ITERS)]


def _loop(tmp, use_fp16, resume="", **over):
    from models.cm.resample import LogNormalSampler
    from models.cm.train_util import DMTrainLoop
    from test_hip_cm_train import PLAIN
    # a fake denoiser that starts AT the teacher makes the first generator gradient exactly zero (the fixed point): another salt here
    gen_net, fake = build(PLAIN, "", GEN_SCALE), build(PLAIN, "fake:", FAKE_SCALE)
    gen_net.train()
    fake.train()
    kw = dict(model=gen_net, diffusion=_diffusion(), real_model=build(PLAIN, "", GEN_SCALE), real_diffusion=_diffusion(), fake_model=fake,
              num_scales=S_NET, gen_update_every=EVERY, fake_lr=2 * LR, data=None, batch_size=4, microbatch=2, lr=LR, ema_rate="0.999,0.9",
              log_interval=2, save_interval=100, resume_checkpoint=resume, use_fp16=use_fp16, schedule_sampler=LogNormalSampler(),
              log_dir=str(tmp))
    kw.update(over)
    return DMTrainLoop(**kw)


def _flat(ps):
    return torch.cat([p.detach().reshape(-1) for p in ps])


def _run(tl, k, z):
    torch.manual_seed(1000 + k)          # the draws of iteration k (indices, noise, sigmas, DSM noise): the device's global stream
    return tl.run_step(z[k].to(DEV), {})


@pytest.mark.parametrize("use_fp16", [True, False])
def test_dmtrainloop_on_the_device(ops, tmp_path, use_fp16):
    from dxmi_hip.optim import RAdam
    z = _latents()
    tl = _loop(tmp_path, use_fp16)
    assert isinstance(tl.fake_opt, RAdam) and tl.fake_opt is not tl.opt and tl.fake_trainer is not tl.mp_trainer
    probe = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    pt = torch.tensor([1.5, -2.0], device=DEV)
    teacher_out = tl.real_model.forward_inference(probe, pt).clone()
    infer = lambda net: net.forward_inference(probe, pt).clone()
    gens, fakes, emas, lg = {}, {}, {}, None
    g_prev, f_prev = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
    e_prev, out_prev = _flat(tl.ema_params[0]).clone(), infer(tl.model)
    for k in range(ITERS):
        took_gen, took_fake = _run(tl, k, z)
        on = k % EVERY == 0
        assert took_gen == on and took_fake, k
        gens[k], fakes[k] = _flat(tl.model.parameters()).clone(), _flat(tl.fake_model.parameters()).clone()
        emas[k] = torch.cat([_flat(p) for p in tl.ema_params]).clone()
        assert torch.equal(gens[k], g_prev) != on and not torch.equal(fakes[k], f_prev), k
        assert torch.equal(_flat(tl.ema_params[0]), e_prev) != on, k
        assert torch.equal(tl.real_model.forward_inference(probe, pt), teacher_out), k      # the teacher is untouched
        out = infer(tl.model)
        assert torch.equal(out, out_prev) != on, k                   # forward_inference reads the new weights: the packs followed
        assert tl.model._packed_key == tl.model._param_key() and tl.fake_model.forward_inference(probe, pt) is not None
        assert tl.fake_model._packed_key == tl.fake_model._param_key()
        g_prev, f_prev, e_prev, out_prev = gens[k], fakes[k], _flat(tl.ema_params[0]).clone(), out
        if tl.step == 2:
            tl.save()
            lg = (tl.mp_trainer.lg_loss_scale, tl.fake_trainer.lg_loss_scale)
    row = tl.dumpkvs()
    assert {"loss", "dm_norm", "fake_mse", "fake_xs_mse"} <= set(row) and all(math.isfinite(row[k]) for k in ("loss", "dm_norm", "fake_mse"))
    if use_fp16:
        assert "lg_loss_scale" in row and "fake_lg_loss_scale" in row
    files = set(os.listdir(tmp_path))
    assert {"model000002.pt", "opt000002.pt", "ema_0.999_000002.pt", "ema_0.9_000002.pt", "fake_model000002.pt", "fake_opt000002.pt"} <= files

    tr = _loop(tmp_path, use_fp16, resume=str(tmp_path / "model000002.pt"))
    assert tr.step == 2 and torch.equal(_flat(tr.model.parameters()), gens[1]) and torch.equal(_flat(tr.fake_model.parameters()), fakes[1])
    tr.mp_trainer.lg_loss_scale, tr.fake_trainer.lg_loss_scale = lg          # the loss scales are not checkpointed
    for k in (2, 3, 4):
        _run(tr, k, z)
        assert torch.equal(_flat(tr.model.parameters()), gens[k]), k
        assert torch.equal(_flat(tr.fake_model.parameters()), fakes[k]), k
        assert torch.equal(torch.cat([_flat(p) for p in tr.ema_params]), emas[k]), k
    os.remove(tmp_path / "fake_model000002.pt")
    with pytest.raises(FileNotFoundError, match="fake_model000002"):
        _loop(tmp_path, use_fp16, resume=str(tmp_path / "model000002.pt"))
    with pytest.raises(NotImplementedError, match="use_graph"):
        _loop(tmp_path / "g", True, use_graph=True)


# ------------------------------------------------------------------------------------------ sampler
class _Analytic(torch.nn.Module):
    def forward(self, x_in, t, **kw):
        return 4.0 * torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


class _Replay:
    def __init__(self, z):
        self.z = z

    def randn(self, *shape, device=None):
        assert tuple(shape) == tuple(self.z.shape)
        return self.z.to(device)


@pytest.mark.parametrize("model", ["analytic", "unet"])
def test_dm_sample_vs_fp64_and_nfe(ops, model):
    from models.cm.karras_diffusion import dm_sample
    net = _Analytic() if model == "analytic" else build(None, "", GEN_SCALE)
    kw = {} if model == "analytic" else {"y": torch.tensor(NET_Y, device=DEV)}
    z = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(21))
    seen = []
    hook = net.register_forward_hook(lambda m, a, out: seen.append(out.detach().clone()))
    try:
        outs = {clip: dm_sample(_diffusion(), net, z.shape, clip_denoised=clip, model_kwargs=kw, generator=_Replay(z), device=DEV)
                for clip in (True, False)}
    finally:
        hook.remove()
    assert len(seen) == 2                                  # NFE = 1 per call
    cs, co, _ = scal64(torch.full((4,), GEN_SIGMA))
    for clip, F in zip((True, False), seen):
        ref = co * F.cpu().double() + cs * z.double() * GEN_SIGMA
        M = (co * F.cpu().double()).abs() + (cs * z.double() * GEN_SIGMA).abs()
        assert close(outs[clip], ref.clamp(-1, 1) if clip else ref, M)
    assert outs[True].min() >= -1 and outs[True].max() <= 1 and torch.equal(outs[True], outs[False].clamp(-1, 1))
    if model == "analytic":
        assert outs[False].abs().max() > 1                # the clamp had something to do
    drawn = dm_sample(_diffusion(), net, z.shape, model_kwargs=kw, device=DEV)
    assert torch.isfinite(drawn).all() and drawn.std() > 0


@pytest.mark.parametrize("kind", ["determ", "determ-indiv"])
def test_dm_sample_batch_invariance(ops, kind):
    from models.cm.karras_diffusion import dm_sample
    from models.cm.random_util import get_generator
    net = build(None, "", GEN_SCALE)
    y = torch.tensor([3, 871, 40, 999, 7, 512], device=DEV)
    gen = get_generator(kind, 6, seed=(1 << 35) + 3)

    def run(done, rows):
        gen.set_done_samples(done)
        out = dm_sample(_diffusion(), net, (rows.stop - rows.start, 3, 16, 16), model_kwargs={"y": y[rows]}, generator=gen, device=DEV)
        assert gen.draw == 1
        return out.clone()
    whole = run(0, slice(0, 6))
    parts = torch.cat([run(0, slice(0, 3)), run(3, slice(3, 6))])
    assert torch.equal(whole, parts) and not torch.equal(whole[0], whole[1])
    with pytest.raises(NotImplementedError, match="--cm_sampler onestep"):
        dm_sample(_diffusion(distillation=True), net, (2, 3, 16, 16), model_kwargs={"y": y[:2]}, device=DEV)


# ------------------------------------------------------------------------------------------ command line
def test_cli_cm_train_dm_then_sample(ops, tmp_path):
    """cm_train.py --training_mode dm, 3 iterations on a shrunken config from a saved teacher, no data flag; then
    generate_large.py --karras_sampler dm on the generator it wrote."""
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
                        "--ema_rate", "0.999,0.9", "--lr", "1e-4", "--log_dir", str(tmp_path / "run")] + args, cwd=PKG, env=env,
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = set(os.listdir(tmp_path / "run"))
    want = {"model000002.pt", "ema_0.999_000002.pt", "ema_0.9_000002.pt", "opt000002.pt", "fake_model000002.pt", "fake_opt000002.pt",
            "model000003.pt", "progress.jsonl"}
    assert want <= files, files
    student = torch.load(tmp_path / "run" / "model000002.pt", map_location=DEV)
    fake_sd = torch.load(tmp_path / "run" / "fake_model000002.pt", map_location=DEV)
    te = teacher.state_dict()
    assert all(torch.isfinite(v).all() for v in student.values()) and all(torch.isfinite(v).all() for v in fake_sd.values())
    # the fake denoiser has trained; the generator's first step met fake == real, whose gradient is exactly zero (the fixed point)
    assert any(not torch.equal(fake_sd[k], te[k]) for k in te) and all(torch.equal(student[k], te[k]) for k in te)
    import json
    rows = [json.loads(l) for l in open(tmp_path / "run" / "progress.jsonl")]
    assert len(rows) == 3 and all(math.isfinite(r_[k]) for r_ in rows for k in ("loss", "dm_norm", "fake_mse", "fake_xs_mse"))
    assert rows[0]["loss"] == 0 and rows[2]["loss"] > 0 and all(r_["dm_norm"] > 0 for r_ in rows)

    import dxmi_config
    os.makedirs(tmp_path / "gen")
    samp = dict(sample_shape=[3, 16, 16], n_timesteps=4, class_cond=True, num_classes=1000, trainable_beta="fix_last",
                stochastic_last=True, rho=4.0)
    dxmi_config.save(dxmi_config.Cfg({"diffusion": dict(over, distillation=False), "sampler": samp, "training": {"seed": 42}}),
                     os.path.join(tmp_path / "gen", "config.yaml"))
    gen_args = ["--log_dir", str(tmp_path / "gen"), "--karras_sampler", "dm", "--pretrained", str(tmp_path / "run" / "model000002.pt"),
                "--n_sample", "4", "--batchsize", "2"]
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "generate_large.py"] + gen_args, cwd=PKG, env=env,
                       capture_output=True, text=True, timeout=700)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "1 NFE/image (dm, 1 steps)" in r.stdout, r.stdout[-2000:]
    npz = np.load(tmp_path / "gen" / "samples_4.npz")["arr_0"]
    assert npz.shape == (4, 16, 16, 3) and npz.dtype == np.uint8 and npz.std() > 0
