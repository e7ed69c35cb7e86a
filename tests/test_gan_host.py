"""Host side of DMD2's GAN term: the wiring of the new entry points, the head's torch path against a float64 restatement written
here, the generator term of KarrasDenoiser.dm_generator_losses and gan_discriminator_losses on small analytic modules that offer
`encode`, the refusals, DMTrainLoop with a head (clocks, save / resume), the command line, and the C entry points of
csrc/gan_head.hip under the host sanitizers.  No GPU.

Error bounds of the fp32 torch path against float64 (u = 2^-24), in the form of test_dm_host.py: an elementwise result is held to
16 u M, M the magnitude of the operands that meet in it, a per-sample mean to 64 u of the mean of its terms' magnitudes.
  logit      The last product is a sum with magnitude A = sum_c |w_c a_c| + |b|: 16 u A for the product itself.  What the earlier
             layers rounded reaches it through the two GroupNorms, each of which turns a relative perturbation of its input into one
             kappa = max_g (m^2 + var) / (var + eps) times as large (the conditioning term of forward_bounds, on the float64 values,
             per sample): |logit - logit64| <= 16 u A kappa1 kappa2.  A worst-case running bound (K u sum|w||x| per conv, added
             coherently) is 1e4 u here and would let a wrong fourth digit pass; this one is of the order of the error.
  inputs     An error E of the head's input (the features, known elementwise from 16 u M of every step before them) reaches the logit
             through the float64 Jacobian: sum |d logit / d feat| E, first order.
  gradients  forward and backward pass ten fp32 steps of 16 u each and the two norms: 256 u kappa1 kappa2 of the magnitude of the terms
             that meet in the gradient (given at each check), and the GAN part of a checked gradient must be at least 4 bounds large, so
             that neither its omission nor an error of a quarter of it fits.
Measured on the CPU (this file's prints): the head's logit at C = 64 errs by 0.12 of its bound (46 u); in the loss tests the logit
bounds are 140 to 190 u, most of it the elementwise steps' 16 u M carried through the Jacobian, and the errors 0.02 to 0.03 of them;
the GAN part of the generator's gradient is 50 (a) and 537 (w) bounds large; the discriminator's gradients err by 0.005 of theirs."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from test_dm_host import U, _diffusion, _flat, _loop, _operands, _restate64, _t4, _Tanh, _Tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dxmi_gan_head_supported", "dxmi_gan_conv4s2_pack", "dxmi_gan_conv4s2_fwd", "dxmi_gan_conv4s2_dgrad", "dxmi_gan_conv4s2_wgrad",
           "dxmi_gan_logit_loss_fwd", "dxmi_gan_logit_loss_bwd", "dxmi_gan_join")
KEYS = [f"cls_pred_branch.{i}.{p}" for i in (0, 1, 3, 4, 6) for p in ("weight", "bias")]
FC, FMAP, FG = 8, 4, 2          # the small head of the loss tests: 8 channels in 2 groups on a 4x4 map


# ------------------------------------------------------------------------------------------ wiring
def test_entry_points_are_declared_everywhere():
    from dxmi_hip import _lib, ops
    header = open(os.path.join(ROOT, "include", "dxmi_hip.h")).read()
    makefile = open(os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc", "Makefile")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header) and sym in _lib.SIGNATURES, sym
        assert hasattr(ops, sym[len("dxmi_"):]), sym
    assert "dxmi_gan_conv4s2_workspace_bytes" in _lib.SIGNATURES and "dxmi_gan_conv4s2_slices" in _lib.SIGNATURES
    assert "gan_head.hip" in re.search(r"^SRCS = (.*)$", makefile, flags=re.M).group(1).split()
    assert "asan_gan" in makefile and os.path.exists(os.path.join(ROOT, "tests", "host", "cabi_malformed_gan.c"))
    assert "Yin et al. 2024" in header and "DMD2" in header


# ------------------------------------------------------------------------------------------ the head's torch path
def _head(C=FC, m=FMAP, groups=FG, seed=3, scale=1.0):
    from models.cm.gan_head import GANHead
    torch.manual_seed(seed)
    head = GANHead(C, m, groups)
    with torch.no_grad():
        for p in head.parameters():          # away from the default init's near-zero biases and unit gains: every term takes part
            p.add_(0.05 * torch.randn_like(p))
            p.mul_(scale)
    return head


def _head64(head, h):
    """float64 restatement of the head on an NCHW input (differentiable) -> (logit [N], A [N], kappa1 kappa2 [N], detached)."""
    sd = {k: v.detach().double() for k, v in head.state_dict().items()}
    G, k = head.groups, head.map_size // 2
    kap = []

    def gn_silu(x, i):
        N = x.shape[0]
        xg = x.reshape(N, G, -1)
        mu, var = xg.mean(2, keepdim=True), xg.var(2, unbiased=False, keepdim=True)
        kap.append(((mu ** 2 + var) / (var + 1e-5)).detach().reshape(N, G).max(1).values)
        y = ((xg - mu) * (var + 1e-5) ** -0.5).reshape(x.shape) * sd[KEYS[i]][None, :, None, None] + sd[KEYS[i + 1]][None, :, None, None]
        return y * torch.sigmoid(y)

    a1 = gn_silu(F.conv2d(h.double(), sd[KEYS[0]], sd[KEYS[1]], stride=2, padding=1), 2)
    a2 = gn_silu(F.conv2d(a1, sd[KEYS[4]], sd[KEYS[5]], stride=k), 6)
    w, b = sd[KEYS[8]], sd[KEYS[9]]
    logit = F.conv2d(a2, w, b).reshape(-1)
    A = F.conv2d(a2.detach().abs(), w.abs(), b.abs()).reshape(-1)
    return logit, A, kap[0] * kap[1]


def _logit_bound(head, feat, E_feat):
    """-> (logit64, bound) at float64 features known to within E_feat: 16 u A kappa1 kappa2 + sum |d logit / d feat| E_feat."""
    f = feat.detach().clone().requires_grad_(True)
    logit, A, kap = _head64(head, f)
    J, = torch.autograd.grad(logit.sum(), f)
    return logit.detach(), 16 * U * A * kap + (J.abs() * E_feat).flatten(1).sum(1)


@pytest.mark.parametrize("C,m", [(64, 8), (64, 4)])
def test_head_torch_path_against_float64(C, m):
    from models.cm.gan_head import GANHead
    head = _head(C, m, 4)          # 16 channels per group: the second norm (one pixel) then has groups of 16 values, not of 2
    assert list(head.state_dict()) == KEYS and list(GANHead(C, m).state_dict()) == KEYS
    b = head.cls_pred_branch
    assert (b[0].kernel_size, b[0].stride, b[0].padding) == ((4, 4), (2, 2), (1, 1))
    assert (b[3].kernel_size, b[3].stride, b[3].padding) == ((m // 2, m // 2), (m // 2, m // 2), (0, 0))
    assert b[6].weight.shape == (1, C, 1, 1) and b[1].eps == 1e-5 and b[4].eps == 1e-5 and GANHead(C, m).cls_pred_branch[1].num_groups == 32
    h = torch.randn(5, C, m, m, generator=torch.Generator().manual_seed(1))
    logit = head(h)
    assert logit.shape == (5,) and logit.dtype == torch.float32 and logit.requires_grad
    l64, E = _logit_bound(head, h, torch.zeros_like(h, dtype=torch.float64))
    ratio = float(((logit.detach().double() - l64).abs() / E).max())
    print(f"head torch path (C={C}, map={m}): worst |logit - logit64| / (16 u A kappa1 kappa2) = {ratio:.3f} (bound {float(E.max()):.2e}, "
          f"{float((E / U).max()):.0f} u; |logit| up to {float(l64.abs().max()):.3f})")
    assert ratio <= 1
    # and the restatement is the module: float64 module against the restatement
    import copy
    m64 = copy.deepcopy(b).double()
    assert torch.allclose(m64(h.double()).reshape(-1), l64, rtol=1e-12, atol=1e-12)
    for bad in (6, 16):
        with pytest.raises(ValueError, match="map_size"):
            GANHead(C, bad)


# ------------------------------------------------------------------------------------------ analytic modules with an encode
class _TanhEnc(_Tanh):
    """_Tanh with bottleneck features: encode = tanh(E . avgpool2(x_in) + 1e-3 t), [N, 8, 4, 4] for an 8x8 image."""

    def __init__(self, w, a=1.0, dtype=torch.float32):
        super().__init__(w, a, dtype)
        gen = torch.Generator().manual_seed(17)
        self.e = torch.nn.Parameter((torch.randn(FC, 3, generator=gen) * 0.8).to(dtype))

    def encode(self, x_in, t, **kw):
        return torch.tanh(torch.einsum("oc,nchw->nohw", self.e, F.avg_pool2d(x_in, 2)) + 1e-3 * _t4(t))


def _encode64(fake64, x_in, E_in, t):
    """-> (features, their bound, first order): the pool is a mean of 4 (4 u), the mix a sum of 3 products and the time term (8 u of
    their magnitudes), tanh passes an error of its argument on with its derivative 1 - tanh^2."""
    p, Ep = F.avg_pool2d(x_in, 2), F.avg_pool2d(E_in, 2) + 4 * U * F.avg_pool2d(x_in.abs(), 2)
    e = fake64.e.detach()
    arg = torch.einsum("oc,nchw->nohw", e, p) + 1e-3 * _t4(t)
    Ea = torch.einsum("oc,nchw->nohw", e.abs(), Ep) + 8 * U * (torch.einsum("oc,nchw->nohw", e.abs(), p.abs()) + 1e-3 * _t4(t.abs()))
    out = torch.tanh(arg)
    return out, (1 - out ** 2) * Ea + 4 * U * out.abs()


def _gan_operands(N=6, shape=(3, 8, 8), S=18, seed=23):
    gen = torch.Generator().manual_seed(seed)
    gan_noise = torch.randn(N, *shape, generator=gen)
    gan_idx = torch.randint(0, S, (N,), generator=gen)
    gan_idx[0], gan_idx[1] = S - 1, 0
    return gan_noise, gan_idx


def _nets(dtype=torch.float32):
    return _Tanh(0.7, dtype=dtype), _Tanh(0.9, 0.8, dtype), _TanhEnc(0.5, 0.6, dtype)


W_GAN = 0.3


def test_generator_term_torch_path_against_float64():
    from models.cm.karras_diffusion import cd_levels
    S = 18
    z, noise, idx = _operands(S=S)
    gan_noise, gan_idx = _gan_operands(S=S)
    gen, real, fake = _nets()
    head = _head()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx)
    terms = _diffusion().dm_generator_losses(gen, z, S, gan_head=head, gan_gen_weight=W_GAN, gan_noise=gan_noise, gan_indices=gan_idx, **kw)
    assert set(terms) == {"loss", "x", "dm_norm", "gan_loss", "gan_logit"}
    assert terms["gan_loss"].shape == (6,) and terms["gan_logit"].shape == (6,)
    assert not terms["gan_loss"].requires_grad and not terms["gan_logit"].requires_grad and terms["loss"].requires_grad
    plain = _diffusion().dm_generator_losses(gen, z, S, **kw)
    assert set(plain) == {"loss", "x", "dm_norm"} and torch.equal(plain["x"], terms["x"])
    plain["loss"].sum().backward()
    headless = {id(p): p.grad.double().clone() for p in gen.parameters()}
    gen.zero_grad()
    # float64: the DM part by test_dm_host's restatement, the GAN part through encode and the head
    g64, r64, f64 = _nets(torch.float64)
    r = _restate64(g64, r64, f64, z, noise, idx, S, "dmd")
    tab = cd_levels(S, 0.002, 80.0, 7.0).table.double()
    tg = tab[gan_idx]
    c_in = 1 / (tg ** 2 + 0.25) ** 0.5
    x = r["x"]
    # the GAN term's values are judged at the x the fp32 path had (x itself is held to test_dm_host's 16 u M_x, which is large: x is a
    # small difference of c_skip sigma_G z and c_out F): what separates the two paths from there on is the elementwise steps' 16 u M
    x32 = terms["x"].double()
    x_in = _t4(c_in) * (x32 + gan_noise.double() * _t4(tg))
    E_in = 16 * U * _t4(c_in) * (x32.abs() + (gan_noise.double() * _t4(tg)).abs())
    feat, E_feat = _encode64(f64, x_in.detach(), E_in, 250 * torch.log(tg))
    l64, E_l = _logit_bound(head, feat, E_feat)
    gl64 = F.softplus(-l64)
    e_logit = float(((terms["gan_logit"].double() - l64).abs() / E_l).max())
    e_gl = float(((terms["gan_loss"].double() - gl64).abs() / (E_l + 16 * U * gl64)).max())
    # loss = dm_loss + w gan_loss, the DM part bit for bit the head-less call's (itself held to 64 u l_mag by test_dm_host.py)
    loss64 = plain["loss"].detach().double() + W_GAN * gl64
    b_loss = W_GAN * (E_l + 16 * U * gl64) + 16 * U * (plain["loss"].detach().double().abs() + W_GAN * gl64)
    e_loss = float(((terms["loss"].detach().double() - loss64).abs() / b_loss).max())
    assert ((plain["loss"].detach().double() - r["loss"].detach()).abs() <= 64 * U * r["l_mag"]).all()
    print(f"generator term vs fp64: |err| / bound gan_logit {e_logit:.3f}, gan_loss {e_gl:.3f}, loss {e_loss:.3f}; logit bound "
          f"{float((E_l / U).max()):.0f} u at |logit| {[round(v, 4) for v in l64.tolist()]}")
    assert e_logit <= 1 and e_gl <= 1 and e_loss <= 1
    # the gradient: float64 autograd of dm surrogate + w softplus(-logit), the GAN part through x alone, the two parts apart
    params64 = [g64.w, g64.a]
    feat_g = f64.encode(_t4(c_in) * (x + gan_noise.double() * _t4(tg)), 250 * torch.log(tg))
    feat_g.retain_grad()
    gan64 = F.softplus(-_head64(head, feat_g)[0]).sum()
    g_dm = torch.autograd.grad(r["surrogate"].sum(), params64, retain_graph=True)
    g_gan = torch.autograd.grad(W_GAN * gan64, params64, retain_graph=True)
    d_feat, = torch.autograd.grad(gan64, feat_g)
    terms["loss"].sum().backward()
    # the magnitude of the terms of d gan_loss / d x: |d_feat| back through encode with every factor in absolute value (tanh', |e|, the
    # 2x2 mean's 1/4, c_in); the DM part's bound is test_dm_host's
    kap = _head64(head, feat)[2]
    m = torch.einsum("oc,nohw->nchw", f64.e.detach().abs(), d_feat.abs() * (1 - feat_g.detach() ** 2))
    M_glx = _t4(c_in) * m.repeat_interleave(2, 2).repeat_interleave(2, 3) / 4
    per_elem = ((16 * U * r["M_g"] + 16 * U * r["g"].abs()) / z[0].numel() + W_GAN * 256 * U * _t4(kap) * M_glx) * _t4(r["c_out_g"])
    # The GAN part alone: the head-less call on the same operands forms bit for bit the same DM direction g, and the backward is
    # linear in the direction, so (gradient with the head) - (head-less gradient) is the GAN part up to its own error, 256 u kappa of
    # its terms, and the rounding of the two sums over the elements, 64 u of their terms' magnitudes each
    g32 = r["g"].abs() + 16 * U * r["M_g"]
    diff_elem = (W_GAN * 256 * U * _t4(kap) * M_glx + 2 * 64 * U * (g32 / z[0].numel() + W_GAN * M_glx)) * _t4(r["c_out_g"])
    for p, gd, gg, dx in ((gen.w, g_dm[0], g_gan[0], abs(float(g64.a.detach())) * r["x_in_g"].abs()),
                          (gen.a, g_dm[1], g_gan[1], torch.ones_like(z, dtype=torch.float64))):
        name = "w" if p is gen.w else "a"
        ref, bound = float(gd + gg), float((per_elem * dx).sum())
        err = abs(float(p.grad) - ref)
        part, b_part = float(p.grad.double() - headless[id(p)]), float((diff_elem * dx).sum())
        e_part = abs(part - float(gg))
        print(f"  d loss / d {name}: {float(p.grad):.7g} vs {ref:.7g}, |err| / bound {err / bound:.3f}; GAN part {part:.6g} vs {float(gg):.6g}, "
              f"|err| / bound {e_part / b_part:.3f}, GAN part / bound {abs(float(gg)) / b_part:.0f}")
        assert p.grad is not None and err <= bound and e_part <= b_part
        assert abs(float(gg)) >= 4 * b_part          # neither the GAN part's omission nor an error of a quarter of it fits
    for net in (real, fake, head):
        assert all(p.grad is None for p in net.parameters())


def test_generator_term_weight_zero_and_draw_order():
    S = 18
    z, noise, idx = _operands(S=S)
    gan_noise, gan_idx = _gan_operands(S=S)
    gen, real, fake = _nets()
    head = _head()
    kw = dict(real_model=real, real_diffusion=_diffusion(), fake_model=fake, noise=noise, indices=idx)
    a = _diffusion().dm_generator_losses(gen, z, S, **kw)
    a["loss"].sum().backward()
    ga = (gen.w.grad.clone(), gen.a.grad.clone())
    gen.zero_grad()
    b = _diffusion().dm_generator_losses(gen, z, S, gan_head=head, gan_gen_weight=0.0, gan_noise=gan_noise, gan_indices=gan_idx, **kw)
    b["loss"].sum().backward()
    for k in ("loss", "x", "dm_norm"):
        assert torch.equal(a[k].detach(), b[k].detach()), k
    assert torch.equal(ga[0], gen.w.grad) and torch.equal(ga[1], gen.a.grad)
    with torch.no_grad():
        c = _diffusion().dm_generator_losses(gen, z, S, gan_head=head, gan_gen_weight=W_GAN, gan_noise=gan_noise, gan_indices=gan_idx, **kw)
    assert not c["loss"].requires_grad and torch.equal(c["gan_logit"], b["gan_logit"])
    # draw order: the head-less call's indices and noise first, then gan_indices over the GAN term's range, then gan_noise
    seen = []

    class _Spy(_TanhEnc):
        def forward(self, x_in, t, **kw):
            seen.append(("forward", t.clone()))
            return super().forward(x_in, t, **kw)

        def encode(self, x_in, t, **kw):
            seen.append(("encode", t.clone(), x_in.clone()))
            return super().encode(x_in, t, **kw)
    spy = _Spy(0.5, 0.6)
    base = dict(real_model=real, real_diffusion=_diffusion(), fake_model=spy)
    state = torch.get_rng_state()
    g1 = torch.Generator().manual_seed(11)
    with torch.no_grad():
        t1 = _diffusion().dm_generator_losses(gen, z, S, generator=g1, gan_head=head, gan_gen_weight=W_GAN, gan_min_step_frac=0.5, **base)
    assert torch.equal(torch.get_rng_state(), state)
    g2 = torch.Generator().manual_seed(11)
    with torch.no_grad():
        t0 = _diffusion().dm_generator_losses(gen, z, S, generator=g2, **base)
    assert torch.equal(t1["dm_norm"], t0["dm_norm"]) and torch.equal(t1["x"], t0["x"])          # the same indices and noise
    from models.cm.karras_diffusion import cd_levels, dm_index_range
    lo, hi = dm_index_range(S, 0.5, 1.0)
    want_idx = torch.randint(lo, hi + 1, (6,), generator=g2)
    want_noise = torch.randn(z.shape, generator=g2)
    enc = [s for s in seen if s[0] == "encode"][0]
    tab = cd_levels(S, 0.002, 80.0, 7.0).table
    tg = tab[want_idx]
    assert torch.equal(enc[1], 1000 * 0.25 * torch.log(tg + 1e-44))
    c_in = 1 / (tg ** 2 + 0.25) ** 0.5
    want64 = _t4(c_in.double()) * (t1["x"].double() + want_noise.double() * _t4(tg.double()))      # the elementwise steps: 16 u M
    M_in = _t4(c_in.double()) * (t1["x"].double().abs() + (want_noise.double() * _t4(tg.double())).abs())
    assert ((enc[2].double() - want64).abs() <= 16 * U * M_in).all()


# ------------------------------------------------------------------------------------------ the discriminator loss
def test_discriminator_loss_torch_path_against_float64():
    from models.cm.karras_diffusion import cd_levels
    S, N = 18, 4
    gen = torch.Generator().manual_seed(31)
    x_fake, x_real = torch.randn(N, 3, 8, 8, generator=gen) * 0.5, torch.rand(N, 3, 8, 8, generator=gen) * 2 - 1
    noise = torch.randn(2 * N, 3, 8, 8, generator=gen)
    idx = torch.randint(0, S, (2 * N,), generator=gen)
    fake, head, other = _TanhEnc(0.5, 0.6), _head(), _Tanh(0.7)
    terms = _diffusion().gan_discriminator_losses(fake, head, x_fake, x_real, S, noise=noise, indices=idx)
    assert set(terms) == {"loss", "logit_fake", "logit_real"} and all(v.shape == (N,) for v in terms.values())
    assert terms["loss"].requires_grad and not terms["logit_fake"].requires_grad and not terms["logit_real"].requires_grad
    f64 = _TanhEnc(0.5, 0.6, torch.float64)
    t = cd_levels(S, 0.002, 80.0, 7.0).table.double()[idx]
    c_in = 1 / (t ** 2 + 0.25) ** 0.5
    x = torch.cat([x_fake, x_real]).double()
    x_t = x + noise.double() * _t4(t)
    x_in = _t4(c_in) * x_t
    E_in = _t4(c_in) * 4 * U * (x.abs() + (noise.double() * _t4(t)).abs()) + 4 * U * x_in.abs()
    feat, E_feat = _encode64(f64, x_in, E_in, 250 * torch.log(t))
    l64, E_l = _logit_bound(head, feat, E_feat)
    got = torch.cat([terms["logit_fake"], terms["logit_real"]]).double()
    e_logit = float(((got - l64).abs() / E_l).max())
    sp = torch.cat([F.softplus(l64[:N]), F.softplus(-l64[N:])])
    loss64 = sp[:N] + sp[N:]
    b_loss = E_l[:N] + E_l[N:] + 16 * U * loss64
    e_loss = float(((terms["loss"].detach().double() - loss64).abs() / b_loss).max())
    print(f"discriminator loss vs fp64: |err| / bound logits {e_logit:.3f}, loss {e_loss:.3f}; logit bound {float((E_l / U).max()):.0f} u")
    assert e_logit <= 1 and e_loss <= 1
    # gradients: float64 autograd through the float64 module and encode; they reach the head and encode's parameter, nothing else.
    # The terms that meet in a parameter's gradient are the 2N samples' own gradients: M = sum_n |d loss_n / d p| (a cancellation inside
    # one sample's sum over pixels is not visible to M, so the tensors are compared in the 2-norm): ||got - ref|| <= 256 u kappa ||M||
    import copy
    head64 = copy.deepcopy(head.cls_pred_branch).double()
    named = [("encode.e", fake.e, f64.e)] + [(n, p, dict(head64.named_parameters())[n]) for n, p in head.cls_pred_branch.named_parameters()]
    lg = head64(f64.encode(x_in, 250 * torch.log(t))).reshape(-1)
    per_sample = torch.cat([F.softplus(lg[:N]), F.softplus(-lg[N:])])
    M = [torch.zeros_like(q) for _, _, q in named]
    ref = [torch.zeros_like(q) for _, _, q in named]
    for n in range(2 * N):
        for j, g in enumerate(torch.autograd.grad(per_sample[n], [q for _, _, q in named], retain_graph=True)):
            M[j] += g.abs()
            ref[j] += g
    terms["loss"].sum().backward()
    kap = float(_head64(head, feat)[2].max())
    worst = 0.0
    for (name, p, _), r64, m in zip(named, ref, M):
        assert p.grad is not None and float(r64.norm()) > 0, name
        err, bound = float((p.grad.double() - r64).norm()), 256 * U * kap * float(m.norm())
        worst = max(worst, err / bound)
        assert err <= bound, (name, err, bound)
        assert float(r64.norm()) >= 4 * bound, name
    print(f"discriminator gradients: worst ||err|| / (256 u kappa ||M||) = {worst:.3f} (kappa {kap:.2f})")
    assert fake.w.grad is None and fake.a.grad is None and all(p.grad is None for p in other.parameters())


def test_discriminator_loss_fixed_points_and_refusals():
    S, N = 18, 3
    gen = torch.Generator().manual_seed(32)
    x_fake, x_real = torch.randn(N, 3, 8, 8, generator=gen), torch.randn(N, 3, 8, 8, generator=gen)
    fake, head = _TanhEnc(0.5, 0.6), _head()
    with torch.no_grad():
        for p in head.parameters():
            p.zero_()
    terms = _diffusion().gan_discriminator_losses(fake, head, x_fake, x_real, S)
    two_ln2 = torch.full((N,), 2 * 0.6931471805599453)
    assert torch.allclose(terms["loss"].detach(), two_ln2, rtol=4 * U, atol=0) and torch.equal(terms["logit_fake"], torch.zeros(N))
    for level in (100.0, -100.0):                        # saturated logits: finite losses and gradients
        head = _head()
        with torch.no_grad():
            head.cls_pred_branch[6].weight.zero_()
            head.cls_pred_branch[6].bias.fill_(level)
        terms = _diffusion().gan_discriminator_losses(fake, head, x_fake, x_real, S)
        small, large = 3.8e-44, 100.0                    # softplus(-100) is a denormal: an absolute floor stands in for a relative bound
        assert torch.isfinite(terms["loss"]).all()
        assert torch.allclose(terms["loss"].detach().double(), torch.full((N,), small + large, dtype=torch.float64), rtol=4 * U, atol=1e-37)
        terms["loss"].sum().backward()
        g = head.cls_pred_branch[6].bias.grad
        assert torch.isfinite(g).all() and abs(float(g) - (N if level > 0 else -N)) <= 1e-5
    with pytest.raises(ValueError, match="one shape"):
        _diffusion().gan_discriminator_losses(fake, head, x_fake, x_real[:2], S)
    with pytest.raises(NotImplementedError, match="encode"):
        _diffusion().gan_discriminator_losses(_Tanh(0.5), head, x_fake, x_real, S)
    # one draw of indices [2N], then noise [2N, C, H, W], from the generator
    seen = []

    class _Spy(_TanhEnc):
        def encode(self, x_in, t, **kw):
            seen.append(t.clone())
            return super().encode(x_in, t, **kw)
    from models.cm.karras_diffusion import cd_levels, dm_index_range
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    _diffusion().gan_discriminator_losses(_Spy(0.5), head, x_fake, x_real, S, generator=g1, gan_max_step_frac=0.5)
    lo, hi = dm_index_range(S, 0.0, 0.5)
    want = torch.randint(lo, hi + 1, (2 * N,), generator=g2)
    assert torch.equal(seen[0], 1000 * 0.25 * torch.log(cd_levels(S, 0.002, 80.0, 7.0).table[want] + 1e-44))


def test_generator_term_refusals(tmp_path):
    z, noise, idx = _operands()
    gen, real, fake = _nets()
    kw = dict(real_model=real, real_diffusion=_diffusion(), noise=noise, indices=idx)
    with pytest.raises(NotImplementedError, match="encode"):
        _diffusion().dm_generator_losses(gen, z, 18, fake_model=_Tanh(0.5), gan_head=_head(), **kw)
    with pytest.raises(ValueError, match="gan_gen_weight"):
        _diffusion().dm_generator_losses(gen, z, 18, fake_model=fake, gan_head=_head(), gan_gen_weight=float("nan"), **kw)
    with pytest.raises(TypeError):
        _diffusion().sid_generator_losses(gen, z, 18, fake_model=fake, gan_head=_head(), **kw)
    with pytest.raises(NotImplementedError, match="SiDA"):
        _loop(tmp_path, objective="sid", gan_head=_head(), real_data=iter([]))
    with pytest.raises(ValueError, match="real_data"):
        _loop(tmp_path, gan_head=_head())


# ------------------------------------------------------------------------------------------ DMTrainLoop with a head
class _TinyEnc(_Tiny):
    def __init__(self, seed):
        super().__init__(seed)
        gen = torch.Generator().manual_seed(seed + 100)
        self.e = torch.nn.Parameter(torch.randn(FC, 3, generator=gen) * 0.8)

    def encode(self, x, t):
        return torch.tanh(torch.einsum("oc,nchw->nohw", self.e, F.avg_pool2d(x, 2)) + 1e-3 * _t4(t))


GAN_ITERS, GAN_EVERY = 4, 2


def _data(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(4, 3, 8, 8, generator=gen) for _ in range(GAN_ITERS)]


def _gan_loop(tmp, resume="", start=0, **over):
    reals = [(x.clamp(-1, 1), {}) for x in _data(77)]
    kw = dict(fake_model=_TinyEnc(2), gan_head=_head(seed=9), real_data=iter(reals[start:]), gen_update_every=GAN_EVERY, gan_gen_weight=0.5,
              gan_dis_weight=0.7)
    kw.update(over)
    return _loop(tmp, resume, **kw)


def _step(tl, k, z):
    torch.manual_seed(2000 + k)
    return tl.run_step(z[k], {})


def test_dmtrainloop_with_head_clocks_save_resume(tmp_path):
    z = _data(99)
    tl = _gan_loop(tmp_path)
    assert len(tl.fake_trainer.master_params) == 3 + 10          # the fake net's (a, b, e) and the head's ten tensors, one trainer
    gens, fakes, heads = {}, {}, {}
    prev = [_flat(m.parameters()).clone() for m in (tl.model, tl.fake_model, tl.gan_head)]
    for k in range(GAN_ITERS):
        took_gen, took_fake = _step(tl, k, z)
        now = [_flat(m.parameters()).clone() for m in (tl.model, tl.fake_model, tl.gan_head)]
        on = k % GAN_EVERY == 0
        assert took_fake and took_gen == on
        assert torch.equal(now[0], prev[0]) != on, k                                   # the generator on its turn only
        assert not torch.equal(now[1], prev[1]) and not torch.equal(now[2], prev[2]), k      # the fake net and the head at every iteration
        assert not torch.equal(tl.fake_model.e.detach(), _TinyEnc(2).e.detach())       # encode's parameter trains through the head alone
        gens[k], fakes[k], heads[k], prev = now[0], now[1], now[2], now
        if tl.step == 2:
            tl.save()
    row = tl.dumpkvs()
    assert {"gan_gen", "gan_dis", "logit_fake", "logit_real", "loss", "dm_norm", "fake_mse"} <= set(row)
    files = set(os.listdir(tmp_path))
    assert {"model000002.pt", "fake_model000002.pt", "fake_opt000002.pt", "gan_head000002.pt"} <= files
    assert list(torch.load(tmp_path / "gan_head000002.pt")) == KEYS
    assert set(torch.load(tmp_path / "fake_model000002.pt")) == {"a", "b", "e"}         # the bare net's keys
    assert torch.equal(torch.cat([v.reshape(-1) for v in torch.load(tmp_path / "gan_head000002.pt").values()]), heads[1])

    tr = _gan_loop(tmp_path, resume=str(tmp_path / "model000002.pt"), start=2)
    assert tr.step == 2 and torch.equal(_flat(tr.gan_head.parameters()), heads[1]) and torch.equal(_flat(tr.fake_model.parameters()), fakes[1])
    for k in (2, 3):
        _step(tr, k, z)
        assert torch.equal(_flat(tr.model.parameters()), gens[k]), k
        assert torch.equal(_flat(tr.fake_model.parameters()), fakes[k]), k
        assert torch.equal(_flat(tr.gan_head.parameters()), heads[k]), k

    # a fake_opt written without a head does not fit a run with one
    plain = tmp_path / "plain"
    tp = _loop(plain, fake_model=_TinyEnc(2), gen_update_every=GAN_EVERY)
    for k in range(2):
        _step(tp, k, z)
    tp.save()
    shutil.copy(tmp_path / "gan_head000002.pt", plain / "gan_head000002.pt")
    with pytest.raises(ValueError, match=r"3 parameters.*trains 13"):
        _gan_loop(plain, resume=str(plain / "model000002.pt"), start=2)
    os.remove(tmp_path / "gan_head000002.pt")
    with pytest.raises(FileNotFoundError, match="gan_head000002"):
        _gan_loop(tmp_path, resume=str(tmp_path / "model000002.pt"), start=2)


# ------------------------------------------------------------------------------------------ the command line
def test_command_line(capsys):
    import cm_train
    a = cm_train.parse_args(["--training_mode", "dm", "--dm_gan", "True", "--synthetic_data", "True"])
    assert a.dm_gan and (a.gan_gen_weight, a.gan_dis_weight, a.gan_max_step_frac) == (3e-3, 1e-2, 1.0)
    a = cm_train.parse_args(["--training_mode", "dm", "--dm_gan", "True", "--data_npz", "x.npz", "--gan_gen_weight", "1e-3",
                             "--gan_dis_weight", "2e-2", "--gan_max_step_frac", "0.5"])
    assert a.data_npz == "x.npz" and (a.gan_gen_weight, a.gan_dis_weight, a.gan_max_step_frac) == (1e-3, 2e-2, 0.5)
    for argv, msg in ((["--training_mode", "dm", "--dm_gan", "True"], "--dm_gan True needs real images"),
                      (["--training_mode", "dm", "--dm_gan", "True", "--synthetic_data", "True", "--dm_objective", "sid"], "SiDA"),
                      (["--training_mode", "dm", "--gan_gen_weight", "1e-3"], "--gan_gen_weight belongs to --dm_gan"),
                      (["--training_mode", "dm", "--gan_dis_weight", "1e-3"], "--gan_dis_weight belongs to --dm_gan"),
                      (["--training_mode", "dm", "--gan_max_step_frac", "0.5"], "--gan_max_step_frac belongs to --dm_gan"),
                      (["--training_mode", "dm", "--dm_gan", "True", "--synthetic_data", "True", "--gan_max_step_frac", "1.5"],
                       "--gan_max_step_frac"),
                      (["--training_mode", "consistency_training", "--synthetic_data", "True", "--dm_gan", "True"],
                       "--dm_gan belongs to --training_mode dm"),
                      (["--training_mode", "dm", "--data_npz", "x.npz"], "--data_npz does not go with --training_mode dm")):
        with pytest.raises(SystemExit):
            cm_train.parse_args(argv)
        assert msg in capsys.readouterr().err, argv


def test_command_line_refusal_as_a_process():
    script = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "cm_train.py")
    import sys
    r = subprocess.run([sys.executable, script, "--training_mode", "dm", "--dm_gan", "True"], capture_output=True, text=True, timeout=300,
                       cwd=os.path.join(ROOT, "diffusion-by-maxentirl_amd"))
    assert r.returncode == 2 and "--dm_gan True needs real images" in r.stderr


# ------------------------------------------------------------------------------------------ host sanitizers
def test_gan_entry_points_under_address_and_ub_sanitizers():
    """`make asan_gan` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_gan.c, a program with its own main, against it and a no-device HIP runtime stub.  Null and misaligned
    pointers, N <= 0, an unsupported C, H outside {4, 8} and a workspace that is too small must each come back as DXMI_EINVAL with
    the message of their check before any launch: no crash, no sanitizer report.  The program runs as a child process; nothing is
    loaded into python.  A host-only build: machines without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_gan"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_gan")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") == 108        # every case of the driver
