"""The forward error bounds (tests/forward_bounds.py) are tight enough to catch the bugs a forward kernel typically has.

CPU only.  Each case builds the fp64 reference, an fp32 computation organised the way the kernel organises it (bf16 operands,
fp32 accumulation, one bf16 store; one-pass fp32 GroupNorm statistics; bf16 P in attention), and mutants that model real
kernel bugs, judged at the depth of a real census row.  The checker must accept the fp32 computation and reject every mutant.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from backward_bounds import BoundError
from forward_bounds import (LOG2E, FwdChecker, act64, attention_ref, attn_blocks, attn_elem_bound, attn_inputs, attn_max_score,
                            attn_xcd_logical, conv_bound, conv_call_ref, conv_fwd_ref, gn_bound, gn_fwd_plan, gn_ref, linear_ref, lse_bound,
                            stats_depth, stats_ref)
from backward_bounds import U16


def bf(t):
    return t.to(torch.bfloat16).double()


def must_reject(fn):
    with pytest.raises(BoundError):
        fn()


def trunc_bf16(t):
    """bf16 by truncation (round toward zero) instead of round to nearest even."""
    i = t.float().contiguous().view(torch.int32) & ~0xFFFF
    return i.view(torch.float32).double()


# ------------------------------------------------------------------------------------------ conv
def conv_fp32(x, W, bias=None, addvec=None, residual=None, stride=1, pad=1, pad_br=None, act=0):
    """fp32 conv on bf16 operands + fused adds + activation, one round-to-nearest bf16 store (the kernel's arithmetic)."""
    pb = pad if pad_br is None else pad_br
    xn = F.pad(x.float().permute(0, 3, 1, 2), (pad, pb, pad, pb))
    y = F.conv2d(xn, W.float(), stride=stride).permute(0, 2, 3, 1)
    for t in (bias, addvec, residual):
        if t is not None:
            t = t.float()
            y = y + (t[:, None, None, :] if t.dim() == 2 else t)
    return bf(act64(y.double(), act).float())


def _conv_case(g, N, H, W, C0, Co, C1=0, k=3):
    x0 = bf(torch.randn(N, H, W, C0, generator=g))
    x1 = bf(torch.randn(N, H, W, C1, generator=g) * 2) if C1 else None
    x = torch.cat([x0, x1], 3) if C1 else x0
    Wt = bf(torch.randn(Co, C0 + C1, k, k, generator=g) * ((C0 + C1) * k * k) ** -0.5)
    bias = torch.randn(Co, generator=g).double() * 0.1
    return x0, x1, x, Wt, bias


def test_conv_bound_rejects_halo_tile_block_and_store_bugs():
    """Depth of the CIFAR-10 / LSUN 256 -> 256 3x3 rows (K = 2304); tiles of 256 pixels (8 rows x 32 columns of a 32x32 map)."""
    g = torch.Generator().manual_seed(0)
    N, H, W, C, Co = 2, 32, 32, 256, 128
    x, _, _, Wt, bias = _conv_case(g, N, H, W, C, Co)
    av = torch.randn(N, Co, generator=g).double() * 0.3
    ref, A = conv_fwd_ref(x, Wt, bias, av)
    K = C * 9
    bound = conv_bound(ref, A, K, 0)
    ck = FwdChecker()
    got = conv_fp32(x, Wt, bias, av)
    assert ck.within("conv", got, ref, bound) <= 1.0
    # one halo row read one pixel to the left at a single tile seam: image 1, the tile of output rows 8..15 reads input row 7
    xm = x[1:2].clone()
    xm[0, 7, 1:] = x[1, 7, :-1]
    bad = ref.clone()
    bad[1, 8] = conv_fwd_ref(xm, Wt, bias, av[1:2])[0][0, 8]
    must_reject(lambda: ck.within("conv", bad, ref, bound))
    # two 64-cout blocks swapped
    sw = ref.clone()
    sw[..., :64], sw[..., 64:128] = ref[..., 64:128], ref[..., :64]
    must_reject(lambda: ck.within("conv", sw, ref, bound))
    # the addvec row of the neighbouring image
    must_reject(lambda: ck.within("conv", conv_fwd_ref(x, Wt, bias, av.flip(0))[0], ref, bound))
    # the bf16 store truncating instead of rounding to nearest even
    must_reject(lambda: ck.within("conv", trunc_bf16(conv_fwd_ref(x, Wt, bias, av)[0]), ref, bound))


def test_conv_bound_rejects_a_dropped_ragged_tile():
    """Five 8x8 images are 1.25 tiles of 256 pixels: the last tile holds one image and zero padding."""
    g = torch.Generator().manual_seed(1)
    x, _, _, Wt, bias = _conv_case(g, 5, 8, 8, 256, 128)
    ref, A = conv_fwd_ref(x, Wt, bias)
    bound = conv_bound(ref, A, 256 * 9, 0)
    ck = FwdChecker()
    assert ck.within("conv", conv_fp32(x, Wt, bias), ref, bound) <= 1.0
    bad = ref.clone()
    bad[4] = 0
    must_reject(lambda: ck.within("conv", bad, ref, bound))


def test_conv_bound_rejects_a_zero_upper_half_of_the_last_cout_tile():
    """576 couts (ImageNet-64) are 4.5 tiles of 128: the half-empty last tile's upper 32 couts left at zero."""
    g = torch.Generator().manual_seed(2)
    x, _, _, Wt, bias = _conv_case(g, 2, 8, 8, 192, 576)
    ref, A = conv_fwd_ref(x, Wt, bias)
    bound = conv_bound(ref, A, 192 * 9, 0)
    ck = FwdChecker()
    assert ck.within("conv", conv_fp32(x, Wt, bias), ref, bound) <= 1.0
    bad = ref.clone()
    bad[..., 544:] = 0
    must_reject(lambda: ck.within("conv", bad, ref, bound))


def test_conv_bound_rejects_the_wrong_source_and_stride2_padding_side():
    g = torch.Generator().manual_seed(3)
    x0, x1, x, Wt, bias = _conv_case(g, 2, 16, 16, 128, 128, C1=128, k=1)
    ref, A = conv_fwd_ref(x, Wt, bias)
    bound = conv_bound(ref, A, 256, 0)
    ck = FwdChecker()
    assert ck.within("conv1x1", conv_fp32(x, Wt, bias, pad=0), ref, bound) <= 1.0
    must_reject(lambda: ck.within("conv1x1", conv_fwd_ref(torch.cat([x0, x0], 3), Wt, bias)[0], ref, bound))
    # DDPM downsample: 3x3 stride 2, zeros at the bottom / right only (pad 0, pad_br 1); the bug pads top / left
    xs, _, _, Ws, bs = _conv_case(g, 2, 16, 16, 256, 128)
    ref, A = conv_fwd_ref(xs, Ws, bs, stride=2, pad=0, pad_br=1)
    bound = conv_bound(ref, A, 256 * 9, 0)
    assert ck.within("conv_s2", conv_fp32(xs, Ws, bs, stride=2, pad=0, pad_br=1), ref, bound) <= 1.0
    must_reject(lambda: ck.within("conv_s2", conv_fwd_ref(xs, Ws, bs, stride=2, pad=1, pad_br=0)[0], ref, bound))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_whole_tensor_rel_l2_passes_local_faults_the_bound_rejects():
    """The criterion the conv edge tests used alone (rel-L2 < 4e-3 of the whole tensor against an fp32 conv of the same bf16
    operands) against the element-wise bound of conv_call_ref, on 96 images of 32x32, 256 -> 64, 3x3 with bias, a per-image
    vector and a residual.  The honest result (fp32 accumulation, one bf16 store) spends 1.7e-3 of the 4e-3; a stale pixel (one
    pixel of the last image holding its left neighbour's values in every cout) and a missing K chunk (32 input channels left
    out of 4 couts over 7 rows of the last image) fit into the rest, and are hundreds of bounds away element by element."""
    g = torch.Generator().manual_seed(20)
    N, H, Cin, Co = 96, 32, 256, 64
    x = torch.randn(N, H, H, Cin, generator=g).to(torch.bfloat16)
    W = torch.randn(Co, Cin, 3, 3, generator=g) * (Cin * 9) ** -0.5
    bias, av = torch.randn(Co, generator=g), torch.randn(N, Co, generator=g)
    res = torch.randn(N, H, H, Co, generator=g).to(torch.bfloat16)
    Wb = W.to(torch.bfloat16).float()
    conv32 = lambda xx, ww: F.conv2d(xx.float().permute(0, 3, 1, 2), ww, padding=1).permute(0, 2, 3, 1)
    full = conv32(x, Wb) + bias + av[:, None, None, :] + res.float()              # the old reference
    honest = full.to(torch.bfloat16)
    stale = honest.clone()
    stale[N - 1, 16, 16] = honest[N - 1, 16, 15]
    part = conv32(x[N - 1:, 2:11, :, 32:64], Wb[8:12, 32:64])[0, 1:8]              # rows 3..9 from input rows 2..10
    miss = full.clone()
    miss[N - 1, 3:10, :, 8:12] -= part
    miss = miss.to(torch.bfloat16)
    c = conv_call_ref(x, W, None, bias, av, res)
    ck = FwdChecker()
    assert ck.within("conv", honest, c.ref, c.bound) <= 1.0
    for bad in (stale, miss):
        assert rel_l2(honest, full) < rel_l2(bad, full) < 4e-3
        must_reject(lambda: ck.within("conv", bad, c.ref, c.bound))


def test_conv_call_ref_terms():
    """conv_call_ref against direct fp64 restatements: the shared addvec row, the activation mask (and that a dropped mask is
    rejected), zero-stuffed and nearest upsampling, the stem's fp32 image, NCHW fp32 output, unrounded weights."""
    g = torch.Generator().manual_seed(21)
    N, H, C, Co = 2, 8, 32, 16
    x = torch.randn(N, H, H, C, generator=g).to(torch.bfloat16)
    W = torch.randn(Co, C, 3, 3, generator=g) * (C * 9) ** -0.5
    row = torch.randn(Co, generator=g)
    m = torch.randn(N, H, H, Co, generator=g).to(torch.bfloat16)
    Wd = W.to(torch.bfloat16).double()
    conv64 = lambda xx, **kw: F.conv2d(xx.double().permute(0, 3, 1, 2), Wd, **kw).permute(0, 2, 3, 1)
    c = conv_call_ref(x, W, addvec=row, mask_src=m, mask_slope=0.2, act=1)
    slope = float(torch.tensor(0.2, dtype=torch.float32))
    pre = (conv64(x, padding=1) + row.double()) * torch.where(m.double() > 0, 1.0, slope)
    assert torch.allclose(c.ref, act64(pre, 1), rtol=1e-12, atol=1e-12) and c.K == C * 9
    ck = FwdChecker()
    assert ck.within("mask", bf(c.ref.float()), c.ref, c.bound) <= 1.0
    must_reject(lambda: ck.within("mask", bf(act64(conv64(x, padding=1) + row.double(), 1).float()), c.ref, c.bound))
    z = torch.zeros(N, 2 * H, 2 * H, C, dtype=torch.float64)
    z[:, ::2, ::2] = x.double()
    assert torch.allclose(conv_call_ref(x, W, upsample=2, pad=2, pad_br=0).ref, conv64(F.pad(z, (0, 0, 2, 0, 2, 0))), rtol=1e-12, atol=1e-12)
    up = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    assert torch.allclose(conv_call_ref(x, W, upsample=1).ref, conv64(up, padding=1), rtol=1e-12, atol=1e-12)
    c = conv_call_ref(x, W, out_nchw_f32=True)
    assert c.ref.shape == (N, Co, H, H) and torch.equal(c.ref, c.pre.permute(0, 3, 1, 2))
    assert torch.equal(c.bound, conv_bound(c.pre, c.A, c.K, 0, bf16_out=False).permute(0, 3, 1, 2))
    img = torch.randn(N, 3, H, H, generator=g)
    W3 = torch.randn(Co, 3, 3, 3, generator=g) * 27 ** -0.5
    c = conv_call_ref(img, W3)
    assert c.K == 27 and torch.allclose(c.ref, F.conv2d(bf(img), bf(W3), padding=1).permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def test_stats_bound_rejects_a_dropped_partial():
    g = torch.Generator().manual_seed(4)
    o = bf(torch.randn(2, 64, 64, 128, generator=g) + 3)
    P = 32
    parts = o.float().reshape(2, P, -1, 64, 2)
    st = torch.stack([parts.sum((2, 4)), parts.square().sum((2, 4))], -1)      # fp32 partials [N, P, C/2, 2]
    S, Sa = stats_ref(o)
    ck = FwdChecker()
    c = stats_depth(64 * 64, P, 1)
    assert ck.fp32("stats", st.double().sum(1), S, Sa, c) <= 1.0
    must_reject(lambda: ck.fp32("stats", st.double().sum(1) - st[:, 7].double(), S, Sa, c))


# ------------------------------------------------------------------------------------------ GroupNorm
def gn_fp32(x, gamma, beta, groups, eps, silu, ss=None, stats=None):
    """One-pass fp32 statistics (sum and sum of squares), var = q / n - m^2, then the affine, FiLM, SiLU in fp32, bf16 store."""
    xf = x.float()
    N, H, W, C = xf.shape
    g = xf.reshape(N, H * W, groups, C // groups)
    n = H * W * (C // groups)
    s, q = (g.sum((1, 3)), g.square().sum((1, 3))) if stats is None else stats
    m = s / n
    var = q / n - m * m
    rstd = torch.rsqrt(var + eps)
    y = ((g - m[:, None, :, None]) * rstd[:, None, :, None]).reshape(N, H, W, C) * gamma.float() + beta.float()
    if ss is not None:
        y = y * (1 + ss[:, None, None, :C].float()) + ss[:, None, None, C:].float()
    if silu:
        y = F.silu(y)
    return bf(y)


def _gn_x(g, N, H, W, C, cond, G=32):
    """One offset per group, uniform in [-cond, cond], the largest of each image set to cond: (image, group) |mean| / std spreads
    up to cond.  Image 0's first group is zero-mean with a tiny variance, where eps matters."""
    off = (torch.rand(N, G, generator=g) * 2 - 1) * cond
    off[torch.arange(N), off.abs().argmax(1)] = cond
    x = torch.randn(N, H, W, C, generator=g) + off.repeat_interleave(C // G, 1)[:, None, None, :]
    x[0, :, :, :C // G] = 0.003 * torch.randn(H, W, C // G, generator=g)
    return bf(x)


def test_groupnorm_bound_accepts_one_pass_statistics_and_rejects_statistics_bugs():
    """ImageNet-64's 192 channels in 32 groups of 6 on 16x16 maps, with a mean offset (|mean| / std up to ~50), FiLM, SiLU."""
    g = torch.Generator().manual_seed(5)
    N, H, W, C, G, eps = 3, 16, 16, 192, 32, 1e-5
    x = _gn_x(g, N, H, W, C, 50.0)
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).double(), (0.3 * torch.randn(C, generator=g)).double()
    ss = 0.3 * torch.randn(N, 2 * C, generator=g).double()
    yo, parts = gn_ref(x, gamma, beta, G, eps, True, ss)
    assert float((parts["m"].abs() / parts["var"].sqrt()).max()) > 45          # the conditioning really reaches ~50
    d = H * W * C // G + 2
    bound = gn_bound(yo, parts, gamma, beta, d, True)
    ck = FwdChecker()
    assert ck.within("gn", gn_fp32(x, gamma, beta, G, eps, True, ss), yo, bound) <= 1.0
    # image 1 normalised with image 2's statistics
    xf = x.float()
    gg = xf.reshape(N, -1, G, C // G)
    s, q = gg.sum((1, 3)), gg.square().sum((1, 3))
    s2, q2 = s.clone(), q.clone()
    s2[1], q2[1] = s[2], q[2]
    must_reject(lambda: ck.within("gn", gn_fp32(x, gamma, beta, G, eps, True, ss, stats=(s2, q2)), yo, bound))
    # group boundaries off by one channel (groups of 6 read channels 1..6, 7..12, ...)
    sh = torch.roll(x, -1, dims=3)
    bad = torch.roll(gn_ref(sh, gamma.roll(-1), beta.roll(-1), G, eps, True, torch.cat([ss[:, :C].roll(-1, 1), ss[:, C:].roll(-1, 1)], 1))[0], 1, dims=3)
    must_reject(lambda: ck.within("gn", bad, yo, bound))
    # eps 1e-6 in place of 1e-5 (image 0's first group has a tiny variance)
    must_reject(lambda: ck.within("gn", gn_fp32(x, gamma, beta, G, 1e-6, True, ss), yo, bound))
    # the neighbouring image's FiLM scale
    ss_bad = ss.clone()
    ss_bad[1, :C] = ss[2, :C]
    must_reject(lambda: ck.within("gn", gn_fp32(x, gamma, beta, G, eps, True, ss_bad), yo, bound))


def test_groupnorm_bound_rejects_a_dropped_source_share_and_a_dropped_partial():
    """[in0 | in1] with C0 = 64, C1 = 128 in groups of 6: group 10 (channels 60..65) straddles the boundary.  The streaming apply
    with P = 8 statistics partials per source."""
    g = torch.Generator().manual_seed(6)
    N, H, W, C0, C1, G, eps, P = 2, 16, 16, 64, 128, 32, 1e-6, 8
    C = C0 + C1
    x = _gn_x(g, N, H, W, C, 8.0)
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).double(), (0.3 * torch.randn(C, generator=g)).double()
    yo, parts = gn_ref(x, gamma, beta, G, eps, True)
    bound = gn_bound(yo, parts, gamma, beta, P + C // G // 2 + 2, True)
    ck = FwdChecker()
    pix = x.float().reshape(N, P, -1, G, C // G)
    ps, pq = pix.sum((2, 4)), pix.square().sum((2, 4))                        # fp32 partials per group
    assert ck.within("gn_apply", gn_fp32(x, gamma, beta, G, eps, True, stats=(ps.sum(1), pq.sum(1))), yo, bound) <= 1.0
    # partial 3 of every group left out
    must_reject(lambda: ck.within("gn_apply", gn_fp32(x, gamma, beta, G, eps, True,
                                                       stats=(ps.sum(1) - ps[:, 3], pq.sum(1) - pq[:, 3])), yo, bound))
    # the straddling group's in1 share (channels 64, 65) dropped from its statistics
    xf = x.float().reshape(N, H * W, C)
    s, q = ps.sum(1).clone(), pq.sum(1).clone()
    s[:, 10] -= xf[:, :, 64:66].sum((1, 2))
    q[:, 10] -= xf[:, :, 64:66].square().sum((1, 2))
    must_reject(lambda: ck.within("gn_apply", gn_fp32(x, gamma, beta, G, eps, True, stats=(s, q)), yo, bound))


# ------------------------------------------------------------------------------------------ attention
def attention_fp32(qkv, heads, scale, kswap=False):
    """fp32 scores, exp2 with the row max, P rounded to bf16 for P V, fp32 row sums; lse in the log2 domain; bf16 output."""
    N, T, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    q, k, v = (qkv[:, :, i * C:(i + 1) * C].float().reshape(N, T, heads, D).transpose(1, 2) for i in range(3))
    if kswap:
        k = k.roll(1, dims=1)
    s2 = (scale * q @ k.transpose(-1, -2)) * LOG2E
    m = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(-1, keepdim=True)
    o = (p.to(torch.bfloat16).float() @ v) / l
    return bf(o.transpose(1, 2).reshape(N, T, C)), (m + torch.log2(l)).squeeze(-1).double()


def test_attention_bounds_reject_head_and_lse_bugs():
    """T = 256 (16x16 maps), 4 heads of 64 (the ImageNet-64 widths are 64 per head)."""
    g = torch.Generator().manual_seed(7)
    N, T, heads, D = 2, 256, 4, 64
    C = heads * D
    qkv = bf(torch.randn(N, T, 3 * C, generator=g))
    scale = D ** -0.5
    o, lse2, smag = attention_ref(qkv, heads, scale)
    tol = 8 * U16
    ck = FwdChecker()
    got, lse = attention_fp32(qkv, heads, scale)
    assert ck.blocks("attn", attn_blocks(got, heads), attn_blocks(o, heads), tol, 3) <= 1.0
    lb = lse_bound(lse2, smag, D, T)
    assert ck.within("lse2", lse, lse2, lb) <= 1.0
    bad, _ = attention_fp32(qkv, heads, scale, kswap=True)
    must_reject(lambda: ck.blocks("attn", attn_blocks(bad, heads), attn_blocks(o, heads), tol, 3))
    lb_bad = lse.clone()
    lb_bad[1, 2, 128:] = lse[1, 3, 128:]
    must_reject(lambda: ck.within("lse2", lb_bad, lse2, lb))
    must_reject(lambda: ck.within("lse2", lse / LOG2E, lse2, lb))      # natural log instead of log2


def attention_fp32_online(qkv, heads, scale, fault=None, fault_kb=1):
    """attention_kernel<D>'s arithmetic in torch fp32 for any T: key blocks of 64 with a ragged last one, scores scaled into the
    log2 domain, a running maximum with the rescale of l and O per block, l summing the UNROUNDED p, p rounded to bf16 for P V,
    O / l stored as bf16 -> (o [N, T, C], lse2 [N, heads, T]).  fault plants one kernel bug:
      "unmasked"     the first zero-filled key past T of the ragged last block takes part (score 0, value 0)
      "masked_last"  key T - 1 is masked as well
      "l_half"       query 0 of every (image, head): l misses the first 32 keys of the last block (a lost half-wave exchange)
      "skip_rescale" O is not rescaled in key block fault_kb although the maximum moved there (l is)"""
    N, T, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    q, k, v = (qkv[:, :, i * C:(i + 1) * C].float().reshape(N, T, heads, D).transpose(1, 2) for i in range(3))
    sc2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    m = torch.full((N, heads, T, 1), -math.inf)
    l = torch.zeros(N, heads, T, 1)
    o = torch.zeros(N, heads, T, D)
    nkb = -(-T // 64)
    for kb in range(nkb):
        kk, vv = k[:, :, kb * 64:(kb + 1) * 64], v[:, :, kb * 64:(kb + 1) * 64]
        last = kb == nkb - 1
        if last and fault == "unmasked":
            assert kk.shape[2] < 64
            kk, vv = (torch.cat([t, torch.zeros(N, heads, 1, D)], 2) for t in (kk, vv))
        if last and fault == "masked_last":
            kk, vv = kk[:, :, :-1], vv[:, :, :-1]
            if kk.shape[2] == 0:
                break
        s = (q @ kk.transpose(-1, -2)) * sc2
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        p = torch.exp2(s - m_new)
        psum = p.sum(-1, keepdim=True)
        if last and fault == "l_half":
            psum[:, :, 0] -= p[:, :, 0, :32].sum(-1, keepdim=True)
        alpha = torch.exp2(m - m_new)
        l = l * alpha + psum
        if fault == "skip_rescale" and kb == fault_kb:
            assert bool((alpha < 0.5).any())             # the maximum did move in this block
        else:
            o = o * alpha
        o = o + p.to(torch.bfloat16).float() @ vv
        m = m_new
    return bf((o / l).transpose(1, 2).reshape(N, T, C)), (m + torch.log2(l)).squeeze(-1).double()


# (N, T, heads, D, kind): the five shapes the element-wise attention bound was checked on
ATTN_SHAPES = [(2, 200, 2, 64, "gauss"), (2, 200, 2, 64, "below_zero"), (1, 130, 1, 128, "peaked"), (2, 40, 1, 256, "below_zero"),
               (1, 321, 1, 64, "peaked")]


def _attn_case(i):
    N, T, heads, D, kind = ATTN_SHAPES[i]
    qkv = attn_inputs(torch.Generator().manual_seed(30 + i), N, T, heads, D, kind)
    scale = D ** -0.5
    return qkv, heads, scale, attn_elem_bound(qkv, heads, scale)


def _ratio(got, o, bound):
    return float(((got.double() - o).abs() / bound).max())


def test_attention_elem_bound_accepts_the_kernel_arithmetic():
    """The emulation of the kernels' arithmetic stays inside attn_elem_bound on every shape (with margin: worst 0.7 or so), lse
    included; the below-zero inputs keep every true score under -3."""
    ck = FwdChecker()
    for i, (N, T, heads, D, kind) in enumerate(ATTN_SHAPES):
        qkv, heads, scale, (o, lse2, smag, bound) = _attn_case(i)
        got, lse = attention_fp32_online(qkv, heads, scale)
        assert ck.within(f"attn{i}", got, o, bound) <= 1.0
        assert ck.within(f"lse{i}", lse, lse2, lse_bound(lse2, smag, D, T)) <= 1.0
        got1, _ = attention_fp32(qkv, heads, scale)                         # the one-block form (global maximum) as well
        assert ck.within(f"attn{i}_global", got1, o, bound) <= 1.0
        if kind == "below_zero":
            assert attn_max_score(qkv, heads, scale) < -3
    print(ck.report())


def test_attention_elem_bound_rejects_mask_sum_and_rescale_bugs():
    ck = FwdChecker()
    for i in (1, 3):                                                        # below-zero inputs, ragged last block
        qkv, heads, scale, (o, _, _, bound) = _attn_case(i)
        for fault in ("unmasked", "masked_last", "l_half"):
            bad, _ = attention_fp32_online(qkv, heads, scale, fault=fault)
            must_reject(lambda: ck.within(f"attn{i}_{fault}", bad, o, bound))
        assert _ratio(attention_fp32_online(qkv, heads, scale, fault="unmasked")[0], o, bound) > 50
    for i in (2, 4):                                                        # peaked inputs, several key blocks
        qkv, heads, scale, (o, _, _, bound) = _attn_case(i)
        bad, _ = attention_fp32_online(qkv, heads, scale, fault="skip_rescale", fault_kb=1)
        must_reject(lambda: ck.within(f"attn{i}_skip_rescale", bad, o, bound))
    # one query row of a 128-row block scaled by 1.1
    qkv, heads, scale, (o, _, _, bound) = _attn_case(0)
    got, _ = attention_fp32_online(qkv, heads, scale)
    bad = got.clone()
    bad[1, 150] *= 1.1
    must_reject(lambda: ck.within("attn_row", bad, o, bound))


def test_old_attention_measures_pass_faults_the_elem_bound_rejects():
    """What the attention edge tests used alone (whole-tensor rel-L2 < 8e-3) and the program-shape suite's rel-L2 per (image,
    head, 128-row block) within 8 u16, against attn_elem_bound.  (The whole-tensor measure is taken against the fp64 output here;
    the tests took it against torch fp32, which differs from fp64 by 1e-6 of the tolerance.)
      * one query row of 256 scaled by 1.1: both old measures pass it, the bound rejects it;
      * one zero key past T unmasked under Gaussian q, k (T = 200): the whole-tensor measure passes it (about 3e-3) AND SO DOES THE
        BOUND (the denominator moves by 0.3 %, under u16), which is why the ragged cases take below-zero inputs;
      * the same key under below-zero inputs at T = 40, where one block exists: the per-block measure REJECTS it as well (the
        stray key holds nearly all the weight, the block's rel-L2 is close to 1), so no assertion that it passes is made; at
        T = 200 the per-block measure cannot be formed at all (attn_blocks needs T % 128 == 0 or T < 128)."""
    g = torch.Generator().manual_seed(40)
    N, T, heads, D = 2, 256, 4, 64
    qkv = attn_inputs(g, N, T, heads, D, "gauss")
    o, _, _, bound = attn_elem_bound(qkv, heads, D ** -0.5)
    got, _ = attention_fp32_online(qkv, heads, D ** -0.5)
    bad = got.clone()
    bad[1, 77] *= 1.1
    ck = FwdChecker()
    assert ck.within("attn", got, o, bound) <= 1.0
    assert rel_l2(got, o) < rel_l2(bad, o) < 8e-3
    assert ck.blocks("attn_blocks", attn_blocks(bad, heads), attn_blocks(o, heads), 8 * U16, 3) <= 1.0
    must_reject(lambda: ck.within("attn", bad, o, bound))
    # the unmasked key under Gaussian inputs
    qkv, heads, scale, (o, _, _, bound) = _attn_case(0)
    bad, _ = attention_fp32_online(qkv, heads, scale, fault="unmasked")
    assert rel_l2(attention_fp32_online(qkv, heads, scale)[0], o) < rel_l2(bad, o) < 8e-3
    assert _ratio(bad, o, bound) <= 1.0
    # ... and under below-zero inputs: far outside the bound; the per-block measure sees it too where it can be formed
    qkv, heads, scale, (o, _, _, bound) = _attn_case(3)
    bad, _ = attention_fp32_online(qkv, heads, scale, fault="unmasked")
    assert _ratio(bad, o, bound) > 50
    must_reject(lambda: ck.blocks("attn_blocks", attn_blocks(bad, heads), attn_blocks(o, heads), 8 * U16, 3))
    with pytest.raises(RuntimeError):
        attn_blocks(_attn_case(1)[3][0], 2)


def test_attn_xcd_logical_is_a_bijection():
    """The XCD block permutation of csrc/attention.hip (restated in forward_bounds.attn_xcd_logical) maps 0..G-1 onto itself for
    every grid size, and gives the blocks of one XCD (b % 8) consecutive logical ids."""
    for G in range(1, 201):
        ids = [attn_xcd_logical(b, G) for b in range(G)]
        assert sorted(ids) == list(range(G)), G
        for x in range(min(8, G)):
            mine = [attn_xcd_logical(b, G) for b in range(x, G, 8)]
            assert mine == list(range(mine[0], mine[0] + len(mine))), (G, x)


# The plans of the resident GroupNorm forward rows of tests/test_hip_forward_edges.py: (C0, C1, HW, groups) ->
# (VEC, slices, ppp, threads, pieces, ragged, fast, ppt) of dxmi_groupnorm_silu_fwd's slicing walk (the library is not loaded here)
GN_FWD_PLANS = {
    "vec4_cpg4": ((128, 0, 64, 32), (4, 1, 32, 512, 4, False, True, 1)),
    "vec4_c0_132": ((132, 124, 64, 32), (4, 1, 64, 512, 8, False, True, 2)),
    "cpg12_notfast": ((384, 0, 64, 32), (4, 1, 96, 384, 16, False, False, 3)),
    "cpg12_cat_ragged": ((256, 128, 49, 32), (4, 1, 96, 384, 13, True, False, 3)),
    "cpg24_notfast": ((768, 0, 16, 32), (8, 1, 96, 384, 4, False, False, 3)),
    "wide_ppp128_4x4": ((1024, 0, 16, 32), (8, 1, 128, 512, 4, False, False, 4)),
    "wide_ppp128_8x8": ((1024, 0, 64, 32), (8, 1, 128, 512, 16, False, False, 4)),
    "c2048": ((2048, 0, 4, 32), (8, 1, 256, 512, 2, False, False, 8)),
    "map_1x1": ((256, 0, 1, 32), (8, 1, 32, 64, 1, True, True, 1)),
    "map_2x2_cat": ((128, 128, 4, 32), (8, 1, 32, 128, 1, False, True, 1)),
    "map_3x3": ((128, 0, 9, 32), (4, 1, 32, 320, 1, True, True, 1)),
    "ragged_piece": ((256, 0, 35, 32), (8, 1, 32, 512, 3, True, True, 1)),
    "one_group": ((64, 0, 12, 1), (8, 1, 8, 128, 1, True, True, 8)),
    "sliced_vec4_32": ((128, 0, 1024, 32), (4, 2, 16, 512, 32, False, True, 1)),
    "sliced_ragged": ((128, 0, 5000, 32), (4, 16, 2, 512, 20, True, True, 1)),
}


def test_gn_fwd_plan_table_and_refusals():
    keys = ("VEC", "slices", "ppp", "threads", "pieces", "ragged", "fast", "ppt")
    for name, (shape, want) in GN_FWD_PLANS.items():
        plan = gn_fwd_plan(*shape)
        assert plan is not None and tuple(plan[k] for k in keys) == want, (name, plan)
    # 3 and 6 channels per group; a slice whose unit is 576 threads; more than 32 pieces after the last slicing (32 slices of one
    # piece per pixel at 512 threads hold 32 * 512 pixels: 16385 is the smallest map that does not fit, for any channel count)
    for shape in ((96, 0, 100, 32), (192, 0, 64, 32), (288, 0, 16, 8), (128, 0, 16385, 32), (4, 0, 16385, 1)):
        assert gn_fwd_plan(*shape) is None, shape
    assert gn_fwd_plan(128, 0, 16384, 32)["pieces"] == 32 and gn_fwd_plan(4, 0, 16384, 1)["pieces"] == 32


# ------------------------------------------------------------------------------------------ linear
def test_linear_bound_rejects_the_dropped_last_round_of_k_steps():
    """K = 192 (the ImageNet-64 timestep MLP's input) is 12 k16 steps: one round of eight loads in flight plus a partial round
    of four, which the `ks` clamp of linear_small_kernel keeps in range; dropping that partial round loses K 128..191."""
    g = torch.Generator().manual_seed(8)
    P, K, M = 100, 192, 768
    x = torch.randn(P, K, generator=g)
    W = torch.randn(M, K, generator=g) * K ** -0.5
    b = torch.randn(M, generator=g) * 0.1
    for pre, post in ((0, 3), (3, 0)):
        ref, bound = linear_ref(x, W, b, pre, post)
        ck = FwdChecker()
        a = bf(act64(x.double(), pre).float()).float()
        Wb = bf(W).float()
        got = act64((a @ Wb.T + b).double(), post).float()
        assert ck.within("linear", got, ref, bound) <= 1.0
        short = act64((a[:, :128] @ Wb[:, :128].T + b).double(), post)
        must_reject(lambda: ck.within("linear", short, ref, bound))
