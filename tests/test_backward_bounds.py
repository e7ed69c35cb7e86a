"""The backward error bounds (tests/backward_bounds.py) are tight enough to catch the bugs a backward kernel typically has.

CPU only.  Each case builds an fp64 reference, an fp32 computation organised the way the kernel organises it (pixel tiles
summed along split chains, then the splits in order; bf16 operands), and mutants of the reference that model real kernel
bugs.  The checker must accept the fp32 computation and reject every mutant.
"""
import math

import pytest
import torch

from backward_bounds import BoundError, Checker, U16, attention_bwd_ref, groupnorm_bwd_ref, wgrad_depth, wgrad_ref


def bf(t):
    return t.to(torch.bfloat16).double()


def split_fp32(x, dy, k, tile, S, pad=None):
    """fp32 weight gradient computed the way the kernel sums it: 3x3 / 1x1 columns per pixel tile, split s adds tiles s, s + S,
    ... in order, then the S partials are added in order."""
    from backward_bounds import unfold_nhwc
    if pad is None:
        pad = k // 2
    N, OH, OW, Co = dy.shape
    cols = unfold_nhwc(x.float(), k, 1, pad).permute(0, 2, 1).reshape(N * OH * OW, -1)        # [P, Cin*k*k]
    d = dy.float().reshape(N * OH * OW, Co)
    PT = math.ceil(cols.shape[0] / tile)
    parts = []
    for s in range(S):
        acc = torch.zeros(Co, cols.shape[1], dtype=torch.float32)
        for t in range(s, PT, S):
            acc += d[t * tile:(t + 1) * tile].T @ cols[t * tile:(t + 1) * tile]
        parts.append(acc)
    out = parts[0].clone()
    for p in parts[1:]:
        out += p
    return out.reshape(Co, -1, k, k), parts


def tile_contrib(x, dy, k, tile, t):
    """fp64 contribution of pixel tile t to the weight gradient."""
    from backward_bounds import unfold_nhwc
    N, OH, OW, Co = dy.shape
    cols = unfold_nhwc(x.double(), k, 1, k // 2).permute(0, 2, 1).reshape(N * OH * OW, -1)
    d = dy.double().reshape(N * OH * OW, Co)
    return (d[t * tile:(t + 1) * tile].T @ cols[t * tile:(t + 1) * tile]).reshape(Co, -1, k, k)


def must_reject(fn):
    with pytest.raises(BoundError):
        fn()


def test_wgrad_bound_rejects_tile_split_halo_block_and_source_bugs():
    g = torch.Generator().manual_seed(0)
    N, H, W, C0, C1, Co, k = 3, 16, 16, 64, 64, 128, 3
    x0 = bf(torch.randn(N, H, W, C0, generator=g))
    x1 = bf(torch.randn(N, H, W, C1, generator=g) * 2)
    dy = bf(torch.randn(N, H, W, Co, generator=g))
    x = torch.cat([x0, x1], 3)
    ref, A = wgrad_ref(x, dy, k)
    S, tile = 5, 128
    plan = {"PT": N * H * W // tile, "S": S, "tile_px": tile}
    c = wgrad_depth(plan)
    got, parts = split_fp32(x, dy, k, tile, S)
    ck = Checker()
    assert ck.fp32("wgrad", got, ref, A, c) <= 1.0
    # one 64-pixel half tile left out of the sum
    half = tile_contrib(x, dy, k, 64, 7)
    must_reject(lambda: ck.fp32("wgrad", ref - half, ref, A, c))
    # one split counted twice
    must_reject(lambda: ck.fp32("wgrad", got + parts[2].reshape(got.shape), ref, A, c))
    # the halo of image 1 shifted by one pixel (rows read one column to the right)
    xs = x.clone()
    xs[1] = torch.roll(x[1], 1, dims=1)
    xs[1, :, 0] = 0
    must_reject(lambda: ck.fp32("wgrad", wgrad_ref(xs, dy, k)[0], ref, A, c))
    # two 64-channel blocks of the output swapped
    sw = ref.clone()
    sw[:64], sw[64:128] = ref[64:128], ref[:64]
    must_reject(lambda: ck.fp32("wgrad", sw, ref, A, c))
    # the C1 source read in place of C0
    must_reject(lambda: ck.fp32("wgrad", wgrad_ref(torch.cat([x1, x1], 3), dy, k)[0], ref, A, c))
    # the bias gradient: one tile's column sums left out
    db = dy.reshape(-1, Co).sum(0)
    Ab = dy.abs().reshape(-1, Co).sum(0)
    assert ck.fp32("db", dy.float().reshape(-1, Co).sum(0), db, Ab, c) <= 1.0
    must_reject(lambda: ck.fp32("db", db - dy.reshape(-1, Co)[128:192].sum(0), db, Ab, c))


def test_wgrad_bound_rejects_a_halo_row_shifted_at_one_tile_seam():
    """One 128-pixel tile (4 rows x 32 columns of a 64x64 map) reads the halo row above it one pixel to the left: only the
    ky = 0 taps of that tile's first output row change (32 of the 65 536 pixels of the sum), judged at the chain depth of the
    ImageNet-64 192 -> 192 3x3 weight gradient at batch 16 (S = 28 splits of 512 tiles)."""
    g = torch.Generator().manual_seed(5)
    N, H, W, C, Co, k = 16, 64, 64, 64, 64, 3
    x = bf(torch.randn(N, H, W, C, generator=g))
    dy = bf(torch.randn(N, H, W, Co, generator=g))
    ref, A = wgrad_ref(x, dy, k)
    c = wgrad_depth({"PT": 512, "S": 28, "tile_px": 128})
    ck = Checker()
    got, _ = split_fp32(x, dy, k, 128, 28)
    assert ck.fp32("wgrad", got, ref, A, c) <= 1.0
    n, r0, c0 = 5, 20, 32                                   # the tile: image 5, output rows 20..23, columns 32..63
    dyt = torch.zeros_like(dy[n:n + 1])
    dyt[0, r0:r0 + 4, c0:c0 + 32] = dy[n, r0:r0 + 4, c0:c0 + 32]
    xm = x[n:n + 1].clone()
    xm[0, r0 - 1, 1:] = x[n, r0 - 1, :-1]                    # halo row r0 - 1 read one column to the left
    bug = wgrad_ref(xm, dyt, k)[0] - wgrad_ref(x[n:n + 1], dyt, k)[0]
    assert bug[:, :, 1:].abs().max() == 0                   # only the top tap row is touched
    must_reject(lambda: ck.fp32("wgrad", ref + bug, ref, A, c))


def test_wgrad_bound_rejects_a_dropped_ragged_image_group():
    """8x8 maps: a 128-pixel tile holds two images; with an odd batch the last group is one image plus zero padding."""
    g = torch.Generator().manual_seed(1)
    N, H, W, C, Co, k = 5, 8, 8, 64, 64, 3
    x = bf(torch.randn(N, H, W, C, generator=g))
    dy = bf(torch.randn(N, H, W, Co, generator=g))
    ref, A = wgrad_ref(x, dy, k)
    plan = {"PT": 3, "S": 2, "tile_px": 128}
    c = wgrad_depth(plan)
    ck = Checker()
    got, _ = split_fp32(x, dy, k, 128, 2)
    assert ck.fp32("wgrad", got, ref, A, c) <= 1.0
    must_reject(lambda: ck.fp32("wgrad", wgrad_ref(x[:4], dy[:4], k)[0], ref, A, c))


def test_wgrad_bound_rejects_a_missing_tile_at_training_depth():
    """1x1 weight gradient at a training-step depth (64x64 maps, a 2 048-pixel chain per split): one 64-pixel tile of 16 384
    missing is still out of bound."""
    g = torch.Generator().manual_seed(2)
    N, H, W, C, Co = 4, 64, 64, 64, 64
    x = bf(torch.randn(N, H, W, C, generator=g))
    dy = bf(torch.randn(N, H, W, Co, generator=g))
    ref, A = wgrad_ref(x, dy, 1)
    plan = {"PT": N * H * W // 128, "S": 8, "tile_px": 128}
    c = wgrad_depth(plan)
    ck = Checker()
    got, _ = split_fp32(x, dy, 1, 128, 8)
    assert ck.fp32("wgrad", got, ref, A, c) <= 1.0
    must_reject(lambda: ck.fp32("wgrad", ref - tile_contrib(x, dy, 1, 64, 100), ref, A, c))


def test_groupnorm_bound_rejects_neighbouring_statistics():
    g = torch.Generator().manual_seed(3)
    N, H, W, C, G = 3, 8, 8, 64, 32
    x = bf(torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3)
    dy = bf(torch.randn(N, H, W, C, generator=g))
    gamma = torch.randn(C, generator=g).double()
    beta = torch.randn(C, generator=g).double()
    ss = torch.randn(N, 2 * C, generator=g).double() * 0.3
    (dx, dg, db, dss), (Adx, Adg, Adb, Ass) = groupnorm_bwd_ref(x, dy, gamma, beta, G, 1e-5, True, scale_shift=ss)
    # fp32 computation of the same backward, dx rounded to bf16 as the kernel stores it
    (dx32, dg32, db32, dss32), _ = groupnorm_bwd_ref(x.float(), dy.float(), gamma.float(), beta.float(), G, 1e-5, True, scale_shift=ss.float())
    ck = Checker()
    depth = H * W * (C // G) + 16
    assert ck.bf16("gn_dx", dx32.to(torch.bfloat16), dx, Adx, depth) <= 1.0
    assert ck.fp32("gn_dgamma", dg32, dg, Adg, N * H * W + 16) <= 1.0
    assert ck.fp32("gn_dss", dss32, dss, Ass, H * W + 16) <= 1.0
    # image 1 normalised with image 2's statistics (mean and rstd of the neighbour's groups)
    import torch.nn.functional as F
    xg = x.reshape(N, -1, G, C // G)
    mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
    mean[1], var[1] = mean[2].clone(), var[2].clone()
    xd = x.clone().requires_grad_(True)
    xhat = ((xd.reshape(N, -1, G, C // G) - mean[:, None, :, None]) / (var[:, None, :, None] + 1e-5).sqrt()).reshape(N, H, W, C)
    yn = (xhat * gamma + beta) * (1 + ss[:, None, None, :C]) + ss[:, None, None, C:]
    (F.silu(yn) * dy).sum().backward()
    wrong = dx.clone()
    wrong[1] = xd.grad[1]
    must_reject(lambda: ck.bf16("gn_dx", wrong, dx, Adx, depth))


def test_attention_block_bound_rejects_the_neighbouring_heads_lse():
    g = torch.Generator().manual_seed(4)
    N, T, heads, D = 2, 256, 3, 64
    C = heads * D
    qkv = bf(torch.randn(N, T, 3 * C, generator=g))
    do = bf(torch.randn(N, T, C, generator=g))
    scale = D ** -0.5
    ref, _ = attention_bwd_ref(qkv, do, heads, scale)
    ck = Checker()

    def blocks(d):       # [N, T, 3C] -> (image, q|k|v, head, 128-row block) blocks
        return d.reshape(N, T // 128, 128, 3, heads, D).permute(0, 3, 4, 1, 2, 5)

    # fp32 with bf16 P and dS (the kernel's MFMA operands)
    q, k, v = (qkv[:, :, i * C:(i + 1) * C].float().reshape(N, T, heads, D).transpose(1, 2) for i in range(3))
    o_ = do.float().reshape(N, T, heads, D).transpose(1, 2)
    s = scale * q @ k.transpose(-1, -2)
    lse = torch.logsumexp(s, -1, keepdim=True)

    def bwd(lse):
        p = torch.exp(s - lse)
        pb = p.to(torch.bfloat16).float()
        dv = pb.transpose(-1, -2) @ o_
        dp = o_ @ v.transpose(-1, -2)
        delta = (dp * p).sum(-1, keepdim=True)
        ds = (p * (dp - delta)).to(torch.bfloat16).float()
        dq, dk = scale * ds @ k, scale * ds.transpose(-1, -2) @ q
        return torch.cat([t.transpose(1, 2).reshape(N, T, C) for t in (dq, dk, dv)], 2).to(torch.bfloat16)

    tol = 8 * U16
    assert ck.blocks("attn", blocks(bwd(lse)), blocks(ref), tol, 4) <= 1.0
    bad = lse.clone()
    bad[1, 1, 128:256] = lse[1, 2, 128:256]
    must_reject(lambda: ck.blocks("attn", blocks(bwd(bad)), blocks(ref), tol, 4))


def test_dropout_hash_restatement_matches_the_oracles():
    """backward_bounds.dropout_keep (torch int64) and oracle.unet_small.dropout_keep_mask (numpy) state the same hash."""
    import backward_bounds as bb
    from oracle.unet_small import dropout_keep_mask
    for shp, p, seed in (((3, 8, 8, 64), 0.1, 12345), ((2, 5, 7, 24), 0.5, 0xDEADBEEF), ((1, 4, 4, 8), 0.0, 7)):
        a = bb.dropout_keep(shp, p, seed, "cpu")
        b = dropout_keep_mask((shp[0], shp[3], shp[1], shp[2]), p, seed).permute(0, 2, 3, 1) != 0
        assert torch.equal(a, b)


def test_silu_bwd_bound_holds_for_fp32_torch_and_catches_a_bf16_ulp():
    """The fp32 evaluation of the expression stays inside 16 u32 A on the host; one bf16 ulp on one element does not."""
    import backward_bounds as bb
    g = torch.Generator().manual_seed(0)
    pre, gy = torch.randn(32, 768, generator=g) * 3, torch.randn(32, 768, generator=g)
    ref, A = bb.silu_bwd_ref(pre, gy)
    s = torch.sigmoid(pre)
    got = gy * (s * (1 + pre * (1 - s)))
    c = bb.Checker()
    assert c.fp32("silu_bwd", got, ref, A, 16) < 1.0
    assert float((16 * bb.U32 * A / ref.abs().clamp_min(1e-30)).median()) < 1e-4          # not vacuous
    i = int(ref.abs().argmax())
    bad = got.clone()
    bad.view(-1)[i] *= 1 + 2.0 ** -8
    with pytest.raises(bb.BoundError):
        c.fp32("silu_bwd", bad, ref, A, 16)
