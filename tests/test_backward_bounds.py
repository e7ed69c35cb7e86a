"""The backward error bounds (tests/backward_bounds.py) are tight enough to catch the bugs a backward kernel typically has.

CPU only.  Each case builds an fp64 reference, an fp32 computation organised the way the kernel organises it (pixel tiles
summed along split chains, then the splits in order; bf16 operands), and mutants of the reference that model real kernel
bugs.  The checker must accept the fp32 computation and reject every mutant.
"""
import math

import pytest
import torch

from backward_bounds import (BoundError, Checker, U16, attention_blocks_judge, attention_bwd_ref, groupnorm_bwd_ref, wgrad_depth,
                             wgrad_ref)


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


# ------------------------------------------------------------------------------------------ the edge tests' judges
def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def attn_emulate(qkv, do, heads, scale):
    """Attention backward in fp32 with the kernels' rounding points: bf16 o (delta = <dO, o>), bf16 P and dS as the MFMA
    operands, bf16 outputs."""
    N, T, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    q, k, v = (qkv[:, :, i * C:(i + 1) * C].float().reshape(N, T, heads, D).transpose(1, 2) for i in range(3))
    d = do.float().reshape(N, T, heads, D).transpose(1, 2)
    p = torch.softmax(scale * q @ k.transpose(-1, -2), -1)
    o = (p @ v).to(torch.bfloat16).float()
    pb = p.to(torch.bfloat16).float()
    delta = (d * o).sum(-1, keepdim=True)
    ds = (p * (d @ v.transpose(-1, -2) - delta)).to(torch.bfloat16).float()
    dq, dk, dv = scale * ds @ k, scale * ds.transpose(-1, -2) @ q, pb.transpose(-1, -2) @ d
    return torch.cat([t.transpose(1, 2).reshape(N, T, C) for t in (dq, dk, dv)], 2).to(torch.bfloat16)


@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("T", [24, 40, 65, 72, 129, 200, 264, 1032])
def test_attention_tolerance_holds_for_the_rounding_model_at_the_edge_shapes(T, D):
    """The reference side of the edge tests' attention judge: the rounding model alone stays inside 8 u16 per (image, q|k|v,
    head, 128-row block) at every T of tests/test_hip_backward_edges.py, the 1-row block of T = 129 included."""
    g = torch.Generator().manual_seed(T + D)
    N, heads = (1, 1) if T > 300 else (2, 2)
    C = heads * D
    qkv = bf(torch.randn(N, T, 3 * C, generator=g))
    do = bf(torch.randn(N, T, C, generator=g))
    ref, _ = attention_bwd_ref(qkv, do, heads, D ** -0.5)
    ck = Checker()
    worst = attention_blocks_judge(ck, "attn", attn_emulate(qkv, do, heads, D ** -0.5), ref, heads)
    print(f"  T {T} D {D}: worst block rel-L2 / (8 u16) = {worst:.3f}")
    assert worst <= 1.0


def gn_emulate(x, dy, gamma, beta, groups, eps, silu, ss=None):
    """GroupNorm(+FiLM)(+SiLU) backward by fp32 autograd, dx stored as bf16."""
    import torch.nn.functional as F
    N, H, W, C = x.shape
    xf = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ga, be = gamma.float().clone().requires_grad_(True), beta.float().clone().requires_grad_(True)
    s = ss.float().clone().requires_grad_(True) if ss is not None else None
    y = F.group_norm(xf, groups, ga, be, eps)
    if s is not None:
        y = y * (1 + s[:, :C, None, None]) + s[:, C:, None, None]
    y = F.silu(y) if silu else y
    (y * dy.float().permute(0, 3, 1, 2)).sum().backward()
    return xf.grad.permute(0, 2, 3, 1).to(torch.bfloat16), ga.grad, be.grad, s.grad if s is not None else None


@pytest.mark.parametrize("N,H,W,C,G,ss", [(3, 1, 1, 256, 32, False), (2, 2, 2, 256, 32, True), (7, 3, 3, 128, 32, False), (3, 5, 7, 256, 32, True),
                                          (7, 8, 4, 256, 32, False), (3, 10, 20, 192, 32, True), (1, 16, 16, 2048, 32, False)])
def test_groupnorm_bounds_hold_for_fp32_autograd_at_the_edge_shapes(N, H, W, C, G, ss):
    """The reference side of the edge tests' GroupNorm judge: fp32 autograd plus one bf16 store of dx stays inside the
    element-wise bounds at the small, ragged and wide maps of tests/test_hip_backward_edges.py (dx sits close to 1: the bf16
    store alone accounts for up to 1.0 of its bound)."""
    g = torch.Generator().manual_seed(N * H * W + C)
    x = bf(torch.randn(N, H, W, C, generator=g) * 1.5 + 0.25)
    dy = bf(torch.randn(N, H, W, C, generator=g))
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).float().double()
    beta = (0.3 * torch.randn(C, generator=g)).float().double()
    sst = (0.3 * torch.randn(N, 2 * C, generator=g)).float().double() if ss else None
    (dx, dg, db, dss), (Adx, Adg, Adb, Ass) = groupnorm_bwd_ref(x, dy, gamma, beta, G, 1e-5, True, scale_shift=sst)
    edx, edg, edb, edss = gn_emulate(x, dy, gamma, beta, G, 1e-5, True, sst)
    ck = Checker()
    r = [ck.bf16("dx", edx, dx, Adx, H * W * (C // G) + 16), ck.fp32("dgamma", edg, dg, Adg, N * H * W + 16),
         ck.fp32("dbeta", edb, db, Adb, N * H * W + 16)]
    if ss:
        r.append(ck.fp32("dss", edss, dss, Ass, H * W + 16))
    print(f"  {N}x{H}x{W}x{C}: dx {r[0]:.3f}, parameter gradients <= {max(r[1:]):.3f}")
    assert max(r) <= 1.0


def _attn_case(N, T, heads, seed):
    g = torch.Generator().manual_seed(seed)
    C = 64 * heads
    qkv = bf(torch.randn(N, T, 3 * C, generator=g))
    do = bf(torch.randn(N, T, C, generator=g))
    ref, _ = attention_bwd_ref(qkv, do, heads, 0.125)
    return qkv, do, ref, C


def test_planted_stale_query_rows_pass_rel_l2_and_fail_the_block_judge():
    """(a) dq of the last 8 query rows of one (image, head) of a T = 200 batch left stale (zeros): the whole-tensor rel-L2 < 1e-2
    the five-GEMM test judged by accepts it, the per-block judge (last block: rows 128 .. 199) rejects it."""
    N, T, heads = 32, 200, 6
    qkv, do, ref, C = _attn_case(N, T, heads, 11)
    bad = ref.clone()
    bad[N - 1, T - 8:, 64:128] = 0
    old = rel_l2(bad, ref)
    assert old < 1e-2, old
    must_reject(lambda: attention_blocks_judge(Checker(), "attn", bad, ref, heads))
    assert attention_blocks_judge(Checker(), "attn", ref.to(torch.bfloat16), ref, heads) <= 1.0


def test_planted_missing_key_block_passes_rel_l2_and_fails_the_block_judge():
    """(b) one 64-key block (keys 64 .. 127) left out of the dq sum of one query block (rows 128 .. 199) of one (image, head)."""
    N, T, heads = 80, 200, 6
    qkv, do, ref, C = _attn_case(N, T, heads, 12)
    x, d = qkv[N - 1], do[N - 1][:, :64]
    q, k, v = x[:, :64], x[:, C:C + 64], x[:, 2 * C:2 * C + 64]
    p = torch.softmax(0.125 * q @ k.T, -1)
    dp = d @ v.T
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    bad = ref.clone()
    bad[N - 1, 128:200, 0:64] -= 0.125 * ds[128:200, 64:128] @ k[64:128]
    old = rel_l2(bad, ref)
    assert old < 1e-2, old
    must_reject(lambda: attention_blocks_judge(Checker(), "attn", bad, ref, heads))


def _gn_case(N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(N, H, W, C, generator=g) * 1.5 + 0.25)
    dy = bf(torch.randn(N, H, W, C, generator=g))
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).double()
    beta = (0.3 * torch.randn(C, generator=g)).double()
    return x, dy, gamma, beta


def test_planted_missing_image_in_dgamma_fails_the_bound():
    """(c) dgamma missing one image of N = 7.  This fault moves dgamma's own norm by about N^-1/2 (0.3 .. 0.4 here), so the
    rel-L2 < 1e-4 that test_groupnorm_silu_bwd holds dgamma to rejects it as well: the element-wise bound adds nothing for a whole
    missing image.  What only the bound sees is the same fault in ONE channel of a wide layer (one thread's column sum):
    there rel-L2 < 2e-3 (the generic kernels' tolerance) accepts and the bound rejects."""
    N, H, W, C = 7, 4, 4, 64
    x, dy, gamma, beta = _gn_case(N, H, W, C, 13)
    (dx, dg, db, _), (Adx, Adg, Adb, _) = groupnorm_bwd_ref(x, dy, gamma, beta, 32, 1e-6, True)
    (_, dg6, _, _), _ = groupnorm_bwd_ref(x[:6], dy[:6], gamma, beta, 32, 1e-6, True)
    assert rel_l2(dg6, dg) > 1e-4                              # the old judge rejects the whole-image fault too
    must_reject(lambda: Checker().fp32("dgamma", dg6, dg, Adg, N * H * W + 16))
    # one channel of 2048 missing 1/64 of one image's rows
    N, H, W, C = 7, 8, 8, 2048
    x, dy, gamma, beta = _gn_case(N, H, W, C, 14)
    (dx, dg, db, _), (Adx, Adg, Adb, _) = groupnorm_bwd_ref(x, dy, gamma, beta, 32, 1e-5, True)
    xs, dys = x.clone(), dy.clone()
    dys[6, 7, 7, 100] = 0                                     # one pixel of image 6 dropped from channel 100's sums
    (_, dgm, _, _), _ = groupnorm_bwd_ref(xs, dys, gamma, beta, 32, 1e-5, True)
    bad = dg.clone()
    bad[100] = dgm[100]
    assert bad[100] != dg[100] and rel_l2(bad, dg) < 2e-3
    must_reject(lambda: Checker().fp32("dgamma", bad, dg, Adg, N * H * W + 16))


def test_planted_ragged_chunk_with_the_previous_chunks_rows():
    """(d) the dx of the last ragged chunk of a 200-pixel map (rows 134 .. 199: 66 rows) computed from the previous chunk's rows
    (67 .. 132).  With all channels of an image wrong the old rel-L2 < 6e-3 rejects it too; confined to the 8 channels one
    thread owns, in one image of a batch, it passes rel-L2 and fails the element-wise bound."""
    N, H, W, C = 24, 10, 20, 2048
    x, dy, gamma, beta = _gn_case(N, H, W, C, 15)
    (dx, _, _, _), (Adx, _, _, _) = groupnorm_bwd_ref(x, dy, gamma, beta, 32, 1e-5, True)
    dxr, Ar = dx.reshape(N, H * W, C), Adx.reshape(N, H * W, C)
    whole = dxr.clone()
    whole[N - 1, 134:200] = dxr[N - 1, 67:133]
    assert rel_l2(whole, dxr) > 6e-3
    must_reject(lambda: Checker().bf16("dx", whole, dxr, Ar, H * W * (C // 32) + 16))
    bad = dxr.clone()
    bad[N - 1, 134:200, 8] = dxr[N - 1, 67:133, 8]           # one channel of the 8-channel vector
    old = rel_l2(bad, dxr)
    assert old < 4e-3, old
    must_reject(lambda: Checker().bf16("dx", bad, dxr, Ar, H * W * (C // 32) + 16))
    assert Checker().bf16("dx", dxr.to(torch.bfloat16), dxr, Ar, H * W * (C // 32) + 16) <= 1.0


def test_no_shape_hides_a_missing_wgrad_tile_from_the_fp32_rel_l2():
    """(e) one 128-pixel tile missing from one 64 x 64 (co, ci) block of dW.  dW sums P pixels of products of unit variance, so
    the fault is sqrt(128 / P) of the block's norm and sqrt(128 / (P B)) of the tensor's with B blocks: rel-L2 < 1e-4 needs
    P B > 1.28e10, e.g. 5e7 pixels (48 828 images of 32 x 32) at 1024 -> 1024 channels.  No test can build that, so (e) has no
    accept / reject pair and the old fp32 judge stands acquitted here: at 64 images of 32 x 32 both judges reject the fault."""
    g = torch.Generator().manual_seed(16)
    N, H, W, C, Co = 64, 32, 32, 64, 128
    x = bf(torch.randn(N, H, W, C, generator=g))
    dy = bf(torch.randn(N, H, W, Co, generator=g))
    ref, A = wgrad_ref(x, dy, 1)
    bad = ref.clone()
    bad[:64] -= tile_contrib1(x, dy, 300)[:64]
    c = wgrad_depth({"PT": N * H * W // 128, "S": 64, "tile_px": 128})
    assert rel_l2(bad, ref) > 1e-4
    must_reject(lambda: Checker().fp32("wgrad", bad, ref, A, c))


def tile_contrib1(x, dy, t):
    """fp64 contribution of 128-pixel tile t to a 1x1 weight gradient."""
    C, Co = x.shape[3], dy.shape[3]
    xs, ds = x.reshape(-1, C)[t * 128:(t + 1) * 128], dy.reshape(-1, Co)[t * 128:(t + 1) * 128]
    return (ds.T @ xs).reshape(Co, C, 1, 1)


def test_row_blocks_equals_blocks_where_both_apply():
    g = torch.Generator().manual_seed(17)
    a, b = torch.randn(2, 256, 3 * 128, generator=g).double(), torch.randn(2, 256, 3 * 128, generator=g).double()
    blk = lambda d: d.reshape(2, 2, 128, 3, 2, 64).permute(0, 3, 4, 1, 2, 5)
    rb = lambda d: d.reshape(2, 256, 3, 2, 64).permute(0, 2, 3, 1, 4)
    c1, c2 = Checker(), Checker()
    w1 = c1.blocks("x", blk(a + 1e-3 * b), blk(a), 1.0, 4)
    w2 = c2.row_blocks("x", rb(a + 1e-3 * b), rb(a), 1.0, [slice(0, 128), slice(128, 256)])
    assert abs(w1 - w2) <= 1e-12 * w1


# ------------------------------------------------------------------------------------------ the weight-gradient table
def test_wgrad_edge_table_reaches_every_family_reduce_pair_and_condition():
    """Host side of tests/test_hip_backward_edges.py (the plan query needs no device): every row's plan is the (family, reduce)
    it names; the rows reach every pair dxmi_conv2d_wgrad_plan returns over an enumeration of shapes of at most 8 192 pixels
    per launch; every condition of the list is met by its named row; the refused shapes are refused."""
    from dxmi_hip import ops
    import test_hip_backward_edges as E
    have = set()
    for r in E.WGRAD_ROWS:
        plan = E.wgrad_row_plan(ops, r)
        assert (plan["family"], plan["reduce"]) == (r["family"], r["reduce"]), (r["name"], plan)
        have.add((plan["family"], plan["reduce"]))
    reach = set()
    for k in (1, 3):
        for stride in (1, 2):
            for OH in (4, 8, 16, 32, 64):
                for OW in (4, 8, 16, 32, 64):
                    for N in (1, 2, 3, 5, 19, 128):
                        if N * OH * OW > 8192:
                            continue
                        for C0, C1 in ((64, 0), (128, 0), (256, 0), (64, 64), (128, 128), (1024, 0)):
                            for Co in (64, 128, 256, 512, 1024):
                                p = ops.conv2d_wgrad_plan(N, OH * stride, OW * stride, OH, OW, C0, C1, Co, k, stride, k // 2 if stride == 1 else 0)
                                reach.add((p["family"], p["reduce"]))
    assert {f for f, _ in reach} == set(ops.WGRAD_FAMILIES.values())
    assert have == reach, (sorted(reach - have), sorted(have - reach))
    # taps16 needs S >= 64 and Cout * Cin >= 65536: only the 128 x 128 blocks of b128_1x1 leave that many splits
    assert {f for f, r_ in reach if r_ == "taps16"} == {"b128_1x1"} and len(reach) == 22
    for cond, (name, pred) in E.CONDITIONS.items():
        r = E.WGRAD_BY_NAME[name]
        plan = E.wgrad_row_plan(ops, r)
        assert pred(r, plan, E.wgrad_geometry(r, plan)), cond
    for why, a in E.WGRAD_REFUSED:
        with pytest.raises(Exception):
            ops.conv2d_wgrad_plan(*a)
    assert len({r["name"] for r in E.WGRAD_ROWS}) == len(E.WGRAD_ROWS)
