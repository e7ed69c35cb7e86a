"""conv_ws_gn_kernel<16>: a 16x16 map's 3x3 conv whose tile leaves normalised — GroupNorm(+SiLU) applied in place
in the LDS output tile, written INSTEAD of the raw output (dxmi_conv_desc.gn_out with gn_flags bits 1 and 2).

1. bitwise: gn_out == ops.groupnorm_silu(conv2d(..., want_stats=True)) of the same operands (the fused launch adds the same
   partials in the same order and applies the same transform as the two-launch path), and `out` is not touched;
2. accuracy: gn_out element by element against the fp64 GroupNorm(+SiLU) of the fp64 conv under forward_bounds.gn_fused_bound,
   the bound conv_checked states for every fused GroupNorm output (statistics depth = the group size, the raw tensor's error
   propagated through the linearised GroupNorm);
3. shapes outside the scope (Cout 192, 16 channels per group, 32x32 maps, a residual) are declined and run two launches;
4. an image does not depend on the batch it rides in, a launch repeats itself;
5. host only: the new gn_flags bit answers 1 exactly on the scoped shapes; without it every answer is what it was."""
import ctypes
import math

import pytest
import torch

from forward_bounds import EDGE, conv_checked, launch_conv

gpu = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


@pytest.fixture(scope="module")
def small_grids(ops):
    """A handful of images is a small grid: switch off the library's small-grid re-routing (as tests/test_hip_round2_kernels.py),
    so that every case runs the conv_ws family."""
    old = ops.set_tuning("conv_ws_min_tiles", 0)
    yield
    ops.set_tuning("conv_ws_min_tiles", old)


def operands(ops, N, Cin, Cout, seed, H=16):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    return dict(x=torch.randn(N, H, H, Cin, generator=g).to(torch.bfloat16).to(DEV), w=w, pw=ops.pack_conv_weight(w.to(DEV)),
                bias=torch.randn(Cout, generator=g).to(DEV), vec=torch.randn(N, Cout, generator=g).to(DEV),
                gamma=(1 + 0.3 * torch.randn(Cout, generator=g)).to(DEV), beta=(0.3 * torch.randn(Cout, generator=g)).to(DEV))


def two_launches(ops, o, sl, temb, silu):
    """conv with block statistics, then the streaming GroupNorm apply -> (raw, normalised, kernel id of the conv)."""
    groups = o["pw"].Cout // 8
    kw = dict(bias=o["bias"], addvec=o["vec"][sl].contiguous() if temb else None)
    (raw, st), kid = launch_conv(ops, o["x"][sl].contiguous(), o["pw"], want_stats=True, **kw)
    assert st is not None and st.P == 2, "the conv_ws family writes one partial per pixel half of a 16x16 image"
    return raw, ops.groupnorm_silu(raw, o["gamma"], o["beta"], groups=groups, eps=1e-6, silu=silu, stats=(st, None)), kid


def fused(ops, o, sl, temb, silu, judge=False):
    """The fused launch into a canary-filled `out` -> (normalised tensor or None where declined, raw tensor or None, kernel id)."""
    x, groups = o["x"][sl].contiguous(), o["pw"].Cout // 8
    canary = torch.full((x.shape[0], x.shape[1], x.shape[2], o["pw"].Cout), 7.0, dtype=torch.bfloat16, device=DEV)
    kw = dict(bias=o["bias"], addvec=o["vec"][sl].contiguous() if temb else None, out=canary,
              fuse_gn=(o["gamma"], o["beta"], groups, 1e-6, silu, False), gn_ws=True)
    if judge:
        (raw, y), kid = conv_checked(ops, x, o["pw"], o["w"], **kw)
    else:
        (raw, y), kid = launch_conv(ops, x, o["pw"], **kw)
    torch.cuda.synchronize()
    if y is not None:
        assert raw is None and bool((canary == 7.0).all()), "`out` must stay untouched in the instead-of mode"
    return y, raw, kid


# (N, Cin, Cout, temb, silu): 128 channels in are the family's minimum of 4 chunks; Cout 256 = two cout tiles per image.  The last
# two are conv1 of the CIFAR-10 net's 16x16 up blocks (384 / 512 -> 256 over the virtual concat; bits do not depend on the batch)
CASES = [
    (1, 128, 128, True, True),
    (2, 256, 128, False, True),
    (3, 128, 256, True, False),
    (2, 256, 256, False, False),
    (3, 256, 256, True, True),
    (2, 384, 256, True, True),
    (2, 512, 256, True, True),
]


@gpu
@pytest.mark.parametrize("N,Cin,Cout,temb,silu", CASES)
def test_bitwise_and_fp64(ops, small_grids, N, Cin, Cout, temb, silu):
    o = operands(ops, N, Cin, Cout, 1100 + N + Cin + 2 * Cout)
    raw, want, kid2 = two_launches(ops, o, slice(0, N), temb, silu)
    y, _, kid = fused(ops, o, slice(0, N), temb, silu, judge=True)      # element by element against fp64 (conv_fused_gn[ws])
    assert kid == kid2 == 400016, (kid, kid2)
    assert y is not None, "the scoped shape was declined"
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y, want), f"{int((y != want).sum())} of {y.numel()} elements differ from the two-launch path"
    rep = EDGE.report()
    print("conv_fused_gn[ws] worst |err| / bound:", rep.get("conv_fused_gn[ws]"))


@gpu
@pytest.mark.parametrize("N,Cin,Cout", [(3, 128, 256), (2, 256, 128)])
def test_norm_next_rides_on_the_statistics(ops, small_grids, N, Cin, Cout):
    """ops.conv2d(want_stats=True, norm_next=...), the model's call: the launch writes the block statistics AND the normalised
    tensor (both bitwise the two-launch ones), no raw tensor; on a 32x32 map it is the plain want_stats call."""
    o = operands(ops, N, Cin, Cout, 31 + Cin + Cout)
    raw, want, _ = two_launches(ops, o, slice(0, N), True, True)
    _, st = ops.conv2d(o["x"], o["pw"], bias=o["bias"], addvec=o["vec"], want_stats=True)
    (h, sh), kid = launch_conv(ops, o["x"], o["pw"], bias=o["bias"], addvec=o["vec"], want_stats=True,
                               norm_next=(o["gamma"], o["beta"], Cout // 8, 1e-6, True))
    assert kid == 400016 and h is None and sh.P == 2 and sh.normed is not None
    assert torch.equal(sh.normed, want) and torch.equal(sh.buf, st.buf)
    o32 = operands(ops, 2, 128, 128, 5, H=32)
    (h, sh), kid = launch_conv(ops, o32["x"], o32["pw"], bias=o32["bias"], want_stats=True, norm_next=(o32["gamma"], o32["beta"], 16, 1e-6, True))
    assert kid == 400032 and sh.normed is None and sh.P == 8
    assert torch.equal(h, ops.conv2d(o32["x"], o32["pw"], bias=o32["bias"]))


@gpu
def test_second_tile_and_drain_under_the_next_k_loop(ops, small_grids):
    """130 images x 2 cout tiles = 260 tiles on 256 workgroups: four workgroups run a second tile, whose K loop drains the
    first, normalised, tile and whose table fetch refills gamma / beta."""
    N = 130
    o = operands(ops, N, 128, 256, 77)
    raw, want, _ = two_launches(ops, o, slice(0, N), True, True)
    y, _, kid = fused(ops, o, slice(0, N), True, True)
    assert kid == 400016 and y is not None
    assert torch.equal(y, want), f"{int((y != want).sum())} of {y.numel()} elements differ"
    y3, _, _ = fused(ops, o, slice(5, 8), True, True, judge=True)        # three of them against fp64
    assert torch.equal(y3, y[5:8])


@gpu
def test_batch_independent_and_reproducible(ops, small_grids):
    o = operands(ops, 3, 256, 256, 4108)
    full, _, _ = fused(ops, o, slice(0, 3), True, True)
    again, _, _ = fused(ops, o, slice(0, 3), True, True)
    assert torch.equal(full, again)
    for i in range(3):
        one, _, _ = fused(ops, o, slice(i, i + 1), True, True)
        assert torch.equal(one[0], full[i]), i


@gpu
def test_exact_statistics(ops, small_grids):
    """One-hot weights copy input channel c to output channel c.  Image 0 is zero: sums 0, variance 0, so y = beta exactly (SiLU
    off) whatever gamma and rsqrt(eps).  Image 1 holds +v / -v on alternating channels, v = 1 + the group's index: every group's
    sum is exactly 0 and its mean square exactly v^2, so y = +-(v rstd gamma) + beta with rstd = (v^2 + eps)^-1/2: within one
    fp32 rounding of rsqrt, of the product and of the sum, then one bf16 store."""
    N, C = 2, 128
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    v = (1 + torch.arange(C) // 8).double() * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    x = torch.zeros(N, 16, 16, C, dtype=torch.float64)
    x[1] = v
    gamma, beta = torch.linspace(0.5, 2.0, C).to(DEV), torch.linspace(-1.0, 1.0, C).to(DEV)
    (raw, y), kid = launch_conv(ops, x.to(torch.bfloat16).to(DEV), ops.pack_conv_weight(w.to(DEV)),
                                fuse_gn=(gamma, beta, 16, 1e-6, False, False), gn_ws=True)
    assert kid == 400016 and y is not None and raw is None
    assert torch.equal(y[0], beta.to(torch.bfloat16).expand(16, 16, C))
    g64, b64 = gamma.double().cpu(), beta.double().cpu()
    want = v.sign() * (v.abs() / (v * v + 1e-6).sqrt()) * g64 + b64
    err = (y[1].double().cpu() - want).abs()
    bound = 2.0 ** -8 * want.abs() + 8 * 2.0 ** -24 * (g64.abs() + b64.abs())       # half a bf16 ulp, a few fp32 ulps of the terms
    assert bool((err <= bound).all()), float((err / bound).max())


@gpu
@pytest.mark.parametrize("Cin,Cout,groups,H,res", [(128, 192, 24, 16, False), (128, 128, 8, 16, False), (128, 128, 16, 32, False),
                                                  (128, 128, 16, 16, True)])
def test_declined_shapes_run_two_launches(ops, small_grids, Cin, Cout, groups, H, res):
    """Cout 192 (a half-empty cout tile), 16 channels per group, a 32x32 map, a residual: y None, the raw output written by the
    family's plain kernel; the raw C-ABI call with gn_out set is an error."""
    from dxmi_hip import _lib
    o = operands(ops, 2, Cin, Cout, 9 + Cout + groups + H, H=H)
    r = torch.randn(2, H, H, Cout).to(torch.bfloat16).to(DEV) if res else None
    kw = dict(bias=o["bias"], residual=r)
    (raw, y), kid = launch_conv(ops, o["x"], o["pw"], fuse_gn=(o["gamma"], o["beta"], groups, 1e-6, True, False), gn_ws=True, **kw)
    assert y is None and raw is not None and kid == 400000 + min(H, 32)
    assert torch.equal(raw, ops.conv2d(o["x"], o["pw"], **kw))
    d = _lib.ConvDesc()
    yb = torch.empty_like(raw)
    d.in0, d.wpacked, d.out, d.bias = o["x"].data_ptr(), o["pw"].buf.data_ptr(), raw.data_ptr(), o["bias"].data_ptr()
    d.residual = r.data_ptr() if res else None
    d.N, d.IH, d.IW, d.C0, d.C1, d.OH, d.OW, d.Cout = 2, H, H, Cin, 0, H, H, Cout
    d.ksize, d.stride, d.pad = 3, 1, 1
    d.gn_out, d.gn_gamma, d.gn_beta, d.gn_eps, d.gn_groups, d.gn_flags = yb.data_ptr(), o["gamma"].data_ptr(), o["beta"].data_ptr(), 1e-6, groups, 7
    lib = _lib.load()
    assert lib.dxmi_conv2d_gn_fuse_supported(ctypes.byref(d)) == 0
    assert lib.dxmi_conv2d_fwd(ctypes.byref(d), None) != 0
    assert b"GroupNorm" in lib.dxmi_last_error() or b"gn_out" in lib.dxmi_last_error()


def test_fuse_query_host_only():
    """No launch, no device: dxmi_conv2d_gn_fuse_supported over the conv_ws family's shapes.  With gn_flags bit 2 (and bit 1) it
    says 1 exactly for 16x16 maps, Cout % 128 == 0, no residual / mask / upsample; for gn_flags 0 .. 3 it says 0 on all of them,
    as it did before the bit existed."""
    from dxmi_hip import _lib
    lib = _lib.load()
    old = ctypes.c_int(0)
    assert lib.dxmi_get_tuning(b"conv_ws_min_tiles", ctypes.byref(old)) == 0
    assert lib.dxmi_set_tuning(b"conv_ws_min_tiles", 0) == 0
    try:
        def ask(flags, N=4, H=16, Cin=128, Cout=128, groups=None, residual=False, mask=False, upsample=0):
            d = _lib.ConvDesc()
            d.in0, d.wpacked, d.out = 0x1000, 0x2000, 0x3000          # never dereferenced: the query plans, it does not launch
            d.residual = 0x4000 if residual else None
            d.mask_src = 0x5000 if mask else None
            IH = H // 2 if upsample else H
            d.N, d.IH, d.IW, d.C0, d.C1, d.OH, d.OW, d.Cout = N, IH, IH, Cin, 0, H, H, Cout
            d.ksize, d.stride, d.pad, d.upsample = 3, 1, 1, upsample
            d.gn_groups, d.gn_flags = (Cout // 8 if groups is None else groups), flags
            return int(lib.dxmi_conv2d_gn_fuse_supported(ctypes.byref(d))), int(lib.dxmi_conv2d_kernel_id(ctypes.byref(d)))

        scoped = [dict(), dict(Cin=256), dict(Cout=256), dict(Cin=256, Cout=256), dict(N=1), dict(N=260, Cout=256), dict(Cin=512, Cout=384)]
        outside = [dict(Cout=192), dict(Cout=64), dict(groups=8), dict(H=32), dict(H=32, Cout=256), dict(H=64), dict(residual=True),
                   dict(mask=True), dict(upsample=1)]
        for kw in scoped + outside:
            for flags in (0, 1, 2, 3):
                ok, kid = ask(flags, **kw)
                assert ok == 0 and kid // 1000 == 400, (kw, flags, ok, kid)      # the family never served bits 0 / 1 alone
            for flags in (4, 5):                                                # bit 2 without "instead of the raw output"
                assert ask(flags, **kw)[0] == 0, (kw, flags)
            for flags in (6, 7):
                assert ask(flags, **kw)[0] == (1 if kw in scoped else 0), (kw, flags)
        # below the small-grid threshold the shape leaves the family, and the answer with it
        assert lib.dxmi_set_tuning(b"conv_ws_min_tiles", 96) == 0
        assert ask(6, N=4)[0] == 0 and ask(6, N=96)[0] == 1
    finally:
        assert lib.dxmi_set_tuning(b"conv_ws_min_tiles", old.value) == 0
