"""conv_ws_up_kernel (csrc/conv_ws_up.hip): nearest x2 upsample + 3x3 conv with every weight x pixel product computed once.

Every output and the block statistics are judged element by element against fp64 with the bound every forward conv gets
(forward_bounds.conv_call_ref / stats_ref / stats_depth, through conv_checked): the kernel adds the same 9 Cin exact products per
output as conv_ws_kernel, in another order.  Shapes: both map widths of the scope (IW 16 and 8), the smallest channel count
(4 chunks) and 8 chunks, two to four 64-cout tiles, one workgroup tile and two to three tiles per workgroup (the persistent
loop with its drain of the previous tile), every epilogue switch.  One-hot inputs with nine distinct tap values make the
reference exact: a wrong DPP shift direction, a missing zero fill at a row end or a leak across lanes 7 / 8 (IW 8) is a whole
weight off.  The kernel id of the family is unchanged, and shapes the selector declines stay on conv_ws_kernel."""
import pytest
import torch

from forward_bounds import EDGE, conv_checked

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    old = o.set_tuning("conv_ws_min_tiles", 0)          # small grids stay on the wave-specialised family
    yield o
    o.set_tuning("conv_ws_min_tiles", old)
    print("\nworst |err| / bound per kernel family (upsample convs):", EDGE.report())


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


def bf(x):
    return x.to(torch.bfloat16)


def family_id(IW):
    return 400000 + min(2 * IW, 32)


def operands(seed, N, IH, Cin, Cout, bias=False, addvec=False, residual=False, mask=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = bf(rnd(g, N, IH, IH, Cin))
    W = rnd(g, Cout, Cin, 3, 3, scale=(Cin * 9) ** -0.5)
    kw = {"upsample": True}
    if bias:
        kw["bias"] = rnd(g, Cout, scale=0.1)
    if addvec:
        kw["addvec"] = rnd(g, N, 3 * Cout, scale=0.3)[:, Cout:2 * Cout]      # a row-strided slice, as the models' temb rows
    if residual:
        kw["residual"] = bf(rnd(g, N, 2 * IH, 2 * IH, Cout))
    if mask:
        kw["mask_src"] = bf(rnd(g, N, 2 * IH, 2 * IH, Cout))
        kw["mask_slope"] = 0.2
    return x, W, kw


CASES = [
    # IH, Cin, Cout, N, bias, addvec, residual, mask, act, want_stats
    (16, 128, 128, 1, True, False, False, False, 0, False),
    (16, 256, 256, 3, True, True, False, False, 0, True),
    (16, 128, 128, 3, False, False, True, False, 0, True),
    (16, 128, 256, 1, True, False, False, True, 1, False),
    (16, 128, 192, 3, True, False, False, False, 0, True),      # three 64-cout tiles
    (16, 128, 256, 17, True, True, True, False, 0, True),       # 272 tiles on 256 workgroups: some run two
    (8, 128, 128, 1, False, False, False, False, 0, False),
    (8, 256, 256, 3, True, True, False, False, 0, True),
    (8, 128, 128, 3, True, False, True, False, 1, True),
    (8, 128, 256, 1, False, True, False, True, 2, True),
    (8, 128, 192, 1, True, False, True, False, 0, False),
    (8, 128, 256, 129, True, True, True, False, 0, True),       # 516 tiles: two or three per workgroup
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_up_conv_against_fp64(ops, case):
    IH, Cin, Cout, N, bias, addvec, residual, mask, act, want_stats = case
    x, W, kw = operands(hash(case) & 0xffff, N, IH, Cin, Cout, bias, addvec, residual, mask)
    pw = ops.pack_conv_weight(W)
    res, kid = conv_checked(ops, x, pw, W, act=act, want_stats=want_stats, **kw)
    assert kid == family_id(IH)
    if want_stats:
        assert res[1] is not None and res[1].P == (2 * IH) ** 2 // 128


def _one_hot_positions(IW):
    last, mid = IW - 1, IW // 2 - 1
    pos = [(0, 0), (0, last), (last, 0), (last, last),            # corners
           (mid, 0), (mid, last),                                  # columns 0 and IW - 1 of an interior row
           (0, mid), (last, mid),                                  # rows 0 and IH - 1
           (mid, mid), (mid + 1, mid + 1)]
    if IW == 8:
        pos += [(2, 7), (3, 0), (3, 7), (4, 0)]                    # neighbours in one 16-lane block: low-res rows (r, r + 1)
    return pos


@pytest.mark.parametrize("IW", [16, 8])
def test_up_conv_one_hot_borders(ops, IW):
    """One nonzero pixel per image; small-integer pixel values and weights with nine distinct tap values per (cout, cin): every
    product and every fp32 sum is exact, so the bound is the bf16 store alone."""
    Cin, Cout = 128, 128
    pos = _one_hot_positions(IW)
    g = torch.Generator(device=DEV).manual_seed(5 + IW)
    x = torch.zeros(len(pos), IW, IW, Cin, device=DEV)
    for n, (r, s) in enumerate(pos):
        x[n, r, s] = torch.randint(-2, 3, (Cin,), generator=g, device=DEV).float()
    taps = torch.arange(1, 10, device=DEV).float().reshape(1, 1, 3, 3)
    sign = torch.randint(0, 2, (Cout, Cin, 1, 1), generator=g, device=DEV).float() * 2 - 1
    W = taps * sign
    pw = ops.pack_conv_weight(W)
    y, kid = conv_checked(ops, bf(x), pw, W, upsample=True)
    assert kid == family_id(IW)
    # an image's output is nonzero on the 4 x 4 hi-res pixels around (2 r, 2 s) .. (2 r + 1, 2 s + 1) only
    for n, (r, s) in enumerate(pos):
        m = torch.ones(2 * IW, 2 * IW, dtype=torch.bool, device=DEV)
        m[max(2 * r - 1, 0):2 * r + 3, max(2 * s - 1, 0):2 * s + 3] = False
        assert not y[n][m].any(), (n, r, s)


@pytest.mark.parametrize("IW", [16, 8])
def test_up_conv_bitwise(ops, IW):
    """An image's result does not depend on the batch it rides in, and a launch repeats bit for bit (statistics included)."""
    x, W, kw = operands(31 + IW, 3, IW, 256, 256, bias=True, addvec=True, residual=True)
    pw = ops.pack_conv_weight(W)
    y, st = ops.conv2d(x, pw, want_stats=True, **kw)
    y2, st2 = ops.conv2d(x, pw, want_stats=True, **kw)
    assert torch.equal(y, y2) and torch.equal(st.buf, st2.buf)
    for i in range(3):
        one = {k: (v[i:i + 1].contiguous() if torch.is_tensor(v) and v.dim() > 1 else v) for k, v in kw.items()}
        yi, sti = ops.conv2d(x[i:i + 1].contiguous(), pw, want_stats=True, **one)
        assert torch.equal(yi[0], y[i]), i
        assert torch.equal(sti.buf[0], st.buf[i]), i


def test_up_conv_declined_shapes_stay_on_conv_ws(ops):
    """ups == 1 outside the scope (OW = 64; a virtual concat) runs conv_ws_kernel's own upsample path, within the same bound."""
    x, W, kw = operands(77, 1, 32, 128, 128, bias=True)
    _, kid = conv_checked(ops, x, ops.pack_conv_weight(W), W, want_stats=True, **kw)
    assert kid == 400032
    g = torch.Generator(device=DEV).manual_seed(78)
    x0, x1 = bf(rnd(g, 2, 16, 16, 64)), bf(rnd(g, 2, 16, 16, 64))
    W = rnd(g, 128, 128, 3, 3, scale=(128 * 9) ** -0.5)
    _, kid = conv_checked(ops, x0, ops.pack_conv_weight(W), W, in1=x1, upsample=True, bias=rnd(g, 128, scale=0.1))
    assert kid == 400032
