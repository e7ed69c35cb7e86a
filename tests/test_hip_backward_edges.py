"""The backward kernels off the program shapes, every launch judged element by element (attention: block by block) against
stock torch in float64 on the same operands, through the helpers of tests/backward_bounds.py that test_hip_backward_shapes.py
uses for the program shapes.  The cases are the tails and routes no program reaches: ragged image groups, chain tails and every
(family, reduce) pair of the weight gradient; ragged pieces, slices and chunks of both GroupNorm backwards, the 256-row-chunk
branch and one channel per group; ragged T in the fused attention backward and the five-GEMM path, the looped softmax kernel.
Every case asserts the plan, family or form it is meant to reach before it launches.  Refusals are asserted through the plan
query (no launch).  test_backward_bounds.py checks WGRAD_ROWS and CONDITIONS on the host.
"""
import math
import zlib

import pytest
import torch

from backward_bounds import (EDGE, U16, U32, attention_bwd_checked, gn_bwd_checked, gn_resident_plan, softmax_bwd_ref, wgrad_checked,
                             wgrad_depth, wgrad_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def bf(t):
    return t.to(torch.bfloat16)


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


def gen(key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------ weight gradient
def W(name, N, IH, IW, OH, OW, C0, C1, Co, k, family, reduce, stride=1, pad=None, ups=False, bias=False, old=False):
    return dict(name=name, N=N, IH=IH, IW=IW, OH=OH, OW=OW, C0=C0, C1=C1, Co=Co, k=k, family=family, reduce=reduce, stride=stride,
                pad=k // 2 if pad is None else pad, ups=ups, bias=bias, old=old)


WGRAD_ROWS = [
    # ragged image groups: SUBS images share a 128-pixel tile, the last group is short
    W("rag2", 5, 8, 8, 8, 8, 128, 0, 128, 3, "ws3", "flat4", bias=True, old=True),
    W("rag8", 19, 4, 4, 4, 4, 128, 0, 128, 3, "reg3", "flat4", bias=True),
    W("rag4_8x4", 3, 8, 4, 8, 4, 128, 0, 128, 3, "reg3_pf", "flat4"),
    W("rag4_4x8", 3, 4, 8, 4, 8, 128, 0, 128, 3, "ws3", "flat4", old=True),
    W("rag2_cat", 5, 8, 8, 8, 8, 64, 64, 128, 3, "ws3", "flat4"),
    W("rag8_cat_1x1", 19, 4, 4, 4, 4, 64, 128, 128, 1, "reg1_pf", "flat4", bias=True),
    W("rag4_cat", 3, 4, 8, 4, 8, 128, 64, 64, 3, "ws3", "flat4"),
    W("rag4_8x4_1x1", 3, 8, 4, 8, 4, 64, 0, 128, 1, "reg1_pf", "flat4"),
    W("rag4_4x8_1x1", 3, 4, 8, 4, 8, 64, 0, 128, 1, "ws1", "flat4"),
    W("rag2_ups", 5, 4, 4, 8, 8, 128, 0, 128, 3, "ws3", "flat4", ups=True),
    W("rag2_ups_cat", 3, 4, 4, 8, 8, 64, 64, 128, 3, "ws3", "flat4", ups=True),
    # chain tails
    W("chain_tail", 9, 16, 16, 16, 16, 256, 0, 256, 3, "ws3", "taps4"),
    W("one_split_3x3", 3, 8, 8, 8, 8, 1024, 0, 1024, 3, "ws3", "taps4"),
    W("one_split_1x1", 3, 8, 8, 8, 8, 1472, 0, 1472, 1, "ws1", "taps4"),
    # reduce variants: every (family, reduce) pair the plan can return
    W("flat16_ws3", 8, 32, 32, 32, 32, 64, 0, 64, 3, "ws3", "flat16"),
    W("flat16_ws1", 8, 32, 32, 32, 32, 64, 0, 64, 1, "ws1", "flat16", old=True),
    W("taps16_b128", 16, 16, 16, 16, 16, 256, 0, 256, 1, "b128_1x1", "taps16", bias=True, old=True),
    W("flat16_reg3_pf", 128, 16, 4, 16, 4, 64, 0, 64, 3, "reg3_pf", "flat16"),
    W("flat16_reg1_pf", 128, 16, 4, 16, 4, 64, 0, 64, 1, "reg1_pf", "flat16"),
    W("flat16_reg3", 128, 8, 32, 4, 16, 64, 0, 64, 3, "reg3", "flat16", stride=2, pad=0),
    W("flat16_reg1", 128, 8, 32, 4, 16, 64, 0, 64, 1, "reg1", "flat16", stride=2, pad=0),
    W("flat16_b128", 128, 4, 8, 4, 8, 128, 0, 128, 1, "b128_1x1", "flat16"),
    W("flat4_b128", 3, 8, 8, 8, 8, 128, 0, 128, 1, "b128_1x1", "flat4", bias=True),
    W("taps4_b128", 3, 8, 8, 8, 8, 128, 0, 512, 1, "b128_1x1", "taps4"),
    W("taps4_reg3", 2, 4, 4, 4, 4, 64, 0, 1024, 3, "reg3", "taps4"),
    W("taps4_reg1_pf", 2, 4, 4, 4, 4, 64, 0, 1024, 1, "reg1_pf", "taps4"),
    W("taps4_reg3_pf", 3, 8, 4, 8, 4, 64, 0, 1024, 3, "reg3_pf", "taps4", old=True),
    W("taps4_reg1", 2, 8, 8, 4, 4, 64, 0, 1024, 1, "reg1", "taps4", stride=2, pad=0),
    # channel counts: multiples of 64 that are no multiples of 128; concats
    W("c192_320", 3, 16, 16, 16, 16, 192, 0, 320, 3, "ws3", "flat4", bias=True),
    W("c320_576", 3, 8, 8, 8, 8, 320, 0, 576, 3, "ws3", "taps4"),
    W("c576_192_1x1", 3, 16, 16, 16, 16, 576, 0, 192, 1, "ws1", "taps4"),
    W("cat_off_b128", 4, 16, 16, 16, 16, 192, 64, 256, 1, "ws1", "taps4", bias=True),
    W("cat_equal_b128", 4, 16, 16, 16, 16, 128, 128, 256, 1, "b128_1x1", "taps4"),
    W("cat_small_first", 4, 16, 16, 16, 16, 64, 192, 256, 1, "ws1", "taps4"),
    # non-square maps
    W("m32x16", 3, 32, 16, 32, 16, 64, 0, 128, 3, "ws3", "flat4"),
    W("m16x32", 3, 16, 32, 16, 32, 64, 0, 128, 3, "ws3", "flat4"),
    W("m64x4", 3, 64, 4, 64, 4, 64, 0, 128, 3, "reg3_pf", "flat4"),
    W("m4x64", 3, 4, 64, 4, 64, 64, 0, 128, 3, "ws3", "flat4"),
    W("m32x16_1x1", 3, 32, 16, 32, 16, 64, 0, 128, 1, "ws1", "flat4"),
    W("m16x32_1x1", 3, 16, 32, 16, 32, 128, 0, 128, 1, "b128_1x1", "flat4"),
    W("m64x4_1x1", 3, 64, 4, 64, 4, 64, 0, 128, 1, "reg1_pf", "flat4"),
    W("m4x64_1x1", 3, 4, 64, 4, 64, 64, 0, 128, 1, "ws1", "flat4"),
    # stride 2 on a non-square map with an odd batch: the programs' padding (0: the zeros are right / below) and the symmetric 1
    W("s2_pad0", 3, 32, 16, 16, 8, 128, 0, 128, 3, "reg3", "flat4", stride=2, pad=0, bias=True),
    W("s2_pad1", 3, 32, 16, 16, 8, 128, 0, 128, 3, "reg3", "flat4", stride=2, pad=1),
    W("s2_1x1", 3, 32, 16, 16, 8, 128, 0, 128, 1, "reg1", "flat4", stride=2, pad=0, old=True),
    # the XCD block remap (maps of >= 256 pixels) from both sides of its threshold, grid no multiple of 8
    W("xcd_on", 3, 16, 16, 16, 16, 192, 0, 192, 3, "ws3", "flat4"),
    W("xcd_off", 3, 16, 8, 16, 8, 192, 0, 192, 3, "ws3", "flat4"),
]
WGRAD_BY_NAME = {r["name"]: r for r in WGRAD_ROWS}


def wgrad_row_plan(ops, r):
    return ops.conv2d_wgrad_plan(r["N"], r["IH"], r["IW"], r["OH"], r["OW"], r["C0"], r["C1"], r["Co"], r["k"], r["stride"], r["pad"], r["ups"])


def wgrad_geometry(r, plan):
    """The tile geometry wgrad_plan derives from the shape (csrc/conv_wgrad.hip): images per 128-pixel tile, 64- or 128-channel
    block counts, the split count the chip asks for before the clamp to PT, the launch grid."""
    TW = min(r["OW"], 32)
    TH = min(128 // TW, r["OH"])
    subs = 128 // (TW * TH)
    b128 = plan["family"] == "b128_1x1"
    cb = 128 if b128 else 64
    blocks = ((r["C0"] + r["C1"]) // cb) * (r["Co"] // cb)
    want = max(1, (256 if (b128 or r["k"] == 3) else 512) // blocks)
    return dict(subs=subs, blocks=blocks, want=want, grid=plan["S"] * blocks, xcd=r["OH"] * r["OW"] >= 256)


DMA, REG = ("ws3", "ws1"), ("reg3", "reg3_pf", "reg1", "reg1_pf")
# condition a row must meet -> (the row that meets it, predicate over (row, plan, geometry))
CONDITIONS = {
    "ragged group, 2 images per tile": ("rag2", lambda r, p, g: g["subs"] == 2 and r["N"] % 2),
    "ragged group, 8 images per tile": ("rag8", lambda r, p, g: g["subs"] == 8 and r["N"] % 8),
    "ragged group, 4 images per tile, 8x4": ("rag4_8x4", lambda r, p, g: g["subs"] == 4 and r["N"] % 4 and (r["OH"], r["OW"]) == (8, 4)),
    "ragged group, 4 images per tile, 4x8": ("rag4_4x8", lambda r, p, g: g["subs"] == 4 and r["N"] % 4 and (r["OH"], r["OW"]) == (4, 8)),
    "ragged group with a concat": ("rag2_cat", lambda r, p, g: g["subs"] == 2 and r["N"] % 2 and r["C1"]),
    "ragged group with upsample from 4x4": ("rag2_ups", lambda r, p, g: r["ups"] and r["IH"] == 4 and r["N"] % g["subs"]),
    "ragged group with upsample and a concat": ("rag2_ups_cat", lambda r, p, g: r["ups"] and r["C1"] and r["N"] % g["subs"]),
    "PT % S != 0": ("chain_tail", lambda r, p, g: p["PT"] % p["S"] != 0 and p["S"] > 1),
    "S clamped to PT": ("rag2", lambda r, p, g: p["S"] == p["PT"] < g["want"]),
    "S == 1, 3x3": ("one_split_3x3", lambda r, p, g: p["S"] == 1 and p["PT"] > 1 and r["k"] == 3 and g["blocks"] >= 256),
    "S == 1, 1x1 off b128": ("one_split_1x1", lambda r, p, g: p["S"] == 1 and p["PT"] > 1 and r["k"] == 1 and g["blocks"] >= 512
                             and p["family"] != "b128_1x1"),
    "flat16 at 64 -> 64, 8 x 32x32": ("flat16_ws3", lambda r, p, g: p["reduce"] == "flat16" and (r["N"], r["OH"], r["C0"], r["Co"]) == (8, 32, 64, 64)),
    "taps16 on b128 with >= 4096 pixels": ("taps16_b128", lambda r, p, g: p["reduce"] == "taps16" and p["family"] == "b128_1x1"
                                           and r["N"] * r["OH"] * r["OW"] >= 4096 and (r["C0"], r["Co"]) == (256, 256)),
    "flat4 DMA-staged": ("rag2", lambda r, p, g: p["reduce"] == "flat4" and p["family"] in DMA),
    "flat4 register-staged": ("rag8", lambda r, p, g: p["reduce"] == "flat4" and p["family"] in REG),
    "taps4 DMA-staged": ("chain_tail", lambda r, p, g: p["reduce"] == "taps4" and p["family"] in DMA),
    "taps4 register-staged": ("taps4_reg3", lambda r, p, g: p["reduce"] == "taps4" and p["family"] in REG),
    "192 channels": ("c192_320", lambda r, p, g: r["C0"] == 192 and r["Co"] % 128),
    "320 channels": ("c320_576", lambda r, p, g: r["C0"] == 320 and r["Co"] % 128),
    "576 channels": ("c576_192_1x1", lambda r, p, g: r["C0"] == 576 and r["Co"] % 128),
    "1x1 concat with C0 % 128 != 0 leaves b128 for ws1": ("cat_off_b128", lambda r, p, g: r["k"] == 1 and r["C0"] % 128 and r["C1"] and
                                                          (r["C0"] + r["C1"]) % 128 == 0 and r["Co"] % 128 == 0 and p["family"] == "ws1"),
    "concat C0 > C1": ("cat_off_b128", lambda r, p, g: r["C0"] > r["C1"] > 0),
    "concat C0 < C1": ("cat_small_first", lambda r, p, g: 0 < r["C0"] < r["C1"]),
    "concat C0 == C1": ("cat_equal_b128", lambda r, p, g: r["C0"] == r["C1"]),
    "32x16": ("m32x16", lambda r, p, g: (r["OH"], r["OW"]) == (32, 16)),
    "16x32": ("m16x32", lambda r, p, g: (r["OH"], r["OW"]) == (16, 32)),
    "8x4": ("rag4_8x4", lambda r, p, g: (r["OH"], r["OW"]) == (8, 4)),
    "4x8": ("rag4_4x8", lambda r, p, g: (r["OH"], r["OW"]) == (4, 8)),
    "64x4": ("m64x4", lambda r, p, g: (r["OH"], r["OW"]) == (64, 4)),
    "4x64": ("m4x64", lambda r, p, g: (r["OH"], r["OW"]) == (4, 64)),
    "32x16 1x1": ("m32x16_1x1", lambda r, p, g: (r["OH"], r["OW"], r["k"]) == (32, 16, 1)),
    "16x32 1x1": ("m16x32_1x1", lambda r, p, g: (r["OH"], r["OW"], r["k"]) == (16, 32, 1)),
    "64x4 1x1": ("m64x4_1x1", lambda r, p, g: (r["OH"], r["OW"], r["k"]) == (64, 4, 1)),
    "4x64 1x1": ("m4x64_1x1", lambda r, p, g: (r["OH"], r["OW"], r["k"]) == (4, 64, 1)),
    "stride 2, pad 0, non-square, odd N": ("s2_pad0", lambda r, p, g: r["stride"] == 2 and r["pad"] == 0 and r["OH"] != r["OW"] and r["N"] % 2 and r["k"] == 3),
    "stride 2, pad 1, non-square, odd N": ("s2_pad1", lambda r, p, g: r["stride"] == 2 and r["pad"] == 1 and r["OH"] != r["OW"] and r["N"] % 2 and r["k"] == 3),
    "stride-2 1x1": ("s2_1x1", lambda r, p, g: r["stride"] == 2 and r["k"] == 1),
    "XCD remap on, grid % 8 != 0": ("xcd_on", lambda r, p, g: g["xcd"] and r["OH"] * r["OW"] == 256 and g["grid"] % 8),
    "XCD remap off, grid % 8 != 0": ("xcd_off", lambda r, p, g: not g["xcd"] and r["OH"] * r["OW"] == 128 and g["grid"] % 8),
    "with_bias on a ragged case": ("rag8", lambda r, p, g: r["bias"] and r["N"] % g["subs"]),
    "accumulate into a random tensor": ("rag2", lambda r, p, g: r["old"]),
}

WGRAD_REFUSED = [
    # (N, IH, IW, OH, OW, C0, C1, Cout, k, stride, pad)
    ("OH no power of two", (2, 12, 8, 12, 8, 64, 0, 64, 3, 1, 1)),
    ("OW no power of two", (2, 8, 12, 8, 12, 64, 0, 64, 3, 1, 1)),
    ("OH below 4", (2, 2, 8, 2, 8, 64, 0, 64, 3, 1, 1)),
    ("OW below 4", (2, 8, 2, 8, 2, 64, 0, 64, 3, 1, 1)),
    ("Cin no multiple of 64", (2, 8, 8, 8, 8, 96, 0, 64, 3, 1, 1)),
    ("C0 no multiple of 64 in a concat", (2, 8, 8, 8, 8, 32, 96, 64, 3, 1, 1)),
    ("Cout no multiple of 64", (2, 8, 8, 8, 8, 64, 0, 96, 3, 1, 1)),
    ("stride 3", (2, 24, 24, 8, 8, 64, 0, 64, 3, 3, 1)),
    ("ksize 5", (2, 8, 8, 8, 8, 64, 0, 64, 5, 1, 2)),
]


@pytest.mark.parametrize("r", WGRAD_ROWS, ids=lambda r: r["name"])
def test_wgrad_edges(ops, r):
    plan = wgrad_row_plan(ops, r)
    assert (plan["family"], plan["reduce"]) == (r["family"], r["reduce"]), plan
    geo = wgrad_geometry(r, plan)
    for cond, (name, pred) in CONDITIONS.items():
        if name == r["name"]:
            assert pred(r, plan, geo), cond
    g = gen(r["name"])
    x0 = bf(rnd(g, r["N"], r["IH"], r["IW"], r["C0"]))
    x1 = bf(rnd(g, r["N"], r["IH"], r["IW"], r["C1"], scale=2.0)) if r["C1"] else None
    dy = bf(rnd(g, r["N"], r["OH"], r["OW"], r["Co"]))
    # the tensor accumulated into is random and as large as dW itself (|dW| ~ sqrt(pixels)), so neither summand hides the other
    old = rnd(g, r["Co"], r["C0"] + r["C1"], r["k"], r["k"], scale=math.sqrt(r["N"] * r["OH"] * r["OW"])) if r["old"] else None
    dw, db, _ = wgrad_checked(ops, x0, dy, r["k"], in1=x1, pad=r["pad"], stride=r["stride"], upsample=r["ups"], with_bias=r["bias"], old=old)
    again = ops._conv2d_wgrad(x0, dy, r["k"], in1=x1, pad=r["pad"], stride=r["stride"], upsample=r["ups"])
    assert torch.equal(dw, again), "the weight gradient is not bitwise reproducible"


@pytest.mark.parametrize("why,a", WGRAD_REFUSED, ids=[w for w, _ in WGRAD_REFUSED])
def test_wgrad_refusals_through_the_plan_query(ops, why, a):
    """Shapes the library rejects: asserted through the return code of dxmi_conv2d_wgrad_plan (the launch decides through the
    same function); nothing is launched."""
    import ctypes
    out = (ctypes.c_int32 * 4)()
    N, IH, IW, OH, OW, C0, C1, Co, k, stride, pad = a
    rc = ops.load().dxmi_conv2d_wgrad_plan(N, IH, IW, OH, OW, C0, C1, Co, k, stride, pad, 0, out)
    assert rc != 0, why
    with pytest.raises(Exception):
        ops.conv2d_wgrad_plan(N, IH, IW, OH, OW, C0, C1, Co, k, stride, pad)


@pytest.mark.parametrize("N,H,Wd,Co", [(3, 32, 16, 128), (5, 16, 32, 64), (1, 8, 64, 192)])
def test_stem_conv_wgrad_odd_batch_non_square(ops, N, H, Wd, Co):
    g = gen(("stem", N, H, Wd, Co))
    x = rnd(g, N, 3, H, Wd)
    dy = bf(rnd(g, N, H, Wd, Co))
    got = ops.stem_conv_wgrad(x, dy)
    ref, A = wgrad_ref(bf(x).permute(0, 2, 3, 1), dy, 3)        # the im2col operand is the bf16-rounded image
    plan = ops.conv2d_wgrad_plan(N, H, Wd, H, Wd, 64, 0, Co, 1)
    EDGE.fp32("stem_wgrad", got, ref, A, wgrad_depth(plan))
    assert torch.equal(got, ops.stem_conv_wgrad(x, dy))


@pytest.mark.parametrize("need_dx", [True, False])
@pytest.mark.parametrize("P", [1, 5, 100, 130])
def test_linear_bwd_ragged_rows(ops, P, need_dx):
    """linear_bwd pads its rows to 64 * 2^k (64, 64, 128, 256 here) for the 1x1 weight gradient; K and M are multiples of 64
    that are no multiples of 128."""
    K, M = 192, 320
    g = gen(("linear_bwd", P))
    x, dy = rnd(g, P, K), rnd(g, P, M, scale=0.1)
    Wt = rnd(g, M, K, scale=K ** -0.5)
    pw_t = ops.pack_conv_weight(Wt, transpose_flip=True) if need_dx else None
    dx, dw, db = ops.linear_bwd(x, dy, pw_t, need_dx=need_dx)
    xb, dyb = bf(x).double(), bf(dy).double()
    rows = 64
    while rows < P:
        rows *= 2
    assert rows == {1: 64, 5: 64, 100: 128, 130: 256}[P]
    plan = ops.conv2d_wgrad_plan(1, rows // 16, 16, rows // 16, 16, K, 0, M, 1)
    assert plan["family"] != "b128_1x1"
    EDGE.fp32("linear_bwd_dw", dw, dyb.T @ xb, dyb.abs().T @ xb.abs(), wgrad_depth(plan))
    assert tuple(db.shape) == (M,)
    torch.testing.assert_close(db.double(), dy.double().sum(0), rtol=0, atol=float((P + 2) * U32 * dy.double().abs().sum(0).max()))
    if need_dx:
        Wb = bf(Wt).double()
        EDGE.fp32("linear_bwd_dx", dx, dyb @ Wb, dyb.abs() @ Wb.abs(), 2 * M + 2)
    else:
        assert dx is None


# ------------------------------------------------------------------------------------------ GroupNorm backward
def gn_operands(key, N, H, Wd, C0, C1, add0, add1, ss):
    g = gen(key)
    C = C0 + C1
    x0 = bf(rnd(g, N, H, Wd, C0) * 1.5 + 0.25)
    x1 = bf(rnd(g, N, H, Wd, C1)) if C1 else None
    dy = bf(rnd(g, N, H, Wd, C))
    gamma, beta = 1 + 0.3 * rnd(g, C), 0.3 * rnd(g, C)
    a0 = bf(rnd(g, N, H, Wd, C0)) if add0 else None
    a1 = bf(rnd(g, N, H, Wd, C1)) if add1 else None
    sst = (0.3 * rnd(g, N, 3 * C))[:, C // 2: C // 2 + 2 * C] if ss else None        # a row-strided slice, as emb_all's
    return x0, x1, dy, gamma, beta, a0, a1, sst


RESIDENT = [
    # (name, N, H, W, C0, C1, groups, add0, add1, silu, what the shape must be in the resident kernel's plan)
    ("vec4_cpg4", 7, 8, 8, 128, 0, 32, True, False, True, lambda p: p["VEC"] == 4),
    ("vec4_c0_132", 1, 8, 8, 132, 124, 32, False, True, True, lambda p: p["VEC"] == 4),
    ("map_1x1", 3, 1, 1, 256, 0, 32, False, False, True, lambda p: p["pieces"] == 1 and p["threads"] == 64 and 1 * p["ppp"] < p["threads"]),
    ("map_2x2", 2, 2, 2, 128, 128, 32, True, True, True, lambda p: 4 * p["ppp"] < 512 and p["threads"] < 512),
    ("map_3x3", 7, 3, 3, 128, 0, 32, False, False, False, lambda p: 9 * p["ppp"] < 512 and p["threads"] < 512),
    ("ragged_piece", 3, 5, 7, 256, 0, 32, True, False, True, lambda p: p["slices"] == 1 and (35 * p["ppp"]) % p["threads"] != 0 and p["pieces"] > 1),
    ("two_slices_ragged", 2, 10, 20, 256, 0, 32, False, False, True, lambda p: p["slices"] == 2 and (200 * p["ppp"]) % p["threads"] != 0),
    ("four_slices", 1, 16, 16, 256, 256, 32, False, True, True, lambda p: p["slices"] >= 2),
    ("no_silu_cat", 7, 8, 4, 64, 192, 32, True, True, False, lambda p: p["VEC"] == 8),
]


@pytest.mark.parametrize("c", RESIDENT, ids=[c[0] for c in RESIDENT])
def test_groupnorm_resident_bwd_edges(ops, c):
    name, N, H, Wd, C0, C1, groups, add0, add1, silu, pred = c
    assert ops.load().dxmi_groupnorm_silu_bwd_supported(C0, C1, H * Wd, groups) == 1
    assert not ((C0 + C1) // groups == 12 and H * Wd >= 256)
    plan = gn_resident_plan(C0, C1, H * Wd, groups)
    assert plan is not None and plan["pieces"] <= 16 and pred(plan), plan
    x0, x1, dy, gamma, beta, a0, a1, _ = gn_operands(c[:7], N, H, Wd, C0, C1, add0, add1, False)
    out = gn_bwd_checked(ops, "groupnorm_silu_bwd", "resident", x0, dy, gamma, beta, in1=x1, add0=a0, add1=a1, groups=groups, eps=1e-6, silu=silu)
    again = ops.groupnorm_silu_bwd(x0, dy, gamma, beta, in1=x1, add0=a0, add1=a1, groups=groups, eps=1e-6, silu=silu)
    for a, b in zip(out[:4], again):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("name,N,H,Wd,C0,C1", [("cpg12_large_map", 2, 16, 16, 384, 0), ("cpg6_unsliceable", 3, 8, 8, 192, 0),
                                               ("cpg12_cat", 2, 16, 16, 256, 128)])
def test_groupnorm_silu_bwd_routes_to_the_generic_kernels(ops, name, N, H, Wd, C0, C1):
    """The two routes away from the resident kernel (12 channels per group on maps of >= 256 pixels; a shape it cannot slice)
    land on the generic path; the result is judged there."""
    C = C0 + C1
    slow = C // 32 == 12 and H * Wd >= 256
    sup = ops.load().dxmi_groupnorm_silu_bwd_supported(C0, C1, H * Wd, 32)
    assert slow == name.startswith("cpg12") and (slow or sup == 0)
    called = []
    orig = ops.groupnorm_generic_bwd
    x0, x1, dy, gamma, beta, a0, a1, _ = gn_operands(name, N, H, Wd, C0, C1, True, bool(C1), False)
    ops.groupnorm_generic_bwd = lambda *a, **k: (called.append(1), orig(*a, **k))[1]
    try:
        gn_bwd_checked(ops, "groupnorm_silu_bwd", "routed-generic", x0, dy, gamma, beta, in1=x1, add0=a0, add1=a1, eps=1e-6)
    finally:
        ops.groupnorm_generic_bwd = orig
    assert called == [1]


def gn_fused_plan(HW, C):
    """gn_fused_plan of csrc/groupnorm.hip restated -> (KMAX, work chunks per image) or (0, 0)."""
    rows_par = 256 // (C // 8)
    if rows_par < 1:
        return 0, 0
    for kmax, cap in ((8, 64), (16, 128)):
        wc = -(-HW // (kmax * rows_par))
        if wc <= cap:
            return kmax, wc
    return 0, 0


def gn_chunks(HW):
    if HW >= 16384:
        return min(64, HW // 256)
    return max(1, min(16, HW // 64))


GENERIC = [
    # (name, N, H, W, C0, C1, groups, silu, scale_shift, add0, statistics: None | "saved" | "blockstats", chunks, rows of the last chunk)
    ("hw200", 3, 10, 20, 192, 0, 32, True, True, True, "saved", 3, 66),
    ("hw200_cat", 2, 10, 20, 64, 128, 32, True, False, False, None, 3, 66),
    ("hw200_blockstats", 2, 10, 20, 192, 0, 32, True, False, False, "blockstats", 3, 66),
    ("hw100", 3, 10, 10, 96, 0, 32, True, False, True, None, 1, 100),
    ("hw63", 2, 7, 9, 192, 0, 32, False, True, False, "saved", 1, 63),
    ("hw35", 5, 5, 7, 64, 64, 32, True, False, False, "blockstats", 1, 35),
    ("hw1", 4, 1, 1, 192, 0, 32, True, True, False, None, 1, 1),
    ("rows256", 1, 128, 128, 64, 0, 32, True, False, False, "saved", 64, 256),
    ("c8", 3, 12, 12, 8, 0, 2, True, False, True, None, 2, 72),
    ("c136_g17", 2, 9, 9, 136, 0, 17, True, True, False, "saved", 1, 81),
    ("c2048", 1, 8, 8, 2048, 0, 32, True, False, False, None, 1, 64),
    ("c2048_cat", 2, 4, 4, 1024, 1024, 32, False, False, True, "blockstats", 1, 16),
    ("one_group", 2, 9, 16, 64, 0, 1, True, False, False, None, 2, 72),
    ("cpg1", 3, 10, 20, 32, 0, 32, True, True, True, "saved", 3, 66),
    ("cpg1_cat", 2, 16, 16, 8, 24, 32, True, False, False, None, 4, 64),
]


@pytest.mark.parametrize("c", GENERIC, ids=[c[0] for c in GENERIC])
def test_groupnorm_generic_bwd_edges(ops, c):
    """The generic backward on both launch forms (knob gn_bwd_fused 0: reduce + apply launches; 2: one launch where its plan
    fits, only at shapes with N * work chunks <= 512: the one-round residency the product's own knob 1 requires)."""
    name, N, H, Wd, C0, C1, groups, silu, ss, add0, stats, chunks, last = c
    HW, C = H * Wd, C0 + C1
    assert gn_chunks(HW) == chunks and HW - (chunks - 1) * -(-HW // chunks) == last
    assert int(ops.load().dxmi_groupnorm_generic_workspace_bytes(N, HW, C)) == N * chunks * 32 * 2 * 4      # the library's chunk count
    if name == "rows256":
        assert HW >= 16384 and -(-HW // chunks) == 256
    if name.startswith("cpg1"):
        assert C // groups == 1 and C % 8 == 0
    x0, x1, dy, gamma, beta, a0, a1, sst = gn_operands(c[:7], N, H, Wd, C0, C1, add0, add0 and bool(C1), ss)
    st = None
    if stats == "saved":
        saved = []
        ops.groupnorm_generic(x0, gamma, beta, in1=x1, groups=groups, eps=1e-5, silu=silu, scale_shift=sst, saved=saved)
        st = saved[0]
    elif stats == "blockstats":
        assert (C // groups) % 2 == 0
        st = ops.gn_blockstats_to_generic(ops.block_stats(x0), ops.block_stats(x1) if C1 else None, N, HW, C0, C1, groups)
    kmax, wchunks = gn_fused_plan(HW, C)
    old = ops.get_tuning("gn_bwd_fused")
    try:
        ops.set_tuning("gn_bwd_fused", 0)
        assert ops.groupnorm_generic_bwd_plan(N, HW, C) == 0
        kw = dict(in1=x1, add0=a0, add1=a1, groups=groups, eps=1e-5, silu=silu, scale_shift=sst, fwd_stats=st)
        two = gn_bwd_checked(ops, "groupnorm_generic_bwd", "two-launch", x0, dy, gamma, beta, **kw)
        if kmax and N * wchunks <= 512:
            ops.set_tuning("gn_bwd_fused", 2)
            form = ops.groupnorm_generic_bwd_plan(N, HW, C)
            assert form in (0, kmax)
            if form:
                one = gn_bwd_checked(ops, "groupnorm_generic_bwd", "one-launch", x0, dy, gamma, beta, **kw)
                again = ops.groupnorm_generic_bwd(x0, dy, gamma, beta, **kw)
                for a, b in zip(one, again):
                    assert (a is None and b is None) or torch.equal(a, b)
    finally:
        ops.set_tuning("gn_bwd_fused", old)
    assert all(t is None or bool(torch.isfinite(t.float()).all()) for t in two)


@pytest.mark.parametrize("N,C,pad", [(1, 8, 0), (7, 136, 8), (19, 200, 24), (3, 2048, 0)])
def test_gn_ss_grads_edges(ops, N, C, pad):
    """dxmi_gn_ss_grads on a row-strided scale_shift: d_scale_shift = (G1 gamma + G0 beta | G0) exactly two products and a sum,
    dgamma / dbeta sums over the N images of G (1 + scale)."""
    g = gen(("ss", N, C))
    G = rnd(g, 2, N, C)
    emb = rnd(g, N, 2 * C + pad)
    ss = emb[:, pad // 2: pad // 2 + 2 * C]
    ga, be = rnd(g, C), rnd(g, C)
    d_ss = torch.empty(N, 2 * C, device=DEV)
    dgb = torch.empty(2, C, device=DEV)
    ops.check(ops.load().dxmi_gn_ss_grads(G.data_ptr(), ss.data_ptr(), ss.stride(0), ga.data_ptr(), be.data_ptr(), d_ss.data_ptr(),
                                          dgb[0].data_ptr(), dgb[1].data_ptr(), N, C, None), "dxmi_gn_ss_grads")
    Gd, gad, bed, one_s = G.double(), ga.double(), be.double(), 1 + ss[:, :C].double()
    EDGE.fp32("gn_ss_grads_dss", d_ss, torch.cat([Gd[1] * gad + Gd[0] * bed, Gd[0]], 1),
              torch.cat([(Gd[1] * gad).abs() + (Gd[0] * bed).abs(), Gd[0].abs()], 1), 4)
    EDGE.fp32("gn_ss_grads_dgamma", dgb[0], (Gd[1] * one_s).sum(0), (Gd[1] * one_s).abs().sum(0), N + 4)
    EDGE.fp32("gn_ss_grads_dbeta", dgb[1], (Gd[0] * one_s).sum(0), (Gd[0] * one_s).abs().sum(0), N + 4)


@pytest.mark.parametrize("P,C", [(1, 64), (5, 8), (513, 128), (1000, 2304), (131073, 64)])
def test_colsum_ragged_rows_and_accumulate(ops, P, C):
    """Column sums of bf16 rows at row counts that are no multiples of the 512-row block (131 073: the block doubles to 1 024
    rows to stay within 256 partials), written and accumulated into a random vector."""
    g = gen(("colsum", P, C))
    x = bf(rnd(g, P, C))
    xd = x.double()
    got = ops.colsum(x)
    EDGE.fp32("colsum", got, xd.sum(0), xd.abs().sum(0), P + 2)
    old = rnd(g, C, scale=math.sqrt(P))
    acc = old.clone()
    ops.colsum(x, out=acc, accumulate=True)
    EDGE.fp32("colsum+old", acc, old.double() + xd.sum(0), old.double().abs() + xd.abs().sum(0), P + 2)


@pytest.mark.parametrize("N,HW,C", [(3, 1, 64), (2, 35, 8), (5, 200, 192), (1, 1025, 2048)])
def test_colsum_per_image_ragged_rows(ops, N, HW, C):
    g = gen(("colsum_pi", N, HW, C))
    x = bf(rnd(g, N, HW, 1, C))
    got = ops.colsum_per_image(x)
    EDGE.fp32("colsum_per_image", got, x.double().sum((1, 2)), x.double().abs().sum((1, 2)), HW + 2)


@pytest.mark.parametrize("B,N,C", [(1, 1, 8), (2, 7, 40), (3, 100, 2304), (1, 513, 17)])
def test_colsum_f32_edges(ops, B, N, C):
    g = gen(("colsum_f32", B, N, C))
    x = rnd(g, B, N, C)
    got = ops.colsum_f32(x)
    EDGE.fp32("colsum_f32", got, x.double().sum(1), x.double().abs().sum(1), N + 2)
    assert torch.equal(got, ops.colsum_f32(x))


# ------------------------------------------------------------------------------------------ attention backward
FUSED = [
    # (N, T, heads): N * heads * ceil(T / 128) = 1, 3, 9, 18 workgroups: the remainders of the XCD block remap
    (1, 40, 1, 1), (3, 65, 1, 3), (3, 129, 3, 18), (1, 200, 3, 6), (3, 200, 3, 18), (1, 264, 3, 9), (3, 40, 3, 9), (1, 65, 2, 2),
]


@pytest.mark.parametrize("N,T,heads,grid", FUSED, ids=[f"N{c[0]}-T{c[1]}-h{c[2]}" for c in FUSED])
def test_attention_bwd_fused_ragged_T(ops, N, T, heads, grid):
    """The fused kernels (64-wide heads) at ragged T, with the output of the kernel's own forward, with and without its
    log-sum-exp: every (image, q|k|v, head, 128-row block) on its own, the last block ragged; bitwise equal on a second run;
    an image's gradient does not depend on the batch; against the five-GEMM path where it accepts T (T % 8 == 0)."""
    D, C = 64, 64 * heads
    assert ops.load().dxmi_attention_bwd_supported(T, C, heads) == 1 and ops.FUSED_ATTENTION_BWD
    assert N * heads * -(-T // 128) == grid and T >= 24
    scale = D ** -0.5
    g = gen(("fused", N, T, heads))
    qkv, do = bf(rnd(g, N, T, 3 * C)), bf(rnd(g, N, T, C))
    o, lse = ops.attention(qkv, heads, scale, want_lse=True)
    assert lse is not None and torch.equal(o, ops.attention(qkv, heads, scale))
    got, ref = attention_bwd_checked(ops, qkv, do, heads, scale, o=o, tag=f"attention_bwd[fused,T{T}]")
    got_l, _ = attention_bwd_checked(ops, qkv, do, heads, scale, o=o, lse=lse, ref=ref, tag=f"attention_bwd[fused,lse,T{T}]")
    assert torch.equal(got, ops.attention_bwd(qkv, do, heads, scale, o=o))
    assert torch.equal(got_l, ops.attention_bwd(qkv, do, heads, scale, o=o, lse=lse))
    if N > 1:
        one = ops.attention_bwd(qkv[1:2].contiguous(), do[1:2].contiguous(), heads, scale, o=o[1:2].contiguous())
        assert torch.equal(one[0], got[1])
    if T % 8 == 0:
        attention_bwd_checked(ops, qkv, do, heads, scale, ref=ref, tag=f"attention_bwd[five-gemm,D64,T{T}]")


GEMM5 = [(2, 24, 1, 256), (2, 40, 2, 128), (1, 200, 3, 32), (3, 24, 2, 32), (2, 40, 1, 256), (2, 200, 1, 128), (1, 200, 1, 256),
         (1, 1032, 1, 256)]


@pytest.mark.parametrize("N,T,heads,D", GEMM5, ids=[f"N{c[0]}-T{c[1]}-h{c[2]}-D{c[3]}" for c in GEMM5])
def test_attention_bwd_five_gemm_tails(ops, N, T, heads, D):
    """bgemm_kernel in its four operand layouts plus dxmi_softmax_bwd: tails of the 32-wide K chunk and of the 64-wide M / N
    tiles; T = 1032 (> 1024) takes the looped softmax kernel, every other T here the register form."""
    C = heads * D
    assert T % 8 == 0 and T >= 24
    assert (T % 4 != 0 or T > 1024) == (T == 1032)
    scale = D ** -0.5
    g = gen(("gemm5", N, T, heads, D))
    qkv, do = bf(rnd(g, N, T, 3 * C)), bf(rnd(g, N, T, C))
    got, _ = attention_bwd_checked(ops, qkv, do, heads, scale, tag=f"attention_bwd[five-gemm,D{D}{',looped-softmax' if T > 1024 else ''}]")
    assert torch.equal(got, ops.attention_bwd(qkv, do, heads, scale))


@pytest.mark.parametrize("rows,T,looped", [(7, 4, False), (5, 36, False), (6, 1024, False), (7, 30, True), (5, 1028, True), (3, 1032, True)])
def test_softmax_bwd_alone(ops, rows, T, looped):
    """dxmi_softmax_bwd called the way ops.attention_bwd calls it (fp32 S and dP in, bf16 P and dS out), a row count that is no
    multiple of the four rows of a workgroup: the register form (T % 4 == 0 and T <= 1024) and the looped form.  P and dS lie
    within one bf16 rounding of the fp64 values plus 16 u32 of the row's largest term (softmax_bwd_ref: the fp32 evaluation's
    error scales with the largest probability of the row, for dS with the largest P (|dP| + sum |dP| P))."""
    assert (T % 4 != 0 or T > 1024) == looped and rows % 4 != 0
    g = gen(("softmax", rows, T))
    S, dP = rnd(g, rows, T, scale=2.0), rnd(g, rows, T)
    P = torch.empty(rows, T, dtype=torch.bfloat16, device=DEV)
    dS = torch.empty_like(P)
    ops.check(ops.load().dxmi_softmax_bwd(S.data_ptr(), dP.data_ptr(), P.data_ptr(), dS.data_ptr(), rows, T, None), "dxmi_softmax_bwd")
    rP, rdS, mP, mS = softmax_bwd_ref(S, dP)
    form = "looped" if looped else "reg"
    for name, got, ref, m in (("P", P, rP, mP), ("dS", dS, rdS, mS)):
        assert bool(torch.isfinite(got.float()).all())
        ratio = float(((got.double() - ref).abs() / (U16 * ref.abs() + 16 * U32 * m)).max())
        EDGE._note(f"softmax_bwd[{form}]_{name}", ratio)
        assert ratio <= 1.0, (name, ratio)


def test_report():
    """Largest |err| / bound per op and family over the cases above (printed; run with -s)."""
    for k, v in EDGE.report().items():
        print(f"  {k:56s} {v:.4f}")
