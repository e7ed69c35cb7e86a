"""The forward attention and GroupNorm kernels off the program shapes, every launch judged element by element against stock
torch in float64 on the same operands, through the helpers of tests/forward_bounds.py that test_hip_forward_shapes.py uses for the
program shapes (attention_checked / attention_case: attn_elem_bound; gn_fwd_checked: gn_bound; stats_depth).  The cases are the
tails and routes no program reaches: ragged T on every head width of attention_kernel<D> (half waves, a second query block of
one row, a last key block of one key, the prefetching form's single and ragged blocks), grids below, at and off a multiple of
the eight XCDs, the scale <= 0 gate, attention64_kernel's and attention256_kernel's smallest grids, the switchable variants in
interpreters of their own; the resident GroupNorm forward's masked-wave-sum reduce, ragged last pieces, maps smaller than a
workgroup and the 32-piece plan; the generic forward's chunk tails; the streaming apply's partial counts and ragged chunks; block
statistics and their fold.  Ragged attention cases take inputs whose true scores all lie far below zero (attn_inputs), where a
zero-filled key left unmasked is hundreds of bounds away.  Every case asserts the plan or route it is meant to reach before it
launches, runs its launch twice (bitwise equal) and image N - 1 alone (bitwise its rows of the batch).  Refusals are asserted
through the library's queries (no launch).  test_forward_bounds.py checks the judge and the restated plans on the host.
"""
import json
import math
import os
import subprocess
import sys
import zlib

import pytest
import torch

from forward_bounds import (EDGE, MIN_COND, attention_case, attn_xcd_logical, block_stats_tensor, fold_passes, gn_apply_chunks, gn_fwd_checked,
                            gn_fwd_plan, gn_input, stats_depth, stats_ref)
from forward_census import attention_kernel
from test_hip_backward_edges import GENERIC, gn_chunks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def gen(key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


# ------------------------------------------------------------------------------------------ attention
def attn_route(T, heads, D, scale):
    """attention_fwd_impl's dispatch (csrc/attention.hip) under the default switches, the scale gate included."""
    if D == 256 and T == 256 and heads == 1:
        return "attention256<false>"
    if D == 64 and T % 256 == 0 and scale > 0:
        return "attention64"
    return f"attention_kernel<{D}>"


BOTH = ("below_zero", "peaked")
ATTN = [
    # (N, T, heads, D, input kinds, workgroups, what the row reaches); grid = N * heads * ceil(T / 128)
    (1, 1, 1, 64, ("below_zero",), 1, "one valid query, three idle waves; a grid below the eight XCDs"),
    (3, 31, 1, 64, ("below_zero",), 3, "half a wave"),
    (7, 33, 1, 64, ("below_zero",), 7, "half a wave and one lane over"),
    (2, 63, 4, 64, ("below_zero",), 8, "the ragged-block branch of the key mask, one key short; a grid of exactly eight"),
    (3, 64, 3, 64, ("below_zero",), 9, "the full-block branch alone; a grid of 8 + 1"),
    (7, 65, 3, 64, BOTH, 21, "a second key block of one key; a grid with G % 8 = 5"),
    (1, 127, 2, 64, BOTH, 2, "the last query of the block idle"),
    (2, 129, 1, 64, BOTH, 4, "a second query block that holds one row"),
    (2, 200, 2, 64, BOTH, 8, "the ragged case of test_attention"),
    (1, 321, 1, 64, BOTH, 3, "six key blocks, the last of one key"),
    (1, 64, 2, 128, ("below_zero",), 2, "PF = true with one block: the prefetch must not run; head stride != C"),
    (2, 65, 2, 128, BOTH, 4, "PF = true, the fetched second block is the ragged one"),
    (1, 130, 2, 128, BOTH, 4, "PF = true, three key blocks, a second query block of two rows"),
    (3, 200, 2, 128, BOTH, 12, "PF = true, four key blocks, last of eight keys"),
    (3, 16, 1, 256, ("below_zero",), 3, "a quarter block of the widest head"),
    (2, 40, 1, 256, ("below_zero",), 2, "one ragged block"),
    (1, 65, 1, 256, BOTH, 1, "PF = true at D = 256, second block of one key"),
    (1, 256, 2, 256, BOTH, 4, "T = 256 of 256-wide heads with two heads: NOT attention256_kernel"),
]


@pytest.mark.parametrize("c", ATTN, ids=[f"N{c[0]}-T{c[1]}-h{c[2]}-D{c[3]}" for c in ATTN])
def test_attention_generic_kernel_edges(ops, c):
    N, T, heads, D, kinds, grid, _ = c
    kern = f"attention_kernel<{D}>"
    assert attn_route(T, heads, D, D ** -0.5) == kern == attention_kernel(T, heads * D, heads)
    assert N * heads * -(-T // 128) == grid and N <= 7
    assert (len(kinds) == 2) == (T > 64)                       # several key blocks: both input kinds
    assert ops.load().dxmi_attention_fwd_lse_supported(T, heads * D, heads) == 1
    for i, kind in enumerate(kinds):
        want_lse = i == 0
        _, res = attention_case(ops, N, T, heads, D, kind, kern, want_lse=want_lse)
        assert not want_lse or res[1] is not None


def test_attention_negative_scale_leaves_attention64(ops):
    """scale <= 0 at D = 64, T = 256: attention64_kernel keeps the running maximum on the RAW logits and folds scale * log2(e)
    into the exponential, which is only a maximum of the scaled logits for scale > 0, so attention_fwd_impl sends the shape to
    attention_kernel<64>.  The route itself is unobserved: the library exports no query for the choice and the census wrapper
    (forward_census.attention_kernel) mirrors the dispatch by shape alone.  What is observed is the result, against fp64: on
    the peaked inputs a maximum taken on the wrong end of the logits overflows the exponentials of attention64_kernel."""
    N, T, heads, D = 2, 256, 1, 64
    assert attn_route(T, heads, D, -(D ** -0.5)) == "attention_kernel<64>" and attn_route(T, heads, D, D ** -0.5) == "attention64"
    for kind in ("gauss", "peaked"):
        attention_case(ops, N, T, heads, D, kind, "attention_kernel<64>, scale < 0", scale=-(D ** -0.5), want_lse=kind == "peaked")


ATTN64 = [(1, 256, 1, BOTH, 1), (1, 256, 3, BOTH, 3), (3, 256, 1, BOTH, 3), (3, 256, 3, BOTH, 9), (1, 512, 2, ("peaked",), 4)]


@pytest.mark.parametrize("N,T,heads,kinds,grid", ATTN64, ids=[f"N{c[0]}-T{c[1]}-h{c[2]}" for c in ATTN64])
def test_attention64_edges(ops, N, T, heads, kinds, grid):
    """attention64_kernel (a workgroup = 256 queries) on its smallest grids; the output with the lse is bitwise the one without."""
    assert attn_route(T, heads, 64, 0.125) == "attention64" == attention_kernel(T, heads * 64, heads) and N * heads * (T // 256) == grid
    for kind in kinds:
        qkv, (out, lse) = attention_case(ops, N, T, heads, 64, kind, "attention64", want_lse=True)
        assert lse is not None
        _, plain = attention_case(ops, N, T, heads, 64, kind, "attention64", want_lse=False)
        assert torch.equal(out, plain)


@pytest.mark.parametrize("N,kinds", [(1, BOTH), (3, ("peaked",)), (7, ("below_zero",))], ids=["N1", "N3", "N7"])
def test_attention256_edges(ops, N, kinds):
    """attention256_kernel<false> (one head, T = C = 256) on one-image and odd batches; it keeps no row log-sum-exp."""
    assert attn_route(256, 1, 256, 1 / 16) == "attention256<false>" == attention_kernel(256, 256, 1)
    assert ops.load().dxmi_attention_fwd_lse_supported(256, 256, 1) == 0
    for kind in kinds:
        _, (out, lse) = attention_case(ops, N, 256, 1, 256, kind, "attention256<false>", want_lse=True)
        assert lse is None


KNOBS = ["pf1_d64", "pf0_d128", "generic", "xcd0"]


def test_attention_switchable_variants():
    """DXMI_ATTN_PF / DXMI_ATTN_GENERIC / DXMI_ATTN64 / DXMI_ATTN_XCD are read once per process: four fresh
    interpreters, one after another, each under its own time limit, each running a reduced table (tests/_attn_knob_worker.py) under
    the same bound.  The first child that does not return 0 fails the test and no further child is started."""
    from _attn_knob_worker import TABLES
    for table in KNOBS:
        set_env, tag, _ = TABLES[table]
        env = {k: v for k, v in os.environ.items() if not k.startswith("DXMI_ATTN")}
        env.update(set_env)
        p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "_attn_knob_worker.py"), table], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, f"{table} ({set_env}): return code {p.returncode}\n{p.stderr[-3000:]}"
        worst = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        assert worst and all(v <= 1.0 for v in worst.values()), worst
        for k, v in worst.items():
            EDGE._note(k, v)


# ------------------------------------------------------------------------------------------ resident GroupNorm forward
RESIDENT = [
    # (name, N, H, W, C0, C1, groups, silu, what the shape must be in gn_silu_kernel's plan)
    ("vec4_cpg4", 7, 8, 8, 128, 0, 32, True, lambda p: p["VEC"] == 4 and p["fast"]),
    ("vec4_c0_132", 2, 8, 8, 132, 124, 32, True, lambda p: p["VEC"] == 4 and p["fast"]),        # VEC 4 because C0 % 8 != 0
    ("cpg12_notfast", 3, 8, 8, 384, 0, 32, True, lambda p: p["VEC"] == 4 and p["ppt"] == 3 and not p["fast"] and p["threads"] == 384 and p["pieces"] == 16),
    ("cpg12_cat_ragged", 2, 7, 7, 256, 128, 32, True, lambda p: not p["fast"] and p["ragged"]),
    ("cpg24_notfast", 5, 4, 4, 768, 0, 32, True, lambda p: p["VEC"] == 8 and p["ppt"] == 3 and not p["fast"]),
    ("wide_ppp128_4x4", 3, 4, 4, 1024, 0, 32, True, lambda p: p["ppp"] == 128 and not p["fast"]),
    ("wide_ppp128_8x8", 2, 8, 8, 1024, 0, 32, True, lambda p: p["ppp"] == 128 and not p["fast"] and p["pieces"] == 16),
    ("c2048", 3, 2, 2, 2048, 0, 32, True, lambda p: p["ppp"] == 256 and p["pieces"] == 2),
    ("map_1x1", 3, 1, 1, 256, 0, 32, True, lambda p: p["threads"] == 64 and p["pieces"] == 1 and 1 * p["ppp"] < p["threads"]),
    ("map_2x2_cat", 2, 2, 2, 128, 128, 32, True, lambda p: p["threads"] == 128),
    ("map_3x3", 7, 3, 3, 128, 0, 32, True, lambda p: p["threads"] == 320 and p["ragged"]),
    ("ragged_piece", 3, 5, 7, 256, 0, 32, True, lambda p: p["pieces"] == 3 and p["ragged"]),
    ("one_group", 3, 3, 4, 64, 0, 1, True, lambda p: p["ppt"] == 8),
    ("sliced_vec4_32", 2, 32, 32, 128, 0, 32, True, lambda p: p["VEC"] == 4 and p["slices"] == 2 and p["pieces"] == 32),
    ("sliced_ragged", 2, 50, 100, 128, 0, 32, True, lambda p: p["slices"] == 16 and p["ragged"]),
    ("no_silu_cpg12_cat_ragged", 3, 7, 7, 256, 128, 32, False, lambda p: not p["fast"] and p["ragged"]),
    ("no_silu_ragged_piece", 2, 5, 7, 256, 0, 32, False, lambda p: p["fast"] and p["ragged"]),
]


def _gn_operands(key, N, H, W, C0, C1, groups, ss=False):
    g = gen(key)
    C = C0 + C1
    xc = gn_input(g, N, H, W, C, MIN_COND, groups)
    x0 = xc[..., :C0].contiguous()
    x1 = xc[..., C0:].contiguous() if C1 else None
    gamma, beta = 1 + 0.3 * rnd(g, C), 0.3 * rnd(g, C)
    sst = (0.3 * rnd(g, N, 3 * C))[:, C // 2: C // 2 + 2 * C] if ss else None           # a row-strided slice, as emb_all's
    return x0, x1, gamma, beta, sst


def _last(t, N):
    return None if t is None else t[N - 1:].contiguous()


@pytest.mark.parametrize("c", RESIDENT, ids=[c[0] for c in RESIDENT])
def test_groupnorm_resident_fwd_edges(ops, c):
    name, N, H, W, C0, C1, groups, silu, pred = c
    assert ops.load().dxmi_groupnorm_silu_supported(C0, C1, H * W, groups) == 1 and N <= 7
    plan = gn_fwd_plan(C0, C1, H * W, groups)
    assert plan is not None and plan["pieces"] <= (16 if plan["VEC"] == 8 else 32) and pred(plan), plan
    if name in ("vec4_c0_132", "cpg12_cat_ragged", "no_silu_cpg12_cat_ragged"):
        assert C1 and C0 % ((C0 + C1) // groups) != 0, "a group straddles the concat"
    if name == "vec4_c0_132":
        assert ((C0 + C1) // groups) % 8 == 0 and C0 % 8 != 0
    x0, x1, gamma, beta, _ = _gn_operands(c[:7], N, H, W, C0, C1, groups)
    y = gn_fwd_checked(ops, "resident", x0, gamma, beta, in1=x1, groups=groups, eps=1e-6, silu=silu)
    assert torch.equal(y, ops.groupnorm_silu(x0, gamma, beta, in1=x1, groups=groups, eps=1e-6, silu=silu))
    one = ops.groupnorm_silu(_last(x0, N), gamma, beta, in1=_last(x1, N), groups=groups, eps=1e-6, silu=silu)
    assert torch.equal(one[0], y[N - 1])


@pytest.mark.parametrize("why,shape", [("cpg3", (96, 0, 100, 32)), ("cpg6", (192, 0, 64, 32)), ("unit576", (288, 0, 16, 8)),
                                       ("33_pieces", (128, 0, 16385, 32)), ("33_pieces_one_group", (4, 0, 16385, 1))])
def test_groupnorm_resident_fwd_refusals_through_the_query(ops, why, shape):
    """Channels per group no multiple of 4; a slice whose thread unit lcm(ppp, 64) is 576 > 512; a map one pixel larger than the
    32 slices x 32 pieces x 512 threads the last slicing holds (16384 pixels is served).  No launch: ops.groupnorm_silu sends
    these to the generic kernels."""
    assert gn_fwd_plan(*shape) is None and ops.load().dxmi_groupnorm_silu_supported(*shape) == 0
    if why.startswith("33_pieces"):
        C0, _, HW, groups = shape
        assert gn_fwd_plan(C0, 0, HW - 1, groups)["pieces"] == 32 and ops.load().dxmi_groupnorm_silu_supported(C0, 0, HW - 1, groups) == 1


# ------------------------------------------------------------------------------------------ generic GroupNorm forward
GENERIC_FWD = [c for c in GENERIC if c[0] != "hw200_blockstats"]       # that row differs from hw200 in the backward's statistics only


def test_generic_rows_are_the_issue_list():
    assert [c[0] for c in GENERIC_FWD] == ["hw200", "hw200_cat", "hw100", "hw63", "hw35", "hw1", "rows256", "c8", "c136_g17", "c2048",
                                           "c2048_cat", "one_group", "cpg1", "cpg1_cat"]


@pytest.mark.parametrize("c", GENERIC_FWD, ids=[c[0] for c in GENERIC_FWD])
def test_groupnorm_generic_fwd_edges(ops, c):
    """ops.groupnorm_generic on the chunk tails of the backward's table (its silu and row-strided scale_shift choices), into the
    shared workspace and into a saved statistics tensor of its own."""
    name, N, H, W, C0, C1, groups, silu, ss, _, _, chunks, last = c
    HW, C = H * W, C0 + C1
    assert gn_chunks(HW) == chunks and HW - (chunks - 1) * -(-HW // chunks) == last and N <= 7
    assert int(ops.load().dxmi_groupnorm_generic_workspace_bytes(N, HW, C)) == N * chunks * 32 * 2 * 4      # the library's chunk count
    x0, x1, gamma, beta, sst = _gn_operands(c[:7], N, H, W, C0, C1, groups, ss)
    kw = dict(in1=x1, groups=groups, eps=1e-5, silu=silu, scale_shift=sst)
    y = gn_fwd_checked(ops, "generic", x0, gamma, beta, **kw)
    saved = []
    ys = gn_fwd_checked(ops, "generic", x0, gamma, beta, saved=saved, tag="generic, saved", **kw)
    assert len(saved) == 1 and saved[0].numel() == N * chunks * 32 * 2
    assert torch.equal(y, ys) and torch.equal(y, ops.groupnorm_generic(x0, gamma, beta, **kw))
    one = ops.groupnorm_generic(_last(x0, N), gamma, beta, in1=_last(x1, N), groups=groups, eps=1e-5, silu=silu, scale_shift=_last(sst, N))
    assert torch.equal(one[0], y[N - 1])


# ------------------------------------------------------------------------------------------ streaming apply
APPLY = [
    # (name, N, H, W, C0, C1, groups, P0, P1, silu, scale_shift, (rows per chunk, chunks) of the launcher)
    ("p1_hw35", 3, 5, 7, 512, 0, 32, 1, 0, True, False, (32, 2)),
    ("pmax_hw200_ss", 2, 10, 20, 192, 0, 32, "MAX", 0, True, True, (80, 3)),
    ("p8_p2_cat_cpg6", 3, 10, 20, 64, 128, 32, 8, 2, True, False, (80, 3)),
    ("p3_hw35_cat", 2, 5, 7, 128, 64, 32, 3, 5, False, True, (35, 1)),
    ("c8", 5, 5, 7, 8, 0, 2, 3, 0, True, False, (35, 1)),
    ("c2048_hw35", 2, 5, 7, 2048, 0, 32, 4, 0, False, True, (8, 5)),
    ("c2048_cat", 1, 10, 20, 1024, 1024, 32, 2, 7, True, False, (8, 25)),
]


@pytest.mark.parametrize("c", APPLY, ids=[c[0] for c in APPLY])
def test_groupnorm_apply_edges(ops, c):
    """ops.groupnorm_apply from statistics formed in fp64 (one rounding each): one partial, the most the kernel keeps in flight,
    different counts per concat source, chunks whose last trip is ragged, the narrowest and the widest tensor.  The split form
    (DXMI_GN_APPLY_SPLIT) is a process-wide switch of ops, not a per-call argument: test_groupnorm_apply_split_is_bit_identical
    covers it in a process of its own."""
    name, N, H, W, C0, C1, groups, P0, P1, silu, ss, (rpc, chunks) = c
    P0 = ops.MAX_APPLY_PARTIALS if P0 == "MAX" else P0
    HW, C = H * W, C0 + C1
    assert gn_apply_chunks(HW, C) == (rpc, chunks) and N <= 7 and max(P0, P1) <= ops.MAX_APPLY_PARTIALS
    assert (C // groups) % 2 == 0 and C0 % 8 == 0 and C1 % 8 == 0 and C <= 2048                          # the launcher's argument check
    if name == "p8_p2_cat_cpg6":
        assert C // groups == 6 and C0 % 6 != 0
    x0, x1, gamma, beta, sst = _gn_operands(c[:9], N, H, W, C0, C1, groups, ss)
    st0 = ops.BlockStats(block_stats_tensor(x0, P0), P0)
    st1 = ops.BlockStats(block_stats_tensor(x1, P1), P1) if C1 else None
    kw = dict(groups=groups, eps=1e-6, silu=silu)
    y = gn_fwd_checked(ops, "apply", x0, gamma, beta, in1=x1, st0=st0, st1=st1, scale_shift=sst, **kw)
    assert torch.equal(y, ops.groupnorm_apply(x0, st0, gamma, beta, in1=x1, st1=st1, scale_shift=sst, **kw))
    s0 = ops.BlockStats(_last(st0.buf, N), P0)
    s1 = ops.BlockStats(_last(st1.buf, N), P1) if C1 else None
    one = ops.groupnorm_apply(_last(x0, N), s0, gamma, beta, in1=_last(x1, N), st1=s1, scale_shift=_last(sst, N), **kw)
    assert torch.equal(one[0], y[N - 1])


# ------------------------------------------------------------------------------------------ block statistics and their fold
@pytest.mark.parametrize("N,HW,C", [(3, 1, 64), (2, 35, 8), (5, 200, 192), (1, 1025, 2048), (2, 81, 136)])
def test_block_stats_edges(ops, N, HW, C):
    """gn_block_stats_kernel: one row, a tensor of one 8-channel piece, ragged rows per chunk (1025 rows in four chunks of 257),
    and C = 136: 17 pieces per row, 256 // 17 = 15 row lanes and one idle thread."""
    P = HW // 256 if HW >= 512 else 1
    assert int(ops.load().dxmi_gn_block_stats_partials(HW)) == P <= ops.MAX_APPLY_PARTIALS
    if C == 136:
        assert (C // 8) == 17 and 256 % 17 != 0
    x = gn_input(gen(("bs", N, HW, C)), N, HW, 1, C, MIN_COND, math.gcd(C, 32))
    st = ops.block_stats(x)
    assert st.P == P and tuple(st.buf.shape) == (N, P, C // 2, 2)
    S, Sa = stats_ref(x)
    EDGE.fp32("block_stats", st.buf.double().sum(1), S, Sa, stats_depth(HW, P, fold_passes(P)))
    assert torch.equal(st.buf, ops.block_stats(x).buf)
    assert torch.equal(ops.block_stats(x[N - 1:].contiguous()).buf[0], st.buf[N - 1])


def _fold_ref(ops, b, group):
    """ops.fold_stats in fp64: `group` consecutive partials added, again while more than MAX_APPLY_PARTIALS are left -> (sums,
    sums of absolute values, passes)."""
    ref, A, passes = b, b.abs(), 0
    while ref.shape[1] > ops.MAX_APPLY_PARTIALS:
        N, P, C2, _ = ref.shape
        PG = -(-P // group)
        pad = ref.new_zeros(N, PG * group - P, C2, 2)
        ref = torch.cat([ref, pad], 1).reshape(N, PG, group, C2, 2).sum(2)
        A = torch.cat([A, pad], 1).reshape(N, PG, group, C2, 2).sum(2)
        passes += 1
    return ref, A, passes


@pytest.mark.parametrize("N,P,C,group,passes", [(2, 1, 64, 32, 0), (1, 31, 2, 32, 1), (3, 33, 2304, 32, 1), (1, 1025, 64, 32, 2), (2, 9, 192, 4, 1)])
def test_fold_stats_edges(ops, N, P, C, group, passes):
    """gn_stats_fold_kernel: a last group of one partial (P = 33), P below the group (31), two passes (1025 -> 33 -> 2), the
    narrowest row (C = 2) and one of nine 256-thread blocks (C = 2304); P = 1 is returned as it is.  Each folded partial is an
    fp32 sum of `group` partials per pass, in order: depth (group + 1) per pass."""
    g = gen(("fold", N, P, C, group))
    buf = (rnd(g, N, P, C // 2, 2) + 3.0).contiguous()
    st = ops.fold_stats(ops.BlockStats(buf, P), group)
    ref, A, n = _fold_ref(ops, buf.double(), group)
    assert n == passes and st.P == ref.shape[1] <= ops.MAX_APPLY_PARTIALS
    if passes == 0:
        assert st.buf is buf
    EDGE.fp32("fold_stats", st.buf, ref, A, max(1, passes) * (group + 1))
    assert torch.equal(st.buf, ops.fold_stats(ops.BlockStats(buf, P), group).buf)
    assert torch.equal(ops.fold_stats(ops.BlockStats(buf[N - 1:].contiguous(), P), group).buf[0], st.buf[N - 1])


def test_xcd_permutation_covers_the_launched_grids():
    """The grids the attention rows launch (below eight, eight, and off a multiple of eight) are permuted onto themselves."""
    grids = sorted({c[5] for c in ATTN} | {c[4] for c in ATTN64})
    assert {1, 3, 7, 8, 9, 21} <= set(grids)
    for G in grids:
        assert sorted(attn_xcd_logical(b, G) for b in range(G)) == list(range(G))


def test_report():
    print("\nworst |err| / bound per kernel family (forward edges):", EDGE.report())
