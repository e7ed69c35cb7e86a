"""Every launch of the FID / evaluator InceptionV3 program (pytorch_fid/inception.py on csrc/inception_ops.hip) against fp64, element
by element, on the net's own activations and at the batch sizes and input formats the programs use.

test_walk runs the HIP program once under inception_walk.Recorder (every public `ops` function is wrapped: a call that is not one
of the extractor's six launch ops or an allowed helper fails the test) and then walks the architecture as oracle/inception.py
states it over the device tensors of that run (inception_walk.DeviceGraph):
    dataflow      the input the oracle's wiring assembles for a layer (torch.cat order, pool kind, stride) from the stored bf16
                  outputs of earlier launches is torch.equal to what the HIP launch of that layer received;
    arithmetic    the launch's output is within the derived bound (tests/forward_bounds.py) of the fp64 result of the layer on
                  that input: 94 convs (weight operand: the unpacked packed buffer), 9 average and 4 max pools (11 in the Mixed
                  blocks, 2 after the stem), the global average pool, the resize, the NCHW conversions (bitwise), and the 94
                  weight packs against the fp64 BatchNorm fold of the checkpoint's tensors;
    completeness  launches judged == launches recorded per op, every name of model._convs() visited exactly once.
WALKS: N = 3 with all four taps; N = 50 (fid_score.get_activations_from_tensor's batch); N = 64 and 16 uint8 NHWC 64x64 through
EvalInceptionV3 (the evaluator's batch and the remainder batch of 50 000 / 10 000 images), which also pins `spatial` bitwise to
Mixed_6d.branch1x1[..., :7] and `pool` to the judged global average; N = 1 at 256x256; N = 2 without resize or normalisation on a
139 x 203 input (non-square maps all the way down).

The row tests reach what the program never does but the C ABI accepts (relu off, channel windows next to sentinels, SH != SW,
PH != PW, a kernel as large as the padded map, Cout < 32 and 33, pool stride 2 with padding, 1-output pools, cnt = 6 / 4
averages, down-scaling and non-square resizes, HW = 1 global pools), on seeded inputs with the same bounds.

All references are stock torch in float64 on the device; no project kernel takes part in one.  No element is left out of any
comparison.  PARITY with the reference's weights stays unpinned (torchvision and the FID weight file are absent): the weights are
the formula weights of inception_walk.tv_state_dict.

Measured on an MI355X (test_report prints them): worst |err| / bound 0.91 - 0.99 for the convs, the average pool, the weight
pack and the resize (the bf16 store's u16 |ref| term, reached at a rounding midpoint), 0.31 for the packed bias, 0.05 for the
global average pool; the module runs in about 5 s.  Why it exists: with the Mixed_5c average pool made to count its padding, the
per-block norm test of test_inception.py still passes (block 2 at 2.3e-2 of its 3e-2) while the walk fails at 143 times the
average pool's bound; swapped channel windows in an InceptionA block fail the bitwise dataflow check, a truncating bf16 store in
the conv epilogue fails at 1.97 times the conv bound.
"""
import pytest
import torch

import forward_bounds as fb
import inception_walk as iw
from backward_bounds import BoundError
from forward_bounds import FwdChecker

DEV = "cuda:0"
CHECK = FwdChecker()

# id -> (N, input, output_blocks, resize_input, normalize_input); input: ("float", H, W) NCHW in (0, 1) or ("uint8", H, W) NHWC
WALKS = {
    "n3_all_taps": (3, ("float", 32, 32), [0, 1, 2, 3], True, True),
    "n50_fid_batch": (50, ("float", 32, 32), [3], True, True),
    "n64_eval_uint8": (64, ("uint8", 64, 64), None, True, True),
    "n16_eval_uint8_remainder": (16, ("uint8", 64, 64), None, True, True),
    "n1_lsun256": (1, ("float", 256, 256), [3], True, True),
    "n2_noresize_139x203": (2, ("float", 139, 203), [3], False, False),
}


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    """(state dict on the CPU, path of the torch.save'd file): formula weights, non-zero fc.weight."""
    from pytorch_fid.inception import InceptionV3
    sd = iw.tv_state_dict(InceptionV3(), fc=True)
    path = tmp_path_factory.mktemp("fid_weights") / "pt_inception.pth"
    torch.save(sd, path)
    return sd, str(path)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def walk(ops, model, sd, inp, run, resize_input, normalize_input, output_blocks):
    """Run `run()` (the HIP program on `inp`-derived input) under the recorder, walk the oracle's graph over the records.
    -> (recorder, graph, what run() returned)."""
    from oracle import inception as oinc
    with iw.Recorder(ops, model) as rec:
        ret = run()
    torch.cuda.synchronize()
    assert not rec.unknown, f"ops functions called by the extractor that are neither judged launches nor allowed helpers: {sorted(rec.unknown)}"
    g = iw.DeviceGraph(rec, model, sd, CHECK)
    g.judge_packs()
    outs = oinc.forward(sd, inp, resize_input=resize_input, normalize_input=normalize_input, last_block=3, g=g)
    return rec, g, ret, outs


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(WALKS))
def test_walk(ops, weights, monkeypatch, case):
    from pytorch_fid.inception import EvalInceptionV3, InceptionV3
    sd, path = weights
    N, (kind, H, W), blocks, resize_input, normalize_input = WALKS[case]
    gen = _gen(sorted(WALKS).index(case) + 11)
    if kind == "uint8":
        monkeypatch.setenv("DXMI_FID_WEIGHTS", path)
        model = EvalInceptionV3().to(DEV)
        images = torch.randint(0, 256, (N, H, W, 3), generator=gen, device=DEV, dtype=torch.uint8)
        inp = images.permute(0, 3, 1, 2).float() / 255.0                     # what the evaluator's contract feeds the net
        rec, g, (pool, spatial), outs = walk(ops, model, sd, inp, lambda: model(images), True, True, [3])
        g.complete(rec)
        b1 = g.by_name["Mixed_6d.branch1x1"][0]
        assert b1.coff == 0 and b1.C == 192 and tuple(b1.out.shape) == (N, 17, 17, 768)
        assert spatial.dtype == torch.float32 and tuple(spatial.shape) == (N, 2023)
        assert torch.equal(spatial, b1.out[..., :7].float().reshape(N, -1)), "spatial is not Mixed_6d.branch1x1[..., :7] flattened NHWC"
        gap = g.by_name["pool3"][0]
        assert pool.dtype == torch.float32 and tuple(pool.shape) == (N, 2048) and torch.equal(pool, gap.out)
        ref, bound = fb.global_avgpool_ref(gap.x)
        CHECK.within("global_avgpool", pool, ref, bound)
        assert torch.equal(model.softmax_weight, sd["fc.weight"].t().contiguous().to(DEV)) and float(model.softmax_weight.abs().max()) > 0
        return
    model = InceptionV3(output_blocks=blocks, resize_input=resize_input, normalize_input=normalize_input, weights=sd).to(DEV)
    inp = torch.rand(N, 3, H, W, generator=gen, device=DEV)
    rec, g, outputs, outs = walk(ops, model, sd, inp, lambda: model(inp), resize_input, normalize_input, blocks)
    g.judge_taps(outs, outputs, blocks)
    g.complete(rec)
    assert rec.count("gconv") == 94 and rec.count("gconv_pack") == 94 and rec.count("pool3x3") == 13
    assert rec.count("nhwc_bf16_to_nchw_f32") == len([b for b in blocks if b < 3])
    if case == "n3_all_taps":
        assert [tuple(o.shape) for o in outputs] == [(3, 64, 73, 73), (3, 192, 35, 35), (3, 768, 17, 17), (3, 2048, 1, 1)]
    if case == "n2_noresize_139x203":
        assert tuple(g.by_name["pool3"][0].x.shape) == (2, 3, 5, 2048)


@pytest.mark.gpu
def test_unjudged_ops_call_is_refused(ops, weights):
    """The guard itself: an extractor that launches one more `ops` kernel than the six judged ones is refused by name."""
    from pytorch_fid.inception import InceptionV3
    sd, _ = weights
    model = InceptionV3(output_blocks=[0], weights=sd).to(DEV)
    inp = torch.rand(1, 3, 32, 32, generator=_gen(3), device=DEV)
    with iw.Recorder(ops, model) as rec:
        out = model(inp)[0]
        ops.nchw_f32_to_nhwc_bf16(out)                       # a launch op of the library that has no judge here
    assert rec.unknown == {"nchw_f32_to_nhwc_bf16"}
    with iw.Recorder(ops, model) as rec:
        model(inp)
    assert not rec.unknown and rec.count("gconv") == 3 and rec.count("gconv_pack") == 0      # packed once, cached


# ------------------------------------------------------------------------------------------------ launches the graph does not reach
PACK_ROWS = [   # (Cout, Cin, KH, KW, with BatchNorm)
    (32, 3, 3, 3, True), (32, 3, 3, 3, False), (80, 64, 1, 1, True), (80, 64, 1, 1, False), (33, 20, 1, 7, True), (8, 16, 7, 1, True),
    (448, 40, 3, 1, True),
]


def _bn(g, c):
    r = lambda: torch.rand(c, generator=g, device=DEV)
    return (0.5 + r(), 0.4 * r() - 0.2, 0.6 * r() - 0.3, 0.5 + r())


@pytest.mark.gpu
@pytest.mark.parametrize("row", PACK_ROWS, ids=str)
def test_gconv_pack(ops, row):
    Cout, Cin, KH, KW, with_bn = row
    g = _gen(hash(row) % (1 << 31))
    w = torch.randn(Cout, Cin, KH, KW, generator=g, device=DEV) * (2.0 / (Cin * KH * KW)) ** 0.5
    bn = _bn(g, Cout) if with_bn else None
    pk = ops.gconv_pack(w, bn, eps=1e-3)
    assert pk.w.numel() == (-(-Cout // 32) * 32) * KH * KW * (-(-Cin // 16) * 16)
    iw.judge_pack(CHECK, pk, w, bn, 1e-3)


SENT = 7.0      # sentinel of the channels outside a launch's window (exact in bf16)

GCONV_ROWS = [  # (N, IH, IW, Cin, Cout, (KH, KW), (SH, SW), (PH, PW), relu, coff, channels right of the window)
    (2, 9, 11, 32, 48, (3, 3), (1, 1), (1, 1), False, 0, 0),          # relu off
    (2, 17, 17, 64, 80, (1, 1), (1, 1), (0, 0), True, 8, 24),         # window inside a wider tensor, Cout 80 -> 96
    (3, 19, 23, 16, 32, (3, 3), (2, 1), (1, 1), True, 0, 0),          # SH != SW
    (2, 13, 13, 32, 64, (3, 5), (1, 1), (0, 2), True, 16, 8),         # PH != PW
    (3, 5, 5, 16, 40, (7, 7), (1, 1), (1, 1), True, 0, 0),            # kernel as large as the padded map: OH = OW = 1
    (2, 35, 35, 48, 8, (5, 5), (1, 1), (2, 2), True, 0, 0),           # Cout < 32
    (2, 17, 17, 128, 33, (1, 7), (1, 1), (0, 3), True, 3, 4),         # Cout = 33: one row of the second block, unaligned window
    (2, 17, 17, 160, 33, (7, 1), (1, 1), (3, 0), False, 1, 0),
    (2, 37, 37, 3, 32, (3, 3), (2, 2), (0, 0), True, 0, 0),           # Cin 3 -> 16
    (5, 8, 8, 448, 384, (3, 3), (1, 1), (1, 1), True, 0, 0),          # 320 pixels = 5 tiles exactly, Cin 448
    (1, 8, 8, 384, 320, (1, 3), (1, 1), (0, 1), True, 64, 64),        # 64 pixels = one tile, Cout 320 = 5 blocks of 64
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", GCONV_ROWS, ids=str)
def test_gconv(ops, row):
    N, IH, IW, Cin, Cout, k, s, p, relu, coff, right = row
    g = _gen(hash(row) % (1 << 31))
    CinP = -(-Cin // 16) * 16
    w = torch.randn(Cout, Cin, *k, generator=g, device=DEV) * (2.0 / (Cin * k[0] * k[1])) ** 0.5
    pk = ops.gconv_pack(w, _bn(g, Cout), eps=1e-3)
    x = torch.zeros(N, IH, IW, CinP, dtype=torch.bfloat16, device=DEV)
    x[..., :Cin] = torch.randn(N, IH, IW, Cin, generator=g, device=DEV).to(torch.bfloat16)
    OH, OW = (IH + 2 * p[0] - k[0]) // s[0] + 1, (IW + 2 * p[1] - k[1]) // s[1] + 1
    wide = torch.full((N, OH, OW, coff + Cout + right), SENT, dtype=torch.bfloat16, device=DEV)
    ret = ops.gconv(x, pk, stride=s, pad=p, relu=relu, out=wide, coff=coff)
    assert ret is wide
    w4 = fb.gconv_unpack(pk.w, Cout, Cin, *k)[:Cout]
    iw.judge_gconv(CHECK, wide[..., coff:coff + Cout], x, w4, pk.bias[:Cout], s, p, relu)
    assert bool((wide[..., :coff] == SENT).all()) and bool((wide[..., coff + Cout:] == SENT).all()), "wrote outside its channel window"
    if coff == 0 and right == 0:
        assert torch.equal(ops.gconv(x, pk, stride=s, pad=p, relu=relu), wide)         # the allocating form is the same launch


POOL_ROWS = [   # (N, IH, IW, C, stride, pad, avg, coff, channels right of the window)
    (2, 9, 11, 16, 2, 1, False, 0, 0), (2, 9, 11, 16, 2, 1, True, 0, 0),       # stride 2 with padding
    (3, 3, 3, 8, 1, 0, False, 0, 0), (3, 3, 3, 8, 1, 0, True, 0, 0),           # one output
    (2, 2, 5, 8, 1, 1, True, 0, 0), (2, 2, 5, 8, 1, 1, False, 0, 0),           # 2-row map: cnt = 6 / 4
    (2, 7, 7, 24, 1, 1, True, 8, 16), (2, 7, 6, 24, 2, 0, False, 16, 8),       # window next to sentinels
    (2, 17, 17, 32, 1, 1, True, 0, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", POOL_ROWS, ids=str)
def test_pool3x3(ops, row):
    N, IH, IW, C, stride, pad, avg, coff, right = row
    x = torch.randn(N, IH, IW, C, generator=_gen(hash(row) % (1 << 31)), device=DEV).to(torch.bfloat16)
    OH, OW = (IH + 2 * pad - 3) // stride + 1, (IW + 2 * pad - 3) // stride + 1
    wide = torch.full((N, OH, OW, coff + C + right), SENT, dtype=torch.bfloat16, device=DEV)
    assert ops.pool3x3(x, stride, pad, avg_exclude_pad=avg, out=wide, coff=coff) is wide
    got = wide[..., coff:coff + C]
    if avg:
        ref, bound, cnt = fb.avgpool3x3_ref(x, stride, pad)
        CHECK.within("avgpool3x3", got, ref, bound)
        if (IH, pad) == (2, 1):
            assert sorted(set(cnt.flatten().tolist())) == [4.0, 6.0]
    else:
        assert torch.equal(got.double(), fb.maxpool3x3_ref(x, stride, pad))
    assert bool((wide[..., :coff] == SENT).all()) and bool((wide[..., coff + C:] == SENT).all()), "wrote outside its channel window"


RESIZE_ROWS = [  # (N, IH, IW, OH, OW, normalize)
    (2, 32, 32, 299, 299, True), (2, 64, 64, 299, 299, True), (1, 256, 256, 299, 299, True), (2, 299, 299, 299, 299, True),
    (1, 512, 512, 299, 299, True), (2, 139, 203, 299, 299, True), (2, 48, 80, 151, 77, True), (2, 32, 32, 299, 299, False),
    (2, 139, 203, 139, 203, False),
]


def test_resize_bound_holds_for_the_fp32_emulation():
    """Host-side: the kernel's fp32 expressions, emulated by torch on the CPU, stay inside the pre-store part of the resize bound for
    every resize case of this module (measured 0.10 - 0.13 of it, 0 for a same-size resize), the bf16-rounded emulation inside
    the whole bound, and the closed-form fp64 reference agrees with F.interpolate in fp64."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)
    rows = RESIZE_ROWS + [(N, H, W, 299 if rs else H, 299 if rs else W, nm) for N, (_, H, W), _, rs, nm in WALKS.values()]
    for (N, IH, IW, OH, OW, nm) in rows:
        x = torch.rand(min(N, 2), 3, IH, IW, generator=g)
        ref, bound = fb.resize_ref(x, OH, OW, nm)
        it = F.interpolate(x.double(), size=(OH, OW), mode="bilinear", align_corners=False)
        assert float((ref - (2 * it - 1 if nm else it).permute(0, 2, 3, 1)).abs().max()) < 1e-13
        em = fb.resize_emulate_f32(x, OH, OW, nm)
        core = (bound - (fb.U16 + 4 * fb.U32) * ref.abs()) / (1 + fb.U16)
        assert float(((em.double() - ref).abs() / core).max()) < 0.5, (IH, IW, OH, OW)
        assert float(((em.to(torch.bfloat16).double() - ref).abs() / bound).max()) <= 1.0, (IH, IW, OH, OW)


@pytest.mark.gpu
@pytest.mark.parametrize("row", RESIZE_ROWS, ids=str)
def test_resize(ops, row):
    N, IH, IW, OH, OW, nm = row
    x = torch.rand(N, 3, IH, IW, generator=_gen(hash(row) % (1 << 31)), device=DEV)
    iw.judge_resize(CHECK, ops.resize_bilinear_nhwc16(x, OH, OW, normalize=nm), x, OH, OW, nm)


GAP_ROWS = [(3, 1, 1, 2048), (2, 8, 8, 2048), (2, 17, 17, 768), (3, 17, 17, 200), (1, 1, 1, 8), (50, 8, 8, 2048)]


@pytest.mark.gpu
@pytest.mark.parametrize("row", GAP_ROWS, ids=str)
def test_global_avgpool(ops, row):
    N, H, W, C = row
    x = torch.randn(N, H, W, C, generator=_gen(hash(row) % (1 << 31)), device=DEV).to(torch.bfloat16)
    got = ops.global_avgpool(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, C)
    ref, bound = fb.global_avgpool_ref(x)
    CHECK.within("global_avgpool", got, ref, bound)


def test_fp64_references_match_the_oracle_on_a_tiny_input():
    """Host-side: the fp64 references the walk judges with, chained as the oracle chains them on CPU tensors (fp64 activations,
    fp32 weights folded in fp64), reproduce oracle.inception.forward (fp32) on a 75 x 75 input without resize."""
    from oracle import inception as oinc
    from pytorch_fid.inception import InceptionV3
    sd = iw.tv_state_dict(InceptionV3())

    class Ref64(oinc.Graph):
        def prep(self, x, resize_input, normalize_input):
            return fb.resize_ref(x, *x.shape[2:], normalize_input)[0].permute(0, 3, 1, 2)

        def bc(self, sd, name, x, stride=1, padding=0):
            bn = tuple(sd[f"{name}.bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
            fold, bias, _ = fb.gconv_pack_ref(sd[name + ".conv.weight"], bn, 1e-3)
            ref, _ = fb.gconv_ref(x.permute(0, 2, 3, 1), fold, bias, iw._pair(stride), iw._pair(padding))
            return ref.clamp_min(0).permute(0, 3, 1, 2)

        def avg(self, where, x):
            return fb.avgpool3x3_ref(x.permute(0, 2, 3, 1), 1, 1)[0].permute(0, 3, 1, 2)

        def maxpool(self, where, x, stride, padding=0):
            return fb.maxpool3x3_ref(x.permute(0, 2, 3, 1), stride, padding).permute(0, 3, 1, 2)

        def gap(self, where, x):
            return fb.global_avgpool_ref(x.permute(0, 2, 3, 1))[0][:, :, None, None]

    x = torch.rand(1, 3, 75, 75, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = oinc.forward(sd, x, resize_input=False)
        got = oinc.forward(sd, x, resize_input=False, g=Ref64())
    for a, b in zip(got, want):
        assert a.shape == b.shape and float((a - b.double()).norm() / b.double().norm()) < 1e-5


@pytest.mark.gpu
def test_report():
    """Largest |err| / bound per op over the cases above (printed; run with -s)."""
    for k, v in CHECK.report().items():
        print(f"{k:48s} {v:.4f}")
