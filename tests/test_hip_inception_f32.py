"""The fp32 mode of the FID / evaluator InceptionV3 (pytorch_fid/inception.py precision="fp32", dxmi_hip/inception_f32_ops.py,
csrc/inception_f32.hip): every launch against fp64, element by element, with fp32-output bounds (inception_walk_f32.py states them).

Row tests: seeded inputs, a sentinel-filled wide output (untouched outside the window), no element left out, every launch run
twice with identical bits.  test_walk_f32 records every launch of an fp32 forward ("record or refuse" over the public functions of
the fp32 ops module, nested in inception_walk.Recorder over dxmi_hip.ops, which must see no launch at all) and walks
oracle.inception.forward over the recorded device tensors: bitwise dataflow, bounds, 94 convs visited once, launches judged ==
launches recorded per op.  Batch independence: image 2's pool3 features are the same bits at N = 1 and inside N = 5; the bf16
program gives the same bits before and after an fp32 forward on the same model object.  End to end (N = 2, 32x32, formula weights):
per image, the rel-L2 error of the fp32 program's pool3 features against oracle.inception.forward in float64 on the CPU is at most
1/64 of the bf16 program's (one bf16 store rounding per layer is ~0.3 u16 rms ~ 2e4 u32; an fp32 chain of depth K <= 18432 costs
~sqrt(K) u32 <= 136 u32 rms: a ratio >= ~140 in the worst layer, 1/64 leaves a factor of two).  The two CLI tests run
train_cifar10.py --fid_extractor pytorch_fid.inception:FIDInceptionV3FP32 and evaluator.py --extractor
pytorch_fid.inception:EvalInceptionV3FP32 on a formula-weight file, each in a child process with its own time limit (their time
goes to the 2 400 / 2 x 2 560 images that a full-rank 2048 x 2048 covariance needs and to the matrix square roots).

All references are stock torch in float64; no project kernel takes part in one.  PARITY with the reference's weights stays
unpinned (the FID weight file is absent): the weights are inception_walk.tv_state_dict's formula weights.

Measured on an MI355X (test_report / test_end_to_end print them): worst |err| / bound 0.002 - 0.067 for the convs
(the bound is a worst case in K, the error grows like sqrt(K)), 0.38 average pool, 0.56 / 0.31 packed scale / shift, 0.21 global
average pool, 0.14 resize.  pool3 rel-L2 against float64, per image: bf16 program 4.9e-3 / 5.1e-3, fp32 program 8.2e-7 / 8.3e-7,
torch fp32 on the CPU 6.9e-7 / 8.6e-7: the fp32 program is ~6000 times closer than the bf16 one.  The module runs in ~27 s, 15 s
of them the two child processes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import forward_bounds as fb
import inception_walk as iw
import inception_walk_f32 as iwf
from forward_bounds import FwdChecker

DEV = "cuda:0"
CHECK = FwdChecker()
SENT = 7.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffusion-by-maxentirl_amd")
TESTS = os.path.join(ROOT, "tests")


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


@pytest.fixture(scope="module")
def f32ops(ops):
    from dxmi_hip import inception_f32_ops
    return inception_f32_ops


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    """(state dict on the CPU, path of the torch.save'd file): formula weights, non-zero fc.weight."""
    from pytorch_fid.inception import InceptionV3
    sd = iw.tv_state_dict(InceptionV3(), fc=True)
    path = tmp_path_factory.mktemp("fid_weights_f32") / "pt_inception.pth"
    torch.save(sd, path)
    return sd, str(path)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _seed(row):
    return hash(row) % (1 << 31)


def _bn(g, c):
    r = lambda: torch.rand(c, generator=g, device=DEV)
    return (0.5 + r(), 0.4 * r() - 0.2, 0.6 * r() - 0.3, 0.5 + r())


def _sentinel_untouched(wide, coff, C):
    assert bool((wide[..., :coff] == SENT).all()) and bool((wide[..., coff + C:] == SENT).all()), "wrote outside its channel window"


# ------------------------------------------------------------------------------------------------ row tests
GCONV_ROWS = [  # (N, IH, IW, Cin, Cout, (KH, KW), (SH, SW), (PH, PW), relu, coff, channels right of the window)
    (2, 9, 11, 32, 48, (3, 3), (1, 1), (1, 1), False, 0, 0),          # relu off
    (2, 17, 17, 64, 80, (1, 1), (1, 1), (0, 0), True, 8, 24),         # window inside a wider tensor
    (3, 19, 23, 8, 32, (3, 3), (2, 1), (1, 1), True, 0, 0),           # one granule per tap, SH != SW
    (2, 13, 13, 24, 64, (3, 5), (1, 1), (0, 2), True, 16, 8),         # three granules, PH != PW
    (3, 5, 5, 16, 40, (7, 7), (1, 1), (1, 1), True, 0, 0),            # one output pixel
    (2, 35, 35, 48, 8, (5, 5), (1, 1), (2, 2), True, 0, 0),           # Cout < 32
    (2, 17, 17, 128, 33, (1, 7), (1, 1), (0, 3), True, 3, 4),         # unaligned channel window
    (2, 17, 17, 160, 33, (7, 1), (1, 1), (3, 0), False, 1, 0),        # Cout = 33, relu off
    (2, 37, 37, 3, 32, (3, 3), (2, 2), (0, 0), True, 0, 0),           # Cin 3, padded to 8
    (5, 8, 8, 448, 384, (3, 3), (1, 1), (1, 1), True, 0, 0),          # K = 4032, the net's longest chain; whole tiles
    (1, 8, 8, 2048, 320, (1, 1), (1, 1), (0, 0), True, 64, 64),       # K = 2048
    (1, 8, 8, 384, 320, (1, 3), (1, 1), (0, 1), True, 0, 0),          # (1, 3) kernel
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", GCONV_ROWS, ids=str)
def test_gconv_f32(f32ops, row):
    N, IH, IW, Cin, Cout, k, s, p, relu, coff, right = row
    g = _gen(_seed(row))
    CinP = -(-Cin // 8) * 8
    w = torch.randn(Cout, Cin, *k, generator=g, device=DEV) * (2.0 / (Cin * k[0] * k[1])) ** 0.5
    pk = f32ops.gconv_pack(w, _bn(g, Cout), eps=1e-3)
    x = torch.zeros(N, IH, IW, CinP, device=DEV)
    x[..., :Cin] = torch.randn(N, IH, IW, Cin, generator=g, device=DEV)
    OH, OW = (IH + 2 * p[0] - k[0]) // s[0] + 1, (IW + 2 * p[1] - k[1]) // s[1] + 1
    wide = torch.full((N, OH, OW, coff + Cout + right), SENT, device=DEV)
    assert f32ops.gconv(x, pk, stride=s, pad=p, relu=relu, out=wide, coff=coff) is wide
    w4 = iwf.gconv_unpack_f32(pk.w, Cout, Cin, *k)[:Cout]
    assert torch.equal(w4[:, :Cin], w)
    iwf.judge_gconv_f32(CHECK, wide[..., coff:coff + Cout], x, w4, pk.scale[:Cout], pk.shift[:Cout], s, p, relu)
    _sentinel_untouched(wide, coff, Cout)
    again = torch.full_like(wide, SENT)
    f32ops.gconv(x, pk, stride=s, pad=p, relu=relu, out=again, coff=coff)
    assert torch.equal(again, wide), "two launches on the same operands differ"
    if coff == 0 and right == 0:
        assert torch.equal(f32ops.gconv(x, pk, stride=s, pad=p, relu=relu), wide)         # the allocating form is the same launch


PACK_ROWS = [   # (Cout, Cin, KH, KW, with BatchNorm): test_hip_inception_launches.PACK_ROWS
    (32, 3, 3, 3, True), (32, 3, 3, 3, False), (80, 64, 1, 1, True), (80, 64, 1, 1, False), (33, 20, 1, 7, True), (8, 16, 7, 1, True),
    (448, 40, 3, 1, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", PACK_ROWS, ids=str)
def test_gconv_pack_f32(f32ops, row):
    Cout, Cin, KH, KW, with_bn = row
    g = _gen(_seed(row))
    w = torch.randn(Cout, Cin, KH, KW, generator=g, device=DEV) * (2.0 / (Cin * KH * KW)) ** 0.5
    bn = _bn(g, Cout) if with_bn else None
    pk = f32ops.gconv_pack(w, bn, eps=1e-3)
    assert pk.w.numel() == (-(-Cout // 32) * 32) * KH * KW * (-(-Cin // 8) * 8)
    iwf.judge_pack_f32(CHECK, pk, w, bn, 1e-3)
    again = f32ops.gconv_pack(w, bn, eps=1e-3)
    assert all(torch.equal(getattr(again, k), getattr(pk, k)) for k in ("w", "scale", "shift"))
    if not with_bn:
        bias = torch.randn(Cout, generator=g, device=DEV)
        iwf.judge_pack_f32(CHECK, f32ops.gconv_pack(w, None, bias=bias), w, None, 1e-3, bias=bias)


POOL_ROWS = [   # (N, IH, IW, C, stride, pad, avg, coff, right): the shapes of the bf16 suite's POOL_ROWS, C of one and three granules
    (2, 9, 11, 8, 2, 1, False, 0, 0), (2, 9, 11, 24, 2, 1, True, 0, 0),
    (3, 3, 3, 8, 1, 0, False, 0, 0), (3, 3, 3, 24, 1, 0, True, 0, 0),
    (2, 2, 5, 8, 1, 1, True, 0, 0), (2, 2, 5, 24, 1, 1, False, 0, 0),
    (2, 7, 7, 24, 1, 1, True, 8, 16), (2, 7, 6, 24, 2, 0, False, 16, 8), (2, 7, 7, 8, 1, 1, False, 4, 4),
    (2, 17, 17, 24, 1, 1, True, 0, 0), (2, 17, 17, 8, 1, 1, True, 0, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", POOL_ROWS, ids=str)
def test_pool3x3_f32(f32ops, row):
    N, IH, IW, C, stride, pad, avg, coff, right = row
    x = torch.randn(N, IH, IW, C, generator=_gen(_seed(row)), device=DEV)
    OH, OW = (IH + 2 * pad - 3) // stride + 1, (IW + 2 * pad - 3) // stride + 1
    wide = torch.full((N, OH, OW, coff + C + right), SENT, device=DEV)
    assert f32ops.pool3x3(x, stride, pad, avg_exclude_pad=avg, out=wide, coff=coff) is wide
    got = wide[..., coff:coff + C]
    if avg:
        ref, bound, cnt = iwf.avgpool_f32_ref(x, stride, pad)
        CHECK.within("avgpool3x3_f32", got, ref, bound)
        if (IH, pad) == (2, 1):
            assert sorted(set(cnt.flatten().tolist())) == [4.0, 6.0]
    else:
        assert torch.equal(got.double(), fb.maxpool3x3_ref(x, stride, pad))
    _sentinel_untouched(wide, coff, C)
    again = torch.full_like(wide, SENT)
    f32ops.pool3x3(x, stride, pad, avg_exclude_pad=avg, out=again, coff=coff)
    assert torch.equal(again, wide)


RESIZE_ROWS = [  # (N, IH, IW, OH, OW, normalize): test_hip_inception_launches.RESIZE_ROWS
    (2, 32, 32, 299, 299, True), (2, 64, 64, 299, 299, True), (1, 256, 256, 299, 299, True), (2, 299, 299, 299, 299, True),
    (1, 512, 512, 299, 299, True), (2, 139, 203, 299, 299, True), (2, 48, 80, 151, 77, True), (2, 32, 32, 299, 299, False),
    (2, 139, 203, 139, 203, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", RESIZE_ROWS, ids=str)
def test_resize_f32(f32ops, row):
    N, IH, IW, OH, OW, nm = row
    x = torch.rand(N, 3, IH, IW, generator=_gen(_seed(row)), device=DEV)
    got = f32ops.resize_bilinear_nhwc(x, OH, OW, normalize=nm)
    iwf.judge_resize_f32(CHECK, got, x, OH, OW, nm)
    assert torch.equal(f32ops.resize_bilinear_nhwc(x, OH, OW, normalize=nm), got)


GAP_ROWS = [(3, 1, 1, 2048), (2, 8, 8, 2048), (2, 17, 17, 768), (3, 17, 17, 200), (1, 1, 1, 8), (50, 8, 8, 2048)]


@pytest.mark.gpu
@pytest.mark.parametrize("row", GAP_ROWS, ids=str)
def test_global_avgpool_f32(f32ops, row):
    N, H, W, C = row
    x = torch.randn(N, H, W, C, generator=_gen(_seed(row)), device=DEV)
    got = f32ops.global_avgpool(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, C)
    ref, bound = fb.global_avgpool_ref(x)
    CHECK.within("global_avgpool_f32", got, ref, bound)
    assert torch.equal(f32ops.global_avgpool(x), got)


@pytest.mark.gpu
def test_nhwc_to_nchw_f32(f32ops):
    x = torch.randn(3, 5, 7, 24, generator=_gen(5), device=DEV)
    got = f32ops.nhwc_to_nchw(x)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (3, 24, 5, 7) and torch.equal(got, x.permute(0, 3, 1, 2))
    out = torch.full((3, 24, 5, 7), SENT, device=DEV)
    assert f32ops.nhwc_to_nchw(x, out=out) is out and torch.equal(out, got)


@pytest.mark.gpu
def test_wrappers_refuse_malformed_tensors(f32ops):
    from dxmi_hip import DxmiError
    w = torch.randn(32, 8, 3, 3, device=DEV)
    pk = f32ops.gconv_pack(w)
    x = torch.randn(1, 5, 5, 8, device=DEV)
    with pytest.raises(DxmiError):
        f32ops.gconv(x.to(torch.bfloat16), pk)                                       # dtype
    with pytest.raises(DxmiError):
        f32ops.gconv(torch.randn(1, 5, 5, 16, device=DEV), pk)                       # channels
    with pytest.raises(DxmiError):
        f32ops.gconv(x, pk, out=torch.empty(1, 3, 3, 40, device=DEV), coff=16)       # window outside the output
    with pytest.raises(DxmiError):
        f32ops.gconv(x[:, :2, :2].contiguous(), pk)                                  # kernel larger than the map
    with pytest.raises(DxmiError):
        f32ops.pool3x3(torch.randn(1, 5, 5, 12, device=DEV), 1, 1)                   # granule
    with pytest.raises(DxmiError):
        f32ops.pool3x3(x, 1, 1, out=torch.empty(1, 5, 5, 18, device=DEV), coff=2)    # unaligned window
    with pytest.raises(DxmiError):
        f32ops.global_avgpool(torch.randn(1, 2, 2, 12, device=DEV))
    with pytest.raises(DxmiError):
        f32ops.resize_bilinear_nhwc(torch.rand(1, 4, 8, 8, device=DEV), 16, 16)
    with pytest.raises(DxmiError):
        f32ops.gconv_pack(w, _bn(_gen(1), 32), bias=torch.zeros(32, device=DEV))


# ------------------------------------------------------------------------------------------------ the program, launch by launch
WALKS = {   # id -> (N, input, output_blocks, resize_input, normalize_input)
    "n3_all_taps": (3, ("float", 32, 32), [0, 1, 2, 3], True, True),
    "n2_noresize_139x203": (2, ("float", 139, 203), [3], False, False),
    "n16_eval_uint8": (16, ("uint8", 64, 64), None, True, True),
}


def walk(ops, f32ops, model, sd, inp, run, resize_input, normalize_input):
    from oracle import inception as oinc
    with iw.Recorder(ops, model) as bf, iwf.RecorderF32(f32ops, model) as rec:
        ret = run()
    torch.cuda.synchronize()
    assert not bf.unknown and not bf.records, f"the fp32 program called dxmi_hip.ops: {sorted(bf.unknown)} {[r.op for r in bf.records]}"
    assert not rec.unknown, f"public names of the fp32 ops module that are neither judged launches nor known classes: {sorted(rec.unknown)}"
    g = iwf.DeviceGraphF32(rec, model, sd, CHECK)
    g.judge_packs()
    outs = oinc.forward(sd, inp, resize_input=resize_input, normalize_input=normalize_input, last_block=3, g=g)
    return rec, g, ret, outs


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(WALKS))
def test_walk_f32(ops, f32ops, weights, monkeypatch, case):
    from pytorch_fid.inception import EvalInceptionV3FP32, InceptionV3
    sd, path = weights
    N, (kind, H, W), blocks, resize_input, normalize_input = WALKS[case]
    gen = _gen(sorted(WALKS).index(case) + 31)
    if kind == "uint8":
        monkeypatch.setenv("DXMI_FID_WEIGHTS", path)
        model = EvalInceptionV3FP32().to(DEV)
        assert model.precision == "fp32"
        images = torch.randint(0, 256, (N, H, W, 3), generator=gen, device=DEV, dtype=torch.uint8)
        inp = images.permute(0, 3, 1, 2).float() / 255.0
        rec, g, (pool, spatial), outs = walk(ops, f32ops, model, sd, inp, lambda: model(images), True, True)
        g.complete(rec)
        b1 = g.by_name["Mixed_6d.branch1x1"][0]
        assert b1.coff == 0 and b1.C == 192 and tuple(b1.out.shape) == (N, 17, 17, 768) and b1.out.dtype == torch.float32
        assert spatial.dtype == torch.float32 and tuple(spatial.shape) == (N, 2023)
        assert torch.equal(spatial, b1.out[..., :7].reshape(N, -1)), "spatial is not Mixed_6d.branch1x1[..., :7] of the fp32 tensor"
        gap = g.by_name["pool3"][0]
        assert pool.dtype == torch.float32 and tuple(pool.shape) == (N, 2048) and torch.equal(pool, gap.out)
        assert torch.equal(model.softmax_weight, sd["fc.weight"].t().contiguous().to(DEV))
        return
    model = InceptionV3(output_blocks=blocks, resize_input=resize_input, normalize_input=normalize_input, weights=sd, precision="fp32").to(DEV)
    inp = torch.rand(N, 3, H, W, generator=gen, device=DEV)
    rec, g, outputs, outs = walk(ops, f32ops, model, sd, inp, lambda: model(inp), resize_input, normalize_input)
    g.judge_taps(outs, outputs, blocks)
    g.complete(rec)
    assert rec.count("gconv") == 94 and rec.count("gconv_pack") == 94 and rec.count("pool3x3") == 13
    assert rec.count("nhwc_to_nchw") == len([b for b in blocks if b < 3])
    if case == "n3_all_taps":
        assert [tuple(o.shape) for o in outputs] == [(3, 64, 73, 73), (3, 192, 35, 35), (3, 768, 17, 17), (3, 2048, 1, 1)]
        with iwf.RecorderF32(f32ops, model) as rec2:
            again = model(inp)
        assert rec2.count("gconv") == 94 and rec2.count("gconv_pack") == 0                     # packed once, cached
        assert all(torch.equal(a, b) for a, b in zip(again, outputs)), "two forwards on the same input differ"
    if case == "n2_noresize_139x203":
        assert tuple(g.by_name["pool3"][0].x.shape) == (2, 3, 5, 2048)


# ------------------------------------------------------------------------------------------------ batch independence, caches
@pytest.mark.gpu
def test_pool3_does_not_depend_on_the_batch(weights):
    from pytorch_fid.inception import InceptionV3
    sd, _ = weights
    model = InceptionV3(weights=sd, precision="fp32").to(DEV)
    inp = torch.rand(5, 3, 32, 32, generator=_gen(77), device=DEV)
    inside = model(inp)[0][2]
    alone = model(inp[2:3].clone())[0][0]
    assert torch.equal(inside, alone), "image 2's pool3 features differ between N = 1 and N = 5"


@pytest.mark.gpu
def test_bf16_program_unchanged_after_an_fp32_forward(weights):
    from pytorch_fid.inception import InceptionV3
    sd, _ = weights
    model = InceptionV3(output_blocks=[2, 3], weights=sd).to(DEV)
    assert model.precision == "bf16"
    inp = torch.rand(2, 3, 32, 32, generator=_gen(78), device=DEV)
    before = [t.clone() for t in model(inp)]
    pk16 = model._packed
    model.precision = "fp32"
    f32 = model(inp)
    pk32 = model._packed
    assert pk32 is not pk16 and all(v.w.dtype == torch.float32 for v in pk32.values()) and all(v.w.dtype == torch.bfloat16 for v in pk16.values())
    model.precision = "bf16"
    after = model(inp)
    assert model._packed is pk16, "the bf16 weights were packed again"
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "the bf16 program changed after an fp32 forward on the same model"
    assert not torch.equal(f32[1], before[1])
    with pytest.raises(ValueError):
        model.precision = "fp16"
    model.load_fid_weights(sd)
    assert model._packed is None                                                        # both caches dropped


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.gpu
def test_end_to_end_fp32_is_64x_closer_to_fp64_than_bf16(weights):
    """Measured on an MI355X (per image): bf16 4.9e-3 / 5.1e-3, fp32 8.2e-7 / 8.3e-7, torch fp32 on the CPU 6.9e-7 / 8.6e-7."""
    from oracle import inception as oinc
    from pytorch_fid.inception import InceptionV3
    sd, _ = weights
    inp = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(5))
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        ref = oinc.forward(sd64, inp.double())[3].reshape(2, -1)
        cpu32 = oinc.forward(sd, inp)[3].reshape(2, -1).double()
    model = InceptionV3(weights=sd).to(DEV)
    bf = model(inp.to(DEV))[0].reshape(2, -1).double().cpu()
    model.precision = "fp32"
    fp = model(inp.to(DEV))[0].reshape(2, -1).double().cpu()
    rel = lambda t: ((t - ref).norm(dim=1) / ref.norm(dim=1))
    e16, e32, ecpu = rel(bf), rel(fp), rel(cpu32)
    print(f"pool3 rel-L2 vs float64 per image: bf16 program {e16.tolist()}  fp32 program {e32.tolist()}  torch fp32 on the CPU {ecpu.tolist()}"
          f"  ratio bf16 / fp32 {(e16 / e32).tolist()}")
    assert bool((e32 <= e16 / 64).all()), (e32.tolist(), e16.tolist())


# ------------------------------------------------------------------------------------------------ the scripts name the classes
@pytest.mark.gpu
def test_cli_train_cifar10_fid_extractor_fp32(weights, tmp_path):
    import re
    import shutil
    _, path = weights
    stats = str(tmp_path / "stats.npz")
    np.savez(stats, mu=np.zeros(2048), sigma=np.eye(2048))
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1", PWD=PKG, DXMI_FID_WEIGHTS=path)
    cmd = [sys.executable, "train_cifar10.py", "--config", "builtin:cifar10_T10", "--dataset", "builtin", "--synthetic_data", "--max_iters", "1",
           "--run", "fid_fp32", "--fid_extractor", "pytorch_fid.inception:FIDInceptionV3FP32", "--fid_stats", stats,
           "--training.fid_every", "1", "--training.fid_epoch", "null", "--training.n_fid_samples", "2400", "--training.sampling_batchsize", "200"]      # 2400 > 2048 features: a full-rank covariance
    try:
        r = subprocess.run(cmd, cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        scores = [float(v) for v in re.findall(r"FID score: ([-0-9.e+naif]+)", r.stdout)]
        print(r.stdout[-600:])
        assert len(scores) >= 1 and all(np.isfinite(scores))
    finally:
        shutil.rmtree(os.path.join(PKG, "results", "cifar10", "cifar10_T10", "fid_fp32"), ignore_errors=True)


@pytest.mark.gpu
def test_cli_evaluator_extractor_fp32(weights, tmp_path):
    _, path = weights
    rs = np.random.RandomState(9)
    rp, sp = str(tmp_path / "ref.npz"), str(tmp_path / "sample.npz")
    np.savez(rp, rs.randint(0, 256, (2560, 32, 32, 3)).astype(np.uint8))                 # more images than features (2048 / 2023)
    np.savez(sp, rs.randint(0, 224, (2560, 32, 32, 3)).astype(np.uint8))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([TESTS, PKG, ROOT]), DXMI_FID_WEIGHTS=path)
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluations", "evaluator.py"), rp, sp, "--extractor",
                        "pytorch_fid.inception:EvalInceptionV3FP32", "--batch_size", "256"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.split(":")[0] in ("Inception Score", "FID", "sFID", "Precision", "Recall")]
    assert [l.split(":")[0] for l in lines] == ["Inception Score", "FID", "sFID", "Precision", "Recall"], r.stdout
    assert all(np.isfinite(float(l.split(":", 1)[1])) for l in lines), r.stdout


@pytest.mark.gpu
def test_report():
    """Largest |err| / bound per op family over the cases above (printed; run with -s)."""
    for k, v in CHECK.report().items():
        print(f"{k:48s} {v:.4f}")
