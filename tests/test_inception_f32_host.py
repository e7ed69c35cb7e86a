"""Host-side tests of the fp32 InceptionV3 mode (csrc/inception_f32.hip, dxmi_hip/inception_f32_ops.py, pytorch_fid/inception.py): the
C ABI's symbols and argument validation (through ctypes with never-dereferenced pointers), the Python surface's refusals, and
CPU-only controls showing that the fp32 bounds of inception_walk_f32.py separate fp32 from bf16 arithmetic."""
import ctypes
import os
import re

import pytest
import torch

import forward_bounds as fb
import inception_walk_f32 as iwf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1       # DXMI_EINVAL
SYMBOLS = ("dxmi_gconv_f32_packed_elems", "dxmi_gconv_f32_pack", "dxmi_gconv_f32_fwd", "dxmi_pool3x3_f32", "dxmi_global_avgpool_f32",
           "dxmi_resize_bilinear_nhwc_f32", "dxmi_nhwc_f32_to_nchw_f32")


def test_symbols_are_declared_exported_and_bound():
    from dxmi_hip import _lib
    text = open(os.path.join(ROOT, "include", "dxmi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dxmi_[a-z0-9_]+)\s*\(", text))
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/dxmi_hip.h"
        assert hasattr(lib, s), f"{s} is not exported by the library"
        assert s in _lib.SIGNATURES
    assert _lib.load().dxmi_gconv_f32_packed_elems(33, 3, 1, 7) == 64 * 7 * 8
    assert _lib.load().dxmi_gconv_f32_packed_elems(0, 3, 1, 7) == 0


def test_entries_reject_bad_arguments():
    """Every entry point validates before it touches the device: EINVAL and a message."""
    from dxmi_hip import _lib
    lib = _lib.load()
    p, null = ctypes.c_void_p(64), ctypes.c_void_p(0)                 # never dereferenced: every call below fails its argument check
    err = lambda: lib.dxmi_last_error()

    def conv(x=p, w=p, scale=p, shift=p, out=p, N=2, IH=9, IW=9, Cin=16, Cout=40, KH=3, KW=3, SH=1, SW=1, PH=1, PW=1, cs=40, co=0, relu=1):
        return lib.dxmi_gconv_f32_fwd(x, w, scale, shift, out, N, IH, IW, Cin, Cout, KH, KW, SH, SW, PH, PW, cs, co, relu, null)
    for k in ("x", "w", "scale", "shift", "out"):
        assert conv(**{k: null}) == EINVAL and b"null pointer" in err(), k
    for k in ("N", "IH", "IW", "Cin", "Cout", "KH", "KW", "SH", "SW"):
        assert conv(**{k: 0}) == EINVAL and conv(**{k: -2}) == EINVAL and b"bad shape" in err(), k
    assert conv(PH=-1) == EINVAL and conv(PW=-1) == EINVAL
    assert conv(Cin=12) == EINVAL and b"multiple of 8" in err()
    assert conv(Cin=3) == EINVAL
    assert conv(cs=39) == EINVAL and b"channel window" in err()
    assert conv(cs=48, co=9) == EINVAL and conv(co=-1) == EINVAL
    assert conv(cs=2 ** 31 - 1, co=2 ** 31 - 8) == EINVAL                                    # co + Cout overflows int32
    assert conv(IH=5, IW=5, KH=8, KW=8) == EINVAL and b"does not fit" in err()
    assert conv(IH=1, KH=4, PH=1) == EINVAL and conv(IW=2, KW=5, PW=1) == EINVAL
    assert conv(N=2 ** 30, IH=2 ** 10, IW=2 ** 10) == EINVAL and b"too many pixels" in err()

    def pack(w=p, g=p, b=p, m=p, v=p, bias=null, wp=p, scale=p, shift=p, Cout=32, Cin=3, KH=3, KW=3):
        return lib.dxmi_gconv_f32_pack(w, g, b, m, v, 1e-3, bias, wp, scale, shift, Cout, Cin, KH, KW, null)
    for k in ("w", "wp", "scale", "shift"):
        assert pack(**{k: null}) == EINVAL and b"null pointer" in err(), k
    for k in ("Cout", "Cin", "KH", "KW"):
        assert pack(**{k: 0}) == EINVAL and pack(**{k: -1}) == EINVAL and b"bad shape" in err(), k
    assert pack(b=null) == EINVAL and pack(m=null) == EINVAL and pack(v=null) == EINVAL and b"BatchNorm needs" in err()
    assert pack(bias=p) == EINVAL and b"excludes BatchNorm" in err()
    assert pack(Cout=2 ** 20, Cin=2 ** 20) == EINVAL and b"too large" in err()

    def pool(x=p, out=p, N=2, IH=7, IW=7, C=24, stride=1, pad=1, avg=1, cs=24, co=0):
        return lib.dxmi_pool3x3_f32(x, out, N, IH, IW, C, stride, pad, avg, cs, co, null)
    assert pool(x=null) == EINVAL and pool(out=null) == EINVAL and b"null pointer" in err()
    for k in ("N", "IH", "IW", "C", "stride"):
        assert pool(**{k: 0}) == EINVAL and pool(**{k: -1}) == EINVAL and b"bad shape" in err(), k
    assert pool(pad=2) == EINVAL and pool(pad=-1) == EINVAL
    assert pool(C=12, cs=12) == EINVAL and b"multiple of 8" in err()
    assert pool(cs=23) == EINVAL and pool(cs=32, co=12) == EINVAL and pool(cs=34, co=2) == EINVAL and b"channel window" in err()
    assert pool(cs=26) == EINVAL and pool(co=-4, cs=32) == EINVAL
    assert pool(IH=2, pad=0) == EINVAL and pool(IW=1, pad=0) == EINVAL and b"does not fit" in err()
    assert pool(N=2 ** 20, IH=2 ** 10, IW=2 ** 10) == EINVAL and b"too many pixels" in err()

    def gap(x=p, out=p, N=2, HW=64, C=2048):
        return lib.dxmi_global_avgpool_f32(x, out, N, HW, C, null)
    assert gap(x=null) == EINVAL and gap(out=null) == EINVAL and b"null pointer" in err()
    for k in ("N", "HW", "C"):
        assert gap(**{k: 0}) == EINVAL and gap(**{k: -1}) == EINVAL and b"bad shape" in err(), k
    assert gap(C=20) == EINVAL and b"multiple of 8" in err()
    assert gap(N=2 ** 20, HW=2 ** 20) == EINVAL and b"too many pixels" in err()

    def resize(x=p, out=p, N=2, IH=32, IW=32, OH=299, OW=299):
        return lib.dxmi_resize_bilinear_nhwc_f32(x, out, N, IH, IW, OH, OW, 1, null)
    assert resize(x=null) == EINVAL and resize(out=null) == EINVAL and b"null pointer" in err()
    for k in ("N", "IH", "IW", "OH", "OW"):
        assert resize(**{k: 0}) == EINVAL and resize(**{k: -1}) == EINVAL and b"bad shape" in err(), k
    assert resize(N=2 ** 20, OH=2 ** 10, OW=2 ** 10) == EINVAL and b"too many pixels" in err()

    def conv_layout(i=p, out=p, N=2, C=24, HW=35):
        return lib.dxmi_nhwc_f32_to_nchw_f32(i, out, N, C, HW, null)
    assert conv_layout(i=null) == EINVAL and conv_layout(out=null) == EINVAL and b"null pointer" in err()
    for k in ("N", "C", "HW"):
        assert conv_layout(**{k: 0}) == EINVAL and conv_layout(**{k: -1}) == EINVAL and b"bad shape" in err(), k
    assert conv_layout(N=2 ** 20, HW=2 ** 20) == EINVAL and b"too many pixels" in err()


def test_precision_argument():
    from pytorch_fid.inception import InceptionV3
    assert InceptionV3(output_blocks=[0]).precision == "bf16"
    m = InceptionV3(output_blocks=[0], precision="fp32")
    assert m.precision == "fp32" and m._packed is None
    for bad in ("fp16", "float32", None, 32):
        with pytest.raises(ValueError, match="precision"):
            InceptionV3(output_blocks=[0], precision=bad)
    with pytest.raises(ValueError):
        m.precision = "fp16"
    assert m.precision == "fp32"


def test_fp32_classes_need_the_weight_file(monkeypatch, tmp_path):
    from dxmi_hip import DxmiError
    from pytorch_fid.inception import EvalInceptionV3, EvalInceptionV3FP32, FIDInceptionV3, FIDInceptionV3FP32
    assert issubclass(FIDInceptionV3FP32, FIDInceptionV3) and issubclass(EvalInceptionV3FP32, EvalInceptionV3)
    assert (FIDInceptionV3.PRECISION, EvalInceptionV3.PRECISION, FIDInceptionV3FP32.PRECISION, EvalInceptionV3FP32.PRECISION) == \
        ("bf16", "bf16", "fp32", "fp32")
    monkeypatch.delenv("DXMI_FID_WEIGHTS", raising=False)
    for cls in (FIDInceptionV3FP32, EvalInceptionV3FP32):
        with pytest.raises(DxmiError, match="DXMI_FID_WEIGHTS"):
            cls()
    monkeypatch.setenv("DXMI_FID_WEIGHTS", str(tmp_path / "absent.pth"))
    for cls in (FIDInceptionV3FP32, EvalInceptionV3FP32):
        with pytest.raises(DxmiError, match="DXMI_FID_WEIGHTS"):
            cls()
    with pytest.raises(DxmiError):
        EvalInceptionV3FP32(weights=str(tmp_path / "absent.pth"))


def test_cpu_tensors_raise():
    from dxmi_hip import DxmiError, inception_f32_ops as o
    from pytorch_fid.inception import InceptionV3
    with pytest.raises(DxmiError):
        InceptionV3(output_blocks=[0], precision="fp32")(torch.rand(1, 3, 32, 32))
    x = torch.zeros(1, 5, 5, 8)
    with pytest.raises(DxmiError):
        o.gconv_pack(torch.zeros(32, 8, 3, 3))
    with pytest.raises(DxmiError):
        o.pool3x3(x, 1, 1)
    with pytest.raises(DxmiError):
        o.global_avgpool(x)
    with pytest.raises(DxmiError):
        o.nhwc_to_nchw(x)
    with pytest.raises(DxmiError):
        o.resize_bilinear_nhwc(torch.zeros(1, 3, 8, 8), 16, 16)
    with pytest.raises(DxmiError):
        o.gconv(x, o.PackedGConvF32(torch.zeros(32 * 9 * 8), torch.ones(32), torch.zeros(32), 32, 8, 8, 3, 3))


def test_ops_module_surface():
    """The public names the program and the recorder rely on; nothing of it is added to dxmi_hip.ops."""
    from dxmi_hip import inception_f32_ops as o, ops
    assert sorted(iwf.public_functions(o)) == sorted(iwf.LAUNCH)
    assert o.GRANULE == 8
    assert not hasattr(ops, "PackedGConvF32") and not hasattr(ops, "resize_bilinear_nhwc")


def test_conv_bound_separates_fp32_from_bf16():
    """CPU-only control: for one conv row, the fp32 rounding of the fp64 result and a torch-fp32 evaluation sit inside the fp32
    conv bound; the bf16 rounding fails it on more than half of the elements."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    N, IH, IW, Cin, Cout, k, s, p = 2, 13, 13, 24, 64, (3, 5), (1, 1), (0, 2)
    w = torch.randn(Cout, Cin, *k, generator=g) * (2.0 / (Cin * k[0] * k[1])) ** 0.5
    x = torch.randn(N, IH, IW, Cin, generator=g)
    scale, shift = 0.5 + torch.rand(Cout, generator=g), 0.4 * torch.rand(Cout, generator=g) - 0.2
    post, bound = iwf.gconv_f32_ref(x, w, scale, shift, s, p, relu=False)            # no ReLU: a zero would be exact in bf16 too
    got32 = (F.conv2d(x.permute(0, 3, 1, 2), w, None, s, p) * scale[:, None, None] + shift[:, None, None]).permute(0, 2, 3, 1)
    r_round = ((post.float().double() - post).abs() / (bound + 1e-300)).max()
    r_torch = ((got32.double() - post).abs() / (bound + 1e-300)).max()
    bad16 = ((post.to(torch.bfloat16).double() - post).abs() > bound).float().mean()
    print(f"conv bound: fp32 rounding {float(r_round):.4f}, torch fp32 {float(r_torch):.4f} of it; bf16 rounding outside on {float(bad16):.3f} of the elements")
    assert float(r_round) <= 1.0 and float(r_torch) <= 1.0
    assert float(bad16) > 0.5


def test_resize_bound_separates_fp32_from_bf16():
    """CPU-only control: the fp32 emulation of the kernel's expressions sits inside the fp32 resize bound on every resize shape of
    the GPU module, bitwise on a same-size resize; its bf16 rounding fails the bound on more than half of the elements for every
    input up to 299 pixels.  (The bound's coordinate term 2 d D, d = 4 u32 (max(IH, IW) + 1), grows with the input: from a 512-pixel
    input it is 16 * 513 u32 = 2^-11, a quarter of a bf16 ulp of a value in [0.5, 1), and the bf16 rounding then exceeds it on about
    a third of the elements only: that row's fraction is printed, and must still be far from none.)"""
    g = torch.Generator().manual_seed(0)
    rows = [(2, 32, 32, 299, 299, True), (2, 64, 64, 299, 299, True), (1, 256, 256, 299, 299, True), (2, 299, 299, 299, 299, True),
            (1, 512, 512, 299, 299, True), (2, 139, 203, 299, 299, True), (2, 48, 80, 151, 77, True), (2, 32, 32, 299, 299, False),
            (2, 139, 203, 139, 203, False)]
    for (N, IH, IW, OH, OW, nm) in rows:
        x = torch.rand(N, 3, IH, IW, generator=g)
        ref, bound = iwf.resize_f32_bound(x, OH, OW, nm)
        em = fb.resize_emulate_f32(x, OH, OW, nm)
        assert float(((em.double() - ref).abs() / bound).max()) <= 1.0, (IH, IW, OH, OW)
        if (IH, IW) == (OH, OW):
            assert torch.equal(em, ((2 * x - 1) if nm else x).permute(0, 2, 3, 1))
        bad = ((em.to(torch.bfloat16).double() - ref).abs() > bound).float().mean()
        print(f"resize {IH}x{IW} -> {OH}x{OW}: bf16 rounding outside the fp32 bound on {float(bad):.3f} of the elements")
        assert float(bad) > (0.5 if max(IH, IW) <= 299 else 0.25), (IH, IW, OH, OW, float(bad))
