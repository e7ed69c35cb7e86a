"""Wrappers of the fp32 InceptionV3 launches (csrc/inception_f32.hip): the op set `pytorch_fid.inception.InceptionV3(precision="fp32")`
runs on.  Activations are NHWC fp32 with a channel count that is a multiple of GRANULE; a malformed call raises DxmiError before
anything is launched (the C entry points validate again).  The bf16 op set of the same program is in dxmi_hip.ops."""
import torch

from . import _lib, ops
from ._lib import check, load
from .ops import _need_cuda, _ptr, _stream

GRANULE = 8          # channel granule of the fp32 maps (csrc/inception_f32.hip: two 16-byte loads per k step)


def _err(msg):
    raise _lib.DxmiError(msg)


def _f32_map(what, t, name):
    if t is None:
        _err(f"{what}: {name} is missing")
    if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous() or t.numel() == 0 or t.data_ptr() % 16:
        _err(f"{what}: {name} must be a non-empty contiguous 16-byte aligned fp32 [N, H, W, C] tensor, got {t.dtype} {tuple(t.shape)}")


def _out_map(what, out, N, OH, OW, C, coff, align):
    _f32_map(what, out, "out")
    if tuple(out.shape[:3]) != (N, OH, OW):
        _err(f"{what}: out is {tuple(out.shape)}, the launch writes [{N}, {OH}, {OW}, .]")
    if coff < 0 or coff + C > out.shape[3] or coff % align or out.shape[3] % align:
        _err(f"{what}: channel window [{coff}, {coff + C}) does not fit the output's {out.shape[3]} channels (alignment {align})")


class PackedGConvF32:
    """One BasicConv2d for gconv: w fp32 [ceil32(Cout)][KH * KW][ceil8(Cin)], bit for bit the checkpoint's conv.weight re-laid-out
    (padding zero); scale / shift fp32 [ceil32(Cout)]: the BatchNorm the epilogue applies (dxmi_gconv_f32_pack)."""

    __slots__ = ("w", "scale", "shift", "Cout", "Cin", "CinP", "KH", "KW")

    def __init__(self, w, scale, shift, Cout, Cin, CinP, KH, KW):
        self.w, self.scale, self.shift, self.Cout, self.Cin, self.CinP, self.KH, self.KW = w, scale, shift, Cout, Cin, CinP, KH, KW


def gconv_pack(weight, bn=None, eps=1e-3, bias=None):
    """weight fp32 [Cout, Cin, KH, KW]; bn = (gamma, beta, running_mean, running_var) or None; bias fp32 [Cout] of a convolution
    without BatchNorm (None: zero)."""
    what = "dxmi_gconv_f32_pack"
    if weight is None or weight.dim() != 4 or weight.numel() == 0:
        _err(f"{what}: weight must be a non-empty [Cout, Cin, KH, KW] tensor")
    _need_cuda(weight)
    w = weight.detach().float().contiguous()
    Cout, Cin, KH, KW = w.shape
    if bn is not None and bias is not None:
        _err(f"{what}: a conv bias excludes BatchNorm")
    vec = lambda t, name: t.detach().float().reshape(-1).contiguous() if t.numel() == Cout and t.is_cuda else _err(
        f"{what}: {name} must be a device tensor of {Cout} elements")
    bnp = [vec(t, "a BatchNorm tensor") for t in bn] if bn is not None else [None] * 4
    cb = vec(bias, "bias") if bias is not None else None
    lib = load()
    CoutP, CinP = (Cout + 31) // 32 * 32, (Cin + GRANULE - 1) // GRANULE * GRANULE
    wp = torch.empty(int(lib.dxmi_gconv_f32_packed_elems(Cout, Cin, KH, KW)), dtype=torch.float32, device=w.device)
    scale = torch.empty(CoutP, dtype=torch.float32, device=w.device)
    shift = torch.empty(CoutP, dtype=torch.float32, device=w.device)
    check(lib.dxmi_gconv_f32_pack(_ptr(w), _ptr(bnp[0]), _ptr(bnp[1]), _ptr(bnp[2]), _ptr(bnp[3]), float(eps), _ptr(cb), _ptr(wp), _ptr(scale),
                                  _ptr(shift), Cout, Cin, KH, KW, _stream()), what)
    return PackedGConvF32(wp, scale, shift, Cout, Cin, CinP, KH, KW)


def gconv(x, pk, stride=(1, 1), pad=(0, 0), relu=True, out=None, coff=0):
    """x NHWC fp32 [N, IH, IW, pk.CinP] -> NHWC fp32 [N, OH, OW, Cout] (or the channel window [coff, coff + Cout) of `out`)."""
    what = "dxmi_gconv_f32_fwd"
    _f32_map(what, x, "x")
    _need_cuda(x, out)
    N, IH, IW, C = x.shape
    if C != pk.CinP:
        _err(f"{what}: input has {C} channels, the packed weight wants {pk.CinP}")
    (SH, SW), (PH, PW) = stride, pad
    if SH < 1 or SW < 1 or PH < 0 or PW < 0 or IH + 2 * PH < pk.KH or IW + 2 * PW < pk.KW:
        _err(f"{what}: the {pk.KH}x{pk.KW} kernel (stride {SH}x{SW}, padding {PH}x{PW}) does not fit the {IH}x{IW} map")
    OH, OW = (IH + 2 * PH - pk.KH) // SH + 1, (IW + 2 * PW - pk.KW) // SW + 1
    if out is None:
        out = torch.empty((N, OH, OW, pk.Cout), dtype=torch.float32, device=x.device)
    _out_map(what, out, N, OH, OW, pk.Cout, coff, 1)
    fl = 2.0 * N * OH * OW * pk.Cout * pk.Cin * pk.KH * pk.KW
    ops._prof("inception", f"gconv_f32_{pk.KH}x{pk.KW}", fl, 4.0 * (x.numel() + N * OH * OW * pk.Cout + pk.w.numel()), lambda: check(
        load().dxmi_gconv_f32_fwd(_ptr(x), _ptr(pk.w), _ptr(pk.scale), _ptr(pk.shift), _ptr(out), N, IH, IW, C, pk.Cout, pk.KH, pk.KW, SH, SW,
                                  PH, PW, out.shape[3], coff, int(relu), _stream()), what))
    return out


def pool3x3(x, stride, pad, avg_exclude_pad=False, out=None, coff=0):
    """3x3 max pool, or the average over the in-bounds pixels of the window (count_include_pad=False), NHWC fp32."""
    what = "dxmi_pool3x3_f32"
    _f32_map(what, x, "x")
    _need_cuda(x, out)
    N, IH, IW, C = x.shape
    if C % GRANULE or stride < 1 or pad not in (0, 1) or IH + 2 * pad < 3 or IW + 2 * pad < 3:
        _err(f"{what}: C ({C}) must be a multiple of {GRANULE}, pad 0 or 1 and the 3x3 window must fit the padded {IH}x{IW} map")
    OH, OW = (IH + 2 * pad - 3) // stride + 1, (IW + 2 * pad - 3) // stride + 1
    if out is None:
        out = torch.empty((N, OH, OW, C), dtype=torch.float32, device=x.device)
    _out_map(what, out, N, OH, OW, C, coff, 4)
    ops._prof("inception", "pool3x3_f32", 9.0 * N * OH * OW * C, 4.0 * (x.numel() + N * OH * OW * C), lambda: check(
        load().dxmi_pool3x3_f32(_ptr(x), _ptr(out), N, IH, IW, C, stride, pad, int(avg_exclude_pad), out.shape[3], coff, _stream()), what))
    return out


def global_avgpool(x):
    """NHWC fp32 [N, H, W, C] -> fp32 [N, C]: the pixels summed in index order, divided by H * W."""
    what = "dxmi_global_avgpool_f32"
    _f32_map(what, x, "x")
    _need_cuda(x)
    N, H, W, C = x.shape
    if C % GRANULE:
        _err(f"{what}: C ({C}) must be a multiple of {GRANULE}")
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    ops._prof("inception", "global_avgpool_f32", float(x.numel()), 4.0 * (x.numel() + N * C), lambda: check(
        load().dxmi_global_avgpool_f32(_ptr(x), _ptr(out), N, H * W, C, _stream()), what))
    return out


def resize_bilinear_nhwc(x, OH, OW, normalize=True):
    """NCHW fp32 [N, 3, H, W] -> NHWC fp32 [N, OH, OW, GRANULE] (bilinear, align_corners=False; 2 x - 1 when normalize; channels
    3.. zero)."""
    what = "dxmi_resize_bilinear_nhwc_f32"
    if x is None or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous() or x.numel() == 0:
        _err(f"{what}: x must be a non-empty contiguous fp32 [N, 3, H, W] tensor")
    _need_cuda(x)
    N, _, H, W = x.shape
    if OH < 1 or OW < 1:
        _err(f"{what}: output size {OH}x{OW}")
    out = torch.empty((N, OH, OW, GRANULE), dtype=torch.float32, device=x.device)
    ops._prof("inception", "resize_f32", 30.0 * N * OH * OW, 4.0 * (x.numel() + out.numel()), lambda: check(
        load().dxmi_resize_bilinear_nhwc_f32(_ptr(x), _ptr(out), N, H, W, int(OH), int(OW), int(normalize), _stream()), what))
    return out


def nhwc_to_nchw(x, out=None):
    """NHWC fp32 -> NCHW fp32, bit for bit."""
    what = "dxmi_nhwc_f32_to_nchw_f32"
    _f32_map(what, x, "x")
    _need_cuda(x, out)
    N, H, W, C = x.shape
    if out is None:
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (N, C, H, W) or not out.is_contiguous():
        _err(f"{what}: out must be a contiguous fp32 [{N}, {C}, {H}, {W}] tensor")
    ops._prof("inception", "nhwc_to_nchw_f32", 0.0, 8.0 * x.numel(), lambda: check(
        load().dxmi_nhwc_f32_to_nchw_f32(_ptr(x), _ptr(out), N, C, H * W, _stream()), what))
    return out
