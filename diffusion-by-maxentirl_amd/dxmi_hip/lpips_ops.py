"""Wrappers of the LPIPS launches (csrc/lpips.hip and the two lpips entries of csrc/cm_train.hip).  Every operand is checked
here, before anything is launched: a malformed call raises DxmiError.  The convolutions themselves are ops.gconv."""
import torch

from . import _lib
from ._lib import check, load
from .ops import _dsm_schedule, _need_cuda, _ptr, _stream

TAP_MAX_C = 512


def _err(msg):
    raise _lib.DxmiError(msg)


def _bf16_map(what, t, name):
    if t is None:
        _err(f"{what}: {name} is missing")
    if t.dtype != torch.bfloat16 or t.dim() != 4 or not t.is_contiguous() or t.numel() == 0 or t.data_ptr() % 16:
        _err(f"{what}: {name} must be a non-empty contiguous 16-byte aligned bf16 [N, H, W, C] tensor, got {t.dtype} {tuple(t.shape)}")


def _f32_images(what, x, name):
    if x is None:
        _err(f"{what}: {name} is missing")
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous() or x.numel() == 0:
        _err(f"{what}: {name} must be a non-empty contiguous fp32 [N, 3, H, W] tensor, got {x.dtype} {tuple(x.shape)}")


def _size(what, size):
    OH, OW = (size, size) if isinstance(size, int) else tuple(size)
    if OH < 1 or OW < 1 or OH > 16384 or OW > 16384:
        _err(f"{what}: output size {OH}x{OW} outside [1, 16384]")
    return int(OH), int(OW)


def front_fwd(x, size=None):
    """x fp32 [N, 3, H, W] in [0, 1] -> bilinear resize to `size` (None: none) -> (v - mean) / std -> bf16 [N, OH, OW, 16]."""
    _f32_images("dxmi_lpips_front_fwd", x, "x")
    _need_cuda(x)
    N, _, H, W = x.shape
    OH, OW = _size("dxmi_lpips_front_fwd", (H, W) if size is None else size)
    out = torch.empty((N, OH, OW, 16), dtype=torch.bfloat16, device=x.device)
    check(load().dxmi_lpips_front_fwd(_ptr(x), _ptr(out), N, H, W, OH, OW, _stream()), "dxmi_lpips_front_fwd")
    return out


def front_bwd(g, H, W):
    """g bf16 [N, OH, OW, 16] (channels 0..2) -> d x fp32 [N, 3, H, W]: the transpose of front_fwd."""
    _bf16_map("dxmi_lpips_front_bwd", g, "g")
    _need_cuda(g)
    N, OH, OW, C = g.shape
    if C != 16:
        _err(f"dxmi_lpips_front_bwd: g has {C} channels, 16 are needed")
    H, W = _size("dxmi_lpips_front_bwd", (H, W))
    dx = torch.empty((N, 3, H, W), dtype=torch.float32, device=g.device)
    check(load().dxmi_lpips_front_bwd(_ptr(g), _ptr(dx), N, H, W, OH, OW, _stream()), "dxmi_lpips_front_bwd")
    return dx


def _pool_shape(what, N, IH, IW, C):
    if IH < 2 or IW < 2 or C % 8:
        _err(f"{what}: the map {IH}x{IW} must be at least 2x2 and C ({C}) a multiple of 8")


def avgpool2x2(x):
    """AvgPool2d(2, 2, 0) on NHWC bf16: [N, IH, IW, C] -> [N, IH // 2, IW // 2, C]."""
    _bf16_map("dxmi_avgpool2x2_fwd", x, "x")
    _need_cuda(x)
    N, IH, IW, C = x.shape
    _pool_shape("dxmi_avgpool2x2_fwd", N, IH, IW, C)
    out = torch.empty((N, IH // 2, IW // 2, C), dtype=torch.bfloat16, device=x.device)
    check(load().dxmi_avgpool2x2_fwd(_ptr(x), _ptr(out), N, IH, IW, C, _stream()), "dxmi_avgpool2x2_fwd")
    return out


def avgpool2x2_bwd(g, IH, IW):
    """g bf16 [N, IH // 2, IW // 2, C] -> the gradient of the [N, IH, IW, C] input (zero in a dropped last row / column)."""
    _bf16_map("dxmi_avgpool2x2_bwd", g, "g")
    _need_cuda(g)
    N, OH, OW, C = g.shape
    _pool_shape("dxmi_avgpool2x2_bwd", N, IH, IW, C)
    if (OH, OW) != (IH // 2, IW // 2):
        _err(f"dxmi_avgpool2x2_bwd: g is {OH}x{OW}, the pool of a {IH}x{IW} map is {IH // 2}x{IW // 2}")
    out = torch.empty((N, IH, IW, C), dtype=torch.bfloat16, device=g.device)
    check(load().dxmi_avgpool2x2_bwd(_ptr(g), _ptr(out), N, IH, IW, C, _stream()), "dxmi_avgpool2x2_bwd")
    return out


def _tap_operands(what, fx, fy, w, per_sample=()):
    _bf16_map(what, fx, "fx")
    _bf16_map(what, fy, "fy")
    if fx.shape != fy.shape:
        _err(f"{what}: fx {tuple(fx.shape)} and fy {tuple(fy.shape)} differ")
    N, H, Wd, C = fx.shape
    if C % 16 or C > TAP_MAX_C:
        _err(f"{what}: C ({C}) must be a multiple of 16, at most {TAP_MAX_C}")
    if N > 65535:
        _err(f"{what}: at most 65535 samples, got {N}")
    if w is None or w.dtype != torch.float32 or not w.is_contiguous() or w.numel() != C:
        _err(f"{what}: w must be {C} contiguous fp32 values")
    for t in per_sample:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != N):
            _err(f"{what}: per-sample operand must be {N} contiguous fp32 values")
    _need_cuda(fx, fy, w, *per_sample)
    if any(t is not None and t.device != fx.device for t in (fy, w) + tuple(per_sample)):
        _err(f"{what}: operands on different devices")
    return N, H * Wd, C


def tap_fwd(fx, fy, w, out=None, scale=None):
    """Per-sample LPIPS distance of one tap: fx, fy bf16 [N, h, w, C], w fp32 [C] -> fp32 [N]; added to `out` if given; the sum is
    multiplied by scale[N] if given."""
    N, HW, C = _tap_operands("dxmi_lpips_tap_fwd", fx, fy, w, (out, scale))
    lib = load()
    partials = torch.empty(N * int(lib.dxmi_lpips_tap_partials(HW, C)), dtype=torch.float32, device=fx.device)
    acc = out is not None
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=fx.device)
    check(lib.dxmi_lpips_tap_fwd(_ptr(fx), _ptr(fy), _ptr(w), _ptr(scale), _ptr(partials), _ptr(out), N, HW, C, int(acc), _stream()),
          "dxmi_lpips_tap_fwd")
    return out


def tap_bwd(g, fx, fy, w):
    """d fx (bf16) of tap_fwd's value for the upstream g fp32 [N] (None: ones), through the per-pixel normalisation."""
    N, HW, C = _tap_operands("dxmi_lpips_tap_bwd", fx, fy, w, (g,))
    d = torch.empty_like(fx)
    check(load().dxmi_lpips_tap_bwd(_ptr(g), _ptr(fx), _ptr(fy), _ptr(w), _ptr(d), N, HW, C, _stream()), "dxmi_lpips_tap_bwd")
    return d


def relu_mask_acc(ga, gb, act):
    """(ga + gb) * (act > 0) in bf16; gb may be None."""
    what = "dxmi_relu_mask_acc"
    _bf16_map(what, ga, "g_a")
    _bf16_map(what, act, "act")
    if gb is not None:
        _bf16_map(what, gb, "g_b")
    for t in (gb, act):
        if t is not None and t.shape != ga.shape:
            _err(f"{what}: operand of shape {tuple(t.shape)} where {tuple(ga.shape)} is needed")
    if ga.numel() % 8:
        _err(f"{what}: numel ({ga.numel()}) must be a multiple of 8")
    _need_cuda(ga, gb, act)
    out = torch.empty_like(ga)
    check(load().dxmi_relu_mask_acc(_ptr(ga), _ptr(gb), _ptr(act), _ptr(out), ga.numel(), _stream()), what)
    return out


def _cd_lpips_operands(what, first, indices, t_table, same, per_sample=()):
    from .ops import _batch_operands
    if first is None or first.dim() != 4:
        _err(f"{what}: [N, C, H, W] tensors are needed")
    N, CHW, S = _batch_operands(what, first, same, per_sample, indices=indices, t_table=t_table)
    if CHW % 4:
        _err(f"{what}: C H W ({CHW}) must be a multiple of 4")
    return N, CHW, S


def cd_lpips_images(f_online, f_target, x_t, x_t2, indices, t_table, weight_schedule, sigma_data=0.5, sigma_min=0.002,
                    distillation=False):
    """-> (x01 fp32 [2 N, C, H, W]: (distiller + 1) / 2 then (target + 1) / 2, weights fp32 [N]) (dxmi_cd_lpips_images)."""
    sched = _dsm_schedule(weight_schedule)
    N, CHW, S = _cd_lpips_operands("dxmi_cd_lpips_images", f_online, indices, t_table, (f_target, x_t, x_t2))
    x01 = torch.empty((2 * N,) + tuple(f_online.shape[1:]), dtype=torch.float32, device=f_online.device)
    w = torch.empty(N, dtype=torch.float32, device=f_online.device)
    check(load().dxmi_cd_lpips_images(_ptr(f_online), _ptr(f_target), _ptr(x_t), _ptr(x_t2), _ptr(indices), _ptr(t_table), S, _ptr(x01),
                                      _ptr(w), N, CHW, float(sigma_data), float(sigma_min), int(bool(distillation)), sched, _stream()),
          "dxmi_cd_lpips_images")
    return x01, w


def cd_lpips_bwd(g_loss, d_x01, indices, t_table, weight_schedule, sigma_data=0.5, sigma_min=0.002, distillation=False):
    """-> d(f_online) = ((g_loss w) d_x01 / 2) c_out(t) (dxmi_cd_lpips_bwd)."""
    sched = _dsm_schedule(weight_schedule)
    if g_loss is None:
        _err("dxmi_cd_lpips_bwd: no upstream gradient")
    N, CHW, S = _cd_lpips_operands("dxmi_cd_lpips_bwd", d_x01, indices, t_table, (), per_sample=(g_loss,))
    d = torch.empty_like(d_x01)
    check(load().dxmi_cd_lpips_bwd(_ptr(g_loss), _ptr(d_x01), _ptr(indices), _ptr(t_table), S, _ptr(d), N, CHW, float(sigma_data),
                                   float(sigma_min), int(bool(distillation)), sched, _stream()), "dxmi_cd_lpips_bwd")
    return d


def pd_lpips_images(f_online, x_t, target_x, indices, t_table, weight_schedule, sigma_data=0.5, sigma_min=0.002, distillation=False):
    """-> (x01 fp32 [2 N, C, H, W]: (denoised + 1) / 2 then (target_x + 1) / 2, weights fp32 [N]) of progdist_losses
    (dxmi_pd_lpips_images).  t_table: the 2 S + 1 levels of ops.pd_solver."""
    from .ops import _pd_operands
    sched = _dsm_schedule(weight_schedule)
    if f_online is None or f_online.dim() != 4:
        _err("dxmi_pd_lpips_images: [N, C, H, W] tensors are needed")
    N, CHW, S = _pd_operands("dxmi_pd_lpips_images", f_online, indices, t_table, same=(x_t, target_x))
    x01 = torch.empty((2 * N,) + tuple(f_online.shape[1:]), dtype=torch.float32, device=f_online.device)
    w = torch.empty(N, dtype=torch.float32, device=f_online.device)
    check(load().dxmi_pd_lpips_images(_ptr(f_online), _ptr(x_t), _ptr(target_x), _ptr(indices), _ptr(t_table), S, _ptr(x01), _ptr(w), N,
                                      CHW, float(sigma_data), float(sigma_min), int(bool(distillation)), sched, _stream()),
          "dxmi_pd_lpips_images")
    return x01, w
