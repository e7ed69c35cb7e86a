"""Error bounds for the forward kernels, checked element by element against an fp64 reference of the same operation.

The references use stock torch only, in float64 on the device (F.unfold + einsum for convolutions, F.group_norm-style group
statistics, softmax attention, a plain matmul for `linear`); none of this project's kernels takes part.  u32 = 2^-24 and
u16 = 2^-8 are the unit roundoffs of fp32 and bf16; `Checker` (backward_bounds) keeps the worst |err| / bound per op.

Conv forward (bf16 operands, fp32 MFMA accumulation, fused adds, activation, one bf16 store).  Every product of two bf16
values is exact in fp32, so the accumulation of the K = Cin * k * k products plus the fused adds (bias, addvec, residual: up
to three more terms) is a recursive fp32 sum of c = K + 3 terms, |fl(s) - s| <= c u32 sum|x_i| (Higham 4.2), whatever the
order.  With A = sum |w||x| + |bias| + |addvec| + |residual| (fp64, same operands) the pre-activation error is c u32 A.  The
activation act is Lipschitz with constant L (1 for none / ReLU / LeakyReLU, 1.1 for SiLU: max |silu'| = 1.0998) and is itself
evaluated in fp32 to a few ulps; the store rounds once more to bf16 (round to nearest even: relative error <= u16; a
truncating store errs by up to 2 u16, and by more than u16 for about half of all values).  So

    |got - act(ref64)| <= L c u32 A (1 + u16) + (u16 + 4 u32) |act(ref64)|

An fp32-output conv (conv_out, NCHW fp32) drops the bf16 term.  conv_call_ref forms reference and bound from the operands of one
ops.conv2d call (activation mask, zero-stuffed upsampling and the stem's fp32 image included); the program-shape suite
(test_hip_forward_shapes.py) and the edge-case suites (conv_checked / linear_checked, worst ratio per kernel family in EDGE) share it.

Block statistics (sum, sum of squares per channel pair).  The kernels sum the STORED bf16 outputs; a bf16 square is exact
in fp32.  One partial adds 2 * pixels-per-partial terms; a fold pass adds `group` partials; summing the remaining partials
(done here in fp64) is exact enough.  So per image and channel pair, with the sums taken over the stored tensor:

    |sum_p st[p] - S64| <= (2 * HW / P0 + 32 * folds + 2) u32 S64abs

GroupNorm forward.  The kernels compute the group statistics in one fp32 pass: m = s / n, var = q / n - m^2 with s, q fp32
sums of depth d.  The streaming apply adds the P partials of each channel pair, then the cpg / 2 pairs of a group: nested
sums whose depths add, d = max(P0, P1) + cpg / 2 (+ 2 for the rounding of given partials); the resident and generic kernels
are charged the group size, valid for any order of their partial sums.  With E|x|, E[x^2] the group means of |x|, x^2:
    dm <= d u32 E|x|,   dq <= d u32 E[x^2],   dvar <= dq + 2 |m| dm + 2 u32 E[x^2] <= (3 d + 2) u32 E[x^2]
(|m| E|x| <= E[x^2]).  rstd = (var + eps)^-1/2 then has relative error (1.5 d + 1) u32 kappa + 4 u32 with the conditioning
term kappa = E[x^2] / (var + eps) = (m^2 + var) / (var + eps), carried explicitly, eps included.  xhat = (x - m) rstd:
    dxhat <= |xhat| drstd + rstd dm + 4 u32 (|x| + |m|) rstd
and y = act(film(gamma xhat + beta)) propagates it with L |gamma| |1 + scale|, plus 4 u32 of the affine terms; one bf16 store:
    |got - y64| <= L |gamma| |1 + scale| dxhat (1 + u16) + 4 u32 (|gamma xhat| + |beta|) |1 + scale| + (u16 + 4 u32) |y64|
A fused GroupNorm in a conv epilogue normalises the conv's bf16-ROUNDED outputs: when the raw tensor is kept, the reference
normalises exactly that stored tensor; when it is not, the propagated term is carried instead (gn_fused_bound): the input
error dh = c u32 A + u16 |h| of every element goes through the linearised GroupNorm, rstd (dh_i + mean_g dh +
|xhat_i| mean_g |xhat| dh).

linear (linear_small_kernel and the tiled path).  pre_act(x) is evaluated in fp32 and rounded to bf16 (the MFMA operand);
the reference rounds at the same point (bf16 of the fp64 pre-activation).  Where the fp64 pre-activation lies within 8 u32
of a bf16 rounding midpoint the kernel's fp32 value may round the other way: such operands carry u16 |pre| |w| in the bound.
Depth K plus the bias add; post_act as for the conv; fp32 output:  |got - ref| <= L (K + 2) u32 A + 4 u32 |ref| + tie term.

Attention.  P is rounded to bf16 before the P V product (an MFMA operand), so the output is judged by rel-L2 per (image, head,
128-row block) within 8 u16, as the backward is (and element by element: next paragraph).  The row log-sum-exp the kernels keep is in the LOG2 domain:
lse2 = log2 sum_j 2^(s_ij log2 e), s = scale q.k.  A score is an fp32 sum of D exact products (error D u32 scale sum|q||k|),
2^x is evaluated to ~2 ulp and summed over T keys, so element-wise
    |got - lse2| <= log2(e) (D + 2) u32 scale max_j sum_d |q_id k_jd| + (T + 8) u32 log2(e) + 4 u32 |lse2|

Attention, element by element (attn_elem_bound; ops.attention alone: a fused projection or GroupNorm-on-load sits outside it).
The per-block rel-L2 averages over 128 rows x D columns: one query row that is 10 % wrong moves it by 0.1 / sqrt(128) = 0.9 %,
under 8 u16 = 3.1 %, and it cannot take a ragged T at all.  What the kernels compute (attention_kernel<D>, attention64_kernel,
attention256_kernel<false>), with P = softmax(s) in fp64, o = P v and a_id = sum_j P_ij |v_jd|:
  * a score is an fp32 sum of D exact bf16 products, scaled once by scale * log2(e) (one rounded constant, one product):
    |s32_ij - s_ij| <= delta_i = (D + 2) u32 smag_i in natural-log units, smag_i = scale max_j sum_d |q_id k_jd| (attention_ref's).
  * p_ij = exp2(t_ij - m_i) in fp32, m_i a running maximum.  The quotient p_ij / sum_j p_ij does not depend on m_i, so only the
    score errors matter: the numerator moves by a factor within e^(+-delta_i) and so does the denominator, 2 delta_i on the
    quotient (first order).  The subtraction and exp2 round to a few ulps of fp32: part of the (T + 8) u32 below.
  * l_i SUMS THE UNROUNDED p (fp32), the P V operand is p rounded to bf16, round to nearest: each term of the numerator carries a
    relative error <= 2^-9 <= u16 that the denominator does not share, u16 a_id in all.
  * O accumulates in fp32 over the T keys and l over the same T terms, with one rescale of both per key block when the maximum
    moved (skipped when no lane's did): recursive sums of depth <= T, the rescales and exp2's ulps in the + 8: (T + 8) u32 a_id.
  * O / l is one reciprocal and one product in fp32, then one bf16 store: (u16 + 4 u32) |o_id|, and (1 + u16) on what came before.
    |got_id - o_id| <= (u16 + 2 delta_i + (T + 8) u32) a_id (1 + u16) + (u16 + 4 u32) |o_id|
The u16 terms carry the bound (T u32 is 1e-5 at T = 200); a wrong key set does not fit: with every true score near -9
(below_zero of attn_inputs) one zero-filled key left unmasked holds nearly all of a row's weight and misses the bound ~100 times
over, where under Gaussian q, k it moves the denominator T e^0.5 by 0.3 %, below u16 (test_forward_bounds.py measures both).

InceptionV3 extractor (csrc/inception_ops.hip).  Bounds of the extractor's launches (tests/test_hip_inception_launches.py).

gconv: the conv bound above with L = 1 (none / ReLU): K = CinP * KH * KW products (the zero-padded channels included: they add
exact zeros), + bias; the weight operand of the reference is the UNPACKED PACKED BUFFER, bit for bit the kernel's operand
(gconv_unpack, written from the layout the kernel's header documents: [CoutP][KH * KW][CinP], CoutP = ceil32(Cout),
CinP = ceil16(Cin)); gconv_pack_ref ties that buffer to the checkpoint's tensors.

gconv_pack: scale = gamma / sqrt(var + eps) is three fp32 operations (add, correctly rounded sqrt and divide), the product
w * scale a fourth, the fp32 value of eps a relative 2^-24 of a small term: <= 8 u32 in all, then one bf16 rounding:
    |wp - fold64| <= (u16 + 8 u32) |fold64|,   |bias - (beta - mean scale)| <= 8 u32 (|beta| + |mean scale|).

Average pool over the cnt in-bounds pixels of a 3x3 window: cnt exact bf16 -> fp32 values are added ((cnt - 1) u32 sum|x|) and
divided by cnt (one rounding): (cnt + 1) u32 mean|x|, then one bf16 store.  Max pool: exact.

Global average pool (fp32 out): HW values added in fp32, one division: (HW + 1) u32 mean|x| + 4 u32 |ref|.

Bilinear resize (+ 2 x - 1).  The kernel evaluates the source coordinate src = (dst + 0.5) * (in / out) - 0.5 in fp32: the quotient,
the sum, the product and the difference round once each, relative to magnitudes <= max(IH, IW) + 1, so
|src32 - src| <= d = 4 u32 (max(IH, IW) + 1).  The interpolant is continuous and piecewise linear in each source coordinate with
slope at most D = the largest absolute difference of vertically or horizontally adjacent input pixels (image-wide), so an error of
d per axis moves it by at most 2 d D, also when the floor lands on the other side of an integer.  The weights 1 - l, l and the
four products and three sums are fp32: 8 u32 max|x| covers them.  With s = 2 when normalising (v -> 2 v - 1), else 1:
    |got - ref64| <= s (2 d D + 8 u32 max|x|) (1 + u16) + (u16 + 4 u32) |ref64|
"""
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

from backward_bounds import U16, U32, BoundError, Checker, unfold_nhwc

LOG2E = 1.0 / math.log(2.0)
ACT_L = {0: 1.0, 1: 1.0, 2: 1.0, 3: 1.1}         # Lipschitz constant per ops.ACT_* (none, leaky 0.2, relu, silu)


class FwdChecker(Checker):
    def within(self, name, got, ref, bound):
        """Element-wise |got - ref| <= bound (all fp64 of the same shape)."""
        got, ref = got.double(), ref.double()
        if got.shape != ref.shape:
            raise BoundError(f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}")
        return self._judge(name, got, ref, bound.double() + 1e-300)


def act64(v, act):
    if act == 1:
        return torch.where(v > 0, v, 0.2 * v)
    if act == 2:
        return v.clamp_min(0)
    if act == 3:
        return v * torch.sigmoid(v)
    return v


def store_bound(core, ref, bf16_out=True):
    """core: propagated fp32 error; + one bf16 (round-to-nearest) store and a few ulps of fp32 epilogue arithmetic."""
    if bf16_out:
        return core * (1 + U16) + (U16 + 4 * U32) * ref.abs()
    return core + 4 * U32 * ref.abs()


# ------------------------------------------------------------------------------------------ conv
def conv_fwd_ref(x, W, bias=None, addvec=None, residual=None, stride=1, pad=None, pad_br=None, upsample=0, chunk_bytes=1 << 29):
    """fp64 pre-activation conv and A = sum |w||x| + |fused adds|: x NHWC (concat applied, any dtype), W [Cout, Cin, k, k],
    bias [Cout], addvec [N, Cout] (a shared row expanded by the caller), residual NHWC.  upsample 1: nearest x2 in front,
    2: zero-stuffed x2 (dxmi_conv_desc.upsample).  Computed a few images at a time."""
    k = W.shape[2]
    pad = k // 2 if pad is None else pad
    pb = pad if pad_br is None else pad_br
    N, IH, IW, Cin = x.shape
    VH, VW = (2 * IH, 2 * IW) if upsample else (IH, IW)
    OH, OW = (VH + pad + pb - k) // stride + 1, (VW + pad + pb - k) // stride + 1
    Co = W.shape[0]
    Wm = W.double().reshape(Co, -1)
    Wa = Wm.abs()
    out = torch.empty(N, OH, OW, Co, dtype=torch.float64, device=x.device)
    A = torch.empty_like(out)
    per = max(1, chunk_bytes // (Cin * k * k * OH * OW * 8 * 2))
    for n0 in range(0, N, per):
        xd = x[n0:n0 + per].double()
        if upsample == 2:
            z = xd.new_zeros(xd.shape[0], VH, VW, Cin)
            z[:, ::2, ::2] = xd
            xd = z
        elif upsample:
            xd = xd.repeat_interleave(2, 1).repeat_interleave(2, 2)
        cols = unfold_nhwc(xd, k, stride, pad, pb)                          # [n, Cin*k*k, OH*OW]
        out[n0:n0 + per] = torch.einsum("ok,nkp->npo", Wm, cols).reshape(-1, OH, OW, Co)
        A[n0:n0 + per] = torch.einsum("ok,nkp->npo", Wa, cols.abs_()).reshape(-1, OH, OW, Co)
        del cols
    for t in (bias, addvec, residual):
        if t is None:
            continue
        t = t.double()
        t = t[:, None, None, :] if t.dim() == 2 else t
        out += t
        A += t.abs()
    return out, A


def conv_bound(ref_post, A, K, act, bf16_out=True):
    """Bound of a conv forward output around act(ref64): depth K + 3 (fused adds), activation Lipschitz, one bf16 store."""
    return store_bound(ACT_L[act] * (K + 3) * U32 * A, ref_post, bf16_out)


class ConvRef(NamedTuple):
    """conv_call_ref's result.  ref / bound: fp64, in the layout of the launch's output (NHWC, or NCHW for out_nchw_f32);
    pre / A: the pre-activation value and its absolute sum, NHWC; K: the accumulation depth Cin * k * k (27 for the stem)."""
    ref: torch.Tensor
    bound: torch.Tensor
    pre: torch.Tensor
    A: torch.Tensor
    K: int

    def dh(self):
        """Error of every stored bf16 element of an NHWC output, as gn_fused_bound takes it for a fused GroupNorm."""
        return (self.K + 3) * U32 * self.A + U16 * self.ref.abs()


def conv_call_ref(x0, W, x1=None, bias=None, addvec=None, residual=None, mask_src=None, mask_slope=0.0, act=0, stride=1, pad=None,
                  pad_br=None, upsample=0, out_nchw_f32=False):
    """fp64 reference and element-wise bound of one ops.conv2d launch, from the operands as the caller holds them (on whatever
    device they are; the GPU suites pass device tensors, so the reference never goes through an fp32 library conv).

    x0: NHWC bf16 (or the stem's NCHW fp32 image [N, 3, H, W], which the kernel stages as bf16: K = 27), x1 the optional concat
    source; W [Cout, Cin, k, k] fp32, rounded to bf16 here exactly as ops.pack_conv_weight rounds it (idempotent for weights
    that already are); bias [Cout]; addvec [N, Cout] or one shared row [Cout]; residual / mask_src NHWC bf16 shaped like the
    output; stride, pad (top / left), pad_br (bottom / right, default pad), upsample 0 / 1 (nearest) / 2 (zero-stuffed).

    Depth: the K = Cin k k products (zero padding and stuffed zeros add exact zeros) and the three fused adds, conv_bound's
    K + 3, for every kernel family: each adds the K products of an output element and the fused terms once, in fp32, in
    whatever order or grouping (no forward conv kernel keeps split-K partials in memory, so nothing is added twice or rounded
    to another format on the way).  The activation mask multiplies the fp32 value by 1 or by the fp32 mask_slope before the
    activation (conv_common.h epilogue; `res_is_mask` in conv_ws.hip / conv_ws8.hip / conv_sm.hip): the reference scales
    value and magnitude by that factor, and the product's rounding is one more term of depth, K + 4.  The depth comes from
    the kernels' code, never from a measured error: a launch beyond the bound is a finding about the kernel."""
    if x0.dtype == torch.float32:
        assert x1 is None and x0.shape[1] == 3, "an fp32 input is the stem's NCHW image"
        xc = x0.to(torch.bfloat16).permute(0, 2, 3, 1)
    else:
        xc = torch.cat([x0, x1], 3) if x1 is not None else x0
    N = xc.shape[0]
    Wb = W.to(torch.bfloat16)
    Cout, Cin, k, _ = Wb.shape
    assert Cin == xc.shape[3], (Cin, xc.shape)
    if addvec is not None and addvec.dim() == 1:
        addvec = addvec[None].expand(N, Cout)
    pre, A = conv_fwd_ref(xc, Wb, bias, addvec, residual, stride, pad, pad_br, upsample)
    K = Cin * k * k
    depth = K
    if mask_src is not None:
        slope = float(torch.tensor(mask_slope, dtype=torch.float32))
        f = torch.where(mask_src.double() > 0, 1.0, slope)
        pre, A, depth = pre * f, A * f, K + 1
    ref = act64(pre, act)
    bound = conv_bound(ref, A, depth, act, bf16_out=not out_nchw_f32)
    if out_nchw_f32:
        ref, bound = ref.permute(0, 3, 1, 2), bound.permute(0, 3, 1, 2)
    return ConvRef(ref, bound, pre, A, K)


def stats_ref(o, pairs=True):
    """Per image and channel pair of a stored NHWC tensor: (sum, sum of squares) and their absolute sums, fp64."""
    od = o.double()
    N, H, W, C = od.shape
    s = od.reshape(N, H * W, C // 2, 2).sum((1, 3))
    q = od.square().reshape(N, H * W, C // 2, 2).sum((1, 3))
    sa = od.abs().reshape(N, H * W, C // 2, 2).sum((1, 3))
    return torch.stack([s, q], -1), torch.stack([sa, q], -1)


def stats_depth(HW, P0, folds):
    return 2 * -(-HW // P0) + 32 * folds + 2


def fold_passes(P, group=32):
    """Passes ops.fold_stats makes over P partials (each adds `group` consecutive partials)."""
    n = 0
    while P > 8:
        P, n = -(-P // group), n + 1
    return n


# ------------------------------------------------------------------------------------------ GroupNorm
def gn_ref(x, gamma, beta, groups, eps, silu, scale_shift=None):
    """fp64 GroupNorm(+FiLM)(+SiLU) of an NHWC tensor and the per-element pieces the bound needs."""
    xd = x.double()
    N, H, W, C = xd.shape
    y = F.group_norm(xd.permute(0, 3, 1, 2), groups, gamma.double(), beta.double(), eps).permute(0, 2, 3, 1)
    g = xd.reshape(N, H * W, groups, C // groups)
    m = g.mean((1, 3), keepdim=True)
    var = (g - m).square().mean((1, 3), keepdim=True)
    ex2 = g.square().mean((1, 3), keepdim=True)
    exa = g.abs().mean((1, 3), keepdim=True)
    rstd = (var + eps).rsqrt()
    xhat = ((g - m) * rstd).reshape(N, H, W, C)
    film = torch.ones(N, 1, 1, C, dtype=torch.float64, device=x.device)
    shift = torch.zeros_like(film)
    if scale_shift is not None:
        film = 1 + scale_shift[:, :C].double()[:, None, None, :]
        shift = scale_shift[:, C:].double()[:, None, None, :]
        y = y * film + shift
    yo = act64(y, 3) if silu else y
    parts = dict(eps=eps, m=m, var=var, ex2=ex2, exa=exa, rstd=rstd, xhat=xhat, film=film, shift=shift, g=g, y=y)
    return yo, parts


def gn_bound(yo, parts, gamma, beta, d, silu):
    """Element-wise bound of a GroupNorm forward whose statistics are fp32 sums of depth d (see the module docstring)."""
    p = parts
    N, H, W, C = yo.shape
    kappa = p["ex2"] / (p["var"] + p["eps"])                 # E[x^2] / (var + eps): the conditioning term
    drstd = (1.5 * d + 1) * U32 * kappa + 4 * U32
    dm = d * U32 * p["exa"]
    x = p["g"]
    dxh = ((x - p["m"]).abs() * p["rstd"] * drstd + p["rstd"] * dm + 4 * U32 * (x.abs() + p["m"].abs()) * p["rstd"]).reshape(N, H, W, C)
    L = 1.1 if silu else 1.0
    ga, ba = gamma.double().abs(), beta.double().abs()
    core = L * (ga * p["film"].abs() * dxh + 4 * U32 * ((ga * p["xhat"].abs() + ba) * p["film"].abs() + p["shift"].abs()))
    return store_bound(core, yo)


def gn_fused_bound(yo, parts, gamma, beta, d, silu, dh):
    """gn_bound plus the propagated error dh (per element) of the GroupNorm's input through the linearised GroupNorm."""
    p = parts
    N, H, W, C = yo.shape
    G = p["g"].shape[2]
    dhg = dh.reshape(N, H * W, G, C // G)
    xh = p["xhat"].reshape(N, H * W, G, C // G).abs()
    lin = (p["rstd"] * (dhg + dhg.mean((1, 3), keepdim=True) + xh * (xh * dhg).mean((1, 3), keepdim=True))).reshape(N, H, W, C)
    L = 1.1 if silu else 1.0
    return gn_bound(yo, parts, gamma, beta, d, silu) + L * gamma.double().abs() * p["film"].abs() * lin * (1 + U16)


MIN_COND = 8.0           # the smallest (image, group) |mean| / std a GroupNorm input of the suites is conditioned to


def gn_input(g, N, H, W, C, cond, groups=32):
    """bf16 activation (on g's device) whose (image, group) |mean| / std spread up to `cond`: one offset per group, uniform in
    [-cond, cond] (unit-variance noise inside), the largest |offset| of every image set to cond; image 0's first group zero-mean
    with a tiny variance, where eps matters."""
    dev = g.device
    off = (torch.rand(N, groups, generator=g, device=dev) * 2 - 1) * cond
    off[torch.arange(N, device=dev), off.abs().argmax(1)] = cond
    x = torch.randn(N, H, W, C, generator=g, device=dev) + off.repeat_interleave(C // groups, 1)[:, None, None, :]
    x[0, :, :, :C // groups] = 0.003 * torch.randn(H, W, C // groups, generator=g, device=dev)
    return x.to(torch.bfloat16)


def block_stats_tensor(x, P):
    """fp32 BlockStats buffer [N, P, C/2, 2] of x: P contiguous chunks of ceil(HW / P) pixels (the last ones short or empty when
    P does not divide HW), sums in fp64 then rounded once."""
    N, H, W, C = x.shape
    HW = H * W
    per = -(-HW // P)
    xd = x.double().reshape(N, HW, C // 2, 2)
    xd = torch.cat([xd, xd.new_zeros(N, P * per - HW, C // 2, 2)], 1).reshape(N, P, per, C // 2, 2)
    return torch.stack([xd.sum((2, 4)), xd.square().sum((2, 4))], -1).float().contiguous()


def gn_fwd_plan(C0, C1, HW, groups=32):
    """The slicing walk of dxmi_groupnorm_silu_fwd (csrc/groupnorm.hip) restated -> the plan of gn_silu_kernel<VEC, PIECES>, or
    None where dxmi_groupnorm_silu_supported refuses: VEC channels per piece, `slices` channel slices (whole groups each), ppp
    pieces per pixel of a slice, `threads` a multiple of lcm(ppp, 64), `pieces` per thread (<= 16 at VEC 8, <= 32 at VEC 4 before
    another halving is tried; <= 32 at the last), `ragged` when the last piece of some thread lies past the map, ppt pieces per
    group and pixel, `fast`: the xor-shuffle group reduce (else a masked wave sum per group)."""
    C = C0 + C1
    if groups <= 0 or groups > 32 or C % groups:
        return None
    cpg = C // groups
    if cpg % 4 or C0 % 4:
        return None
    VEC = 8 if (cpg % 8 == 0 and C0 % 8 == 0) else 4
    max_pieces = 16 if VEC == 8 else 32
    slices = 1
    while True:
        if groups % slices:
            return None
        ppp = C // slices // VEC
        unit = ppp // math.gcd(ppp, 64) * 64
        if unit > 512:
            return None
        total = HW * ppp
        threads = (512 // unit) * unit
        if total < threads:
            threads = -(-total // unit) * unit
        pieces = -(-total // threads)
        if pieces <= max_pieces or slices == groups:
            break
        slices *= 2
    if pieces > 32:
        return None
    ppt = cpg // VEC
    fast = ppp <= 64 and ppp & (ppp - 1) == 0 and ppt & (ppt - 1) == 0
    return dict(VEC=VEC, slices=slices, ppp=ppp, threads=threads, pieces=pieces, ragged=total % threads != 0, fast=fast, ppt=ppt)


def gn_apply_chunks(HW, C):
    """gn_apply_impl's chunking under the default knobs: two trips of four rows by 256 // (C / 8) row lanes per workgroup
    -> (rows per chunk, chunks per image)."""
    rpc = min(2 * 4 * (256 // (C // 8)), HW)
    return rpc, -(-HW // rpc)


def gn_fwd_checked(ops, path, x0, gamma, beta, in1=None, groups=32, eps=1e-6, silu=True, scale_shift=None, saved=None, st0=None,
                   st1=None, cond=None, tag=None, check=None):
    """One GroupNorm(+FiLM)(+SiLU) forward launch on `path` under gn_bound, tagged groupnorm[<tag or path>] in `check` (default
    EDGE): "resident" (ops.groupnorm_silu without statistics; dxmi_groupnorm_silu_supported is asserted), "generic"
    (ops.groupnorm_generic, `saved` as given) or "apply" (ops.groupnorm_apply with the BlockStats st0 / st1).  Depth of the
    statistics: the group size + 2 (any order of the partial sums) for the first two, max(P0, P1) + cpg / 2 + 2 for the apply
    (a pair adds its P partials, then a group its cpg / 2 pairs, + the rounding of the given partials).  cond: the largest
    (image, group) |mean| / std of the input must exceed 0.9 cond.  -> the kernel's output."""
    check = EDGE if check is None else check
    N, H, W, C0 = x0.shape
    C1 = in1.shape[3] if in1 is not None else 0
    C = C0 + C1
    if path == "apply":
        got = ops.groupnorm_apply(x0, st0, gamma, beta, in1=in1, st1=st1, groups=groups, eps=eps, silu=silu, scale_shift=scale_shift)
        d = max(st0.P, st1.P if st1 is not None else 0) + C // groups // 2 + 2
    elif path == "generic":
        got = ops.groupnorm_generic(x0, gamma, beta, in1=in1, groups=groups, eps=eps, silu=silu, scale_shift=scale_shift, saved=saved)
        d = H * W * C // groups + 2
    else:
        assert path == "resident" and scale_shift is None
        assert ops.load().dxmi_groupnorm_silu_supported(C0, C1, H * W, groups) == 1
        got = ops.groupnorm_silu(x0, gamma, beta, in1=in1, groups=groups, eps=eps, silu=silu)
        d = H * W * C // groups + 2
    xc = torch.cat([x0, in1], 3) if in1 is not None else x0
    yo, parts = gn_ref(xc, gamma, beta, groups, eps, silu, scale_shift)
    if cond is not None:
        assert float((parts["m"].abs() / parts["var"].sqrt()).max()) > 0.9 * cond          # the stated conditioning is reached
    check.within(f"groupnorm[{tag or path}]", got, yo, gn_bound(yo, parts, gamma, beta, d, silu))
    return got


# ------------------------------------------------------------------------------------------ linear
def bf16_near_tie(v):
    """Mask of fp64 values within 8 u32 |v| of a bf16 rounding midpoint (an fp32 evaluation may round them either way)."""
    b = v.to(torch.bfloat16).double()
    e = torch.floor(torch.log2(b.abs().clamp_min(1e-38)))
    half = 2.0 ** (e - 8)
    return ((v - b).abs() - half).abs() <= 8 * U32 * v.abs() + 1e-300


def linear_ref(x, W, bias, pre_act, post_act, depth=None):
    """fp64 reference of ops.linear and its element-wise bound: x fp32 [P, K], W fp32 [M, K] (bf16-rounded by the pack).
    depth: the accumulation depth of the sum (default K + 2: the K products and the bias; a split-K launch adds its S partial
    sums: K + 2 + S); the tie and store terms do not depend on it."""
    pre = act64(x.double(), pre_act)
    a = pre.to(torch.bfloat16).double()
    Wb = W.to(torch.bfloat16).double()
    y = a @ Wb.T
    A = a.abs() @ Wb.abs().T
    if bias is not None:
        y, A = y + bias.double(), A + bias.double().abs()
    tie = (bf16_near_tie(pre) * pre.abs() * U16) @ Wb.abs().T
    ref = act64(y, post_act)
    K = x.shape[1]
    depth = K + 2 if depth is None else depth
    bound = ACT_L[post_act] * (depth * U32 * A + tie) + 4 * U32 * ref.abs()
    return ref, bound


# ------------------------------------------------------------------------------------------ launches of the edge-case suites
EDGE = FwdChecker()      # shared by the conv / linear edge-case modules: report() gives one worst |err| / bound per kernel family


def conv_family(kid):
    """Kernel family of a dxmi_conv2d_kernel_id value (the names bench.kernel_name groups them by)."""
    if kid >= 600000:
        return "head"
    if kid >= 550000:
        return "rw8"
    if kid >= 500000:
        return "rw"
    if kid >= 450000:
        return "sm"
    if kid >= 400000:
        return "ws8" if kid in (400008, 400009) else "ws"
    if kid >= 300000:
        return "stem"
    if kid >= 200000:
        return "stream1x1"
    return "pipe" if kid >= 10000 else "igemm"


def launch_conv(ops, x0, pw, **kw):
    """ops.conv2d(x0, pw, **kw) -> (its result, the kernel id dxmi_conv2d_kernel_id names for the descriptor it launched)."""
    import ctypes
    kids = []

    class Probe(ops.OpProfiler):
        def launch_conv(self, d):
            kids.append(int(ops.load().dxmi_conv2d_kernel_id(ctypes.byref(d))))
            ops.check(ops.load().dxmi_conv2d_fwd(ctypes.byref(d), ops._stream()), "dxmi_conv2d_fwd")

    old, ops.PROFILER = ops.PROFILER, Probe()
    try:
        res = ops.conv2d(x0, pw, **kw)
    finally:
        ops.PROFILER = old
    assert len(kids) == 1, kids
    return res, kids[0]


def conv_checked(ops, x0, pw, W, check=None, **kw):
    """ops.conv2d(x0, pw, **kw) with everything it writes judged element by element against fp64 (conv_call_ref of the same
    operands; W: the fp32 weight pw was packed from, on any device), tagged conv[<family>] in `check` (default EDGE):
    the raw output; with fuse_gn the fused GroupNorm output (around the stored raw tensor when it is kept, else with the raw
    tensor's error propagated: gn_fused_bound; statistics depth = the group size, valid for any order); with want_stats the
    block statistics of the stored output (stats_depth of the partial count the conv wrote, one fold pass where ops folded).
    -> (the result of ops.conv2d, kernel id)."""
    check = EDGE if check is None else check
    seen, orig_fold = [], ops.fold_stats

    def fold(st, group=32):
        seen.append(st.P)
        return orig_fold(st, group)

    ops.fold_stats = fold
    try:
        res, kid = launch_conv(ops, x0, pw, **kw)
    finally:
        ops.fold_stats = orig_fold
    fam = conv_family(kid)
    fuse, want_stats = kw.get("fuse_gn"), kw.get("want_stats", False)
    c = conv_call_ref(x0, W.to(x0.device), kw.get("in1"), kw.get("bias"), kw.get("addvec"), kw.get("residual"), kw.get("mask_src"),
                      kw.get("mask_slope", 0.0), kw.get("act", 0), kw.get("stride", 1), kw.get("pad"), kw.get("pad_br"),
                      int(kw.get("upsample", 0)), kw.get("out_nchw_f32", False))
    out, st, y = res, None, None
    if fuse is not None:
        out, y = res
    elif want_stats:
        out, st = res
    if out is not None:
        check.within(f"conv[{fam}]", out, c.ref, c.bound)
    if st is not None:
        HW = out.shape[1] * out.shape[2]
        P0 = seen[0] if seen else st.P
        S, Sa = stats_ref(out)
        check.fp32(f"block_stats[{fam}]", st.buf.double().sum(1), S, Sa, stats_depth(HW, P0, fold_passes(P0)))
    if y is not None:
        gamma, beta, groups, eps, silu, keep_raw = fuse
        d = c.ref.shape[1] * c.ref.shape[2] * c.ref.shape[3] // groups
        if out is not None:
            yo, parts = gn_ref(out, gamma, beta, groups, eps, silu)
            bnd = gn_bound(yo, parts, gamma, beta, d, silu)
        else:
            yo, parts = gn_ref(c.ref, gamma, beta, groups, eps, silu)
            bnd = gn_fused_bound(yo, parts, gamma, beta, d, silu, c.dh())
        check.within(f"conv_fused_gn[{fam}]", y, yo, bnd)
    return res, kid


def linear_checked(ops, x, pw, W, bias=None, pre_act=0, post_act=0, splitk=False, check=None):
    """ops.linear under linear_ref's bound, tagged `linear` (`linear[splitk]` when the split-K form ran: its S partial sums
    are added after the K products, depth K + 2 + S)."""
    check = EDGE if check is None else check
    got = ops.linear(x, pw, bias, pre_act=pre_act, post_act=post_act, splitk=splitk)
    P, K = x.shape
    S = int(ops.load().dxmi_linear_splitk_slices(P, K, pw.Cout)) if (splitk and post_act == 0) else 1
    ref, bound = linear_ref(x, W.to(x.device), bias, pre_act, post_act, depth=K + 2 + (S if S > 1 else 0))
    check.within("linear[splitk]" if S > 1 else "linear", got, ref, bound)
    return got


# ------------------------------------------------------------------------------------------ attention
def attention_ref(qkv, heads, scale, chunk=4):
    """fp64 softmax attention of qkv [N, T, 3C] (heads as contiguous channel blocks): o [N, T, C], lse2 [N, heads, T] (log2
    domain) and the per-row score magnitude max_j sum_d |q_id k_jd| [N, heads, T]."""
    N, T, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    o = torch.empty(N, T, C, dtype=torch.float64, device=qkv.device)
    lse = torch.empty(N, heads, T, dtype=torch.float64, device=qkv.device)
    smag = torch.empty_like(lse)
    for n0 in range(0, N, chunk):
        x = qkv[n0:n0 + chunk].double()
        q, k, v = (x[:, :, i * C:(i + 1) * C].reshape(-1, T, heads, D).transpose(1, 2) for i in range(3))
        s = scale * q @ k.transpose(-1, -2)
        lse[n0:n0 + chunk] = torch.logsumexp(s, -1) * LOG2E
        smag[n0:n0 + chunk] = (abs(scale) * q.abs() @ k.abs().transpose(-1, -2)).amax(-1)      # a magnitude: scale may be negative
        o[n0:n0 + chunk] = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(-1, T, C)
    return o, lse, smag


def lse_bound(lse2, smag, D, T):
    return LOG2E * (D + 2) * U32 * smag + (T + 8) * U32 * LOG2E + 4 * U32 * lse2.abs()


def attn_blocks(t, heads, rb=128):
    """[N, T, C] -> (image, head, 128-row block) blocks for Checker.blocks(..., block_dims=3)."""
    N, T, C = t.shape
    rb = min(rb, T)
    return t.reshape(N, T // rb, rb, heads, C // heads).permute(0, 3, 1, 2, 4)


def attn_elem_bound(qkv, heads, scale, chunk=4):
    """attention_ref's (o, lse2, smag) and the element-wise bound of o [N, T, C] derived in the module docstring, a few images
    at a time."""
    N, T, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    o, lse2, smag = attention_ref(qkv, heads, scale, chunk)
    bound = torch.empty_like(o)
    for n0 in range(0, N, chunk):
        x = qkv[n0:n0 + chunk].double()
        n = x.shape[0]
        q, k, v = (x[:, :, i * C:(i + 1) * C].reshape(n, T, heads, D).transpose(1, 2) for i in range(3))
        a = (torch.softmax(scale * q @ k.transpose(-1, -2), -1) @ v.abs()).transpose(1, 2).reshape(n, T, C)
        delta = (D + 2) * U32 * smag[n0:n0 + chunk].transpose(1, 2)[..., None].expand(n, T, heads, D).reshape(n, T, C)
        oc = o[n0:n0 + chunk]
        bound[n0:n0 + chunk] = (U16 + 2 * delta + (T + 8) * U32) * a * (1 + U16) + (U16 + 4 * U32) * oc.abs()
    return o, lse2, smag, bound


def attn_inputs(g, N, T, heads, D, kind):
    """bf16 qkv [N, T, 3 heads D] on g's device.  kind "gauss": unit Gaussians.  "below_zero": the component of every q and k
    head vector along one unit vector u is replaced by -3 D^(1/4) (q) and +3 D^(1/4) (k), so that D^-1/2 q.k = -9 + N(0, 1): every
    true score is far below the exp(0) of a zero-filled key.  "peaked": q and k times 3, scores of +-30 and more, so that the
    running maximum moves in most key blocks."""
    C = heads * D
    x = torch.randn(N, T, 3 * C, generator=g, device=g.device)
    if kind == "below_zero":
        u = torch.randn(D, generator=g, device=g.device)
        u /= u.norm()
        qq, kk = x[:, :, :C].view(N, T, heads, D), x[:, :, C:2 * C].view(N, T, heads, D)
        qq -= (qq @ u)[..., None] * u
        kk -= (kk @ u)[..., None] * u
        qq -= 3.0 * D ** 0.25 * u
        kk += 3.0 * D ** 0.25 * u
    elif kind == "peaked":
        x[:, :, :2 * C] *= 3
    else:
        assert kind == "gauss", kind
    return x.to(torch.bfloat16)


def attn_max_score(qkv, heads, scale):
    """Largest fp64 score scale q.k of the whole batch."""
    N, T, C3 = qkv.shape
    C = C3 // 3
    x = qkv.double()
    q, k = (x[:, :, i * C:(i + 1) * C].reshape(N, T, heads, C // heads).transpose(1, 2) for i in range(2))
    return float((scale * q @ k.transpose(-1, -2)).max())


def attn_xcd_logical(b, G):
    """attn_xcd_logical of csrc/attention.hip restated: hardware block b of a grid of G -> logical block (XCD b % 8 owns
    G // 8 + (b % 8 < G % 8) consecutive logical ids)."""
    x, k = b & 7, b >> 3
    q, r = G >> 3, G & 7
    return x * q + min(x, r) + k


def attention_checked(ops, qkv, heads, scale, tag, want_lse=False, check=None):
    """ops.attention under attn_elem_bound (tagged attention[<tag>] in `check`, default EDGE), the lse, where one is returned,
    under lse_bound; a second identical launch must be bitwise the first.  -> what ops.attention returned."""
    check = EDGE if check is None else check
    N, T, C3 = qkv.shape
    res = ops.attention(qkv, heads, scale, want_lse=want_lse)
    got, lse = res if want_lse else (res, None)
    o, lse2, smag, bound = attn_elem_bound(qkv, heads, scale)
    check.within(f"attention[{tag}]", got, o, bound)
    if lse is not None:
        check.within(f"attention_lse2[{tag}]", lse, lse2, lse_bound(lse2, smag, C3 // 3 // heads, T))
    again = ops.attention(qkv, heads, scale, want_lse=want_lse)
    again, lse_b = again if want_lse else (again, None)
    assert torch.equal(got, again) and (lse is None or torch.equal(lse, lse_b)), f"attention[{tag}]: two launches differ"
    return res


def attention_case(ops, N, T, heads, D, kind, tag, scale=None, want_lse=False, check=None, device="cuda:0"):
    """One edge case of ops.attention on attn_inputs seeded by the case itself: attention_checked, every true score below -3
    for the below-zero kind, and image N - 1 run alone bitwise its rows of the batch.  -> (qkv, what ops.attention returned)."""
    import zlib
    g = torch.Generator(device=device).manual_seed(zlib.crc32(repr((N, T, heads, D, kind)).encode()))
    scale = D ** -0.5 if scale is None else scale
    qkv = attn_inputs(g, N, T, heads, D, kind)
    if kind == "below_zero":
        assert scale > 0 and attn_max_score(qkv, heads, scale) < -3
    res = attention_checked(ops, qkv, heads, scale, tag, want_lse=want_lse, check=check)
    out = res[0] if want_lse else res
    assert torch.equal(ops.attention(qkv[N - 1:].contiguous(), heads, scale)[0], out[N - 1]), f"attention[{tag}]: batch dependence"
    return qkv, res


# ------------------------------------------------------------------------------------------ non-network launches of a step
def pool_act_ref(x, pool, act):
    """2x2 mean pool (optional) + activation of a bf16 NHWC tensor in fp64, and its bound: four exact bf16 -> fp32 values are
    added and scaled by 0.25 (<= 4 u32 of the mean of |x|), the activation is evaluated in fp32, one bf16 store."""
    xd, xa = x.double(), x.double().abs()
    if pool:
        N, H, W, C = x.shape
        xd = xd.reshape(N, H // 2, 2, W // 2, 2, C).mean((2, 4))
        xa = xa.reshape(N, H // 2, 2, W // 2, 2, C).mean((2, 4))
    ref = act64(xd, act)
    return ref, store_bound(4 * U32 * xa, ref)


def edm_scalings64(sigma, sd=0.5):
    """(c_skip, c_out, c_in) of KarrasDenoiser.get_scalings in fp64."""
    s = sigma.double()
    return sd ** 2 / (s ** 2 + sd ** 2), s * sd / (s ** 2 + sd ** 2) ** 0.5, 1 / (s ** 2 + sd ** 2) ** 0.5


def log_sigma_t(sigma):
    """t = 250 ln(sigma) and its bound: logf to <= 4 ulp and two fp32 products (16 u32 |t| covers them generously), plus the
    absolute error of ln near sigma = 1, where |t| is small: 250 * 4 u32."""
    lt = 250 * torch.log(sigma.double())
    return lt, 16 * U32 * lt.abs() + 250 * 4 * U32


def scaled_input_ref(x, sigma, noise=None):
    """x_in = c_in(sigma) (x [+ noise sigma]) per sample (edm_precond without noise, edm_dsm_prep with it), x [N, CHW] -> (ref, A).
    c_in is an fp32 expression of four operations and a powf (<= 8 u32 relative), the sum and the product add two roundings:
    |got - ref| <= 16 u32 A with A = c_in (|x| + |noise sigma|)."""
    c_in = edm_scalings64(sigma)[2][:, None]
    xt, M = x.double(), x.double().abs()
    if noise is not None:
        ns = noise.double() * sigma.double()[:, None]
        xt, M = xt + ns, M + ns.abs()
    return c_in * xt, c_in * M


def dsm_error_terms(F, x0, noise, sigma, scalings):
    """e = c_out F + c_skip (x0 + noise sigma) - x0 of the DSM loss and the sum Me of its absolute terms, fp64 [N, CHW].
    In fp32 every factor (c_out, c_skip, x_t) carries <= 8 u32 and the three-term sum two more roundings: |fl(e) - e| <= 16 u32 Me."""
    c_skip, c_out = scalings[0][:, None], scalings[1][:, None]
    xt = x0.double() + noise.double() * sigma.double()[:, None]
    e = c_out * F.double() + c_skip * xt - x0.double()
    Me = (c_out * F.double()).abs() + (c_skip * xt).abs() + x0.double().abs()
    return e, Me, c_out


def dsm_loss_fwd_bound(e, Me, w=None):
    """Bound of the per-sample DSM terms mean_CHW(e^2) (and w times it).  Each square is computed from fl(e) with
    |fl(e) - e| <= 16 u32 Me: |fl(e)^2 - e^2| <= 2 * 16 u32 Me (|e| + 16 u32 Me), its mean the second term.  The sum of the CHW
    squares, in whatever order, and the division by CHW: (CHW + 16) u32 mean(e^2), the first term (the depth-d bound; no measured
    constant).  The weighted term multiplies by the fp32 weight w(sigma), an expression of <= 6 operations: 8 u32 relative on
    the product, hence (1 + 8 u32) on the bound and 8 u32 w mean(e^2)."""
    CHW = e.shape[1]
    m = (e ** 2).mean(1)
    b = (CHW + 16) * U32 * m + 2 * 16 * U32 * (Me * (e.abs() + 16 * U32 * Me)).mean(1)
    if w is None:
        return m, b
    return w * m, w * b * (1 + 8 * U32) + 8 * U32 * w * m


def td_gather_cost_ref(xn, x, beta):
    """Running cost mean_CHW (x' - x)^2 / (2 beta) in fp64 and the sum of its absolute terms: the differences and squares are
    fp32 (<= 3 roundings, covered by taking (|x'| + |x|)^2 as the term magnitude), the sum has depth CHW: c = CHW + 8."""
    b2 = 2 * beta.double()
    xn, x = xn.double(), x.double()
    return ((xn - x) ** 2).mean(1) / b2, ((xn.abs() + x.abs()) ** 2).mean(1) / b2


def var_step_ref(x, eps, z, xm, cm, sg):
    """The VAR transition (models/DxMI/var_sampler.py:285 / :399) in fp64, x / eps / z [N, CHW], per-sample xm, cm, sg [N]:
    control = cm eps, mean = xm x + control, x' = mean + sg z, logp = mean_CHW(-(x' - mean)^2 / (2 sg^2) - ln sg - ln sqrt(2 pi)).
    -> {name: (ref, bound)}.  The three image outputs are sums of <= 3 fp32 products: 4 u32 A, A = |xm x| + |cm eps| + |sg z|
    (either association of the sum).  The kernel forms d = x' - mean from the ROUNDED x': |fl(d) - sg z| <= 3 u32 A =: dd (the
    rounding of x', of sg z and of the difference), so a log-prob term errs by (2 |sg z| dd + dd^2) / (2 sg^2) plus 4 u32 of its
    own absolute terms T = z^2 / 2 + |ln sg| + ln sqrt(2 pi); the sum over CHW, in any order, adds (CHW + 8) u32 mean(T)."""
    import math
    e = lambda v: v.double()[:, None]
    x, eps, z = x.double(), eps.double(), z.double()
    control = e(cm) * eps
    mean = x * e(xm) + control
    xn = mean + e(sg) * z
    A = (x * e(xm)).abs() + control.abs() + (e(sg) * z).abs()
    c = math.log(math.sqrt(2 * math.pi))
    logp = (-(z ** 2) / 2 - torch.log(e(sg)) - c).mean(1)
    T = z ** 2 / 2 + torch.log(e(sg)).abs() + c
    dd = 3 * U32 * A
    CHW = x.shape[1]
    lb = ((2 * (e(sg) * z).abs() * dd + dd ** 2) / (2 * e(sg) ** 2) + 4 * U32 * T).mean(1) + (CHW + 8) * U32 * T.mean(1)
    return {"x_next": (xn, 4 * U32 * A), "mean": (mean, 4 * U32 * A), "control": (control, 4 * U32 * control.abs()), "logp": (logp, lb)}


def edm_step_ref(x, F, z, sigma, sdn, sup, sd=0.5):
    """The Euler-ancestral EDM transition (models/DxMI/openai_diffusion.py:71-94) in fp64, [N, CHW] and per-sample scalars:
    den = c_out F + c_skip x, mu = x + (x - den) / sigma (sigma_down - sigma), x' = mu + z sigma_up -> (mu, x', A_mu, A_x'),
    each within 16 u32 A: the scalings carry <= 8 u32, every further operation one rounding of its absolute terms
    A_mu = |x| + (|x| + |c_out F| + |c_skip x|) |sigma_down - sigma| / sigma, A_x' = A_mu + |z sigma_up|."""
    e = lambda v: v.double()[:, None]
    c_skip, c_out, _ = [c[:, None] for c in edm_scalings64(sigma, sd)]
    x, F, z = x.double(), F.double(), z.double()
    den = c_out * F + c_skip * x
    dt = e(sdn) - e(sigma)
    mu = x + (x - den) / e(sigma) * dt
    A = x.abs() + (x.abs() + (c_out * F).abs() + (c_skip * x).abs()) / e(sigma) * dt.abs()
    return mu, mu + z * e(sup), A, A + (z * e(sup)).abs()


# ------------------------------------------------------------------------------------------ InceptionV3 extractor (csrc/inception_ops.hip)
def gconv_unpack(wp, Cout, Cin, KH, KW):
    """Packed buffer [CoutP][KH * KW][CinP] (flat bf16) -> [CoutP, CinP, KH, KW] in the OIHW order of the checkpoint."""
    CoutP, CinP = -(-Cout // 32) * 32, -(-Cin // 16) * 16
    assert wp.numel() == CoutP * KH * KW * CinP, (wp.numel(), CoutP, KH, KW, CinP)
    return wp.reshape(CoutP, KH * KW, CinP).permute(0, 2, 1).reshape(CoutP, CinP, KH, KW)


def gconv_pack_ref(weight, bn, eps):
    """fp64 fold of BatchNorm into the conv: (w scale [Cout, Cin, KH, KW], bias [Cout], bias magnitude |beta| + |mean scale|)."""
    w = weight.double()
    if bn is None:
        z = torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
        return w, z, z
    gamma, beta, mean, var = (t.double() for t in bn)
    scale = gamma / torch.sqrt(var + eps)
    return w * scale[:, None, None, None], beta - mean * scale, beta.abs() + (mean * scale).abs()


def gconv_pack_bounds(fold, bias_mag):
    return (U16 + 8 * U32) * fold.abs(), 8 * U32 * bias_mag


def gconv_ref(x, w4, bias, stride, pad, chunk_bytes=1 << 29):
    """fp64 pre-activation conv with a rectangular kernel and A = sum |w||x| + |bias|: x NHWC [N, IH, IW, C] (any dtype),
    w4 [Cout, C, KH, KW], bias [Cout], stride / pad pairs (h, w).  A few images at a time, as conv_fwd_ref."""
    N, IH, IW, C = x.shape
    Co, Cw, KH, KW = w4.shape
    assert Cw == C, (Cw, C)
    OH, OW = (IH + 2 * pad[0] - KH) // stride[0] + 1, (IW + 2 * pad[1] - KW) // stride[1] + 1
    Wm = w4.double().reshape(Co, -1)
    Wa = Wm.abs()
    out = torch.empty(N, OH, OW, Co, dtype=torch.float64, device=x.device)
    A = torch.empty_like(out)
    per = max(1, chunk_bytes // (C * KH * KW * OH * OW * 8 * 2))
    for n0 in range(0, N, per):
        cols = F.unfold(x[n0:n0 + per].double().permute(0, 3, 1, 2), (KH, KW), padding=tuple(pad), stride=tuple(stride))   # [n, C*KH*KW, OH*OW]
        out[n0:n0 + per] = torch.einsum("ok,nkp->npo", Wm, cols).reshape(-1, OH, OW, Co)
        A[n0:n0 + per] = torch.einsum("ok,nkp->npo", Wa, cols.abs_()).reshape(-1, OH, OW, Co)
        del cols
    b = bias.double()
    out += b
    A += b.abs()
    return out, A


def avgpool3x3_ref(x, stride, pad):
    """Average over the in-bounds pixels of each 3x3 window of an NHWC tensor in fp64 (F.avg_pool2d, count_include_pad=False)
    and its bound."""
    xd = x.double().permute(0, 3, 1, 2)
    ref = F.avg_pool2d(xd, 3, stride, pad, count_include_pad=False).permute(0, 2, 3, 1)
    mabs = F.avg_pool2d(xd.abs(), 3, stride, pad, count_include_pad=False).permute(0, 2, 3, 1)
    cnt = 9 * F.avg_pool2d(torch.ones_like(xd[:, :1]), 3, stride, pad, count_include_pad=True).permute(0, 2, 3, 1)
    return ref, store_bound((cnt + 1) * U32 * mabs, ref), cnt


def maxpool3x3_ref(x, stride, pad):
    return F.max_pool2d(x.double().permute(0, 3, 1, 2), 3, stride, pad).permute(0, 2, 3, 1)


def global_avgpool_ref(x):
    """[N, H, W, C] -> fp64 mean over the pixels [N, C] and its bound (fp32 output)."""
    xd = x.double()
    HW = x.shape[1] * x.shape[2]
    ref = xd.mean((1, 2))
    return ref, store_bound((HW + 1) * U32 * xd.abs().mean((1, 2)), ref, bf16_out=False)


def _src_index(O, I, device):
    """Source coordinate of F.interpolate(mode='bilinear', align_corners=False) in fp64: (i0, i1, l)."""
    s = ((torch.arange(O, dtype=torch.float64, device=device) + 0.5) * (I / O) - 0.5).clamp_min(0)
    i0 = s.floor().clamp_max(I - 1)
    i1 = (i0 + 1).clamp_max(I - 1)
    return i0.long(), i1.long(), s - i0


def resize_ref(x, OH, OW, normalize):
    """Closed-form bilinear resize (+ 2 x - 1) of NCHW [N, 3, IH, IW] in fp64 -> (ref NHWC [N, OH, OW, 3], bound)."""
    xd = x.double()
    N, C, IH, IW = xd.shape
    y0, y1, ly = _src_index(OH, IH, x.device)
    x0, x1, lx = _src_index(OW, IW, x.device)
    ly, lx = ly[:, None], lx[None, :]
    top = xd[:, :, y0][:, :, :, x0] * (1 - lx) + xd[:, :, y0][:, :, :, x1] * lx
    bot = xd[:, :, y1][:, :, :, x0] * (1 - lx) + xd[:, :, y1][:, :, :, x1] * lx
    ref = top * (1 - ly) + bot * ly
    s = 1.0
    if normalize:
        ref, s = 2 * ref - 1, 2.0
    ref = ref.permute(0, 2, 3, 1)
    d = 4 * U32 * (max(IH, IW) + 1)
    D = max(float((xd[:, :, 1:] - xd[:, :, :-1]).abs().max()) if IH > 1 else 0.0,
            float((xd[:, :, :, 1:] - xd[:, :, :, :-1]).abs().max()) if IW > 1 else 0.0)
    core = s * (2 * d * D + 8 * U32 * float(xd.abs().max()))
    return ref, store_bound(torch.full_like(ref, core), ref)


def resize_emulate_f32(x, OH, OW, normalize):
    """The expressions of resize_norm_kernel evaluated by torch in fp32, operation by operation, before the bf16 store: what
    the bound's pre-store part is checked against without a device (NHWC [N, OH, OW, 3] fp32)."""
    N, C, IH, IW = x.shape
    f = torch.float32

    def idx(O, I):
        sc = torch.tensor(I, dtype=f) / torch.tensor(O, dtype=f)
        s = ((torch.arange(O, dtype=f) + 0.5) * sc - 0.5).clamp_min(0)
        i0 = s.to(torch.int64)
        i1 = i0 + (i0 < I - 1).long()
        return i0, i1, s - i0.to(f)
    y0, y1, ly = idx(OH, IH)
    x0, x1, lx = idx(OW, IW)
    ly, lx = ly[:, None], lx[None, :]
    xf = x.to(f)
    g = lambda yi, xi: xf[:, :, yi][:, :, :, xi]
    v = (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))
    if normalize:
        v = 2 * v - 1
    return v.permute(0, 2, 3, 1)
