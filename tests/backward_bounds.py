"""Error bounds for the backward kernels, checked element by element against an fp64 reference of the same operation.

fp32-output GEMM-like kernels (weight gradient, its bias gradient, linear_bwd dW, column sums).  Every output element is a sum
of products a*b of bf16 operands.  A bf16 x bf16 product is exact in fp32 (8 + 8 significant bits), so the only rounding is in
the additions.  The weight-gradient kernel adds the products of one output element along a chain of `L` pixels (the pixel
tiles s, s + S, s + 2S, ... of split s, `tile_px` pixels each, L = ceil(PT / S) * tile_px, zero-padded pixels included), then
the reduce adds the S split partials (and, with accumulate, the old value).  Recursive summation of n terms in precision u
satisfies |fl(sum) - sum| <= (n - 1) u sum |x_i| (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), whatever the
order or grouping of the additions, and the MFMA's internal adds are fp32 adds of the same kind.  With every partial and
chain bounded by the same A = sum |a||b| (computed in fp64 from the same operands):

    |got - ref64| <= c * u32 * A,      c = L + S + 2      (u32 = 2^-24; the 2 covers the accumulate add and the OIHW copy)

bf16-output kernels (data-gradient convs, GroupNorm dx, linear_bwd dx) round the fp32 result once more:

    |got - ref64| <= c * u32 * A * (1 + u16) + u16 * |ref64|      (u16 = 2^-8)

with c the accumulation depth of the kernel (the reduction length K = Cin * k * k of a conv, plus the fused adds).

Kernels that keep bf16 intermediates (attention: P and dS are bf16 MFMA operands) are judged by rel-L2 per output block at
the kernel's own tile size (image, head, 128-query-row block): each block must hold its own error below `tol`, so a wrong
block cannot hide behind the norm of the others.

`Checker` keeps the largest |err| / bound it has seen per op name (the PR reports it).
"""
import math

import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -8


def wgrad_depth(plan):
    """c of the fp32 GEMM bound for a weight-gradient launch described by ops.conv2d_wgrad_plan()."""
    L = -(-plan["PT"] // plan["S"]) * plan["tile_px"]
    return L + plan["S"] + 2


class BoundError(AssertionError):
    pass


class Checker:
    def __init__(self):
        self.worst = {}

    def _note(self, name, ratio):
        if ratio > self.worst.get(name, (0.0,))[0]:
            self.worst[name] = (ratio,)

    def fp32(self, name, got, ref, A, c):
        """Element-wise: |got - ref| <= c * u32 * A.  got: fp32 kernel output, ref / A: fp64 of the same shape."""
        got, ref, A = got.double(), ref.double(), A.double()
        if got.shape != ref.shape:
            raise BoundError(f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}")
        bound = c * U32 * A + 1e-300
        return self._judge(name, got, ref, bound)

    def bf16(self, name, got, ref, A, c):
        """Element-wise: |got - ref| <= c * u32 * A * (1 + u16) + u16 * |ref|.  got: bf16 kernel output."""
        got, ref, A = got.double(), ref.double(), A.double()
        if got.shape != ref.shape:
            raise BoundError(f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}")
        bound = c * U32 * A * (1 + U16) + U16 * ref.abs() + 1e-300
        return self._judge(name, got, ref, bound)

    def _judge(self, name, got, ref, bound):
        if not torch.isfinite(got).all():
            raise BoundError(f"{name}: non-finite output")
        r = ((got - ref).abs() / bound)
        worst = float(r.max())
        self._note(name, worst)
        if worst > 1.0:
            i = int(r.argmax())
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))
            raise BoundError(f"{name}: |err| / bound = {worst:.3g} at {idx} (got {float(got.flatten()[i]):.6g}, "
                             f"ref {float(ref.flatten()[i]):.6g}, bound {float(bound.flatten()[i]):.3g}); "
                             f"{int((r > 1).sum())} of {r.numel()} elements out of bound")
        return worst

    def blocks(self, name, got, ref, tol, block_dims):
        """rel-L2 per block: got / ref are reshaped so that the dims listed in block_dims index the blocks and the rest are
        flattened into the block; every block's ||got - ref|| / ||ref|| must stay <= tol."""
        got, ref = got.double(), ref.double()
        if not torch.isfinite(got).all():
            raise BoundError(f"{name}: non-finite output")
        nb = math.prod(got.shape[: block_dims])
        d = (got - ref).reshape(nb, -1).norm(dim=1)
        n = ref.reshape(nb, -1).norm(dim=1) + 1e-300
        r = d / n / tol
        worst = float(r.max())
        self._note(name, worst)
        if worst > 1.0:
            raise BoundError(f"{name}: block {int(r.argmax())} rel-L2 {worst * tol:.3g} > {tol:.3g} "
                             f"({int((r > 1).sum())} of {nb} blocks out of bound)")
        return worst

    def report(self):
        return {k: round(v[0], 4) for k, v in sorted(self.worst.items())}


# ------------------------------------------------------------------------------------------ fp64 references (stock torch)
def unfold_nhwc(x, k, stride, pad, pad_br=None):
    """[N, H, W, C] -> [N, C*k*k, L] columns of F.unfold (channel-major, then ky, kx: the OIHW order)."""
    import torch.nn.functional as F
    xn = x.permute(0, 3, 1, 2)
    pb = pad if pad_br is None else pad_br
    xn = F.pad(xn, (pad, pb, pad, pb)) if pb >= 0 else F.pad(xn, (pad, 0, pad, 0))[:, :, : pb, : pb]
    return F.unfold(xn, k, stride=stride)


def wgrad_ref(x, dy, k, stride=1, pad=None, upsample=0):
    """dW [Cout, Cin, k, k] and A = sum |dy||x| in fp64; x [N, IH, IW, Cin] (concat already applied), dy [N, OH, OW, Cout]."""
    if pad is None:
        pad = k // 2
    x = x.double()
    if upsample:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    N, OH, OW, Co = dy.shape
    pb = (OH - 1) * stride + k - x.shape[1] - pad               # bottom / right zeros that make the output OH x OW
    cols = unfold_nhwc(x, k, stride, pad, pb)                   # [N, Cin*k*k, OH*OW]
    d = dy.double().reshape(N, OH * OW, Co)
    dw = torch.einsum("npo,nkp->ok", d, cols)
    A = torch.einsum("npo,nkp->ok", d.abs(), cols.abs())
    Cin = x.shape[3]
    return dw.reshape(Co, Cin, k, k), A.reshape(Co, Cin, k, k)


def attention_bwd_ref(qkv, do, heads, scale):
    """dqkv of plain softmax attention in fp64 under autograd; qkv [N, T, 3C] with heads as contiguous channel blocks."""
    N, T, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = (x[:, :, i * C:(i + 1) * C].reshape(N, T, heads, D).transpose(1, 2) for i in range(3))
    p = torch.softmax(scale * q @ k.transpose(-1, -2), dim=-1)
    o = (p @ v).transpose(1, 2).reshape(N, T, C)
    (o * do.double()).sum().backward()
    return x.grad, o.detach()


def groupnorm_bwd_ref(x, dy, gamma, beta, groups, eps, silu, scale_shift=None, add=None):
    """GroupNorm(+FiLM scale-shift)(+SiLU) backward in fp64 under autograd (F.group_norm), x / dy NHWC [N, H, W, C].
    -> (dx, dgamma, dbeta, d_scale_shift | None) and the magnitudes the bound scales with: A_dx, A_dgamma, A_dbeta, A_ss."""
    import torch.nn.functional as F
    N, H, W, C = x.shape
    xd = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    g = gamma.double().clone().requires_grad_(True)
    b = beta.double().clone().requires_grad_(True)
    ss = scale_shift.double().clone().requires_grad_(True) if scale_shift is not None else None
    y = F.group_norm(xd, groups, g, b, eps)
    if ss is not None:
        y = y * (1 + ss[:, :C, None, None]) + ss[:, C:, None, None]
    yo = y * torch.sigmoid(y) if silu else y
    dyd = dy.double().permute(0, 3, 1, 2)
    (yo * dyd).sum().backward()
    dx = xd.grad.permute(0, 2, 3, 1)
    if add is not None:
        dx = dx + add.double()
    # magnitudes: dyy = d loss / d (normalised, affine) value, xhat, rstd per (image, group)
    with torch.no_grad():
        xg = xd.detach().reshape(N, groups, -1)
        mean = xg.mean(-1, keepdim=True)
        var = xg.var(-1, unbiased=False, keepdim=True)
        rstd = (var + eps).rsqrt()
        kappa = 1 + (xg * xg).mean(-1, keepdim=True) / (var + eps)      # conditioning of the fp32 statistics
        xhat = ((xg - mean) * rstd).reshape(N, C, H, W)
        yn = xhat * g.detach()[None, :, None, None] + b.detach()[None, :, None, None]
        if ss is not None:
            y2 = yn * (1 + ss.detach()[:, :C, None, None]) + ss.detach()[:, C:, None, None]
        else:
            y2 = yn
        sg = torch.sigmoid(y2)
        dsil = sg * (1 + y2 * (1 - sg)) if silu else torch.ones_like(y2)
        dyy = (dyd * dsil).abs()                                         # |d loss / d y2|
        film = (1 + ss.detach()[:, :C, None, None]).abs() if ss is not None else 1.0
        gx = (dyy * film * g.detach().abs()[None, :, None, None]).reshape(N, groups, -1)
        xh = xhat.abs().reshape(N, groups, -1)
        A_dx = (rstd * kappa * (gx + gx.mean(-1, keepdim=True) + xh * (gx * xh).mean(-1, keepdim=True))).reshape(N, C, H, W)
        A_dx = A_dx.permute(0, 2, 3, 1)
        if add is not None:
            A_dx = A_dx + add.double().abs()
        A_db = (dyy * film).sum((0, 2, 3))
        A_dg = (dyy * film * xhat.abs() * kappa.repeat_interleave(C // groups, 1).reshape(N, C, 1, 1)).sum((0, 2, 3))
        A_ss = None
        if ss is not None:
            G0 = dyy.sum((2, 3))
            G1 = (dyy * yn.abs() * kappa.repeat_interleave(C // groups, 1).reshape(N, C, 1, 1)).sum((2, 3))
            A_ss = torch.cat([G1, G0], 1)
    return (dx, g.grad, b.grad, ss.grad if ss is not None else None), (A_dx, A_dg, A_db, A_ss)
