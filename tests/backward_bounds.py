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

    def row_blocks(self, name, got, ref, tol, rows):
        """rel-L2 per block with the row blocks given as slices: got / ref are [..., T, D]; every leading index and every
        slice of `rows` (over T) is one block.  The form for a ragged last block, which a reshape by T // rb cannot express."""
        got, ref = got.double(), ref.double()
        if got.shape != ref.shape:
            raise BoundError(f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}")
        if not torch.isfinite(got).all():
            raise BoundError(f"{name}: non-finite output")
        d = torch.stack([(got - ref)[..., s, :].flatten(-2).norm(dim=-1) for s in rows], -1)
        n = torch.stack([ref[..., s, :].flatten(-2).norm(dim=-1) for s in rows], -1) + 1e-300
        r = d / n / tol
        worst = float(r.max())
        self._note(name, worst)
        if worst > 1.0:
            idx = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape))
            raise BoundError(f"{name}: block {idx} (rows {rows[idx[-1]]}) rel-L2 {worst * tol:.3g} > {tol:.3g} "
                             f"({int((r > 1).sum())} of {r.numel()} blocks out of bound)")
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
        # magnitude of SiLU's derivative s (1 + y (1 - s)) as the fp32 evaluation sees it: the sum of its absolute terms
        # s (1 + |y| (1 - s)), as silu_bwd_ref takes it.  The derivative crosses zero at y = -1.278, and the evaluation's error
        # there is a few u32 of s (1 + |y| (1 - s)), not of the cancelled result; with |s (1 + y (1 - s))| in its place a sum of
        # ONE term (a 1x1 map's per-image FiLM gradient) has no room for it.  The two agree for y >= 0.
        dsil = sg * (1 + y2.abs() * (1 - sg)) if silu else torch.ones_like(y2)
        dyy = dyd.abs() * dsil                                           # |d loss / d y2|
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
            # d scale = sum dyy (xhat gamma + beta): the terms' magnitudes |xhat gamma| + |beta|, not |xhat gamma + beta| (the two
            # can cancel, and a 1x1 map sums one such term)
            ynm = xhat.abs() * g.detach().abs()[None, :, None, None] + b.detach().abs()[None, :, None, None]
            G1 = (dyy * ynm * kappa.repeat_interleave(C // groups, 1).reshape(N, C, 1, 1)).sum((2, 3))
            A_ss = torch.cat([G1, G0], 1)
    return (dx, g.grad, b.grad, ss.grad if ss is not None else None), (A_dx, A_dg, A_db, A_ss)


# ------------------------------------------------------------------------------------------ ops outside the original ten
def silu_bwd_ref(pre, g):
    """g * s (1 + x (1 - s)), s = sigmoid(x), in fp64, and the magnitude A of its fp32 bound |got - ref| <= 16 u32 A.
    ops.silu_bwd evaluates the expression in fp32: s to <= 4 u32 (exp, add, divide), 1 - s to 5 u32 absolute, x (1 - s) to
    6 u32 |x|, 1 + x (1 - s) to 7 u32 (1 + |x|), its product with s to 12 u32 (1 + |x|) (s <= 1, |1 + x (1 - s)| <= 1 + |x|),
    and the product with g adds one rounding: 13 u32 |g| (1 + |x|), rounded up to c = 16 with A = |g| (1 + |x|)."""
    x, gd = pre.double(), g.double()
    s = torch.sigmoid(x)
    return gd * s * (1 + x * (1 - s)), gd.abs() * (1 + x.abs())


def dropout_keep(shape_nhwc, p, seed, device):
    """The counter hash of dxmi_dropout_bf16 restated in torch int64 on `device`: keep(i) = (mix32(i ^ seed) >> 8) >= p 2^24
    over the NHWC linear index i (oracle.unet_small.dropout_keep_mask states the same hash in numpy; the two are compared on
    the host by test_backward_bounds.py).  -> bool tensor of shape_nhwc."""
    n = math.prod(shape_nhwc)
    m = 0xFFFFFFFF
    h = torch.arange(n, dtype=torch.int64, device=device) ^ (int(seed) & m)
    h = h ^ (h >> 16)
    h = (h * 0x7feb352d) & m
    h = h ^ (h >> 15)
    h = (h * 0x846ca68b) & m
    h = h ^ (h >> 16)
    return ((h >> 8) >= int(float(p) * 16777216.0)).reshape(shape_nhwc)


def dropout_ref(x, p, seed):
    """bf16(x / (1 - p)) computed in fp64 where kept, 0 elsewhere.  The kernel multiplies by the fp32 scalar 1 / (1 - p); where
    the fp64 quotient lies within 4 u32 of a bf16 rounding midpoint either neighbour is accepted (mask `tie`)."""
    keep = dropout_keep(tuple(x.shape), p, seed, x.device)
    q = x.double() / (1.0 - float(p))
    b = q.to(torch.bfloat16)
    e = torch.floor(torch.log2(b.double().abs().clamp_min(1e-38)))
    tie = ((q - b.double()).abs() - 2.0 ** (e - 8)).abs() <= 4 * U32 * q.abs() + 1e-300
    return keep, torch.where(keep, b, torch.zeros_like(b)), tie & keep


def value_head_bwd_ref(feat, w, dy):
    """fp64 autograd through y[n] = sum_c w[c] sum_hw relu(feat[n, hw, c]) (the expressions of
    test_hip_backward.py::test_colsum_and_pool_bwd_and_head_bwd: F.relu, whose derivative at exactly 0 is 0 as the kernel's
    `v > 0` is; clamp_min's is 1 there, and a randn draw that is exactly 0 does occur in these batches)
    -> (dfeat, s = the relu-sum features, sum |relu| for s)."""
    f = feat.double().clone().requires_grad_(True)
    s = torch.relu(f).sum((1, 2))
    ((s @ w.double()) * dy.double()).sum().backward()
    return f.grad, s.detach(), feat.double().clamp_min(0).sum((1, 2))


def value_head_pgrad_ref(s, w, b, dy, ow):
    """fp64 autograd through y = (s . w + b) ow + ob -> [C + 3] = d w | d b | d ow | d ob (zeros for the last two without
    out_scale), and the sums of absolute terms A of the same layout.  The kernel's sums over the N images have depth N, the
    dot product s[n] . w depth C: c = N + C + 8 covers both and the scalar products."""
    sd, dyd = s.double(), dy.double()
    wd = w.double().clone().requires_grad_(True)
    bd = b.double().clone().requires_grad_(True)
    owd = (ow.double().reshape(()) if ow is not None else torch.ones((), dtype=torch.float64, device=s.device)).clone().requires_grad_(True)
    obd = torch.zeros((), dtype=torch.float64, device=s.device, requires_grad=True)
    y = (sd @ wd + bd) * owd + obd
    (y * dyd).sum().backward()
    z = torch.zeros(1, dtype=torch.float64, device=s.device)
    ref = torch.cat([wd.grad, bd.grad.reshape(1), owd.grad.reshape(1) if ow is not None else z, obd.grad.reshape(1) if ow is not None else z])
    sc = owd.detach().abs()
    pre = sd.abs() @ wd.detach().abs() + bd.detach().abs()
    A = torch.cat([(dyd.abs()[:, None] * sc * sd.abs()).sum(0), (dyd.abs() * sc).sum().reshape(1),
                   (dyd.abs() * pre).sum().reshape(1) if ow is not None else z, dyd.abs().sum().reshape(1) if ow is not None else z])
    return ref, A


def td_loss_ref(v, cost, extra):
    """mse(v[B:], v[:B] + extra) in fp64 under autograd -> (d loss / d v [2B], logs [3], A_grad, A_logs).  The kernel's three
    means are sums of depth B (any order) of terms evaluated with <= 4 roundings: c = B + 8."""
    B = cost.numel()
    vd = v.double().clone().requires_grad_(True)
    ex = extra.double() if extra is not None else 0.0
    target = (vd[:B] + ex).detach()
    d = vd[B:] - target
    loss = (d * d).mean()
    loss.backward()
    logs = torch.stack([loss.detach(), vd[B:].detach().mean(), cost.double().mean()])
    mag = vd[B:].detach().abs() + vd[:B].detach().abs() + (extra.double().abs() if extra is not None else 0.0)
    A_grad = torch.cat([torch.zeros(B, dtype=torch.float64, device=v.device), 2 * mag / B])
    A_logs = torch.stack([(mag * mag).mean(), vd[B:].detach().abs().mean(), cost.double().abs().mean()])
    return vd.grad, logs, A_grad, A_logs


def dsm_loss_bwd_ref(e, Me, c_out, gm, gx, w):
    """d(model_out) = 2 e a c_out of the DSM terms, a = g_mse w / CHW + g_xs / CHW per sample (either gradient may be None), and
    the product of the factors' absolute terms: fl(e) carries 16 u32 Me (forward_bounds.dsm_error_terms), a and c_out <= 8 u32
    each, two products: |got - ref| <= 16 u32 A covers them only together with the factor 2 kept in A = 2 Me Ma |c_out|."""
    CHW = e.shape[1]
    z = torch.zeros(e.shape[0], 1, dtype=torch.float64, device=e.device)
    a = (gm.double()[:, None] / CHW * w[:, None] if gm is not None else z) + (gx.double()[:, None] / CHW if gx is not None else z)
    Ma = (gm.double().abs()[:, None] / CHW * w[:, None] if gm is not None else z) + (gx.double().abs()[:, None] / CHW if gx is not None else z)
    return 2 * e * a * c_out, 2 * Me * Ma * c_out.abs()


def var_step_bwd_ref(g_next, g_mean, g_control, g_logp, z, cm, sg):
    """Gradients of the VAR transition w.r.t. eps and sigma by fp64 autograd through the expressions of
    test_hip_round5_kernels.py::test_var_and_edm_step_backward_vs_torch_autograd (x' detached inside the log-prob), [N, CHW]
    tensors and per-sample [N] scalars; any incoming gradient may be None.  -> (d_eps, d_sigma, A_eps, A_sigma).
    d_eps = cm (g_x' + g_mean + g_control + g_logp z / (sg CHW)): four fp32 terms and a product, 8 u32 A_eps.
    d_sigma = sum_CHW g_x' z + g_logp (mean z^2 - 1) / sg: two sums of depth CHW in any order, (CHW + 8) u32 A_sigma with
    A_sigma = sum |g_x' z| + |g_logp| (mean z^2 + 1) / sg."""
    import math
    N, CHW = z.shape
    e = lambda v: v[:, None]
    zd, cmd = z.double(), cm.double()
    eps = torch.zeros(N, CHW, dtype=torch.float64, device=z.device, requires_grad=True)      # linear in eps: any point serves
    sgd = sg.double().clone().requires_grad_(True)
    control = e(cmd) * eps
    mean = control                                       # the xm x term has no gradient w.r.t. eps or sigma
    xn = mean + e(sgd) * zd
    lp = (-((xn.detach() - mean) ** 2) / (2 * e(sgd) ** 2) - torch.log(e(sgd)) - math.log(math.sqrt(2 * math.pi))).mean(1)
    loss = 0
    zero = torch.zeros(N, CHW, dtype=torch.float64, device=z.device)
    for out, g in ((xn, g_next), (mean, g_mean), (control, g_control), (lp, g_logp)):
        if g is not None:
            loss = loss + (out * g.double()).sum()
    loss.backward()
    ab = lambda g: zero if g is None else g.double().abs()
    gl = torch.zeros(N, dtype=torch.float64, device=z.device) if g_logp is None else g_logp.double().abs()
    sd_ = sg.double()
    A_eps = e(cmd.abs()) * (ab(g_next) + ab(g_mean) + ab(g_control) + e(gl / (sd_ * CHW)) * zd.abs())
    A_sig = (ab(g_next) * zd.abs()).sum(1) + gl * ((zd ** 2).mean(1) + 1) / sd_
    return eps.grad, sgd.grad, A_eps, A_sig


def edm_step_bwd_ref(g_sample, g_mean, z, sigma, sdn, sd=0.5):
    """Gradients of the EDM transition w.r.t. the network output F and sigma_up by fp64 autograd through
    mu = x + (x - c_out F - c_skip x) / sigma (sigma_down - sigma), x' = mu + z sigma_up (x = 0: it has no part in either
    gradient).  d_F = -(c_out (sigma_down - sigma) / sigma) (g_x' + g_mu): the coefficient carries <= 12 u32, one sum, one
    product: 16 u32 A_F.  d_sigma_up = sum_CHW g_x' z: depth CHW, (CHW + 8) u32 sum |g_x' z|."""
    N, CHW = z.shape
    e = lambda v: v.double()[:, None]
    s = sigma.double()
    c_out = (s * sd / (s ** 2 + sd ** 2) ** 0.5)[:, None]
    F = torch.zeros(N, CHW, dtype=torch.float64, device=z.device, requires_grad=True)
    up = torch.ones(N, dtype=torch.float64, device=z.device, requires_grad=True)
    mu = (0 - c_out * F) / e(sigma) * (e(sdn) - e(sigma))
    smp = mu + z.double() * up[:, None]
    zero = torch.zeros(N, CHW, dtype=torch.float64, device=z.device)
    gs = zero if g_sample is None else g_sample.double()
    gm = zero if g_mean is None else g_mean.double()
    ((smp * gs).sum() + (mu * gm).sum()).backward()
    coef = (c_out * (e(sdn) - e(sigma)) / e(sigma)).abs()
    return F.grad, up.grad, coef * (gs.abs() + gm.abs()), (gs.abs() * z.double().abs()).sum(1)


# ------------------------------------------------------------------------------------------ judged launches
# One definition of each judged launch: test_hip_backward_shapes.py (the program shapes) and the off-program edge tests call
# these, so a launch is judged the same way wherever it is made.  EDGE collects the edge tests' worst |err| / bound.
EDGE = Checker()


def wgrad_checked(ops, x0, dy, k, check=None, *, in1=None, pad=None, stride=1, upsample=False, with_bias=False, old=None, tag=None):
    """ops._conv2d_wgrad(x0, dy, k, ...) judged element by element: dW within wgrad_depth(plan) * u32 * sum|dy||x| of
    wgrad_ref on the same operands (db, with_bias, against the column sums of dy at the same depth), tagged
    wgrad[family/reduce] unless `tag` is given.  accumulate=True into a copy of the result must give bitwise twice it.
    old: an fp32 tensor of dW's shape; accumulate=True into a copy of it is judged against old + dW with A + |old| at the same
    depth (the + 2 of wgrad_depth counts that add).  -> (dw, db | None, plan)."""
    check = EDGE if check is None else check
    N, IH, IW, C0 = x0.shape
    C1 = in1.shape[3] if in1 is not None else 0
    _, OH, OW, Co = dy.shape
    if pad is None:
        pad = k // 2
    plan = ops.conv2d_wgrad_plan(N, IH, IW, OH, OW, C0, C1, Co, k, stride, pad, upsample)
    c = wgrad_depth(plan)
    xc = torch.cat([x0, in1], 3) if C1 else x0
    ref, A = wgrad_ref(xc, dy, k, stride, pad, int(bool(upsample)))
    tag = tag or f"wgrad[{plan['family']}/{plan['reduce']}]"
    kw = dict(in1=in1, pad=pad, stride=stride, upsample=bool(upsample))
    db = None
    if with_bias:
        dw, db = ops._conv2d_wgrad(x0, dy, k, with_bias=True, **kw)
        d = dy.double().reshape(-1, Co)
        check.fp32("wgrad_db", db, d.sum(0), d.abs().sum(0), c)
    else:
        dw = ops._conv2d_wgrad(x0, dy, k, **kw)
    check.fp32(tag, dw, ref, A, c)
    acc = dw.clone()
    ops._conv2d_wgrad(x0, dy, k, out=acc, accumulate=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(acc, dw * 2), "accumulate=True is not bitwise 2x the first result"
    if old is not None:
        acc = old.clone()
        ops._conv2d_wgrad(x0, dy, k, out=acc, accumulate=True, **kw)
        check.fp32(tag + "+old", acc, old.double() + ref, A + old.double().abs(), c)
    return dw, db, plan


def gn_bwd_checked(ops, op, form, x0, dy, gamma, beta, check=None, *, in1=None, add0=None, add1=None, groups=32, eps, silu=True,
                   scale_shift=None, fwd_stats=None):
    """ops.groupnorm_generic_bwd / ops.groupnorm_silu_bwd (op) judged against groupnorm_bwd_ref: dx (both concat sources,
    fused adds) with Checker.bf16 at c = H W cpg + 16, dgamma / dbeta at N H W + 16, the FiLM gradient at H W + 16; tagged
    <op>[<form>]_dx ... (form: resident, two-launch, one-launch).  -> (dx0, dx1, dgamma, dbeta, d_scale_shift | None)."""
    check = EDGE if check is None else check
    N, H, W, C0 = x0.shape
    c1 = in1.shape[3] if in1 is not None else 0
    C = C0 + c1
    kw = dict(in1=in1, add0=add0, add1=add1, groups=groups, eps=eps, silu=silu)
    if op == "groupnorm_generic_bwd":
        dx0, dx1, dg, db, dss = ops.groupnorm_generic_bwd(x0, dy, gamma, beta, scale_shift=scale_shift, fwd_stats=fwd_stats, **kw)
    else:
        assert op == "groupnorm_silu_bwd" and scale_shift is None and fwd_stats is None
        dx0, dx1, dg, db = ops.groupnorm_silu_bwd(x0, dy, gamma, beta, **kw)
        dss = None
    xc = torch.cat([x0, in1], 3) if c1 else x0
    addc = None
    if add0 is not None or add1 is not None:
        addc = torch.cat([add0 if add0 is not None else torch.zeros_like(x0), add1 if add1 is not None else torch.zeros_like(in1)], 3) \
            if c1 else add0
    (rdx, rdg, rdb, rdss), (Adx, Adg, Adb, Ass) = groupnorm_bwd_ref(xc, dy, gamma, beta, groups, eps, silu, scale_shift=scale_shift, add=addc)
    cpg = C // groups
    tag = f"{op}[{form}]"
    dx = torch.cat([dx0, dx1], 3) if c1 else dx0
    check.bf16(tag + "_dx", dx, rdx, Adx, H * W * cpg + 16)
    check.fp32(tag + "_dgamma", dg, rdg, Adg, N * H * W + 16)
    check.fp32(tag + "_dbeta", db, rdb, Adb, N * H * W + 16)
    if scale_shift is not None:
        check.fp32(tag + "_dscale_shift", dss, rdss, Ass, H * W + 16)
    return dx0, dx1, dg, db, dss


ATTN_TOL = 8 * U16


def attn_row_slices(T, rb=128):
    return [slice(r, min(r + rb, T)) for r in range(0, T, rb)]


def attention_blocks_judge(check, name, got, ref, heads, tol=ATTN_TOL):
    """dqkv [N, T, 3C] per (image, q|k|v, head, 128-row block) within rel-L2 `tol`; the last block is ragged when T % 128 != 0."""
    N, T, C3 = got.shape
    D = C3 // 3 // heads
    rb = 128 if T >= 128 else T
    if T % rb == 0:
        blk = lambda d: d.reshape(N, T // rb, rb, 3, heads, D).permute(0, 3, 4, 1, 2, 5)
        return check.blocks(name, blk(got), blk(ref), tol, 4)
    blk = lambda d: d.reshape(N, T, 3, heads, D).permute(0, 2, 3, 1, 4)
    return check.row_blocks(name, blk(got), blk(ref), tol, attn_row_slices(T, rb))


def attention_bwd_checked(ops, qkv, do, heads, scale, check=None, *, o=None, lse=None, ref=None, tag=None):
    """ops.attention_bwd(qkv, do, heads, scale, o=o, lse=lse) judged per (image, q|k|v, head, 128-row block) within rel-L2
    8 u16 of attention_bwd_ref (P and dS are bf16 MFMA operands in the kernels, so the bound is per block at the kernel's tile
    size rather than per element).  ref: attention_bwd_ref's result when the caller already has it.  -> (dqkv, ref)."""
    check = EDGE if check is None else check
    N, T, C3 = qkv.shape
    if ref is None:
        ref = attention_bwd_ref(qkv, do, heads, scale)
    got = ops.attention_bwd(qkv, do, heads, scale, o=o, lse=lse)
    tag = tag or f"attention_bwd[T{T},h{heads}{',lse' if lse is not None else ''}]"
    attention_blocks_judge(check, tag, got, ref[0], heads)
    return got, ref


def softmax_bwd_ref(S, dP):
    """P = softmax(S), dS = P (dP - sum_k dP_k P_k) per row in fp64, and each row's largest term: max_j P_j for P, and
    max_j P_j (|dP_j| + sum_k |dP_k| P_k) for dS (the magnitude the fp32 evaluation's absolute error scales with)."""
    s, g = S.double(), dP.double()
    P = torch.softmax(s, -1)
    dot = (g * P).sum(-1, keepdim=True)
    dS = P * (g - dot)
    mP = P.amax(-1, keepdim=True)
    mS = (P * (g.abs() + (g.abs() * P).sum(-1, keepdim=True))).amax(-1, keepdim=True)
    return P, dS, mP, mS


def gn_resident_plan(C0, C1, HW, groups):
    """The slicing walk of the register-resident GroupNorm backward (gn_plan in csrc/groupnorm.hip with its limits of 8 / 16
    pieces per thread) restated, so a test can say which of its paths a shape takes -> dict(VEC, slices, threads, pieces, ppp)
    or None where the walk fails; whether the kernel serves the shape is asked of dxmi_groupnorm_silu_bwd_supported."""
    C = C0 + C1
    cpg = C // groups
    VEC = 8 if (cpg % 8 == 0 and C0 % 8 == 0) else 4
    max_pieces = 8 if VEC == 8 else 16
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
            return dict(VEC=VEC, slices=slices, threads=threads, pieces=pieces, ppp=ppp)
        slices *= 2
