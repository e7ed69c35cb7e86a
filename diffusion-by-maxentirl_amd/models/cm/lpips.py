"""LPIPS on VGG16 (piq's `LPIPS(replace_pooling=True, reduction="none")`), the `lpips` loss norm of the consistency losses
(reference models/cm/karras_diffusion.py:221-234; the reference's own import of piq is commented out, :10, so there is no
reference run to pin parity to: DESIGN 5.15).

    lpips(x, y), x, y [N, 3, H, W] in [0, 1] -> [N]
      z = (x - mean) / std; torchvision VGG16 `features` with AvgPool2d(2, 2, 0) in place of the max pools; the taps relu1_2,
      relu2_2, relu3_3, relu4_3, relu5_3, each normalised per pixel f / (sqrt(sum_c f^2) + 1e-10);
      sum over the taps of mean_hw sum_c w_k[c] (fx - fy)^2.

No weights ship with this package: the caller supplies torchvision's VGG16 state dict and piq's five linear weights,
directly, as two files, or through DXMI_LPIPS_VGG16 / DXMI_LPIPS_LIN.

CPU tensors (or a y that requires grad) take the torch fp32 expressions under autograd.  Device tensors take the HIP path: ONE
autograd node that differentiates x only; online and target images ride one stacked [2 N] batch through the 13 convolutions
(ops.gconv), the backward runs the data-gradient convolutions (ops.gconv on transposed-and-flipped packed weights) on the online
half, with the launches of dxmi_hip.lpips_ops between them."""
import os

import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
GROUPS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))      # positions in CONV_INDICES; a 2x2 average pool between groups
TAP_WIDTHS = (64, 128, 256, 512, 512)
EPS = 1e-10
ENV_VGG16, ENV_LIN = "DXMI_LPIPS_VGG16", "DXMI_LPIPS_LIN"


def _load_file(path):
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except TypeError:      # a torch without weights_only
        return torch.load(path, map_location="cpu")


def tap_distance(fx, fy, w):
    """fx, fy [N, C, h, w], w [C] -> [N]: both maps normalised per pixel, f / (sqrt(sum_c f^2) + 1e-10), then
    mean_hw sum_c w_c (fx - fy)^2.  vector_norm is sqrt(sum f^2) with a backward of 0 (not NaN) at an all-zero pixel."""
    fx = fx / (torch.linalg.vector_norm(fx, dim=1, keepdim=True) + EPS)
    fy = fy / (torch.linalg.vector_norm(fy, dim=1, keepdim=True) + EPS)
    return ((fx - fy) ** 2 * w.view(1, -1, 1, 1)).mean(dim=(2, 3)).sum(dim=1)


def _lpips_forward(lp, xy, resize, scale=None, keep=False):
    """xy fp32 [2 N, 3, H, W]: the online images then the targets -> (value fp32 [N], times scale[N] if given; what the backward
    needs if `keep`, else None).  Kept per convolution: the stacked [2 N] activation at the five taps (the tap gradient reads both
    halves), a copy of the online half elsewhere, so the target half of those eight is freed as soon as the next layer has read it."""
    from dxmi_hip import lpips_ops as lo
    from dxmi_hip import ops
    N = xy.shape[0] // 2
    fw, _, lin = lp._device_weights(xy.device)
    h = lo.front_fwd(xy, resize)
    acts, out = [] if keep else None, None
    for gi, group in enumerate(GROUPS):
        for l in group:
            h = ops.gconv(h, fw[l], pad=(1, 1), relu=True)
            if keep:
                acts.append(h if l == group[-1] else h[:N].clone())
        out = lo.tap_fwd(h[:N], h[N:], lin[gi], out=out, scale=scale if gi == len(GROUPS) - 1 else None)
        if gi < len(GROUPS) - 1:
            h = lo.avgpool2x2(h)
    return out, acts


class _LPIPSFn(torch.autograd.Function):
    """front end -> 13 x (conv + ReLU), 4 pools, 5 tap distances on the stacked batch, as one node; d x only."""

    @staticmethod
    def forward(ctx, lp, x, y, resize):
        out, acts = _lpips_forward(lp, torch.cat([x, y], 0), resize, keep=True)
        ctx.lp, ctx.acts, ctx.hw = lp, acts, tuple(x.shape[2:])
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 4
        dx = _lpips_backward(ctx.lp, ctx.acts, ctx.hw, g.detach().float().contiguous())
        ctx.acts = None
        return None, dx, None, None


def _lpips_backward(lp, acts, hw, g):
    """d x fp32 [N, 3, H, W] for the upstream g fp32 [N] (None: ones) from the 13 activations _lpips_forward kept."""
    from dxmi_hip import lpips_ops as lo
    from dxmi_hip import ops
    N = acts[0].shape[0]
    _, bw, lin = lp._device_weights(acts[0].device)
    ga = None
    for gi in reversed(range(len(GROUPS))):
        group = GROUPS[gi]
        for l in reversed(group):
            a, acts[l] = acts[l], None      # each activation is dropped once its layer's gradient is formed
            gt = lo.tap_bwd(g, a[:N], a[N:], lin[gi]) if l == group[-1] else None
            gm = lo.relu_mask_acc(ga, gt, a[:N]) if ga is not None else lo.relu_mask_acc(gt, None, a[:N])
            out = None
            if l == 0:      # 3 gradient channels in the front end's 16-channel layout
                out = torch.zeros(gm.shape[:3] + (16,), dtype=torch.bfloat16, device=gm.device)
            ga = ops.gconv(gm, bw[l], pad=(1, 1), relu=False, out=out)
        if gi > 0:
            prev = acts[GROUPS[gi - 1][-1]]
            ga = lo.avgpool2x2_bwd(ga, prev.shape[1], prev.shape[2])
        del a, gt, gm
    return lo.front_bwd(ga, *hw)


class LPIPS:
    def __init__(self, vgg_state_dict, lin_weights, replace_pooling=True, reduction="none"):
        if not replace_pooling:
            raise NotImplementedError("LPIPS: only replace_pooling=True (average pools) is implemented")
        if reduction != "none":
            raise NotImplementedError(f"LPIPS: only reduction='none' (one value per sample) is implemented, got {reduction!r}")
        self.convs = []
        for idx, (cin, cout) in zip(CONV_INDICES, zip((3,) + CONV_WIDTHS[:-1], CONV_WIDTHS)):
            w, b = (self._entry(vgg_state_dict, idx, k) for k in ("weight", "bias"))
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f"LPIPS: VGG16 features.{idx} has weight {tuple(w.shape)} / bias {tuple(b.shape)}, expected "
                                 f"{(cout, cin, 3, 3)} / {(cout,)}")
            self.convs.append((w.detach().float().contiguous(), b.detach().float().contiguous()))
        lin = list(lin_weights.values()) if isinstance(lin_weights, dict) else list(lin_weights)
        if len(lin) != len(TAP_WIDTHS):
            raise ValueError(f"LPIPS: {len(lin)} linear weights, expected {len(TAP_WIDTHS)}")
        self.lin = []
        for k, (w, c) in enumerate(zip(lin, TAP_WIDTHS)):
            w = torch.as_tensor(w)
            if w.numel() != c or tuple(w.shape) not in ((1, c, 1, 1), (c,)):
                raise ValueError(f"LPIPS: linear weight {k} has shape {tuple(w.shape)}, expected {(1, c, 1, 1)}")
            self.lin.append(w.detach().float().reshape(c).contiguous())
        self._dev = None

    @staticmethod
    def _entry(sd, idx, kind):
        for key in (f"features.{idx}.{kind}", f"{idx}.{kind}"):
            if key in sd:
                return torch.as_tensor(sd[key])
        raise ValueError(f"LPIPS: the VGG16 state dict has neither features.{idx}.{kind} nor {idx}.{kind}")

    @classmethod
    def from_files(cls, vgg_path, lin_path, **kw):
        return cls(_load_file(vgg_path), _load_file(lin_path), **kw)

    @classmethod
    def from_env(cls, **kw):
        vgg, lin = os.environ.get(ENV_VGG16), os.environ.get(ENV_LIN)
        if not vgg or not lin:
            return None
        return cls.from_files(vgg, lin, **kw)

    def _device_weights(self, device):
        """(forward packs, data-gradient packs, lin weights) on `device`: packed on the first call and kept for the device used
        last, so an object moved between devices holds one set of packs (about 59 MB), not one per device."""
        key = str(device)
        if self._dev is None or self._dev[0] != key:
            from dxmi_hip import ops
            fw, bw = [], []
            for w, b in self.convs:
                w = w.to(device)
                fw.append(ops.gconv_pack(w, bias=b))
                bw.append(ops.gconv_pack(w.transpose(0, 1).flip(2, 3)))
            self._dev = (key, (fw, bw, [w.to(device) for w in self.lin]))
        return self._dev[1]

    # ------------------------------------------------------------------------------------------------ torch path
    def features(self, x):
        """The five taps (before the per-pixel normalisation) of x [N, 3, H, W] in [0, 1] (torch, the dtype and device of x)."""
        mean = torch.tensor(MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
        std = torch.tensor(STD, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
        h = (x - mean) / std
        taps = []
        for gi, group in enumerate(GROUPS):
            if gi:
                h = F.avg_pool2d(h, 2, 2, 0)
            for l in group:
                w, b = self.convs[l]
                h = F.relu(F.conv2d(h, w.to(x), b.to(x), padding=1))
            taps.append(h)
        return taps

    def _torch(self, x, y, resize):
        if resize is not None:
            x = F.interpolate(x, size=resize, mode="bilinear")
            y = F.interpolate(y, size=resize, mode="bilinear")
        total = 0
        for fx, fy, w in zip(self.features(x), self.features(y), self.lin):
            total = total + tap_distance(fx, fy, w.to(fx))
        return total

    def _check(self, x, y):
        if x.dim() != 4 or x.shape[1] != 3 or x.shape != y.shape:
            raise ValueError(f"LPIPS: x {tuple(x.shape)} and y {tuple(y.shape)} must be two [N, 3, H, W] batches of one shape")

    def __call__(self, x, y, resize=None):
        self._check(x, y)
        if not x.is_cuda:
            return self._torch(x.float(), y.float(), resize)
        if y.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("LPIPS on the device differentiates x only: y must not require grad")
        return self.device_value(x, y, resize)

    def device_value(self, x, y, resize=None):
        from dxmi_hip import graph as _graph
        if _graph.current() is not None:
            raise NotImplementedError("LPIPS: capture into a hipGraph is not supported")
        x32, y32 = x.float().contiguous(), y.detach().float().contiguous()
        if resize is not None and not isinstance(resize, int):
            resize = tuple(resize)
        if torch.is_grad_enabled() and x.requires_grad:
            return _LPIPSFn.apply(self, x32, y32, resize)
        with torch.no_grad():
            return _lpips_forward(self, torch.cat([x32, y32], 0), resize)[0]
