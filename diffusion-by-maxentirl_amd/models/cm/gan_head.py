"""The classifier head of DMD2's GAN term (Yin et al. 2024, "Improved Distribution Matching Distillation for Fast Image Synthesis",
section 4.3; the layout and key names of its released ImageNet-64 `cls_pred_branch`): a small classifier on the fake denoiser's
bottleneck features, trained with the fake denoiser to tell noised real images from noised generated ones.

    Conv2d(C, C, 4, stride 2, pad 1) - GroupNorm(groups, C) - SiLU - Conv2d(C, C, map/2, stride map/2) - GroupNorm - SiLU - Conv2d(C, 1, 1)

GANHead is a parameter container like the project's other modules.  On CPU tensors forward() is plain torch on an NCHW input: the
torch path of the losses, and what the host tests hold against float64.  On the device it takes the NHWC bf16 bottleneck of
models.cm.unet_train.encoder_forward and every product, norm and activation is a HIP launch; between them stands torch glue on small
tensors (dtype casts, the slab sum of the split-K linear, the bias gradient's column sum, the re-ordering of conv 3's weight gradient):
    conv 0      dxmi_gan_conv4s2_fwd / _dgrad / _wgrad (csrc/gan_head.hip), packs cached through dxmi_hip.packs.WeightPacks
    norms       dxmi_groupnorm_generic_fwd / _bwd_saved at HW = (map/2)^2 and HW = 1
    conv 3      the whole remaining map -> 1x1 is a dense layer [N, (map/2)^2 C] -> C: dxmi_linear_splitk on the weight re-ordered to
                (kh, kw, Cin) columns, dxmi_linear_* and the 1x1 pixel-GEMM weight gradient backward
    conv 6      dxmi_gan_logit_loss_fwd / _bwd: the C -> 1 product fused with the per-sample softplus(sign logit)
It offers the pieces of the tape API: features() with its saved tensors, logit_loss(), and backward() in a full (parameter gradients
and d_h) and an input-only (d_h alone) form; the two give the same d_h bit for bit.
"""
import torch
import torch.nn as nn

from dxmi_hip import ops
from dxmi_hip.packs import PackedWeights, WeightPacks

MAP_SIZES = (4, 8)
_WGRAD_COLS = 2048      # columns of the dense layer's weight gradient per pixel-GEMM launch


def _build_packs(head, ps):
    b = head.cls_pred_branch
    w0, w3 = b[0].weight, b[3].weight
    ps.derived("c0", lambda out: ops.gan_conv4s2_pack(w0, out=out))
    C, k = w3.shape[0], w3.shape[2]
    # the dense form of the whole-map conv: columns in the (kh, kw, Cin) order of the flattened NHWC map
    rows = ps.stage((C, k * k * C), lambda out: out.view(C, k, k, C).copy_(w3.detach().permute(0, 2, 3, 1)))
    ps.pack("c3", rows)
    ps.pack("c3_t", rows, transpose_flip=True)


class GANHead(PackedWeights, nn.Module):
    def __init__(self, channels, map_size, groups=32):
        super().__init__()
        if map_size not in MAP_SIZES:
            raise ValueError(f"GANHead: map_size must be one of {MAP_SIZES} (the bottleneck of the EDM nets), got {map_size!r}")
        if channels % groups:
            raise ValueError(f"GANHead: {channels} channels do not divide into {groups} groups")
        self.channels, self.map_size, self.groups = int(channels), int(map_size), int(groups)
        C, k = self.channels, self.map_size // 2
        self.cls_pred_branch = nn.Sequential(
            nn.Conv2d(C, C, 4, 2, 1), nn.GroupNorm(groups, C), nn.SiLU(),
            nn.Conv2d(C, C, k, k, 0), nn.GroupNorm(groups, C), nn.SiLU(),
            nn.Conv2d(C, 1, 1, 1, 0))
        self._packs = WeightPacks(self, _build_packs)

    def _check_map(self, h):
        C, m = self.channels, self.map_size
        ops.gan_head_supported(C, m)
        if h.dtype != torch.bfloat16 or h.dim() != 4 or tuple(h.shape[1:]) != (m, m, C):
            raise ValueError(f"GANHead on the device takes the NHWC bf16 bottleneck [N, {m}, {m}, {C}], got {tuple(h.shape)} {h.dtype}")

    def forward(self, h):
        """-> logits [N] fp32.  CPU: h NCHW, plain torch.  Device: h NHWC bf16, the HIP launches."""
        if not h.is_cuda:
            return self.cls_pred_branch(h).reshape(h.shape[0]).float()
        a2, _ = self.features(h)
        return self.logit_loss(a2, torch.ones(h.shape[0], dtype=torch.float32, device=h.device))[0]

    # ---- the device pieces
    def features(self, h):
        """h NHWC bf16 [N, map, map, C] -> (a2 bf16 [N, C], saved): the second SiLU's output and what backward() reads."""
        self._check_map(h)
        b, pk, N, C, G = self.cls_pred_branch, self.packed(), h.shape[0], self.channels, self.groups
        h = h.contiguous()
        y1 = ops.gan_conv4s2_fwd(h, pk["c0"], b[0].bias)
        s1, s2 = [], []
        a1 = ops.groupnorm_generic(y1, b[1].weight, b[1].bias, groups=G, eps=b[1].eps, silu=True, saved=s1)
        x2 = a1.view(N, -1).float()
        y2 = ops.linear(x2, pk["c3"], b[3].bias, splitk=True).to(torch.bfloat16).view(N, 1, 1, C)
        a2 = ops.groupnorm_generic(y2, b[4].weight, b[4].bias, groups=G, eps=b[4].eps, silu=True, saved=s2)
        return a2.view(N, C), (h, y1, s1[0], x2, y2, s2[0], a2)

    def logit_loss(self, a2, sign):
        """-> (logit [N], softplus(sign logit) [N]) for sign fp32 [N] of -1 / +1, in one launch."""
        b = self.cls_pred_branch
        return ops.gan_logit_loss_fwd(a2, b[6].weight.detach().reshape(-1), b[6].bias.detach(), sign)

    def backward(self, saved, sign, logit, upstream, weight=1.0, params=True):
        """The backward of sum_n upstream_n weight softplus(sign_n logit_n) -> (d_h NHWC bf16, gradients in self.parameters() order |
        None).  params=False: the input-only form, no weight or bias gradient of a conv is launched."""
        h, y1, s1, x2, y2, s2, a2 = saved
        b, pk, N, C, G = self.cls_pred_branch, self.packed(), h.shape[0], self.channels, self.groups
        k = self.map_size // 2
        d_a2, dw6, db6 = ops.gan_logit_loss_bwd(a2.view(N, C), b[6].weight.detach().reshape(-1), sign, logit, upstream, weight, params)
        d_y2, _, dg4, dbt4, _ = ops.groupnorm_generic_bwd(y2, d_a2.view(N, 1, 1, C), b[4].weight, b[4].bias, groups=G, eps=b[4].eps,
                                                          silu=True, fwd_stats=s2)
        d_y2 = d_y2.view(N, C).float()
        d_a1 = ops.linear(d_y2, pk["c3_t"], splitk=True).to(torch.bfloat16).view(N, k, k, C)
        d_y1, _, dg1, dbt1, _ = ops.groupnorm_generic_bwd(y1, d_a1, b[1].weight, b[1].bias, groups=G, eps=b[1].eps, silu=True,
                                                          fwd_stats=s1)
        d_h = ops.gan_conv4s2_dgrad(d_y1, pk["c0"])
        if not params:
            return d_h, None
        dw0, db0 = ops.gan_conv4s2_wgrad(h, d_y1)
        K = x2.shape[1]
        dw3 = torch.cat([ops.linear_bwd(x2[:, c0:c0 + _WGRAD_COLS].contiguous(), d_y2, None, need_dx=False)[1]
                         for c0 in range(0, K, _WGRAD_COLS)], dim=1)
        dw3 = dw3.view(C, k, k, C).permute(0, 3, 1, 2).contiguous()
        return d_h, (dw0, db0, dg1, dbt1, dw3, d_y2.sum(0), dg4, dbt4, dw6.view(1, C, 1, 1), db6)
