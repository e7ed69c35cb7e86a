"""`pytorch_fid.inception.InceptionV3` on the gfx950 kernels — the feature extractor of the FID evaluation (SURVEY 8 f4;
reference pytorch_fid/inception.py:16-163: blocks, resize / normalise, `forward -> list of feature maps`; the FID patches of
:193-310 — average pools that do not count padding in Mixed_5b-5d / 6b-6e / 7b, a MAX pool in Mixed_7c — over torchvision's
Inception3, whose published architecture is restated here because torchvision is not in the target image).

The torch.nn layers are parameter CONTAINERS with torchvision's names (`Mixed_5b.branch1x1.conv.weight`, `...bn.running_mean`),
so the FID weight file (pt_inception-2015-12-05-6726825d.pth: inception.py:13) loads with `load_fid_weights()`; the module's own
state dict has the reference class's keys (`blocks.0.0.conv.weight` ...).  forward() runs the HIP program: bilinear resize + 2x-1
into NHWC bf16, every BasicConv2d as one generic implicit-GEMM MFMA launch with its BatchNorm folded into the weights and ReLU in
the epilogue, the blocks' concatenations written in place (channel windows of one tensor), the FID pools, the global average pool.
`precision="fp32"` runs the same program on the fp32 op set (dxmi_hip/inception_f32_ops.py): NHWC fp32 activations, the checkpoint's
fp32 weights re-laid-out without arithmetic on the exact f32-input MFMA, BatchNorm + ReLU in the epilogue — the reference's
arithmetic, which the default bf16 mode departs from by about one bf16 rounding per layer.
PARITY IS UNPINNED: neither torchvision nor the weight file exists in this image, so the tests check the program against a
torch-CPU restatement of the same architecture on formula weights (oracle/inception.py), not against the reference's outputs.
No CPU path: non-device tensors raise.
"""
import os

import torch
import torch.nn as nn

from dxmi_hip import inception_f32_ops, ops
from dxmi_hip._lib import DxmiError

# precision -> (op module, activation dtype, name of its resize op, name of its NHWC -> NCHW fp32 op).  Both modules have gconv_pack,
# gconv, pool3x3 and global_avgpool with one calling convention; the ops are looked up on the module at every call.
_PRECISIONS = {"bf16": (ops, torch.bfloat16, "resize_bilinear_nhwc16", "nhwc_bf16_to_nchw_f32"),
               "fp32": (inception_f32_ops, torch.float32, "resize_bilinear_nhwc", "nhwc_to_nchw")}


class BasicConv2d(nn.Module):
    """Conv2d(bias=False) + BatchNorm2d(eps=0.001) + ReLU container (torchvision.models.inception.BasicConv2d)."""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)
        pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        self.k, self.s, self.p = pair(kernel_size), pair(stride), pair(padding)


def _named(**mods):
    m = nn.Module()
    for k, v in mods.items():
        setattr(m, k, v)
    return m


def InceptionA(cin, pool_features):
    return _named(kind="A", branch1x1=BasicConv2d(cin, 64, 1), branch5x5_1=BasicConv2d(cin, 48, 1), branch5x5_2=BasicConv2d(48, 64, 5, padding=2),
                  branch3x3dbl_1=BasicConv2d(cin, 64, 1), branch3x3dbl_2=BasicConv2d(64, 96, 3, padding=1),
                  branch3x3dbl_3=BasicConv2d(96, 96, 3, padding=1), branch_pool=BasicConv2d(cin, pool_features, 1))


def InceptionB(cin):
    return _named(kind="B", branch3x3=BasicConv2d(cin, 384, 3, stride=2), branch3x3dbl_1=BasicConv2d(cin, 64, 1),
                  branch3x3dbl_2=BasicConv2d(64, 96, 3, padding=1), branch3x3dbl_3=BasicConv2d(96, 96, 3, stride=2))


def InceptionC(cin, c7):
    return _named(kind="C", branch1x1=BasicConv2d(cin, 192, 1), branch7x7_1=BasicConv2d(cin, c7, 1),
                  branch7x7_2=BasicConv2d(c7, c7, (1, 7), padding=(0, 3)), branch7x7_3=BasicConv2d(c7, 192, (7, 1), padding=(3, 0)),
                  branch7x7dbl_1=BasicConv2d(cin, c7, 1), branch7x7dbl_2=BasicConv2d(c7, c7, (7, 1), padding=(3, 0)),
                  branch7x7dbl_3=BasicConv2d(c7, c7, (1, 7), padding=(0, 3)), branch7x7dbl_4=BasicConv2d(c7, c7, (7, 1), padding=(3, 0)),
                  branch7x7dbl_5=BasicConv2d(c7, 192, (1, 7), padding=(0, 3)), branch_pool=BasicConv2d(cin, 192, 1))


def InceptionD(cin):
    return _named(kind="D", branch3x3_1=BasicConv2d(cin, 192, 1), branch3x3_2=BasicConv2d(192, 320, 3, stride=2),
                  branch7x7x3_1=BasicConv2d(cin, 192, 1), branch7x7x3_2=BasicConv2d(192, 192, (1, 7), padding=(0, 3)),
                  branch7x7x3_3=BasicConv2d(192, 192, (7, 1), padding=(3, 0)), branch7x7x3_4=BasicConv2d(192, 192, 3, stride=2))


def InceptionE(cin, max_pool):
    return _named(kind="E2" if max_pool else "E1", branch1x1=BasicConv2d(cin, 320, 1), branch3x3_1=BasicConv2d(cin, 384, 1),
                  branch3x3_2a=BasicConv2d(384, 384, (1, 3), padding=(0, 1)), branch3x3_2b=BasicConv2d(384, 384, (3, 1), padding=(1, 0)),
                  branch3x3dbl_1=BasicConv2d(cin, 448, 1), branch3x3dbl_2=BasicConv2d(448, 384, 3, padding=1),
                  branch3x3dbl_3a=BasicConv2d(384, 384, (1, 3), padding=(0, 1)), branch3x3dbl_3b=BasicConv2d(384, 384, (3, 1), padding=(1, 0)),
                  branch_pool=BasicConv2d(cin, 192, 1))


# torchvision's attribute names of the layers, in block order (reference inception.py:83-124)
_LAYOUT = [["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"], ["Conv2d_3b_1x1", "Conv2d_4a_3x3"],
           ["Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"], ["Mixed_7a", "Mixed_7b", "Mixed_7c"]]


class InceptionV3(nn.Module):
    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True, requires_grad=False,
                 use_fid_inception=True, weights=None, precision="bf16"):
        """Constructor of the reference class (inception.py:31-36) + `weights`: path of the FID weight file (or a state dict with
        torchvision's names); None leaves the torch default initialisation — the reference downloads the file, which this image
        cannot.  `precision`: "bf16" (activations and BatchNorm-folded weights in bf16, csrc/inception_ops.hip) or "fp32" (the
        reference's arithmetic: fp32 activations and weights, BatchNorm in the conv epilogue, csrc/inception_f32.hip); the
        attribute may be set again later, each precision keeps its own packed weights."""
        super().__init__()
        self._cache = {}
        self.precision = precision
        if not use_fid_inception:
            raise NotImplementedError("use_fid_inception=False (torchvision's own weights and pools) is not built: the DxMI scripts score FID")
        if requires_grad:
            raise NotImplementedError("InceptionV3 on the HIP path is an inference-only extractor")
        self.resize_input, self.normalize_input = resize_input, normalize_input
        self.output_blocks = sorted(output_blocks)
        self.last_needed_block = max(output_blocks)
        assert self.last_needed_block <= 3, "Last possible output block index is 3"
        layers = {"Conv2d_1a_3x3": BasicConv2d(3, 32, 3, stride=2), "Conv2d_2a_3x3": BasicConv2d(32, 32, 3),
                  "Conv2d_2b_3x3": BasicConv2d(32, 64, 3, padding=1), "Conv2d_3b_1x1": BasicConv2d(64, 80, 1),
                  "Conv2d_4a_3x3": BasicConv2d(80, 192, 3), "Mixed_5b": InceptionA(192, 32), "Mixed_5c": InceptionA(256, 64),
                  "Mixed_5d": InceptionA(288, 64), "Mixed_6a": InceptionB(288), "Mixed_6b": InceptionC(768, 128),
                  "Mixed_6c": InceptionC(768, 160), "Mixed_6d": InceptionC(768, 160), "Mixed_6e": InceptionC(768, 192),
                  "Mixed_7a": InceptionD(768), "Mixed_7b": InceptionE(1280, False), "Mixed_7c": InceptionE(2048, True)}
        self.blocks = nn.ModuleList()
        self._by_name = {}
        tails = [nn.MaxPool2d(kernel_size=3, stride=2), nn.MaxPool2d(kernel_size=3, stride=2), None, nn.AdaptiveAvgPool2d(output_size=(1, 1))]
        for b in range(self.last_needed_block + 1):
            mods = [layers[n] for n in _LAYOUT[b]]
            for n in _LAYOUT[b]:
                self._by_name[n] = layers[n]
            self.blocks.append(nn.Sequential(*(mods + ([tails[b]] if tails[b] is not None else []))))
        for prm in self.parameters():
            prm.requires_grad = False
        if weights is not None:
            self.load_fid_weights(torch.load(weights, map_location="cpu") if isinstance(weights, (str, os.PathLike)) else weights)

    def load_fid_weights(self, state_dict):
        """Load a torchvision-named Inception3 state dict (`Conv2d_1a_3x3.conv.weight`, `Mixed_5b.branch1x1.bn.running_var` ...: the
        FID weight file); the classifier (`fc.*`) and layers beyond `last_needed_block` are ignored, a missing needed tensor raises."""
        for name, mod in self._by_name.items():
            sub = {k[len(name) + 1:]: v for k, v in state_dict.items() if k.startswith(name + ".")}
            mod.load_state_dict(sub, strict=True)
        self._packed = None

    # ------------------------------------------------------------------ precision and packed weights
    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, value):
        if value not in _PRECISIONS:
            raise ValueError(f"InceptionV3: precision must be one of {sorted(_PRECISIONS)}, got {value!r}")
        self._precision = value

    @property
    def _packed(self):
        """The packed weights of the current precision, {id(BasicConv2d): packed}; None before the first forward."""
        return self._cache.get(self._precision, (None, None))[1]

    @_packed.setter
    def _packed(self, value):
        assert value is None, "the packed weights are made by packed()"
        self._cache.clear()

    def _convs(self):
        for name, mod in self._by_name.items():
            if isinstance(mod, BasicConv2d):
                yield name, mod
            else:
                for cn, c in mod.named_children():
                    if isinstance(c, BasicConv2d):
                        yield f"{name}.{cn}", c

    def packed(self):
        key = tuple((t.data_ptr(), t._version) for _, c in self._convs() for t in (c.conv.weight, c.bn.weight, c.bn.bias, c.bn.running_mean, c.bn.running_var))
        if self._cache.get(self._precision, (None, None))[0] != key:
            o = _PRECISIONS[self._precision][0]
            self._cache[self._precision] = (key, {id(c): o.gconv_pack(c.conv.weight, (c.bn.weight, c.bn.bias, c.bn.running_mean, c.bn.running_var), c.bn.eps)
                                                  for _, c in self._convs()})
        return self._cache[self._precision][1]

    # ------------------------------------------------------------------ program
    def _run(self, pk, c, x, out=None, coff=0):
        return _PRECISIONS[self._precision][0].gconv(x, pk[id(c)], stride=c.s, pad=c.p, relu=True, out=out, coff=coff)

    def _mixed(self, pk, m, x):
        run = lambda c, t, out=None, coff=0: self._run(pk, c, t, out, coff)
        N, H, W, _ = x.shape
        o, dtype = _PRECISIONS[self._precision][:2]
        new = lambda h, w, c: torch.empty((N, h, w, c), dtype=dtype, device=x.device)
        k = m.kind
        if k == "A":
            pf = m.branch_pool.conv.out_channels
            out = new(H, W, 224 + pf)
            run(m.branch1x1, x, out, 0)
            run(m.branch5x5_2, run(m.branch5x5_1, x), out, 64)
            run(m.branch3x3dbl_3, run(m.branch3x3dbl_2, run(m.branch3x3dbl_1, x)), out, 128)
            run(m.branch_pool, o.pool3x3(x, 1, 1, avg_exclude_pad=True), out, 224)
        elif k == "B":
            OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
            out = new(OH, OW, 480 + x.shape[3])
            run(m.branch3x3, x, out, 0)
            run(m.branch3x3dbl_3, run(m.branch3x3dbl_2, run(m.branch3x3dbl_1, x)), out, 384)
            o.pool3x3(x, 2, 0, out=out, coff=480)
        elif k == "C":
            out = new(H, W, 768)
            run(m.branch1x1, x, out, 0)
            run(m.branch7x7_3, run(m.branch7x7_2, run(m.branch7x7_1, x)), out, 192)
            t = run(m.branch7x7dbl_2, run(m.branch7x7dbl_1, x))
            run(m.branch7x7dbl_5, run(m.branch7x7dbl_4, run(m.branch7x7dbl_3, t)), out, 384)
            run(m.branch_pool, o.pool3x3(x, 1, 1, avg_exclude_pad=True), out, 576)
        elif k == "D":
            OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
            out = new(OH, OW, 512 + x.shape[3])
            run(m.branch3x3_2, run(m.branch3x3_1, x), out, 0)
            run(m.branch7x7x3_4, run(m.branch7x7x3_3, run(m.branch7x7x3_2, run(m.branch7x7x3_1, x))), out, 320)
            o.pool3x3(x, 2, 0, out=out, coff=512)
        else:           # E1 / E2
            out = new(H, W, 2048)
            run(m.branch1x1, x, out, 0)
            t = run(m.branch3x3_1, x)
            run(m.branch3x3_2a, t, out, 320)
            run(m.branch3x3_2b, t, out, 704)
            t = run(m.branch3x3dbl_2, run(m.branch3x3dbl_1, x))
            run(m.branch3x3dbl_3a, t, out, 1088)
            run(m.branch3x3dbl_3b, t, out, 1472)
            # Mixed_7b: average over the in-bounds pixels; Mixed_7c: MAX pool (the FID model's own quirk, inception.py:303-308)
            pooled = o.pool3x3(x, 1, 1, avg_exclude_pad=(k == "E1"))
            run(m.branch_pool, pooled, out, 1856)
        return out

    @torch.no_grad()
    def forward(self, inp):
        """inp [B, 3, H, W] in (0, 1) on the device -> list of fp32 NCHW feature maps of the selected blocks (reference :129-163)."""
        if not inp.is_cuda:
            raise DxmiError("pytorch_fid.inception.InceptionV3 runs only on the HIP device path (no CPU fallback)")
        pk = self.packed()
        x = inp.contiguous().float()
        N, _, H, W = x.shape
        OH, OW = (299, 299) if self.resize_input else (H, W)
        o, _, resize, to_nchw = _PRECISIONS[self._precision]
        h = getattr(o, resize)(x, OH, OW, normalize=self.normalize_input)
        outp = []
        for idx in range(self.last_needed_block + 1):
            for name in _LAYOUT[idx]:
                m = self._by_name[name]
                h = self._run(pk, m, h) if isinstance(m, BasicConv2d) else self._mixed(pk, m, h)
            if idx in (0, 1):
                h = o.pool3x3(h, 2, 0)
            if idx == 3:
                feat = o.global_avgpool(h)
                if idx in self.output_blocks:
                    outp.append(feat.view(N, -1, 1, 1))
            elif idx in self.output_blocks:
                outp.append(getattr(o, to_nchw)(h))
        return outp


class FIDInceptionV3(InceptionV3):
    """The extractor `--fid_extractor pytorch_fid.inception:FIDInceptionV3` resolves to (the scripts instantiate a class): InceptionV3
    pool3 features with the FID weights named by DXMI_FID_WEIGHTS (pt_inception-2015-12-05-6726825d.pth).  Without the file this
    raises — scoring FID on an untrained extractor is never what the caller wants.  This class computes in bf16 (PRECISION);
    FIDInceptionV3FP32 is the same extractor in the reference's fp32."""

    PRECISION = "bf16"

    def __init__(self, dims=2048):
        path = os.environ.get("DXMI_FID_WEIGHTS")
        if not path or not os.path.exists(path):
            raise DxmiError("DXMI_FID_WEIGHTS must name the FID Inception weight file (pt_inception-2015-12-05-6726825d.pth); "
                            "it cannot be downloaded into this image")
        super().__init__([InceptionV3.BLOCK_INDEX_BY_DIM[dims]], weights=path, precision=self.PRECISION)


class FIDInceptionV3FP32(FIDInceptionV3):
    """`--fid_extractor pytorch_fid.inception:FIDInceptionV3FP32`: FIDInceptionV3 with every activation, weight and sum in fp32, the
    arithmetic of the reference's extractor (csrc/inception_f32.hip).  Same contract, same DXMI_FID_WEIGHTS."""

    PRECISION = "fp32"


class EvalInceptionV3(InceptionV3):
    """The feature extractor of `evaluations/evaluator.py` (the ADM evaluator's three Inception taps, reference
    evaluations/evaluator.py:23-24, 584-616), on the FID weights named by DXMI_FID_WEIGHTS; raises without the file.

    Extractor contract the evaluator relies on (a weight-free stand-in only has to meet it):
      __call__(images)  images uint8 [B, H, W, 3] (NHWC, the `arr_0` batches of an evaluator .npz) on the device
                        -> (pool fp32 [B, 2048], spatial fp32 [B, S]) on the device
      softmax_weight    fp32 [2048, C] device tensor: pool . softmax_weight are the classifier logits (no bias)

    pool is `pool_3:0`.  spatial is `mixed_6/conv:0[..., :7]` flattened NHWC (17 x 17 x 7 = 2023): the TF graph numbers its
    mixed blocks mixed, mixed_1 ... mixed_10 for torchvision's Mixed_5b, 5c, 5d, 6a, 6b, 6c, 6d, 6e, 7a, 7b, 7c (eleven blocks
    both ways; mixed_3 / Mixed_6a is the 35 -> 17 reduction and mixed_8 / Mixed_7a the 17 -> 8 one), so mixed_6 is Mixed_6d, a
    17 x 17 block, and its `conv` is the un-prefixed first branch, the 1x1 conv + BN + ReLU that torchvision calls
    `Mixed_6d.branch1x1` (192 channels, written first into the block's concatenation).  2023 = 17 * 17 * 7 is the sFID feature
    size of the reference, which only a 17 x 17 tap gives.  softmax_weight is `fc.weight`^T (`softmax/logits/MatMul`'s
    operand; the reference drops the bias, evaluator.py:603-616).  This class computes in bf16 (PRECISION); EvalInceptionV3FP32
    is the same extractor in fp32."""

    SPATIAL_CHANNELS = 7
    PRECISION = "bf16"

    def __init__(self, weights=None):
        path = weights or os.environ.get("DXMI_FID_WEIGHTS")
        if not path or not os.path.exists(path):
            raise DxmiError("DXMI_FID_WEIGHTS must name the FID Inception weight file (pt_inception-2015-12-05-6726825d.pth, with "
                            "its fc.weight); it cannot be downloaded into this image")
        sd = torch.load(path, map_location="cpu")
        if "fc.weight" not in sd:
            raise DxmiError(f"{path}: no fc.weight (the Inception Score needs the classifier weight)")
        super().__init__([InceptionV3.DEFAULT_BLOCK_INDEX], weights=sd, precision=self.PRECISION)
        self.softmax_weight = sd["fc.weight"].float().t().contiguous().cuda()
        self.to(self.softmax_weight.device)          # evaluator.py calls the instance as it is built: the weights go where the images are
        self._tap = None

    def _mixed(self, pk, m, x):
        out = super()._mixed(pk, m, x)
        if m is self._by_name["Mixed_6d"]:
            self._tap = out[..., :self.SPATIAL_CHANNELS].float().reshape(out.shape[0], -1)
        return out

    @torch.no_grad()
    def __call__(self, images):
        if not images.is_cuda:
            raise DxmiError("EvalInceptionV3 runs only on the HIP device path (no CPU fallback)")
        x = images.permute(0, 3, 1, 2).float().div_(255.0)
        pool = self.forward(x)[0].reshape(x.shape[0], -1)
        spatial, self._tap = self._tap, None
        return pool, spatial


class EvalInceptionV3FP32(EvalInceptionV3):
    """`evaluator.py --extractor pytorch_fid.inception:EvalInceptionV3FP32`: EvalInceptionV3 in fp32 (csrc/inception_f32.hip); `spatial`
    is Mixed_6d.branch1x1[..., :7] of the fp32 tensor.  Same contract, same weight file."""

    PRECISION = "fp32"
