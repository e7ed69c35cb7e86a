"""Record the launches of the HIP InceptionV3 program and walk the oracle's graph over them (test_hip_inception_launches.py).

`Recorder` intercepts EVERY public function of `dxmi_hip.ops` while a forward of the extractor runs ("record or refuse", as
backward_census.Census): a call is one of the six launch ops of the extractor (LAUNCH: it gets a record: the layer it belongs to,
its input tensor, the output tensor and the channel window written), a helper on backward_census.ALLOWED, or unknown: its name
lands in `Recorder.unknown` and the test fails naming it.  The records keep references, not copies: every window of a
concatenation is written once and no launch of the program writes its input.

`DeviceGraph` is an oracle.inception.Graph whose values are NCHW views of the bf16 NHWC tensors the HIP launches wrote.  The
oracle's own wiring (its torch.cat order, its choice of pool per block, its strides and paddings) assembles the input of every
layer from those tensors; each hook then
    1. takes the record of the launch with that layer's name (a missing or a second one is an error),
    2. demands that the assembled input is torch.equal to the input the launch received (dataflow, bitwise),
    3. judges the launch's output element by element against the fp64 reference of the layer AS THE ORACLE STATES IT (its stride
       and padding, the checkpoint's kernel size, the packed buffer of that layer's name) on that input (forward_bounds),
    4. hands the launch's output on.
Layer names: a conv has its torchvision name ("Mixed_6d.branch1x1"); the pool of a Mixed block is "<block>.pool", the pools
after the two stem blocks "pool1" / "pool2", the global average "pool3", the resize "prep", the k-th layout conversion "tap<k>".
"""
import inspect

import torch

import backward_census
import forward_bounds as fb
from backward_bounds import BoundError
from oracle import inception as oinc

LAUNCH = ("resize_bilinear_nhwc16", "gconv", "pool3x3", "global_avgpool", "nhwc_bf16_to_nchw_f32", "gconv_pack")


def tv_state_dict(model, fc=False):
    """A torchvision-named state dict (the FID weight file's naming) with formula weights that keep activations O(1) through the
    ~45 conv layers: He-scaled conv weights, BatchNorm statistics near identity.  fc: give the classifier weight formula values
    (EvalInceptionV3's softmax_weight) instead of zeros."""
    from oracle.weights import formula_tensor
    sd = {}
    for name, c in model._convs():
        w = formula_tensor(name + ".conv.weight", c.conv.weight.shape) * (6.0 ** 0.5)          # uniform(+-1/sqrt(fan_in)) -> variance 2 / fan_in
        n = c.bn.weight.numel()
        f = lambda k: formula_tensor(f"{name}.bn.{k}", (n,)) * (n ** 0.5)                      # uniform(+-1)
        sd[name + ".conv.weight"] = w
        sd[name + ".bn.weight"] = 1.0 + 0.2 * f("weight")
        sd[name + ".bn.bias"] = 0.1 * f("bias")
        sd[name + ".bn.running_mean"] = 0.1 * f("running_mean")
        sd[name + ".bn.running_var"] = 1.0 + 0.3 * f("running_var").abs()
        sd[name + ".bn.num_batches_tracked"] = torch.tensor(0)
    sd["fc.weight"] = formula_tensor("fc.weight", (1008, 2048)) if fc else torch.zeros(1008, 2048)   # the FID file has both
    sd["fc.bias"] = torch.zeros(1008)
    return sd


class Rec:
    __slots__ = ("op", "name", "x", "out", "coff", "C", "args", "judged")

    def __init__(self, op, name, x, out, coff, C, args):
        self.op, self.name, self.x, self.out, self.coff, self.C, self.args, self.judged = op, name, x, out, coff, C, args, False

    def window(self):
        return self.out[..., self.coff:self.coff + self.C]


class Recorder:
    """`with Recorder(ops, model) as r: model(x)` -> r.records (in launch order), r.unknown."""

    def __init__(self, ops, model):
        self.ops, self.model, self.records, self.saved = ops, model, [], {}
        self.unknown = set(backward_census.unknown_classes(ops))
        self.block, self.stem_pools, self.taps = None, 0, 0

    def _record(self, name, fn, a, kw):
        b = inspect.signature(fn).bind(*a, **kw)
        b.apply_defaults()
        p = dict(b.arguments)
        out = fn(*a, **kw)
        if name == "gconv":
            r = Rec(name, None, p["x"], out, int(p["coff"]), p["pk"].Cout, p)          # layer name: resolved from pk after the run
        elif name == "pool3x3":
            if self.block is None:
                self.stem_pools += 1
            r = Rec(name, f"{self.block}.pool" if self.block else f"pool{self.stem_pools}", p["x"], out, int(p["coff"]), p["x"].shape[3], p)
        elif name == "global_avgpool":
            r = Rec(name, "pool3", p["x"], out, 0, out.shape[-1], p)
        elif name == "resize_bilinear_nhwc16":
            r = Rec(name, "prep", p["x"], out, 0, 16, p)
        elif name == "nhwc_bf16_to_nchw_f32":
            r = Rec(name, f"tap{self.taps}", p["x"], out, 0, out.shape[1], p)
            self.taps += 1
        else:                                                                            # gconv_pack: out is the PackedGConv
            r = Rec(name, None, p["weight"], out, 0, out.Cout, p)
        self.records.append(r)
        return out

    def _wrap(self, name, fn):
        launch = name in LAUNCH
        judged = launch or name in backward_census.ALLOWED

        def w(*a, **kw):
            if launch:
                return self._record(name, fn, a, kw)
            if not judged:
                self.unknown.add(name)
            return fn(*a, **kw)
        return w

    def __enter__(self):
        for n, fn in backward_census.public_functions(self.ops).items():
            self.saved[(self.ops, n)] = fn
            setattr(self.ops, n, self._wrap(n, fn))
        names = {id(m): n for n, m in self.model._by_name.items()}
        mixed = self.model._mixed

        def in_block(pk, m, x):
            self.block = names[id(m)]
            try:
                return mixed(pk, m, x)
            finally:
                self.block = None
        self.model._mixed = in_block
        return self

    def __exit__(self, *exc):
        for (obj, n), v in self.saved.items():
            setattr(obj, n, v)
        del self.model._mixed                        # the instance attribute; the class's method is back
        packed = self.model._packed or {}
        by_pk = {id(packed[id(c)]): n for n, c in self.model._convs() if id(c) in packed}
        for r in self.records:
            if r.op == "gconv":
                r.name = by_pk.get(id(r.args["pk"]))
            elif r.op == "gconv_pack":
                r.name = by_pk.get(id(r.out))
        return False

    def count(self, op):
        return sum(r.op == op for r in self.records)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


class DeviceGraph(oinc.Graph):
    """See the module docstring.  check: a forward_bounds.FwdChecker; sd: the checkpoint (CPU tensors, torchvision names)."""

    def __init__(self, recorder, model, sd, check):
        self.model, self.sd, self.check = model, sd, check
        self.by_name = {}
        for r in recorder.records:
            if r.op != "gconv_pack":
                self.by_name.setdefault(r.name, []).append(r)
        self.packs = [r for r in recorder.records if r.op == "gconv_pack"]
        self.convs = dict(model._convs())
        self.visited = []
        self.judged = {}

    def _take(self, name, op, x_nchw):
        recs = self.by_name.get(name, [])
        if len(recs) != 1 or recs[0].judged:
            raise BoundError(f"{name}: the oracle's graph calls this layer once, the HIP program launched it {len(recs)} time(s)"
                             + (" and it was already visited" if recs and recs[0].judged else ""))
        r = recs[0]
        if r.op != op:
            raise BoundError(f"{name}: the oracle's graph has a {op} here, the HIP program launched {r.op}")
        want = x_nchw if op == "resize_bilinear_nhwc16" else x_nchw.permute(0, 2, 3, 1)
        if want.shape != r.x.shape or want.dtype != r.x.dtype or not torch.equal(want, r.x):
            raise BoundError(f"{name}: dataflow: the input the HIP launch received ({tuple(r.x.shape)}, {r.x.dtype}) is not the tensor the "
                             f"oracle's wiring assembles from the earlier launches' outputs ({tuple(want.shape)}, {want.dtype})")
        r.judged = True
        self.visited.append(name)
        self.judged[op] = self.judged.get(op, 0) + 1
        return r

    # ---------------------------------------------------------------- hooks of the oracle's graph
    def prep(self, x, resize_input, normalize_input):
        r = self._take("prep", "resize_bilinear_nhwc16", x)
        OH, OW = (299, 299) if resize_input else tuple(x.shape[2:])
        judge_resize(self.check, r.out, x, OH, OW, normalize_input)
        return _nchw(r.out)

    def bc(self, sd, name, x, stride=1, padding=0):
        r = self._take(name, "gconv", x)
        c = self.convs[name]
        pk = self.model._packed[id(c)]
        if r.args["pk"] is not pk:
            raise BoundError(f"{name}: launched with another layer's packed weights")
        Cout, Cin, KH, KW = sd[name + ".conv.weight"].shape
        assert (pk.Cout, pk.Cin, pk.KH, pk.KW) == (Cout, Cin, KH, KW), name
        w4 = fb.gconv_unpack(pk.w, Cout, Cin, KH, KW)[:Cout]
        judge_gconv(self.check, r.window(), r.x, w4, pk.bias[:Cout], _pair(stride), _pair(padding), relu=True)
        return _nchw(r.window())

    def avg(self, where, x):
        r = self._take(where, "pool3x3", x)
        ref, bound, _ = fb.avgpool3x3_ref(r.x, 1, 1)
        self.check.within("avgpool3x3", r.window(), ref, bound)
        return _nchw(r.window())

    def maxpool(self, where, x, stride, padding=0):
        r = self._take(where, "pool3x3", x)
        ref = fb.maxpool3x3_ref(r.x, stride, padding)
        got = r.window()
        if got.shape != ref.shape or not torch.equal(got.double(), ref):
            raise BoundError(f"{where}: not bitwise the maximum of its 3x3 window (stride {stride}, padding {padding})")
        return _nchw(got)

    def gap(self, where, x):
        r = self._take(where, "global_avgpool", x)
        ref, bound = fb.global_avgpool_ref(r.x)
        self.check.within("global_avgpool", r.out, ref, bound)
        return r.out.view(r.out.shape[0], -1, 1, 1)

    # ---------------------------------------------------------------- what the graph does not state
    def judge_packs(self):
        """Every gconv_pack launch of the run against the fp64 fold of the checkpoint's tensors of its layer."""
        seen = set()
        for r in self.packs:
            if r.name is None or r.name in seen:
                raise BoundError(f"gconv_pack: a launch that is not the one pack of a conv layer ({r.name})")
            seen.add(r.name)
            dev = r.out.w.device
            bn = tuple(self.sd[f"{r.name}.bn.{k}"].to(dev) for k in ("weight", "bias", "running_mean", "running_var"))
            judge_pack(self.check, r.out, self.sd[r.name + ".conv.weight"].to(dev), bn, 1e-3)
            r.judged = True
            self.judged["gconv_pack"] = self.judged.get("gconv_pack", 0) + 1
        return seen

    def judge_taps(self, outs, outputs, output_blocks):
        """The NCHW fp32 conversions: the k-th one received the oracle's block output (bitwise) and returned its exact fp32 image;
        `outputs` (what the model returned) are those tensors, the last block's the judged global average."""
        assert len(outputs) == len(output_blocks)
        k = 0
        for o, b in zip(outputs, sorted(output_blocks)):
            if b == 3:
                if not torch.equal(o, outs[3]):
                    raise BoundError("block 3: the returned pool3 features are not the global average pool's output")
                continue
            r = self._take(f"tap{k}", "nhwc_bf16_to_nchw_f32", outs[b])
            k += 1
            if r.out.dtype != torch.float32 or not torch.equal(r.out, _nchw(r.x).float()) or not torch.equal(o, r.out):
                raise BoundError(f"block {b}: the NCHW fp32 conversion is not bitwise its input")

    def complete(self, recorder):
        """Every recorded launch was judged, per op; every conv name was visited exactly once."""
        left = [(r.op, r.name) for r in recorder.records if not r.judged]
        if left:
            raise BoundError(f"launches the walk did not judge: {left}")
        for op in LAUNCH:
            if recorder.count(op) != self.judged.get(op, 0):
                raise BoundError(f"{op}: {recorder.count(op)} launches recorded, {self.judged.get(op, 0)} judged")
        convs = sorted(n for n in self.visited if n in self.convs)
        if convs != sorted(self.convs):
            raise BoundError(f"conv layers visited {len(convs)}, the model has {len(self.convs)}: {set(convs) ^ set(self.convs)}")


# -------------------------------------------------------------------------------------------- judges shared with the row tests
def judge_gconv(check, got, x, w4, bias, stride, pad, relu):
    KH, KW = w4.shape[2:]
    ref, A = fb.gconv_ref(x, w4, bias, stride, pad)
    post = fb.act64(ref, 2 if relu else 0)
    del ref
    return check.within(f"gconv{KH}x{KW}", got, post, fb.conv_bound(post, A, x.shape[3] * KH * KW, 2 if relu else 0))


def judge_pack(check, pk, weight, bn, eps):
    """A PackedGConv against the fp64 fold of (weight, bn): the real block within its bounds, the padding exactly zero."""
    Cout, Cin, KH, KW = weight.shape
    if (pk.Cout, pk.Cin, pk.KH, pk.KW, pk.CinP) != (Cout, Cin, KH, KW, -(-Cin // 16) * 16):
        raise BoundError(f"gconv_pack: header {(pk.Cout, pk.Cin, pk.KH, pk.KW, pk.CinP)} for a weight {tuple(weight.shape)}")
    w4 = fb.gconv_unpack(pk.w, Cout, Cin, KH, KW)
    fold, bias, mag = fb.gconv_pack_ref(weight, bn, eps)
    bw, bb = fb.gconv_pack_bounds(fold, mag)
    if pk.bias.dtype != torch.float32 or pk.bias.numel() != w4.shape[0]:
        raise BoundError("gconv_pack: bias is not fp32 [CoutP]")
    if float(w4[Cout:].float().abs().max() if w4.shape[0] > Cout else 0) != 0 or float(pk.bias[Cout:].abs().max() if w4.shape[0] > Cout else 0) != 0:
        raise BoundError("gconv_pack: padded cout rows are not zero")
    if w4.shape[1] > Cin and float(w4[:, Cin:].float().abs().max()) != 0:
        raise BoundError("gconv_pack: padded cin channels are not zero")
    if bn is None:
        if not torch.equal(w4[:Cout, :Cin].double(), weight.to(torch.bfloat16).double()) or float(pk.bias.abs().max()) != 0:
            raise BoundError("gconv_pack without BatchNorm: not the bf16 rounding of the weight with a zero bias")
    check.within("gconv_pack.w", w4[:Cout, :Cin], fold, bw)
    check.within("gconv_pack.bias", pk.bias[:Cout], bias, bb)


def judge_resize(check, got, x, OH, OW, normalize):
    """got NHWC bf16 [N, OH, OW, 16] from x NCHW fp32: channels 0..2 within the bound, 3..15 exactly zero; a same-size
    'resize' is bitwise the bf16 rounding of the fp32 value (2 x - 1 or x)."""
    N = x.shape[0]
    if tuple(got.shape) != (N, OH, OW, 16) or got.dtype != torch.bfloat16:
        raise BoundError(f"resize: output {tuple(got.shape)} {got.dtype}")
    if float(got[..., 3:].float().abs().max()) != 0:
        raise BoundError("resize: padding channels 3..15 are not zero")
    ref, bound = fb.resize_ref(x, OH, OW, normalize)
    check.within("resize", got[..., :3], ref, bound)
    if (OH, OW) == tuple(x.shape[2:]):
        v = (2 * x - 1) if normalize else x
        if not torch.equal(got[..., :3], v.permute(0, 2, 3, 1).to(torch.bfloat16)):
            raise BoundError("resize to the same size is not bitwise the bf16 rounding of the fp32 value")
