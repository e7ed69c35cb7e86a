"""Record the launches of the fp32 InceptionV3 program (pytorch_fid.inception, precision="fp32", on dxmi_hip/inception_f32_ops.py)
and walk the oracle's graph over them: inception_walk.Recorder / DeviceGraph for the fp32 op set (test_hip_inception_f32.py).

`RecorderF32` wraps EVERY public function of the fp32 ops module while a forward runs ("record or refuse"): a call is one of the
six launch ops (LAUNCH: it gets a record) or unknown, and then the test fails naming it; a public class of the module that is not
KNOWN_CLASSES is unknown too.  The test runs it nested inside an inception_walk.Recorder over dxmi_hip.ops, which must record
nothing: the fp32 program launches no bf16 kernel.

`DeviceGraphF32` is an oracle.inception.Graph over the NHWC fp32 tensors the launches wrote: for every layer the oracle's wiring
names, the assembled input must be torch.equal to what the launch received, and the output is judged element by element against
stock torch in float64 on the device, on the fp32 bits the launch read, with these bounds (u32 = 2^-24):

  conv      operands: the input tensor, the checkpoint weight (which the packed buffer must reproduce BITWISE when un-laid-out:
            judge_pack_f32), the device scale / shift buffers.  An fmaf chain of K = CinP * KH * KW products has error
            <= K u32 sum|w||x| (Higham 4.2, any order); v = acc * scale + shift rounds at most twice more, then ReLU (Lipschitz 1):
                |got - act(ref64)| <= (K + 3) u32 (|scale| sum|w||x| + |shift|) + 4 u32 |act(ref64)|
            = fb.conv_bound(post, A, K, act, bf16_out=False) with A = |scale| sum|w||x| + |shift|.
  pack      weight bitwise, padding exactly zero; scale = gamma / sqrt(var + eps) is an add, a correctly rounded sqrt and divide
            and the fp32 value of eps: within 4 u32 |scale64|; shift = beta - mean * scale: within 8 u32 (|beta| + |mean scale|).
            Without BatchNorm: scale exactly 1, shift exactly the bias (or 0).
  avg pool  cnt fp32 values added in order and one division: (cnt + 1) u32 mean|x| + 4 u32 |ref|.  Max pool: bitwise.
  global average pool: fb.global_avgpool_ref as it is (fp32 output).
  resize    the pre-store part of fb.resize_ref's bound (its core, recovered from the bf16 bound exactly as
            test_resize_bound_holds_for_the_fp32_emulation does) + 4 u32 |ref|; a same-size resize is bitwise the fp32 value;
            channels 3..7 exactly zero.
  NHWC -> NCHW: bitwise.
"""
import inspect

import torch
import torch.nn.functional as F

import forward_bounds as fb
import inception_walk as iw
from backward_bounds import BoundError
from oracle import inception as oinc

U32 = fb.U32
GRAN = 8
LAUNCH = ("resize_bilinear_nhwc", "gconv", "pool3x3", "global_avgpool", "nhwc_to_nchw", "gconv_pack")
KNOWN_CLASSES = ("PackedGConvF32",)


def public_functions(mod):
    return {n: v for n, v in vars(mod).items() if inspect.isfunction(v) and not n.startswith("_") and v.__module__ == mod.__name__}


class RecorderF32:
    """`with RecorderF32(f32ops, model) as r: model(x)` -> r.records (in launch order), r.unknown."""

    def __init__(self, mod, model):
        self.mod, self.model, self.records, self.saved = mod, model, [], {}
        self.unknown = {n for n, v in vars(mod).items()
                        if inspect.isclass(v) and not n.startswith("_") and v.__module__ == mod.__name__ and n not in KNOWN_CLASSES}
        self.block, self.stem_pools, self.taps = None, 0, 0

    def _record(self, name, fn, a, kw):
        b = inspect.signature(fn).bind(*a, **kw)
        b.apply_defaults()
        p = dict(b.arguments)
        out = fn(*a, **kw)
        if name == "gconv":
            r = iw.Rec(name, None, p["x"], out, int(p["coff"]), p["pk"].Cout, p)
        elif name == "pool3x3":
            if self.block is None:
                self.stem_pools += 1
            r = iw.Rec(name, f"{self.block}.pool" if self.block else f"pool{self.stem_pools}", p["x"], out, int(p["coff"]), p["x"].shape[3], p)
        elif name == "global_avgpool":
            r = iw.Rec(name, "pool3", p["x"], out, 0, out.shape[-1], p)
        elif name == "resize_bilinear_nhwc":
            r = iw.Rec(name, "prep", p["x"], out, 0, GRAN, p)
        elif name == "nhwc_to_nchw":
            r = iw.Rec(name, f"tap{self.taps}", p["x"], out, 0, out.shape[1], p)
            self.taps += 1
        else:
            r = iw.Rec(name, None, p["weight"], out, 0, out.Cout, p)
        self.records.append(r)
        return out

    def _wrap(self, name, fn):
        def w(*a, **kw):
            if name in LAUNCH:
                return self._record(name, fn, a, kw)
            self.unknown.add(name)
            return fn(*a, **kw)
        return w

    def __enter__(self):
        for n, fn in public_functions(self.mod).items():
            self.saved[n] = fn
            setattr(self.mod, n, self._wrap(n, fn))
        names = {id(m): n for n, m in self.model._by_name.items()}
        self.prev_mixed = self.model.__dict__.get("_mixed")
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
        for n, v in self.saved.items():
            setattr(self.mod, n, v)
        if self.prev_mixed is None:
            del self.model._mixed
        else:
            self.model._mixed = self.prev_mixed
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


# -------------------------------------------------------------------------------------------- references, bounds, judges
def gconv_unpack_f32(wp, Cout, Cin, KH, KW):
    """Packed buffer [CoutP][KH * KW][CinP] (flat fp32, CoutP = ceil32, CinP = ceil8: include/dxmi_hip.h) -> [CoutP, CinP, KH, KW]."""
    CoutP, CinP = -(-Cout // 32) * 32, -(-Cin // GRAN) * GRAN
    assert wp.dtype == torch.float32 and wp.numel() == CoutP * KH * KW * CinP, (wp.dtype, wp.numel(), CoutP, KH, KW, CinP)
    return wp.reshape(CoutP, KH * KW, CinP).permute(0, 2, 1).reshape(CoutP, CinP, KH, KW)


def gconv_f32_ref(x, w4, scale, shift, stride, pad, relu):
    """-> (act(ref64), bound): x NHWC [N, IH, IW, CinP], w4 [Cout, CinP, KH, KW], scale / shift [Cout] (any float dtype: their bits)."""
    z = torch.zeros(w4.shape[0], dtype=torch.float64, device=x.device)
    conv, A = fb.gconv_ref(x, w4, z, stride, pad)
    sc, sh = scale.double(), shift.double()
    act = 2 if relu else 0
    post = fb.act64(conv * sc + sh, act)
    A = A * sc.abs() + sh.abs()
    return post, fb.conv_bound(post, A, x.shape[3] * w4.shape[2] * w4.shape[3], act, bf16_out=False)


def judge_gconv_f32(check, got, x, w4, scale, shift, stride, pad, relu):
    if got.dtype != torch.float32:
        raise BoundError(f"gconv_f32: output dtype {got.dtype}")
    post, bound = gconv_f32_ref(x, w4, scale, shift, stride, pad, relu)
    return check.within(f"gconv_f32_{w4.shape[2]}x{w4.shape[3]}", got, post, bound)


def pack_f32_ref(bn, eps):
    """fp64 (scale, shift, shift magnitude |beta| + |mean scale|) of a BatchNorm."""
    gamma, beta, mean, var = (t.double() for t in bn)
    scale = gamma / torch.sqrt(var + eps)
    return scale, beta - mean * scale, beta.abs() + (mean * scale).abs()


def judge_pack_f32(check, pk, weight, bn, eps, bias=None):
    Cout, Cin, KH, KW = weight.shape
    CoutP, CinP = -(-Cout // 32) * 32, -(-Cin // GRAN) * GRAN
    if (pk.Cout, pk.Cin, pk.KH, pk.KW, pk.CinP) != (Cout, Cin, KH, KW, CinP):
        raise BoundError(f"gconv_pack f32: header {(pk.Cout, pk.Cin, pk.KH, pk.KW, pk.CinP)} for a weight {tuple(weight.shape)}")
    w4 = gconv_unpack_f32(pk.w, Cout, Cin, KH, KW)
    if not torch.equal(w4[:Cout, :Cin], weight.float()):
        raise BoundError("gconv_pack f32: the un-laid-out packed weight is not bitwise the checkpoint's weight")
    if float(w4[Cout:].abs().sum()) != 0 or float(w4[:, Cin:].abs().sum()) != 0:
        raise BoundError("gconv_pack f32: padded couts / channels are not zero")
    for t in (pk.scale, pk.shift):
        if t.dtype != torch.float32 or t.numel() != CoutP or float(t[Cout:].abs().sum()) != 0:
            raise BoundError("gconv_pack f32: scale / shift are not fp32 [CoutP] with zero padding")
    if bn is None:
        want = torch.zeros(Cout, device=weight.device) if bias is None else bias.float()
        if not torch.equal(pk.scale[:Cout], torch.ones_like(want)) or not torch.equal(pk.shift[:Cout], want):
            raise BoundError("gconv_pack f32 without BatchNorm: scale is not 1 or shift is not the bias")
        return
    scale, shift, mag = pack_f32_ref(bn, eps)
    check.within("gconv_pack_f32.scale", pk.scale[:Cout], scale, 4 * U32 * scale.abs())
    check.within("gconv_pack_f32.shift", pk.shift[:Cout], shift, 8 * U32 * mag)


def avgpool_f32_ref(x, stride, pad):
    """-> (ref64, bound, cnt) of the exclude-pad 3x3 average of an NHWC fp32 tensor."""
    ref, _, cnt = fb.avgpool3x3_ref(x, stride, pad)
    mabs = F.avg_pool2d(x.double().abs().permute(0, 3, 1, 2), 3, stride, pad, count_include_pad=False).permute(0, 2, 3, 1)
    return ref, fb.store_bound((cnt + 1) * U32 * mabs, ref, bf16_out=False), cnt


def resize_f32_bound(x, OH, OW, normalize):
    """-> (ref64 NHWC [N, OH, OW, 3], bound): the pre-store part of fb.resize_ref's bound + 4 u32 |ref|."""
    ref, bound16 = fb.resize_ref(x, OH, OW, normalize)
    core = (bound16 - (fb.U16 + 4 * U32) * ref.abs()) / (1 + fb.U16)
    return ref, fb.store_bound(core, ref, bf16_out=False)


def judge_resize_f32(check, got, x, OH, OW, normalize):
    N = x.shape[0]
    if tuple(got.shape) != (N, OH, OW, GRAN) or got.dtype != torch.float32:
        raise BoundError(f"resize f32: output {tuple(got.shape)} {got.dtype}")
    if float(got[..., 3:].abs().sum()) != 0:
        raise BoundError("resize f32: padding channels 3..7 are not zero")
    ref, bound = resize_f32_bound(x, OH, OW, normalize)
    check.within("resize_f32", got[..., :3], ref, bound)
    if (OH, OW) == tuple(x.shape[2:]):
        v = (2 * x - 1) if normalize else x
        if not torch.equal(got[..., :3], v.permute(0, 2, 3, 1)):
            raise BoundError("resize f32 to the same size is not bitwise the fp32 value")


class DeviceGraphF32(oinc.Graph):
    """inception_walk.DeviceGraph for the fp32 program.  check: a forward_bounds.FwdChecker; sd: the checkpoint (CPU, torchvision names)."""

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
        want = x_nchw if op == "resize_bilinear_nhwc" else x_nchw.permute(0, 2, 3, 1)
        if want.shape != r.x.shape or want.dtype != r.x.dtype or r.x.dtype != torch.float32 or not torch.equal(want, r.x):
            raise BoundError(f"{name}: dataflow: the input the HIP launch received ({tuple(r.x.shape)}, {r.x.dtype}) is not the tensor the "
                             f"oracle's wiring assembles from the earlier launches' outputs ({tuple(want.shape)}, {want.dtype})")
        r.judged = True
        self.visited.append(name)
        self.judged[op] = self.judged.get(op, 0) + 1
        return r

    def prep(self, x, resize_input, normalize_input):
        r = self._take("prep", "resize_bilinear_nhwc", x)
        OH, OW = (299, 299) if resize_input else tuple(x.shape[2:])
        judge_resize_f32(self.check, r.out, x, OH, OW, normalize_input)
        return iw._nchw(r.out)

    def bc(self, sd, name, x, stride=1, padding=0):
        r = self._take(name, "gconv", x)
        pk = self.model._packed[id(self.convs[name])]
        if r.args["pk"] is not pk:
            raise BoundError(f"{name}: launched with another layer's packed weights")
        w = sd[name + ".conv.weight"]
        Cout, Cin, KH, KW = w.shape
        assert (pk.Cout, pk.Cin, pk.KH, pk.KW) == (Cout, Cin, KH, KW), name
        w4 = gconv_unpack_f32(pk.w, Cout, Cin, KH, KW)[:Cout]
        if not torch.equal(w4[:, :Cin], w.to(w4.device)):                       # the conv's operand IS the checkpoint's weight
            raise BoundError(f"{name}: the packed weight is not bitwise the checkpoint's")
        judge_gconv_f32(self.check, r.window(), r.x, w4, pk.scale[:Cout], pk.shift[:Cout], iw._pair(stride), iw._pair(padding), relu=True)
        return iw._nchw(r.window())

    def avg(self, where, x):
        r = self._take(where, "pool3x3", x)
        ref, bound, _ = avgpool_f32_ref(r.x, 1, 1)
        self.check.within("avgpool3x3_f32", r.window(), ref, bound)
        return iw._nchw(r.window())

    def maxpool(self, where, x, stride, padding=0):
        r = self._take(where, "pool3x3", x)
        got = r.window()
        ref = fb.maxpool3x3_ref(r.x, stride, padding)
        if got.dtype != torch.float32 or got.shape != ref.shape or not torch.equal(got.double(), ref):
            raise BoundError(f"{where}: not bitwise the maximum of its 3x3 window (stride {stride}, padding {padding})")
        return iw._nchw(got)

    def gap(self, where, x):
        r = self._take(where, "global_avgpool", x)
        ref, bound = fb.global_avgpool_ref(r.x)
        self.check.within("global_avgpool_f32", r.out, ref, bound)
        return r.out.view(r.out.shape[0], -1, 1, 1)

    def judge_packs(self):
        seen = set()
        for r in self.packs:
            if r.name is None or r.name in seen:
                raise BoundError(f"gconv_pack: a launch that is not the one pack of a conv layer ({r.name})")
            seen.add(r.name)
            dev = r.out.w.device
            bn = tuple(self.sd[f"{r.name}.bn.{k}"].to(dev) for k in ("weight", "bias", "running_mean", "running_var"))
            judge_pack_f32(self.check, r.out, self.sd[r.name + ".conv.weight"].to(dev), bn, 1e-3)
            r.judged = True
            self.judged["gconv_pack"] = self.judged.get("gconv_pack", 0) + 1
        return seen

    def judge_taps(self, outs, outputs, output_blocks):
        assert len(outputs) == len(output_blocks)
        k = 0
        for o, b in zip(outputs, sorted(output_blocks)):
            if b == 3:
                if not torch.equal(o, outs[3]):
                    raise BoundError("block 3: the returned pool3 features are not the global average pool's output")
                continue
            r = self._take(f"tap{k}", "nhwc_to_nchw", outs[b])
            k += 1
            if r.out.dtype != torch.float32 or not r.out.is_contiguous() or not torch.equal(r.out, iw._nchw(r.x)) or not torch.equal(o, r.out):
                raise BoundError(f"block {b}: the NCHW conversion is not bitwise its input")

    def complete(self, recorder):
        left = [(r.op, r.name) for r in recorder.records if not r.judged]
        if left:
            raise BoundError(f"launches the walk did not judge: {left}")
        for op in LAUNCH:
            if recorder.count(op) != self.judged.get(op, 0):
                raise BoundError(f"{op}: {recorder.count(op)} launches recorded, {self.judged.get(op, 0)} judged")
        convs = sorted(n for n in self.visited if n in self.convs)
        if convs != sorted(self.convs):
            raise BoundError(f"conv layers visited {len(convs)}, the model has {len(self.convs)}: {set(convs) ^ set(self.convs)}")
