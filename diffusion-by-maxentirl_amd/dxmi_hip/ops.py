"""Tensor-level wrappers over the C-ABI.  torch is used only for device memory and streams.

Activations are torch.bfloat16 NHWC tensors of shape [N, H, W, C]; network edges are fp32 NCHW.
Every function launches asynchronously on torch's current stream and allocates its output with
torch.empty unless `out=` is given (pass `out=` inside hipGraph capture to keep addresses fixed).
"""
import ctypes
import math
import os

import torch

from . import _lib
from . import graph as _graph
from ._lib import ConvDesc, check, load

ACT_NONE, ACT_LEAKY02, ACT_RELU, ACT_SILU = 0, 1, 2, 3
IN_NHWC_BF16, IN_NCHW_F32_K27 = 0, 1
OUT_NHWC_BF16, OUT_NCHW_F32 = 0, 1


# torch.cuda.current_stream() costs ~9 us of Python per call (device-index and availability checks, a Stream object) and sits in
# front of every launch: a train step spent 14 ms of its 57 ms of host time there (tools/host_profile.py).  The raw handle of the
# same stream comes from two C calls.
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    if _RAW_STREAM is not None and _GET_DEVICE is not None:
        return ctypes.c_void_p(_RAW_STREAM(_GET_DEVICE()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tree_fingerprint(module):
    """Cheap identity of a module tree: changes when a submodule is added, removed or replaced anywhere below `module`."""
    fp, stack = [], [module]
    while stack:
        m = stack.pop()
        subs = m._modules
        fp.append(id(subs))
        fp.append(len(subs))
        for c in subs.values():
            if c is not None:
                fp.append(id(c))
                stack.append(c)
    return tuple(fp)


def fast_parameters(module):
    """module.parameters() without nn.Module's name-building / de-duplication machinery (a U-Net's `tuple(... for p in
    net.parameters())` was ~1 ms of Python per forward): the submodules are listed once, their `_parameters` dictionaries are read
    live, in the order `parameters()` yields.  The cached list is dropped when the module tree changes: the root's direct children
    are compared on EVERY call (count + identities, ~1 us), the whole tree's fingerprint (~30 us for the U-Net) on every 64th —
    a submodule replaced deeper down is seen within 64 calls, one replaced at the root at once — and on first use the result is
    checked against `module.parameters()` (a parameter shared between two modules would be yielded twice here: de-duplicated
    by identity)."""
    cache = module.__dict__.get("_dxmi_param_modules")
    if cache is not None:
        cache[2] += 1
        subs = module._modules
        if len(subs) != len(cache[4]) or any(a is not b for a, b in zip(subs.values(), cache[4])):
            cache = None
        elif cache[2] & 63 == 0 and _tree_fingerprint(module) != cache[1]:
            cache = None
    if cache is None:
        # every submodule, also those without parameters today: the samplers register `log_betas` on a net after construction
        mods = list(module.modules())
        cache = [mods, _tree_fingerprint(module), 0, False, tuple(module._modules.values())]
        module.__dict__["_dxmi_param_modules"] = cache
        seen = set()
        flat = [prm for m in mods for prm in m._parameters.values() if prm is not None and not (id(prm) in seen or seen.add(id(prm)))]
        cache[3] = len(flat) != sum(1 for m in mods for prm in m._parameters.values() if prm is not None)      # shared parameters
        assert len(flat) == sum(1 for _ in module.parameters()), "fast_parameters: module tree walk disagrees with module.parameters()"
    if cache[3]:
        seen = set()
        for m in cache[0]:
            for prm in m._parameters.values():
                if prm is not None and id(prm) not in seen:
                    seen.add(id(prm))
                    yield prm
        return
    for m in cache[0]:
        for prm in m._parameters.values():
            if prm is not None:
                yield prm


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.DxmiError("dxmi_hip ops need device tensors: the HIP library is the only compute path "
                                 "(the CPU oracle lives under oracle/ and is test infrastructure)")


def device_check():
    check(load().dxmi_device_check(), "dxmi_device_check")


def set_tuning(name, value):
    """Kernel-selection knob of the library (include/dxmi_hip.h: dxmi_set_tuning); returns the previous value."""
    old = get_tuning(name)
    check(load().dxmi_set_tuning(name.encode(), int(value)), "dxmi_set_tuning")
    _STATS_P.clear()          # per-shape answers of the selection queries (statistics partials, fused GroupNorm) depend on the knobs
    return old


_TUNING_SAVED = []


def tune_for_throughput(on=True):
    """Training entry points: route convs whose 256-pixel-tile grid leaves most CUs idle (small per-GPU batches) to kernels with
    smaller tiles.  Off (the library default), every layer shape runs one kernel whatever the batch size, which keeps an image's
    result bitwise independent of the batch it rides in (generation scripts, parity tests).  `tune_for_throughput(False)`
    RESTORES the values that were in effect before the matching `tune_for_throughput(True)` (environment overrides such as
    DXMI_CONV_SM / DXMI_CONV_WS_MIN_TILES survive a train leg); `with ops.throughput_tuning():` does both."""
    if on:
        _TUNING_SAVED.append((set_tuning("conv_ws_min_tiles", 96), set_tuning("conv_sm_mask", 13)))
    elif _TUNING_SAVED:
        ws, sm = _TUNING_SAVED.pop()
        set_tuning("conv_ws_min_tiles", ws)
        set_tuning("conv_sm_mask", sm)


class throughput_tuning:
    """`with ops.throughput_tuning():` — tune_for_throughput(True) inside, the previous knob values restored on exit."""

    def __enter__(self):
        tune_for_throughput(True)
        return self

    def __exit__(self, *exc):
        tune_for_throughput(False)
        return False


def get_tuning(name):
    v = ctypes.c_int(0)
    check(load().dxmi_get_tuning(name.encode(), ctypes.byref(v)), "dxmi_get_tuning")
    return v.value


def conv_ws_clock_ghz():
    """Shader clock (GHz) the chip held during the most recent conv_ws_kernel launch (dxmi_conv_ws_last_clock), or None when the
    kernel has not run / the counters did not advance.  Synchronises."""
    buf = (ctypes.c_uint64 * 4)()
    check(load().dxmi_conv_ws_last_clock(buf), "dxmi_conv_ws_last_clock")
    dc, dr = int(buf[2]) - int(buf[0]), int(buf[3]) - int(buf[1])
    return (dc / dr) * 0.1 if dc > 0 and dr > 0 else None


class PackedConvWeight:
    """bf16 MFMA-fragment-ordered copy of an OIHW fp32 weight (transpose_flip: packed as the data-gradient weight of that conv)."""

    __slots__ = ("buf", "Cout", "Cin", "ksize", "k27", "transpose_flip")

    def __init__(self, buf, Cout, Cin, ksize, k27, transpose_flip=False):
        self.buf, self.Cout, self.Cin, self.ksize, self.k27 = buf, Cout, Cin, ksize, k27
        self.transpose_flip = bool(transpose_flip)


_PACK_BATCH = None
PACK_GENERATION = 0         # bumped by every full build of a packed-weight set (dxmi_hip/packs.py); dxmi_hip/graph.py re-captures


class pack_batch:
    """`with ops.pack_batch():` — every pack_conv_weight() inside allocates its destination and is DEFERRED; on exit all of
    them run as a few multi-tensor launches (dxmi_pack_conv_weights), and `.plan` is the PackPlan that ran them (None when nothing
    was deferred).  The nets' packed-weight sets are built in one (dxmi_hip/packs.py): after an optimiser step ~60 (CIFAR U-Net)
    to ~330 (ImageNet-64 EDM net) weights are refreshed."""

    def __enter__(self):
        global _PACK_BATCH
        self.plan = None
        self.outer = _PACK_BATCH is not None or os.environ.get("DXMI_PACK_BATCH", "1") == "0"     # (=0: one launch per weight, A/B timing)
        if not self.outer:
            _PACK_BATCH = []
        return self

    def __exit__(self, *exc):
        global _PACK_BATCH
        if self.outer:
            return False
        items, _PACK_BATCH = _PACK_BATCH, None
        if items and exc[0] is None:
            arr = (_lib.PackItem * len(items))()
            for i, (w, out, Cout, Cin, k, flip, k27) in enumerate(items):
                arr[i].w, arr[i].dst = w.data_ptr(), out.data_ptr()
                arr[i].Cout, arr[i].Cin, arr[i].ksize, arr[i].transpose_flip, arr[i].k27 = Cout, Cin, k, int(flip), int(k27)
            self.plan = PackPlan(arr, items)
            self.plan.replay()
        return False


def pack_tensor(shape, dtype, device):
    """The destination buffer of a pack (a plain allocation; no launch)."""
    return torch.empty(shape, dtype=dtype, device=device)


PACK_PLAN_REPLAY = os.environ.get("DXMI_PACK_PLAN", "1") != "0"      # 0: rebuild descriptors and buffers at every re-pack (A/B timing)


class PackPlan:
    """The descriptor array of one pack_batch, replayable: after an optimiser step the SAME fp32 sources (parameters updated in
    place: same addresses) are packed again into the SAME fragment buffers with one call — building the ~330 descriptors and
    buffers of the ImageNet-64 net anew was 3.6 ms of host time per pack, twenty times per EDM train step.  Holds the source and
    destination tensors alive; the caller checks that the parameters have not moved before replaying."""

    def __init__(self, arr, items):
        self.arr, self.items = arr, items

    def replay(self):
        check(load().dxmi_pack_conv_weights(self.arr, len(self.items), _stream()), "dxmi_pack_conv_weights")


def pack_conv_weight(w, transpose_flip=False, k27=False, out=None):
    """w: fp32 [Cout, Cin, k, k] (or [M, K] for a linear layer) on the device.  Inside `with pack_batch():` the launch is
    deferred to the end of the block (the returned buffer is filled then)."""
    _need_cuda(w)
    if w.dim() == 2:
        w = w[:, :, None, None]
    w = w.detach().contiguous().float()
    O, I, k, _ = w.shape
    Cout, Cin = (I, O) if transpose_flip else (O, I)
    lib = load()
    nbytes = lib.dxmi_packed_conv_weight_bytes(Cout, Cin, k, int(k27))
    if out is None:
        out = pack_tensor(nbytes, torch.uint8, w.device)
    assert out.numel() == nbytes
    if _PACK_BATCH is not None:
        _PACK_BATCH.append((w, out, Cout, Cin, k, transpose_flip, k27))      # (w is kept alive until the launch)
    else:
        check(lib.dxmi_pack_conv_weight(_ptr(w), _ptr(out), Cout, Cin, k, int(transpose_flip), int(k27), _stream()),
              "dxmi_pack_conv_weight")
    return PackedConvWeight(out, Cout, Cin, k, k27, transpose_flip)


class BlockStats:
    """GroupNorm block statistics of an NHWC bf16 activation: fp32 [N, P, C/2, 2] = (sum, sum of squares) of the stored
    values per channel PAIR, over the pixels of partial p of the image (dxmi_conv_desc.gn_stats / dxmi_gn_block_stats).
    Travels with the tensor it describes; `groupnorm_silu(..., stats=...)` then runs as one streaming read + write."""

    __slots__ = ("buf", "P", "normed")

    def __init__(self, buf, P):
        self.buf, self.P = buf, P
        self.normed = None      # conv2d(norm_next=...): the GroupNorm(+SiLU) of the tensor, written by its producer instead of it


_STATS_P = {}
GN_FLAG_WS = 4      # dxmi_conv_desc.gn_flags bit 2: the conv_ws family's fused GroupNorm output may serve the request


def conv2d(x, pw, *, in1=None, bias=None, addvec=None, residual=None, stride=1, pad=None, pad_br=None, upsample=False,
           act=ACT_NONE, out=None, out_nchw_f32=False, variant=0, mask_src=None, mask_slope=0.0, want_stats=False, fuse_gn=None,
           gn_ws=False, norm_next=None):
    """x: NHWC bf16 [N,IH,IW,C0] (or NCHW fp32 [N,3,H,W] when pw.k27).
    want_stats: return (out, BlockStats | None) — the output's GroupNorm block statistics written by the conv's own epilogue
    where the selected kernel can (None otherwise: the caller falls back to block_stats() or the one-pass GroupNorm).
    fuse_gn = (gamma, beta, groups, eps, silu, keep_raw): return (out | None, y | None) with y = GroupNorm(+SiLU)(out) written
    by the conv's own epilogue where the selected kernel can (4x4 maps; y None otherwise: the caller normalises `out` itself);
    keep_raw False drops the un-normalised tensor (out None) when y is produced.
    gn_ws (with fuse_gn, keep_raw False): also take the wave-specialised 3x3 kernel's fused output (GN_FLAG_WS: 16x16 maps; y is
    bitwise groupnorm_silu(out, stats=...) of the two-launch path).
    norm_next = (gamma, beta, groups, eps, silu), with want_stats: the GroupNorm that is the ONLY reader of the output.  Where the
    wave-specialised kernel can (GN_FLAG_WS), it writes the statistics and, instead of the raw output, that normalisation: the
    call returns (None, BlockStats) with BlockStats.normed = y; everywhere else it is the plain want_stats call."""
    _need_cuda(x, in1, bias, addvec, residual, out)
    k = pw.ksize
    if pad is None:
        pad = k // 2
    d = ConvDesc()
    if pw.k27:
        N, _, IH, IW = x.shape
        C0, C1 = 3, 0
        assert x.dtype == torch.float32 and x.is_contiguous()
    else:
        N, IH, IW, C0 = x.shape
        C1 = in1.shape[3] if in1 is not None else 0
        assert x.dtype == torch.bfloat16 and x.is_contiguous()
        assert in1 is None or (in1.dtype == torch.bfloat16 and in1.is_contiguous() and in1.shape[:3] == x.shape[:3])
        assert C0 + C1 == pw.Cin, f"conv2d: input channels {C0}+{C1} != packed Cin {pw.Cin}"
    VIH, VIW = (IH * 2, IW * 2) if upsample else (IH, IW)
    if pad_br is None:
        pad_br = pad
    # pad = top/left zeros, pad_br = bottom/right zeros (DDPM Downsample: pad=0, pad_br=1, k3 s2;
    # unet_small.py:69-76)
    OH, OW = (VIH + pad + pad_br - k) // stride + 1, (VIW + pad + pad_br - k) // stride + 1
    Cout = pw.Cout
    if out is None:
        if out_nchw_f32:
            out = torch.empty((N, Cout, OH, OW), dtype=torch.float32, device=x.device)
        else:
            out = torch.empty((N, OH, OW, Cout), dtype=torch.bfloat16, device=x.device)
    d.in0, d.in1, d.wpacked = x.data_ptr(), (in1.data_ptr() if in1 is not None else None), pw.buf.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    if addvec is not None:
        assert addvec.dtype == torch.float32 and addvec.stride(-1) == 1
        d.addvec = addvec.data_ptr()
        d.addvec_ld = addvec.stride(0) if addvec.dim() == 2 else 0
    else:
        d.addvec, d.addvec_ld = None, 0
    if residual is not None:
        assert residual.dtype == torch.bfloat16 and residual.is_contiguous() and tuple(residual.shape) == (N, OH, OW, Cout)
    d.residual = residual.data_ptr() if residual is not None else None
    d.out = out.data_ptr()
    d.N, d.IH, d.IW, d.C0, d.C1, d.OH, d.OW, d.Cout = N, IH, IW, C0, C1, OH, OW, Cout
    d.ksize, d.stride, d.pad, d.upsample, d.act = k, stride, pad, int(upsample), act
    d.in_mode = IN_NCHW_F32_K27 if pw.k27 else IN_NHWC_BF16
    d.out_mode = OUT_NCHW_F32 if out_nchw_f32 else OUT_NHWC_BF16
    d.variant = variant
    if mask_src is not None:
        assert mask_src.dtype == torch.bfloat16 and mask_src.is_contiguous() and tuple(mask_src.shape) == (N, OH, OW, Cout)
    d.mask_src = mask_src.data_ptr() if mask_src is not None else None
    d.mask_slope = float(mask_slope)
    d.gn_stats = None
    stats = None
    if want_stats and not out_nchw_f32 and variant == 0:
        key = (N, IH, IW, C0, C1, OH, OW, Cout, k, stride, pad, int(upsample), act, d.in_mode, residual is not None, mask_src is not None)
        P = _STATS_P.get(key)
        if P is None:
            P = _STATS_P[key] = int(load().dxmi_conv2d_gn_stats_partials(ctypes.byref(d)))
        if P > 0:
            stats = BlockStats(torch.empty((N, P, Cout // 2, 2), dtype=torch.float32, device=x.device), P)
            d.gn_stats = stats.buf.data_ptr()
    d.gn_out, y = None, None
    assert norm_next is None or (fuse_gn is None and want_stats)
    fuse = fuse_gn if norm_next is None else (tuple(norm_next) + (False,) if stats is not None else None)
    if fuse is not None:
        assert not want_stats or norm_next is not None
        gamma, beta, groups, eps, silu, keep_raw = fuse
        ws_too = bool(gn_ws) or norm_next is not None
        d.gn_groups = groups
        d.gn_flags = int(bool(silu)) | (0 if keep_raw else 2) | (GN_FLAG_WS if ws_too else 0)
        key = ("gn", N, IH, IW, C0, C1, OH, OW, Cout, k, stride, pad, int(upsample), act, d.in_mode, d.out_mode, variant,
               residual is not None, mask_src is not None, groups, bool(keep_raw), ws_too, norm_next is not None)
        ok = _STATS_P.get(key)
        if ok is None:
            ok = int(load().dxmi_conv2d_gn_fuse_supported(ctypes.byref(d)))
            if ok and norm_next is not None:      # ... and only that kernel's: it writes the statistics beside the fused output
                d.gn_flags &= ~GN_FLAG_WS
                ok = int(not load().dxmi_conv2d_gn_fuse_supported(ctypes.byref(d)))
                d.gn_flags |= GN_FLAG_WS
            _STATS_P[key] = ok
        if ok:
            assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == Cout and beta.numel() == Cout
            y = torch.empty((N, OH, OW, Cout), dtype=torch.bfloat16, device=x.device)
            d.gn_out, d.gn_gamma, d.gn_beta, d.gn_eps = y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps)
    if PROFILER is not None:
        PROFILER.launch_conv(d)
    else:
        check(load().dxmi_conv2d_fwd(ctypes.byref(d), _stream()), "dxmi_conv2d_fwd")
    if stats is not None and stats.P > MAX_APPLY_PARTIALS:
        stats = fold_stats(stats)
    if fuse_gn is not None:
        return (out if (y is None or fuse_gn[5]) else None), y
    if y is not None:           # norm_next was served: the raw tensor does not exist
        stats.normed = y
        return None, stats
    return (out, stats) if want_stats else out


class OpProfiler:
    """Brackets kernel launches with HIP events on the launch stream (bench.py roofline leg) and records, per launch,
    (class, kernel name, algorithmic FLOPs, algorithmic bytes, start, end).  Classes: "conv3x3" / "conv1x1" / "conv_stem" /
    "conv_other" (by dxmi_conv2d_kernel_id), "groupnorm", "attention", "sampler_step", "wgrad", "groupnorm_bwd", "optimizer"."""

    def __init__(self):
        self.records = []

    def bracket(self, cls, name, flops, nbytes, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.records.append((cls, name, float(flops), float(nbytes), e0, e1))
        return out

    def launch_conv(self, d):
        lib = load()
        kid = lib.dxmi_conv2d_kernel_id(ctypes.byref(d))
        cin = 27 if d.in_mode == IN_NCHW_F32_K27 else (d.C0 + d.C1) * d.ksize * d.ksize
        flops = 2.0 * d.N * d.OH * d.OW * d.Cout * cin
        in_b = d.N * d.IH * d.IW * (d.C0 + d.C1) * (4 if d.in_mode == IN_NCHW_F32_K27 else 2)
        out_b = d.N * d.OH * d.OW * d.Cout * (4 if d.out_mode == OUT_NCHW_F32 else 2)
        res_b = out_b if d.residual else 0
        if d.gn_out:                                  # fused GroupNorm: the normalised tensor out, the raw one only if kept
            res_b += out_b if not (d.gn_flags & 2) else 0
        w_b = d.Cout * cin * 2
        cls = "conv_other" if kid >= 600000 else "conv1x1" if kid >= 500000 else "conv3x3" if kid >= 400000 else "conv_stem" if kid >= 300000 else ("conv1x1" if kid >= 200000 else ("conv3x3" if kid >= 30000 else "conv_other"))
        if kid == 400008 and d.gn_out:
            kid = 400009                                  # conv_ws8_kernel<true> (bench.py kernel_name)
        if kid == 400016 and d.gn_out:
            kid = 400116                                  # conv_ws_gn_kernel<16>: GroupNorm time inside (printed as conv_ws_kernel<116>)
        self.bracket(cls, kid, flops, in_b + out_b + res_b + w_b,
                     lambda: check(lib.dxmi_conv2d_fwd(ctypes.byref(d), _stream()), "dxmi_conv2d_fwd"))

    def summary(self):
        """(class, name) -> dict(launches, ms, flops, bytes); call after torch.cuda.synchronize()."""
        out = {}
        for cls, name, fl, by, e0, e1 in self.records:
            s = out.setdefault((cls, name), {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            s["launches"] += 1
            s["ms"] += e0.elapsed_time(e1)
            s["flops"] += fl
            s["bytes"] += by
        return out


PROFILER = None


def _prof(cls, name, flops, nbytes, fn):
    return fn() if PROFILER is None else PROFILER.bracket(cls, name, flops, nbytes, fn)


_WS = {}


def _workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream): split-K partials, column sums, generic-GroupNorm partials.  Keyed by
    the launch stream so that work overlapped on a second stream never shares it; a buffer captured into a hipGraph is
    never re-allocated (growth during capture raises: size it with one eager call first)."""
    if _graph.capturing():
        # inside a StepGraph capture: a scratch tensor of its own from the graph's private pool (stream-ordered reuse is the
        # allocator's business there; the address is fixed for every replay)
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device)
    key = (str(device), stream.cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None and torch.cuda.is_current_stream_capturing():
            raise _lib.DxmiError("dxmi_hip workspace would have to grow during hipGraph capture: run the step once eagerly first")
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


WGRAD_SIDE_STREAM = os.environ.get("DXMI_WGRAD_STREAM", "0") == "1"      # measured slower on gfx950 (B = 32: 35.9 -> 38.9 ms per train step, B = 256: 90.0 -> 92.5): off unless asked for


class wgrad_branch:
    """`with ops.wgrad_branch(reads):` — inside a StepGraph capture the block's launches go to the graph's SIDE stream (a parallel
    branch behind everything captured so far: StepGraph.fork_side); outside a capture, or with DXMI_WGRAD_STREAM=0, a no-op.
    Weight gradients have no consumer until the optimiser: the backward's data-gradient chain need not wait for them.
    `ops.wgrad_join()` before their first consumer on the main stream (the end of every autograd backward here)."""

    def __init__(self, reads=()):
        self.reads, self.ctx = reads, None

    def __enter__(self):
        cap = _graph.current()
        if cap is not None and WGRAD_SIDE_STREAM and PROFILER is None:
            self.ctx = torch.cuda.stream(cap.fork_side(self.reads))
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


def wgrad_join():
    cap = _graph.current()
    if cap is not None:
        cap.join_side()


def conv2d_wgrad(x, dy, ksize, **kw):
    """Weight gradient of a conv (see _conv2d_wgrad); inside a captured step it runs as a parallel branch (wgrad_branch)."""
    with wgrad_branch((x, dy, kw.get("in1"), kw.get("out"))):
        return _conv2d_wgrad(x, dy, ksize, **kw)


def _conv2d_wgrad(x, dy, ksize, *, in1=None, pad=None, stride=1, upsample=False, out=None, accumulate=False, with_bias=False):
    """Weight gradient of a conv: x [N,IH,IW,C0] (| in1), dy [N,OH,OW,Cout] NHWC bf16 ->
    fp32 OIHW [Cout, C0+C1, k, k] (written, or added when accumulate).  with_bias: also the bias gradient
    (column sums of dy) from the same launch -> (dw, db)."""
    _need_cuda(x, in1, dy, out)
    N, IH, IW, C0 = x.shape
    C1 = in1.shape[3] if in1 is not None else 0
    _, OH, OW, Cout = dy.shape
    assert x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16 and x.is_contiguous() and dy.is_contiguous()
    if pad is None:
        pad = ksize // 2
    if out is None:
        out = torch.empty((Cout, C0 + C1, ksize, ksize), dtype=torch.float32, device=x.device)
        accumulate = False
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (Cout, C0 + C1, ksize, ksize)
    lib = load()
    ws = _workspace(lib.dxmi_conv2d_wgrad_workspace_bytes(N, OH, OW, C0 + C1, Cout, ksize), x.device)
    fl = 2.0 * N * OH * OW * Cout * (C0 + C1) * ksize * ksize
    by = 2.0 * (x.numel() + (in1.numel() if in1 is not None else 0) + dy.numel()) + 4.0 * out.numel()
    if with_bias:
        db = torch.empty(Cout, dtype=torch.float32, device=x.device)
        _prof("wgrad", f"k{ksize}", fl, by, lambda: check(
            lib.dxmi_conv2d_wgrad_bias(_ptr(x), C0, _ptr(in1), C1, _ptr(dy), _ptr(out), _ptr(db), _ptr(ws), N, IH, IW, OH, OW,
                                       Cout, ksize, stride, pad, int(upsample), 0, _stream()), "dxmi_conv2d_wgrad_bias"))
        return out, db
    _prof("wgrad", f"k{ksize}", fl, by, lambda: check(
        lib.dxmi_conv2d_wgrad(_ptr(x), C0, _ptr(in1), C1, _ptr(dy), _ptr(out), _ptr(ws), N, IH, IW, OH, OW, Cout, ksize,
                              stride, pad, int(upsample), int(accumulate), _stream()), "dxmi_conv2d_wgrad"))
    return out


WGRAD_FAMILIES = {0: "b128_1x1", 1: "ws3", 2: "ws1", 3: "reg3_pf", 4: "reg3", 5: "reg1_pf", 6: "reg1"}
WGRAD_REDUCES = {0: "taps4", 1: "taps16", 2: "flat4", 3: "flat16"}
WGRAD_TILE_PIXELS = {"b128_1x1": 64}          # every other family: 128-pixel tiles


def conv2d_wgrad_plan(N, IH, IW, OH, OW, C0, C1, Cout, ksize, stride=1, pad=None, upsample=False):
    """The kernel choice of dxmi_conv2d_wgrad for a shape (dxmi_conv2d_wgrad_plan: the launch decides through the same function)
    -> dict(family, S, PT, reduce, tile_px); split s of the S sums the pixel tiles s, s + S, ... < PT.  Needs no device."""
    if pad is None:
        pad = ksize // 2
    out = (ctypes.c_int32 * 4)()
    check(load().dxmi_conv2d_wgrad_plan(N, IH, IW, OH, OW, C0, C1, Cout, ksize, stride, pad, int(bool(upsample)), out),
          "dxmi_conv2d_wgrad_plan")
    fam = WGRAD_FAMILIES[out[0]]
    return {"family": fam, "S": out[1], "PT": out[2], "reduce": WGRAD_REDUCES[out[3]], "tile_px": WGRAD_TILE_PIXELS.get(fam, 128)}


def groupnorm_generic_bwd_plan(N, HW, C):
    """Launch form of groupnorm_generic_bwd for the shape under the current knobs: 0 = reduce + apply launches, 8 / 16 = the
    one-launch form (dxmi_groupnorm_generic_bwd_plan; the device's CU count enters its residency guard)."""
    return int(load().dxmi_groupnorm_generic_bwd_plan(N, HW, C))


def colsum(x2d, out=None, accumulate=False):
    """Column sums of a bf16 tensor viewed as [P, C] -> fp32 [C] (bias gradients)."""
    _need_cuda(x2d, out)
    C = x2d.shape[-1]
    P = x2d.numel() // C
    assert x2d.dtype == torch.bfloat16 and x2d.is_contiguous()
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=x2d.device)
        accumulate = False
    ws = _workspace(max(256, (P + 511) // 512) * C * 4, x2d.device)
    check(load().dxmi_colsum_bf16(_ptr(x2d), _ptr(out), _ptr(ws), P, C, int(accumulate), _stream()), "dxmi_colsum_bf16")
    return out


def colsum_f32(x):
    """fp32 [B, N, C] (or [N, C]) -> [B, C] ([C]): sums over N in a fixed order (one launch; torch's reduce took 14 us)."""
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    B, (N, C) = (x.shape[0] if x.dim() == 3 else 1), x.shape[-2:]
    out = torch.empty((B, C) if x.dim() == 3 else (C,), dtype=torch.float32, device=x.device)
    check(load().dxmi_colsum_f32(_ptr(x), _ptr(out), B, N, C, _stream()), "dxmi_colsum_f32")
    return out


def colsum_per_image(x):
    """x [N,H,W,C] bf16 -> [N,C] fp32 sums over H*W."""
    _need_cuda(x)
    N, H, W, C = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    check(load().dxmi_colsum_blocks_bf16(_ptr(x), _ptr(out), N * H * W, C, H * W, _stream()), "dxmi_colsum_blocks_bf16")
    return out


def value_head_pgrad(s, w, b, dy, ow=None):
    """Parameter gradients of the value head in one launch (dxmi_value_head_pgrad): s [N, C] relu-sum features, w [C], b [1], dy [N],
    ow: the out_scale weight (device scalar) or None -> fp32 [C + 3] = d linear.weight | d linear.bias | d out_scale.weight |
    d out_scale.bias."""
    _need_cuda(s, w, b, dy, ow)
    N, C = s.shape
    assert s.dtype == torch.float32 and s.is_contiguous() and dy.dtype == torch.float32 and dy.is_contiguous() and dy.numel() == N
    out = torch.empty(C + 3, dtype=torch.float32, device=s.device)
    check(load().dxmi_value_head_pgrad(_ptr(s), _ptr(w), _ptr(b), _ptr(dy), _ptr(ow), _ptr(out), N, C, _stream()), "dxmi_value_head_pgrad")
    return out


def td_gather_cost(traj2d, state_rows, beta, *, next_rows=None, next_dense=None, out_pair):
    """One TD step's data (dxmi_td_gather_cost): out_pair [2B, ...] receives [next_state | state] gathered from the ring's trajectory
    block traj2d [rows, CHW] (INT path), returns the running cost [B] = mean_CHW (x' - x)^2 / (2 beta); beta: device scalar."""
    _need_cuda(traj2d, state_rows, beta, next_rows, next_dense, out_pair)
    B = state_rows.numel()
    CHW = traj2d.shape[1]
    assert traj2d.dtype == torch.float32 and traj2d.is_contiguous() and state_rows.dtype == torch.int64 and state_rows.is_contiguous()
    assert out_pair.dtype == torch.float32 and out_pair.is_contiguous() and out_pair.numel() == 2 * B * CHW
    assert beta.dtype == torch.float32 and beta.numel() == 1
    assert next_rows is None or (next_rows.dtype == torch.int64 and next_rows.is_contiguous() and next_rows.numel() == B)
    cost = torch.empty(B, dtype=torch.float32, device=traj2d.device)
    flat = out_pair.view(2 * B, CHW)
    _prof("replay_gather", f"td_row{CHW * 4}", 0.0, 16.0 * B * CHW, lambda: check(
        load().dxmi_td_gather_cost(_ptr(traj2d), _ptr(state_rows), _ptr(next_rows), _ptr(next_dense), _ptr(beta), _ptr(flat[:B]),
                                   _ptr(flat[B:]), _ptr(cost), B, CHW, traj2d.shape[0], _stream()), "dxmi_td_gather_cost"))
    return cost


def td_loss(v, cost, extra=None):
    """mse(v[B:], (v[:B] + extra).detach()) of one TD step (dxmi_td_loss) -> (d loss / d v [2B] with zeros in the target half,
    logs fp32 [3] = (loss, mean v(x_t), mean running cost)); extra: device scalar or None."""
    _need_cuda(v, cost, extra)
    B = cost.numel()
    assert v.dtype == torch.float32 and v.is_contiguous() and v.numel() == 2 * B and cost.dtype == torch.float32 and cost.is_contiguous()
    grad = torch.empty(2 * B, dtype=torch.float32, device=v.device)
    logs = torch.empty(3, dtype=torch.float32, device=v.device)
    check(load().dxmi_td_loss(_ptr(v), _ptr(cost), _ptr(extra), _ptr(grad), _ptr(logs), B, _stream()), "dxmi_td_loss")
    return grad, logs


def pool_act_bwd(dout, act_out, pool, slope, out=None):
    _need_cuda(dout, act_out, out)
    N, OH, OW, C = dout.shape
    H, W = (OH * 2, OW * 2) if pool else (OH, OW)
    assert dout.dtype == torch.bfloat16 and dout.is_contiguous() and act_out.shape == dout.shape and act_out.is_contiguous()
    if out is None:
        out = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=dout.device)
    check(load().dxmi_pool_act_bwd(_ptr(dout), _ptr(act_out), _ptr(out), N, H, W, C, int(pool), float(slope), _stream()),
          "dxmi_pool_act_bwd")
    return out


def value_head_bwd(feat, w, dy):
    """feat [N,H,W,C] bf16, w [C] fp32, dy [N] fp32 -> (dfeat bf16 like feat, s [N,C] fp32)."""
    _need_cuda(feat, w, dy)
    N, H, W, C = feat.shape
    dfeat = torch.empty_like(feat)
    s = torch.empty((N, C), dtype=torch.float32, device=feat.device)
    check(load().dxmi_value_head_bwd(_ptr(feat), _ptr(w), _ptr(dy), _ptr(dfeat), _ptr(s), N, H * W, C, _stream()),
          "dxmi_value_head_bwd")
    return dfeat, s


def groupnorm_silu_bwd(x, dy, gamma, beta, *, in1=None, add0=None, add1=None, groups=32, eps=1e-6, silu=True):
    """-> (dx0, dx1 or None, dgamma [C], dbeta [C])."""
    _need_cuda(x, in1, dy, add0, add1, gamma, beta)
    N, H, W, C0 = x.shape
    C1 = in1.shape[3] if in1 is not None else 0
    C = C0 + C1
    assert dy.dtype == torch.bfloat16 and dy.is_contiguous() and tuple(dy.shape) == (N, H, W, C)
    # 12 channels per group on the large maps (the 384-channel concat inputs of the CIFAR net's up path): the register-resident kernel
    # slices them badly (414 us at 32x32, 101 us at 16x16, B = 256) and the generic three-launch path is ahead (285 / 79 us:
    # tools/gn_bwd_time.py); every other shape of the net is faster on the resident kernel.  Only the MEASURED case is routed away
    # (20 / 28 / 36 ... channels per group stay where they were)
    slow_resident = (C // groups) == 12 and H * W >= 256
    if slow_resident or not load().dxmi_groupnorm_silu_bwd_supported(C0, C1, H * W, groups):
        # shapes the register-resident backward cannot slice (the forward falls back the same way): generic three-launch path
        dx0, dx1, dg, db, _ = groupnorm_generic_bwd(x, dy, gamma, beta, in1=in1, add0=add0, add1=add1, groups=groups, eps=eps, silu=silu)
        return dx0, dx1, dg, db
    dx0 = torch.empty_like(x)
    dx1 = torch.empty_like(in1) if in1 is not None else None
    part = torch.empty((2, N, C), dtype=torch.float32, device=x.device)
    nb = 2.0 * N * H * W * C * (3 + (add0 is not None))     # x, dy (+ add) in, dx out
    _prof("groupnorm_bwd", "resident", 0.0, nb, lambda: check(
        load().dxmi_groupnorm_silu_bwd(_ptr(x), C0, _ptr(in1), C1, _ptr(dy), _ptr(add0), _ptr(add1), _ptr(gamma), _ptr(beta),
                                       _ptr(dx0), _ptr(dx1), _ptr(part[0]), _ptr(part[1]), N, H * W, groups, float(eps),
                                       int(silu), _stream()), "dxmi_groupnorm_silu_bwd"))
    red = colsum_f32(part)  # [2, C]: fixed-order reduction over images
    return dx0, dx1, red[0], red[1]


def bgemm(A, B, C, M, N, K, a_strides, a_ld, a_kc, b_strides, b_ld, b_kc, c_strides, c_ld, alpha, outer, inner):
    """Raw batched bf16 GEMM (see include/dxmi_hip.h); tensors are only used for their base pointers."""
    check(load().dxmi_bgemm_bf16(_ptr(A), _ptr(B), _ptr(C), M, N, K, a_strides[0], a_strides[1], a_ld, int(a_kc), b_strides[0],
                                 b_strides[1], b_ld, int(b_kc), c_strides[0], c_strides[1], c_ld, int(C.dtype == torch.float32),
                                 float(alpha), outer, inner, _stream()), "dxmi_bgemm_bf16")
    return C


FUSED_ATTENTION_BWD = True      # A-B switch: False keeps the five-GEMM path for every head size


def attention_bwd(qkv, do, heads, scale, o=None, lse=None):
    """qkv [N,T,3C] ([q|k|v], heads = contiguous channel blocks), do [N,T,C] -> dqkv [N,T,3C] (bf16).
    o: the forward pass's attention output [N,T,C]; with it, 64-wide heads take the fused kernels (no [T,T] tensor in HBM).
    lse: what attention(want_lse=True) returned for these qkv: the fused backward skips its log-sum-exp sweep."""
    _need_cuda(qkv, do, o, lse)
    N, T, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    dev = qkv.device
    assert qkv.dtype == torch.bfloat16 and do.dtype == torch.bfloat16 and qkv.is_contiguous() and do.is_contiguous()
    if o is not None and FUSED_ATTENTION_BWD and load().dxmi_attention_bwd_supported(T, C, heads):
        assert o.dtype == torch.bfloat16 and o.is_contiguous() and o.numel() == N * T * C
        dqkv = torch.empty_like(qkv)
        ws = _workspace(max(256, load().dxmi_attention_bwd_workspace_bytes(N, T, heads)), dev)
        if lse is not None:
            assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (N, heads, T)
            _prof("attention_bwd", f"T{T}_D{D}", 14.0 * N * T * T * C, 2.0 * (2 * qkv.numel() + 2 * do.numel()) * 2, lambda: check(
                load().dxmi_attention_bwd_lse(_ptr(qkv), _ptr(o), _ptr(do), _ptr(dqkv), _ptr(lse), _ptr(ws), N, T, C, heads, float(scale),
                                              _stream()), "dxmi_attention_bwd_lse"))
            return dqkv
        _prof("attention_bwd", f"T{T}_D{D}", 16.0 * N * T * T * C, 2.0 * (2 * qkv.numel() + 2 * do.numel()) * 2, lambda: check(
            load().dxmi_attention_bwd(_ptr(qkv), _ptr(o), _ptr(do), _ptr(dqkv), _ptr(ws), N, T, C, heads, float(scale), _stream()),
            "dxmi_attention_bwd"))
        return dqkv
    S = torch.empty((N, heads, T, T), dtype=torch.float32, device=dev)
    dP = torch.empty_like(S)
    P = torch.empty((N, heads, T, T), dtype=torch.bfloat16, device=dev)
    dS = torch.empty_like(P)
    dqkv = torch.empty_like(qkv)
    q, k, v = qkv[:, :, 0:C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
    dq, dk, dv = dqkv[:, :, 0:C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:]
    qs, os_, ss = (T * C3, D), (T * C, D), (heads * T * T, T * T)
    bgemm(q, k, S, T, T, D, qs, C3, True, qs, C3, True, ss, T, scale, N, heads)          # S = scale Q K^T
    bgemm(do, v, dP, T, T, D, os_, C, True, qs, C3, True, ss, T, 1.0, N, heads)           # dP = dO V^T
    check(load().dxmi_softmax_bwd(_ptr(S), _ptr(dP), _ptr(P), _ptr(dS), N * heads * T, T, _stream()), "dxmi_softmax_bwd")
    bgemm(P, do, dv, T, D, T, ss, T, False, os_, C, False, qs, C3, 1.0, N, heads)         # dV = P^T dO
    bgemm(dS, k, dq, T, D, T, ss, T, True, qs, C3, False, qs, C3, scale, N, heads)        # dQ = scale dS K
    bgemm(dS, q, dk, T, D, T, ss, T, False, qs, C3, False, qs, C3, scale, N, heads)       # dK = scale dS^T Q
    return dqkv


MAX_APPLY_PARTIALS = 8      # more partials per image than this are folded into one before the apply pass (dxmi_gn_stats_fold)


def fold_stats(st, group=32):
    """[N, P, C/2, 2] -> [N, P', C/2, 2] with P' <= MAX_APPLY_PARTIALS: `group` consecutive partials are added per thread, in
    order; a second pass folds what is left (P > 256: the 256x256 maps of the LSUN net)."""
    while st.P > MAX_APPLY_PARTIALS:
        N, P, C2, _ = st.buf.shape
        PG = (P + group - 1) // group
        out = torch.empty((N, PG, C2, 2), dtype=torch.float32, device=st.buf.device)
        _prof("groupnorm", "fold", 0.0, 4.0 * (st.buf.numel() + out.numel()), lambda: check(
            load().dxmi_gn_stats_fold(_ptr(st.buf), _ptr(out), N, P, C2 * 2, group, _stream()), "dxmi_gn_stats_fold"))
        st = BlockStats(out, PG)
    return st


def block_stats(x):
    """GroupNorm block statistics of an activation that has none from its producer (one read of x)."""
    _need_cuda(x)
    N, H, W, C = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    lib = load()
    P = int(lib.dxmi_gn_block_stats_partials(H * W))
    st = BlockStats(torch.empty((N, P, C // 2, 2), dtype=torch.float32, device=x.device), P)
    _prof("groupnorm", "block_stats", 0.0, 2.0 * x.numel(), lambda: check(
        lib.dxmi_gn_block_stats(_ptr(x), _ptr(st.buf), N, H * W, C, _stream()), "dxmi_gn_block_stats"))
    return fold_stats(st) if P > MAX_APPLY_PARTIALS else st


GN_APPLY_SPLIT = os.environ.get("DXMI_GN_APPLY_SPLIT", "0") == "1"      # dxmi_groupnorm_apply_split: finalize launch + prologue-free apply


def groupnorm_apply(x, st, gamma, beta, *, in1=None, st1=None, groups=32, eps=1e-6, silu=True, out=None, scale_shift=None):
    """GroupNorm(+FiLM scale-shift)(+SiLU) of [x | in1] given their block statistics: one streaming read + write
    (dxmi_groupnorm_apply)."""
    _need_cuda(x, in1, gamma, beta, out, st.buf, st1.buf if st1 is not None else None, scale_shift)
    N, H, W, C0 = x.shape
    C1 = in1.shape[3] if in1 is not None else 0
    C = C0 + C1
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and (in1 is None or (in1.is_contiguous() and st1 is not None))
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C
    assert tuple(st.buf.shape) == (N, st.P, C0 // 2, 2) and (st1 is None or tuple(st1.buf.shape) == (N, st1.P, C1 // 2, 2))
    ss_ld = 0
    if scale_shift is not None:
        assert scale_shift.dtype == torch.float32 and scale_shift.stride(-1) == 1 and scale_shift.shape[1] == 2 * C
        ss_ld = scale_shift.stride(0)
    if out is None:
        out = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=x.device)
    if GN_APPLY_SPLIT:
        ab = torch.empty((N, C, 2), dtype=torch.float32, device=x.device)
        _prof("groupnorm", "apply", 0.0, 4.0 * N * H * W * C, lambda: check(
            load().dxmi_groupnorm_apply_split(_ptr(x), C0, _ptr(st.buf), st.P, _ptr(in1), C1, _ptr(st1.buf) if st1 is not None else None,
                                              st1.P if st1 is not None else 0, _ptr(gamma), _ptr(beta), _ptr(scale_shift), ss_ld, _ptr(out),
                                              _ptr(ab), N, H * W, groups, float(eps), int(silu), _stream()), "dxmi_groupnorm_apply_split"))
        return out
    _prof("groupnorm", "apply", 0.0, 4.0 * N * H * W * C, lambda: check(
        load().dxmi_groupnorm_apply(_ptr(x), C0, _ptr(st.buf), st.P, _ptr(in1), C1, _ptr(st1.buf) if st1 is not None else None,
                                    st1.P if st1 is not None else 0, _ptr(gamma), _ptr(beta), _ptr(scale_shift), ss_ld, _ptr(out),
                                    N, H * W, groups, float(eps), int(silu), _stream()), "dxmi_groupnorm_apply"))
    return out


def groupnorm_silu(x, gamma, beta, *, in1=None, groups=32, eps=1e-6, silu=True, out=None, scale_shift=None, stats=None, saved=None):
    """GroupNorm(+SiLU).  stats = (BlockStats of x, BlockStats of in1 | None): the streaming apply kernel.  saved: a list that
    receives the statistics tensor groupnorm_generic_bwd(fwd_stats=...) takes, on the streaming and the generic path.  Otherwise the
    register-resident one-pass kernel serves channels-per-group % 4 == 0 slices that fit; everything else (EDM shapes,
    scale-shift norm) goes to the generic two-kernel path."""
    _need_cuda(x, in1, gamma, beta, out, scale_shift)
    N, H, W, C0 = x.shape
    C1 = in1.shape[3] if in1 is not None else 0
    if stats is not None and stats[0] is not None and (in1 is None or stats[1] is not None) \
            and ((C0 + C1) // groups) % 2 == 0 and C0 % 8 == 0 and C1 % 8 == 0:
        if saved is not None:       # the training forward: the same sums in the generic backward's format
            saved.append(gn_blockstats_to_generic(stats[0], stats[1] if in1 is not None else None, N, H * W, C0, C1, groups))
        return groupnorm_apply(x, stats[0], gamma, beta, in1=in1, st1=stats[1] if in1 is not None else None, groups=groups,
                               eps=eps, silu=silu, out=out, scale_shift=scale_shift)
    if scale_shift is not None or not load().dxmi_groupnorm_silu_supported(C0, C1, H * W, groups):
        return groupnorm_generic(x, gamma, beta, in1=in1, groups=groups, eps=eps, silu=silu, out=out, scale_shift=scale_shift, saved=saved)
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C0 + C1
    if out is None:
        out = torch.empty((N, H, W, C0 + C1), dtype=torch.bfloat16, device=x.device)
    _prof("groupnorm", "resident", 0.0, 4.0 * N * H * W * (C0 + C1), lambda: check(
        load().dxmi_groupnorm_silu_fwd(_ptr(x), C0, _ptr(in1), C1, _ptr(gamma), _ptr(beta), _ptr(out), N, H * W,
                                       groups, float(eps), int(silu), _stream()), "dxmi_groupnorm_silu_fwd"))
    return out


def groupnorm_silu_shortcut(x, gamma, beta, pw, *, in1=None, bias=None, groups=32, eps=1e-6, silu=True, stats=None):
    """GroupNorm(+SiLU) of [x | in1] from their block statistics `stats` (groupnorm_silu's streaming path) AND the 1x1 conv pw of the
    same input (conv2d(x, pw, in1=in1, bias=bias): a ResnetBlock's nin_shortcut) in one pass over the input
    (dxmi_groupnorm_silu_shortcut) -> (y, sc), bitwise the two ops' results.  None where the pair is out of the kernel's scope:
    the caller runs the two ops."""
    _need_cuda(x, in1, gamma, beta, bias)
    if stats is None or stats[0] is None or (in1 is not None and stats[1] is None) or pw.k27 or pw.ksize != 1:
        return None
    N, H, W, C0 = x.shape
    C1 = in1.shape[3] if in1 is not None else 0
    C = C0 + C1
    if (C // groups) % 2 != 0 or C0 % 8 != 0 or C1 % 8 != 0:
        return None
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and C == pw.Cin
    assert in1 is None or (in1.dtype == torch.bfloat16 and in1.is_contiguous() and in1.shape[:3] == x.shape[:3])
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C and beta.numel() == C
    st0, st1 = stats[0], (stats[1] if in1 is not None else None)
    assert tuple(st0.buf.shape) == (N, st0.P, C0 // 2, 2) and (st1 is None or tuple(st1.buf.shape) == (N, st1.P, C1 // 2, 2))
    Cout = pw.Cout
    sc = torch.empty((N, H, W, Cout), dtype=torch.bfloat16, device=x.device)
    d = ConvDesc()
    d.in0, d.in1, d.wpacked = x.data_ptr(), (in1.data_ptr() if in1 is not None else None), pw.buf.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.out = sc.data_ptr()
    d.N, d.IH, d.IW, d.C0, d.C1, d.OH, d.OW, d.Cout = N, H, W, C0, C1, H, W, Cout
    d.ksize, d.stride, d.pad, d.upsample, d.act = 1, 1, 0, 0, ACT_NONE
    d.in_mode, d.out_mode = IN_NHWC_BF16, OUT_NHWC_BF16
    lib = load()
    key = ("gn_shortcut", N, H, W, C0, C1, Cout, groups, bias is not None)
    ok = _STATS_P.get(key)
    if ok is None:
        ok = _STATS_P[key] = int(lib.dxmi_groupnorm_silu_shortcut_supported(ctypes.byref(d), groups))
    if not ok:
        return None
    y = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=x.device)
    ab = torch.empty((N, C, 2), dtype=torch.float32, device=x.device)
    px = N * H * W
    _prof("groupnorm", "gn_shortcut", 2.0 * px * C * Cout, 2.0 * (2 * px * C + px * Cout + C * Cout), lambda: check(
        lib.dxmi_groupnorm_silu_shortcut(ctypes.byref(d), _ptr(st0.buf), st0.P, _ptr(st1.buf) if st1 is not None else None,
                                         st1.P if st1 is not None else 0, _ptr(gamma), _ptr(beta), groups, float(eps), int(silu),
                                         _ptr(y), _ptr(ab), _stream()), "dxmi_groupnorm_silu_shortcut"))
    return y, sc


def gn_blockstats_to_generic(st0, st1, N, HW, C0, C1, groups=32):
    """BlockStats of x (| in1) -> the fp32 statistics tensor groupnorm_generic_bwd(fwd_stats=...) takes (dxmi_gn_blockstats_to_generic)."""
    lib = load()
    ws = torch.empty(lib.dxmi_groupnorm_generic_workspace_bytes(N, HW, C0 + C1) // 4, dtype=torch.float32, device=st0.buf.device)
    check(lib.dxmi_gn_blockstats_to_generic(_ptr(st0.buf), st0.P, C0, _ptr(st1.buf) if st1 is not None else None, st1.P if st1 is not None else 0,
                                            C1, _ptr(ws), N, HW, groups, _stream()), "dxmi_gn_blockstats_to_generic")
    return ws


def groupnorm_generic(x, gamma, beta, *, in1=None, groups=32, eps=1e-5, silu=True, out=None, scale_shift=None, saved=None):
    """saved: a list; the forward's statistics partials (a small fp32 tensor of its own instead of the shared workspace) are
    appended to it for groupnorm_generic_bwd(fwd_stats=...), which then skips its statistics pass over the input."""
    _need_cuda(x, in1, gamma, beta, out, scale_shift)
    N, H, W, C0 = x.shape
    C1 = in1.shape[3] if in1 is not None else 0
    C = C0 + C1
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    if out is None:
        out = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=x.device)
    ss_ld = 0
    if scale_shift is not None:
        assert scale_shift.dtype == torch.float32 and scale_shift.stride(-1) == 1 and scale_shift.shape[1] == 2 * C
        ss_ld = scale_shift.stride(0)
    lib = load()
    nbytes = lib.dxmi_groupnorm_generic_workspace_bytes(N, H * W, C)
    if saved is not None:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        saved.append(ws)
    else:
        ws = _workspace(nbytes, x.device)
    _prof("groupnorm", "generic", 0.0, 4.0 * N * H * W * C, lambda: check(
        lib.dxmi_groupnorm_generic_fwd(_ptr(x), C0, _ptr(in1), C1, _ptr(gamma), _ptr(beta), _ptr(scale_shift), ss_ld, _ptr(out),
                                       _ptr(ws), N, H * W, groups, float(eps), int(silu), _stream()), "dxmi_groupnorm_generic_fwd"))
    return out


def groupnorm_generic_bwd(x, dy, gamma, beta, *, in1=None, add0=None, add1=None, groups=32, eps=1e-5, silu=True, scale_shift=None,
                          fwd_stats=None):
    """-> (dx0, dx1 | None, dgamma [C], dbeta [C], d_scale_shift [N, 2C] | None).  fwd_stats: the tensor groupnorm_generic(saved=...)
    kept for this input."""
    _need_cuda(x, in1, dy, add0, add1, gamma, beta, scale_shift, fwd_stats)
    N, H, W, C0 = x.shape
    C1 = in1.shape[3] if in1 is not None else 0
    C = C0 + C1
    assert dy.dtype == torch.bfloat16 and dy.is_contiguous() and tuple(dy.shape) == (N, H, W, C)
    dx0 = torch.empty_like(x)
    dx1 = torch.empty_like(in1) if in1 is not None else None
    g = torch.empty((2, N, C), dtype=torch.float32, device=x.device)
    ss_ld = scale_shift.stride(0) if scale_shift is not None else 0
    lib = load()
    ws = _workspace(lib.dxmi_groupnorm_generic_bwd_workspace_bytes(N, H * W, C), x.device)
    if fwd_stats is not None:
        assert fwd_stats.dtype == torch.float32 and fwd_stats.numel() * 4 == lib.dxmi_groupnorm_generic_workspace_bytes(N, H * W, C)
    check(lib.dxmi_groupnorm_generic_bwd_saved(_ptr(x), C0, _ptr(in1), C1, _ptr(dy), _ptr(add0), _ptr(add1), _ptr(gamma), _ptr(beta),
                                               _ptr(scale_shift), ss_ld, _ptr(dx0), _ptr(dx1), _ptr(g), _ptr(fwd_stats), _ptr(ws), N, H * W,
                                               groups, float(eps), int(silu), _stream()), "dxmi_groupnorm_generic_bwd")
    if scale_shift is None:
        red = colsum_f32(g)          # [2, N, C] -> [2, C]: both parameter gradients from ONE launch (fixed order over the images)
        return dx0, dx1, red[1], red[0], None
    d_ss = torch.empty((N, 2 * C), dtype=torch.float32, device=x.device)
    dgb = torch.empty((2, C), dtype=torch.float32, device=x.device)
    check(lib.dxmi_gn_ss_grads(_ptr(g), _ptr(scale_shift), ss_ld, _ptr(gamma), _ptr(beta), _ptr(d_ss), _ptr(dgb[0]), _ptr(dgb[1]), N, C,
                               _stream()), "dxmi_gn_ss_grads")
    return dx0, dx1, dgb[0], dgb[1], d_ss


def upsample2x(x, out=None):
    _need_cuda(x, out)
    N, H, W, C = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    if out is None:
        out = torch.empty((N, 2 * H, 2 * W, C), dtype=torch.bfloat16, device=x.device)
    check(load().dxmi_upsample2x(_ptr(x), _ptr(out), N, H, W, C, _stream()), "dxmi_upsample2x")
    return out


def edm_precond(x, sigma, sigma_data=0.5):
    _need_cuda(x, sigma)
    N = x.shape[0]
    x_in = torch.empty_like(x)
    t = torch.empty(N, dtype=torch.float32, device=x.device)
    check(load().dxmi_edm_precond(_ptr(x), _ptr(sigma), _ptr(x_in), _ptr(t), N, x.numel() // N, float(sigma_data), _stream()),
          "dxmi_edm_precond")
    return x_in, t


def edm_step(x, model_out, z, sigma, sigma_down, sigma_up, sigma_data=0.5, outs=None):
    _need_cuda(x, model_out, z, sigma, sigma_down, sigma_up)
    N = x.shape[0]
    sample, mean = (torch.empty_like(x), torch.empty_like(x)) if outs is None else outs
    assert sample.is_contiguous() and mean.is_contiguous() and sample.shape == x.shape and mean.shape == x.shape
    check(load().dxmi_edm_step_fwd(_ptr(x), _ptr(model_out), _ptr(z), _ptr(sigma), _ptr(sigma_down), _ptr(sigma_up), _ptr(sample),
                                   _ptr(mean), N, x.numel() // N, float(sigma_data), _stream()), "dxmi_edm_step_fwd")
    return sample, mean


# dxmi_edm_dsm_* weight schedules (include/dxmi_hip.h), by the reference's names (karras_diffusion.py:18-31)
DSM_WEIGHT_SCHEDULES = {"snr": 0, "snr+1": 1, "karras": 2, "truncated-snr": 3, "uniform": 4}


_NO_LEVELS = object()


def _batch_operands(what, first, same=(), per_sample=(), *, indices=_NO_LEVELS, t_table=_NO_LEVELS, chw4=False):
    """The operand check of the elementwise training launches (csrc/ew_common.h).  `first` and `same`: fp32 contiguous 16-byte
    aligned device tensors of one shape [N, ...] (the kernels read N x CHW elements of each); `per_sample`: the same with N
    elements; a None among `same` / `per_sample` is an absent optional operand.  A launch that gathers levels names `indices`
    (int64 [N]) and `t_table` (fp32 [L >= 2]).  chw4: refuse here, not in the library, a CHW that is no multiple of 4.
    -> (N, CHW, L), L = 0 without a table."""
    levels = t_table is not _NO_LEVELS
    ts = (first,) + tuple(same) + tuple(per_sample)
    _need_cuda(*((indices, t_table) if levels else ()), *ts)
    for t in ts + ((t_table,) if levels else ()):
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0):
            raise _lib.DxmiError(f"{what}: fp32 contiguous 16-byte aligned device tensors")
    if first.dim() < 2 or first.numel() == 0:
        raise _lib.DxmiError(f"{what}: a non-empty batch [N, ...] is needed, got {tuple(first.shape)}")
    N = first.shape[0]
    for t in same:
        if t is not None and t.shape != first.shape:
            raise _lib.DxmiError(f"{what}: operand of shape {tuple(t.shape)} where {tuple(first.shape)} is needed")
    for t in per_sample:
        if t is not None and t.numel() != N:
            raise _lib.DxmiError(f"{what}: per-sample operand of {t.numel()} elements for a batch of {N}")
    if levels:
        if indices.dtype != torch.int64 or not indices.is_contiguous() or indices.numel() != N:
            raise _lib.DxmiError(f"{what}: indices must be {N} contiguous int64 values")
        if t_table.dim() != 1 or t_table.numel() < 2:
            raise _lib.DxmiError(f"{what}: t_table must hold num_scales >= 2 levels, got {tuple(t_table.shape)}")
    if any(t is not None and t.device != first.device for t in ts + ((indices, t_table) if levels else ())):
        raise _lib.DxmiError(f"{what}: operands on different devices")
    CHW = first.numel() // N
    if chw4 and CHW % 4:
        raise _lib.DxmiError(f"{what}: the elements per sample ({CHW}) must be a multiple of 4")
    return N, CHW, t_table.numel() if levels else 0


def _dsm_schedule(weight_schedule):
    if weight_schedule not in DSM_WEIGHT_SCHEDULES:
        raise NotImplementedError(f"weight schedule {weight_schedule!r}")
    return DSM_WEIGHT_SCHEDULES[weight_schedule]


def edm_dsm_prep(x_start, noise, sigma, sigma_data=0.5, out=None):
    """-> (x_in = c_in(sigma) (x_start + noise sigma), t = 250 ln(sigma + 1e-44)) of the DSM loss (dxmi_edm_dsm_prep)."""
    N, CHW, _ = _batch_operands("dxmi_edm_dsm_prep", x_start, same=(noise, out), per_sample=(sigma,))
    x_in = torch.empty_like(x_start) if out is None else out
    t = torch.empty(N, dtype=torch.float32, device=x_start.device)
    check(load().dxmi_edm_dsm_prep(_ptr(x_start), _ptr(noise), _ptr(sigma), _ptr(x_in), _ptr(t), N, CHW,
                                   float(sigma_data), _stream()), "dxmi_edm_dsm_prep")
    return x_in, t


def edm_dsm_loss_fwd(model_out, x_start, noise, sigma, weight_schedule, sigma_data=0.5, sigma_min=0.002, distillation=False):
    """-> per-sample (xs_mse, mse) of the DSM loss (dxmi_edm_dsm_loss_fwd)."""
    N, CHW, _ = _batch_operands("dxmi_edm_dsm_loss_fwd", x_start, same=(model_out, noise), per_sample=(sigma,))
    xs = torch.empty(N, dtype=torch.float32, device=x_start.device)
    mse = torch.empty_like(xs)
    check(load().dxmi_edm_dsm_loss_fwd(_ptr(model_out), _ptr(x_start), _ptr(noise), _ptr(sigma), _ptr(xs), _ptr(mse), N,
                                       CHW, float(sigma_data), float(sigma_min), int(bool(distillation)),
                                       _dsm_schedule(weight_schedule), _stream()), "dxmi_edm_dsm_loss_fwd")
    return xs, mse


def edm_dsm_loss_bwd(g_mse, g_xs, model_out, x_start, noise, sigma, weight_schedule, sigma_data=0.5, sigma_min=0.002,
                     distillation=False, out=None):
    """-> d(model_out) of the DSM terms for the device upstream gradients g_mse / g_xs [N] (either may be None)."""
    N, CHW, _ = _batch_operands("dxmi_edm_dsm_loss_bwd", x_start, same=(model_out, noise, out), per_sample=(sigma, g_mse, g_xs))
    d = torch.empty_like(model_out) if out is None else out
    check(load().dxmi_edm_dsm_loss_bwd(_ptr(g_mse), _ptr(g_xs), _ptr(model_out), _ptr(x_start), _ptr(noise), _ptr(sigma), _ptr(d), N,
                                       CHW, float(sigma_data), float(sigma_min), int(bool(distillation)),
                                       _dsm_schedule(weight_schedule), _stream()), "dxmi_edm_dsm_loss_bwd")
    return d


def _ddpm_per_sample(name, t, N):
    """t_idx (int64) and g_loss of the DDPM launches: a device tensor of N contiguous elements, its dtype the caller's to check."""
    _need_cuda(t)
    if not (t.is_contiguous() and t.numel() == N):
        raise _lib.DxmiError(f"{name}: per-sample operand of {t.numel()} elements (contiguous) for a batch of {N}")


def ddpm_prep(x_start, noise, t_idx, table, out=None):
    """-> (x_t = table[0][t] x_start + table[1][t] noise, float(t)): the DDPM forward process q(x_t | x_0) and the network's time
    input (dxmi_ddpm_prep).  table: fp32 [2, T] on the device; t_idx: int64 [N] on the device."""
    name = "dxmi_ddpm_prep"
    _need_cuda(table)
    N, chw, _ = _batch_operands(name, x_start, same=(noise, out), chw4=True)
    _ddpm_per_sample(name, t_idx, N)
    if t_idx.dtype != torch.int64:
        raise _lib.DxmiError(f"{name}: t_idx must be int64, got {t_idx.dtype}")
    if not (table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2 and table.shape[0] == 2 and table.shape[1] >= 1):
        raise _lib.DxmiError(f"{name}: table must be a contiguous fp32 [2, T], got {table.dtype} {tuple(table.shape)}")
    x_t = torch.empty_like(x_start) if out is None else out
    t = torch.empty(N, dtype=torch.float32, device=x_start.device)
    check(load().dxmi_ddpm_prep(_ptr(x_start), _ptr(noise), _ptr(t_idx), _ptr(table), int(table.shape[1]), _ptr(x_t), _ptr(t), N, chw,
                                _stream()), name)
    return x_t, t


def ddpm_loss_fwd(eps_pred, noise):
    """-> per-sample mean_flat((eps_pred - noise)^2) of the noise-prediction loss (dxmi_ddpm_loss_fwd)."""
    N, chw, _ = _batch_operands("dxmi_ddpm_loss_fwd", eps_pred, same=(noise,), chw4=True)
    loss = torch.empty(N, dtype=torch.float32, device=eps_pred.device)
    check(load().dxmi_ddpm_loss_fwd(_ptr(eps_pred), _ptr(noise), _ptr(loss), N, chw, _stream()), "dxmi_ddpm_loss_fwd")
    return loss


def ddpm_loss_bwd(g_loss, eps_pred, noise, out=None):
    """-> d(eps_pred) of the noise-prediction loss for the device upstream gradient g_loss [N] (dxmi_ddpm_loss_bwd)."""
    name = "dxmi_ddpm_loss_bwd"
    N, chw, _ = _batch_operands(name, eps_pred, same=(noise, out), chw4=True)
    _ddpm_per_sample(name, g_loss, N)
    if g_loss.dtype != torch.float32:
        raise _lib.DxmiError(f"{name}: g_loss must be fp32, got {g_loss.dtype}")
    d = torch.empty_like(eps_pred) if out is None else out
    check(load().dxmi_ddpm_loss_bwd(_ptr(g_loss), _ptr(eps_pred), _ptr(noise), _ptr(d), N, chw, _stream()), name)
    return d


# dxmi_cd_solver modes and dxmi_cd_loss_* norms (include/dxmi_hip.h), by the reference's names (karras_diffusion.py:206-220)
CD_EULER_X0, CD_HEUN_PRED, CD_HEUN_CORR = range(3)
CD_LOSS_NORMS = {"l1": 0, "l2": 1, "l2-32": 2}


def cd_prep(x_start, noise, indices, t_table, sigma_data=0.5, teacher_sigma_data=None):
    """-> (x_t = x_start + noise t, x_in = c_in(t) x_t, time = 250 ln(t + 1e-44), x_in_teacher | None) with t = t_table[indices]
    (dxmi_cd_prep).  x_in_teacher is written only where teacher_sigma_data is given and differs from sigma_data."""
    N, CHW, S = _batch_operands("dxmi_cd_prep", x_start, indices=indices, t_table=t_table, same=(noise,))
    x_t, x_in = torch.empty_like(x_start), torch.empty_like(x_start)
    t = torch.empty(N, dtype=torch.float32, device=x_start.device)
    own = teacher_sigma_data is not None and float(teacher_sigma_data) != float(sigma_data)
    x_te = torch.empty_like(x_start) if own else None
    check(load().dxmi_cd_prep(_ptr(x_start), _ptr(noise), _ptr(indices), _ptr(t_table), S, _ptr(x_t), _ptr(x_in), _ptr(t), _ptr(x_te),
                              N, CHW, float(sigma_data), float(teacher_sigma_data if own else sigma_data), _stream()), "dxmi_cd_prep")
    return x_t, x_in, t, x_te


def cd_solver(mode, x_t, indices, t_table, x_start=None, model_out=None, d=None, samples=None, sigma_data=0.5, sigma_min=0.002,
              distillation=False, next_sigma_data=0.5):
    """One stage of euler_solver / heun_solver (dxmi_cd_solver).  sigma_data / sigma_min / distillation: the diffusion whose
    denoise() forms the denoiser (the teacher's); next_sigma_data: the diffusion of the network that reads the returned input.
      CD_EULER_X0  (x_start)                 -> (x_t2, target input, target time)
      CD_HEUN_PRED (model_out)               -> (d, samples, teacher's second input, its time)
      CD_HEUN_CORR (model_out, d, samples)   -> (x_t2, target input, target time)"""
    need = {CD_EULER_X0: (x_start,), CD_HEUN_PRED: (model_out,), CD_HEUN_CORR: (model_out, d, samples)}.get(mode)
    if need is None:
        raise _lib.DxmiError(f"dxmi_cd_solver: unknown mode {mode!r}")
    if any(v is None for v in need):
        raise _lib.DxmiError("dxmi_cd_solver: EULER_X0 needs x_start, HEUN_PRED model_out, HEUN_CORR model_out, d and samples")
    N, CHW, S = _batch_operands("dxmi_cd_solver", x_t, indices=indices, t_table=t_table, same=need)
    x_next, t_next = torch.empty_like(x_t), torch.empty(N, dtype=torch.float32, device=x_t.device)
    x_t2 = None
    if mode == CD_HEUN_PRED:
        d, samples = torch.empty_like(x_t), torch.empty_like(x_t)
    else:
        x_t2 = torch.empty_like(x_t)
    check(load().dxmi_cd_solver(int(mode), _ptr(x_start), _ptr(x_t), _ptr(model_out), _ptr(d), _ptr(samples), _ptr(indices),
                                _ptr(t_table), S, _ptr(x_t2), _ptr(x_next), _ptr(t_next), N, CHW, float(sigma_data), float(sigma_min),
                                int(bool(distillation)), float(next_sigma_data), _stream()), "dxmi_cd_solver")
    return (d, samples, x_next, t_next) if mode == CD_HEUN_PRED else (x_t2, x_next, t_next)


def _cd_loss_args(what, f_online, loss_norm, weight_schedule):
    if loss_norm not in CD_LOSS_NORMS:
        raise _lib.DxmiError(f"{what}: loss norm {loss_norm!r} is not one of {sorted(CD_LOSS_NORMS)}")
    if f_online.dim() != 4:
        raise _lib.DxmiError(f"{what}: [N, C, H, W] tensors are needed, got {tuple(f_online.shape)}")
    return CD_LOSS_NORMS[loss_norm], _dsm_schedule(weight_schedule)


def cd_loss_fwd(f_online, f_target, x_t, x_t2, indices, t_table, loss_norm, weight_schedule, sigma_data=0.5, sigma_min=0.002,
                distillation=False):
    """-> per-sample consistency loss mean_flat(norm(distiller - target)) * get_weightings(snr(t)) (dxmi_cd_loss_fwd)."""
    norm, sched = _cd_loss_args("dxmi_cd_loss_fwd", f_online, loss_norm, weight_schedule)
    N, _, S = _batch_operands("dxmi_cd_loss_fwd", f_online, indices=indices, t_table=t_table, same=(f_target, x_t, x_t2))
    _, C, H, W = f_online.shape
    loss = torch.empty(N, dtype=torch.float32, device=f_online.device)
    check(load().dxmi_cd_loss_fwd(_ptr(f_online), _ptr(f_target), _ptr(x_t), _ptr(x_t2), _ptr(indices), _ptr(t_table), S, _ptr(loss),
                                  N, C, H, W, norm, float(sigma_data), float(sigma_min), int(bool(distillation)), sched, _stream()),
          "dxmi_cd_loss_fwd")
    return loss


def cd_loss_bwd(g_loss, f_online, f_target, x_t, x_t2, indices, t_table, loss_norm, weight_schedule, sigma_data=0.5,
                sigma_min=0.002, distillation=False):
    """-> d(f_online) of the consistency loss for the device upstream gradient g_loss [N] (dxmi_cd_loss_bwd)."""
    norm, sched = _cd_loss_args("dxmi_cd_loss_bwd", f_online, loss_norm, weight_schedule)
    if g_loss is None:
        raise _lib.DxmiError("dxmi_cd_loss_bwd: no upstream gradient")
    N, _, S = _batch_operands("dxmi_cd_loss_bwd", f_online, indices=indices, t_table=t_table, same=(f_target, x_t, x_t2), per_sample=(g_loss,))
    _, C, H, W = f_online.shape
    d = torch.empty_like(f_online)
    check(load().dxmi_cd_loss_bwd(_ptr(g_loss), _ptr(f_online), _ptr(f_target), _ptr(x_t), _ptr(x_t2), _ptr(indices), _ptr(t_table), S,
                                  _ptr(d), N, C, H, W, norm, float(sigma_data), float(sigma_min), int(bool(distillation)), sched,
                                  _stream()), "dxmi_cd_loss_bwd")
    return d


# the schedules of dxmi_cd_huber_fwd / _bwd: the DSM ones and DXMI_DSM_W_ICT (1 / (t - t2)), which only these two have the levels for
HUBER_WEIGHT_SCHEDULES = dict(DSM_WEIGHT_SCHEDULES, ict=5)


def _cd_huber_args(what, huber_c, weight_schedule):
    if weight_schedule not in HUBER_WEIGHT_SCHEDULES:
        raise NotImplementedError(f"weight schedule {weight_schedule!r}")
    c = float(huber_c)
    if not (math.isfinite(c) and c > 0):
        raise _lib.DxmiError(f"{what}: huber_c must be finite and positive, got {huber_c!r}")
    return c, HUBER_WEIGHT_SCHEDULES[weight_schedule]


def cd_huber_fwd(f_online, f_target, x_t, x_t2, indices, t_table, huber_c, weight_schedule, sigma_data=0.5, sigma_min=0.002,
                 distillation=False):
    """-> (loss, ssq): ssq = sum((distiller - target)^2) per sample and the pseudo-Huber consistency loss
    w ssq / (sqrt(ssq + huber_c^2) + huber_c), w the weight schedule ("ict": 1 / (t - t2)) (dxmi_cd_huber_fwd)."""
    c, sched = _cd_huber_args("dxmi_cd_huber_fwd", huber_c, weight_schedule)
    N, CHW, S = _batch_operands("dxmi_cd_huber_fwd", f_online, indices=indices, t_table=t_table, same=(f_target, x_t, x_t2), chw4=True)
    loss = torch.empty(N, dtype=torch.float32, device=f_online.device)
    ssq = torch.empty_like(loss)
    check(load().dxmi_cd_huber_fwd(_ptr(f_online), _ptr(f_target), _ptr(x_t), _ptr(x_t2), _ptr(indices), _ptr(t_table), S, _ptr(loss),
                                   _ptr(ssq), N, CHW, c, float(sigma_data), float(sigma_min), int(bool(distillation)), sched, _stream()),
          "dxmi_cd_huber_fwd")
    return loss, ssq


def cd_huber_bwd(g_loss, ssq, f_online, f_target, x_t, x_t2, indices, t_table, huber_c, weight_schedule, sigma_data=0.5,
                 sigma_min=0.002, distillation=False):
    """-> d(f_online) of the pseudo-Huber consistency loss for the device upstream gradient g_loss [N], with the forward's ssq
    (dxmi_cd_huber_bwd)."""
    c, sched = _cd_huber_args("dxmi_cd_huber_bwd", huber_c, weight_schedule)
    if g_loss is None or ssq is None:
        raise _lib.DxmiError("dxmi_cd_huber_bwd: no upstream gradient / no ssq of the forward")
    N, CHW, S = _batch_operands("dxmi_cd_huber_bwd", f_online, indices=indices, t_table=t_table, same=(f_target, x_t, x_t2), per_sample=(g_loss, ssq),
                                chw4=True)
    d = torch.empty_like(f_online)
    check(load().dxmi_cd_huber_bwd(_ptr(g_loss), _ptr(ssq), _ptr(f_online), _ptr(f_target), _ptr(x_t), _ptr(x_t2), _ptr(indices),
                                   _ptr(t_table), S, _ptr(d), N, CHW, c, float(sigma_data), float(sigma_min), int(bool(distillation)),
                                   sched, _stream()), "dxmi_cd_huber_bwd")
    return d


# dxmi_pd_solver modes (include/dxmi_hip.h); the progdist norms are the consistency ones without l2-32 (karras_diffusion.py:311-329)
PD_MID, PD_END = range(2)
PD_LOSS_NORMS = {"l1": 0, "l2": 1}


def _pd_operands(what, first, indices, t_table, same=(), per_sample=()):
    """_batch_operands for the progressive-distillation launches: t_table holds 2 S + 1 levels (S + 1 coarse, then S half steps).
    -> (N, CHW, S)."""
    if t_table is None or t_table.dim() != 1 or t_table.numel() < 3 or t_table.numel() % 2 == 0:
        raise _lib.DxmiError(f"{what}: t_table must hold 2 num_scales + 1 levels (num_scales >= 1), got "
                             f"{None if t_table is None else tuple(t_table.shape)}")
    N, CHW, L = _batch_operands(what, first, same, per_sample, indices=indices, t_table=t_table, chw4=True)
    return N, CHW, (L - 1) // 2


def pd_solver(mode, x_t, model_out, indices, t_table, x_t2=None, sigma_data=0.5, sigma_min=0.002, distillation=False,
              next_sigma_data=0.5):
    """One Euler stage of progdist_losses (dxmi_pd_solver).  sigma_data / sigma_min / distillation: the diffusion whose denoise()
    forms the denoiser (the teacher's); next_sigma_data: the diffusion of the network that reads the returned input.
      PD_MID (model_out at (x_t, t))          -> (x_t2, the teacher's second input, its time)
      PD_END (model_out at (x_t2, t2), x_t2)  -> target_x"""
    if mode not in (PD_MID, PD_END):
        raise _lib.DxmiError(f"dxmi_pd_solver: unknown mode {mode!r}")
    if model_out is None or (mode == PD_END and x_t2 is None):
        raise _lib.DxmiError("dxmi_pd_solver: MID needs model_out, END model_out and x_t2")
    N, CHW, S = _pd_operands("dxmi_pd_solver", x_t, indices, t_table, same=(model_out, x_t2))
    out = torch.empty_like(x_t)
    x_next = t_next = None
    if mode == PD_MID:
        x_next, t_next = torch.empty_like(x_t), torch.empty(N, dtype=torch.float32, device=x_t.device)
    check(load().dxmi_pd_solver(int(mode), _ptr(x_t), _ptr(x_t2), _ptr(model_out), _ptr(indices), _ptr(t_table), S, _ptr(out),
                                _ptr(x_next), _ptr(t_next), N, CHW, float(sigma_data), float(sigma_min), int(bool(distillation)),
                                float(next_sigma_data), _stream()), "dxmi_pd_solver")
    return (out, x_next, t_next) if mode == PD_MID else out


def _pd_loss_args(what, loss_norm, weight_schedule):
    if loss_norm not in PD_LOSS_NORMS:
        raise _lib.DxmiError(f"{what}: loss norm {loss_norm!r} is not one of {sorted(PD_LOSS_NORMS)}")
    return PD_LOSS_NORMS[loss_norm], _dsm_schedule(weight_schedule)


def pd_loss_fwd(f_online, x_t, target_x, indices, t_table, loss_norm, weight_schedule, sigma_data=0.5, sigma_min=0.002,
                distillation=False):
    """-> per-sample progdist loss mean_flat(norm(denoised - target_x)) * get_weightings(snr(t)) (dxmi_pd_loss_fwd)."""
    norm, sched = _pd_loss_args("dxmi_pd_loss_fwd", loss_norm, weight_schedule)
    N, CHW, S = _pd_operands("dxmi_pd_loss_fwd", f_online, indices, t_table, same=(x_t, target_x))
    loss = torch.empty(N, dtype=torch.float32, device=f_online.device)
    check(load().dxmi_pd_loss_fwd(_ptr(f_online), _ptr(x_t), _ptr(target_x), _ptr(indices), _ptr(t_table), S, _ptr(loss), N, CHW, norm,
                                  float(sigma_data), float(sigma_min), int(bool(distillation)), sched, _stream()), "dxmi_pd_loss_fwd")
    return loss


def pd_loss_bwd(g_loss, f_online, x_t, target_x, indices, t_table, loss_norm, weight_schedule, sigma_data=0.5, sigma_min=0.002,
                distillation=False):
    """-> d(f_online) of the progdist loss for the device upstream gradient g_loss [N] (dxmi_pd_loss_bwd)."""
    norm, sched = _pd_loss_args("dxmi_pd_loss_bwd", loss_norm, weight_schedule)
    if g_loss is None:
        raise _lib.DxmiError("dxmi_pd_loss_bwd: no upstream gradient")
    N, CHW, S = _pd_operands("dxmi_pd_loss_bwd", f_online, indices, t_table, same=(x_t, target_x), per_sample=(g_loss,))
    d = torch.empty_like(f_online)
    check(load().dxmi_pd_loss_bwd(_ptr(g_loss), _ptr(f_online), _ptr(x_t), _ptr(target_x), _ptr(indices), _ptr(t_table), S, _ptr(d), N,
                                  CHW, norm, float(sigma_data), float(sigma_min), int(bool(distillation)), sched, _stream()),
          "dxmi_pd_loss_bwd")
    return d


# dxmi_dm_grad_fwd weightings (include/dxmi_hip.h): DMD's normaliser mean|x - D_real|, or Diff-Instruct's plain score difference
DM_WEIGHTINGS = {"dmd": 0, "none": 1}
DM_REG_CHW = 12288      # dxmi_dm_grad_fwd keeps an image's D_fake - D_real in registers up to this many elements (csrc/dm_train.hip)


def _dm_scalar(what, name, v):
    v = float(v)
    if not (math.isfinite(v) and v > 0):
        raise _lib.DxmiError(f"{what}: {name} must be positive and finite, got {v!r}")
    return v


def _dm_operands(what, first, indices, t_table, same=(), per_sample=()):
    """_batch_operands for the launches of csrc/dm_train.hip and sid_train.hip that gather t = t_table[indices] (the table of
    cd_levels: >= 2 levels); none of their operands is optional."""
    if any(v is None for v in (first, indices, t_table) + tuple(same)):
        raise _lib.DxmiError(f"{what}: a needed operand is None")
    return _batch_operands(what, first, same, per_sample, indices=indices, t_table=t_table, chw4=True)


def dm_gen_in(z, gen_sigma, sigma_data=0.5):
    """-> (x_in = c_in(sigma_G) (sigma_G z), time [N] = 250 ln(sigma_G + 1e-44)): the one-step generator's input (dxmi_dm_gen_in)."""
    if z is None:
        raise _lib.DxmiError("dxmi_dm_gen_in: no latents")
    N, CHW, _ = _batch_operands("dxmi_dm_gen_in", z, chw4=True)
    sg, sd = _dm_scalar("dxmi_dm_gen_in", "gen_sigma", gen_sigma), _dm_scalar("dxmi_dm_gen_in", "sigma_data", sigma_data)
    x_in, t = torch.empty_like(z), torch.empty(N, dtype=torch.float32, device=z.device)
    check(load().dxmi_dm_gen_in(_ptr(z), _ptr(x_in), _ptr(t), N, CHW, sg, sd, _stream()), "dxmi_dm_gen_in")
    return x_in, t


def dm_gen_out(f_gen, z, gen_sigma, sigma_data=0.5, clip=True, out=None):
    """-> x = c_skip(sigma_G) (sigma_G z) + c_out(sigma_G) f_gen, clamped to [-1, 1] when `clip` (dxmi_dm_gen_out)."""
    if f_gen is None or z is None:
        raise _lib.DxmiError("dxmi_dm_gen_out: f_gen and z are needed")
    N, CHW, _ = _batch_operands("dxmi_dm_gen_out", f_gen, same=(z, out), chw4=True)
    sg, sd = _dm_scalar("dxmi_dm_gen_out", "gen_sigma", gen_sigma), _dm_scalar("dxmi_dm_gen_out", "sigma_data", sigma_data)
    x = torch.empty_like(f_gen) if out is None else out
    check(load().dxmi_dm_gen_out(_ptr(f_gen), _ptr(z), _ptr(x), N, CHW, sg, sd, int(bool(clip)), _stream()), "dxmi_dm_gen_out")
    return x


def dm_gen_prep(f_gen, z, noise, indices, t_table, gen_sigma, sigma_data=0.5, real_sigma_data=0.5, fake_sigma_data=None):
    """-> (x, x_t = x + noise t, x_in_real = c_in_real(t) x_t, time = 250 ln(t + 1e-44), x_in_fake | None) with x the generator's
    unclamped image and t = t_table[indices] (dxmi_dm_gen_prep).  x_in_fake is written only where fake_sigma_data is given and
    differs from real_sigma_data."""
    N, CHW, S = _dm_operands("dxmi_dm_gen_prep", f_gen, indices, t_table, same=(z, noise))
    what = "dxmi_dm_gen_prep"
    sg, sd, sdr = _dm_scalar(what, "gen_sigma", gen_sigma), _dm_scalar(what, "sigma_data", sigma_data), _dm_scalar(what, "sigma_data", real_sigma_data)
    own = fake_sigma_data is not None and float(fake_sigma_data) != float(real_sigma_data)
    sdf = _dm_scalar(what, "sigma_data", fake_sigma_data) if own else sdr
    x, x_t, x_in = torch.empty_like(f_gen), torch.empty_like(f_gen), torch.empty_like(f_gen)
    t = torch.empty(N, dtype=torch.float32, device=f_gen.device)
    x_fk = torch.empty_like(f_gen) if own else None
    check(load().dxmi_dm_gen_prep(_ptr(f_gen), _ptr(z), _ptr(noise), _ptr(indices), _ptr(t_table), S, _ptr(x), _ptr(x_t), _ptr(x_in),
                                  _ptr(t), _ptr(x_fk), N, CHW, sg, sd, sdr, sdf, _stream()), what)
    return x, x_t, x_in, t, x_fk


def _dm_diffusion(d, sigma_data=0.5, sigma_min=0.002, distillation=False):
    return (sigma_data, sigma_min, distillation) if d is None else (d["sigma_data"], d["sigma_min"], d["distillation"])


def dm_grad_fwd(f_real, f_fake, x, x_t, indices, t_table, weighting="dmd", real=None, fake=None):
    """-> (g [N, ...], loss [N], s [N]): D_r = c_out_r(t) f_real + c_skip_r(t) x_t, D_f likewise, s = mean|x - D_r|,
    g = (D_f - D_r) / s ("dmd") or D_f - D_r ("none"), loss = 0.5 mean(g^2); s == 0 gives g = 0 (dxmi_dm_grad_fwd).
    real / fake: dict(sigma_data, sigma_min, distillation) of the denoiser's diffusion (None: 0.5, 0.002, False; fake None: real's)."""
    what = "dxmi_dm_grad_fwd"
    if weighting not in DM_WEIGHTINGS:
        raise _lib.DxmiError(f"{what}: weighting {weighting!r} is not one of {sorted(DM_WEIGHTINGS)}")
    N, CHW, S = _dm_operands(what, f_real, indices, t_table, same=(f_fake, x, x_t))
    sdr, smr, dr = _dm_diffusion(real)
    sdf, smf, df = _dm_diffusion(fake if fake is not None else real)
    sdr, sdf = _dm_scalar(what, "sigma_data", sdr), _dm_scalar(what, "sigma_data", sdf)
    g = torch.empty_like(f_real)
    loss = torch.empty(N, dtype=torch.float32, device=f_real.device)
    s = torch.empty_like(loss)
    check(load().dxmi_dm_grad_fwd(_ptr(f_real), _ptr(f_fake), _ptr(x), _ptr(x_t), _ptr(indices), _ptr(t_table), S, _ptr(g), _ptr(loss),
                                  _ptr(s), N, CHW, DM_WEIGHTINGS[weighting], sdr, float(smr), int(bool(dr)), sdf, float(smf),
                                  int(bool(df)), _stream()), what)
    return g, loss, s


def dm_gen_bwd(upstream, g, gen_sigma, sigma_data=0.5):
    """-> d(f_gen) = ((upstream[n] / CHW) g[n]) c_out(sigma_G) for the device upstream gradient [N] (dxmi_dm_gen_bwd)."""
    if upstream is None or g is None:
        raise _lib.DxmiError("dxmi_dm_gen_bwd: no upstream gradient / no g of the forward")
    N, CHW, _ = _batch_operands("dxmi_dm_gen_bwd", g, per_sample=(upstream,), chw4=True)
    sg, sd = _dm_scalar("dxmi_dm_gen_bwd", "gen_sigma", gen_sigma), _dm_scalar("dxmi_dm_gen_bwd", "sigma_data", sigma_data)
    d = torch.empty_like(g)
    check(load().dxmi_dm_gen_bwd(_ptr(upstream), _ptr(g), _ptr(d), N, CHW, sg, sd, _stream()), "dxmi_dm_gen_bwd")
    return d


def _dmms_ladder(what, gen_sigmas, first, steps=None, need_steps=False):
    """The ladder and the per-image steps of the K-step generator's launches (csrc/dm_train.hip): gen_sigmas fp32 [K >= 1] contiguous
    on the device of `first`, steps None or int64 [N] contiguous there.  -> K"""
    if gen_sigmas is None or (need_steps and steps is None):
        raise _lib.DxmiError(f"{what}: a needed operand is None")
    _need_cuda(gen_sigmas, steps)
    if not (gen_sigmas.dtype == torch.float32 and gen_sigmas.is_contiguous() and gen_sigmas.dim() == 1 and gen_sigmas.numel() >= 1
            and gen_sigmas.device == first.device):
        raise _lib.DxmiError(f"{what}: gen_sigmas must be a contiguous fp32 [K >= 1] on the operands' device")
    if steps is not None and not (steps.dtype == torch.int64 and steps.is_contiguous() and steps.dim() == 1
                                  and steps.numel() == first.shape[0] and steps.device == first.device):
        raise _lib.DxmiError(f"{what}: steps must be {first.shape[0]} contiguous int64 values on the operands' device")
    return gen_sigmas.numel()


def dmms_in(z, gen_sigmas, sigma_data=0.5):
    """-> (x = sigma_0 z, x_in = c_in(sigma_0) x, time [N] = 250 ln(sigma_0 + 1e-44)): step 0 of the K-step generator
    (dxmi_dmms_in).  gen_sigmas: the fp32 device ladder [K]."""
    what = "dxmi_dmms_in"
    if z is None:
        raise _lib.DxmiError(f"{what}: no latents")
    N, CHW, _ = _batch_operands(what, z, chw4=True)
    K = _dmms_ladder(what, gen_sigmas, z)
    sd = _dm_scalar(what, "sigma_data", sigma_data)
    x, x_in, t = torch.empty_like(z), torch.empty_like(z), torch.empty(N, dtype=torch.float32, device=z.device)
    check(load().dxmi_dmms_in(_ptr(z), _ptr(gen_sigmas), K, _ptr(x), _ptr(x_in), _ptr(t), N, CHW, sd, _stream()), what)
    return x, x_in, t


def dmms_stage(f_gen, stage, gen_sigmas, x, x_in, t_out, steps=None, eps=None, sample_index=None, seed=0, draw=0, sigma_data=0.5):
    """ONE launch between generator evaluations `stage` and `stage` + 1, in place (dxmi_dmms_stage): for an image with steps None
    or steps[n] > stage, x = G_stage(x) + eps sigma_{stage+1}, x_in = c_in(sigma_{stage+1}) x, t_out[n] its time; an image with
    steps[n] <= stage is frozen (its rows are neither read nor written).  eps [N, ...] given, or sample_index (int64 [N]) with seed /
    draw: made in the launch, the values of randn_indexed(sample_index, x.shape[1:], seed, draw).  Not both."""
    what = "dxmi_dmms_stage"
    if f_gen is None or x is None or x_in is None or t_out is None:
        raise _lib.DxmiError(f"{what}: a needed operand is None")
    if (eps is None) == (sample_index is None):
        raise _lib.DxmiError(f"{what}: noise is either given (eps) or made here (sample_index): exactly one of them")
    N, CHW, _ = _batch_operands(what, f_gen, same=(x, x_in, eps), per_sample=(t_out,), chw4=True)
    K = _dmms_ladder(what, gen_sigmas, f_gen, steps)
    if not (0 <= int(stage) <= K - 2):
        raise _lib.DxmiError(f"{what}: stage {stage!r} outside [0, K - 2 = {K - 2}]")
    if sample_index is not None:
        _need_cuda(sample_index)
        if not (sample_index.dtype == torch.int64 and sample_index.is_contiguous() and sample_index.shape == (N,)
                and sample_index.device == f_gen.device):
            raise _lib.DxmiError(f"{what}: sample_index must be a contiguous int64 [{N}] on the operands' device")
    sd = _dm_scalar(what, "sigma_data", sigma_data)
    check(load().dxmi_dmms_stage(_ptr(f_gen), _ptr(eps), _ptr(sample_index), int(draw) & 0xFFFFFFFF, int(seed) & _U64, _ptr(steps),
                                 _ptr(gen_sigmas), K, int(stage), _ptr(x), _ptr(x_in), _ptr(t_out), N, CHW, sd, _stream()), what)


def dmms_prep(f_gen, x_k, noise, steps, gen_sigmas, indices, t_table, sigma_data=0.5, real_sigma_data=0.5, fake_sigma_data=None):
    """dm_gen_prep of the K-step generator (dxmi_dmms_prep): x = c_skip(sigma_k) x_k + c_out(sigma_k) f_gen with sigma_k =
    gen_sigmas[steps[n]] -> (x, x_t, x_in_real, time, x_in_fake | None)."""
    what = "dxmi_dmms_prep"
    N, CHW, S = _dm_operands(what, f_gen, indices, t_table, same=(x_k, noise))
    K = _dmms_ladder(what, gen_sigmas, f_gen, steps, need_steps=True)
    sd, sdr = _dm_scalar(what, "sigma_data", sigma_data), _dm_scalar(what, "sigma_data", real_sigma_data)
    own = fake_sigma_data is not None and float(fake_sigma_data) != float(real_sigma_data)
    sdf = _dm_scalar(what, "sigma_data", fake_sigma_data) if own else sdr
    x, x_t, x_in = torch.empty_like(f_gen), torch.empty_like(f_gen), torch.empty_like(f_gen)
    t = torch.empty(N, dtype=torch.float32, device=f_gen.device)
    x_fk = torch.empty_like(f_gen) if own else None
    check(load().dxmi_dmms_prep(_ptr(f_gen), _ptr(x_k), _ptr(noise), _ptr(steps), _ptr(gen_sigmas), K, _ptr(indices), _ptr(t_table), S,
                                _ptr(x), _ptr(x_t), _ptr(x_in), _ptr(t), _ptr(x_fk), N, CHW, sd, sdr, sdf, _stream()), what)
    return x, x_t, x_in, t, x_fk


def dmms_out(f_gen, x_k, gen_sigmas, sigma_data=0.5, clip=True, out=None):
    """-> x = c_skip(sigma_{K-1}) x_k + c_out(sigma_{K-1}) f_gen, clamped to [-1, 1] when `clip` (dxmi_dmms_out)."""
    what = "dxmi_dmms_out"
    if f_gen is None or x_k is None:
        raise _lib.DxmiError(f"{what}: f_gen and x_k are needed")
    N, CHW, _ = _batch_operands(what, f_gen, same=(x_k, out), chw4=True)
    K = _dmms_ladder(what, gen_sigmas, f_gen)
    sd = _dm_scalar(what, "sigma_data", sigma_data)
    x = torch.empty_like(f_gen) if out is None else out
    check(load().dxmi_dmms_out(_ptr(f_gen), _ptr(x_k), _ptr(gen_sigmas), K, _ptr(x), N, CHW, sd, int(bool(clip)), _stream()), what)
    return x


def dmms_bwd(upstream, g, steps, gen_sigmas, sigma_data=0.5):
    """-> d(f_gen) = ((upstream[n] / CHW) g[n]) c_out(gen_sigmas[steps[n]]) for the device upstream gradient [N] (dxmi_dmms_bwd)."""
    what = "dxmi_dmms_bwd"
    if upstream is None or g is None:
        raise _lib.DxmiError(f"{what}: no upstream gradient / no g of the forward")
    N, CHW, _ = _batch_operands(what, g, per_sample=(upstream,), chw4=True)
    K = _dmms_ladder(what, gen_sigmas, g, steps, need_steps=True)
    sd = _dm_scalar(what, "sigma_data", sigma_data)
    d = torch.empty_like(g)
    check(load().dxmi_dmms_bwd(_ptr(upstream), _ptr(g), _ptr(steps), _ptr(gen_sigmas), K, _ptr(d), N, CHW, sd, _stream()), what)
    return d


def sid_grad_fwd(f_real, f_fake, x, x_t, indices, t_table, alpha=1.2, real=None, fake=None, outs=None):
    """-> (v_real, v_fake, d_dir [N, ...], loss [N], s [N]) of score identity distillation (dxmi_sid_grad_fwd): with D_r, D_f as in
    dm_grad_fwd, delta = D_r - D_f, e = D_f - x, s = mean|x - D_r|: loss = ((1 - alpha) sum(delta^2) + sum(delta e)) / (CHW s);
    v_real = c_out_r (2 (1 - alpha) delta + e) and v_fake = c_out_f ((2 alpha - 1) delta - e), the cotangents on f_real and f_fake,
    and d_dir, the paths to x through no network; all three without the 1 / s (sid_join applies it).  real / fake as in dm_grad_fwd.
    outs: (v_real, v_fake, d_dir, loss, s) to write into."""
    what = "dxmi_sid_grad_fwd"
    alpha = float(alpha)
    if not math.isfinite(alpha):
        raise _lib.DxmiError(f"{what}: alpha must be finite, got {alpha!r}")
    N, CHW, S = _dm_operands(what, f_real, indices, t_table, same=(f_fake, x, x_t))
    sdr, smr, dr = _dm_diffusion(real)
    sdf, smf, df = _dm_diffusion(fake if fake is not None else real)
    sdr, sdf = _dm_scalar(what, "sigma_data", sdr), _dm_scalar(what, "sigma_data", sdf)
    if outs is None:
        v_r, v_f, d_dir = torch.empty_like(f_real), torch.empty_like(f_real), torch.empty_like(f_real)
        loss = torch.empty(N, dtype=torch.float32, device=f_real.device)
        s = torch.empty_like(loss)
    else:
        v_r, v_f, d_dir, loss, s = outs
        _batch_operands(what, f_real, same=(v_r, v_f, d_dir), per_sample=(loss, s), chw4=True)
        if any(v is None for v in outs):
            raise _lib.DxmiError(f"{what}: outs holds five tensors")
    check(load().dxmi_sid_grad_fwd(_ptr(f_real), _ptr(f_fake), _ptr(x), _ptr(x_t), _ptr(indices), _ptr(t_table), S, alpha, _ptr(v_r),
                                   _ptr(v_f), _ptr(d_dir), _ptr(loss), _ptr(s), N, CHW, sdr, float(smr), int(bool(dr)), sdf, float(smf),
                                   int(bool(df)), _stream()), what)
    return v_r, v_f, d_dir, loss, s


def sid_join(d_dir, g_real, g_fake, s, indices, t_table, real_sigma_data=0.5, fake_sigma_data=None, out=None):
    """-> g = ((d_dir + c_in_r g_real) + c_in_f g_fake) / s, 0 where s == 0 (dxmi_sid_join): the operand of dm_gen_bwd.  g_real /
    g_fake: the input gradients of the two denoisers at sid_grad_fwd's cotangents.  out: d_dir itself (in place) or a fresh tensor."""
    what = "dxmi_sid_join"
    if s is None:
        raise _lib.DxmiError(f"{what}: a needed operand is None")
    N, CHW, S = _dm_operands(what, d_dir, indices, t_table, same=(g_real, g_fake), per_sample=(s,))
    sdr = _dm_scalar(what, "sigma_data", real_sigma_data)
    sdf = sdr if fake_sigma_data is None else _dm_scalar(what, "sigma_data", fake_sigma_data)
    if out is None:
        out = torch.empty_like(d_dir)
    elif out is not d_dir:
        _batch_operands(what, d_dir, same=(out,), chw4=True)
        if any(out.data_ptr() == v.data_ptr() for v in (d_dir, g_real, g_fake)):
            raise _lib.DxmiError(f"{what}: out may be d_dir itself or a tensor of its own")
    check(load().dxmi_sid_join(_ptr(d_dir), _ptr(g_real), _ptr(g_fake), _ptr(s), _ptr(indices), _ptr(t_table), S, _ptr(out), N, CHW,
                               sdr, sdf, _stream()), what)
    return out


# ---- SiDA's parameter-free discriminator on the fake denoiser's bottleneck (csrc/sida_train.hip)
def _sida_host(what, values, N, ctype, name):
    """A per-image host operand (a scalar stands for every image; a sequence or a CPU tensor of N values) -> a ctypes array."""
    if torch.is_tensor(values):
        if values.is_cuda:
            raise _lib.DxmiError(f"{what}: {name} is a host operand (it is checked and passed as a kernel argument), got a device tensor")
        values = values.reshape(-1).tolist()
    elif not isinstance(values, (list, tuple)):
        values = [values] * N
    if len(values) != N:
        raise _lib.DxmiError(f"{what}: {name} holds {len(values)} values for {N} images")
    return (ctype * N)(*values)


def _sida_map(what, h):
    _need_cuda(h)
    if h is None or h.dtype != torch.bfloat16 or not h.is_contiguous() or h.dim() < 3:
        raise _lib.DxmiError(f"{what}: a contiguous NHWC bf16 activation [N, ..., Cb] is needed")
    N, Cb = h.shape[0], h.shape[-1]
    if N == 0 or h.numel() == 0:
        raise _lib.DxmiError(f"{what}: empty activation {tuple(h.shape)}")
    return N, h.numel() // (N * Cb), Cb


def sida_map_fwd(h, sign):
    """h NHWC bf16 [N, hb, wb, Cb] (or [N, P, Cb]), sign: -1 / +1 per image on the HOST (an int for all, or N of them) ->
    (logit fp32 [N, P] = mean_c h, a fp32 [N] = mean_p softplus(sign_n logit[n, p])) (dxmi_sida_map_fwd)."""
    what = "dxmi_sida_map_fwd"
    N, P, Cb = _sida_map(what, h)
    signs = _sida_host(what, sign, N, ctypes.c_int32, "sign")
    logit = torch.empty((N, P), dtype=torch.float32, device=h.device)
    a = torch.empty(N, dtype=torch.float32, device=h.device)
    check(load().dxmi_sida_map_fwd(_ptr(h), signs, _ptr(logit), _ptr(a), N, P, Cb, _stream()), what)
    return logit, a


def sida_map_bwd(logit, sign, coef, Cb, upstream=None, shape=None):
    """-> d_h bf16 [N, P, Cb] (of `shape`, e.g. [N, hb, wb, Cb], where given), d_h[n, p, :] = (coef_n upstream_n) sign_n sigmoid(sign_n logit[n, p])
    / (P Cb), rounded once (dxmi_sida_map_bwd).  sign and coef live on the HOST (a scalar for all images, or N values); upstream:
    fp32 [N] on the device, or None for 1."""
    what = "dxmi_sida_map_bwd"
    _need_cuda(logit, upstream)
    if logit is None or logit.dtype != torch.float32 or not logit.is_contiguous() or logit.dim() != 2 or logit.numel() == 0:
        raise _lib.DxmiError(f"{what}: logit is a contiguous fp32 [N, P] tensor")
    N, P = logit.shape
    Cb = int(Cb)
    if upstream is not None and not (upstream.dtype == torch.float32 and upstream.is_contiguous() and upstream.numel() == N):
        raise _lib.DxmiError(f"{what}: upstream is a contiguous fp32 tensor of {N} elements")
    signs = _sida_host(what, sign, N, ctypes.c_int32, "sign")
    coefs = _sida_host(what, coef, N, ctypes.c_float, "coef")
    shape = (N, P, Cb) if shape is None else tuple(shape)
    if math.prod(shape) != N * P * Cb or shape[0] != N or shape[-1] != Cb:
        raise _lib.DxmiError(f"{what}: shape {shape} is not [N = {N}, ..., Cb = {Cb}] with {P} positions")
    d_h = torch.empty(shape, dtype=torch.bfloat16, device=logit.device)
    check(load().dxmi_sida_map_bwd(_ptr(logit), signs, coefs, _ptr(upstream), _ptr(d_h), N, P, Cb, _stream()), what)
    return d_h


# ---- DMD2's GAN head (csrc/gan_head.hip; models/cm/gan_head.py)
def gan_head_supported(C, map_size):
    """Raise DxmiError (its message names the value) where the head's kernels do not serve C channels on a map_size^2 bottleneck."""
    check(load().dxmi_gan_head_supported(int(C), int(map_size)), "dxmi_gan_head_supported")


def gan_conv4s2_slices(dgrad=False):
    """The number of fp32 slabs dxmi_gan_conv4s2_fwd (dgrad: _dgrad) sums per output element."""
    return int(load().dxmi_gan_conv4s2_slices(int(bool(dgrad))))


def gan_conv4s2_pack(w, out=None):
    """w fp32 [C, C, 4, 4] -> (w_fwd, w_t), the two bf16 forms of the head's 4x4 stride-2 weight: [16 taps][Cout][Cin] and
    [16 taps][Cin][Cout] (dxmi_gan_conv4s2_pack); out: such a pair to rewrite in place."""
    _need_cuda(w)
    if w.dim() != 4 or w.shape[0] != w.shape[1] or tuple(w.shape[2:]) != (4, 4):
        raise _lib.DxmiError(f"dxmi_gan_conv4s2_pack: a [C, C, 4, 4] weight is needed, got {tuple(w.shape)}")
    w = w.detach().contiguous().float()
    C = w.shape[0]
    if out is None:
        out = (torch.empty((16, C, C), dtype=torch.bfloat16, device=w.device), torch.empty((16, C, C), dtype=torch.bfloat16, device=w.device))
    if any(tuple(t.shape) != (16, C, C) or t.dtype != torch.bfloat16 or not t.is_contiguous() for t in out):
        raise _lib.DxmiError(f"dxmi_gan_conv4s2_pack: out is a pair of contiguous bf16 [16, {C}, {C}] tensors")
    check(load().dxmi_gan_conv4s2_pack(_ptr(w), _ptr(out[0]), _ptr(out[1]), C, _stream()), "dxmi_gan_conv4s2_pack")
    return out


def _gan_map(what, t, C=None, H=None):
    _need_cuda(t)
    if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.dim() != 4 or t.shape[1] != t.shape[2]:
        raise _lib.DxmiError(f"{what}: a contiguous NHWC bf16 square map is needed, got {tuple(t.shape)} {t.dtype}")
    if (C is not None and t.shape[3] != C) or (H is not None and t.shape[1] != H):
        raise _lib.DxmiError(f"{what}: map of shape {tuple(t.shape)} where [N, {H}, {H}, {C}] is needed")
    return t.shape[0], t.shape[1], t.shape[3]


def gan_conv4s2_fwd(x, pw, bias=None):
    """x NHWC bf16 [N, H, H, C] -> bf16 [N, H/2, H/2, C] = conv(x, w, 4x4, stride 2, pad 1) + bias (dxmi_gan_conv4s2_fwd); pw: the
    pair of gan_conv4s2_pack."""
    what = "dxmi_gan_conv4s2_fwd"
    N, H, C = _gan_map(what, x, pw[0].shape[1])
    _need_cuda(bias)
    lib = load()
    nbytes = lib.dxmi_gan_conv4s2_workspace_bytes(N, H, C, 0)
    ws = _workspace(max(nbytes, 16), x.device)
    y = torch.empty((N, H // 2, H // 2, C), dtype=torch.bfloat16, device=x.device)
    check(lib.dxmi_gan_conv4s2_fwd(_ptr(x), _ptr(pw[0]), _ptr(bias), _ptr(y), _ptr(ws), nbytes, N, H, C, _stream()), what)
    return y


def gan_conv4s2_dgrad(dy, pw):
    """dy NHWC bf16 [N, H/2, H/2, C] -> dx bf16 [N, H, H, C], the data gradient of gan_conv4s2_fwd (dxmi_gan_conv4s2_dgrad)."""
    what = "dxmi_gan_conv4s2_dgrad"
    N, OH, C = _gan_map(what, dy, pw[1].shape[1])
    H = 2 * OH
    lib = load()
    nbytes = lib.dxmi_gan_conv4s2_workspace_bytes(N, H, C, 1)
    ws = _workspace(max(nbytes, 16), dy.device)
    dx = torch.empty((N, H, H, C), dtype=torch.bfloat16, device=dy.device)
    check(lib.dxmi_gan_conv4s2_dgrad(_ptr(dy), _ptr(pw[1]), _ptr(dx), _ptr(ws), nbytes, N, H, C, _stream()), what)
    return dx


def gan_conv4s2_wgrad(x, dy):
    """-> (dw fp32 [C, C, 4, 4], db fp32 [C]) of gan_conv4s2_fwd from its input x and output gradient dy (dxmi_gan_conv4s2_wgrad)."""
    what = "dxmi_gan_conv4s2_wgrad"
    N, H, C = _gan_map(what, x)
    _gan_map(what, dy, C, H // 2)
    if dy.shape[0] != N:
        raise _lib.DxmiError(f"{what}: x holds {N} images, dy {dy.shape[0]}")
    dw = torch.empty((C, C, 4, 4), dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    check(load().dxmi_gan_conv4s2_wgrad(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), N, H, C, _stream()), what)
    return dw, db


def _gan_logit_operands(what, a, w, per_sample):
    _need_cuda(a, w, *per_sample)
    if a.dtype != torch.bfloat16 or not a.is_contiguous() or a.dim() < 2:
        raise _lib.DxmiError(f"{what}: a contiguous bf16 [N, C] activation is needed")
    N, C = a.shape[0], a.numel() // a.shape[0]
    for t, n in ((w, C),) + tuple((t, N) for t in per_sample):
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
            raise _lib.DxmiError(f"{what}: fp32 contiguous operand of {n} elements needed")
    return N, C


def gan_logit_loss_fwd(a, w, b, sign):
    """a bf16 [N, C] (or [N, 1, 1, C]), w fp32 [C], b fp32 [1], sign fp32 [N] of -1 / +1 -> (logit [N] = w . a_n + b,
    loss [N] = softplus(sign_n logit_n)) in one launch (dxmi_gan_logit_loss_fwd)."""
    what = "dxmi_gan_logit_loss_fwd"
    N, C = _gan_logit_operands(what, a, w, (sign,))
    _need_cuda(b)
    if b.dtype != torch.float32 or b.numel() != 1:
        raise _lib.DxmiError(f"{what}: b is one fp32 value")
    logit = torch.empty(N, dtype=torch.float32, device=a.device)
    loss = torch.empty_like(logit)
    check(load().dxmi_gan_logit_loss_fwd(_ptr(a), _ptr(w), _ptr(b), _ptr(sign), _ptr(logit), _ptr(loss), N, C, _stream()), what)
    return logit, loss


def gan_logit_loss_bwd(a, w, sign, logit, upstream, weight=1.0, params=True):
    """-> (d_a bf16 like a, dw [C] | None, db [1] | None) for the per-sample upstream [N] and the weight of the term
    (dxmi_gan_logit_loss_bwd); params False: the input-only backward."""
    what = "dxmi_gan_logit_loss_bwd"
    N, C = _gan_logit_operands(what, a, w, (sign, logit, upstream))
    weight = float(weight)
    if not math.isfinite(weight):
        raise _lib.DxmiError(f"{what}: weight must be finite, got {weight!r}")
    d_a = torch.empty_like(a)
    dw = torch.empty(C, dtype=torch.float32, device=a.device) if params else None
    db = torch.empty(1, dtype=torch.float32, device=a.device) if params else None
    check(load().dxmi_gan_logit_loss_bwd(_ptr(a), _ptr(w), _ptr(sign), _ptr(logit), _ptr(upstream), weight, _ptr(d_a), _ptr(dw), _ptr(db),
                                         N, C, _stream()), what)
    return d_a, dw, db


def gan_join(g, d_xin, indices, t_table, weight, sigma_data=0.5, out=None):
    """-> g + (CHW weight c_in(t)) d_xin, t = t_table[indices] (dxmi_gan_join): the DM direction joined with the GAN term's gradient
    with respect to the fake denoiser's input.  out: g itself (in place) or a fresh tensor."""
    what = "dxmi_gan_join"
    N, CHW, S = _dm_operands(what, g, indices, t_table, same=(d_xin,))
    weight = float(weight)
    if not math.isfinite(weight):
        raise _lib.DxmiError(f"{what}: weight must be finite, got {weight!r}")
    sd = _dm_scalar(what, "sigma_data", sigma_data)
    if out is None:
        out = torch.empty_like(g)
    elif out is not g:
        _batch_operands(what, g, same=(out,), chw4=True)
        if out.data_ptr() == d_xin.data_ptr():
            raise _lib.DxmiError(f"{what}: out may be g itself or a tensor of its own")
    check(load().dxmi_gan_join(_ptr(g), _ptr(d_xin), _ptr(indices), _ptr(t_table), S, _ptr(out), N, CHW, weight, sd, _stream()), what)
    return out


EMA_MAX_RATES = 4


def ema_update(targets, sources, rates, found_inf=None):
    """targets: one list of fp32 device tensors per rate (up to EMA_MAX_RATES), each parallel to `sources`;
    targets[k][i] = rates[k] targets[k][i] + (1 - rates[k]) sources[i] in one launch series (dxmi_ema_update).
    found_inf: device fp32 [1] flag: when it is non-zero the launches leave every target untouched."""
    rates = [float(r) for r in rates]
    K, n = len(rates), len(sources)
    if not 1 <= K <= EMA_MAX_RATES or len(targets) != K or any(len(t) != n for t in targets):
        raise _lib.DxmiError(f"ema_update: 1..{EMA_MAX_RATES} rates, one target list of {n} tensors per rate")
    _need_f32_dense(sources, *targets)
    for ts in targets:
        for t, s in zip(ts, sources):
            if t.numel() != s.numel():
                raise _lib.DxmiError("ema_update: target and source sizes differ")
    if found_inf is not None:
        assert found_inf.is_cuda and found_inf.dtype == torch.float32
    ema = _ptr_array([t for ts in targets for t in ts])
    check(load().dxmi_ema_update(ema, _ptr_array(sources), _numel_array(sources), n, K, (ctypes.c_double * K)(*rates),
                                 _ptr(found_inf), _stream()), "dxmi_ema_update")


# dxmi_karras_stage modes and table columns (include/dxmi_hip.h)
KARRAS_FIRST, KARRAS_PRED, KARRAS_HEUN_CORR, KARRAS_DPM_CORR, KARRAS_EULER, KARRAS_ANCESTRAL = range(6)
KT_SIGMA, KT_CSKIP, KT_COUT, KT_DT, KT_SIGMA_UP, KT_CHURN, KT_SNOISE, KT_CIN, KT_T, KT_XSCALE, KT_CLIP = range(11)
KT_COLS = 16


def karras_stage(mode, last, tab, row, x, x2=None, d=None, model_out=None, noise=None, x_in=None, t=None, out=None, denoised=None):
    """One stage of the Karras samplers between two network evaluations (dxmi_karras_stage).  tab: fp32 [rows, KT_COLS] on the
    device; x / x2 / d: the sampler state, read and written in place; every tensor fp32 [N, C, H, W] contiguous (t: [N])."""
    _need_cuda(tab, x, x2, d, model_out, noise, x_in, t, out, denoised)
    for v in (tab, x, x2, d, model_out, noise, x_in, t, out, denoised):
        assert v is None or (v.dtype == torch.float32 and v.is_contiguous()), "karras_stage: fp32 contiguous tensors only"
    for v in (x2, d, model_out, noise, x_in, out, denoised):
        assert v is None or v.shape == x.shape, "karras_stage: every image tensor has the state's shape"
    assert tab.dim() == 2 and tab.shape[1] == KT_COLS and 0 <= row < tab.shape[0], "karras_stage: table row out of range"
    N = x.shape[0]
    assert t is None or t.shape == (N,)
    check(load().dxmi_karras_stage(int(mode), int(bool(last)), _ptr(tab), int(row), _ptr(x), _ptr(x2), _ptr(d), _ptr(model_out),
                                   _ptr(noise), _ptr(x_in), _ptr(t), _ptr(out), _ptr(denoised), N, x.numel() // N, _stream()),
          "dxmi_karras_stage")


# dxmi_cm_stage modes, edit kinds and table columns (include/dxmi_hip.h)
CM_FIRST, CM_STEP = range(2)
CM_EDIT_NONE, CM_EDIT_MASK, CM_EDIT_COLOUR, CM_EDIT_PATCH = range(4)
CT_CSKIP, CT_COUT, CT_NOISE, CT_CIN, CT_T, CT_XSCALE, CT_CLIP, CT_OUTCLAMP = range(8)
CT_COLS = 8


def cm_stage(mode, last, tab, row, x, edit=CM_EDIT_NONE, Q=None, model_out=None, noise=None, ref=None, mask=None, x_in=None,
             t=None, out=None, denoised=None):
    """One stage of the consistency-model samplers and editing loops between two network evaluations (dxmi_cm_stage).
    tab: fp32 [rows, CT_COLS] on the device; x: the state [N, C, H, W], read and written in place; Q: fp32 3x3 (colour) or
    64x64 (patch); every tensor fp32 contiguous (t: [N])."""
    _need_cuda(tab, x, Q, model_out, noise, ref, mask, x_in, t, out, denoised)
    for v in (tab, x, Q, model_out, noise, ref, mask, x_in, t, out, denoised):
        assert v is None or (v.dtype == torch.float32 and v.is_contiguous()), "cm_stage: fp32 contiguous tensors only"
    assert x.dim() == 4, "cm_stage: x is [N, C, H, W]"
    for v in (model_out, noise, ref, mask, x_in, out, denoised):
        assert v is None or v.shape == x.shape, "cm_stage: every image tensor has the state's shape"
    assert tab.dim() == 2 and tab.shape[1] == CT_COLS and 0 <= row < tab.shape[0], "cm_stage: table row out of range"
    dim = {CM_EDIT_COLOUR: 3, CM_EDIT_PATCH: 64}.get(edit)
    assert Q is None or dim is None or Q.shape == (dim, dim), f"cm_stage: Q must be {dim}x{dim}"
    N, C, H, W = x.shape
    assert t is None or t.shape == (N,)
    check(load().dxmi_cm_stage(int(mode), int(edit), int(bool(last)), _ptr(tab), int(row), _ptr(Q), _ptr(x), _ptr(model_out),
                               _ptr(noise), _ptr(ref), _ptr(mask), _ptr(x_in), _ptr(t), _ptr(out), _ptr(denoised), N, C, H, W,
                               _stream()), "dxmi_cm_stage")

def attention(qkv, heads, scale, out=None, want_lse=False):
    """qkv: [N, T, 3C] bf16 laid out [q|k|v]; returns [N, T, C] bf16.  want_lse: -> (out, lse | None): the row log-sum-exp the
    kernel leaves for attention_bwd(lse=...) (fp32 [N, heads, T], log2 domain; None for the shapes that have no such kernel)."""
    _need_cuda(qkv, out)
    N, T, C3 = qkv.shape
    C = C3 // 3
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous()
    if out is None:
        out = torch.empty((N, T, C), dtype=torch.bfloat16, device=qkv.device)
    lib = load()
    if want_lse and lib.dxmi_attention_fwd_lse_supported(T, C, heads):
        lse = torch.empty((N, heads, T), dtype=torch.float32, device=qkv.device)
        _prof("attention", f"T{T}_D{C // heads}", 4.0 * N * T * T * C, 2.0 * N * T * 4 * C, lambda: check(
            lib.dxmi_attention_fwd_lse(_ptr(qkv), _ptr(out), _ptr(lse), N, T, C, heads, float(scale), _stream()), "dxmi_attention_fwd_lse"))
        return out, lse
    _prof("attention", f"T{T}_D{C // heads}", 4.0 * N * T * T * C, 2.0 * N * T * 4 * C, lambda: check(
        lib.dxmi_attention_fwd(_ptr(qkv), _ptr(out), N, T, C, heads, float(scale), _stream()), "dxmi_attention_fwd"))
    return (out, None) if want_lse else out


def attention_proj_supported(T, C, heads):
    return bool(load().dxmi_attention_proj_supported(T, C, heads))


def pack_attn_proj_weight(w, out=None):
    """proj_out weight [256, 256(, 1, 1)] fp32 -> the 128 KiB bf16 fragment image dxmi_attention_proj_fwd reads (out: rewrite that
    image in place)."""
    _need_cuda(w)
    w2 = w.detach().float().reshape(w.shape[0], -1).contiguous()
    assert tuple(w2.shape) == (256, 256)
    dst = pack_tensor(256 * 256, torch.bfloat16, w.device) if out is None else out
    check(load().dxmi_pack_attn_proj_weight(_ptr(w2), _ptr(dst), _stream()), "dxmi_pack_attn_proj_weight")
    return dst


def attention_proj(qkv, wproj_packed, bias, residual, heads, scale, out=None, want_stats=False):
    """x + proj_out(attention(qkv)) + bias in one launch (see include/dxmi_hip.h).  qkv [N,T,3C], residual [N,T,C] bf16.
    want_stats: -> (out, BlockStats of out) from the same launch."""
    _need_cuda(qkv, wproj_packed, bias, residual, out)
    N, T, C3 = qkv.shape
    C = C3 // 3
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and residual.dtype == torch.bfloat16 and residual.is_contiguous()
    assert residual.numel() == N * T * C and bias.dtype == torch.float32 and bias.numel() == C
    if out is None:
        out = torch.empty((N, T, C), dtype=torch.bfloat16, device=qkv.device)
    stats = BlockStats(torch.empty((N, 8, C // 2, 2), dtype=torch.float32, device=qkv.device), 8) if want_stats else None
    _prof("attention", f"T{T}_D{C // heads}_proj", 4.0 * N * T * T * C + 2.0 * N * T * C * C, 2.0 * N * T * 5 * C, lambda: check(
        load().dxmi_attention_proj_fwd(_ptr(qkv), _ptr(wproj_packed), _ptr(bias), _ptr(residual), _ptr(out),
                                       stats.buf.data_ptr() if want_stats else None, N, T, C, heads, float(scale), _stream()),
        "dxmi_attention_proj_fwd"))
    return (out, stats) if want_stats else out


def attn_block_supported(T, C, heads, groups=32):
    return bool(load().dxmi_attn_block_supported(T, C, heads, groups))


def attn_block_pack(wq, bq, wk, wv, bv, wproj, bproj, scale, out=None):
    """Folded + packed weights of a whole AttnBlock (include/dxmi_hip.h: dxmi_attn_block_pack): G = scale Wk^T Wq, W' = Wproj Wv,
    g = scale Wk^T bq, b' = bproj + Wproj bv.  The k bias has no effect on the block (constant along the key axis of the softmax)."""
    ws = [t.detach().float().reshape(t.shape[0], -1).contiguous() for t in (wq, wk, wv, wproj)]
    bs = [t.detach().float().contiguous() for t in (bq, bv, bproj)]
    _need_cuda(*ws, *bs)
    assert all(tuple(w.shape) == (256, 256) for w in ws) and all(b.numel() == 256 for b in bs)
    dst = pack_tensor(int(load().dxmi_attn_block_packed_bytes()), torch.uint8, ws[0].device) if out is None else out
    check(load().dxmi_attn_block_pack(_ptr(ws[0]), _ptr(bs[0]), _ptr(ws[1]), _ptr(ws[2]), _ptr(bs[1]), _ptr(ws[3]), _ptr(bs[2]),
                                      float(scale), _ptr(dst), _stream()), "dxmi_attn_block_pack")
    return dst


def attn_block(x, stats, gamma, beta, packed, eps=1e-6, out=None, want_stats=False):
    """x + proj_out(attention(q, k, v of GroupNorm(x))) in ONE launch (reference unet_small.py:167-191; dxmi_attn_block_fwd).
    x [N,16,16,256] or [N,256,256] bf16, stats = its BlockStats; want_stats: -> (out, BlockStats of out)."""
    _need_cuda(x, stats.buf, gamma, beta, packed, out)
    shape = x.shape
    N, C = shape[0], shape[-1]
    T = x.numel() // (N * C)
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and tuple(stats.buf.shape) == (N, stats.P, C // 2, 2)
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C and beta.numel() == C
    if stats.P > MAX_APPLY_PARTIALS:
        stats = fold_stats(stats)
    if out is None:
        out = torch.empty_like(x)
    st = BlockStats(torch.empty((N, 8, C // 2, 2), dtype=torch.float32, device=x.device), 8) if want_stats else None
    _prof("attention", f"block_T{T}_C{C}", 8.0 * N * T * C * C, 4.0 * N * T * C, lambda: check(
        load().dxmi_attn_block_fwd(_ptr(x), _ptr(stats.buf), stats.P, _ptr(gamma), _ptr(beta), float(eps), _ptr(packed), _ptr(out),
                                   st.buf.data_ptr() if want_stats else None, N, T, C, _stream()), "dxmi_attn_block_fwd"))
    return (out, st) if want_stats else out


def timestep_embedding(t, dim, order=0, max_period=10000.0, out=None):
    _need_cuda(t, out)
    t = t.float().contiguous()
    if out is None:
        out = torch.empty((t.numel(), dim), dtype=torch.float32, device=t.device)
    check(load().dxmi_timestep_embedding(_ptr(t), _ptr(out), t.numel(), dim, order, float(max_period), _stream()),
          "dxmi_timestep_embedding")
    return out


def linear(x, pw, bias=None, pre_act=ACT_NONE, post_act=ACT_NONE, out=None, splitk=False):
    """x fp32 [P, K] -> fp32 [P, M]; pw = pack_conv_weight(W[M, K]).
    splitk: allow the split-K form for skinny products with a long K.  Its slice count depends on the number of rows, so the
    fp32 summation order of a row would change with the batch it rides in: only the training backward (linear_bwd) asks for
    it; forward calls keep one reduction order per shape (bitwise batch independence of the generation path)."""
    _need_cuda(x, bias, out)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == pw.Cin
    P, K = x.shape
    S = load().dxmi_linear_splitk_slices(P, K, pw.Cout) if (splitk and post_act == ACT_NONE) else 1
    if S > 1:      # skinny product with a long K: slices of K in parallel, summed in slice order (deterministic)
        part = torch.empty((S, P, pw.Cout), dtype=torch.float32, device=x.device)
        check(load().dxmi_linear_splitk(_ptr(x), _ptr(pw.buf), _ptr(part), P, K, pw.Cout, pre_act, _stream()), "dxmi_linear_splitk")
        res = part.sum(0) if bias is None else part.sum(0).add_(bias)
        return res if out is None else out.copy_(res)
    if out is None:
        out = torch.empty((P, pw.Cout), dtype=torch.float32, device=x.device)
    check(load().dxmi_linear_fwd(_ptr(x), _ptr(pw.buf), _ptr(bias), _ptr(out), P, K, pw.Cout, pre_act, post_act,
                                 _stream()), "dxmi_linear_fwd")
    return out


def _rows_as_map(t_f32, rows_pad):
    """fp32 [P, K] -> bf16 [1, rows_pad / 16, 16, K] (zero rows appended): the pixel-GEMM operand form of a dense layer's rows."""
    P, K = t_f32.shape
    out = torch.zeros((rows_pad, K), dtype=torch.bfloat16, device=t_f32.device)
    out[:P] = t_f32
    return out.view(1, rows_pad // 16, 16, K)


def linear_bwd(x, dy, pw_t, need_dx=True):
    """Backward of y = x @ W^T + b for the small dense layers of the embedding graphs (temb MLP, temb_proj / emb_layers,
    reference unet_small.py:296-299,123 and models/cm/unet.py:775-779,249) on the HIP kernels — no BLAS library call:
      dx = dy @ W            dxmi_linear_fwd on the transposed pack (pw_t = pack_conv_weight(W, transpose_flip=True))
      dW = dy^T @ x          dxmi_conv2d_wgrad with ksize 1: the rows are the 'pixels' of a 1x1 conv (zero rows pad the count)
      db = column sums of dy
    x [P, K], dy [P, M] fp32 (K, M multiples of 64) -> (dx [P, K] | None, dW [M, K], db [M]) fp32; bf16 MFMA operands as the
    forward's."""
    _need_cuda(x, dy)
    P, K = x.shape
    M = dy.shape[1]
    assert dy.shape[0] == P and x.dtype == torch.float32 and dy.dtype == torch.float32
    dy = dy.contiguous()
    dx = linear(dy, pw_t, splitk=True) if need_dx else None
    rows = 64
    while rows < P:
        rows *= 2
    dw = conv2d_wgrad(_rows_as_map(x, rows), _rows_as_map(dy, rows), 1)          # [M, K, 1, 1]
    return dx, dw.view(M, K), dy.sum(0)


def silu_bwd(pre, g):
    """g * d/dpre [pre * sigmoid(pre)] (elementwise, fp32)."""
    sg = torch.sigmoid(pre)
    return g * (sg * (1 + pre * (1 - sg)))


def var_gather_sched(t, continuous_steps, xmul_tab, cmul_tab, log_betas_all, sigma_out=None):
    _need_cuda(t, continuous_steps, xmul_tab, cmul_tab, log_betas_all, sigma_out)
    assert t.dtype == torch.int64
    N, T = t.numel(), continuous_steps.numel()
    outs = [torch.empty(N, dtype=torch.float32, device=t.device) for _ in range(3)]
    outs.append(sigma_out if sigma_out is not None else torch.empty(N, dtype=torch.float32, device=t.device))
    assert outs[3].is_contiguous() and outs[3].numel() == N and outs[3].dtype == torch.float32
    check(load().dxmi_var_gather_sched(_ptr(t), _ptr(continuous_steps), _ptr(xmul_tab), _ptr(cmul_tab),
                                       _ptr(log_betas_all), *[_ptr(o) for o in outs], N, T, _stream()),
          "dxmi_var_gather_sched")
    return outs  # tau, xmul, cmul, sigma


def var_step(x, eps, z, xmul, cmul, sigma, want_mean=True, want_control=True, outs=None, assoc=0):
    """Fused sampler transition; all tensors fp32, x/eps/z [N,C,H,W], per-sample scalars [N]."""
    _need_cuda(x, eps, z, xmul, cmul, sigma)
    N = x.shape[0]
    CHW = x.numel() // N
    for t_ in (x, eps, z):
        assert t_.dtype == torch.float32 and t_.is_contiguous()
    if outs is None:
        x_next = torch.empty_like(x)
        mean = torch.empty_like(x) if want_mean else None
        control = torch.empty_like(x) if want_control else None
        logp = torch.empty(N, dtype=torch.float32, device=x.device)
    else:
        x_next, mean, control, logp = outs
    nb = 4.0 * N * CHW * (3 + 1 + (mean is not None) + (control is not None))
    _prof("sampler_step", "var_step", 0.0, nb, lambda: check(
        load().dxmi_var_step_fwd(_ptr(x), _ptr(eps), _ptr(z), _ptr(xmul), _ptr(cmul), _ptr(sigma), _ptr(x_next),
                                 _ptr(mean), _ptr(control), _ptr(logp), N, CHW, assoc, _stream()), "dxmi_var_step_fwd"))
    return x_next, mean, control, logp


def var_step_bwd(g_next, g_mean, g_control, g_logp, z, cmul, sigma):
    """Backward of the VAR transition (dxmi_var_step_bwd): -> (d eps [N, ...], d sigma [N]); any gradient may be None."""
    _need_cuda(g_next, g_mean, g_control, g_logp, z, cmul, sigma)
    N = z.shape[0]
    CHW = z.numel() // N
    for t_ in (g_next, g_mean, g_control, z):
        assert t_ is None or (t_.dtype == torch.float32 and t_.is_contiguous() and t_.numel() == N * CHW)
    assert g_logp is None or (g_logp.dtype == torch.float32 and g_logp.is_contiguous() and g_logp.numel() == N)
    d_eps = torch.empty_like(z)
    d_sigma = torch.empty(N, dtype=torch.float32, device=z.device)
    check(load().dxmi_var_step_bwd(_ptr(g_next), _ptr(g_mean), _ptr(g_control), _ptr(g_logp), _ptr(z), _ptr(cmul), _ptr(sigma), _ptr(d_eps),
                                   _ptr(d_sigma), N, CHW, _stream()), "dxmi_var_step_bwd")
    return d_eps, d_sigma


def edm_step_bwd(g_sample, g_mean, z, sigma, sigma_down, sigma_data=0.5):
    """Backward of the EDM transition (dxmi_edm_step_bwd): -> (d model_output, d sigma_up [N])."""
    _need_cuda(g_sample, g_mean, z, sigma, sigma_down)
    N = z.shape[0]
    CHW = z.numel() // N
    for t_ in (g_sample, g_mean, z):
        assert t_ is None or (t_.dtype == torch.float32 and t_.is_contiguous() and t_.numel() == N * CHW)
    d_out = torch.empty_like(z)
    d_up = torch.empty(N, dtype=torch.float32, device=z.device)
    check(load().dxmi_edm_step_bwd(_ptr(g_sample), _ptr(g_mean), _ptr(z), _ptr(sigma), _ptr(sigma_down), _ptr(d_out), _ptr(d_up), N, CHW,
                                   float(sigma_data), _stream()), "dxmi_edm_step_bwd")
    return d_out, d_up


def pool_act(x, pool, act, out=None):
    _need_cuda(x, out)
    N, H, W, C = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    if out is None:
        out = torch.empty((N, H // 2, W // 2, C) if pool else (N, H, W, C), dtype=torch.bfloat16, device=x.device)
    check(load().dxmi_pool_act(_ptr(x), _ptr(out), N, H, W, C, int(pool), act, _stream()), "dxmi_pool_act")
    return out


def value_head(x, w, b, out_w=None, out_b=None, out=None):
    """out_w / out_b: device scalars of the Linear(1,1) out_scale, or None."""
    _need_cuda(x, w, b, out_w, out_b, out)
    N, H, W, C = x.shape
    if out is None:
        out = torch.empty((N, 1), dtype=torch.float32, device=x.device)
    check(load().dxmi_value_head(_ptr(x), _ptr(w), _ptr(b), _ptr(out_w), _ptr(out_b), _ptr(out), N, H * W, C,
                                 _stream()), "dxmi_value_head")
    return out


def stem_conv_wgrad(x_nchw, dy):
    """Weight gradient of a 3-channel 3x3/s1/p1 image conv: x [N,3,H,W] fp32, dy [N,H,W,Cout] bf16 ->
    fp32 [Cout,3,3,3] (im2col to K=27(+37 zero) then the 1x1 MFMA pixel-GEMM)."""
    _need_cuda(x_nchw, dy)
    N, C, H, W = x_nchw.shape
    assert C == 3 and x_nchw.dtype == torch.float32 and x_nchw.is_contiguous()
    with wgrad_branch((x_nchw, dy)):                    # (im2col, the pixel-GEMM and the slice: one branch of a captured step)
        cols = torch.empty((N, H, W, 64), dtype=torch.bfloat16, device=x_nchw.device)
        check(load().dxmi_im2col27(_ptr(x_nchw), _ptr(cols), N, H, W, _stream()), "dxmi_im2col27")
        dw = _conv2d_wgrad(cols, dy, 1)                 # [Cout, 64, 1, 1]
        return dw[:, :27, 0, 0].reshape(dy.shape[3], 3, 3, 3).contiguous()


def quantize_u8(x, mode=0, nhwc=True, out=None):
    """Output stage: NCHW fp32 [N,C,H,W] -> uint8 [N,H,W,C] (nhwc) or [N,C,H,W]; mode 0 = rescale + save_image rounding
    (generate_cifar10.py:205-209), mode 1 = (x + 1) * 127.5 truncated (generate_large.py:43).  Bit-exact pixel values."""
    _need_cuda(x, out)
    N, C, H, W = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    if out is None:
        out = torch.empty((N, H, W, C) if nhwc else (N, C, H, W), dtype=torch.uint8, device=x.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == x.numel()
    _prof("output_stage", f"quantize{mode}", 0.0, 5.0 * x.numel(), lambda: check(
        load().dxmi_quantize_u8(_ptr(x), _ptr(out), N, C, H * W, mode, int(nhwc), _stream()), "dxmi_quantize_u8"))
    return out


def fid_stats(act):
    """Activation statistics of the FID: act fp32 [N, D] (device) -> (mu fp64 [D], sigma fp64 [D, D]) = np.mean(act, axis=0),
    np.cov(act, rowvar=False) of train_image_large.py:62-69, on the f32-input MFMA (csrc/fid_stats.hip)."""
    _need_cuda(act)
    assert act.dim() == 2 and act.dtype == torch.float32 and act.is_contiguous()
    N, D = act.shape
    lib = load()
    mu = torch.empty(D, dtype=torch.float64, device=act.device)
    sigma = torch.empty((D, D), dtype=torch.float64, device=act.device)
    ws = _workspace(max(256, lib.dxmi_fid_stats_workspace_bytes(N, D)), act.device)
    _prof("fid_stats", f"d{D}", float(N) * D * (D + 128), 4.0 * act.numel() * ((D + 127) // 128 + 1) / 2, lambda: check(
        lib.dxmi_fid_stats(_ptr(act), N, D, _ptr(mu), _ptr(sigma), _ptr(ws), _stream()), "dxmi_fid_stats"))
    return mu, sigma


# ------------------------------------------------------------------------------------------ Frechet distance in fp64 (csrc/frechet.hip)
def _square_f64(x, what):
    _need_cuda(x)
    if not (x.dim() == 2 and x.shape[0] == x.shape[1] and x.dtype == torch.float64 and x.is_contiguous()):
        raise ValueError(f"{what}: need a contiguous float64 [n, n] device tensor, got {tuple(x.shape)} {x.dtype}")
    return x.shape[0]


def gemm_f64(a, b, alpha=1.0, diag=0.0, out=None, trace=None):
    """C = alpha * A @ B + diag * I for fp64 [n, n] device tensors (n % 16 == 0, 16 <= n <= 4096) on the f64 MFMA.  `trace`: a
    one-element fp64 device tensor that receives trace(C).  `out` must not share memory with `a` or `b`."""
    n = _square_f64(a, "gemm_f64(a)")
    if _square_f64(b, "gemm_f64(b)") != n:
        raise ValueError(f"gemm_f64: a is {n} x {n}, b is {b.shape[0]} x {b.shape[0]}")
    if out is None:
        out = torch.empty_like(a)
    elif _square_f64(out, "gemm_f64(out)") != n:
        raise ValueError("gemm_f64: out has another size")
    if trace is not None:
        _need_cuda(trace)
        assert trace.dtype == torch.float64 and trace.numel() == 1
    _prof("frechet", f"gemm_f64_n{n}", 2.0 * n * n * n, 24.0 * n * n, lambda: check(
        load().dxmi_gemm_f64(_ptr(a), _ptr(b), _ptr(out), n, float(alpha), float(diag), _ptr(trace), _stream()), "dxmi_gemm_f64"))
    return out


def frob_norm_f64(x, out=None):
    """||x||_F of an fp64 [n, n] device tensor -> one-element fp64 device tensor (fixed summation order)."""
    n = _square_f64(x, "frob_norm_f64")
    lib = load()
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=x.device)
    ws = _workspace(max(256, lib.dxmi_frechet_workspace_bytes(n)), x.device)
    _prof("frechet", f"frob_n{n}", 2.0 * n * n, 8.0 * n * n, lambda: check(
        lib.dxmi_frob_norm_f64(_ptr(x), n, _ptr(out), _ptr(ws), _stream()), "dxmi_frob_norm_f64"))
    return out


def scale_f64(x, alpha, out=None):
    """alpha * x for an fp64 [n, n] device tensor (`out` may be `x`)."""
    n = _square_f64(x, "scale_f64")
    if out is None:
        out = torch.empty_like(x)
    elif _square_f64(out, "scale_f64(out)") != n:
        raise ValueError("scale_f64: out has another size")
    _prof("frechet", f"scale_n{n}", 1.0 * n * n, 16.0 * n * n, lambda: check(
        load().dxmi_scale_f64(_ptr(x), _ptr(out), n, float(alpha), _stream()), "dxmi_scale_f64"))
    return out


def symmetrize_f64(x):
    """x <- (x + x^T) / 2 in place (fp64 [n, n] device tensor)."""
    n = _square_f64(x, "symmetrize_f64")
    _prof("frechet", f"symmetrize_n{n}", 1.0 * n * n, 16.0 * n * n, lambda: check(
        load().dxmi_symmetrize_f64(_ptr(x), n, _stream()), "dxmi_symmetrize_f64"))
    return x


def _newton_schulz_sqrt(m, tol, max_iters, eye, want_matrix):
    """Coupled Newton-Schulz iteration on a symmetric PSD fp64 device matrix: Y -> (m / c)^(1/2), Z -> its inverse, c = ||m||_F.
    -> (m^(1/2) or None, trace of it, iterations, converged).  Per iteration three GEMMs and one 8-byte readback (the trace)."""
    c = float(frob_norm_f64(m).item())
    y = scale_f64(m, 1.0 / c if c != 0.0 else float("inf"))
    z = eye.clone()
    t, y2, z2 = torch.empty_like(m), torch.empty_like(m), torch.empty_like(m)
    tr_dev = torch.empty(1, dtype=torch.float64, device=m.device)
    rc = c ** 0.5 if c >= 0.0 else float("nan")
    prev, tr, k, ok = None, float("nan"), 0, False
    while k < max_iters:
        gemm_f64(z, y, -0.5, 1.5, out=t)
        gemm_f64(y, t, out=y2, trace=tr_dev)
        gemm_f64(t, z, out=z2)
        y, y2, z, z2 = y2, y, z2, z
        k += 1
        tr = float(tr_dev.item()) * rc
        if tr != tr or tr in (float("inf"), float("-inf")):
            break
        if prev is not None and abs(tr - prev) <= tol * abs(tr):
            ok = True
            break
        prev = tr
    return (scale_f64(y, rc, out=y) if want_matrix and ok else None), tr, k, ok


def frechet_trace_sqrt(sigma1, sigma2, tol=1e-8, max_iters=100):
    """tr sqrt(sigma1 sigma2) of two symmetric PSD fp64 [n, n] device matrices -> (trace, (k1, k2), converged), by the two-stage
    Newton-Schulz iteration on symmetric matrices: R = sigma1^(1/2), then the trace of (R sigma2 R)^(1/2).  A stage
    ends not converged when its trace is not finite or after max_iters iterations; k2 = 0 when stage 1 did not converge.
    Everything stays on the device but the norm of each stage and one trace per iteration."""
    n = _square_f64(sigma1, "frechet_trace_sqrt(sigma1)")
    if _square_f64(sigma2, "frechet_trace_sqrt(sigma2)") != n:
        raise ValueError("frechet_trace_sqrt: sigma1 and sigma2 differ in size")
    eye = torch.eye(n, dtype=torch.float64, device=sigma1.device)
    r, _, k1, ok = _newton_schulz_sqrt(sigma1, tol, max_iters, eye, True)
    if not ok:
        return float("nan"), (k1, 0), False
    symmetrize_f64(r)
    m = gemm_f64(gemm_f64(r, sigma2), r)
    symmetrize_f64(m)
    _, tr, k2, ok = _newton_schulz_sqrt(m, tol, max_iters, eye, False)
    return tr, (k1, k2), ok


# ------------------------------------------------------------------------------------------ evaluator metrics
KNN_KMAX = 7


def _rows_f32(x, what):
    _need_cuda(x)
    if not (x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError(f"{what}: need a contiguous float32 [N, D] device tensor, got {tuple(x.shape)} {x.dtype}")
    return x.shape


def knn_radii(x, k=3, splits=0, workspace=None):
    """k-NN radii of ManifoldEstimator.manifold_radii (evaluations/evaluator.py:243-280): x fp32 [N, D] (device) -> fp32 [N],
    radii[i] = np.partition(d(x_i, x_*), k)[k] over the squared distances of x_i to every row (itself included), on the f32
    MFMA (csrc/eval_metrics.hip).  `splits` (0: automatic) and `workspace` (a uint8 device tensor) do not change the result."""
    N, D = _rows_f32(x, "knn_radii")
    lib = load()
    radii = torch.empty(N, dtype=torch.float32, device=x.device)
    need = lib.dxmi_knn_radii_workspace_bytes(N, D, k, splits)
    if workspace is None:
        workspace = _workspace(max(256, need), x.device)
    elif workspace.numel() < need:
        raise ValueError(f"knn_radii: workspace of {workspace.numel()} bytes, need {need}")
    _prof("eval_metrics", f"radii_d{D}", 2.0 * N * N * D, 4.0 * N * D * ((N + 127) // 128), lambda: check(
        lib.dxmi_knn_radii(_ptr(x), N, D, k, splits, _ptr(radii), _ptr(workspace), _stream()), "dxmi_knn_radii"))
    return radii


def pr_membership(a, ra, b, rb):
    """Manifold membership of ManifoldEstimator.evaluate_pr (evaluator.py:328-417): reference rows a fp32 [NA, D] with radii ra,
    sample rows b fp32 [NB, D] with radii rb -> (a_in_b int32 [NA], b_in_a int32 [NB]) 0 / 1 flags:
    a_in_b[i] = any_j d(a_i, b_j) <= rb[j] (its mean is the recall), b_in_a[j] = any_i d(a_i, b_j) <= ra[i] (the precision)."""
    NA, D = _rows_f32(a, "pr_membership")
    NB, DB = _rows_f32(b, "pr_membership")
    if DB != D:
        raise ValueError(f"pr_membership: feature sizes differ ({D} vs {DB})")
    _need_cuda(ra, rb)
    if ra.shape != (NA,) or rb.shape != (NB,) or ra.dtype != torch.float32 or rb.dtype != torch.float32:
        raise ValueError("pr_membership: radii must be float32 [NA] and [NB]")
    ra, rb = ra.contiguous(), rb.contiguous()
    lib = load()
    a_in_b = torch.empty(NA, dtype=torch.int32, device=a.device)
    b_in_a = torch.empty(NB, dtype=torch.int32, device=a.device)
    ws = _workspace(max(256, lib.dxmi_pr_membership_workspace_bytes(NA, NB)), a.device)
    _prof("eval_metrics", f"member_d{D}", 2.0 * NA * NB * D, 4.0 * D * (NA * ((NB + 127) // 128) + NB * ((NA + 127) // 128)), lambda: check(
        lib.dxmi_pr_membership(_ptr(a), NA, _ptr(ra), _ptr(b), NB, _ptr(rb), D, _ptr(a_in_b), _ptr(b_in_a), _ptr(ws), _stream()),
        "dxmi_pr_membership"))
    return a_in_b, b_in_a


def kid_sums(x, y, idx_x=None, idx_y=None, gamma=None, coef0=1.0, workspace=None):
    """Gram sums of the Kernel Inception Distance (Binkowski et al. 2018; include/dxmi_hip.h: dxmi_kid_sums): x fp32 [NX, D], y fp32
    [NY, D], idx_x int32 [S, mx] and idx_y int32 [S, my] the rows of S subsets (both None: one subset of every row) -> fp64 [S, 3]
    (device): Sxx = sum_{i != j} k(x_i, x_j), Syy likewise, Sxy = sum_{i, j} k(x_i, y_j), k(u, v) = ((double)(u . v) gamma + coef0)^3
    with the f32 dot of the evaluator kernels; gamma None: 1 / D.  One launch over all subsets, bitwise reproducible; `workspace`
    (a uint8 device tensor) does not change the result.  Indices are checked against [0, NX) / [0, NY) before the launch."""
    NX, D = _rows_f32(x, "kid_sums")
    NY, DY = _rows_f32(y, "kid_sums")
    if DY != D:
        raise ValueError(f"kid_sums: feature sizes differ ({D} vs {DY})")
    if (idx_x is None) != (idx_y is None):
        raise ValueError("kid_sums: idx_x and idx_y must both be given or both be None")
    S, mx, my = 1, NX, NY
    if idx_x is not None:
        _need_cuda(idx_x, idx_y)
        for idx, n, name in ((idx_x, NX, "idx_x"), (idx_y, NY, "idx_y")):
            if not (idx.dim() == 2 and idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() > 0):
                raise ValueError(f"kid_sums: {name} must be a contiguous non-empty int32 [S, m] device tensor, got {tuple(idx.shape)} {idx.dtype}")
            lo, hi = int(idx.min()), int(idx.max())
            if lo < 0 or hi >= n:
                raise ValueError(f"kid_sums: {name} holds a row index outside [0, {n}) (min {lo}, max {hi})")
        if idx_x.shape[0] != idx_y.shape[0]:
            raise ValueError(f"kid_sums: idx_x names {idx_x.shape[0]} subsets, idx_y {idx_y.shape[0]}")
        S, mx, my = idx_x.shape[0], idx_x.shape[1], idx_y.shape[1]
    gamma = 1.0 / D if gamma is None else float(gamma)
    lib = load()
    sums = torch.empty((S, 3), dtype=torch.float64, device=x.device)
    need = lib.dxmi_kid_sums_workspace_bytes(S, mx, my, D)
    if workspace is None:
        workspace = _workspace(max(256, need), x.device)
    elif workspace.numel() < need:
        raise ValueError(f"kid_sums: workspace of {workspace.numel()} bytes, need {need}")
    pairs = mx * (mx + 1) // 2 + my * (my + 1) // 2 + mx * my
    _prof("eval_metrics", f"kid_d{D}", 2.0 * S * pairs * D, 4.0 * S * D * (mx + my) * ((mx + my + 127) // 128), lambda: check(
        lib.dxmi_kid_sums(_ptr(x), NX, _ptr(y), NY, D, _ptr(idx_x), _ptr(idx_y), S, mx, my, gamma, float(coef0), _ptr(sums), _ptr(workspace),
                          _stream()), "dxmi_kid_sums"))
    return sums


def dc_counts(a, ra, b, splits=0, workspace=None):
    """Ball counts of density / coverage (Naeem et al. 2020; include/dxmi_hip.h: dxmi_dc_counts): reference rows a fp32 [NA, D] with
    their k-NN radii ra fp32 [NA], sample rows b fp32 [NB, D] -> int32 [NA], counts[i] = #{j : d(a_i, b_j) < ra[i]} (strict, where
    pr_membership compares with <=).  `splits` (0: automatic) and `workspace` (a uint8 device tensor) do not change the result."""
    NA, D = _rows_f32(a, "dc_counts")
    NB, DB = _rows_f32(b, "dc_counts")
    if DB != D:
        raise ValueError(f"dc_counts: feature sizes differ ({D} vs {DB})")
    _need_cuda(ra)
    if ra.shape != (NA,) or ra.dtype != torch.float32:
        raise ValueError("dc_counts: radii must be float32 [NA]")
    ra = ra.contiguous()
    lib = load()
    counts = torch.empty(NA, dtype=torch.int32, device=a.device)
    need = lib.dxmi_dc_counts_workspace_bytes(NA, NB, splits)
    if workspace is None:
        workspace = _workspace(max(256, need), a.device)
    elif workspace.numel() < need:
        raise ValueError(f"dc_counts: workspace of {workspace.numel()} bytes, need {need}")
    _prof("eval_metrics", f"dc_d{D}", 2.0 * NA * NB * D, 4.0 * D * (NA * ((NB + 127) // 128) + NB * ((NA + 127) // 128)), lambda: check(
        lib.dxmi_dc_counts(_ptr(a), NA, _ptr(ra), _ptr(b), NB, D, splits, _ptr(counts), _ptr(workspace), _stream()), "dxmi_dc_counts"))
    return counts


def inception_score_kl(pool, w, split_size=5000):
    """Per-split mean KL of Evaluator.compute_inception_score (evaluator.py:179-193): pool fp32 [N, D], w fp32 [C, D] (fc.weight
    layout, no bias) -> fp64 [ceil(N / split_size)] (device): mean_r sum_c p (log p - log p_bar), p = softmax(pool . w^T) in f32,
    p_bar the split's marginal, the reductions in fp64.  The score is exp(kl).mean()."""
    N, D = _rows_f32(pool, "inception_score")
    C, DW = _rows_f32(w, "inception_score")
    if DW != D:
        raise ValueError(f"inception_score: pool has {D} features, the weight {DW}")
    lib = load()
    kl = torch.empty((N + split_size - 1) // split_size, dtype=torch.float64, device=pool.device)
    ws = _workspace(max(256, lib.dxmi_inception_score_workspace_bytes(N, C, split_size)), pool.device)
    _prof("eval_metrics", f"is_c{C}", 2.0 * N * D * C, 4.0 * (N * D + 4 * N * C), lambda: check(
        lib.dxmi_inception_score(_ptr(pool), N, D, _ptr(w), C, split_size, _ptr(kl), _ptr(ws), _stream()), "dxmi_inception_score"))
    return kl


def inception_score(pool, w, split_size=5000):
    """Inception Score: mean over splits of exp(mean KL) (float, host)."""
    return float(torch.exp(inception_score_kl(pool, w, split_size).cpu()).mean())


def nchw_f32_to_nhwc_bf16(x, out=None):
    _need_cuda(x, out)
    N, C, H, W = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    if out is None:
        out = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=x.device)
    check(load().dxmi_nchw_f32_to_nhwc_bf16(_ptr(x), _ptr(out), N, C, H * W, _stream()), "dxmi_nchw_f32_to_nhwc_bf16")
    return out


def nhwc_bf16_to_nchw_f32(x, out=None):
    _need_cuda(x, out)
    N, H, W, C = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    if out is None:
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    check(load().dxmi_nhwc_bf16_to_nchw_f32(_ptr(x), _ptr(out), N, C, H * W, _stream()), "dxmi_nhwc_bf16_to_nchw_f32")
    return out


# ------------------------------------------------------------------------------------------ train-step tail
def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _numel_array(tensors):
    return (ctypes.c_int64 * len(tensors))(*[t.numel() for t in tensors])


def _need_f32_dense(*lists):
    for ts in lists:
        for t in ts:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise _lib.DxmiError("multi-tensor kernels take contiguous fp32 device tensors")


def adam_step(params, grads, exp_avgs, exp_avg_sqs, step_sizes, beta1, beta2, eps, bc2_sqrt, grad_scale=None,
              write_back_grad=False, cache=None, hyper=None):
    """One torch.optim.Adam update of every tensor in the lists (see dxmi_adam_step).  step_sizes: python floats
    -(lr_i / (1 - beta1^t)).  cache: dict reused across calls for the pointer arrays of params / moments (stable).
    hyper: DEVICE fp32 [1 + n] = (bc2_sqrt, step sizes) instead of the two host arguments (dxmi_adam_step_dev: a step that is
    replayed from a hipGraph)."""
    _need_f32_dense(params, grads, exp_avgs, exp_avg_sqs)
    n = len(params)
    if cache is None or cache.get("n") != n:
        c = {"n": n, "p": _ptr_array(params), "m": _ptr_array(exp_avgs), "v": _ptr_array(exp_avg_sqs), "numel": _numel_array(params)}
        if cache is not None:
            cache.update(c)
        cache = c
    if "elems" not in cache:
        cache["elems"] = sum(p.numel() for p in params)
    garr = _ptr_array(grads)
    if hyper is not None:
        assert hyper.is_cuda and hyper.dtype == torch.float32 and hyper.numel() == n + 1
        check(load().dxmi_adam_step_dev(cache["p"], garr, cache["m"], cache["v"], cache["numel"], n, beta1, beta2, eps, _ptr(hyper),
                                        _ptr(grad_scale), int(write_back_grad), _stream()), "dxmi_adam_step_dev")
        return
    ss = (ctypes.c_float * n)(*step_sizes)
    _prof("optimizer", "adam", 0.0, 28.0 * cache["elems"], lambda: check(
        load().dxmi_adam_step(cache["p"], garr, cache["m"], cache["v"], cache["numel"], ss, n, beta1, beta2, eps,
                              bc2_sqrt, _ptr(grad_scale), int(write_back_grad), _stream()), "dxmi_adam_step"))


def radam_step(params, grads, exp_avgs, exp_avg_sqs, lrs, beta1, beta2, eps, bc1, bc2_sqrt, rect, grad_scale=None,
               found_inf=None, cache=None, hyper=None):
    """One torch.optim.RAdam update (see dxmi_radam_step); rect < 0 selects the un-rectified branch.
    hyper: DEVICE fp32 [3 + n] = (fp32(1 / bc1), bc2_sqrt, rect, lrs) instead of the host arguments (dxmi_radam_step_dev)."""
    _need_f32_dense(params, grads, exp_avgs, exp_avg_sqs)
    n = len(params)
    if cache is None or cache.get("n") != n:
        c = {"n": n, "p": _ptr_array(params), "m": _ptr_array(exp_avgs), "v": _ptr_array(exp_avg_sqs), "numel": _numel_array(params)}
        if cache is not None:
            cache.update(c)
        cache = c
    if hyper is not None:
        assert hyper.is_cuda and hyper.dtype == torch.float32 and hyper.numel() == n + 3
        check(load().dxmi_radam_step_dev(cache["p"], _ptr_array(grads), cache["m"], cache["v"], cache["numel"], n, beta1, beta2, eps,
                                         _ptr(hyper), _ptr(grad_scale), _ptr(found_inf), _stream()), "dxmi_radam_step_dev")
        return
    lr = (ctypes.c_float * n)(*lrs)
    check(load().dxmi_radam_step(cache["p"], _ptr_array(grads), cache["m"], cache["v"], cache["numel"], lr, n, beta1, beta2, eps,
                                 bc1, bc2_sqrt, rect, _ptr(grad_scale), _ptr(found_inf), _stream()), "dxmi_radam_step")


def gradnorm_clip(grads, max_norm, scale_in_place=True, out=None):
    """Global L2 norm of `grads` and the clip coefficient, on the device: returns fp32 [3] = (norm, coef, non-finite flag).
    max_norm <= 0: norm only."""
    _need_f32_dense(grads)
    lib = load()
    numel = _numel_array(grads)
    nb = lib.dxmi_mt_blocks(numel, len(grads))
    dev = grads[0].device
    ws = _workspace(int(nb) * 4 + 64, dev)
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=dev)
    check(lib.dxmi_gradnorm_clip(_ptr_array(grads), numel, len(grads), float(max_norm), _ptr(ws), _ptr(out),
                                 int(scale_in_place and max_norm > 0), _stream()), "dxmi_gradnorm_clip")
    return out


def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_ without the host round trip: returns the total norm as a DEVICE scalar."""
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return None
    return gradnorm_clip(grads, max_norm)[0]


def dropout_site_seed(base, n):
    """32-bit seed of dropout site number `n` under the 64-bit `base` seed: a counter hash, so the nets' dropout draws nothing from
    torch's generators (whose streams the trainers' parity tests depend on)."""
    x = (int(base) * 0x9E3779B97F4A7C15 + int(n) * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 32
    x = (x * 0xD6E8FEB86659FD93) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 32
    return x & 0xFFFFFFFF


def dropout(x, p, seed, out=None):
    """Counter-hash dropout of a bf16 tensor (see dxmi_dropout_bf16); call again with the same seed on the gradient.
    seed: python int, or a DEVICE int32 tensor holding the 32-bit seed (dxmi_dropout_bf16_dev: hipGraph-replayed steps)."""
    _need_cuda(x, out)
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    if torch.is_tensor(seed):
        assert seed.is_cuda and seed.dtype == torch.int32 and seed.numel() == 1
        check(load().dxmi_dropout_bf16_dev(_ptr(x), _ptr(out), x.numel(), float(p), _ptr(seed), _stream()), "dxmi_dropout_bf16_dev")
        return out
    check(load().dxmi_dropout_bf16(_ptr(x), _ptr(out), x.numel(), float(p), int(seed) & 0xFFFFFFFF, _stream()), "dxmi_dropout_bf16")
    return out


def gather_rows(src, idx, out=None):
    """out[r] = src[idx[r]] along dim 0 (INT path of the replay buffer); idx int64 on the device."""
    _need_cuda(src, idx, out)
    assert src.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous() and idx.dim() == 1
    n = idx.numel()
    row_bytes = (src.numel() // max(src.shape[0], 1)) * src.element_size()
    if out is None:
        out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    assert out.is_contiguous() and out.dtype == src.dtype and out.numel() * out.element_size() == n * row_bytes
    if n:
        _prof("replay_gather", f"row{row_bytes}", 0.0, 2.0 * n * row_bytes, lambda: check(
            load().dxmi_gather_rows(_ptr(src), _ptr(idx), _ptr(out), n, src.shape[0], row_bytes, _stream()), "dxmi_gather_rows"))
    return out


IMG_NORM_ADM, IMG_NORM_TOTENSOR = 0, 1


def image_batch(store, idx, flip, norm, out=None):
    """One training batch from a uint8 image array (see dxmi_image_batch): store uint8 [M, H, W, C] (C = 3 or 1), idx int64 [B] (None:
    rows 0 .. B-1, with B from flip or out), flip uint8 [B] (None: no flips) -> fp32 [B, C, H, W], normalised by IMG_NORM_ADM
    (v / 127.5 - 1) or IMG_NORM_TOTENSOR (2 (v / 255) - 1).  An index outside [0, M) gives a NaN image."""
    _need_cuda(store, idx, flip, out)
    assert store.dtype == torch.uint8 and store.dim() == 4 and store.is_contiguous(), "image_batch: store is a contiguous uint8 [M, H, W, C]"
    M, H, W, C = store.shape
    assert M >= 1 and C in (1, 3), f"image_batch: store {tuple(store.shape)} needs rows and 3 or 1 channels"
    assert norm in (IMG_NORM_ADM, IMG_NORM_TOTENSOR), f"image_batch: norm {norm!r}"
    if idx is not None:
        assert idx.dtype == torch.int64 and idx.dim() == 1 and idx.is_contiguous(), "image_batch: idx is a contiguous int64 [B]"
    if flip is not None:
        assert flip.dtype == torch.uint8 and flip.dim() == 1 and flip.is_contiguous(), "image_batch: flip is a contiguous uint8 [B]"
    sized = [t.shape[0] for t in (idx, flip, out) if t is not None]
    assert sized, "image_batch: the batch size comes from idx, flip or out"
    B = sized[0]
    assert B >= 1 and all(n == B for n in sized), f"image_batch: idx / flip / out disagree on the batch size {sized}"
    assert idx is not None or B <= M, f"image_batch: without idx the batch ({B}) is rows 0 .. B-1 of {M}"
    if out is None:
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=store.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, C, H, W), \
        f"image_batch: out must be a contiguous fp32 {(B, C, H, W)}"
    _prof("data", f"image_batch{H}x{W}x{C}", 0.0, 5.0 * out.numel(), lambda: check(
        load().dxmi_image_batch(_ptr(store), M, _ptr(idx), _ptr(flip), _ptr(out), B, H, W, C, int(norm), _stream()), "dxmi_image_batch"))
    return out


def _indexed_operands(what, sample_index, shape_tail, dtype, out):
    """The checks of the indexed draws: sample_index a contiguous int64 [N >= 1] device tensor, shape_tail non-negative sizes with
    at least one element per row, out (if given) a contiguous `dtype` [N, *shape_tail] on the same device.  -> (N, per_sample, out)."""
    _need_cuda(sample_index, out)
    if sample_index.dtype != torch.int64 or sample_index.dim() != 1 or not sample_index.is_contiguous() or sample_index.numel() < 1:
        raise _lib.DxmiError(f"{what}: sample_index must be a non-empty contiguous int64 [N] device tensor")
    N, tail = sample_index.numel(), tuple(int(s) for s in shape_tail)
    per = 1
    for s in tail:
        per *= s
    if per < 1 or any(s < 0 for s in tail):
        raise _lib.DxmiError(f"{what}: every row needs at least one element, got the shape tail {tail}")
    if out is None:
        out = torch.empty((N,) + tail, dtype=dtype, device=sample_index.device)
    elif not (out.dtype == dtype and out.is_contiguous() and tuple(out.shape) == (N,) + tail and out.device == sample_index.device):
        raise _lib.DxmiError(f"{what}: out must be a contiguous {dtype} {(N,) + tail} on the device of sample_index")
    return N, per, out


_U64 = (1 << 64) - 1


def randn_indexed(sample_index, shape_tail, seed, draw, out=None):
    """Standard normals fp32 [N, *shape_tail] whose row n is a function of (seed, sample_index[n], draw) alone: the same row whatever
    batch it is drawn in (dxmi_randn_indexed; Philox-4x32-10 + Box-Muller, include/dxmi_hip.h).  sample_index: int64 [N] on the
    device; seed: any integer, taken modulo 2^64; draw: the draw number, modulo 2^32."""
    N, per, out = _indexed_operands("dxmi_randn_indexed", sample_index, shape_tail, torch.float32, out)
    check(load().dxmi_randn_indexed(_ptr(out), _ptr(sample_index), N, per, int(seed) & _U64, int(draw) & 0xFFFFFFFF, _stream()),
          "dxmi_randn_indexed")
    return out


def randint_indexed(sample_index, shape_tail, low, high, seed, draw, out=None):
    """Integers in [low, high), int64 [N, *shape_tail], from the words of the same generator (dxmi_randint_indexed): row n is a
    function of (seed, sample_index[n], draw) alone.  1 <= high - low <= 2^31."""
    N, per, out = _indexed_operands("dxmi_randint_indexed", sample_index, shape_tail, torch.int64, out)
    check(load().dxmi_randint_indexed(_ptr(out), _ptr(sample_index), N, per, int(low), int(high), int(seed) & _U64,
                                      int(draw) & 0xFFFFFFFF, _stream()), "dxmi_randint_indexed")
    return out


def _step_indexed_operands(what, x, net_out, sample_index, ctl, per_sample, same, logp=None):
    """The checks of the transitions that make their own noise: the checks of the indexed draws (_indexed_operands) on sample_index and
    the state's shape tail, then x and net_out fp32 contiguous [N, ...] with a multiple of 4 elements per row, `same` (outputs, None
    allowed) of that shape, `per_sample` fp32 contiguous with N elements, ctl (if given) a contiguous int32 [4].  The shapes are
    judged before the devices, so a malformed call is named as such on a host without a device too.  -> (N, CHW)."""
    if x.dim() < 2 or x.numel() == 0 or x.dtype != torch.float32 or not x.is_contiguous():
        raise _lib.DxmiError(f"{what}: the state must be a non-empty fp32 contiguous batch [N, ...], got {x.dtype} {tuple(x.shape)}")
    N = x.shape[0]
    chw = x.numel() // N
    if chw % 4:
        raise _lib.DxmiError(f"{what}: a row must hold a multiple of 4 elements, got {chw}")
    if not torch.is_tensor(sample_index) or sample_index.shape != (N,):
        raise _lib.DxmiError(f"{what}: sample_index must hold the state's {N} rows")
    for v in (net_out,) + tuple(same):
        if v is not None and not (v.dtype == torch.float32 and v.is_contiguous() and v.shape == x.shape and v.device == x.device):
            raise _lib.DxmiError(f"{what}: fp32 contiguous tensors of the state's shape {tuple(x.shape)} on its device")
    for v in tuple(per_sample) + (logp,):
        if v is not None and not (v.dtype == torch.float32 and v.is_contiguous() and v.numel() == N and v.device == x.device):
            raise _lib.DxmiError(f"{what}: the per-sample vectors must be fp32 contiguous with {N} elements on the state's device")
    if ctl is not None and not (ctl.dtype == torch.int32 and ctl.is_contiguous() and ctl.numel() == 4 and ctl.device == x.device):
        raise _lib.DxmiError(f"{what}: ctl must be a contiguous int32 [4] on the state's device")
    _need_cuda(x, net_out, ctl, logp, *per_sample, *same)
    _indexed_operands(what, sample_index, tuple(x.shape[1:]), torch.float32, x)
    return N, chw


def var_step_indexed(x, eps, sample_index, xmul, cmul, sigma, seed=0, draw=0, ctl=None, want_mean=True, want_control=True, outs=None,
                     assoc=0):
    """var_step with its noise made in the launch (dxmi_var_step_fwd_indexed): bit for bit var_step(x, eps, z, ...) on z =
    randn_indexed(sample_index, x.shape[1:], seed, draw).  ctl: an int32 [4] device block (unused, draw, seed low, seed high) that
    replaces draw / seed, so a captured launch is fed per replay.  outs = (x_next, mean, control, logp), the last three None or not."""
    what = "dxmi_var_step_fwd_indexed"
    if assoc not in (0, 1):
        raise _lib.DxmiError(f"{what}: assoc must be 0 or 1, got {assoc}")
    if outs is None:
        x_next = torch.empty_like(x)
        mean = torch.empty_like(x) if want_mean else None
        control = torch.empty_like(x) if want_control else None
        logp = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    else:
        x_next, mean, control, logp = outs
        if x_next is None:
            raise _lib.DxmiError(f"{what}: outs needs x_next")
    N, CHW = _step_indexed_operands(what, x, eps, sample_index, ctl, (xmul, cmul, sigma), (x_next, mean, control), logp)
    nb = 4.0 * N * CHW * (2 + 1 + (mean is not None) + (control is not None))
    _prof("sampler_step", "var_step_indexed", 0.0, nb, lambda: check(
        load().dxmi_var_step_fwd_indexed(_ptr(x), _ptr(eps), _ptr(sample_index), _ptr(ctl), int(draw) & 0xFFFFFFFF, int(seed) & _U64,
                                         _ptr(xmul), _ptr(cmul), _ptr(sigma), _ptr(x_next), _ptr(mean), _ptr(control), _ptr(logp), N,
                                         CHW, int(assoc), _stream()), what))
    return x_next, mean, control, logp


def edm_step_indexed(x, model_out, sample_index, sigma, sigma_down, sigma_up, sigma_data=0.5, seed=0, draw=0, ctl=None, outs=None):
    """edm_step with its noise made in the launch (dxmi_edm_step_fwd_indexed): bit for bit edm_step(x, model_out, z, ...) on z =
    randn_indexed(sample_index, x.shape[1:], seed, draw).  ctl as in var_step_indexed.  outs = (sample, mean)."""
    what = "dxmi_edm_step_fwd_indexed"
    sample, mean = (torch.empty_like(x), torch.empty_like(x)) if outs is None else outs
    if sample is None or mean is None:
        raise _lib.DxmiError(f"{what}: outs needs sample and mean")
    N, CHW = _step_indexed_operands(what, x, model_out, sample_index, ctl, (sigma, sigma_down, sigma_up), (sample, mean))
    check(load().dxmi_edm_step_fwd_indexed(_ptr(x), _ptr(model_out), _ptr(sample_index), _ptr(ctl), int(draw) & 0xFFFFFFFF,
                                           int(seed) & _U64, _ptr(sigma), _ptr(sigma_down), _ptr(sigma_up), _ptr(sample), _ptr(mean), N,
                                           CHW, float(sigma_data), _stream()), what)
    return sample, mean


def _sampler_stage(name, cols, mode, first, tab, t_out, row, x, eps, z, sample_index, seed, draw, ctl, out, pred_xstart, hist=(),
                   x_in=(), xc=(), slots=3):
    """The checks and the call of the stage launches of csrc/stage_common.h.  cols: the table's row length; first: the sampler's
    FIRST mode; hist: () for a sampler without a history, else (the tensor or None,), of `slots` slots; x_in: () for a sampler
    without the second output stream, else (the tensor or None,): FIRST then takes x and x_in, and a transition's x_in may be None on
    the table's last row given by value.  xc: () for a sampler with one state, else (the second state or None,): such an entry adds
    no noise and takes no draw, seed, z or sample_index."""
    _need_cuda(tab, t_out, x, eps, z, sample_index, ctl, *hist, *x_in, *xc, out, pred_xstart)
    if not (tab.dtype == torch.float32 and tab.is_contiguous() and tab.dim() == 2 and tab.shape[1] == cols and tab.shape[0] >= 1):
        raise _lib.DxmiError(f"{name}: tab must be a contiguous fp32 [rows, {cols}], got {tab.dtype} {tuple(tab.shape)}")
    if not (t_out.dtype == torch.float32 and t_out.is_contiguous() and t_out.dim() == 1):
        raise _lib.DxmiError(f"{name}: t_out must be a contiguous fp32 [N]")
    N = t_out.numel()
    chw = 1
    if mode == first and x_in:
        if x is None or x_in[0] is None:
            raise _lib.DxmiError(f"{name}: FIRST scales x and writes x_in: both are needed")
        for v in (x, x_in[0]):
            if not (v.dtype == torch.float32 and v.is_contiguous() and v.shape == x.shape):
                raise _lib.DxmiError(f"{name}: fp32 contiguous tensors of the state's shape {tuple(x.shape)}")
        if x.dim() < 2 or x.shape[0] != N or x.numel() == 0:
            raise _lib.DxmiError(f"{name}: the state [N, ...] must hold t_out's {N} samples, got {tuple(x.shape)}")
        chw = x.numel() // N
    if mode != first:
        if x is None or eps is None or out is None or any(h is None for h in hist):
            raise _lib.DxmiError(f"{name}: a transition needs x, eps{', hist' if hist else ''} and out")
        if x_in and x_in[0] is None and (ctl is not None or int(row) != tab.shape[0] - 1):
            raise _lib.DxmiError(f"{name}: x_in is needed on every row but the table's last, given by value")
        for v in (x, eps, z, out, pred_xstart, *x_in, *xc):
            if v is not None and not (v.dtype == torch.float32 and v.is_contiguous() and v.shape == x.shape):
                raise _lib.DxmiError(f"{name}: fp32 contiguous tensors of the state's shape {tuple(x.shape)}")
        if x.dim() < 2 or x.shape[0] != N or x.numel() == 0:
            raise _lib.DxmiError(f"{name}: the state [N, ...] must hold t_out's {N} samples, got {tuple(x.shape)}")
        for h in hist:
            if not (h.dtype == torch.float32 and h.is_contiguous() and tuple(h.shape) == (slots,) + tuple(x.shape)):
                raise _lib.DxmiError(f"{name}: hist must be a contiguous fp32 {(slots,) + tuple(x.shape)}, got {h.dtype} {tuple(h.shape)}")
        chw = x.numel() // N
        if sample_index is not None and not (sample_index.dtype == torch.int64 and sample_index.is_contiguous()
                                             and sample_index.shape == (N,)):
            raise _lib.DxmiError(f"{name}: sample_index must be a contiguous int64 [{N}]")
    if ctl is not None and not (ctl.dtype == torch.int32 and ctl.is_contiguous() and ctl.numel() == 4):
        raise _lib.DxmiError(f"{name}: ctl must be a contiguous int32 [4]")
    if xc:
        if z is not None or sample_index is not None:
            raise _lib.DxmiError(f"{name}: the solver adds no noise: neither z nor sample_index")
        if xc[0] is not None and x is not None and xc[0].data_ptr() == x.data_ptr():
            raise _lib.DxmiError(f"{name}: xc and x are two states: they may not be one tensor")
        check(getattr(load(), name)(int(mode), _ptr(tab), int(tab.shape[0]), _ptr(ctl), int(row), _ptr(x), _ptr(xc[0]), _ptr(eps),
                                    *(_ptr(h) for h in hist), *(_ptr(v) for v in x_in), _ptr(t_out), _ptr(out), _ptr(pred_xstart), N,
                                    chw, _stream()), name)
        return
    check(getattr(load(), name)(int(mode), _ptr(tab), int(tab.shape[0]), _ptr(ctl), int(row), int(draw) & 0xFFFFFFFF,
                                int(seed) & _U64, _ptr(x), _ptr(eps), _ptr(z), _ptr(sample_index), *(_ptr(h) for h in hist),
                                *(_ptr(v) for v in x_in), _ptr(t_out), _ptr(out), _ptr(pred_xstart), N, chw, _stream()), name)


# dxmi_ddpm_stage modes, table columns and flags (include/dxmi_hip.h)
DDPM_FIRST, DDPM_STEP = range(2)
DT_T, DT_T_NEXT, DT_XM, DT_C, DT_S, DT_A, DT_B, DT_Q, DT_R, DT_C0, DT_C1, DT_FLAGS = range(12)
DT_COLS = 16
DT_FLAG_CLIP, DT_FLAG_LAST = 1, 2


def ddpm_stage(mode, tab, t_out, row=0, x=None, eps=None, z=None, sample_index=None, seed=0, draw=0, ctl=None, out=None,
               pred_xstart=None):
    """One transition of the DDPM teacher's ancestral / DDIM samplers between two network evaluations (dxmi_ddpm_stage): x is
    updated in place, t_out [N] takes the next evaluation's time, out the clamped sample on the row flagged last.  tab: fp32
    [rows, DT_COLS] on the device.  Noise: z [N, ...] given, or sample_index (int64 [N]) with seed / draw: made in the launch, the
    values of randn_indexed.  ctl: an int32 [4] device block (row, draw, seed low, seed high) that replaces row / draw / seed: a
    captured launch then serves every row.  DDPM_FIRST writes t_out of `row` only."""
    _sampler_stage("dxmi_ddpm_stage", DT_COLS, mode, DDPM_FIRST, tab, t_out, row, x, eps, z, sample_index, seed, draw, ctl, out,
                   pred_xstart)


# dxmi_dpm_stage modes, table columns and flags (include/dxmi_hip.h)
DPM_FIRST, DPM_STEP = range(2)
MT_T, MT_T_NEXT, MT_CX, MT_W0, MT_W1, MT_W2, MT_S, MT_A, MT_B, MT_FLAGS, MT_ORDER = range(11)
MT_COLS = 16
MT_FLAG_CLIP, MT_FLAG_LAST = 1, 2


def dpm_stage(mode, tab, t_out, row=0, x=None, eps=None, z=None, sample_index=None, seed=0, draw=0, ctl=None, hist=None, out=None,
              pred_xstart=None):
    """One multistep DPM-Solver++ transition between two network evaluations (dxmi_dpm_stage): x is updated in place, this
    evaluation's data prediction goes to hist[row % 3] (hist: fp32 [3, *x.shape]; the two before it are read from the other slots
    where the row's weights are not 0), t_out [N] takes the next evaluation's time, out the clamped sample on the row flagged last.
    tab: fp32 [rows, MT_COLS] on the device.  Noise: z [N, ...] given, or sample_index (int64 [N]) with seed / draw: made in the
    launch, the values of randn_indexed.  ctl: an int32 [4] device block (row, draw, seed low, seed high) that replaces row / draw /
    seed: a captured launch then serves every row.  DPM_FIRST writes t_out of `row` only."""
    _sampler_stage("dxmi_dpm_stage", MT_COLS, mode, DPM_FIRST, tab, t_out, row, x, eps, z, sample_index, seed, draw, ctl, out,
                   pred_xstart, hist=(hist,))


# dxmi_edm_dpm_stage modes, table columns and flags (include/dxmi_hip.h): columns 0-10 are MT_*'s with c_skip, c_out for A, B
EDM_DPM_FIRST, EDM_DPM_STEP = range(2)
(ET_T, ET_T_NEXT, ET_CX, ET_W0, ET_W1, ET_W2, ET_S, ET_CSKIP, ET_COUT, ET_FLAGS, ET_ORDER, ET_CIN, ET_CIN_NEXT, ET_XSCALE,
 ET_SIGMA) = range(15)
ET_COLS = 16
ET_FLAG_CLIP, ET_FLAG_LAST = 1, 2


def edm_dpm_stage(mode, tab, t_out, row=0, x=None, model_out=None, z=None, sample_index=None, seed=0, draw=0, ctl=None, hist=None,
                  x_in=None, out=None, pred_xstart=None):
    """One multistep DPM-Solver++ transition of the EDM nets between two network evaluations (dxmi_edm_dpm_stage): model_out is
    turned into the data prediction by the Karras preconditioning and filed in hist[row % 3] (hist: fp32 [3, *x.shape]), x is
    updated in place, x_in takes the next evaluation's input c_in x' on every row that is not last, t_out [N] its time, out the
    clamped sample on the row flagged last.  tab: fp32 [rows, ET_COLS] on the device.  Noise and ctl as dpm_stage.
    EDM_DPM_FIRST scales x by the row's XSCALE in place and writes x_in = c_in x and t_out of `row`."""
    _sampler_stage("dxmi_edm_dpm_stage", ET_COLS, mode, EDM_DPM_FIRST, tab, t_out, row, x, model_out, z, sample_index, seed, draw, ctl,
                   out, pred_xstart, hist=(hist,), x_in=(x_in,))


# dxmi_unipc_stage modes, table columns and flags (include/dxmi_hip.h): MT_*'s columns (the solver has no noise: S's place holds the
# corrector's order) and the corrector's five
UNIPC_FIRST, UNIPC_STEP = range(2)
(UT_T, UT_T_NEXT, UT_CX, UT_W0, UT_W1, UT_W2, UT_CORDER, UT_A, UT_B, UT_FLAGS, UT_ORDER, UT_CCX, UT_CV0, UT_CV1, UT_CV2,
 UT_CV3) = range(16)
UT_COLS = 16
UT_FLAG_CLIP, UT_FLAG_LAST, UT_FLAG_CORR = 1, 2, 4


def unipc_stage(mode, tab, t_out, row=0, x=None, xc=None, eps=None, ctl=None, hist=None, out=None, pred_xstart=None):
    """One UniPC transition of the DDPM teacher between two network evaluations (dxmi_unipc_stage): this evaluation's data
    prediction goes to hist[row % 4] (hist: fp32 [4, *x.shape]), on a row flagged CORR the corrected state xc is re-done with it,
    x (the predicted state the network sees) and xc are updated in place, t_out [N] takes the next evaluation's time, out the
    clamped sample on the row flagged last.  xc None: no corrected state, every row runs uncorrected.  tab: fp32 [rows, UT_COLS] on
    the device.  ctl: an int32 [4] device block whose first word replaces row.  UNIPC_FIRST writes t_out of `row` only."""
    _sampler_stage("dxmi_unipc_stage", UT_COLS, mode, UNIPC_FIRST, tab, t_out, row, x, eps, None, None, 0, 0, ctl, out, pred_xstart,
                   hist=(hist,), xc=(xc,), slots=4)


# dxmi_edm_unipc_stage: ET_*'s columns (S's place holds the corrector's order) and the corrector's five
EDM_UNIPC_FIRST, EDM_UNIPC_STEP = range(2)
(EUT_T, EUT_T_NEXT, EUT_CX, EUT_W0, EUT_W1, EUT_W2, EUT_CORDER, EUT_CSKIP, EUT_COUT, EUT_FLAGS, EUT_ORDER, EUT_CIN, EUT_CIN_NEXT,
 EUT_XSCALE, EUT_SIGMA, EUT_CCX, EUT_CV0, EUT_CV1, EUT_CV2, EUT_CV3) = range(20)
EUT_COLS = 20
EUT_FLAG_CLIP, EUT_FLAG_LAST, EUT_FLAG_CORR = 1, 2, 4


def edm_unipc_stage(mode, tab, t_out, row=0, x=None, xc=None, model_out=None, ctl=None, hist=None, x_in=None, out=None,
                    pred_xstart=None):
    """One UniPC transition of the EDM nets between two network evaluations (dxmi_edm_unipc_stage): unipc_stage with the Karras
    preconditioning of edm_dpm_stage; x_in takes the next evaluation's input c_in x' on every row that is not last.  tab: fp32
    [rows, EUT_COLS] on the device.  EDM_UNIPC_FIRST scales x by the row's XSCALE in place and writes x_in = c_in x and t_out."""
    _sampler_stage("dxmi_edm_unipc_stage", EUT_COLS, mode, EDM_UNIPC_FIRST, tab, t_out, row, x, model_out, None, None, 0, 0, ctl, out,
                   pred_xstart, hist=(hist,), x_in=(x_in,), xc=(xc,), slots=4)


# dxmi_pf_ll_stage modes, table columns and flags (include/dxmi_hip.h)
PF_LL_FIRST, PF_LL_PREDICT, PF_LL_CORRECT = range(3)
(PL_T, PL_T_NEXT, PL_CIN, PL_CIN_NEXT, PL_XSCALE, PL_LOGDET0, PL_KA, PL_KB, PL_DB, PL_KA2, PL_KB2, PL_DB2, PL_H, PL_HH, PL_FLAGS,
 PL_PRIOR_Q, PL_PRIOR_C, PL_BPD_SCALE, PL_SIGMA, PL_SIGMA_NEXT) = range(20)
PL_COLS = 20
PL_FLAG_LAST = 2


def pf_ll_stage(mode, tab, t_out, row=0, x=None, model_out=None, vjp=None, eps=None, sample_index=None, seed=0, draw=0, ctl=None,
                k1=None, xt=None, x_in=None, div1=None, ell=None, prior=None, logp=None, bpd=None):
    """The launch after each evaluation of the probability-flow likelihood (dxmi_pf_ll_stage): Heun on (x, ell) over the rows of
    tab (fp32 [rows, PL_COLS] on the device).  PF_LL_FIRST scales x by the row's XSCALE in place, writes x_in = c_in x, t_out and
    ell = logdet0.  PF_LL_PREDICT (model_out = F, vjp = g of the evaluation at x): writes k1, xt (if given), x_in = c_in_next xt,
    t_out and the per-image div1; x is read only.  PF_LL_CORRECT (F, g of the evaluation at xt): x in place, x_in, t_out,
    ell += (h / 2)(div1 + div2) and, on the row flagged last, prior, logp and bpd.  The probe: eps [N, ...] given, or sample_index
    (int64 [N]) with seed / draw: Rademacher signs made in the launch, the signs of randn_indexed's normals.  ctl: an int32 [4]
    device block (row, draw, seed low, seed high) that replaces row / draw / seed.  t_out, div1, ell, prior, logp, bpd: fp32 [N]."""
    name = "dxmi_pf_ll_stage"
    same, per = (x, model_out, vjp, eps, k1, xt, x_in), (t_out, div1, ell, prior, logp, bpd)
    _need_cuda(tab, ctl, sample_index, *same, *per)
    if mode not in (PF_LL_FIRST, PF_LL_PREDICT, PF_LL_CORRECT):
        raise _lib.DxmiError(f"{name}: unknown mode {mode}")
    if not (tab.dtype == torch.float32 and tab.is_contiguous() and tab.dim() == 2 and tab.shape[1] == PL_COLS and tab.shape[0] >= 1):
        raise _lib.DxmiError(f"{name}: tab must be a contiguous fp32 [rows, {PL_COLS}], got {tab.dtype} {tuple(tab.shape)}")
    if t_out is None or not (t_out.dtype == torch.float32 and t_out.is_contiguous() and t_out.dim() == 1):
        raise _lib.DxmiError(f"{name}: t_out must be a contiguous fp32 [N]")
    N = t_out.numel()
    if x is None or x.dim() < 2 or x.shape[0] != N or x.numel() == 0:
        raise _lib.DxmiError(f"{name}: the state [N, ...] must hold t_out's {N} images")
    need = {PF_LL_FIRST: dict(x_in=x_in, ell=ell),
            PF_LL_PREDICT: dict(model_out=model_out, vjp=vjp, k1=k1, x_in=x_in, div1=div1),
            PF_LL_CORRECT: dict(model_out=model_out, vjp=vjp, k1=k1, div1=div1, ell=ell, prior=prior, logp=logp, bpd=bpd)}[mode]
    missing = [k for k, v in need.items() if v is None]
    if missing:
        raise _lib.DxmiError(f"{name}: mode {mode} needs {', '.join(missing)}")
    if mode != PF_LL_FIRST and (eps is None) == (sample_index is None):
        raise _lib.DxmiError(f"{name}: the probe is either given (eps) or made in the launch (sample_index): exactly one")
    if x_in is None and (ctl is not None or int(row) != tab.shape[0] - 1):
        raise _lib.DxmiError(f"{name}: x_in is needed on every row but the table's last, given by value")
    for v in same:
        if v is not None and not (v.dtype == torch.float32 and v.is_contiguous() and v.shape == x.shape):
            raise _lib.DxmiError(f"{name}: fp32 contiguous tensors of the state's shape {tuple(x.shape)}")
    for v in per:
        if v is not None and not (v.dtype == torch.float32 and v.is_contiguous() and v.shape == (N,)):
            raise _lib.DxmiError(f"{name}: the per-image vectors must be contiguous fp32 [{N}]")
    if sample_index is not None and not (sample_index.dtype == torch.int64 and sample_index.is_contiguous()
                                         and sample_index.shape == (N,)):
        raise _lib.DxmiError(f"{name}: sample_index must be a contiguous int64 [{N}]")
    if ctl is not None and not (ctl.dtype == torch.int32 and ctl.is_contiguous() and ctl.numel() == 4):
        raise _lib.DxmiError(f"{name}: ctl must be a contiguous int32 [4]")
    first = mode == PF_LL_FIRST
    check(load().dxmi_pf_ll_stage(int(mode), _ptr(tab), int(tab.shape[0]), _ptr(ctl), int(row), int(draw) & 0xFFFFFFFF,
                                  int(seed) & _U64, _ptr(x), _ptr(model_out), _ptr(vjp), None if first else _ptr(eps),
                                  None if first else _ptr(sample_index), _ptr(k1), _ptr(xt), _ptr(x_in), _ptr(t_out), _ptr(div1),
                                  _ptr(ell), _ptr(prior), _ptr(logp), _ptr(bpd), N, x.numel() // N, _stream()), name)


# ------------------------------------------------------------------------------------------ InceptionV3 of the FID (f4)
class PackedGConv:
    """BatchNorm-folded bf16 weights [ceil32(Cout)][KH * KW][ceil16(Cin)] + fp32 bias of one BasicConv2d (dxmi_gconv_pack)."""

    __slots__ = ("w", "bias", "Cout", "Cin", "CinP", "KH", "KW")

    def __init__(self, w, bias, Cout, Cin, CinP, KH, KW):
        self.w, self.bias, self.Cout, self.Cin, self.CinP, self.KH, self.KW = w, bias, Cout, Cin, CinP, KH, KW


def gconv_pack(weight, bn=None, eps=1e-3, bias=None):
    """weight fp32 [Cout, Cin, KH, KW]; bn = (gamma, beta, running_mean, running_var) or None; bias fp32 [Cout] of a convolution
    without BatchNorm (None: zero)."""
    _need_cuda(weight)
    w = weight.detach().float().contiguous()
    Cout, Cin, KH, KW = w.shape
    conv_bias, lib = bias, load()
    wp = torch.empty(int(lib.dxmi_gconv_packed_elems(Cout, Cin, KH, KW)), dtype=torch.bfloat16, device=w.device)
    CoutP, CinP = (Cout + 31) // 32 * 32, (Cin + 15) // 16 * 16
    bias = torch.empty(CoutP, dtype=torch.float32, device=w.device)
    bnp = [t.detach().float().contiguous() for t in bn] if bn is not None else [None] * 4
    check(lib.dxmi_gconv_pack(_ptr(w), _ptr(bnp[0]), _ptr(bnp[1]), _ptr(bnp[2]), _ptr(bnp[3]), float(eps), _ptr(wp), _ptr(bias), Cout, Cin, KH, KW,
                              _stream()), "dxmi_gconv_pack")
    if conv_bias is not None:
        assert bn is None and conv_bias.numel() == Cout, "gconv_pack: bias is [Cout] and excludes bn"
        bias[:Cout].copy_(conv_bias.detach().float().reshape(Cout))
    return PackedGConv(wp, bias, Cout, Cin, CinP, KH, KW)


def gconv(x, pk, stride=(1, 1), pad=(0, 0), relu=True, out=None, coff=0):
    """x NHWC bf16 [N, IH, IW, pk.CinP] -> NHWC bf16 [N, OH, OW, Cout] (or the channel window [coff, coff + Cout) of `out`)."""
    _need_cuda(x, out)
    N, IH, IW, C = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and C == pk.CinP, f"gconv: input has {C} channels, the packed weight wants {pk.CinP}"
    OH, OW = (IH + 2 * pad[0] - pk.KH) // stride[0] + 1, (IW + 2 * pad[1] - pk.KW) // stride[1] + 1
    if out is None:
        out = torch.empty((N, OH, OW, pk.Cout), dtype=torch.bfloat16, device=x.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape[:3]) == (N, OH, OW)
    fl = 2.0 * N * OH * OW * pk.Cout * pk.Cin * pk.KH * pk.KW
    _prof("inception", f"gconv{pk.KH}x{pk.KW}", fl, 2.0 * (x.numel() + N * OH * OW * pk.Cout + pk.w.numel()), lambda: check(
        load().dxmi_gconv_fwd(_ptr(x), _ptr(pk.w), _ptr(pk.bias), _ptr(out), N, IH, IW, C, pk.Cout, pk.KH, pk.KW, stride[0], stride[1], pad[0],
                              pad[1], out.shape[3], coff, int(relu), _stream()), "dxmi_gconv_fwd"))
    return out


def pool3x3(x, stride, pad, avg_exclude_pad=False, out=None, coff=0):
    """3x3 max pool, or the average over the in-bounds pixels of the window (count_include_pad=False)."""
    _need_cuda(x, out)
    N, IH, IW, C = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    OH, OW = (IH + 2 * pad - 3) // stride + 1, (IW + 2 * pad - 3) // stride + 1
    if out is None:
        out = torch.empty((N, OH, OW, C), dtype=torch.bfloat16, device=x.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape[:3]) == (N, OH, OW)
    check(load().dxmi_pool3x3(_ptr(x), _ptr(out), N, IH, IW, C, stride, pad, int(avg_exclude_pad), out.shape[3], coff, _stream()), "dxmi_pool3x3")
    return out


def global_avgpool(x):
    _need_cuda(x)
    N, H, W, C = x.shape
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    check(load().dxmi_global_avgpool(_ptr(x), _ptr(out), N, H * W, C, _stream()), "dxmi_global_avgpool")
    return out


def resize_bilinear_nhwc16(x, OH, OW, normalize=True):
    """NCHW fp32 [N, 3, H, W] -> NHWC bf16 [N, OH, OW, 16] (bilinear, align_corners=False; 2 x - 1 when normalize)."""
    _need_cuda(x)
    N, C, H, W = x.shape
    assert C == 3 and x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty((N, OH, OW, 16), dtype=torch.bfloat16, device=x.device)
    check(load().dxmi_resize_bilinear_nhwc16(_ptr(x), _ptr(out), N, H, W, OH, OW, int(normalize), _stream()), "dxmi_resize_bilinear_nhwc16")
    return out
