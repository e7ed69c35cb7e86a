"""Shape census of the forward launches of the sampling and training programs (used by test_hip_forward_shapes.py).

`FwdCensus` intercepts every public function of `dxmi_hip.ops` (backward_census.Census: "record or refuse") and records a
signature for every launch op (FWD_OPS, the network kernels, and STEP_OPS, the non-network forward launches of a step) called
OUTSIDE the instrumented backward() methods (backward_census.Census.region_classes); a call that is neither a launch op nor on
the allow-list backward_census.ALLOWED nor a backward launch op called from a backward lands in
`FwdCensus.unknown`.  A row holds operand shapes plus every field that takes part in choosing a kernel or an epilogue, including the conv kernel id dxmi_conv2d_kernel_id reports for the launch (read through an ops.PROFILER, as
tools/conv_shapes.py does) and the knobs in effect.  The programs (PROGRAMS) run eagerly with graphs off, each under the tuning
it really uses.  For every GroupNorm row the census also keeps the largest |mean| / std over (image, group) of the activation
it normalised (`cond`): these are random-init nets, not trained weights, so this measures the conditioning of the census's own
activations only.
"""
import ctypes
import inspect

import torch

import backward_census

FWD_OPS = ("conv2d", "linear", "groupnorm_silu", "groupnorm_apply", "groupnorm_generic", "block_stats", "fold_stats",
           "gn_blockstats_to_generic", "attention", "attention_proj", "attn_block", "timestep_embedding", "upsample2x", "pool_act",
           "value_head")
# Non-network forward launches of a step: the DSM loss kernels, the TD kernels (td_loss also returns the gradient: it has a row
# in both censuses), dropout, the input layout conversion, the sampler stages and transitions
STEP_OPS = ("dropout", "nchw_f32_to_nhwc_bf16", "edm_dsm_prep", "edm_dsm_loss_fwd", "td_gather_cost", "td_loss", "karras_stage",
            "cm_stage", "var_step", "edm_step", "groupnorm_silu_shortcut", "edm_precond", "var_gather_sched", "nhwc_bf16_to_nchw_f32",
            "quantize_u8")
THROUGHPUT_KNOBS = (96, 13)          # (conv_ws_min_tiles, conv_sm_mask) under ops.throughput_tuning()


def _c(t):
    return 0 if t is None else int(t.shape[-1])


# Dispatch overrides that would make attention_kernel() name a kernel that did not run (csrc/attention.hip attention_fwd_impl)
ATTN_ENV = ("DXMI_ATTN64", "DXMI_ATTN_GENERIC")


def attention_kernel(T, C, heads, proj=False):
    """The attention kernel dxmi_attention_fwd / dxmi_attention_proj_fwd launch for the shape.  The library exports no query for
    this choice, so this mirrors attention_fwd_impl (csrc/attention.hip: 256 x 256 single head -> attention256_kernel, D = 256 /
    128 -> attention_kernel<D>, D = 64 with T % 256 == 0 -> attention64_kernel, else attention_kernel<64>); FwdCensus refuses
    to record while an ATTN_ENV override is set, and a change of that dispatch must be mirrored here."""
    D = C // heads
    if proj:
        return "attention256<true>"
    if D == 256 and T == 256 and heads == 1:
        return "attention256<false>"
    if D == 64 and T % 256 == 0:
        return "attention64"
    return f"attention_kernel<{D}>"


class FwdCensus(backward_census.Census):
    """`with FwdCensus(ops) as c:` ... c.rows = set of forward launch signatures, c.cond[row] = largest |mean| / std seen."""

    def __init__(self, ops):
        super().__init__(ops)
        self.cond, self.kid, self.gn_frames = {}, None, []
        self.sigs = {n: inspect.signature(getattr(ops, n)) for n in FWD_OPS + STEP_OPS}

    def tuning(self):
        knobs = (self.ops.get_tuning("conv_ws_min_tiles"), self.ops.get_tuning("conv_sm_mask"))
        return "throughput" if knobs == THROUGHPUT_KNOBS else "default"

    def _gn_cond(self, row, x, in1, groups):
        xc = torch.cat([x, in1], -1) if in1 is not None else x
        N, C = xc.shape[0], xc.shape[-1]
        g = xc.reshape(N, -1, groups, C // groups).float()
        m = g.mean((1, 3))
        sd = (g - m[:, None, :, None]).square().mean((1, 3)).sqrt()
        r = float((m.abs() / sd.clamp_min(1e-30)).max())
        self.cond[row] = max(self.cond.get(row, 0.0), round(r, 3))

    def _wrap(self, name, fn):
        if name not in self.sigs:
            judged = name in backward_census.ALLOWED

            def other(*a, **kw):
                # inside a backward(): the backward census judges the call; outside, a backward launch op is as unknown as any
                if not self.depth and not judged:
                    self.unknown.add(name)
                return fn(*a, **kw)
            return other
        sig = self.sigs[name]

        def w(*a, **kw):
            if self.depth:
                return fn(*a, **kw)
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            p = b.arguments
            if name == "groupnorm_silu":
                self.gn_frames.append(False)
                try:
                    out = fn(*a, **kw)
                finally:
                    served = self.gn_frames.pop()
                if not served:
                    x, in1 = p["x"], p["in1"]
                    row = ("gn", "resident", tuple(x.shape), _c(in1), int(p["groups"]), float(p["eps"]), bool(p["silu"]), False, False,
                           0, 0)
                    self.rows.add(row)
                    self._gn_cond(row, x, in1, int(p["groups"]))
                return out
            if name == "conv2d":
                self.kid = None
                out = fn(*a, **kw)
                self.rows.add(self._conv_row(p, out))
                return out
            out = fn(*a, **kw)
            row = self._row(name, p, out)
            if row is None:                     # the op declined the shape and launched nothing (groupnorm_silu_shortcut)
                return out
            self.rows.add(row)
            if row[0] == "gn":
                if self.gn_frames:
                    self.gn_frames[-1] = True
                self._gn_cond(row, p["x"], p["in1"], int(p["groups"]))
            return out
        return w

    def _conv_row(self, p, out):
        x, pw = p["x"], p["pw"]
        k = pw.ksize
        pad = k // 2 if p["pad"] is None else int(p["pad"])
        av = p["addvec"]
        addvec = "-" if av is None else ("image" if av.dim() == 2 else "shared")
        fg = p["fuse_gn"]
        fuse = None if fg is None else (int(fg[2]), bool(fg[4]), bool(fg[5]))
        P = 0
        if p["want_stats"] and out[1] is not None:
            P = out[1].P
        kid, gn_out = self.kid
        if fg is not None:
            fuse = fuse + (bool(gn_out),)                    # whether the selected kernel wrote the normalised tensor itself
        return ("conv2d", tuple(x.shape), _c(p["in1"]), pw.Cout, k, bool(pw.k27), int(p["stride"]), pad, p["pad_br"],
                int(p["upsample"] or 0), p["bias"] is not None, addvec, p["residual"] is not None, p["mask_src"] is not None,
                int(p["act"]), bool(p["out_nchw_f32"]), bool(p["want_stats"]), fuse, int(p["variant"]), P, self.tuning(), kid)

    def _row(self, name, p, out):
        ops = self.ops
        if name in ("linear", "upsample2x", "pool_act"):
            return backward_census.forward_style_row(ops, name, p)
        has = lambda *names: tuple(n for n in names if p[n] is not None)
        if name == "dropout":
            return backward_census._NEW["dropout"](p)
        if name == "td_loss":
            return backward_census._NEW["td_loss"](p)
        if name == "nchw_f32_to_nhwc_bf16":
            return ("nchw_f32_to_nhwc_bf16", tuple(p["x"].shape))
        if name == "edm_dsm_prep":
            return ("edm_dsm_prep", tuple(p["x_start"].shape))
        if name == "edm_dsm_loss_fwd":
            return ("edm_dsm_loss_fwd", tuple(p["x_start"].shape), p["weight_schedule"], bool(p["distillation"]))
        if name == "td_gather_cost":
            return ("td_gather_cost", int(p["state_rows"].numel()), int(p["traj2d"].shape[1]), has("next_rows", "next_dense"))
        if name == "karras_stage":
            return ("karras_stage", int(p["mode"]), bool(p["last"]), tuple(p["x"].shape),
                    has("x2", "d", "model_out", "noise", "x_in", "t", "out", "denoised"))
        if name == "cm_stage":
            return ("cm_stage", int(p["mode"]), int(p["edit"]), bool(p["last"]), tuple(p["x"].shape),
                    has("Q", "model_out", "noise", "ref", "mask", "x_in", "t", "out", "denoised"))
        if name == "var_step":
            outs = p["outs"]
            mean, control = (p["want_mean"], p["want_control"]) if outs is None else (outs[1] is not None, outs[2] is not None)
            return ("var_step", tuple(p["x"].shape), bool(mean), bool(control), int(p["assoc"]))
        if name == "edm_step":
            return ("edm_step", tuple(p["x"].shape))
        if name == "groupnorm_silu_shortcut":
            if out is None:
                return None
            st = p["stats"]
            return ("gn_shortcut", tuple(p["x"].shape), _c(p["in1"]), p["pw"].Cout, int(p["groups"]), float(p["eps"]), bool(p["silu"]),
                    p["bias"] is not None, st[0].P, st[1].P if p["in1"] is not None else 0)
        if name == "edm_precond":
            return ("edm_precond", tuple(p["x"].shape))
        if name == "var_gather_sched":
            return ("var_gather_sched", int(p["t"].numel()), int(p["continuous_steps"].numel()))
        if name == "nhwc_bf16_to_nchw_f32":
            return ("nhwc_bf16_to_nchw_f32", tuple(p["x"].shape))
        if name == "quantize_u8":
            return ("quantize_u8", tuple(p["x"].shape), int(p["mode"]), bool(p["nhwc"]))
        if name in ("groupnorm_apply", "groupnorm_generic"):
            x, in1 = p["x"], p["in1"]
            if name == "groupnorm_apply":
                path, saved, P0, P1 = "apply", False, p["st"].P, (p["st1"].P if p["st1"] is not None else 0)
            else:
                path, saved, P0, P1 = "generic", p["saved"] is not None, 0, 0
            return ("gn", path, tuple(x.shape), _c(in1), int(p["groups"]), float(p["eps"]), bool(p["silu"]),
                    p["scale_shift"] is not None, saved, P0, P1)
        if name == "block_stats":
            return ("block_stats", tuple(p["x"].shape), int(ops.load().dxmi_gn_block_stats_partials(p["x"].shape[1] * p["x"].shape[2])))
        if name == "fold_stats":
            N, P, C2, _ = p["st"].buf.shape
            return ("fold_stats", int(N), int(P), int(C2) * 2, int(p["group"]))
        if name == "gn_blockstats_to_generic":
            return ("gn_bs2gen", int(p["N"]), int(p["HW"]), int(p["C0"]), int(p["C1"]), int(p["groups"]), p["st0"].P,
                    p["st1"].P if p["st1"] is not None else 0)
        if name == "attention":
            N, T, C3 = p["qkv"].shape
            lse = out[1] is not None if p["want_lse"] else False
            return ("attention", int(N), int(T), C3 // 3, int(p["heads"]), bool(p["want_lse"]), lse,
                    attention_kernel(T, C3 // 3, int(p["heads"])))
        if name == "attention_proj":
            N, T, C3 = p["qkv"].shape
            return ("attention_proj", int(N), int(T), C3 // 3, int(p["heads"]), bool(p["want_stats"]))
        if name == "attn_block":
            return ("attn_block", tuple(p["x"].shape), p["stats"].P, bool(p["want_stats"]))
        if name == "timestep_embedding":
            return ("timestep_embedding", int(p["t"].numel()), int(p["dim"]), int(p["order"]), float(p["max_period"]))
        if name == "value_head":
            return ("value_head", tuple(p["x"].shape), p["out_w"] is not None)
        raise KeyError(name)

    def __enter__(self):
        import os
        assert not [v for v in ATTN_ENV if v in os.environ], f"unset {ATTN_ENV}: attention_kernel() names the default dispatch"
        ops, census = self.ops, self

        class _KernelIdProbe(ops.OpProfiler):
            """Launches unchanged; the conv launch notes the kernel id it runs (tools/conv_shapes.py reads it the same way)."""

            def bracket(self, cls, name, flops, nbytes, fn):
                return fn()

            def launch_conv(self, d):
                lib = ops.load()
                census.kid = (int(lib.dxmi_conv2d_kernel_id(ctypes.byref(d))), bool(d.gn_out))
                ops.check(lib.dxmi_conv2d_fwd(ctypes.byref(d), ops._stream()), "dxmi_conv2d_fwd")

        self.saved[(ops, "PROFILER")] = ops.PROFILER
        ops.PROFILER = _KernelIdProbe()
        self._instrument()
        return self


def conv_kernel_id(ops, r):
    """dxmi_conv2d_kernel_id of a conv2d census row under its recorded tuning: a host-side query (no launch, no device memory)."""
    return conv_query(ops, r, "dxmi_conv2d_kernel_id")


def conv_query(ops, r, fn, *args, **fields):
    """lib.fn(descriptor of a conv2d census row, *args) under the row's recorded tuning, with `fields` set on the descriptor: a
    host-side query (no launch, no device memory)."""
    (_, xs, c1, Cout, k, k27, stride, pad, pad_br, ups, has_bias, addvec, has_res, has_mask, act, nchw, want_stats, fuse, variant,
     P, tuning, kid) = r
    d = ops.ConvDesc()
    if k27:
        N, _, IH, IW = xs
        C0 = 3
    else:
        N, IH, IW, C0 = xs
    pb = pad if pad_br is None else pad_br
    VH, VW = (2 * IH, 2 * IW) if ups else (IH, IW)
    d.in0, d.in1, d.wpacked, d.out = 16, (16 if c1 else None), 16, 16
    d.bias = 16 if has_bias else None
    d.addvec, d.addvec_ld = (16 if addvec != "-" else None), (3 * Cout if addvec == "image" else 0)
    d.residual, d.mask_src, d.gn_stats, d.gn_out = (16 if has_res else None), (16 if has_mask else None), None, None
    d.N, d.IH, d.IW, d.C0, d.C1, d.Cout = N, IH, IW, C0, c1, Cout
    d.OH, d.OW = (VH + pad + pb - k) // stride + 1, (VW + pad + pb - k) // stride + 1
    d.ksize, d.stride, d.pad, d.upsample, d.act = k, stride, pad, ups, act
    d.in_mode = ops.IN_NCHW_F32_K27 if k27 else ops.IN_NHWC_BF16
    d.out_mode = ops.OUT_NCHW_F32 if nchw else ops.OUT_NHWC_BF16
    d.variant = variant
    for name, v in fields.items():
        setattr(d, name, v)
    tune = ops.throughput_tuning() if tuning == "throughput" else backward_census._nullctx()
    with tune:
        return int(getattr(ops.load(), fn)(ctypes.byref(d), *args))


def cifar10_sample(device, B, T):
    """VARSampler.sample of generate_cifar10.py (cifar10_T10 DDPM U-Net) at batch B, T steps, random init."""
    import configs_builtin
    from models.DxMI.unet_small import Model
    from models.DxMI.var_sampler import VARSampler
    kw = {k: v for k, v in configs_builtin.CONFIGS["cifar10_T10"]["sampler_net"].items() if k != "_target_"}
    torch.manual_seed(0)
    sampler = VARSampler(Model(**kw), T, [3, 32, 32], trainable_beta="fix_last").to(device).eval()
    sampler.use_graph = False
    with torch.no_grad():
        sampler.sample(B, device=device)
    torch.cuda.synchronize()


def edm_sample(device, name, B, class_cond):
    """OpenAIDiffusion.sample of generate_large.py on the named EDM / ADM net, set up as bench.py's generation leg sets it up
    (random init, zero-initialised layers given weights); class_cond: one random label per image."""
    import configs_builtin
    from models.cm.script_util import create_model_and_diffusion
    from models.DxMI.openai_diffusion import OpenAIDiffusion
    cfg = configs_builtin.get(name)
    torch.manual_seed(0)
    with torch.device(device):
        net, diffusion = create_model_and_diffusion(**cfg.diffusion)
    with torch.no_grad():
        for p in net.parameters():
            if float(p.abs().max()) == 0:
                torch.nn.init.normal_(p, std=0.02)
    s = OpenAIDiffusion(net, diffusion, **cfg.sampler)
    net.to(device).eval()
    s.use_graph = False
    kw = {}
    if class_cond:
        kw["i_class"] = torch.randint(0, 1000, (B,), device=device, generator=torch.Generator(device=device).manual_seed(1))
    with torch.no_grad():
        s.sample(B, device=device, **kw)
    torch.cuda.synchronize()
    del s, net


def edm_teacher(device):
    """The class-conditional ImageNet-64 EDM net as generate_large.py --karras_sampler / --cm_sampler sets it up (imagenet64_T10's
    diffusion block, fp16 conversion, eval mode), random init with the zero-initialised layers given weights."""
    import configs_builtin
    from models.cm.script_util import create_model_and_diffusion
    cfg = configs_builtin.get("imagenet64_T10")
    torch.manual_seed(0)
    with torch.device(device):
        net, diffusion = create_model_and_diffusion(**cfg.diffusion)
    with torch.no_grad():
        for p in net.parameters():
            if float(p.abs().max()) == 0:
                torch.nn.init.normal_(p, std=0.02)
    net.to(device)
    if cfg.diffusion.use_fp16:
        net.convert_to_fp16()
    net.eval()
    return net, diffusion


def _labels(device, B):
    return torch.randint(0, 1000, (B,), device=device, generator=torch.Generator(device=device).manual_seed(1))


def karras_heun(device, B, steps=3):
    """karras_sample(..., sampler="heun") of generate_large.py --karras_sampler heun at batch B, graphs off.  `steps` = 3 gives
    two Heun steps with the corrector and the final Euler step: the launch signatures of the documented 40 steps."""
    from models.cm.karras_diffusion import karras_sample
    net, diffusion = edm_teacher(device)
    with torch.no_grad():
        karras_sample(diffusion, net, (B, 3, 64, 64), steps, model_kwargs={"y": _labels(device, B)}, device=device,
                      sigma_min=diffusion.sigma_min, sigma_max=diffusion.sigma_max, sampler="heun", use_graph=False)
    torch.cuda.synchronize()
    del net


def cm_multistep(device, B):
    """generate_large.py --cm_sampler multistep --ts 0,22,39 (steps 40, distillation=True) at batch B, graphs off."""
    from models.cm.karras_diffusion import karras_sample
    net, diffusion = edm_teacher(device)
    diffusion.distillation = True
    with torch.no_grad():
        karras_sample(diffusion, net, (B, 3, 64, 64), 40, model_kwargs={"y": _labels(device, B)}, device=device,
                      sigma_min=diffusion.sigma_min, sigma_max=diffusion.sigma_max, sampler="multistep", ts=(0, 22, 39),
                      use_graph=False)
    torch.cuda.synchronize()
    del net


def cm_inpainting(device, B=14):
    """iterative_inpainting (zero-shot editing) on the full-size net at the batch tests/test_hip_cm_sample.py drives it with
    (14 images, ts = (0, 10, 20), steps 40, a mask that keeps the first seven images)."""
    from models.cm import karras_diffusion as kd
    net, diffusion = edm_teacher(device)
    diffusion.distillation = True
    g = torch.Generator(device=device).manual_seed(5)
    images = torch.rand(B, 3, 64, 64, device=device, generator=g) * 2 - 1
    x = torch.randn(B, 3, 64, 64, device=device, generator=g) * 80.0
    mask = torch.zeros_like(x)
    mask[: B // 2] = 1.0
    with torch.no_grad():
        kd.iterative_inpainting(kd.KarrasDenoiserFn(diffusion, net, True, {"y": _labels(device, B)}), images, x, (0, 10, 20),
                                steps=40, generator=None, mask=mask)
    torch.cuda.synchronize()
    del net


# program -> (runner(device), tuning)
PROGRAMS = {
    "edm_dsm_train_b16": (lambda d: backward_census.edm_dsm_step(d, 16), "default"),
    "edm_dsm_train_b32": (lambda d: backward_census.edm_dsm_step(d, 32), "default"),
    "imagenet64_karras_heun_b100": (lambda d: karras_heun(d, 100), "default"),
    "imagenet64_cm_multistep_b100": (lambda d: cm_multistep(d, 100), "default"),
    "imagenet64_cm_inpainting_b14": (lambda d: cm_inpainting(d, 14), "default"),
    "cifar10_sample_T10_b256": (lambda d: cifar10_sample(d, 256, 10), "default"),
    "cifar10_sample_T10_b32": (lambda d: cifar10_sample(d, 32, 10), "default"),
    "cifar10_sample_T4_b128": (lambda d: cifar10_sample(d, 128, 4), "default"),
    "cifar10_train_b256": (lambda d: backward_census.cifar10_step(d, 256), "throughput"),
    "cifar10_train_b128": (lambda d: backward_census.cifar10_step(d, 128), "throughput"),
    "cifar10_train_b32": (lambda d: backward_census.cifar10_step(d, 32), "throughput"),
    "imagenet64_sample_b100": (lambda d: edm_sample(d, "imagenet64_T10", 100, True), "default"),
    "imagenet64_train_b16": (lambda d: backward_census.imagenet64_step(d, 16), "throughput"),
    "lsun_sample_T4_b16": (lambda d: edm_sample(d, "lsun_bedroom_T4", 16, False), "default"),
}


def record(ops, program, device="cuda:0"):
    """(rows, cond, unknown) of one program's forward launches, under the tuning the program uses."""
    run, tuning = PROGRAMS[program]
    with backward_census.tuned(ops, tuning), FwdCensus(ops) as c:
        run(device)
    torch.cuda.empty_cache()
    return c.rows, c.cond, sorted(c.unknown)
