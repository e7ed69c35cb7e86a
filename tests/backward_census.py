"""Shape census of the backward launches of the training programs (used by test_hip_backward_shapes.py).

`Census` intercepts EVERY public function of `dxmi_hip.ops` while it is active.  A call made inside an instrumented region is
one of: a launch op (LAUNCH: it gets a signature row: operand shapes plus every flag that takes part in the kernel choice), a
helper on the commented allow-list ALLOWED (it launches nothing a row could describe), or unknown: its name lands in `Census.unknown` and test_census_is_covered fails
naming it ("record or refuse").  The instrumented region is every autograd backward of the recorded steps that launches a
project kernel: the backward() methods of REGION_CLASSES (the three network functions of models/cm/unet_train.py,
models/DxMI/unet_small_train.py and models/value_train.py, the DSM loss node of models/cm/karras_diffusion.py and the two
sampler-step nodes), plus `ops.td_loss` wherever it is called: models/DxMI/trainer.py has no autograd node for the TD loss, the
kernel itself returns d loss / d v and `res.backward(gradient=grad)` carries it into the value net.  Forward launches are not
recorded here (tests/forward_census.py).  Public classes of `ops` cannot be wrapped without breaking isinstance / subclassing;
each must be named in CLASSES, so a new one is refused the same way.

PROGRAMS (each one eager iteration, graphs off, so every launch is issued from Python), with the tuning it is recorded under:
    imagenet64   DxMI_Trainer_Cond step on imagenet64_T10, per-GPU batch 16      ops.throughput_tuning() (train_image_large.py)
    cifar10      DxMI_Trainer step on cifar10_T10 + the value net, batch 128     ops.throughput_tuning() (train_cifar10.py)
    edm_dsm_b16  DSM microbatch of models/cm/train_util.TrainLoop, 16 images     default knobs
    edm_dsm_b32  the same at 32 images                                           default knobs
TrainLoop never calls ops.tune_for_throughput() (the only callers are train_image_large.py and train_cifar10.py, which do not
drive TrainLoop), so the DSM step runs under the library's default knobs.
"""
import contextlib
import inspect

import torch

# Launch ops of the backward regions: every one has a row format in signature() and a per-row test in
# test_hip_backward_shapes.py.  linear / pool_act / upsample2x are forward kernels the backward() methods call (recomputed
# pre-activations of the embedding MLPs, the transposes of nearest-x2 and of the 2x2 mean pool); their rows have the forward
# census's format.
OPS = ("conv2d", "_conv2d_wgrad", "stem_conv_wgrad", "linear_bwd", "groupnorm_generic_bwd", "groupnorm_silu_bwd", "attention_bwd",
       "colsum", "colsum_per_image", "pool_act_bwd", "silu_bwd", "dropout", "value_head_bwd", "value_head_pgrad",
       "edm_dsm_loss_bwd", "var_step_bwd", "edm_step_bwd", "td_loss", "linear", "pool_act", "upsample2x")
ALWAYS = ("td_loss",)               # recorded wherever called (see the module docstring)

# Helpers that may be called inside an instrumented region and launch nothing a row could describe (shared by both censuses)
ALLOWED = {
    "conv2d_wgrad": "front of _conv2d_wgrad (which is recorded): returns (dW, db) as the layers want them",
    "pack_conv_weight": "weight re-layout into the MFMA operand order; it does launch (one pack kernel per weight or per "
                        "pack_batch): a copy without arithmetic, compared bit for bit in test_hip_kernels.py; every conv / linear "
                        "row test packs its weight through it, so a wrong pack fails those rows",
    "pack_attn_proj_weight": "re-layout of the attention projection weight (same remark as pack_conv_weight)",
    "attn_block_pack": "re-layout of the attention block's weights (same remark as pack_conv_weight)",
    "bgemm": "the batched GEMMs of attention_bwd's five-GEMM path (FUSED_ATTENTION_BWD off or no fused kernel for the head size): "
             "launched only from inside attention_bwd, whose row judges their result",
    "colsum_f32": "fixed-order reduction of the per-image dgamma / dbeta partials, launched only from inside groupnorm_silu_bwd / "
                  "groupnorm_generic_bwd, whose rows judge dgamma and dbeta",
    "pack_tensor": "allocates (or hands out) the destination buffer of a pack; no launch",
    "fast_parameters": "cached list of a module's parameters; no launch",
    "wgrad_join": "joins the weight-gradient side stream; no launch",
    "dropout_site_seed": "host integer hash; no launch",
    "get_tuning": "host query", "set_tuning": "host knob", "tune_for_throughput": "host knobs",
    "conv_ws_clock_ghz": "host query",
    "conv2d_wgrad_plan": "host query", "groupnorm_generic_bwd_plan": "host query",
    "attention_proj_supported": "host query", "attn_block_supported": "host query",
    "device_check": "host query",
    # optimiser, clip and EMA launches: out of the censuses' scope, compared bit for bit / against fp64 on deliberately
    # awkward sizes by test_hip_train_tail.py (adam_step, radam_step, gradnorm_clip, clip_grad_norm_, gather_rows) and
    # test_hip_edm_dsm.py::test_ema_update_vs_fp64_and_torch (ema_update)
    "adam_step": "optimiser: test_hip_train_tail.py", "radam_step": "optimiser: test_hip_train_tail.py",
    "gradnorm_clip": "clip: test_hip_train_tail.py", "clip_grad_norm_": "clip: test_hip_train_tail.py",
    "ema_update": "EMA: test_hip_edm_dsm.py::test_ema_update_vs_fp64_and_torch",
    "gather_rows": "replay-buffer row copy (no arithmetic): test_hip_train_tail.py compares it with torch indexing bit for bit",
}
# Public classes of ops (not wrapped): context managers and plain records; none launches a kernel a row could describe
CLASSES = ("throughput_tuning", "PackedConvWeight", "pack_batch", "PackPlan", "BlockStats", "OpProfiler", "wgrad_branch", "PackedGConv",
           "ConvDesc")


def public_functions(ops):
    """name -> function for every public function defined in dxmi_hip.ops, plus the private entry point _conv2d_wgrad the
    networks call directly."""
    out = {n: v for n, v in vars(ops).items() if inspect.isfunction(v) and not n.startswith("_") and v.__module__ == ops.__name__}
    out["_conv2d_wgrad"] = ops._conv2d_wgrad
    return out


def unknown_classes(ops):
    return sorted(n for n, v in vars(ops).items()
                  if inspect.isclass(v) and not n.startswith("_") and v.__module__ == ops.__name__ and n not in CLASSES)


def _c(t):
    return 0 if t is None else int(t.shape[-1])


def signature(name, a, kw, fns=None, ops=None):
    """One hashable row per launch: (op, shape and dispatch fields...).  fns: name -> unwrapped ops function, ops: the module
    (both needed for the rows that bind their arguments: the ops of _NEW and the forward kernels)."""
    if name == "conv2d":
        x, pw = a[0], a[1]
        pad = kw.get("pad")
        return ("conv2d", tuple(x.shape), _c(kw.get("in1")), pw.Cout, pw.ksize, pw.transpose_flip, int(kw.get("stride", 1)),
                pw.ksize // 2 if pad is None else int(pad), kw.get("pad_br"), int(kw.get("upsample", False) or 0),
                kw.get("residual") is not None, kw.get("mask_src") is not None, kw.get("bias") is not None,
                int(kw.get("act", 0)), bool(kw.get("out_nchw_f32", False)))
    if name == "_conv2d_wgrad":
        x, dy, k = a[0], a[1], a[2]
        pad = kw.get("pad")
        return ("wgrad", tuple(x.shape), _c(kw.get("in1")), tuple(dy.shape), int(k), k // 2 if pad is None else int(pad),
                int(kw.get("stride", 1)), int(bool(kw.get("upsample", False))), bool(kw.get("out") is not None and kw.get("accumulate")),
                bool(kw.get("with_bias", False)))
    if name == "stem_conv_wgrad":
        return ("stem_wgrad", tuple(a[0].shape), tuple(a[1].shape))
    if name == "linear_bwd":
        need_dx = kw.get("need_dx", True) and a[2] is not None
        return ("linear_bwd", tuple(a[0].shape), tuple(a[1].shape), bool(need_dx))
    if name in ("groupnorm_generic_bwd", "groupnorm_silu_bwd"):
        x = a[0]
        return (name, tuple(x.shape), _c(kw.get("in1")), kw.get("add0") is not None, kw.get("add1") is not None,
                int(kw.get("groups", 32)), bool(kw.get("silu", True)), kw.get("scale_shift") is not None, kw.get("fwd_stats") is not None)
    if name == "attention_bwd":
        qkv, heads = a[0], a[2]
        o = kw.get("o", a[4] if len(a) > 4 else None)
        lse = kw.get("lse", a[5] if len(a) > 5 else None)
        return ("attention_bwd", tuple(qkv.shape), int(heads), o is not None, lse is not None)
    if name == "colsum":
        return ("colsum", tuple(a[0].shape), bool(kw.get("accumulate", False)))
    if name == "colsum_per_image":
        return ("colsum_per_image", tuple(a[0].shape))
    if name == "pool_act_bwd":
        return ("pool_act_bwd", tuple(a[0].shape), bool(a[2]))
    if name in _NEW:
        b = inspect.signature(fns[name]).bind(*a, **kw)
        b.apply_defaults()
        return _NEW[name](b.arguments)
    if name in ("linear", "pool_act", "upsample2x"):
        b = inspect.signature(fns[name]).bind(*a, **kw)
        b.apply_defaults()
        return forward_style_row(ops, name, b.arguments)
    raise KeyError(name)


def _dt(t):
    return str(t.dtype).split(".")[1]


# rows of the ops outside the original ten, from their bound arguments
_NEW = {
    "silu_bwd": lambda p: ("silu_bwd", tuple(p["pre"].shape), _dt(p["pre"]), _dt(p["g"])),
    # seed_on_device: a device int32 seed selects dxmi_dropout_bf16_dev (captured steps), a python int dxmi_dropout_bf16
    "dropout": lambda p: ("dropout", tuple(p["x"].shape), float(p["p"]), torch.is_tensor(p["seed"])),
    "value_head_bwd": lambda p: ("value_head_bwd", tuple(p["feat"].shape)),
    "value_head_pgrad": lambda p: ("value_head_pgrad", tuple(p["s"].shape), p["ow"] is not None),
    "edm_dsm_loss_bwd": lambda p: ("edm_dsm_loss_bwd", tuple(p["x_start"].shape), p["weight_schedule"], bool(p["distillation"]),
                                   p["g_mse"] is not None, p["g_xs"] is not None),
    "var_step_bwd": lambda p: ("var_step_bwd", tuple(p["z"].shape), p["g_next"] is not None, p["g_mean"] is not None,
                               p["g_control"] is not None, p["g_logp"] is not None),
    "edm_step_bwd": lambda p: ("edm_step_bwd", tuple(p["z"].shape), p["g_sample"] is not None, p["g_mean"] is not None),
    "td_loss": lambda p: ("td_loss", int(p["cost"].numel()), p["extra"] is not None),
}

def forward_style_row(ops, name, p):
    """Rows of linear / pool_act / upsample2x, shared with tests/forward_census.py (p: the bound arguments)."""
    if name == "linear":
        x, pw = p["x"], p["pw"]
        P, K = x.shape
        S = int(ops.load().dxmi_linear_splitk_slices(P, K, pw.Cout)) if (p["splitk"] and p["post_act"] == ops.ACT_NONE) else 1
        form = "small" if (P <= 4096 and pw.Cout % 4 == 0) else "tiled"      # mirrors dxmi_linear_fwd (csrc/conv_igemm.hip)
        return ("linear", int(P), int(K), pw.Cout, int(p["pre_act"]), int(p["post_act"]), p["bias"] is not None, form, S)
    if name == "upsample2x":
        return ("upsample2x", tuple(p["x"].shape))
    if name == "pool_act":
        return ("pool_act", tuple(p["x"].shape), bool(p["pool"]), int(p["act"]))
    raise KeyError(name)


class Census:
    """`with Census(ops) as c:` ... c.rows = set of signatures of the backward launches made inside the block, c.unknown = names
    of ops functions called inside an instrumented region that are neither a launch op nor on an allow-list."""
    LAUNCH = OPS

    def __init__(self, ops):
        self.ops, self.rows, self.depth, self.saved, self.unknown = ops, set(), 0, {}, set(unknown_classes(ops))

    def in_region(self, name):
        return self.depth > 0 or name in ALWAYS

    def _wrap(self, name, fn):
        launch = name in self.LAUNCH
        judged = launch or name in ALLOWED

        def w(*a, **kw):
            if self.in_region(name):
                if launch:
                    self.rows.add(signature(name, a, kw, self.orig, self.ops))
                elif not judged:
                    self.unknown.add(name)
            return fn(*a, **kw)
        return w

    def _wrap_bwd(self, fn):
        def b(ctx, *g):
            self.depth += 1
            try:
                return fn(ctx, *g)
            finally:
                self.depth -= 1
        return staticmethod(b)

    @staticmethod
    def region_classes():
        from models.cm import karras_diffusion, unet_train
        from models.DxMI import openai_diffusion, unet_small_train, var_sampler_train
        from models import value_train
        return (unet_train._EDMUNetFn, unet_small_train._UNetFn, value_train._ValueNetFn, karras_diffusion._DSMLossFn,
                var_sampler_train._VarStepFn, openai_diffusion._EdmStepFn)

    def _instrument(self):
        fns = self.orig = public_functions(self.ops)
        for n, fn in fns.items():
            self.saved[(self.ops, n)] = fn
            setattr(self.ops, n, self._wrap(n, fn))
        for cls in self.region_classes():
            self.saved[(cls, "backward")] = cls.__dict__["backward"]
            cls.backward = self._wrap_bwd(cls.__dict__["backward"].__func__)

    def __enter__(self):
        self._instrument()
        return self

    def __exit__(self, *exc):
        for (obj, n), v in self.saved.items():
            setattr(obj, n, v)
        return False


def imagenet64_step(device, B=16):
    """One eager DxMI_Trainer_Cond iteration on the imagenet64_T10 net at per-GPU batch B, set up as the benchmark's
    ImageNet-64 train leg sets it up (random init, zero-initialised layers given weights, fp16 master-weight trainer)."""
    import configs_builtin
    import dxmi_config
    from dxmi_hip.optim import Adam, RAdam
    from models.cm.fp16_util import MixedPrecisionTrainer
    from models.cm.script_util import create_model_and_diffusion
    from models.DxMI.openai_diffusion import OpenAIDiffusion
    from models.DxMI.replay import TransitionRing
    from models.DxMI.trainer import append_buffer, reset_buffer
    cfg = configs_builtin.get("imagenet64_T10")
    torch.manual_seed(0)
    with torch.device(device):
        unet, diffusion = create_model_and_diffusion(**cfg.diffusion)
    with torch.no_grad():
        for p in unet.parameters():
            if float(p.abs().max()) == 0:
                torch.nn.init.normal_(p, std=0.02)
    sampler = OpenAIDiffusion(unet, diffusion, **cfg.sampler)
    unet.to(device)
    v = dxmi_config.instantiate(cfg.value).to(device)
    mp = MixedPrecisionTrainer(model=unet, use_fp16=True, initial_lg_loss_scale=20, special_key="log_betas")
    opt = RAdam([{"params": mp.master_params[1:], "lr": 1e-8}, {"params": mp.master_params[0:1], "lr": 1e-6}])
    opt_v = Adam(v.parameters(), lr=1e-5)
    trainer = dxmi_config.instantiate(cfg.trainer, batchsize=B)
    trainer.set_models(v=v, sampler=sampler, optimizer=opt, optimizer_v=opt_v)
    trainer.use_graphs = sampler.use_graph = False
    res = cfg.diffusion.image_size
    g = torch.Generator(device=device).manual_seed(1)
    ring = TransitionRing(1, trainer.n_timesteps, B, sampler.sample_shape, device, with_y=True, sigma_dims=1)
    data = torch.rand(B, 3, res, res, device=device, generator=g) * 2 - 1
    y = torch.randint(0, 1000, (B,), device=device, generator=g)
    sampler.eval()
    d = sampler.sample(B, device=device, i_class=y, out=ring.next_slot())
    buf = append_buffer(ring, d)
    trainer.update_f_v(data, d, buf, y=y)
    trainer.update_sampler_mixed_precision(buf, mp_trainer=mp)
    reset_buffer(device, ring=ring)
    torch.cuda.synchronize()


def cifar10_step(device, B=128, T=10):
    """One eager DxMI_Trainer iteration of train_cifar10.py (cifar10_T10: DDPM U-Net sampler + IGEBM value net) at batch B."""
    from dxmi_hip.optim import Adam
    from models.DxMI.replay import TransitionRing
    from models.DxMI.trainer import DxMI_Trainer, append_buffer, reset_buffer
    from models.DxMI.unet_small import Model
    from models.DxMI.var_sampler import VARSampler
    from models.modules import IGEBMEncoderV2
    from models.value import TimeIndependentValue
    import configs_builtin
    kw = {k: v for k, v in configs_builtin.CONFIGS["cifar10_T10"]["sampler_net"].items() if k != "_target_"}
    torch.manual_seed(0)
    net = Model(**kw)
    sampler = VARSampler(net, T, [3, 32, 32], trainable_beta="fix_last").to(device).eval()
    sampler.use_graph = False
    v = TimeIndependentValue(IGEBMEncoderV2(in_chan=3, out_chan=1, use_spectral_norm=False, keepdim=False, out_activation="linear",
                                            avg_pool_dim=1, learn_out_scale=True, nh=128)).to(device)
    not_beta = [p for n, p in net.named_parameters() if "log_betas" not in n]
    opt = Adam([{"params": net.log_betas, "lr": 1e-5}, {"params": not_beta, "lr": 1e-7}])
    opt_v = Adam(v.parameters(), lr=1e-5)
    tr = DxMI_Trainer(batchsize=B, tau1=0.1, tau2=0.01, gamma=1, use_sampler_beta=True, time_cost=0, adavelreg=0.99,
                      entropy_in_value=None, velocity_in_value=None, time_cost_sig=True, n_timesteps=T)
    tr.set_models(f=None, v=v, sampler=sampler, optimizer=opt, optimizer_fstar=None, optimizer_v=opt_v)
    tr.use_graphs = False
    ring = TransitionRing(1, T, B, (3, 32, 32), device)
    g = torch.Generator(device=device).manual_seed(2)
    imgs = torch.rand(B, 3, 32, 32, device=device, generator=g) * 2 - 1
    sampler.eval()
    d = sampler.sample(B, device=device, out=ring.next_slot())
    buf = append_buffer(ring, d)
    tr.update_f_v(imgs, d, buf)
    tr.update_sampler(buf, 1)
    reset_buffer(device, ring=ring)
    torch.cuda.synchronize()


EDM_DSM_MODEL = dict(image_size=64, class_cond=True, learn_sigma=False, num_channels=192, num_res_blocks=3, channel_mult="",
                     num_heads=4, num_head_channels=64, num_heads_upsample=-1, attention_resolutions="32,16,8", dropout=0.1,
                     use_checkpoint=False, use_scale_shift_norm=True, resblock_updown=True, use_fp16=True,
                     use_new_attention_order=False, weight_schedule="karras")


def edm_dsm_setup(device, init_zero_layers=True):
    """The full-size (295.9 M parameters) class-conditional ImageNet-64 EDM U-Net in train mode with ResBlock dropout 0.1, its
    KarrasDenoiser and the fp16 master-weight trainer, as models/cm/train_util.TrainLoop builds them."""
    from models.cm.fp16_util import MixedPrecisionTrainer
    from models.cm.script_util import create_model_and_diffusion
    torch.manual_seed(0)
    net, diffusion = create_model_and_diffusion(**EDM_DSM_MODEL)
    if init_zero_layers:
        with torch.no_grad():
            for p in net.parameters():
                if float(p.abs().max()) == 0:
                    torch.nn.init.normal_(p, std=0.02)
    net = net.to(device).train()
    return net, diffusion, MixedPrecisionTrainer(model=net, use_fp16=True)


def edm_dsm_step(device, B):
    """One eager microbatch of DSM training as TrainLoop.forward_backward drives it: LogNormalSampler sigmas and weights,
    diffusion.training_losses, the weighted mean, MixedPrecisionTrainer.backward.  Default knobs (see the module docstring)."""
    from models.cm.resample import LogNormalSampler
    net, diffusion, mp = edm_dsm_setup(device)
    g = torch.Generator(device=device).manual_seed(3)
    x0 = torch.rand(B, 3, 64, 64, device=device, generator=g) * 2 - 1
    y = torch.randint(0, 1000, (B,), device=device, generator=g)
    sig, w = LogNormalSampler().sample(B, device)
    mp.zero_grad()
    losses = diffusion.training_losses(net, x0, sig, model_kwargs={"y": y})
    mp.backward((losses["loss"] * w).mean())
    torch.cuda.synchronize()
    assert torch.isfinite(losses["loss"]).all()
    del net, mp


@contextlib.contextmanager
def _nullctx():
    yield


# program -> (runner(device), tuning)
PROGRAMS = {
    "imagenet64": (lambda d: imagenet64_step(d), "throughput"),
    "cifar10": (lambda d: cifar10_step(d), "throughput"),
    "edm_dsm_b16": (lambda d: edm_dsm_step(d, 16), "default"),
    "edm_dsm_b32": (lambda d: edm_dsm_step(d, 32), "default"),
}


def tuned(ops, tuning):
    return ops.throughput_tuning() if tuning == "throughput" else _nullctx()


def record(ops, which, device="cuda:0"):
    """(rows, unknown) of one eager iteration of PROGRAMS[which], under the tuning the program runs under."""
    run, tuning = PROGRAMS[which]
    with tuned(ops, tuning), Census(ops) as c:
        run(device)
    torch.cuda.empty_cache()
    return c.rows, sorted(c.unknown)
