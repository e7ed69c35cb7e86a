"""Shape census of the backward launches of the training steps (used by test_hip_backward_shapes.py).

`Census` wraps the `ops` entry points that the autograd paths of models/cm/unet_train.py, models/DxMI/unet_small_train.py and
models/value_train.py call, and records a signature for every call made inside one of their backward() methods: operand shapes
plus every flag that takes part in the kernel choice.  Forward launches are not recorded.  `imagenet64_step` and `cifar10_step`
run one eager training iteration of the two training programs (graphs off, so every launch is issued from Python).
"""
import contextlib

import torch

OPS = ("conv2d", "_conv2d_wgrad", "stem_conv_wgrad", "linear_bwd", "groupnorm_generic_bwd", "groupnorm_silu_bwd", "attention_bwd",
       "colsum", "colsum_per_image", "pool_act_bwd")


def _c(t):
    return 0 if t is None else int(t.shape[-1])


def signature(name, a, kw):
    """One hashable row per launch: (op, shape and dispatch fields...)."""
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
    raise KeyError(name)


class Census:
    """`with Census(ops) as c:` ... c.rows = set of signatures of the backward launches made inside the block."""

    def __init__(self, ops):
        self.ops, self.rows, self.depth, self.saved = ops, set(), 0, {}

    def _wrap(self, name, fn):
        def w(*a, **kw):
            if self.depth:
                self.rows.add(signature(name, a, kw))
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

    def __enter__(self):
        from models.cm import unet_train
        from models.DxMI import unet_small_train
        from models import value_train
        for n in OPS:
            self.saved[(self.ops, n)] = getattr(self.ops, n)
            setattr(self.ops, n, self._wrap(n, getattr(self.ops, n)))
        for cls in (unet_train._EDMUNetFn, unet_small_train._UNetFn, value_train._ValueNetFn):
            self.saved[(cls, "backward")] = cls.__dict__["backward"]
            cls.backward = self._wrap_bwd(cls.__dict__["backward"].__func__)
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


@contextlib.contextmanager
def _nullctx():
    yield


def record(ops, which, device="cuda:0"):
    """Signatures of the backward launches of one eager iteration: which = "imagenet64" (under ops.throughput_tuning(), as the
    ImageNet-64 training program runs) or "cifar10" (also under throughput tuning: train_cifar10.py sets it)."""
    with ops.throughput_tuning(), Census(ops) as c:
        if which == "imagenet64":
            imagenet64_step(device)
        else:
            cifar10_step(device)
    return c.rows
