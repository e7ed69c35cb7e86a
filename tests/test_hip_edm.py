"""EDM / ADM generation path on the GPU, through the C-ABI: kernel-level parity against torch fp32 on the
same bf16-rounded operands, network / sampler parity against (a) golden vectors produced by the reference
and (b) the pinned oracle with the bf16 storage model.

Tolerances: activations and weight operands are bf16 with fp32 accumulation (the reference computes this
torso in fp16), so: per kernel rel-L2 <= 4e-3 (one bf16 rounding of the output); whole shrunken net
<= 1.5e-2 vs the reference's fp32 golden; few-step samples <= 3e-2 of the sample scale.  The kernel-level conv launches are
also judged element by element against fp64 within the derived bound (forward_bounds.conv_checked).
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from forward_bounds import attention_checked, conv_checked, gn_fwd_checked

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TINY_KW = dict(image_size=16, class_cond=True, learn_sigma=False, num_channels=64, num_res_blocks=1, channel_mult="1,2",
               num_heads=4, num_head_channels=64, num_heads_upsample=-1, attention_resolutions="8", dropout=0.0,
               use_checkpoint=False, use_scale_shift_norm=True, resblock_updown=True, use_fp16=False,
               use_new_attention_order=False, weight_schedule="uniform")
PLAIN = dict(class_cond=False, use_scale_shift_norm=False, resblock_updown=False)
IMAGENET64_KW = dict(image_size=64, class_cond=True, learn_sigma=False, num_channels=192, num_res_blocks=3, channel_mult="",
                     num_heads=4, num_head_channels=64, num_heads_upsample=-1, attention_resolutions="32,16,8", dropout=0.0,
                     use_checkpoint=False, use_scale_shift_norm=True, resblock_updown=True, use_fp16=True,
                     use_new_attention_order=False, weight_schedule="uniform")


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)


def nchw(y):
    return y.float().cpu().permute(0, 3, 1, 2)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)


def build(kw, over=None):
    from models.cm.script_util import create_model_and_diffusion
    from oracle.weights import formula_tensor
    kw = dict(kw)
    kw.update(over or {})
    net, diffusion = create_model_and_diffusion(**kw)
    sd = {k: formula_tensor(k, v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    return net.to(DEV).eval(), diffusion, sd


# ------------------------------------------------------------------------------------------ kernels
GN_CASES = [
    # N, C0, C1, H, silu, scale_shift
    (2, 192, 0, 64, True, False),    # 6 channels / group, 64x64 map (two-kernel path)
    (2, 192, 0, 64, True, True),
    (3, 576, 0, 16, True, True),     # 18 / group
    (2, 384, 192, 32, True, False),  # concat, 18 / group straddling the seam
    (2, 768, 576, 8, True, False),   # 42 / group
    (2, 384, 0, 32, False, False),   # attention norm
    (2, 64, 0, 16, True, True),      # 2 / group (shrunken test net)
    (1, 256, 0, 256, True, False),   # lsun 256x256 map: slice too large for the resident kernel
]


@pytest.mark.parametrize("N,C0,C1,H,silu,ss", GN_CASES)
def test_groupnorm_generic(ops, N, C0, C1, H, silu, ss):
    g = torch.Generator().manual_seed(C0 + C1 + H)
    C = C0 + C1
    x = bf(torch.randn(N, C, H, H, generator=g) * 2 + 0.5)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    ref = F.group_norm(x, 32, gamma, beta, 1e-5)
    sst = None
    if ss:
        sst = torch.randn(N, 3 * 2 * C, generator=g) * 0.3     # wider row: exercises ss_ld
        sl = sst[:, 2 * C:4 * C]
        ref = ref * (1 + sl[:, :C, None, None]) + sl[:, C:, None, None]
    if silu:
        ref = F.silu(ref)
    x0 = nhwc(x[:, :C0])
    x1 = nhwc(x[:, C0:]) if C1 else None
    sd = sst.to(DEV)[:, 2 * C:4 * C] if ss else None
    y = gn_fwd_checked(ops, "generic", x0, gamma.to(DEV), beta.to(DEV), in1=x1, eps=1e-5, silu=silu, scale_shift=sd)    # fp64, element by element
    torch.cuda.synchronize()
    assert rel_l2(nchw(y), ref) < 4e-3
    # the dispatcher picks the same result whichever kernel it routes to
    y2 = ops.groupnorm_silu(x0, gamma.to(DEV), beta.to(DEV), in1=x1, eps=1e-5, silu=silu, scale_shift=sd)
    assert rel_l2(nchw(y2), ref) < 4e-3


CONV_CASES = [
    # N, C0, C1, Cout, H, k, stride, ups
    (2, 192, 0, 192, 64, 3, 1, False),
    (2, 384, 192, 192, 32, 3, 1, False),   # Cout % 128 == 64 through the pipelined kernel
    (2, 576, 0, 576, 16, 3, 1, False),
    (2, 768, 576, 576, 8, 3, 1, False),
    (2, 192, 0, 384, 32, 1, 1, False),     # skip_connection 1x1
    (2, 384, 0, 1152, 32, 1, 1, False),    # qkv 1x1
    (2, 192, 0, 192, 32, 3, 1, True),      # ResBlock(up): nearest x2 staged by the conv
    (2, 192, 0, 192, 32, 3, 2, False),     # Downsample conv (stride 2, symmetric pad 1)
]


@pytest.mark.parametrize("N,C0,C1,Cout,H,k,stride,ups", CONV_CASES)
def test_conv_edm_shapes(ops, N, C0, C1, Cout, H, k, stride, ups):
    g = torch.Generator().manual_seed(C0 + C1 + Cout + H + k)
    Cin = C0 + C1
    x = bf(torch.randn(N, Cin, H, H, generator=g))
    w = bf(torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k))
    b = torch.randn(Cout, generator=g)
    xi = F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x
    ref = F.conv2d(xi, w, b, stride=stride, padding=k // 2)
    res = bf(torch.randn(ref.shape, generator=g))
    ref = ref + res
    pw = ops.pack_conv_weight(w.to(DEV))
    y, _ = conv_checked(ops, nhwc(x[:, :C0]), pw, w, in1=nhwc(x[:, C0:]) if C1 else None, bias=b.to(DEV), stride=stride,
                        pad=k // 2, upsample=ups, residual=nhwc(res))
    torch.cuda.synchronize()
    assert nchw(y).shape == ref.shape
    assert rel_l2(nchw(y), ref) < 4e-3


def test_conv_in_192_and_out(ops):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 64, generator=g)
    w = bf(torch.randn(192, 3, 3, 3, generator=g) / math.sqrt(27))
    b = torch.randn(192, generator=g)
    y, _ = conv_checked(ops, x.to(DEV), ops.pack_conv_weight(w.to(DEV), k27=True), w, bias=b.to(DEV))
    assert rel_l2(nchw(y), F.conv2d(bf(x), w, b, padding=1)) < 4e-3
    h = bf(torch.randn(2, 192, 64, 64, generator=g))
    w2 = bf(torch.randn(3, 192, 3, 3, generator=g) / math.sqrt(9 * 192))
    y2, _ = conv_checked(ops, nhwc(h), ops.pack_conv_weight(w2.to(DEV)), w2, bias=b[:3].to(DEV), out_nchw_f32=True)
    assert rel_l2(y2.cpu(), F.conv2d(h, w2, b[:3], padding=1)) < 1e-5


def test_upsample_and_mean_pool(ops):
    g = torch.Generator().manual_seed(6)
    x = bf(torch.randn(3, 192, 16, 16, generator=g))
    up = ops.upsample2x(nhwc(x))
    assert torch.equal(nchw(up), F.interpolate(x, scale_factor=2, mode="nearest"))
    dn = ops.pool_act(nhwc(x), True, ops.ACT_NONE)
    assert rel_l2(nchw(dn), F.avg_pool2d(x, 2, 2)) < 3e-3


def test_attention_multi_head_legacy_layout(ops):
    """QKVAttentionLegacy: channels are (three, head, d); heads of 64 (unet.py:413-441)."""
    g = torch.Generator().manual_seed(8)
    N, heads, D, T = 2, 6, 64, 1024
    C = heads * D
    qkv = bf(torch.randn(N, 3 * C, T, generator=g))
    q, k, v = [z.reshape(N * heads, D, T) for z in qkv.reshape(N, 3, heads, D, T).unbind(1)]
    s = 1 / math.sqrt(math.sqrt(D))
    wgt = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
    ref = torch.einsum("bts,bcs->bct", wgt, v).reshape(N, C, T)
    y = attention_checked(ops, qkv.permute(0, 2, 1).contiguous().to(torch.bfloat16).to(DEV), heads, 1 / math.sqrt(D), "legacy layout")
    assert rel_l2(y.float().cpu().permute(0, 2, 1), ref) < 6e-3


@pytest.mark.parametrize("N,T,heads,amp", [(3, 256, 9, 1.0), (2, 1024, 6, 1.0), (2, 512, 2, 4.0), (1, 1024, 1, 0.05)])
def test_attention64_long_sequences(ops, N, T, heads, amp):
    """attention64_kernel (64-wide heads, T % 256 == 0: the ADM nets' 16x16 / 32x32 blocks, unet.py:413-441): against fp32 softmax
    attention on the same bf16 operands, with logits from flat (amp 0.05) to peaked (amp 4: the running maximum moves and the
    rescale branch runs); bitwise reproducible and independent of the batch an image rides in."""
    g = torch.Generator().manual_seed(31 + T + heads)
    D = 64
    C = heads * D
    qkv = bf(torch.randn(N, T, 3 * C, generator=g) * amp)
    q, k, v = [z.view(N, T, heads, D).transpose(1, 2) for z in qkv.split(C, dim=2)]
    scale = 1 / math.sqrt(D)
    ref = (torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v).transpose(1, 2).reshape(N, T, C)
    x = qkv.to(torch.bfloat16).to(DEV)
    y = attention_checked(ops, x, heads, scale, "attention64")          # fp64, element by element; two launches bitwise equal
    assert rel_l2(y.float().cpu(), ref) < 8e-3, rel_l2(y.float().cpu(), ref)
    i = N - 1
    assert torch.equal(ops.attention(x[i:i + 1].contiguous(), heads, scale)[0], y[i])


def test_edm_precond_and_step_kernels(ops):
    g = torch.Generator().manual_seed(9)
    N, shape = 5, (3, 16, 16)
    x, Fo, z = (torch.randn(N, *shape, generator=g) for _ in range(3))
    sigma = torch.tensor([80.0, 12.3, 1.0, 0.05, 0.002])
    down, up = sigma * 0.6, sigma * 0.3
    sd = 0.5
    c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
    c_out = sigma * sd / (sigma ** 2 + sd ** 2) ** 0.5
    c_in = 1 / (sigma ** 2 + sd ** 2) ** 0.5
    e = lambda s: s[:, None, None, None]
    x_in, t = ops.edm_precond(x.to(DEV), sigma.to(DEV))
    np.testing.assert_allclose(x_in.cpu().numpy(), (e(c_in) * x).numpy(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(t.cpu().numpy(), (250 * torch.log(sigma + 1e-44)).numpy(), rtol=2e-6)
    den = e(c_out) * Fo + e(c_skip) * x
    mu = x + (x - den) / e(sigma) * e(down - sigma)
    smp = mu + z * e(up)
    s2, m2 = ops.edm_step(x.to(DEV), Fo.to(DEV), z.to(DEV), sigma.to(DEV), down.to(DEV), up.to(DEV))
    np.testing.assert_allclose(m2.cpu().numpy(), mu.numpy(), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(s2.cpu().numpy(), smp.numpy(), rtol=1e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------ network
@pytest.mark.parametrize("tag", ["", "_plain"])
def test_unet_forward_vs_reference_and_oracle(golden_dir, tag):
    from oracle import Precision, edm
    net, diffusion, sd = build(TINY_KW, PLAIN if tag else None)
    g = load(golden_dir, f"edm_unet_forward{tag}")
    assert sum(p.numel() for p in net.parameters()) == int(g["n_params"])
    x, t, y = (torch.from_numpy(g[k]) for k in ("x", "t", "y"))
    cc = not tag
    kw = {"y": y.to(DEV)} if cc else {}
    with torch.no_grad():
        out = net(x.to(DEV), t.to(DEV), **kw).cpu()
    assert out.shape == (2, 3, 16, 16) and out.dtype == torch.float32
    cfg = edm.EDMConfig(image_size=16, model_channels=64, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                        **(dict(num_classes=None, use_scale_shift_norm=False, resblock_updown=False) if tag else {}))
    with torch.no_grad():
        ob = edm.unet_forward(sd, cfg, x, t, prec=Precision("bf16"), **({"y": y} if cc else {}))
    r_ref, r_orc = rel_l2(out, g["out"]), rel_l2(out, ob)
    print(f"edm unet{tag}: rel-L2 vs reference fp32 {r_ref:.3e}, vs oracle bf16-model {r_orc:.3e}")
    assert r_ref < 1.5e-2 and r_orc < 1.5e-2


def test_unet_blocks_vs_oracle_trace(golden_dir):
    """Block-by-block: each HIP block output against the oracle's bf16-model trace — errors must stay at the
    bf16 floor through the depth (no block is wrong by more than rounding)."""
    from oracle import Precision, edm
    net, _, sd = build(TINY_KW)
    g = load(golden_dir, "edm_unet_forward")
    x, t, y = (torch.from_numpy(g[k]) for k in ("x", "t", "y"))
    cfg = edm.EDMConfig(image_size=16, model_channels=64, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2))
    th, to = [], []
    with torch.no_grad():
        net.forward_inference(x.to(DEV), t.to(DEV), y.to(DEV), trace=th)
        edm.unet_forward(sd, cfg, x, t, y=y, prec=Precision("bf16"), trace=to)
    to = dict(to)
    assert len(th) == len(to)
    for name, v in th:
        got = v.float().cpu() if v.dim() == 2 else nchw(v)
        r = rel_l2(got, to[name])
        assert r < 1.2e-2, (name, r)


@pytest.mark.parametrize("tag", ["", "_plain"])
def test_sampling_T4_vs_reference(golden_dir, tag):
    from models.DxMI.openai_diffusion import OpenAIDiffusion
    cc = not tag
    net, diffusion, _ = build(TINY_KW, PLAIN if tag else None)
    s = OpenAIDiffusion(net, diffusion, n_timesteps=4, sample_shape=(3, 16, 16), class_cond=cc, num_classes=1000 if cc else 0,
                        trainable_beta="fix_last", stochastic_last=True, rho=4.0)
    net.to(DEV)
    g = load(golden_dir, f"edm_sampling_T4{tag}")
    torch.manual_seed(int(g["seed"]))
    noise = torch.stack([torch.randn(2, 3, 16, 16) for _ in range(5)])
    with torch.no_grad():
        d = s.sample(2, device=DEV, i_class=7 if cc else None, noise=noise)
    ls = torch.stack(d["l_sample"]).cpu()
    assert ls.shape == (5, 2, 3, 16, 16)
    assert torch.equal(ls[0], noise[0] * 80.0)
    for i in range(1, 5):
        assert rel_l2(ls[i], g["l_sample"][i]) < 3e-2, i
    assert rel_l2(torch.stack(d["mean"]).cpu(), g["mean"]) < 3e-2
    np.testing.assert_allclose(torch.stack(d["sigma"]).cpu().numpy(), g["sigma"], rtol=1e-6)
    assert (d["y"] is None) == (not cc)

    g = load(golden_dir, f"edm_sample_step_T4{tag}")
    torch.manual_seed(int(g["seed"]))
    z = torch.randn(2, 3, 16, 16)
    kw = {"y": torch.from_numpy(g["y"]).to(DEV)} if cc else {}
    with torch.no_grad():
        ds = s.sample_step(torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["idx"]), noise=z.to(DEV), **kw)
    assert rel_l2(ds["sample"].cpu(), g["sample"]) < 2e-2 and rel_l2(ds["mean"].cpu(), g["mean"]) < 2e-2
    np.testing.assert_allclose(ds["sigma"].cpu().numpy(), g["sigma"], rtol=1e-6)


@pytest.mark.parametrize("tag,tb", [("fixlast3", "fix_last3"), ("allbeta", True)])
def test_edm_sample_step_learnable_sigma_variants(golden_dir, tag, tb):
    """OpenAIDiffusion(trainable_beta in {'fix_last3', True}) against the reference's step at T = 6 (openai_diffusion.py:76-84),
    log_betas off their initial values."""
    from models.DxMI.openai_diffusion import OpenAIDiffusion
    net, diffusion, _ = build(TINY_KW)
    s = OpenAIDiffusion(net, diffusion, n_timesteps=6, sample_shape=(3, 16, 16), class_cond=True, num_classes=1000, trainable_beta=tb,
                        stochastic_last=True, rho=4.0)
    net.to(DEV)
    g = load(golden_dir, f"edm_sample_step_T6_{tag}")
    with torch.no_grad():
        net.log_betas.copy_(torch.from_numpy(g["log_betas"]))
        ds = s.sample_step(torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["idx"]), noise=torch.from_numpy(g["z"]).to(DEV),
                           y=torch.from_numpy(g["y"]).to(DEV))
    assert rel_l2(ds["sample"].cpu(), g["sample"]) < 2e-2 and rel_l2(ds["mean"].cpu(), g["mean"]) < 2e-2
    np.testing.assert_allclose(ds["sigma"].cpu().numpy(), g["sigma"], rtol=1e-6)


def test_imagenet64_unet_full_size_vs_oracle():
    """configs/imagenet64 network (192 ch, 3 res blocks, (1,2,3,4), attention at 32/16/8, class-cond,
    scale-shift, resblock up/down; 295.9M parameters) at 64x64 against the fp32 oracle on the CPU."""
    from oracle import edm
    net, diffusion, sd = build(IMAGENET64_KW)
    assert sum(p.numel() for p in net.parameters()) == 295_899_267
    g = torch.Generator().manual_seed(64)
    x = torch.randn(2, 3, 64, 64, generator=g)
    sig = torch.tensor([80.0, 0.5])
    y = torch.tensor([1, 999])
    c_in = 1 / (sig ** 2 + 0.25) ** 0.5
    t = 250 * torch.log(sig)
    with torch.no_grad():
        out = net(x.to(DEV) * c_in.to(DEV)[:, None, None, None] * sig.to(DEV)[:, None, None, None], t.to(DEV), y=y.to(DEV)).cpu()
        ref = edm.unet_forward(sd, edm.EDMConfig(), x * (c_in * sig)[:, None, None, None], t, y=y)
    assert torch.isfinite(out).all()
    r = rel_l2(out, ref)
    print(f"imagenet64 unet: rel-L2 vs oracle fp32 {r:.3e}; params {sum(p.numel() for p in net.parameters())}")
    assert r < 2e-2


def test_imagenet64_batch_independence():
    """Size-independent property at a larger batch: each image's output does not depend on its batch mates."""
    net, _, _ = build(IMAGENET64_KW)
    g = torch.Generator().manual_seed(65)
    x = torch.randn(8, 3, 64, 64, generator=g).to(DEV)
    t = torch.linspace(-1500, 1000, 8).to(DEV)
    y = torch.arange(8).to(DEV) * 100
    with torch.no_grad():
        full = net(x, t, y=y)
        part = net(x[2:5].contiguous(), t[2:5].contiguous(), y=y[2:5].contiguous())
    assert rel_l2(part.cpu(), full[2:5].cpu()) < 1e-2


def test_lsun256_unet_full_size():
    """configs/lsun network (256 ch, (1,1,2,2,4,4), attention at 32/16/8, unconditional) at 256x256, batch 2:
    finite, and image 1 of the pair equals the same image run alone (size-independent property; the CPU oracle
    needs ~2 TFLOP per image at this size, so the oracle comparison is made on the imagenet64 net instead)."""
    import configs_builtin
    net, _, _ = build(dict(configs_builtin.CONFIGS["lsun_bedroom_T4"]["diffusion"]), {"distillation": False})
    g = torch.Generator().manual_seed(256)
    x = torch.randn(2, 3, 256, 256, generator=g).to(DEV)
    t = torch.tensor([900.0, -700.0]).to(DEV)
    with torch.no_grad():
        full = net(x, t)
        one = net(x[1:].contiguous(), t[1:].contiguous())
    assert full.shape == (2, 3, 256, 256) and torch.isfinite(full).all()
    assert rel_l2(one.cpu(), full[1:].cpu()) < 1e-2


def test_cli_generate_large(tmp_path):
    """generate_large.py end to end on one GPU from a log dir holding config.yaml + sampler.pth."""
    import subprocess
    import sys
    import dxmi_config
    from models.DxMI.openai_diffusion import OpenAIDiffusion
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusion-by-maxentirl_amd")
    net, diffusion, _ = build(TINY_KW)
    samp = dict(sample_shape=[3, 16, 16], n_timesteps=4, class_cond=True, num_classes=1000, trainable_beta="fix_last",
                stochastic_last=True, rho=4.0)
    OpenAIDiffusion(net, diffusion, **samp)
    logdir = str(tmp_path)
    dxmi_config.save(dxmi_config.Cfg({"diffusion": dict(TINY_KW, distillation=False), "sampler": samp,
                                      "training": {"seed": 42}}), os.path.join(logdir, "config.yaml"))
    torch.save({"state_dict": net.state_dict(), "fid": 0.0, "i_iter": 0}, os.path.join(logdir, "sampler.pth"))
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run([sys.executable, "generate_large.py", "--log_dir", logdir, "--n_sample", "8", "--batchsize", "4",
                        "--skip_fid"], cwd=pkg, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len([f for f in os.listdir(os.path.join(logdir, "generated")) if f.endswith(".png")]) == 8
    r = subprocess.run([sys.executable, "generate_large.py", "--log_dir", logdir, "--n_sample", "8", "--batchsize", "4"],
                       cwd=pkg, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    arr = np.load(os.path.join(logdir, "samples_8.npz"))["arr_0"]
    assert arr.shape == (8, 16, 16, 3) and arr.dtype == np.uint8
    assert "FID needs --fid_extractor" in r.stdout
    # the FID mode proper (round 4): user-supplied extractor + dataset statistics; activations -> all_gather -> statistics on the
    # device (dxmi_fid_stats) -> distance, as the reference's fid() (generate_large.py:57-74).  Checked against the oracle's
    # host statistics of the very samples the run saved.
    import re
    import sys as _sys
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    _sys.path.insert(0, tests_dir)
    from fid_extractor_stub import PatchFeatures
    from oracle import fid as ofid
    rs = np.random.RandomState(3)
    ref_act = (rs.random_sample((200, 16)) * 0.5 + 0.2).astype(np.float32)
    m2, s2 = ofid.activation_statistics(ref_act)
    np.savez(os.path.join(logdir, "VIRTUAL_stub.npz"), mu=m2, sigma=s2)
    env2 = dict(env, PYTHONPATH=tests_dir + os.pathsep + env.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "generate_large.py", "--log_dir", logdir, "--n_sample", "48", "--batchsize", "16",
                        "--fid_extractor", "fid_extractor_stub:PatchFeatures", "--fid_stats", os.path.join(logdir, "VIRTUAL_stub.npz"),
                        "--fid_dims", "16"], cwd=pkg, env=env2, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = float(re.search(r"FID from 48 samples: ([-0-9.e+]+)", r.stdout).group(1))
    saved = torch.from_numpy(np.load(os.path.join(logdir, "samples_48.npz"))["arr_0"]).permute(0, 3, 1, 2)
    act = PatchFeatures()((saved / 255.0).float())[0][:, :, 0, 0].numpy()
    m1, s1 = ofid.activation_statistics(act)
    want = float(ofid.frechet_distance(m1, s1, m2, s2))
    assert abs(got - want) <= 1e-4 * abs(want), (got, want)


# ------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("N,C0,C1,H,silu,ss", [(2, 192, 0, 32, True, True), (2, 384, 192, 16, True, False),
                                                 (2, 64, 0, 16, False, False), (1, 768, 576, 8, True, True)])
def test_groupnorm_generic_bwd(ops, N, C0, C1, H, silu, ss):
    g = torch.Generator().manual_seed(C0 + H)
    C = C0 + C1
    x = bf(torch.randn(N, C, H, H, generator=g) * 1.5 + 0.3).requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.1).requires_grad_(True)
    dy = bf(torch.randn(N, C, H, H, generator=g))
    add = bf(torch.randn(N, C, H, H, generator=g))
    sst = (torch.randn(N, 2 * C, generator=g) * 0.3).requires_grad_(True) if ss else None
    y = F.group_norm(x, 32, gamma, beta, 1e-5)
    if ss:
        y = y * (1 + sst[:, :C, None, None]) + sst[:, C:, None, None]
    if silu:
        y = F.silu(y)
    (y * dy).sum().backward()
    xd = x.detach()
    x0, x1 = nhwc(xd[:, :C0]), (nhwc(xd[:, C0:]) if C1 else None)
    a0, a1 = nhwc(add[:, :C0]), (nhwc(add[:, C0:]) if C1 else None)
    from backward_bounds import gn_bwd_checked
    form = "one-launch" if ops.groupnorm_generic_bwd_plan(N, H * H, C) else "two-launch"
    dx0, dx1, dg, db, dss = gn_bwd_checked(ops, "groupnorm_generic_bwd", form, x0, nhwc(dy), gamma.detach().to(DEV), beta.detach().to(DEV),
                                           in1=x1, add0=a0, add1=a1, eps=1e-5, silu=silu, scale_shift=sst.detach().to(DEV) if ss else None)
    ref_dx = x.grad + add
    got = torch.cat([nchw(dx0)] + ([nchw(dx1)] if C1 else []), 1)
    assert rel_l2(got, ref_dx) < 6e-3
    assert rel_l2(dg.cpu(), gamma.grad) < 2e-3 and rel_l2(db.cpu(), beta.grad) < 2e-3
    if ss:
        assert rel_l2(dss.cpu(), sst.grad) < 2e-3
    # with the forward's statistics kept (dxmi_groupnorm_generic_bwd_saved): bitwise the results of the recomputing form
    saved = []
    ops.groupnorm_generic(x0, gamma.detach().to(DEV), beta.detach().to(DEV), in1=x1, eps=1e-5, silu=silu,
                          scale_shift=sst.detach().to(DEV) if ss else None, saved=saved)
    assert len(saved) == 1
    r2 = ops.groupnorm_generic_bwd(x0, nhwc(dy), gamma.detach().to(DEV), beta.detach().to(DEV), in1=x1, add0=a0, add1=a1, eps=1e-5,
                                   silu=silu, scale_shift=sst.detach().to(DEV) if ss else None, fwd_stats=saved[0])
    for a, b in zip((dx0, dx1, dg, db, dss), r2):
        assert (a is None and b is None) or torch.equal(a, b)


def test_imagenet64_unet_backward_full_size_vs_oracle():
    """Every parameter gradient of the full configs/imagenet64 network (295.9M parameters, 64x64, N = 2) against torch autograd
    through the pinned oracle on the CPU in fp32, with the bound of the shrunken-net test: 2 x the oracle's own bf16-storage-model
    noise floor + 1.5e-2 per parameter tensor.  The only check that the per-launch results are put together into the right
    parameter gradients at full size (concatenated skip sources, emb_layers rows, accumulation across res blocks)."""
    import time
    from oracle import Precision, edm
    t0 = time.perf_counter()
    net, _, sd = build(IMAGENET64_KW)
    g = torch.Generator().manual_seed(18)
    x = torch.randn(2, 3, 64, 64, generator=g)
    t = torch.tensor([700.0, -900.0])
    y = torch.tensor([5, 321])
    w_out = torch.randn(2, 3, 64, 64, generator=g)
    for p in net.parameters():
        p.requires_grad_(True)
    out = net(x.to(DEV), t.to(DEV), y=y.to(DEV))
    assert out.requires_grad
    (out * w_out.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    ref = {}
    for mode in ("fp32", "bf16"):
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        yo = edm.unet_forward(leaves, edm.EDMConfig(), x, t, prec=Precision(mode), y=y)
        (yo * w_out).sum().backward()
        ref[mode] = {k: leaves[k].grad for k in leaves}
        del leaves, yo
    P = dict(net.named_parameters())
    assert len(P) == len(ref["fp32"])
    worst = ("", 0.0)
    for k, p in P.items():
        assert p.grad is not None and p.grad.shape == ref["fp32"][k].shape, k
        r = rel_l2(p.grad.cpu(), ref["fp32"][k])
        fl = rel_l2(ref["bf16"][k], ref["fp32"][k])
        assert r < 2.0 * fl + 1.5e-2, (k, r, fl)
        if r > worst[1]:
            worst = (k, r)
    print(f"imagenet64 unet backward: worst parameter-gradient rel-L2 vs oracle fp32 = {worst[1]:.2e} ({worst[0]}); "
          f"{len(P)} tensors; device part {t_dev:.1f} s, total {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("tag", ["", "_plain"])
def test_unet_backward_vs_oracle(golden_dir, tag):
    """Every parameter gradient of the shrunken ADM U-Net (both variants) against torch autograd through the pinned
    oracle in fp32; the bound is the oracle's own bf16-storage-model noise floor (as for the DDPM U-Net)."""
    from oracle import Precision, edm
    net, _, sd = build(TINY_KW, PLAIN if tag else None)
    cc = not tag
    cfg = edm.EDMConfig(image_size=16, model_channels=64, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                        **(dict(num_classes=None, use_scale_shift_norm=False, resblock_updown=False) if tag else {}))
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, 3, 16, 16, generator=g)
    t = torch.tensor([700.0, -900.0])
    y = torch.tensor([5, 321])
    w_out = torch.randn(2, 3, 16, 16, generator=g)
    for p in net.parameters():
        p.requires_grad_(True)
    out = net(x.to(DEV), t.to(DEV), **({"y": y.to(DEV)} if cc else {}))
    assert out.requires_grad
    (out * w_out.to(DEV)).sum().backward()
    ref = {}
    for mode in ("fp32", "bf16"):
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        yo = edm.unet_forward(leaves, cfg, x, t, prec=Precision(mode), **({"y": y} if cc else {}))
        (yo * w_out).sum().backward()
        ref[mode] = {k: leaves[k].grad for k in leaves}
    P = dict(net.named_parameters())
    worst = ("", 0.0)
    for k, p in P.items():
        assert p.grad is not None and p.grad.shape == ref["fp32"][k].shape, k
        r = rel_l2(p.grad.cpu(), ref["fp32"][k])
        fl = rel_l2(ref["bf16"][k], ref["fp32"][k])
        assert r < 2.0 * fl + 1.5e-2, (k, r, fl)
        if r > worst[1]:
            worst = (k, r)
    print(f"edm unet{tag} backward: worst parameter-gradient rel-L2 vs oracle fp32 = {worst[1]:.2e} ({worst[0]})")
