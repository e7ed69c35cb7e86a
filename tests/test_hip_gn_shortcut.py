"""A changing ResnetBlock's norm1 GroupNorm(+SiLU) and nin_shortcut from one read of its input (dxmi_groupnorm_silu_shortcut:
conv1x1_rw_kernel with a GroupNorm side output) against the two launches it replaces, bit for bit: y against ops.groupnorm_silu on
the streaming path, sc against ops.conv2d.  Shapes: the seven such blocks of the CIFAR-10 DDPM U-Net (models/DxMI/unet_small.py
_resblock) at B = 256, and small batches where conv1x1_rw_kernel takes the shape (33 images of 32x32) or does not (7: the op declines)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

UNET_KW = dict(ch=128, out_ch=3, ch_mult=(1, 2, 2, 2), num_res_blocks=2, attn_resolutions=[16], dropout=0.1,
               in_channels=3, resolution=32)

# (H, C0, C1, Cout): down level 1 block 0; up level 1 blocks 0 / 1 and 2; up level 0 block 0 (C = 384 at 12 channels per group:
# group 21 straddles the x0 | x1 boundary) and blocks 1 / 2
SHAPES = [(16, 128, 0, 256), (16, 256, 256, 256), (16, 256, 128, 256), (32, 256, 128, 128), (32, 128, 128, 128)]


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def _case(ops, N, H, C0, C1, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    C = C0 + C1
    x0 = torch.randn(N, H, H, C0, generator=g).to(torch.bfloat16).to(DEV)
    x1 = (torch.randn(N, H, H, C1, generator=g) * 2 + 0.5).to(torch.bfloat16).to(DEV) if C1 else None
    s0, s1 = ops.block_stats(x0), (ops.block_stats(x1) if C1 else None)
    ga, be = (torch.rand(C, generator=g) + 0.5).to(DEV), torch.randn(C, generator=g).to(DEV)
    pw = ops.pack_conv_weight((torch.randn(Cout, C, 1, 1, generator=g) * 0.05).to(DEV))
    b = torch.randn(Cout, generator=g).to(DEV)
    return x0, x1, (s0, s1), ga, be, pw, b


# every shape at B = 256 and 7; 33 images on the 32x32 maps (528 tiles: the pixel streams walk unequal tile counts)
CASES = [(256,) + s for s in SHAPES] + [(33,) + s for s in SHAPES if s[0] == 32] + [(7,) + s for s in SHAPES]


@pytest.mark.parametrize("N,H,C0,C1,Cout", CASES)
def test_gn_shortcut_equals_the_two_ops(ops, N, H, C0, C1, Cout):
    x0, x1, st, ga, be, pw, b = _case(ops, N, H, C0, C1, Cout, seed=N * 31 + C0 + C1 + Cout)
    y_ref = ops.groupnorm_silu(x0, ga, be, in1=x1, eps=1e-6, silu=True, stats=st)
    sc_ref = ops.conv2d(x0, pw, in1=x1, bias=b)
    r = ops.groupnorm_silu_shortcut(x0, ga, be, pw, in1=x1, bias=b, eps=1e-6, silu=True, stats=st)
    # conv1x1_rw_kernel takes >= 512 tiles of 64 pixels: every B = 256 shape and 33 images of 32x32; 7 images: none
    assert (r is not None) == (N * H * H >= 32768), (N, H)
    if r is None:
        return
    y, sc = r
    assert torch.equal(y, y_ref), (N, H, C0, C1, Cout)
    assert torch.equal(sc, sc_ref), (N, H, C0, C1, Cout)
    y2, sc2 = ops.groupnorm_silu_shortcut(x0, ga, be, pw, in1=x1, bias=b, eps=1e-6, silu=True, stats=st)
    assert torch.equal(y2, y) and torch.equal(sc2, sc)                       # bitwise reproducible


def test_gn_shortcut_declines_out_of_scope(ops):
    """No block statistics for x1, or a 3x3 shortcut: the op declines and the caller runs the two ops."""
    x0, x1, st, ga, be, pw, b = _case(ops, 64, 32, 256, 128, 128, seed=5)
    assert ops.groupnorm_silu_shortcut(x0, ga, be, pw, in1=x1, bias=b, stats=(st[0], None)) is None
    pw3 = ops.pack_conv_weight((torch.randn(128, 384, 3, 3) * 0.02).to(DEV))
    assert ops.groupnorm_silu_shortcut(x0, ga, be, pw3, in1=x1, bias=b, stats=st) is None


def _net():
    from models.DxMI.unet_small import Model
    from oracle.weights import formula_tensor
    torch.manual_seed(0)
    net = Model(**UNET_KW)
    net.load_state_dict({k: formula_tensor(k, v.shape) for k, v in net.state_dict().items()})
    return net.to(DEV).eval()


def test_forward_bitwise_with_and_without_the_fused_shortcut():
    """The whole U-Net forward at B = 256 (all seven blocks fused) is bitwise the two-launch forward; an image's output does not
    depend on the batch it rides in (33: the 32x32 blocks fused, the 16x16 ones not; 7: none fused)."""
    net = _net()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(256, 3, 32, 32, generator=g).to(DEV)
    t = (torch.rand(256, generator=g) * 999).to(DEV)
    with torch.no_grad():
        outs = {}
        for on in (True, False):
            net.FUSE_GN_SHORTCUT = on
            outs[on] = net.forward_inference(x, t).clone()
        assert torch.isfinite(outs[True]).all()
        assert torch.equal(outs[True], outs[False])
        net.FUSE_GN_SHORTCUT = True
        assert torch.equal(net.forward_inference(x, t), outs[True])            # reproducible
        for n in (33, 7):
            small = {}
            for on in (True, False):
                net.FUSE_GN_SHORTCUT = on
                small[on] = net.forward_inference(x[:n].contiguous(), t[:n].contiguous()).clone()
            assert torch.equal(small[True], small[False]), n
            assert torch.equal(small[True], outs[True][:n]), n
        net.FUSE_GN_SHORTCUT = True


def test_sampler_graph_matches_eager_with_the_fused_shortcut():
    """The sampler's captured step replays the fused launches (64 images: the 32x32 blocks take them) with the eager results."""
    from models.DxMI.var_sampler import VARSampler
    from oracle.weights import formula_tensor
    from models.DxMI.unet_small import Model
    T, B = 2, 64
    outs = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        net = Model(**UNET_KW)
        s = VARSampler(net, T, [3, 32, 32], trainable_beta="fix_last")
        net.load_state_dict({k: (v if k in ("log_betas", "std") else formula_tensor(k, v.shape)) for k, v in net.state_dict().items()})
        s = s.to(DEV).eval()
        s.use_graph = mode == "graph"
        torch.cuda.manual_seed(5)
        outs[mode] = [s.sample(B, device=DEV)["sample"].clone() for _ in range(3)]
    for i in range(3):
        assert torch.equal(outs["eager"][i], outs["graph"][i]), i
