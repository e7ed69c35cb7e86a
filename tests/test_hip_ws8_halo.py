"""conv_ws8_kernel's halo image without stored padding: the zero rows written once per launch, the zero strip
that tap columns outside the map read, and the four interior DMAs per image and chunk.

1. exact: integer inputs and one-hot weights make every output a copy of one shifted input pixel (or the padding's zero);
2. bitwise: an image does not depend on the batch it rides in, a launch repeats itself (raw and fused-GroupNorm output);
3. against torch fp32 on the same bf16 operands, one bf16 rounding of the output (rel-L2 < 4e-3, as tests/test_hip_round2_kernels.py),
   and element by element against fp64 within the derived bound (forward_bounds.conv_checked), the fused GroupNorm output too."""
import math

import pytest
import torch
import torch.nn.functional as F

from forward_bounds import EDGE, conv_checked

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


@pytest.fixture(scope="module", autouse=True)
def kernels_under_test(ops):
    """A handful of images is a small grid: switch off the library's small-grid re-routing for this module (as
    tests/test_hip_round2_kernels.py), so that every case runs conv_ws8_kernel."""
    old = ops.set_tuning("conv_ws_min_tiles", 0), ops.set_tuning("conv_sm_mask", 1)
    yield
    ops.set_tuning("conv_ws_min_tiles", old[0])
    ops.set_tuning("conv_sm_mask", old[1])


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)


def launch(ops, *a, **kw):
    """-> (result of ops.conv2d, kernel id of the launch)"""
    prof = ops.OpProfiler()
    ops.PROFILER = prof
    try:
        y = ops.conv2d(*a, **kw)
    finally:
        ops.PROFILER = None
    torch.cuda.synchronize()
    return y, prof.records[-1][1]


# (N, C0, C1, upsample)
EXACT_CASES = [
    (5, 128, 0, False),          # the last tile holds one image
    (3, 128, 128, False),        # the concat crosses the part boundary
    (6, 128, 0, True),           # nearest x2 upsample 4x4 -> 8x8 in front
    (9, 256, 256, False),        # 16 chunks
]


@pytest.mark.parametrize("N,C0,C1,ups", EXACT_CASES)
def test_padding_exact(ops, N, C0, C1, ups):
    """Output channel t = 3 ky + kx copies tap (ky, kx) of one input channel; the nine channels lie in different 32-channel
    chunks (both halo buffers, several chunks).  Everything is a small integer, exact in bf16 and in the fp32 sums."""
    Cin, H = C0 + C1, 4 if ups else 8
    nchunks = Cin // 32
    n, c, y, x = torch.meshgrid(torch.arange(N), torch.arange(Cin), torch.arange(H), torch.arange(H), indexing="ij")
    xin = (1 + (y * H + x + 13 * n + 5 * c) % 200).float()               # 1 .. 200: never the padding's zero
    w = torch.zeros(64, Cin, 3, 3)
    chan = [((3 * t) % nchunks) * 32 + (7 * t + 3) % 32 for t in range(9)]
    assert len({ch // 32 for ch in chan}) >= min(4, nchunks) and {(ch // 32) & 1 for ch in chan} == {0, 1}
    for t in range(9):
        w[t, chan[t], t // 3, t % 3] = 1.0
    out, kid = launch(ops, nhwc(xin[:, :C0]), ops.pack_conv_weight(w.to(DEV)), in1=nhwc(xin[:, C0:]) if C1 else None, upsample=ups)
    assert kid == 400008, f"expected conv_ws8_kernel, got kernel id {kid}"
    v = F.interpolate(xin, scale_factor=2.0, mode="nearest") if ups else xin
    vp = F.pad(v, (1, 1, 1, 1))
    want = torch.zeros(N, 8, 8, 64)
    for t in range(9):
        want[..., t] = vp[:, chan[t], t // 3:t // 3 + 8, t % 3:t % 3 + 8]
    assert tuple(out.shape) == (N, 8, 8, 64)
    got = out.float().cpu()
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {want.numel()} outputs differ"


@pytest.fixture(scope="module")
def operands7(ops):
    g = torch.Generator().manual_seed(4108)
    N, C = 7, 256
    x = nhwc(torch.randn(N, C, 8, 8, generator=g))
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    return dict(x=x, w=w, pw=ops.pack_conv_weight(w.to(DEV)),
                bias=torch.randn(C, generator=g).to(DEV), vec=torch.randn(N, C, generator=g).to(DEV),
                res=nhwc(torch.randn(N, C, 8, 8, generator=g)),
                gamma=(1 + 0.3 * torch.randn(C, generator=g)).to(DEV), beta=(0.3 * torch.randn(C, generator=g)).to(DEV))


@pytest.mark.parametrize("gn", [False, True])
def test_batch_independent_and_reproducible(ops, operands7, gn):
    """256 -> 256 with bias, residual and a per-image vector; gn: GroupNorm + SiLU of the output written instead of it."""
    o = operands7

    def run(sl, judge=False):
        kw = dict(bias=o["bias"], addvec=o["vec"][sl].contiguous(), residual=o["res"][sl].contiguous())
        if gn:
            kw["fuse_gn"] = (o["gamma"], o["beta"], 32, 1e-6, True, False)
        if judge:       # element by element against fp64: the raw output, or the GroupNorm + SiLU written instead of it
            r, kid = conv_checked(ops, o["x"][sl].contiguous(), o["pw"], o["w"], **kw)
            kid = 400009 if (gn and kid == 400008) else kid      # the id bench.kernel_name gives the <true> form
        else:
            r, kid = launch(ops, o["x"][sl].contiguous(), o["pw"], **kw)
        assert kid == (400009 if gn else 400008), f"expected conv_ws8_kernel, got kernel id {kid}"      # 400009: its <true> form
        if gn:
            assert r[0] is None and r[1] is not None
            return r[1]
        return r

    full = run(slice(0, 7), judge=True)
    assert torch.isfinite(full.float()).all()
    assert torch.equal(full, run(slice(0, 7)))
    for i in range(7):
        assert torch.equal(run(slice(i, i + 1))[0], full[i]), i


@pytest.mark.parametrize("N", [5, 260])
def test_against_fp32(ops, N):
    """N = 260: 260 tiles over 256 workgroups, so four workgroups reach the tile switch and the drain."""
    g = torch.Generator().manual_seed(977 + N)
    C = 256
    x = torch.randn(N, C, 8, 8, generator=g).to(torch.bfloat16).float()
    w = (torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)).to(torch.bfloat16).float()
    b = torch.randn(C, generator=g)
    res = torch.randn(N, C, 8, 8, generator=g).to(torch.bfloat16).float()
    vec = torch.randn(N, C, generator=g)
    ref = F.conv2d(x.to(DEV), w.to(DEV), b.to(DEV), padding=1) + res.to(DEV) + vec.to(DEV)[:, :, None, None]
    y, kid = conv_checked(ops, nhwc(x), ops.pack_conv_weight(w.to(DEV)), w, bias=b.to(DEV), addvec=vec.to(DEV), residual=nhwc(res))
    assert kid == 400008, f"expected conv_ws8_kernel, got kernel id {kid}"
    got, ref = y.float().permute(0, 3, 1, 2).double(), ref.double()
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"N={N}: rel-L2 {rel:.3e}")
    assert rel < 4e-3


def test_edge_bounds_report():
    """Worst |err| / bound per kernel family over the conv / linear edge-case modules that ran before this one in the session
    (forward_bounds.EDGE: test_hip_conv_sweep, test_hip_edm, test_hip_kernels, test_hip_round2 / 3 / 5_kernels and this module);
    every entry was asserted <= 1 where it was measured."""
    rep = EDGE.report()
    print("edge-case bounds:", rep)
    assert all(v <= 1.0 for v in rep.values()), rep
