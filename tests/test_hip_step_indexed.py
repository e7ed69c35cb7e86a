"""GPU: the two DxMI transitions that make their own noise (dxmi_var_step_fwd_indexed / dxmi_edm_step_fwd_indexed,
csrc/step_indexed.hip) against the pair they replace, bit for bit:

    z = ops.randn_indexed(idx, shape, seed, draw);  ops.var_step(x, eps, z, ...)  /  ops.edm_step(x, F, z, ...)

torch.equal on every output.  The pair's kernels (csrc/elementwise.hip) are compiled with contraction on, the new ones with every
fused multiply-add written out: this test is what holds the two forms together.  Rows of 192 (less than one 1024-element trip of a
workgroup), 1024 (one trip), 1028 (one trip and one lane) and 3072 (three trips) elements; the third index has a high counter word;
the draw numbers are the two ends of the 32-bit range; both associations of the VAR update; mean / control / logp present and
absent; the seed and the draw by value and from the control block (whose by-value twins are then wrong on purpose)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3
INDEX = [0, 7, 2 ** 32 + 5]
SEED = 0x0123456789ABCDEF
DRAWS = (0, 2 ** 32 - 1)
SHAPES = {192: (3, 8, 8), 1024: (1, 32, 32), 1028: (1, 4, 257), 3072: (3, 32, 32)}


def inputs(chw):
    g = torch.Generator().manual_seed(chw)
    shape = (N,) + SHAPES[chw]
    x = torch.randn(shape, generator=g).to(DEV)
    net = torch.randn(shape, generator=g).to(DEV)
    idx = torch.tensor(INDEX, dtype=torch.int64, device=DEV)
    return x, net, idx


def control(ctl, draw):
    """The keywords of one launch: by value, or a device block next to by-value arguments that must be ignored."""
    if not ctl:
        return dict(seed=SEED, draw=draw)
    block = torch.tensor([12345, draw, SEED & 0xFFFFFFFF, SEED >> 32], dtype=torch.int64).to(torch.int32).to(DEV)
    return dict(seed=SEED ^ 0x5555, draw=(draw + 1) & 0xFFFFFFFF, ctl=block)


@pytest.mark.parametrize("ctl", [False, True], ids=["by_value", "control_block"])
@pytest.mark.parametrize("chw", sorted(SHAPES))
def test_var_step_indexed_is_the_pair(chw, ctl):
    from dxmi_hip import ops
    x, eps, idx = inputs(chw)
    xm = torch.tensor([1.0152, 1.2071, 1.0007], device=DEV)
    cm = torch.tensor([-0.1318, -0.6544, -0.0112], device=DEV)
    sg = torch.tensor([0.3127, 0.7413, 0.001], device=DEV)
    for draw in DRAWS:
        z = ops.randn_indexed(idx, x.shape[1:], SEED, draw)
        for assoc in (0, 1):
            want = ops.var_step(x, eps, z, xm, cm, sg, assoc=assoc)
            got = ops.var_step_indexed(x, eps, idx, xm, cm, sg, assoc=assoc, **control(ctl, draw))
            for name, w, g_ in zip(("x_next", "mean", "control", "logp"), want, got):
                assert torch.equal(w, g_), f"{name}: CHW={chw} draw={draw} assoc={assoc}: max |diff| {(w - g_).abs().max().item():.3e}"
            assert not torch.equal(want[0], want[1])          # the noise is in x_next
            # optional outputs absent: x_next alone is written, and is the same
            bare = torch.full_like(x, 7.0)
            out = ops.var_step_indexed(x, eps, idx, xm, cm, sg, assoc=assoc, outs=(bare, None, None, None), **control(ctl, draw))
            assert out[0] is bare and out[1] is None and out[2] is None and out[3] is None and torch.equal(bare, want[0])
            # each optional output on its own
            mean, ctrl, logp = torch.empty_like(x), torch.empty_like(x), torch.empty(N, device=DEV)
            ops.var_step_indexed(x, eps, idx, xm, cm, sg, assoc=assoc, outs=(torch.empty_like(x), mean, None, None), **control(ctl, draw))
            ops.var_step_indexed(x, eps, idx, xm, cm, sg, assoc=assoc, outs=(torch.empty_like(x), None, ctrl, None), **control(ctl, draw))
            ops.var_step_indexed(x, eps, idx, xm, cm, sg, assoc=assoc, outs=(torch.empty_like(x), None, None, logp), **control(ctl, draw))
            assert torch.equal(mean, want[1]) and torch.equal(ctrl, want[2]) and torch.equal(logp, want[3])
    # want_mean / want_control of the wrapper
    got = ops.var_step_indexed(x, eps, idx, xm, cm, sg, seed=SEED, draw=0, want_mean=False, want_control=False)
    assert got[1] is None and got[2] is None and got[3] is not None


@pytest.mark.parametrize("ctl", [False, True], ids=["by_value", "control_block"])
@pytest.mark.parametrize("chw", sorted(SHAPES))
def test_edm_step_indexed_is_the_pair(chw, ctl):
    from dxmi_hip import ops
    x, fout, idx = inputs(chw)
    x = x * torch.tensor([80.0, 2.5, 0.3], device=DEV).view(N, 1, 1, 1)
    sigma = torch.tensor([80.0, 2.4431, 0.1072], device=DEV)
    down = torch.tensor([5.3106, 0.2117, 0.0], device=DEV)
    up = torch.tensor([23.417, 0.9562, 0.002], device=DEV)
    for draw in DRAWS:
        z = ops.randn_indexed(idx, x.shape[1:], SEED, draw)
        want = ops.edm_step(x, fout, z, sigma, down, up, 0.5)
        got = ops.edm_step_indexed(x, fout, idx, sigma, down, up, 0.5, **control(ctl, draw))
        for name, w, g_ in zip(("sample", "mean"), want, got):
            assert torch.equal(w, g_), f"{name}: CHW={chw} draw={draw}: max |diff| {(w - g_).abs().max().item():.3e}"
        assert not torch.equal(want[0], want[1])
        outs = (torch.empty_like(x), torch.empty_like(x))
        assert ops.edm_step_indexed(x, fout, idx, sigma, down, up, 0.5, outs=outs, **control(ctl, draw))[0] is outs[0]
        assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])


def test_rows_follow_their_index_not_their_place():
    """The noise of a row is its index's: the same index at another row of another batch gives the same transition."""
    from dxmi_hip import ops
    x, eps, _ = inputs(1028)
    one = torch.tensor([0.9, -0.2, 0.5], device=DEV)
    a = ops.var_step_indexed(x, eps, torch.tensor([5, 9, 5], dtype=torch.int64, device=DEV), one[[0, 0, 0]], one[[1, 1, 1]],
                             one[[2, 2, 2]], seed=3, draw=4, assoc=1)
    b = ops.var_step_indexed(x[2:], eps[2:], torch.tensor([5], dtype=torch.int64, device=DEV), one[:1], one[1:2], one[2:], seed=3,
                             draw=4, assoc=1)
    assert torch.equal(a[0][2], b[0][0]) and torch.equal(a[3][2:], b[3])
    assert not torch.equal(a[0][0] - a[1][0], a[0][1] - a[1][1])          # rows 0 and 1 have different indices: different noise
    z = ops.randn_indexed(torch.tensor([5, 9, 5], dtype=torch.int64, device=DEV), x.shape[1:], 3, 4)
    assert torch.equal(z[0], z[2]) and not torch.equal(z[0], z[1])


def test_wrapper_checks_on_the_device():
    """What tests/test_step_indexed_host.py cannot reach without a device: the checks of sample_index (_indexed_operands)."""
    from dxmi_hip import DxmiError, ops
    x, eps, idx = inputs(192)
    s = torch.ones(N, device=DEV)
    for bad in (idx.int(), idx.cpu(), torch.arange(2 * N, dtype=torch.int64, device=DEV)[::2]):
        with pytest.raises(DxmiError):
            ops.var_step_indexed(x, eps, bad, s, s, s)
        with pytest.raises(DxmiError):
            ops.edm_step_indexed(x, eps, bad, s, s, s)
    with pytest.raises(DxmiError, match="ctl"):
        ops.var_step_indexed(x, eps, idx, s, s, s, ctl=torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(DxmiError, match="ctl"):
        ops.edm_step_indexed(x, eps, idx, s, s, s, ctl=torch.zeros(3, dtype=torch.int32, device=DEV))
