"""GPU: the indexed draws (dxmi_randn_indexed / dxmi_randint_indexed, csrc/randn_indexed.hip) and the deterministic generators of
models.cm.random_util on the device.

  * bits: the integers of randint over [0, 2^31) are the low 31 bits of the NumPy restatement's words (tests/philox_ref.py, itself
    checked against the Random123 known-answer vectors on the host), exactly; over [0, 2^31 - 1) the modulus involves all 32 bits;
  * normals vs float64 Box-Muller on the same (exact) uniforms: the worst |err| over the 98 304 values of 8 rows of 3 x 64 x 64 was
    measured as NORMAL_ERR_MEASURED = 1.434e-6 on an MI355X (ROCm's logf / sinf / cosf at 1 ulp, the fp32 product 2 pi u, r <= 5.77); the bound is
    twice that, under the ceiling 1e-5.  The worst error of every case is printed;
  * invariance, bit for bit: one batch of 8 = two batches of 4 = the interleave of two ranks; draws and seeds differ; clamped rows repeat;
  * moments over 2^20 values at 5 sigma; the seed was chosen on the restatement so that the float64 values sit inside 3 sigma (1.0,
    0.1, 1.5 and 0.5 sigma for the mean, the variance and the two correlations);
  * end to end: karras_sample with heun + churn, and multistep on a distilled diffusion, 8 images as one batch = two batches of 4."""
import math

import numpy as np
import pytest
import torch

import philox_ref
from test_hip_karras_sample import build, tiny_kw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INDICES = (0, 1, 49_999, (1 << 32) + 5)
NORMAL_ERR_MEASURED = 1.434e-6      # MI355X, ROCm 7.2: the worst of the 8 x 12 288 case below
NORMAL_CEILING = 1e-5
Z_MAX = math.sqrt(-2.0 * math.log(2.0 ** -25))
MOMENT_SEED = 1


def dev_idx(indices):
    return torch.tensor(list(indices), dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("per_sample", [4, 75, 192])
def test_words_exact(per_sample):
    from dxmi_hip import ops
    seed, draw = 0x1234_5678_9abc_def0, 3
    tail = (3, 8, 8) if per_sample == 192 else (per_sample,)
    want = philox_ref.words(INDICES, per_sample, seed, draw).astype(np.int64)
    got = ops.randint_indexed(dev_idx(INDICES), tail, 0, 1 << 31, seed, draw)
    assert got.dtype == torch.int64 and tuple(got.shape) == (4,) + tail
    np.testing.assert_array_equal(got.reshape(4, per_sample).cpu().numpy(), want & 0x7FFFFFFF)
    got = ops.randint_indexed(dev_idx(INDICES), tail, -7, (1 << 31) - 8, seed, draw)          # range 2^31 - 1: every bit counts
    np.testing.assert_array_equal(got.reshape(4, per_sample).cpu().numpy(), want % ((1 << 31) - 1) - 7)
    small = ops.randint_indexed(dev_idx(INDICES), tail, 0, 1000, seed, draw)
    np.testing.assert_array_equal(small.reshape(4, per_sample).cpu().numpy(), want % 1000)


def test_rows_do_not_depend_on_position_or_geometry():
    """A row is a function of its index: the same index at another row, in a batch of another size and length class."""
    from dxmi_hip import ops
    a = ops.randn_indexed(dev_idx([7, 3, 7, 11, 3]), (3, 64, 64), 5, 2)
    assert torch.equal(a[0], a[2]) and torch.equal(a[1], a[4]) and not torch.equal(a[0], a[1])
    b = ops.randn_indexed(dev_idx([3]), (3, 64, 64), 5, 2)
    assert torch.equal(b[0], a[1])
    c = ops.randn_indexed(dev_idx([3]), (75,), 5, 2)          # a shorter row is a prefix: elements depend on (index, element) only
    assert torch.equal(c[0], a[1].reshape(-1)[:75])
    out = torch.full((2, 75), 9.0, device=DEV)
    assert ops.randn_indexed(dev_idx([3, 3]), (75,), 5, 2, out=out) is out and torch.equal(out[0], c[0]) and torch.equal(out[1], c[0])


def test_wrapper_checks():
    from dxmi_hip import DxmiError, ops
    with pytest.raises(DxmiError):
        ops.randn_indexed(dev_idx([0, 1]).int(), (4,), 0, 0)
    with pytest.raises(DxmiError):
        ops.randn_indexed(dev_idx(range(8))[::2], (4,), 0, 0)
    with pytest.raises(DxmiError):
        ops.randn_indexed(dev_idx([0, 1]), (4, 0), 0, 0)
    with pytest.raises(DxmiError):
        ops.randn_indexed(dev_idx([0, 1]), (4,), 0, 0, out=torch.empty(2, 5, device=DEV))
    with pytest.raises(DxmiError):
        ops.randint_indexed(dev_idx([0, 1]), (4,), 0, (1 << 31) + 1, 0, 0)
    with pytest.raises(DxmiError):
        ops.randint_indexed(dev_idx([0, 1]), (4,), 3, 3, 0, 0)


# --------------------------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("indices, per_sample", [(INDICES, 4), (INDICES, 75), (INDICES, 192), (tuple(range(40_000, 40_008)), 12_288)])
def test_normals_vs_float64(indices, per_sample):
    from dxmi_hip import ops
    seed, draw = 42, 1
    got = ops.randn_indexed(dev_idx(indices), (per_sample,), seed, draw)
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    got = got.cpu().numpy().astype(np.float64)
    want = philox_ref.normals64(indices, per_sample, seed, draw)
    err = np.abs(got - want).max()
    print(f"randn_indexed {len(indices)} x {per_sample}: worst |err| vs float64 Box-Muller {err:.3e}, max |z| {np.abs(got).max():.3f}")
    assert np.abs(got).max() <= Z_MAX
    assert err <= NORMAL_CEILING
    assert err <= 2 * NORMAL_ERR_MEASURED


# ------------------------------------------------------------------------------------------------------------ invariance
@pytest.mark.parametrize("cls", ["determ", "determ-indiv"])
@pytest.mark.parametrize("shape", [(3, 8, 8), (75,)])
def test_batch_and_rank_invariance(cls, shape):
    import models.cm.random_util as ru
    kind = {"determ": ru.DeterministicGenerator, "determ-indiv": ru.DeterministicIndividualGenerator}[cls]

    def draws(g, batch):      # what a sampler does per batch: labels, x_T, then one randn_like per step
        y = g.randint(0, 1000, (batch,), device=DEV)
        x = g.randn(batch, *shape, device=DEV)
        return y, x, g.randn_like(x), g.randn_like(x)
    one = draws(ru.get_generator(cls, 8, seed=3), 8)
    assert one[0].dtype == torch.int64 and one[1].dtype == torch.float32 and tuple(one[1].shape) == (8,) + shape
    g = ru.get_generator(cls, 8, seed=3)
    first = draws(g, 4)
    g.set_done_samples(4)
    second = draws(g, 4)
    for a, b, c in zip(one, first, second):
        assert torch.equal(a, torch.cat([b, c]))
    r0, r1 = (draws(kind(8, seed=3, rank=r, world_size=2), 4) for r in (0, 1))
    for a, b, c in zip(one, r0, r1):
        assert torch.equal(a, torch.stack([b, c], dim=1).reshape(a.shape))
    # both classes give one stream; draws differ from each other, seeds differ
    other = draws(ru.get_generator("determ" if cls == "determ-indiv" else "determ-indiv", 8, seed=3), 8)
    assert all(torch.equal(a, b) for a, b in zip(one, other))
    assert not torch.equal(one[1], one[2]) and not torch.equal(one[2], one[3])
    assert not torch.equal(one[1], ru.get_generator(cls, 8, seed=4).randn(8, *shape, device=DEV))
    # the restatement: draw 1 of seed 3 at indices 0..7
    want = philox_ref.normals64(range(8), int(np.prod(shape)), 3, 1)
    assert np.abs(one[1].reshape(8, -1).cpu().numpy() - want).max() <= NORMAL_CEILING


def test_clamped_rows_repeat_the_last_sample():
    import models.cm.random_util as ru
    g = ru.get_generator("determ", 6, seed=0)
    x = g.randn(8, 3, 8, 8, device=DEV)
    y = g.randint(0, 1 << 20, (8, 5), device=DEV)
    assert torch.equal(x[6], x[5]) and torch.equal(x[7], x[5]) and not torch.equal(x[4], x[5])
    assert torch.equal(y[6], y[5]) and torch.equal(y[7], y[5]) and not torch.equal(y[4], y[5])
    h = g.randn(8, 3, 8, 8, dtype=torch.float16, device=DEV)      # other dtypes: the fp32 draw, cast
    g.set_done_samples(0)
    g.randn(8, 3, 8, 8, device=DEV), g.randint(0, 2, (8,), device=DEV)
    assert h.dtype == torch.float16 and torch.equal(h, g.randn(8, 3, 8, 8, device=DEV).half())


# --------------------------------------------------------------------------------------------------------------- moments
def test_moments():
    from dxmi_hip import ops
    rows, per = 256, 4096
    n = rows * per
    z = ops.randn_indexed(dev_idx(range(rows)), (per,), MOMENT_SEED, 0).double()
    mean, var = z.mean().item(), z.var(unbiased=False).item()

    def corr(a, b):
        a, b = a - a.mean(), b - b.mean()
        return ((a * b).sum() / (a.norm() * b.norm())).item()
    c_elem, c_index = corr(z[:, :-1].reshape(-1), z[:, 1:].reshape(-1)), corr(z[:-1].reshape(-1), z[1:].reshape(-1))
    s = math.sqrt(n)
    print(f"randn_indexed moments over 2^20: mean {mean * s:+.2f} sigma, var {(var - 1) / math.sqrt(2 / n):+.2f} sigma, "
          f"adjacent elements {c_elem * s:+.2f} sigma, adjacent indices {c_index * s:+.2f} sigma")
    assert abs(mean) <= 5 / s
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(c_elem) <= 5 / s and abs(c_index) <= 5 / s


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("sampler", ["heun", "multistep"])
def test_karras_sample_is_batch_invariant(sampler):
    from models.cm.karras_diffusion import karras_sample
    from models.cm.random_util import get_generator
    tiny, _ = tiny_kw()
    if sampler == "heun":
        net, diffusion = build(tiny)
        steps, extra = 6, dict(s_churn=3.0)              # gamma > 0 on every step: eps is drawn and used
    else:
        net, diffusion = build(tiny, {"distillation": True})
        steps, extra = 40, dict(ts=(0, 22, 39))
    y = torch.tensor([3, 871, 12, 500, 999, 0, 41, 7], device=DEV)

    def run(gen, rows):
        return karras_sample(diffusion, net, (rows.stop - rows.start, 3, 16, 16), steps, model_kwargs={"y": y[rows]}, device=DEV,
                             sampler=sampler, generator=gen, **extra).clone()
    g = get_generator("determ-indiv", 8, seed=3)
    whole = run(g, slice(0, 8))
    g.set_done_samples(0)
    first = run(g, slice(0, 4))
    g.set_done_samples(4)
    second = run(g, slice(4, 8))
    assert torch.isfinite(whole).all() and whole.abs().max() <= 1 and whole.std() > 0.05
    assert torch.equal(whole, torch.cat([first, second]))
    # the same calls on the implicit device generator: the halves see other noise than the batch of 8 did
    torch.cuda.manual_seed(3)
    whole = run(None, slice(0, 8))
    assert not torch.equal(whole, torch.cat([run(None, slice(0, 4)), run(None, slice(4, 8))]))
