"""GPU: the step tail (csrc/optim.hip, the EMA of csrc/edm_dsm.hip), the indexed draws (csrc/randn_indexed.hip) and the row gather
OFF their fast paths: the paths a real run reaches and the sizes of test_hip_train_tail.py / test_hip_randn_indexed.py do not.

  A  full 4096-element chunks behind a base that is only 4-, 8- or 12-byte aligned (the dword loop of mt_adam_kernel, mt_sqnorm_kernel,
     mt_scale_kernel, ema_kernel), every tensor a view of one flat buffer between sentinel guards; reference: the same call on
     separately allocated (aligned) clones, bit for bit;
  B  130 tensors = launches of 64, 64 and 2 with a learning rate of its own per tensor, by value and from device memory (`hyper=`:
     dxmi_adam_step_dev / dxmi_radam_step_dev); reference: 130 single-tensor by-value calls, bit for bit;
  C  more than 4096 norm partials (the second trip of clip_coef_kernel) and launch series whose chunk counts leave 1, 2, 3 mod SQ_CH;
     reference: exact values, and sqrt(sum g.double()^2) under a bound counted from the kernels' additions;
  D  indexed draws longer than the 64 x 256 lanes of one grid; reference: tests/philox_ref.py;
  E  gather_rows behind 8- and 4-byte aligned bases and over two workgroups per row; reference: src[idx], bit for bit.

"Bit for bit" compares the int32 images of the tensors, so -0.0 / +0.0 and NaN payloads count."""
import functools
import math

import numpy as np
import pytest
import torch

import philox_ref
from test_hip_randn_indexed import NORMAL_ERR_MEASURED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 4096                       # MT_CHUNK / EMA_CHUNK
MT_MAX = 64                        # DXMI_MT_MAX
GUARD = 8
SENTINEL = 0x7FC5A5A5              # a quiet NaN with a payload no kernel here produces
B1, B2, EPS = 0.9, 0.999, 1e-8
EDGE_SIZES = (2 * CHUNK + 5, CHUNK, CHUNK - 1, 1)
U = 2.0 ** -24                     # unit roundoff of fp32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _all_same_bits(xs, ys):
    return len(xs) == len(ys) and all(_same_bits(x, y) for x, y in zip(xs, ys))


class Carved:
    """Contiguous views of one flat fp32 buffer; view i starts `offsets[i]` bytes past a 16-byte boundary, with at least GUARD
    sentinel elements before and after it."""

    def __init__(self, values, offsets):
        assert all(o in (0, 4, 8, 12) for o in offsets) and len(values) == len(offsets)
        starts, pos = [], 0
        for v, o in zip(values, offsets):
            pos += GUARD
            pos += (o // 4 - pos) % 4
            starts.append(pos)
            pos += v.numel()
        self.flat = torch.empty(pos + GUARD, dtype=torch.float32, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        _bits(self.flat).fill_(SENTINEL)
        self.guard = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        self.views = []
        for v, s, o in zip(values, starts, offsets):
            view = self.flat[s:s + v.numel()].view(v.shape)
            view.copy_(v)
            assert view.is_contiguous() and view.data_ptr() % 16 == o
            self.guard[s:s + v.numel()] = False
            self.views.append(view)
        assert all(int(self.guard[s - GUARD:s].sum()) == GUARD and int(self.guard[s + v.numel():s + v.numel() + GUARD].sum()) == GUARD
                   for v, s in zip(values, starts))

    def guards_intact(self):
        return bool((_bits(self.flat)[self.guard] == SENTINEL).all())


def _edge_offsets(misaligned):
    """Every size at every misalignment (4, 8, 12 bytes), or the same layout on 16-byte boundaries."""
    return [o if misaligned else 0 for _ in EDGE_SIZES for o in (4, 8, 12)]


def _edge_values(seed, positive=False, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in EDGE_SIZES:
        for _ in range(3):
            x = torch.randn(n, generator=g) * scale
            out.append((x.square() if positive else x).to(DEV))
    return out


def _edge_streams(seed, grad_scale=1.0):
    """p, g, m, v of the edge list; gradients are pre-multiplied by 1 / grad_scale as a loss-scaled backward leaves them."""
    return (_edge_values(seed), _edge_values(seed + 1, scale=1.0 / grad_scale), _edge_values(seed + 2, scale=0.1),
            _edge_values(seed + 3, positive=True, scale=0.1))


def _clones(ts):
    out = [t.clone() for t in ts]
    assert all(t.data_ptr() % 16 == 0 for t in out)
    return out


# ------------------------------------------------------------------------------------------------------ A: misaligned bases
MISALIGNED = {"all": "pgmv", "only_p": "p", "only_g": "g", "only_m": "m", "only_v": "v"}


def _carve_streams(streams, which):
    return [Carved(vals, _edge_offsets(name in which)) for name, vals in zip("pgmv", streams)]


@pytest.mark.parametrize("which", list(MISALIGNED))
def test_adam_full_chunks_behind_misaligned_bases(which):
    """mt_adam_kernel<0>: the 16-byte path needs p, g, m AND v aligned; one misaligned stream sends whole chunks through the dword
    loop.  With and without grad_scale, gradients written back exactly when asked."""
    from dxmi_hip import ops
    t = 3
    steps = [-(1e-3 * (1 + i / 5) / (1 - B1 ** t)) for i in range(3 * len(EDGE_SIZES))]
    bc2_sqrt = (1 - B2 ** t) ** 0.5
    for scale, write_back in ((None, False), (None, True), (0.375, False), (0.375, True)):
        streams = _edge_streams(10, grad_scale=scale or 1.0)
        gs = None if scale is None else torch.full((1,), scale, device=DEV)
        ref = [_clones(s) for s in streams]
        ops.adam_step(*ref, steps, B1, B2, EPS, bc2_sqrt, grad_scale=gs, write_back_grad=write_back)
        carved = _carve_streams(streams, MISALIGNED[which])
        ops.adam_step(*[c.views for c in carved], steps, B1, B2, EPS, bc2_sqrt, grad_scale=gs, write_back_grad=write_back)
        case = (which, scale, write_back)
        for name, c, r, before in zip("pgmv", carved, ref, streams):
            assert _all_same_bits(c.views, r), (case, name)
            assert c.guards_intact(), (case, name)
            if name != "g":
                assert not any(_same_bits(x, y) for x, y in zip(c.views, before)), (case, name)      # the step did run
        want_g = [g * gs for g in streams[1]] if (scale is not None and write_back) else streams[1]
        assert _all_same_bits(carved[1].views, want_g), case


@pytest.mark.parametrize("which", list(MISALIGNED))
@pytest.mark.parametrize("t", [2, 10])
def test_radam_full_chunks_behind_misaligned_bases(which, t):
    """mt_adam_kernel<1>: the un-rectified branch (rect < 0 at t = 2) and a rectified step (t = 10, RAdam.radam_scalars)."""
    from dxmi_hip import ops
    from dxmi_hip.optim import RAdam
    _, bc2_sqrt, rect = RAdam.radam_scalars(B1, B2, t)
    assert (rect < 0) == (t == 2)
    lrs = [1e-3 * (1 + i / 5) for i in range(3 * len(EDGE_SIZES))]
    gs = torch.full((1,), 0.375, device=DEV)
    for scale in (None, gs):
        streams = _edge_streams(20)
        ref = [_clones(s) for s in streams]
        ops.radam_step(*ref, lrs, B1, B2, EPS, 1 - B1 ** t, bc2_sqrt, rect, grad_scale=scale)
        carved = _carve_streams(streams, MISALIGNED[which])
        ops.radam_step(*[c.views for c in carved], lrs, B1, B2, EPS, 1 - B1 ** t, bc2_sqrt, rect, grad_scale=scale)
        for name, c, r in zip("pgmv", carved, ref):
            assert _all_same_bits(c.views, r), (which, t, name)
            assert c.guards_intact(), (which, t, name)
        assert _all_same_bits(carved[1].views, streams[1])                  # RAdam never writes gradients back
        assert not any(_same_bits(x, y) for x, y in zip(carved[0].views, streams[0]))


# The norm of the edge list: longest chain of fp32 additions a term g^2 passes through, in the kernels as written.
#   mt_sqnorm_kernel, dword loop (every chunk of a misaligned tensor, every tail): `acc += G[i] * G[i]` for i = tid, tid + 256, ...
#       -> MT_CHUNK / MT_BLOCK = 16 adds;  16-byte path: ((g0^2 + g1^2) + g2^2) + g3^2 = 3 adds, then `acc +=` over R = 4 trips -> 7
#   wave_sum: 6 shuffle-adds;  block: (red0 + red1) + (red2 + red3) = 2
#   clip_coef_kernel with n <= 256 partials: one `acc += v[u]` per lane, wave_sum 6, (red0 + red1) + (red2 + red3) 2
# d = 16 + 6 + 2 + 1 + 6 + 2 = 33, and one rounding for the square itself: |sum' - sum| <= ((1 + u)^(d + 1) - 1) sum for non-negative terms
# (~ (d + 1) 2^-24); the root halves it and adds its own rounding.
def _norm_bound(d):
    return math.sqrt((1 + U) ** (d + 1)) * (1 + U) - 1


EDGE_NORM_DEPTH = 16 + 6 + 2 + 1 + 6 + 2


@pytest.mark.parametrize("misaligned", [True, False])
def test_gradnorm_clip_full_chunks_behind_misaligned_bases(misaligned):
    """mt_sqnorm_kernel and mt_scale_kernel on their dword loops: norm vs fp64 on the device under the counted bound, every gradient
    scaled to fp32(g * coef) with the coefficient the call reports, guards untouched."""
    from dxmi_hip import ops
    grads = _edge_values(30)
    carved = Carved(grads, _edge_offsets(misaligned))
    ref = math.sqrt(sum(float(g.double().square().sum()) for g in grads))
    max_norm = 0.1
    out = ops.gradnorm_clip(carved.views, max_norm)
    torch.cuda.synchronize()
    rel = abs(out[0].item() - ref) / ref
    print(f"gradnorm_clip edge list (misaligned={misaligned}): rel err {rel:.3e}, bound {_norm_bound(EDGE_NORM_DEPTH):.3e}")
    assert rel <= _norm_bound(EDGE_NORM_DEPTH) and rel <= 2e-6
    assert out[2].item() == 0.0
    coef = out[1:2].clone()
    want_coef = np.float32(max_norm) / (np.float32(out[0].item()) + np.float32(1e-6))
    assert 0 < coef.item() < 1e-2 and np.float32(coef.item()) == want_coef
    assert _all_same_bits(carved.views, [g * coef for g in grads])
    assert carved.guards_intact()


EMA_RATES = (0.999, 0.9999, 0.99, 0.5)
EMA_CASES = {"K1": (1, "s0"), "K2": (2, "s01"), "K3": (3, "s012"), "K4": (4, "s0123"), "K3_one_target": (3, "1"), "K3_source_only": (3, "s")}


@pytest.mark.parametrize("case", list(EMA_CASES))
def test_ema_full_chunks_behind_misaligned_bases(case):
    """ema_kernel<K>: the 16-byte path needs the source and all K targets aligned."""
    from dxmi_hip import ops
    K, which = EMA_CASES[case]
    src = _edge_values(40)
    targets = [_edge_values(41 + k) for k in range(K)]
    ref = [_clones(t) for t in targets]
    ops.ema_update(ref, _clones(src), EMA_RATES[:K])
    c_src = Carved(src, _edge_offsets("s" in which))
    c_tgt = [Carved(t, _edge_offsets(str(k) in which)) for k, t in enumerate(targets)]
    ops.ema_update([c.views for c in c_tgt], c_src.views, EMA_RATES[:K])
    for k in range(K):
        assert _all_same_bits(c_tgt[k].views, ref[k]), (case, k)
        assert not any(_same_bits(x, y) for x, y in zip(c_tgt[k].views, targets[k])), (case, k)
        assert c_tgt[k].guards_intact(), (case, k)
    assert _all_same_bits(c_src.views, src) and c_src.guards_intact()
    # an overflow step leaves every target as it is
    ops.ema_update([c.views for c in c_tgt], c_src.views, EMA_RATES[:K], found_inf=torch.ones(1, device=DEV))
    assert all(_all_same_bits(c_tgt[k].views, ref[k]) for k in range(K))


# --------------------------------------------------------------------------------------- B: per-tensor scalars across launches
N_LIST = 2 * MT_MAX + 2                                            # launches of 64, 64 and 2
LIST_SIZES = [CHUNK + 1 if i == 100 else 17 + i for i in range(N_LIST)]      # two chunks inside the second launch
LIST_LRS = [1e-3 * (1 + i / 7) for i in range(N_LIST)]


def _list_streams(seed, grad_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda n, s: torch.randn(n, generator=g) * s
    return ([rnd(n, 1.0).to(DEV) for n in LIST_SIZES], [rnd(n, 1.0 / grad_scale).to(DEV) for n in LIST_SIZES],
            [rnd(n, 0.1).to(DEV) for n in LIST_SIZES], [rnd(n, 0.1).square().to(DEV) for n in LIST_SIZES])


def _one_by_one(step, streams, scalars):
    """The reference of B: one single-tensor by-value call per tensor."""
    ref = [_clones(s) for s in streams]
    for i in range(N_LIST):
        step([ref[0][i]], [ref[1][i]], [ref[2][i]], [ref[3][i]], [scalars[i]])
    return ref


def _assert_streams(got, want, what):
    for name, a, b in zip("pgmv", got, want):
        bad = [i for i, (x, y) in enumerate(zip(a, b)) if not _same_bits(x, y)]
        assert not bad, (what, name, bad[:8])


@pytest.mark.parametrize("scale", [None, 0.375])
def test_adam_per_tensor_step_sizes_across_launches(scale):
    """dxmi_adam_step and dxmi_adam_step_dev: tensor i of launch L takes step size number 64 L + i."""
    from dxmi_hip import ops
    t = 3
    steps = [-(lr / (1 - B1 ** t)) for lr in LIST_LRS]
    bc2_sqrt = (1 - B2 ** t) ** 0.5
    gs = None if scale is None else torch.full((1,), scale, device=DEV)
    kw = dict(grad_scale=gs, write_back_grad=scale is not None)
    streams = _list_streams(50, grad_scale=scale or 1.0)
    ref = _one_by_one(lambda p, g, m, v, s: ops.adam_step(p, g, m, v, s, B1, B2, EPS, bc2_sqrt, **kw), streams, steps)
    assert not any(_same_bits(x, y) for x, y in zip(ref[0], streams[0]))
    by_value = [_clones(s) for s in streams]
    ops.adam_step(*by_value, steps, B1, B2, EPS, bc2_sqrt, **kw)
    _assert_streams(by_value, ref, "by value")
    hyper = torch.tensor([bc2_sqrt] + steps, dtype=torch.float32, device=DEV)
    dev = [_clones(s) for s in streams]
    ops.adam_step(*dev, None, B1, B2, EPS, None, hyper=hyper, **kw)
    _assert_streams(dev, ref, "hyper=")
    assert _all_same_bits(dev[1], [g * gs for g in streams[1]] if scale is not None else streams[1])


@pytest.mark.parametrize("t", [2, 10])
def test_radam_per_tensor_lrs_across_launches(t):
    """dxmi_radam_step and dxmi_radam_step_dev: rect < 0 (t = 2) and a rectified step (t = 10) read from device memory; found_inf
    and grad_scale on the _dev entry."""
    from dxmi_hip import ops
    from dxmi_hip.optim import RAdam
    inv_bc1, bc2_sqrt, rect = RAdam.radam_scalars(B1, B2, t)
    assert (rect < 0) == (t == 2) and inv_bc1 == 1.0 / (1 - B1 ** t)
    bc1 = 1 - B1 ** t
    streams = _list_streams(60)
    ref = _one_by_one(lambda p, g, m, v, lr: ops.radam_step(p, g, m, v, lr, B1, B2, EPS, bc1, bc2_sqrt, rect), streams, LIST_LRS)
    assert not any(_same_bits(x, y) for x, y in zip(ref[0], streams[0]))
    by_value = [_clones(s) for s in streams]
    ops.radam_step(*by_value, LIST_LRS, B1, B2, EPS, bc1, bc2_sqrt, rect)
    _assert_streams(by_value, ref, "by value")
    hyper = torch.tensor([inv_bc1, bc2_sqrt, rect] + LIST_LRS, dtype=torch.float32, device=DEV)
    assert hyper[2].item() == (-1.0 if t == 2 else np.float32(rect))
    dev = [_clones(s) for s in streams]
    ops.radam_step(*dev, None, B1, B2, EPS, None, None, None, hyper=hyper)
    _assert_streams(dev, ref, "hyper=")
    # found_inf = 1: nothing changes, in any launch of the series
    skipped = [_clones(s) for s in streams]
    ops.radam_step(*skipped, None, B1, B2, EPS, None, None, None, hyper=hyper, found_inf=torch.ones(1, device=DEV),
                   grad_scale=torch.full((1,), 0.375, device=DEV))
    _assert_streams(skipped, streams, "found_inf = 1")
    # found_inf = 0 and a grad_scale: the by-value call with the same scale
    gs, zero = torch.full((1,), 0.375, device=DEV), torch.zeros(1, device=DEV)
    scaled_ref = [_clones(s) for s in streams]
    ops.radam_step(*scaled_ref, LIST_LRS, B1, B2, EPS, bc1, bc2_sqrt, rect, grad_scale=gs)
    assert not any(_same_bits(x, y) for x, y in zip(scaled_ref[0], ref[0]))
    scaled = [_clones(s) for s in streams]
    ops.radam_step(*scaled, None, B1, B2, EPS, None, None, None, hyper=hyper, found_inf=zero, grad_scale=gs)
    _assert_streams(scaled, scaled_ref, "found_inf = 0, grad_scale")


def test_fused_adam_two_groups_split_inside_the_second_launch():
    """dxmi_hip.optim.Adam vs torch.optim.Adam over 130 tensors, the lr changing at tensor 70 (inside the second launch of 64):
    parameters and both moments bit-identical over 3 steps."""
    from dxmi_hip.optim import Adam
    base = _list_streams(70)[0]
    a = [p.clone().requires_grad_(True) for p in base]
    b = [p.clone().requires_grad_(True) for p in base]
    mk = lambda ps: [{"params": ps[:70], "lr": 1e-3}, {"params": ps[70:], "lr": 3e-4}]
    ref, new = torch.optim.Adam(mk(a)), Adam(mk(b))
    for step in range(3):
        g = torch.Generator().manual_seed(700 + step)
        for x, y in zip(a, b):
            x.grad = (torch.randn(x.shape, generator=g) * 10.0 ** (-step)).to(DEV)
            y.grad = x.grad.clone()
        ref.step()
        new.step()
        bad = [i for i, (x, y) in enumerate(zip(a, b)) if not _same_bits(x.detach(), y.detach())]
        assert not bad, (step, bad[:8])
        for x, y in zip(a, b):
            assert _same_bits(ref.state[x]["exp_avg"], new.state[y]["exp_avg"])
            assert _same_bits(ref.state[x]["exp_avg_sq"], new.state[y]["exp_avg_sq"])


# -------------------------------------------------------------------------------------------------------- C: norm partials
def test_gradnorm_partials_beyond_one_trip_are_each_read_once():
    """4101 partials: clip_coef_kernel's loop takes a second trip for partials 4096 .. 4100.  One element of 3.0 in an all-zero
    gradient must give exactly 3.0 wherever its chunk lies (a dropped partial gives 0, one read twice sqrt(18)); an inf must flag."""
    from dxmi_hip import ops
    n = 4100 * CHUNK + 3
    g = torch.zeros(n, device=DEV)
    spots = [c * CHUNK + (c * 37) % CHUNK for c in (0, 255, 256, 4095, 4096, 4099)] + [4100 * CHUNK + 1]
    assert spots[-1] < n
    for spot in spots:
        g[spot] = 3.0
        out = ops.gradnorm_clip([g], 0.0).cpu()
        assert out[0].item() == 3.0 and out[1].item() == 1.0 and out[2].item() == 0.0, (spot, out.tolist())
        g[spot] = float("inf")
        out = ops.gradnorm_clip([g], 0.0).cpu()
        assert out[2].item() == 1.0 and math.isinf(out[0].item()), (spot, out.tolist())
        g[spot] = 0.0
    # every partial at once: 4101 chunks of one 3.0 each -> sqrt(9 * 4101) up to the additions of the final reduction (17 + 6 + 2)
    idx = torch.arange(4101, device=DEV) * CHUNK
    g[idx] = 3.0
    out = ops.gradnorm_clip([g], 0.0).cpu()
    want = math.sqrt(9.0 * 4101)
    assert abs(out[0].item() - want) <= _norm_bound(17 + 6 + 2) * want, out.tolist()


# Launch series: every tensor is separately allocated (aligned), so full chunks take the 16-byte path (3 + 4 = 7 adds per lane) and
# the tails, all shorter than 256 elements, one add per lane; wave_sum 6, block 2; the list has fewer than 256 partials, so
# clip_coef_kernel adds one per lane, then wave_sum 6 and the tree 2.  d = 7 + 6 + 2 + 1 + 6 + 2 = 24.
SERIES_NORM_DEPTH = 7 + 6 + 2 + 1 + 6 + 2


def _series_sizes(residues):
    """130 tensors whose three launches hold chunk counts = residues (mod SQ_CH = 4): the first tensor of a launch carries the extra
    full chunks."""
    sizes, counts = [], []
    for launch, r in enumerate(residues):
        n_t = min(MT_MAX, N_LIST - launch * MT_MAX)
        extra = (r - n_t) % 4
        launch_sizes = [extra * CHUNK + 17 + launch] + [18 + launch * MT_MAX + i for i in range(1, n_t)]
        sizes += launch_sizes
        counts.append(sum((s + CHUNK - 1) // CHUNK for s in launch_sizes))
    assert len(sizes) == N_LIST and tuple(c % 4 for c in counts) == tuple(residues), counts
    return sizes


@pytest.mark.parametrize("residues", [(1, 2, 3), (2, 3, 1), (3, 1, 2)])
def test_gradnorm_launch_series_partial_offsets_and_scaling(residues):
    """mt_sqnorm_kernel writes partials[part_offset + bid] with SQ_CH chunks per workgroup: a launch that ends inside a workgroup
    (1, 2, 3 chunks in the last one), followed by the next launch's partials.  The workspace is first filled with the partials of
    a list of 100.0s, so a partial that is not written, or written to another launch's slot, cannot go unnoticed."""
    from dxmi_hip import ops
    sizes = _series_sizes(residues)
    gen = torch.Generator().manual_seed(80 + residues[0])
    grads = [(torch.randn(n, generator=gen) * (0.5 + (i % 5))).to(DEV) for i, n in enumerate(sizes)]
    assert all(g.data_ptr() % 16 == 0 for g in grads)
    ref = math.sqrt(sum(float(g.double().square().sum()) for g in grads))
    ops.gradnorm_clip([torch.full_like(g, 100.0) for g in grads], 0.0)
    out = ops.gradnorm_clip([g.clone() for g in grads], 0.0).cpu()
    rel = abs(out[0].item() - ref) / ref
    print(f"gradnorm_clip series {residues}: rel err {rel:.3e}, bound {_norm_bound(SERIES_NORM_DEPTH):.3e}")
    assert rel <= _norm_bound(SERIES_NORM_DEPTH) and rel <= 2e-6
    assert out[1].item() == 1.0 and out[2].item() == 0.0
    # a clipping max_norm scales every tensor of all three launches, by the coefficient the call reports
    work = [g.clone() for g in grads]
    out2 = ops.gradnorm_clip(work, 0.1)
    assert out2[0].item() == out[0].item()
    coef = out2[1:2].clone()
    assert 0 < coef.item() < 1e-2
    bad = [i for i, (w, g) in enumerate(zip(work, grads)) if not _same_bits(w, g * coef)]
    assert not bad, bad[:8]
    # an inf in the last tensor of the last launch is seen
    work[-1][-1] = float("inf")
    assert ops.gradnorm_clip(work, 0.0)[2].item() == 1.0


# --------------------------------------------------------------------------------------- D: indexed draws beyond one grid
LONG_INDICES = (3, (1 << 32) + 5)
LONG_SEED, LONG_DRAW = 0x1234_5678_9abc_def0, 3
INT_SENTINEL = -0x0123_4567_89AB_CDEF


@functools.lru_cache(maxsize=None)
def _ref_words(per_sample):
    w = philox_ref.words(LONG_INDICES, per_sample, LONG_SEED, LONG_DRAW).astype(np.int64)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _ref_normals(per_sample):
    z = philox_ref.normals64(LONG_INDICES, per_sample, LONG_SEED, LONG_DRAW)
    z.setflags(write=False)
    return z


def _dev_idx(indices):
    return torch.tensor(list(indices), dtype=torch.int64, device=DEV)


# 196 608 = an LSUN-256 row (three trips of the 64 x 256-lane grid); 65 536 + 4: one block in the second trip; 65 536 + 7: the same with
# rows that are only 4-byte (fp32) / 8-byte (int64) aligned and a 3-element tail
@pytest.mark.parametrize("per_sample", [196_608, 65_536 + 4, 65_536 + 7])
def test_indexed_draws_beyond_one_grid(per_sample):
    from dxmi_hip import ops
    N, idx = len(LONG_INDICES), _dev_idx(LONG_INDICES)
    ibuf = torch.full((N * per_sample + 16,), INT_SENTINEL, dtype=torch.int64, device=DEV)
    iout = ibuf[:N * per_sample].view(N, per_sample)
    assert ops.randint_indexed(idx, (per_sample,), 0, 1 << 31, LONG_SEED, LONG_DRAW, out=iout) is iout
    np.testing.assert_array_equal(iout.cpu().numpy(), _ref_words(per_sample) & 0x7FFFFFFF)
    assert bool((ibuf[N * per_sample:] == INT_SENTINEL).all())

    fbuf = torch.empty(N * per_sample + 16, dtype=torch.float32, device=DEV)
    _bits(fbuf).fill_(SENTINEL)
    fout = fbuf[:N * per_sample].view(N, per_sample)
    assert ops.randn_indexed(idx, (per_sample,), LONG_SEED, LONG_DRAW, out=fout) is fout
    assert bool((_bits(fbuf)[N * per_sample:] == SENTINEL).all())
    assert not bool((_bits(fout) == SENTINEL).any())                      # every element was written
    err = np.abs(fout.cpu().numpy().astype(np.float64) - _ref_normals(per_sample)).max()
    print(f"randn_indexed {N} x {per_sample}: worst |err| vs float64 Box-Muller {err:.3e}")
    assert err <= 2 * NORMAL_ERR_MEASURED
    # the rows the suite already pins are prefixes of the long ones, bit for bit
    for short in (75, 12_288):
        z = ops.randn_indexed(idx, (short,), LONG_SEED, LONG_DRAW)
        assert _same_bits(z, fout[:, :short]), short
        k = ops.randint_indexed(idx, (short,), 0, 1 << 31, LONG_SEED, LONG_DRAW)
        assert torch.equal(k, iout[:, :short]), short


# ------------------------------------------------------------------------------------------------------------ E: gather_rows
GATHER_IDX = [5, 0, 39, 39, -1, 17, 2, -40, 40, -41]         # the last two are out of range for 40 rows: poisoned


def _gather_want(src, idx):
    ok = (idx >= -src.shape[0]) & (idx < src.shape[0])
    want = _bits(src)[torch.where(ok, idx, torch.zeros_like(idx))].clone()
    want[~ok] = -1                                             # 0xFF bytes
    return want


@pytest.mark.parametrize("row_elems", [12, 16])               # row_bytes 48 and 64: both multiples of 16
@pytest.mark.parametrize("off_bytes", [8, 4])
@pytest.mark.parametrize("side", ["src", "dst"])
def test_gather_rows_behind_8_and_4_byte_bases(row_elems, off_bytes, side):
    """A row width that fits the 16-byte kernel behind a base that does not: the 8-byte and 4-byte element kernels."""
    from dxmi_hip import ops
    gen = torch.Generator().manual_seed(90)
    rows = torch.randn(40, row_elems, generator=gen).to(DEV)
    idx = torch.tensor(GATHER_IDX, dtype=torch.int64, device=DEV)
    src = Carved([rows], [off_bytes if side == "src" else 0])
    dst = Carved([torch.zeros(len(GATHER_IDX), row_elems, device=DEV)], [off_bytes if side == "dst" else 0])
    assert ops.gather_rows(src.views[0], idx, out=dst.views[0]) is dst.views[0]
    assert torch.equal(_bits(dst.views[0]), _gather_want(rows, idx))
    assert dst.guards_intact() and src.guards_intact() and _same_bits(src.views[0], rows)


def test_gather_rows_two_workgroups_per_row():
    """16 400-byte rows: 1025 vectors, blocks_per_row = 2, the second workgroup owning the last vector alone."""
    from dxmi_hip import ops
    gen = torch.Generator().manual_seed(91)
    rows = torch.randn(40, 4100, generator=gen).to(DEV)
    idx = torch.tensor(GATHER_IDX, dtype=torch.int64, device=DEV)
    dst = Carved([torch.zeros(len(GATHER_IDX), 4100, device=DEV)], [0])
    ops.gather_rows(rows, idx, out=dst.views[0])
    assert torch.equal(_bits(dst.views[0]), _gather_want(rows, idx))
    assert dst.guards_intact()
