"""CPU: the host side of the batch- and rank-invariant sampling noise (models.cm.random_util, dxmi_randn_indexed /
dxmi_randint_indexed).

The NumPy restatement of Philox-4x32-10 (tests/philox_ref.py) reproduces the Random123 known-answer vectors, so the GPU test's
expected words stand on the published generator.  The generators' index arithmetic is the reference's arange + clamp, restated
here, with the kernel call replaced by a recorder (no device needed); the draw counter, get_generator, DummyGenerator, the two
C-ABI symbols, the entries' argument checks (before any device call) and the generate_large.py flags."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import philox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1       # DXMI_EINVAL
SYMBOLS = ("dxmi_randn_indexed", "dxmi_randint_indexed")


# ------------------------------------------------------------------------------------------------------------- generator
@pytest.mark.parametrize("ctr, key, want", [
    # Random123 kat_vectors, philox4x32 with 10 rounds: zero, all ones, the digits of pi
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = philox_ref.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert tuple(int(v) for v in got) == want


def test_restated_words_layout():
    """words(): element e of a row is word e % 4 of the call with counter (e / 4, draw, index low, index high), key = seed halves."""
    idx, seed, draw = (1 << 32) + 5, (0x299f31d0 << 32) | 0xa4093822, 7
    w = philox_ref.words([idx], 11, seed, draw)
    assert w.shape == (1, 11) and w.dtype == np.uint32
    for e in range(11):
        one = philox_ref.philox4x32_10(np.array([e // 4, draw, 5, 1], dtype=np.uint32), np.array([0xa4093822, 0x299f31d0], dtype=np.uint32))
        assert w[0, e] == one[e % 4]


def test_uniforms_exact_and_open():
    """((x >> 9) + 0.5) 2^-23 needs 24 significand bits: fp32 holds it exactly, strictly inside (0, 1), for every word."""
    w = np.array([0, 0x1ff, 0x200, 0x7fffffff, 0x80000000, 0xfffffe00, 0xffffffff], dtype=np.uint32)
    u = philox_ref.uniforms(w)
    exact = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert np.array_equal(u.astype(np.float64), exact)
    assert u.min() == np.float32(2.0 ** -24) and u.max() == np.float32(1 - 2.0 ** -24)


# ----------------------------------------------------------------------------------------------------- models.cm.random_util
class Recorder:
    """Stands for dxmi_hip.ops: records what the generators hand to the kernel wrappers."""

    def __init__(self):
        self.calls = []

    def randn_indexed(self, sample_index, shape_tail, seed, draw, out=None):
        self.calls.append(("randn", sample_index.clone(), tuple(shape_tail), seed, draw))
        return torch.zeros((len(sample_index),) + tuple(shape_tail))

    def randint_indexed(self, sample_index, shape_tail, low, high, seed, draw, out=None):
        self.calls.append(("randint", sample_index.clone(), tuple(shape_tail), seed, draw, low, high))
        return torch.zeros((len(sample_index),) + tuple(shape_tail), dtype=torch.int64)


@pytest.fixture
def rec(monkeypatch):
    import models.cm.random_util as ru
    r = Recorder()
    monkeypatch.setattr(ru, "ops", r)
    return r


def reference_indices(rank, world, batch, done, num_samples):
    """models/cm/random_util.py get_global_size_and_indices / get_size_and_indices of the reference."""
    indices = torch.arange(done + rank, done + world * int(batch), world)
    return torch.clamp(indices, 0, num_samples - 1)


@pytest.mark.parametrize("cls", ["DeterministicGenerator", "DeterministicIndividualGenerator"])
def test_indices_are_the_references(rec, cls):
    import models.cm.random_util as ru
    num_samples = 37
    for world in (1, 2, 3, 8):
        for rank in sorted({0, world // 2, world - 1}):
            g = getattr(ru, cls)(num_samples, seed=5, rank=rank, world_size=world)
            for batch in (1, 4, 5):
                for done in (0, batch * world, 24, 32, 36, 40):      # 32 onwards: the clamp at the end of the run
                    g.set_done_samples(done)
                    rec.calls.clear()
                    g.randn(batch, 3, 2, 2, device="cpu")
                    g.randint(0, 10, (batch,), device="cpu")
                    g.randn_like(torch.zeros(batch, 5))
                    want = reference_indices(rank, world, batch, done, num_samples)
                    assert len(want) == batch and want.max() <= num_samples - 1
                    for c in rec.calls:
                        assert c[1].dtype == torch.int64 and torch.equal(c[1], want), (rank, world, batch, done)
                    assert [c[2] for c in rec.calls] == [(3, 2, 2), (), (5,)]
                    assert [c[3] for c in rec.calls] == [5, 5, 5]
    # the ranks of a world tile the run: every index once, in order
    gs = [ru.DeterministicGenerator(100, rank=r, world_size=4) for r in range(4)]
    tiles = torch.stack([g.get_indices(6, "cpu") for g in gs], dim=1).reshape(-1)
    assert torch.equal(tiles, torch.arange(24))


def test_draw_counter(rec):
    import models.cm.random_util as ru
    g = ru.get_generator("determ-indiv", 16, seed=3)
    assert (g.rank, g.world_size) == (0, 1)          # no process group: single rank
    g.randn(2, 3, device="cpu")
    g.randint(0, 4, (2,), device="cpu")              # randn and randint share one counter
    g.randn_like(torch.zeros(2, 3))
    assert [c[4] for c in rec.calls] == [0, 1, 2]
    g.set_done_samples(2)
    g.randn(2, 3, device="cpu")
    g.randn(2, 3, device="cpu")
    assert [c[4] for c in rec.calls[3:]] == [0, 1]
    g.set_seed(9)
    assert g.get_seed() == 9
    g.randn(2, 3, device="cpu")
    assert rec.calls[-1][3:5] == (9, 0) and torch.equal(rec.calls[-1][1], torch.tensor([2, 3]))      # done_samples kept
    assert rec.calls[-2][3] == 3


def test_dtype_is_a_cast_of_fp32(rec):
    import models.cm.random_util as ru
    g = ru.get_generator("determ", 4)
    assert g.randn(2, 3, device="cpu").dtype == torch.float32
    assert g.randn(2, 3, dtype=torch.float16, device="cpu").dtype == torch.float16
    assert g.randn_like(torch.zeros(2, 3, dtype=torch.bfloat16)).dtype == torch.bfloat16
    assert g.randint(0, 4, (2,), device="cpu").dtype == torch.int64
    assert g.randint(0, 4, (2,), dtype=torch.int32, device="cpu").dtype == torch.int32


def test_get_generator():
    import models.cm.random_util as ru
    assert isinstance(ru.get_generator("dummy"), ru.DummyGenerator)
    assert type(ru.get_generator("determ", 8, 1)) is ru.DeterministicGenerator
    assert type(ru.get_generator("determ-indiv", 8, 1)) is ru.DeterministicIndividualGenerator
    with pytest.raises(NotImplementedError):
        ru.get_generator("x")
    with pytest.raises(ValueError):
        ru.get_generator("determ")                   # num_samples = 0: no index to clamp to
    with pytest.raises(ValueError):
        ru.DeterministicGenerator(8, rank=2, world_size=2)


def test_dummy_generator_forwards_to_torch():
    import models.cm.random_util as ru
    g = ru.DummyGenerator()
    torch.manual_seed(11)
    a, b, c = g.randn(2, 3), g.randint(0, 7, (5,)), g.randn_like(torch.zeros(4, dtype=torch.float64))
    torch.manual_seed(11)
    assert torch.equal(a, torch.randn(2, 3)) and torch.equal(b, torch.randint(0, 7, (5,)))
    assert torch.equal(c, torch.randn_like(torch.zeros(4, dtype=torch.float64))) and c.dtype == torch.float64


def test_cpu_target_is_an_error():
    """No CPU fallback: the wrappers refuse host tensors, and so the generators refuse a CPU target."""
    from dxmi_hip import DxmiError, ops
    import models.cm.random_util as ru
    idx = torch.arange(2)
    with pytest.raises(DxmiError):
        ops.randn_indexed(idx, (4,), 0, 0)
    with pytest.raises(DxmiError):
        ops.randint_indexed(idx, (4,), 0, 5, 0, 0)
    g = ru.get_generator("determ", 4)
    with pytest.raises(DxmiError):
        g.randn(2, 4, device="cpu")
    with pytest.raises(DxmiError):
        g.randn_like(torch.zeros(2, 4))
    with pytest.raises(DxmiError):
        g.randint(0, 5, (2,), device="cpu")


# ------------------------------------------------------------------------------------------------------------------ C-ABI
def test_symbols_declared_and_exported():
    from dxmi_hip import _lib
    text = open(os.path.join(ROOT, "include", "dxmi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dxmi_[a-z0-9_]+)\s*\(", text))
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/dxmi_hip.h"
        assert hasattr(lib, s), f"{s} is not exported by the library"
        assert s in _lib.SIGNATURES


def test_entries_reject_bad_arguments():
    """Both entries validate before they touch the device."""
    from dxmi_hip import _lib
    lib = _lib.load()
    p, odd, null = ctypes.c_void_p(64), ctypes.c_void_p(68), ctypes.c_void_p(0)       # never dereferenced

    def randn(out=p, idx=p, N=2, per=12):
        return lib.dxmi_randn_indexed(out, idx, N, per, 1, 0, null)

    def randint(out=p, idx=p, N=2, per=12, low=0, high=10):
        return lib.dxmi_randint_indexed(out, idx, N, per, low, high, 1, 0, null)
    for fn in (randn, randint):
        assert fn(out=null) == EINVAL and b"null pointer" in lib.dxmi_last_error()
        assert fn(idx=null) == EINVAL
        assert fn(N=0) == EINVAL and fn(N=-3) == EINVAL and fn(N=70000) == EINVAL
        assert fn(per=0) == EINVAL and fn(per=-1) == EINVAL and fn(per=1 << 31) == EINVAL
        assert fn(out=odd) == EINVAL and b"16-byte aligned" in lib.dxmi_last_error()
    assert randint(low=5, high=5) == EINVAL and randint(low=5, high=4) == EINVAL
    assert randint(low=0, high=(1 << 31) + 1) == EINVAL and b"2^31" in lib.dxmi_last_error()
    assert randint(low=-(1 << 63), high=(1 << 63) - 1) == EINVAL


# ------------------------------------------------------------------------------------------------ generate_large.py flags
def test_cli_generator_flags():
    import generate_large as g
    base = ["--log_dir", "d", "--n_sample", "4"]
    a, _ = g.parse_args(base)
    assert (a.generator, a.seed) == ("dummy", None)
    a, _ = g.parse_args(base + ["--karras_sampler", "heun"])
    assert (a.generator, a.seed) == ("dummy", None)
    a, _ = g.parse_args(base + ["--karras_sampler", "heun", "--generator", "determ"])
    assert (a.generator, a.seed) == ("determ", None)
    a, _ = g.parse_args(base + ["--cm_sampler", "multistep", "--ts", "0,22,39", "--generator", "determ-indiv", "--seed", "7"])
    assert (a.generator, a.seed) == ("determ-indiv", 7)
    for extra in (["--generator", "determ"], ["--seed", "3"], ["--karras_sampler", "heun", "--seed", "3"],
                  ["--karras_sampler", "heun", "--generator", "philox"]):
        with pytest.raises(SystemExit):
            g.parse_args(base + extra)


def test_npz_order_is_the_global_index():
    """The gathered ranks' batches, put back into the order of the generators' indices."""
    import generate_large as g
    import models.cm.random_util as ru
    world, batch, n_batches = 3, 4, 2
    per_rank = []
    for r in range(world):
        gen = ru.DeterministicGenerator(world * batch * n_batches, rank=r, world_size=world)
        rows = []
        for b in range(n_batches):
            gen.set_done_samples(b * batch * world)
            rows.append(gen.get_indices(batch, "cpu"))
        per_rank.append(torch.cat(rows).reshape(-1, 1, 1, 1).expand(-1, 3, 2, 2).contiguous())
    out = g.index_order(per_rank, batch)
    assert out.shape == (24, 3, 2, 2) and torch.equal(out[:, 0, 0, 0], torch.arange(24)) and torch.equal(out[:, 2, 1, 1], torch.arange(24))
