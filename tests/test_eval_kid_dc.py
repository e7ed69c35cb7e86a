"""Kernel Inception Distance and density / coverage of the evaluator on the device (csrc/eval_metrics.hip: dxmi_kid_sums,
dxmi_dc_counts; dxmi_hip.ops.kid_sums / dc_counts; evaluations/evaluator.py --kid / --prdc), against an fp64 numpy
restatement of their definitions kept here (the reference evaluator has neither metric, so there is no golden file).

    Sxx = sum_{i != j} k(x_i, x_j)   Syy = sum_{i != j} k(y_i, y_j)   Sxy = sum_{i, j} k(x_i, y_j)   k(u, v) = (u . v gamma + coef0)^3
    KID = Sxx / (mx (mx - 1)) + Syy / (my (my - 1)) - 2 Sxy / (mx my)
    counts[i] = #{ j : d(a_i, b_j) < r_i }   density = sum_i counts[i] / (k NB)   coverage = mean_i (counts[i] > 0)

Bounds, none of them fitted to the kernels' output:
  * integer features (dots below 2^24: f32 and fp64 agree exactly, every term is the same fp64 number on both sides): a sum of n
    terms of one sign taken in two orders differs by at most (n + 16) 2^-52 of it; the counts are equal.
  * float features: |dot_f32 - dot| <= gD A_ij with A_ij = sum_k |u_k v_k|, gD = D u / (1 - D u), u = 2^-24 (a chain of D fused
    multiply-adds); the cube is monotone, so each sum lies in [sum (t - e)^3, sum (t + e)^3], e = gamma gD A_ij, widened by the
    reordering term above (taken of sum |term|, which is the sum itself for non-negative features).  Each count lies between
    #{d64 < r - b_ij} and #{d64 < r + b_ij}, b_ij = (D + 4) 2u (|a_i|^2 + |b_j|^2) (tests/test_eval_metrics.py: _err_bound).
CPU tests check the restatement against literal loops, the subset draw, the flags, the C-ABI's argument checks and the host
sanitizer driver; -m gpu runs the kernels.

Measured on an MI355X when these tests were written: integer features, worst relative difference of a sum 4.0e-16
(bounds 4e-15 .. 2e-11), counts equal; float features, worst relative error of a sum against the restatement beside the relative
half-width of its bracket: D 16 2.0e-10 / 4.6e-7, D 2023 2.8e-9 / 5.2e-5, D 2048 1.0e-9 / 5.2e-5, signed D 16 5.0e-10 / 1.5e-6;
the two count brackets differ in at most 80 of 6954 counted pairs (1000 x 2500, D 2048)."""
import ctypes
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffusion-by-maxentirl_amd")
TESTS = os.path.join(ROOT, "tests")
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from evaluations import evaluator as ev  # noqa: E402

U = 2.0 ** -24          # f32 unit roundoff
EPS64 = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_distances(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T, 0.0)


def np_radii(x, k):
    return np.partition(np_distances(x, x), k, axis=1)[:, k]


def _np_gram(a, b, gamma, coef0, same):
    """(k, A): the kernel matrix in fp64, t = dot * gamma + coef0 and (t * t) * t rounded as the kernel states them, the diagonal
    of a set against itself set to 0; A = sum_k |a_k b_k| for the error bound."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    t = (a @ b.T) * gamma + coef0
    k3 = (t * t) * t
    A = np.abs(a) @ np.abs(b).T
    if same:
        np.fill_diagonal(k3, 0.0)
    return t, k3, A


def np_kid_sums(x, y, gamma=None, coef0=1.0):
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    return np.array([_np_gram(x, x, gamma, coef0, True)[1].sum(), _np_gram(y, y, gamma, coef0, True)[1].sum(),
                     _np_gram(x, y, gamma, coef0, False)[1].sum()])


def kid_terms(mx, my):
    return np.array([mx * (mx - 1), my * (my - 1), mx * my], dtype=np.float64)


def np_kid_brackets(x, y, gamma=None, coef0=1.0):
    """(lo, mid, hi) fp64 [3] each: the restatement's sums and the interval the device sums must lie in (module docstring)."""
    D = x.shape[1]
    gamma = 1.0 / D if gamma is None else gamma
    gD = D * U / (1.0 - D * U)
    lo, mid, hi = np.empty(3), np.empty(3), np.empty(3)
    terms = kid_terms(len(x), len(y))
    for c, (a, b, same) in enumerate(((x, x, True), (y, y, True), (x, y, False))):
        t, k3, A = _np_gram(a, b, gamma, coef0, same)
        e = gamma * gD * A
        l3, h3 = (t - e) ** 3, (t + e) ** 3
        if same:
            np.fill_diagonal(l3, 0.0)
            np.fill_diagonal(h3, 0.0)
        reorder = (terms[c] + 16) * EPS64 * np.maximum(np.abs(l3), np.abs(h3)).sum()
        lo[c], mid[c], hi[c] = l3.sum() - reorder, k3.sum(), h3.sum() + reorder
    return lo, mid, hi


def kid_value(sums, mx, my):
    return sums[..., 0] / (mx * (mx - 1)) + sums[..., 1] / (my * (my - 1)) - 2.0 * sums[..., 2] / (mx * my)


def np_kid(x, y, ix=None, iy=None):
    """Per-subset estimates (fp64 [S]); ix None: the one estimate over all rows."""
    if ix is None:
        return np.array([kid_value(np_kid_sums(x, y), len(x), len(y))])
    return np.array([kid_value(np_kid_sums(x[i], y[j]), len(i), len(j)) for i, j in zip(ix, iy)])


def np_dc_counts(a, r, b, strict=True):
    d = np_distances(a, b)
    return ((d < r[:, None]) if strict else (d <= r[:, None])).sum(1).astype(np.int32)


def np_density_coverage(a, b, k, strict=True):
    c = np_dc_counts(a, np_radii(a, k), b, strict)
    return c.sum() / (k * len(b)), (c > 0).mean()


# ------------------------------------------------------------------------------------------------ feature generators
INT_CASES = [(300, 257, 16, 3), (50, 37, 24, 5), (260, 390, 24, 5), (129, 128, 16, 5)]


@functools.lru_cache(maxsize=None)
def int_features(na, nb, D, k):
    """Small non-negative integer features (tests/golden/make_golden_eval.py): every dot is an integer below 2^24 and every
    distance an integer, so f32 and fp64 agree exactly and ties d == r are common.  A third of the sample rows are shifted by one
    (clipped at the top value); duplicated reference rows, k + 1 copies of one among them, make some radii 0."""
    rng = np.random.default_rng(1000 * na + nb + D + k)
    a, b = rng.integers(0, 6, size=(na, D)), rng.integers(0, 6, size=(nb, D))
    b[::3] = np.minimum(b[::3] + 1, 5)
    if na >= 4 * (k + 1):
        a[1:k + 1] = a[0]
    for i in range(max(1, na // 10)):
        a[na - 1 - i] = a[k + 1 + i] if na > 2 * (k + 2 + i) else a[0]
    a, b = a.astype(np.float32), b.astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def float_features(n, D, seed, shift=0.0, signed=False):
    """pool3-like features relu(z M): ONE projection M per D shared by every set (two projections would give sets that do not
    overlap, and every count 0), z standard normal with latent 16, the sample set's z shifted."""
    M = np.random.default_rng(7000 + D).standard_normal((16, D)) / 4.0
    f = (np.random.default_rng(seed).standard_normal((n, 16)) + shift) @ M
    f = (f if signed else np.maximum(f, 0.0)).astype(np.float32)
    f.setflags(write=False)
    return f


def float_pair(NA, NB, D, signed=False):
    return float_features(NA, D, NA + D, 0.0, signed), float_features(NB, D, NB + D + 1, 0.5, signed)


def dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).cuda()         # the cached features are read-only


# ------------------------------------------------------------------------------------------------ CPU
def test_restatement_against_literal_loops():
    """Diagonal exclusion, the three denominators and the strict comparison, pair by pair at tiny sizes."""
    rng = np.random.default_rng(0)
    x, y = rng.integers(0, 4, size=(5, 3)).astype(np.float32), rng.integers(0, 4, size=(4, 3)).astype(np.float32)
    y[1] = x[2]
    k = lambda u, v: (float(np.dot(u.astype(np.float64), v.astype(np.float64))) / 3.0 + 1.0) ** 3
    sxx = sum(k(x[i], x[j]) for i in range(5) for j in range(5) if i != j)
    syy = sum(k(y[i], y[j]) for i in range(4) for j in range(4) if i != j)
    sxy = sum(k(x[i], y[j]) for i in range(5) for j in range(4))
    got = np_kid_sums(x, y)
    assert np.allclose(got, [sxx, syy, sxy], rtol=1e-14, atol=0)
    assert np_kid(x, y)[0] == pytest.approx(sxx / 20 + syy / 12 - 2 * sxy / 20, rel=1e-13)
    ix, iy = np.array([[0, 2, 4], [1, 2, 3]]), np.array([[3, 1, 0], [0, 1, 2]])
    for s in range(2):
        xs, ys = x[ix[s]], y[iy[s]]
        a = sum(k(xs[i], xs[j]) for i in range(3) for j in range(3) if i != j)
        b = sum(k(ys[i], ys[j]) for i in range(3) for j in range(3) if i != j)
        c = sum(k(xs[i], ys[j]) for i in range(3) for j in range(3))
        assert np_kid(x, y, ix, iy)[s] == pytest.approx((a + b) / 6 - 2 * c / 9, rel=1e-13)
    lo, mid, hi = np_kid_brackets(x, y)
    assert np.array_equal(mid, got) and (lo < mid).all() and (mid < hi).all()
    # counts: d(a_i, b_j) < r_i with r_i the distance to the k-th nearest OTHER row; x[2] == y[1] sits at distance 0
    d = lambda u, v: float(((u.astype(np.float64) - v.astype(np.float64)) ** 2).sum())
    kk = 2
    r = [sorted(d(x[i], x[j]) for j in range(5))[kk] for i in range(5)]
    assert np.array_equal(np_radii(x, kk), r)
    for strict in (True, False):
        c = [sum((d(x[i], y[j]) < r[i]) if strict else (d(x[i], y[j]) <= r[i]) for j in range(4)) for i in range(5)]
        assert np.array_equal(np_dc_counts(x, np.array(r), y, strict), c)
        dens, cov = np_density_coverage(x, y, kk, strict)
        assert dens == sum(c) / (kk * 4) and cov == sum(v > 0 for v in c) / 5
    assert np_dc_counts(x, np.zeros(5), y)[2] == 0 and np_dc_counts(x, np.zeros(5), y, strict=False)[2] == 1


@pytest.mark.parametrize("na,nb,D,k", INT_CASES)
def test_integer_features_pin_the_contract(na, nb, D, k):
    """The integer cases are not vacuous: ties d == r separate `<` from `<=`, some radii are 0, coverage is strictly between 0
    and 1, the sets differ (KID > 0), and every dot is exact in f32."""
    a, b = int_features(na, nb, D, k)
    assert float(max((a * a).sum(1).max(), (b * b).sum(1).max())) < 2 ** 24
    r = np_radii(a, k)
    assert (r == 0).any() and (r > 0).any()
    strict, loose = np_density_coverage(a, b, k, True), np_density_coverage(a, b, k, False)
    assert strict[0] != loose[0] and 0.0 < strict[1] < 1.0
    assert (np_dc_counts(a, r, b)[r == 0] == 0).all()
    assert np_kid(a, b)[0] > 0


def test_kid_subset_indices():
    ix, iy = ev.kid_subset_indices(300, 257, 7, 50, seed=3)
    assert ix.shape == (7, 50) and iy.shape == (7, 50) and ix.dtype == np.int32 and iy.dtype == np.int32
    assert all(len(set(r)) == 50 for r in ix) and all(len(set(r)) == 50 for r in iy)
    assert 0 <= ix.min() and ix.max() < 300 and 0 <= iy.min() and iy.max() < 257
    again = ev.kid_subset_indices(300, 257, 7, 50, seed=3)
    assert np.array_equal(ix, again[0]) and np.array_equal(iy, again[1])
    other = ev.kid_subset_indices(300, 257, 7, 50, seed=4)
    assert not np.array_equal(ix, other[0])
    # the documented draw: one generator, per subset the first set's rows and then the second's
    rng = np.random.default_rng(3)
    for s in range(7):
        assert np.array_equal(ix[s], rng.choice(300, 50, replace=False)) and np.array_equal(iy[s], rng.choice(257, 50, replace=False))
    # m = min(nx, ny, subset_size); a subset of a whole set is a permutation of it
    ix, iy = ev.kid_subset_indices(90, 70, 4, 1000, seed=0)
    assert ix.shape == (4, 70) and iy.shape == (4, 70) and all(sorted(r) == list(range(70)) for r in iy)
    assert ev.kid_subset_indices(40, 70, 2, 50, seed=0)[1].shape == (2, 40)
    assert ev.kid_subset_indices(40, 70, 0, 50, seed=0)[0].shape == (0, 40)


def test_parse_args_new_flags():
    a = ev.parse_args(["r.npz", "s.npz"])
    assert (a.kid, a.kid_subsets, a.kid_subset_size, a.kid_seed, a.prdc, a.dc_k) == (False, 100, 1000, 0, False, 5)
    a = ev.parse_args(["r.npz", "s.npz", "--kid", "--kid_subsets", "4", "--kid_subset_size", "50", "--kid_seed", "9", "--prdc", "--dc_k", "3"])
    assert (a.kid, a.kid_subsets, a.kid_subset_size, a.kid_seed, a.prdc, a.dc_k) == (True, 4, 50, 9, True, 3)
    assert ev.parse_args(["r.npz", "s.npz", "--kid", "--kid_subsets", "0"]).kid_subsets == 0
    for bad in (["--kid_subsets", "-1"], ["--kid_subset_size", "1"], ["--dc_k", "0"]):
        with pytest.raises(SystemExit):
            ev.parse_args(["r.npz", "s.npz"] + bad)


def test_cabi_argument_validation_is_host_side():
    from dxmi_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    kid = lambda X=p, NX=300, Y=p, NY=257, D=16, ix=p, iy=p, S=3, mx=50, my=50, sums=p, ws=p: lib.dxmi_kid_sums(
        X, NX, Y, NY, D, ix, iy, S, mx, my, 1.0 / 16, 1.0, sums, ws, None)
    EINVAL = kid(X=None)
    assert EINVAL != 0 and b"null" in lib.dxmi_last_error()
    for kw in (dict(Y=None), dict(sums=None), dict(ws=None), dict(D=0), dict(D=-4), dict(mx=1), dict(my=1), dict(my=0), dict(S=0), dict(S=-2),
               dict(ix=None), dict(iy=None), dict(NX=0), dict(NY=-1),
               dict(ix=None, iy=None, S=3, mx=300, my=257),              # null indices: one subset
               dict(ix=None, iy=None, S=1, mx=50, my=257),               # null indices: all rows
               dict(ix=None, iy=None, S=1, mx=300, my=256)):
        assert kid(**kw) == EINVAL, kw
        assert lib.dxmi_last_error().startswith(b"dxmi_kid_sums"), kw
    dc = lambda A=p, NA=300, rA=p, B=p, NB=257, D=16, splits=0, counts=p, ws=p: lib.dxmi_dc_counts(A, NA, rA, B, NB, D, splits, counts, ws, None)
    for kw in (dict(A=None), dict(rA=None), dict(B=None), dict(counts=None), dict(ws=None), dict(NA=0), dict(NB=0), dict(NB=-5), dict(D=0),
               dict(splits=-1)):
        assert dc(**kw) == EINVAL, kw
        assert lib.dxmi_last_error().startswith(b"dxmi_dc_counts"), kw


def test_workspace_sizes_are_linear_in_tiles():
    from dxmi_hip import _lib
    lib = _lib.load()
    kw = lib.dxmi_kid_sums_workspace_bytes
    tiles = lambda mx, my: (lambda tx, ty: tx * (tx + 1) // 2 + ty * (ty + 1) // 2 + tx * ty)((mx + 127) // 128, (my + 127) // 128)
    for S, mx, my in ((1, 2, 2), (1, 128, 129), (7, 200, 200), (100, 1000, 1000), (1, 10000, 50000), (1, 50000, 50000)):
        assert kw(S, mx, my, 2048) == 8 * S * tiles(mx, my), (S, mx, my)
    assert kw(1, 50000, 50000, 2048) < 50000 * 50000 * 4 // 1000          # 2.4 MB of partials against a 10 GB Gram matrix
    assert [kw(0, 50, 50, 16), kw(-1, 50, 50, 16), kw(3, 1, 50, 16), kw(3, 50, 1, 16), kw(3, 50, 50, 0), kw(3, 50, -50, 16)] == [0] * 6
    dw = lib.dxmi_dc_counts_workspace_bytes
    pad = lambda n: (4 * n + 255) // 256 * 256
    for NA, NB, s in ((300, 257, 1), (300, 257, 2), (1000, 2500, 7), (6, 2, 1)):
        assert dw(NA, NB, s) == pad(NA) + pad(NB) + min(s, (NB + 127) // 128) * NA * 4, (NA, NB, s)
    assert 0 < dw(10000, 50000, 0) < 10000 * 50000 * 4 // 100 and dw(20000, 50000, 0) < 2.2 * dw(10000, 50000, 0)
    assert [dw(0, 257, 0), dw(300, 0, 0), dw(-1, 257, 0), dw(300, 257, -1)] == [0] * 4


def test_no_gpu_means_loud_failure_for_kid_and_dc():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dxmi_hip import DxmiError, ops
    x, y = torch.rand(16, 8), torch.rand(12, 8)
    with pytest.raises(DxmiError):
        ops.kid_sums(x, y)
    with pytest.raises(DxmiError):
        ops.kid_sums(x, y, torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(DxmiError):
        ops.dc_counts(x, torch.ones(16), y)
    with pytest.raises(DxmiError):
        ev.kernel_inception_distance(x, y, subsets=3, subset_size=5)
    with pytest.raises(DxmiError):
        ev.kernel_inception_distance(x, y, subsets=0)
    with pytest.raises(DxmiError):
        ev.density_coverage(x, y, k=5)


def test_density_coverage_needs_k_plus_one_rows():
    with pytest.raises(ValueError, match="at least 6"):
        ev.density_coverage(torch.rand(5, 8), torch.rand(12, 8), k=5)


def test_kid_and_dc_arguments_under_address_and_ub_sanitizers():
    """`make asan_evalx` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_evalx.c, a program with its own main, against it and a no-device HIP runtime stub.  Null pointers,
    D <= 0, subsets of fewer than two rows, S < 1, one index list without the other, null indices with S != 1 or a subset that is
    not all rows, empty sets, negative splits and tile counts past one launch must each come back as DXMI_EINVAL with the message
    of their check, and as 0 from the workspace functions: no crash, no sanitizer report.  The program runs as a child process;
    nothing is loaded into python.  A host-only build: machines without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_evalx"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_evalx")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") >= 80


# ------------------------------------------------------------------------------------------------ GPU: exact contract
def _assert_sums_reordered(got, want, terms, what):
    """got, want fp64 [3]: sums of the same positive fp64 terms in two orders."""
    rel = np.abs(got - want) / want
    bound = (terms + 16) * EPS64
    print(f"{what}: relative difference {rel} against {bound}")
    assert (rel <= bound).all(), (what, rel, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("mx,my", [(2, 2), (2, 5), (127, 129), (128, 128), (300, 257)])
def test_kid_sums_exact_on_integer_features_all_rows(mx, my):
    from dxmi_hip import ops
    a, b = int_features(300, 257, 16, 3)
    x, y = a[:mx], b[:my]
    got = ops.kid_sums(dev(x), dev(y)).cpu().numpy()
    assert got.shape == (1, 3)
    _assert_sums_reordered(got[0], np_kid_sums(x, y), kid_terms(mx, my), f"all rows {mx} x {my}")


@pytest.mark.gpu
@pytest.mark.parametrize("S,m", [(1, 2), (3, 50), (7, 129), (3, 200), (1, 200), (7, 2)])
def test_kid_sums_exact_on_integer_features_subsets(S, m):
    from dxmi_hip import ops
    x, y = int_features(300, 257, 24, 5)
    ix, iy = ev.kid_subset_indices(300, 257, S, m, seed=S * 1000 + m)
    if S > 1:
        ix[1, 0], iy[1, 0] = ix[0, 0], iy[0, 0]                                   # one row appears in two subsets
        ix[1, 1:], iy[1, 1:] = np.setdiff1d(np.arange(300), ix[1, :1])[:m - 1], np.setdiff1d(np.arange(257), iy[1, :1])[:m - 1]
    got = ops.kid_sums(dev(x), dev(y), dev(ix), dev(iy)).cpu().numpy()
    assert got.shape == (S, 3)
    for s in range(S):
        _assert_sums_reordered(got[s], np_kid_sums(x[ix[s]], y[iy[s]]), kid_terms(m, m), f"subset {s} of {S} x {m}")


@pytest.mark.gpu
def test_kid_sums_unequal_subset_sizes_and_kernel_parameters():
    """mx != my with indices, and gamma / coef0 other than the defaults (exact in fp64: 1 / 8 and 2)."""
    from dxmi_hip import ops
    x, y = int_features(300, 257, 16, 3)
    rng = np.random.default_rng(5)
    ix = np.stack([rng.choice(300, 130, replace=False) for _ in range(3)]).astype(np.int32)
    iy = np.stack([rng.choice(257, 47, replace=False) for _ in range(3)]).astype(np.int32)
    got = ops.kid_sums(dev(x), dev(y), dev(ix), dev(iy), gamma=0.125, coef0=2.0).cpu().numpy()
    for s in range(3):
        _assert_sums_reordered(got[s], np_kid_sums(x[ix[s]], y[iy[s]], 0.125, 2.0), kid_terms(130, 47), f"subset {s}, 130 x 47")


@pytest.mark.gpu
@pytest.mark.parametrize("na,nb,D,k", INT_CASES + [(6, 2, 16, 5)])
def test_dc_counts_exact_on_integer_features(na, nb, D, k):
    from dxmi_hip import ops
    a, b = int_features(na, nb, D, k)
    r = ops.knn_radii(dev(a), k)
    assert np.array_equal(r.cpu().numpy().astype(np.float64), np_radii(a, k))
    got = ops.dc_counts(dev(a), r, dev(b))
    want = torch.from_numpy(np_dc_counts(a, np_radii(a, k), b))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    assert int(got[r == 0].sum()) == 0
    if na > 6:
        assert not np.array_equal(want.numpy(), np_dc_counts(a, np_radii(a, k), b, strict=False))     # `<=` would be caught
    dens, cov = ev.density_coverage(dev(a), dev(b), k)
    assert (dens, cov) == tuple(float(v) for v in np_density_coverage(a, b, k))


# ------------------------------------------------------------------------------------------------ GPU: float features
FLOAT_SHAPES = [(129, 255), (300, 517), (1000, 2500)]


def _check_kid_bracket(x, y, what):
    from dxmi_hip import ops
    got = ops.kid_sums(dev(x), dev(y)).cpu().numpy()[0]
    lo, mid, hi = np_kid_brackets(x, y)
    for c, name in enumerate(("Sxx", "Syy", "Sxy")):
        print(f"{what} {name}: relative error {abs(got[c] - mid[c]) / abs(mid[c]):.3e}, bracket half-width "
              f"{(hi[c] - lo[c]) / 2 / abs(mid[c]):.3e}")
    assert (lo <= got).all() and (got <= hi).all(), (what, lo, got, hi)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 2023, 2048])
@pytest.mark.parametrize("NA,NB", FLOAT_SHAPES)
def test_kid_sums_within_f32_dot_bracket(NA, NB, D):
    x, y = float_pair(NA, NB, D)
    got = _check_kid_bracket(x, y, f"{NA} x {NB} D {D}")
    assert kid_value(got, NA, NB) > 0.05                                            # the shifted set is far from the reference


@pytest.mark.gpu
def test_kid_sums_within_f32_dot_bracket_signed_features():
    x, y = float_pair(300, 517, 16, signed=True)
    assert (x < 0).any() and (y < 0).any()
    _check_kid_bracket(x, y, "signed 300 x 517 D 16")


def _check_count_bracket(a, b, k, what):
    from dxmi_hip import ops
    D = a.shape[1]
    r = ops.knn_radii(dev(a), k)
    got = ops.dc_counts(dev(a), r, dev(b)).cpu().numpy()
    d, r64 = np_distances(a, b), r.cpu().numpy().astype(np.float64)[:, None]
    na, nb = (a.astype(np.float64) ** 2).sum(1), (b.astype(np.float64) ** 2).sum(1)
    bound = (D + 4) * 2.0 * U * (na[:, None] + nb[None, :])
    lo, hi = (d < r64 - bound).sum(1), (d < r64 + bound).sum(1)
    print(f"{what}: {int(got.sum())} pairs counted, brackets differ in {int((hi - lo).sum())}, density {got.sum() / (k * len(b)):.3f}, "
          f"coverage {(got > 0).mean():.3f}")
    assert (lo <= got).all() and (got <= hi).all(), what
    assert got.sum() > 0 and (got > 0).mean() < 1.0                                 # not vacuous
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 2023, 2048])
@pytest.mark.parametrize("NA,NB", FLOAT_SHAPES)
def test_dc_counts_within_f32_distance_bracket(NA, NB, D):
    a, b = float_pair(NA, NB, D)
    _check_count_bracket(a, b, 5, f"{NA} x {NB} D {D}")


@pytest.mark.gpu
def test_dc_counts_within_f32_distance_bracket_signed_features():
    a, b = float_pair(300, 517, 16, signed=True)
    _check_count_bracket(a, b, 3, "signed 300 x 517 D 16")


# ------------------------------------------------------------------------------------------------ GPU: bitwise properties
@pytest.mark.gpu
def test_kid_sums_bitwise_properties():
    from dxmi_hip import _lib, ops
    xn, yn = float_pair(300, 517, 2023)
    x, y = dev(xn), dev(yn)
    ixn, iyn = ev.kid_subset_indices(300, 517, 7, 200, seed=1)
    ix, iy = dev(ixn), dev(iyn)
    base = ops.kid_sums(x, y, ix, iy)
    assert torch.equal(ops.kid_sums(x, y, ix, iy), base)                            # twice: identical
    need = _lib.load().dxmi_kid_sums_workspace_bytes(7, 200, 200, 2023)
    ws = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN-filled scratch of its own
    assert torch.equal(ops.kid_sums(x, y, ix, iy, workspace=ws), base)
    assert torch.isfinite(base).all()
    for s in range(7):
        # the gathered rows as a set of their own, and the subset in a launch of its own
        assert torch.equal(ops.kid_sums(x[ix[s].long()].contiguous(), y[iy[s].long()].contiguous())[0], base[s]), s
        assert torch.equal(ops.kid_sums(x, y, ix[s:s + 1].contiguous(), iy[s:s + 1].contiguous())[0], base[s]), s
    # the order of a subset's sum depends on (mx, my, D) alone: the same subset in another place of another batch
    again = ops.kid_sums(x, y, torch.cat([ix[4:5], ix[:3]]).contiguous(), torch.cat([iy[4:5], iy[:3]]).contiguous())
    assert torch.equal(again[0], base[4]) and torch.equal(again[1:], base[:3])
    full = ops.kid_sums(x, y)
    assert torch.equal(ops.kid_sums(x, y), full)
    ws = torch.full((_lib.load().dxmi_kid_sums_workspace_bytes(1, 300, 517, 2023) + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    assert torch.equal(ops.kid_sums(x, y, workspace=ws), full)
    # the dot is bitwise symmetric: swapping the sets swaps Sxx and Syy and leaves Sxy's terms (their order changes)
    swapped = ops.kid_sums(y, x)
    assert swapped[0, 0] == full[0, 1] and swapped[0, 1] == full[0, 0]
    assert abs(float(swapped[0, 2] - full[0, 2])) <= (300 * 517 + 16) * EPS64 * float(full[0, 2])


@pytest.mark.gpu
def test_dc_counts_bitwise_properties():
    from dxmi_hip import _lib, ops
    an, bn = float_pair(1000, 2500, 2023)
    a, b = dev(an), dev(bn)
    ra = ops.knn_radii(a, 5)
    base = ops.dc_counts(a, ra, b)
    assert torch.equal(ops.dc_counts(a, ra, b), base)
    lib = _lib.load()
    for s in (1, 2, 3, 7, 8):
        ws = torch.full((lib.dxmi_dc_counts_workspace_bytes(1000, 2500, s) + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
        assert torch.equal(ops.dc_counts(a, ra, b, splits=s, workspace=ws), base), s
    g = torch.Generator().manual_seed(1)
    pa, pb = torch.randperm(1000, generator=g).cuda(), torch.randperm(2500, generator=g).cuda()
    assert torch.equal(ops.dc_counts(a[pa].contiguous(), ra[pa].contiguous(), b), base[pa])
    assert torch.equal(ops.dc_counts(a, ra, b[pb].contiguous()), base)             # integers: the order of the columns is nothing
    # a set against itself with its own radii: a row is inside its own ball unless the ball is empty (radius 0, strict)
    ai = dev(int_features(300, 257, 16, 3)[0])
    for x, k in ((a, 5), (ai, 3)):
        r = ops.knn_radii(x, k)
        c = ops.dc_counts(x, r, x)
        assert bool((c[r > 0] >= 1).all()) and bool((c[r == 0] == 0).all())
    assert int((ops.knn_radii(ai, 3) == 0).sum()) >= 4


@pytest.mark.gpu
def test_kid_sums_checks_indices_before_launching():
    from dxmi_hip import ops
    x, y = dev(int_features(300, 257, 16, 3)[0]), dev(int_features(300, 257, 16, 3)[1])
    ixn, iyn = ev.kid_subset_indices(300, 257, 3, 50, seed=0)
    for which, bad in ((0, -1), (0, 300), (1, -1), (1, 257)):
        ix, iy = ixn.copy(), iyn.copy()
        (ix, iy)[which][2, 7] = bad
        with pytest.raises(ValueError, match="outside"):
            ops.kid_sums(x, y, dev(ix), dev(iy))
    with pytest.raises(ValueError, match="both"):
        ops.kid_sums(x, y, dev(ixn), None)
    with pytest.raises(ValueError, match="int32"):
        ops.kid_sums(x, y, dev(ixn.astype(np.int64)), dev(iyn.astype(np.int64)))


# ------------------------------------------------------------------------------------------------ GPU: memory
@pytest.mark.gpu
def test_no_quadratic_memory():
    from dxmi_hip import ops
    m, S = 2500, 4
    x, y = dev(float_features(m, 16, 1)), dev(float_features(m, 16, 2, 0.5))
    ixn, iyn = ev.kid_subset_indices(m, m, S, m, seed=0)
    ix, iy = dev(ixn), dev(iyn)
    ops.kid_sums(x, y, ix, iy)                                                      # the grow-only scratch buffer exists
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    sums = ops.kid_sums(x, y, ix, iy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < m * m * 4 / 10, peak
    assert torch.isfinite(sums).all()
    a, b = dev(float_features(1000, 64, 3)), dev(float_features(2500, 64, 4, 0.5))
    r = ops.knn_radii(a, 5)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    c = ops.dc_counts(a, r, b)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 1000 * 2500 * 4 / 10, peak
    assert int(c.sum()) > 0


# ------------------------------------------------------------------------------------------------ GPU: command line
OLD_LINES = ["Inception Score", "FID", "sFID", "Precision", "Recall"]
NEW_LINES = ["KID", "KID std", "Density", "Coverage"]


def _images(n, seed, hw=16):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(n, 4, 4, 3))
    noise = rng.integers(-20, 21, size=(n, hw, hw, 3))
    return np.clip(np.repeat(np.repeat(base, hw // 4, 1), hw // 4, 2) + noise, 0, 255).astype(np.uint8)


def _run_cli(rp, sp, *flags):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([TESTS, PKG, ROOT]))
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluations", "evaluator.py"), rp, sp, "--extractor",
                        "eval_extractor_stub:PoolSpatialFeatures", "--batch_size", "16", *flags], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [l.split(":", 1) for l in r.stdout.splitlines() if l.split(":")[0] in OLD_LINES + NEW_LINES]


@pytest.mark.gpu
def test_cli_prints_the_new_lines_only_when_asked(tmp_path):
    from dxmi_hip import ops
    from eval_extractor_stub import PoolSpatialFeatures
    ref, sample = _images(90, seed=10), _images(70, seed=11)
    rp, sp = str(tmp_path / "ref.npz"), str(tmp_path / "sample.npz")
    np.savez(rp, ref)
    np.savez_compressed(sp, sample)
    plain = _run_cli(rp, sp)
    assert [l[0] for l in plain] == OLD_LINES
    S, m, k = 4, 50, 3
    asked = _run_cli(rp, sp, "--kid", "--kid_subsets", str(S), "--kid_subset_size", str(m), "--prdc", "--dc_k", str(k))
    assert [l[0] for l in asked] == OLD_LINES + NEW_LINES
    assert asked[:5] == plain                                                        # the five old values, digit for digit
    kid, kid_std, density, coverage = (float(l[1]) for l in asked[5:])
    # the same features the command line computed (same reader, extractor and batch size), and the device's own radii
    ext = PoolSpatialFeatures()
    a_dev, b_dev = ev.read_activations(rp, ext, 16)[0], ev.read_activations(sp, ext, 16)[0]
    a, b = a_dev.cpu().numpy(), b_dev.cpu().numpy()
    ix, iy = ev.kid_subset_indices(90, 70, S, m, seed=0)
    want = np_kid(a, b, ix, iy)
    lo, hi = np.empty(S), np.empty(S)
    for s in range(S):
        slo, _, shi = np_kid_brackets(a[ix[s]], b[iy[s]])
        lo[s] = (slo[0] + slo[1]) / (m * (m - 1)) - 2.0 * shi[2] / (m * m)
        hi[s] = (shi[0] + shi[1]) / (m * (m - 1)) - 2.0 * slo[2] / (m * m)
    assert (lo <= want).all() and (want <= hi).all()
    print(f"KID {kid} in [{lo.mean()}, {hi.mean()}], restatement {want.mean()}; std {kid_std}, restatement {want.std()}")
    assert lo.mean() <= kid <= hi.mean()
    # |std(v) - std(w)| <= sqrt(mean((v - w)^2)) for any two vectors: each device estimate is within its bracket of the restatement's
    half = np.maximum(hi - want, want - lo)
    assert abs(kid_std - want.std()) <= np.sqrt((half ** 2).mean())
    r = ops.knn_radii(a_dev, k).cpu().numpy().astype(np.float64)[:, None]
    d = np_distances(a, b)
    bound = (a.shape[1] + 4) * 2.0 * U * ((a.astype(np.float64) ** 2).sum(1)[:, None] + (b.astype(np.float64) ** 2).sum(1)[None, :])
    clo, chi = (d < r - bound).sum(1), (d < r + bound).sum(1)
    print(f"density {density} in [{clo.sum() / (k * 70)}, {chi.sum() / (k * 70)}], coverage {coverage} in [{(clo > 0).mean()}, {(chi > 0).mean()}]")
    assert clo.sum() / (k * 70) <= density <= chi.sum() / (k * 70)
    assert (clo > 0).mean() <= coverage <= (chi > 0).mean()
    # in process: evaluate keeps its 5-tuple and fills `extra` with the same numbers
    extra = {}
    five = ev.evaluate(rp, sp, ext, 16, kid=dict(subsets=S, subset_size=m, seed=0), prdc=dict(k=k), extra=extra)
    assert len(five) == 5 and [repr(v) for v in five] == [l[1].strip() for l in plain]
    assert extra == {"kid": (kid, kid_std), "prdc": (density, coverage)}
    full, zero = ev.kernel_inception_distance(a_dev, b_dev, subsets=0)
    flo, _, fhi = np_kid_brackets(a, b)
    assert zero == 0.0 and kid_value(np.array([flo[0], flo[1], fhi[2]]), 90, 70) <= full <= kid_value(np.array([fhi[0], fhi[1], flo[2]]), 90, 70)
