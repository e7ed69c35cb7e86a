"""Precision / recall (k-NN radii, manifold membership) and Inception Score of the ADM evaluator on the device
(csrc/eval_metrics.hip, dxmi_hip.ops.knn_radii / pr_membership / inception_score), against:
  * tests/golden/eval_metrics.npz, written by tests/golden/make_golden_eval.py from the reference evaluator's own metric code;
  * an fp64 numpy / torch restatement kept here, with error bounds derived from the f32 arithmetic.
CPU tests check the restatement against the fixture and the C-ABI's argument validation; -m gpu runs the kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_metrics.npz")
U = 2.0 ** -24          # f32 unit roundoff


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_distances(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T, 0.0)


def np_radii(x, k):
    """Sorted position k of each row of the set-against-itself distances (the self-distance and duplicates count)."""
    return np.partition(np_distances(x, x), k, axis=1)[:, k]


def np_precision_recall(a, b, k):
    ra, rb = np_radii(a, k), np_radii(b, k)
    d = np_distances(a, b)
    a_in_b = (d <= rb[None, :]).any(1)          # reference rows inside the sample manifold: recall
    b_in_a = (d <= ra[:, None]).any(0)          # sample rows inside the reference manifold: precision
    return b_in_a.mean(), a_in_b.mean()


def np_inception_score(pool, w, split=5000):
    z = pool.astype(np.float64) @ w.astype(np.float64)
    z -= z.max(1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(1, keepdims=True)
    scores = []
    for i in range(0, len(p), split):
        part = p[i:i + split]
        kl = (part * (np.log(part) - np.log(part.mean(0, keepdims=True)))).sum(1).mean()
        scores.append(np.exp(kl))
    return float(np.mean(scores))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _cases(g):
    return [str(c) for c in g["cases"]]


# ------------------------------------------------------------------------------------------------ CPU
def test_restatement_matches_reference_fixture(golden):
    """The contract the fixture pins: radii = sorted position k with self and duplicates counted, precision = mean over the
    SAMPLE flags, recall = mean over the reference flags, IS over splits of 5000 (the last one short)."""
    for name in _cases(golden):
        a, b, k = golden[f"{name}/a"], golden[f"{name}/b"], int(golden[f"{name}/k"])
        assert np.array_equal(np_radii(a, k), golden[f"{name}/radii_a"].astype(np.float64)), name
        assert np.array_equal(np_radii(b, k), golden[f"{name}/radii_b"].astype(np.float64)), name
        p, r = np_precision_recall(a, b, k)
        assert p == float(golden[f"{name}/precision"]) and r == float(golden[f"{name}/recall"]), name
    assert len(golden["is/pool"]) % 5000 != 0 and len(golden["is/pool"]) > 10000
    assert np_inception_score(golden["is/pool"], golden["is/w"]) == pytest.approx(float(golden["is/score"]), rel=1e-5)


def test_fixture_covers_the_issue_cases(golden):
    sizes = {len(golden[f"{n}/{s}"]) for n in _cases(golden) for s in "ab"}
    assert any(n < 128 for n in sizes) and all(n % 128 for n in sizes)
    assert {int(golden[f"{n}/k"]) for n in _cases(golden)} == {3, 5}
    assert any(len(np.unique(golden[f"{n}/a"], axis=0)) < len(golden[f"{n}/a"]) for n in _cases(golden))


def test_cabi_argument_validation_is_host_side():
    from dxmi_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL = lib.dxmi_knn_radii(None, 16, 4, 3, 0, p, p, None)
    assert EINVAL != 0 and b"null" in lib.dxmi_last_error()
    for N, D, k in ((3, 4, 3), (16, 0, 3), (16, 4, 0), (16, 4, 8)):
        assert lib.dxmi_knn_radii(p, N, D, k, 0, p, p, None) == EINVAL, (N, D, k)
        assert lib.dxmi_knn_radii_workspace_bytes(N, D, k, 0) == 0
    assert lib.dxmi_knn_radii(p, 16, 4, 3, -1, p, p, None) == EINVAL
    assert lib.dxmi_pr_membership(p, 0, p, p, 4, p, 4, p, p, p, None) == EINVAL
    assert lib.dxmi_pr_membership(p, 4, p, p, 4, p, 0, p, p, p, None) == EINVAL
    assert lib.dxmi_pr_membership(p, 4, None, p, 4, p, 4, p, p, p, None) == EINVAL
    assert lib.dxmi_inception_score(p, 4, 8, p, 10, 0, p, p, None) == EINVAL
    assert lib.dxmi_inception_score(p, 4, 8, None, 10, 5, p, p, None) == EINVAL
    # no N x N scratch: the radii workspace is linear in N
    w1, w2 = lib.dxmi_knn_radii_workspace_bytes(50000, 2048, 3, 0), lib.dxmi_knn_radii_workspace_bytes(100000, 2048, 3, 0)
    assert 0 < w1 < 50000 * 400 and w2 < 50000 ** 2


def test_no_gpu_means_loud_failure_for_eval_metrics():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dxmi_hip import DxmiError, ops
    x = torch.rand(16, 8)
    with pytest.raises(DxmiError):
        ops.knn_radii(x, 3)
    with pytest.raises(DxmiError):
        ops.pr_membership(x, torch.zeros(16), x, torch.zeros(16))
    with pytest.raises(DxmiError):
        ops.inception_score(x, torch.rand(4, 8))


# ------------------------------------------------------------------------------------------------ GPU
def _features(N, D, seed, latent=16):
    """pool3-like non-negative features with structure (relu of a low-rank map): distances spread over their own scale."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, latent, generator=g, dtype=torch.float64)
    m = torch.randn(latent, D, generator=g, dtype=torch.float64) / latent ** 0.5
    return torch.relu(z @ m).float()


def _dist64(a, b):
    a, b = a.double(), b.double()
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T).clamp_min(0.0)


def _err_bound(D, na, nb):
    """|d_f32 - d| <= (gamma_D + 2u)(|u|^2 + |v|^2 + 2 sum|u_k v_k|) <= (D + 4) 2^-23 (|u|^2 + |v|^2) for non-negative features
    (fmaf chains of D terms for the dot and the norms, two more roundings; sum u_k v_k <= (|u|^2 + |v|^2) / 2)."""
    return (D + 4) * 2.0 * U * (na[:, None] + nb[None, :])


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 2048, 2023])
@pytest.mark.parametrize("N,k", [(4, 3), (127, 3), (129, 7), (5000, 3)])
def test_radii_vs_fp64(N, D, k):
    from dxmi_hip import ops
    x = _features(N, D, seed=N * 7 + D).cuda()
    got = ops.knn_radii(x, k).double()
    d = _dist64(x, x)
    want = d.kthvalue(k + 1, dim=1).values
    n = (x.double() ** 2).sum(1)
    # the k-th order statistic moves by at most the largest entry error of its row
    bound = _err_bound(D, n, n).max(1).values
    assert (got - want).abs().le(bound).all(), float(((got - want).abs() / bound).max())


@pytest.mark.gpu
def test_radii_independent_of_split_and_workspace():
    from dxmi_hip import _lib, ops
    x = _features(1000, 2023, seed=3).cuda()
    base = ops.knn_radii(x, 3)
    lib = _lib.load()
    for s in (1, 2, 3, 7, 8):
        need = lib.dxmi_knn_radii_workspace_bytes(1000, 2023, 3, s)
        ws = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device="cuda")       # NaN-filled scratch of its own
        assert torch.equal(ops.knn_radii(x, 3, splits=s, workspace=ws), base), s
    assert torch.equal(ops.knn_radii(x, 3), base)                                         # run twice: identical


@pytest.mark.gpu
def test_pr_invariants_bitwise():
    from dxmi_hip import ops
    a, b = _features(700, 2048, seed=11).cuda(), _features(450, 2048, seed=12).cuda()
    ra, rb = ops.knn_radii(a, 3), ops.knn_radii(b, 3)
    # the same set with the same radii: P = R = 1 exactly
    s_in, s_in2 = ops.pr_membership(a, ra, a, ra)
    assert int(s_in.sum()) == 700 and int(s_in2.sum()) == 700
    a_in_b, b_in_a = ops.pr_membership(a, ra, b, rb)
    # precision(A, B) == recall(B, A): swapped arguments give the same flags
    b_in_a2, a_in_b2 = ops.pr_membership(b, rb, a, ra)
    assert torch.equal(a_in_b, a_in_b2) and torch.equal(b_in_a, b_in_a2)
    # permuted rows: permuted radii and flags, same counts
    pa, pb = torch.randperm(700, generator=torch.Generator().manual_seed(1)).cuda(), torch.randperm(450).cuda()
    ra_p, rb_p = ops.knn_radii(a[pa].contiguous(), 3), ops.knn_radii(b[pb].contiguous(), 3)
    assert torch.equal(ra_p, ra[pa]) and torch.equal(rb_p, rb[pb])
    a_in_b_p, b_in_a_p = ops.pr_membership(a[pa].contiguous(), ra_p, b[pb].contiguous(), rb_p)
    assert torch.equal(a_in_b_p, a_in_b[pa]) and torch.equal(b_in_a_p, b_in_a[pb])
    # twice: identical
    again = ops.pr_membership(a, ra, b, rb)
    assert torch.equal(again[0], a_in_b) and torch.equal(again[1], b_in_a)


@pytest.mark.gpu
@pytest.mark.parametrize("NA,NB,D", [(300, 517, 64), (1000, 2500, 2048), (129, 255, 2023)])
def test_membership_vs_fp64_outside_margin(NA, NB, D):
    """Flags equal the fp64 restatement's wherever no pair sits within the a-priori f32 error margin of its threshold."""
    from dxmi_hip import ops
    a, b = _features(NA, D, seed=NA).cuda(), _features(NB, D, seed=NB + 1).cuda()
    ra, rb = ops.knn_radii(a, 3), ops.knn_radii(b, 3)
    a_in_b, b_in_a = ops.pr_membership(a, ra, b, rb)
    d = _dist64(a, b)
    na, nb = (a.double() ** 2).sum(1), (b.double() ** 2).sum(1)
    # every f32 distance and radius carries at most (D + 4) 2^-23 2 max|x|^2 of error: a pair is decided when |d - r| > twice that
    nmax = float(torch.maximum(na.max(), nb.max()))
    margin = 2 * (D + 4) * 2.0 * U * 2 * nmax
    ra64, rb64 = ra.double(), rb.double()
    undecided = 0
    for flags, thr, axis in ((a_in_b, rb64[None, :], 1), (b_in_a, ra64[:, None], 0)):
        sure_in = (d <= thr - margin).any(axis)
        sure_out = (d > thr + margin).all(axis)
        assert flags.bool()[sure_in].all() and not flags.bool()[sure_out].any()
        undecided += int((~sure_in & ~sure_out).sum())
    print(f"NA {NA} NB {NB} D {D}: {undecided} of {NA + NB} flags within the margin")
    assert undecided <= 0.02 * (NA + NB)


@pytest.mark.gpu
def test_golden_through_device(golden):
    from dxmi_hip import ops
    from pytorch_fid.fid_score import activation_statistics, calculate_frechet_distance
    for name in _cases(golden):
        a, b = torch.from_numpy(golden[f"{name}/a"]).cuda(), torch.from_numpy(golden[f"{name}/b"]).cuda()
        k = int(golden[f"{name}/k"])
        ra, rb = ops.knn_radii(a, k), ops.knn_radii(b, k)
        assert np.array_equal(ra.cpu().numpy(), golden[f"{name}/radii_a"]) and np.array_equal(rb.cpu().numpy(), golden[f"{name}/radii_b"])
        a_in_b, b_in_a = ops.pr_membership(a, ra, b, rb)
        assert int(b_in_a.sum()) / len(b_in_a) == float(golden[f"{name}/precision"]), name
        assert int(a_in_b.sum()) / len(a_in_b) == float(golden[f"{name}/recall"]), name
        m1, s1 = activation_statistics(b)
        m2, s2 = activation_statistics(a)
        assert calculate_frechet_distance(m1, s1, m2, s2) == pytest.approx(float(golden[f"{name}/fid"]), rel=1e-5)
    pool, w = torch.from_numpy(golden["is/pool"]).cuda(), torch.from_numpy(golden["is/w"]).cuda()
    assert ops.inception_score(pool, w.t().contiguous()) == pytest.approx(float(golden["is/score"]), rel=1e-5)


@pytest.mark.gpu
def test_inception_score_vs_fp64():
    from dxmi_hip import ops
    g = torch.Generator().manual_seed(9)
    pool = _features(12345, 2048, seed=21)
    w = torch.randn(2048, 1008, generator=g) * 0.02
    got = ops.inception_score(pool.cuda(), w.t().contiguous().cuda())
    want = np_inception_score(pool.numpy(), w.numpy())
    assert got == pytest.approx(want, rel=1e-6)
    assert ops.inception_score(pool.cuda(), w.t().contiguous().cuda()) == got           # bitwise reproducible


@pytest.mark.gpu
def test_sfid_statistics_at_2023_vs_np_cov():
    """The evaluator's sFID path: 2023 features padded to 2024 with one zero column, dxmi_fid_stats, the pad row / column dropped."""
    from pytorch_fid.fid_score import activation_statistics
    x = _features(3000, 2023, seed=5)
    pad = torch.zeros(3000, 2024)
    pad[:, :2023] = x
    mu, sigma = activation_statistics(pad.cuda())
    mu, sigma = mu[:2023], sigma[:2023, :2023]
    x64 = x.double().numpy()
    assert np.allclose(mu, x64.mean(0), rtol=1e-6, atol=1e-7)
    want = np.cov(x64, rowvar=False)
    assert np.linalg.norm(sigma - want) / np.linalg.norm(want) < 1e-5


@pytest.mark.gpu
def test_radii_scale_50000_no_n_squared_memory():
    from dxmi_hip import ops
    N, D = 50000, 2048
    x = _features(N, D, seed=50).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = ops.knn_radii(x, 3)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < N * N * 4 / 100, peak                  # 100 MB against the 10 GB an N x N f32 matrix would take
    rows = torch.arange(0, N, 197, device="cuda")
    d = _dist64(x[rows], x)
    want = d.kthvalue(4, dim=1).values
    n = (x.double() ** 2).sum(1)
    bound = _err_bound(D, n[rows], n).max(1).values
    assert (r[rows].double() - want).abs().le(bound).all()
