"""The Frechet distance on the device (csrc/frechet.hip) on the GPU: dxmi_gemm_f64 element by element against numpy
float64, ops.frechet_trace_sqrt / calculate_frechet_distance_device against the HOST calculate_frechet_distance on the same
float64 statistics, the golden d2048 case, the fallback to the host, fid_from_images(distance="device") and train_cifar10.py's
in-training FID from the command line.

Bounds.  GEMM: the classical one, |err_ij| <= 2 n 2^-53 (|alpha| |A| |B|)_ij + 2^-52 |C_ij| (n products and n - 1 additions of
relative error 2^-53 each in the kernel and again in the numpy reference, one rounding of the scale-and-add).  Distance:
1e-7 (tr S1 + tr S2), the bound of the CPU model against the same host function (tests/test_frechet_host.py, measured <= 1.2e-8)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
PKG = os.path.join(ROOT, "diffusion-by-maxentirl_amd")
sys.path.insert(0, TESTS)
from frechet_model import frechet_trace_sqrt_model  # noqa: E402
from oracle import fid as ofid  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(64, 301, 257), (80, 400, 333), (192, 800, 777)]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "fid_stats.npz"))


@pytest.fixture(scope="module")
def shape_statistics():
    """(mu1, sigma1, mu2, sigma2, host distance, model iterations) per shape, computed once."""
    from pytorch_fid.fid_score import calculate_frechet_distance
    out = {}
    for D, n1, n2 in SHAPES:
        a1 = ofid.synthetic_activations(101, n1, D)
        a2 = ofid.synthetic_activations(102, n2, D, scale=1.1, shift=0.05)
        m1, c1 = ofid.activation_statistics(a1)
        m2, c2 = ofid.activation_statistics(a2)
        m1, m2 = m1.astype(np.float64), m2.astype(np.float64)          # the same float64 statistics for both functions
        _, its, ok = frechet_trace_sqrt_model(c1, c2)
        assert ok
        out[D] = (m1, c1, m2, c2, float(calculate_frechet_distance(m1, c1, m2, c2)), its)
    return out


def case_statistics(name):
    _, dims, n1, n2, s1, s2, scale2, shift2 = next(c for c in ofid.CASES if c[0] == name)
    a1, a2 = ofid.synthetic_activations(s1, n1, dims), ofid.synthetic_activations(s2, n2, dims, scale=scale2, shift=shift2)
    return ofid.activation_statistics(a1) + ofid.activation_statistics(a2)


# ------------------------------------------------------------------------------------------ the GEMM
@pytest.mark.parametrize("alpha,diag", [(1.0, 0.0), (-0.5, 1.5)])
@pytest.mark.parametrize("n", [16, 64, 80, 192])
def test_gemm_f64_against_numpy(n, alpha, diag):
    """One MFMA tile, one full wave tile, a ragged edge of it, two workgroup tiles with a ragged edge (24 K chunks)."""
    from dxmi_hip import ops
    rs = np.random.RandomState(1000 + n)
    A, B = rs.uniform(-0.5, 1.0, (n, n)), rs.uniform(-0.5, 1.0, (n, n))        # mean 0.25: the trace is no cancellation
    want = alpha * (A @ B) + diag * np.eye(n)
    a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    tr = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    c = ops.gemm_f64(a, b, alpha, diag, trace=tr)
    got = c.cpu().numpy()
    bound = 2 * n * 2.0 ** -53 * (abs(alpha) * (np.abs(A) @ np.abs(B))) + 2.0 ** -52 * np.abs(want)
    err = np.abs(got - want)
    print(f"n {n} alpha {alpha} diag {diag}: worst |err| / bound {np.max(err / bound):.3f}, worst |err| {err.max():.3e}")
    assert np.isfinite(got).all() and (err <= bound).all()
    t_got, t_want = float(tr.item()), float(np.trace(got))
    print(f"trace {t_got!r} vs np.trace {t_want!r}: relative {abs(t_got - t_want) / abs(t_want):.2e}")
    assert abs(t_got - t_want) <= 1e-14 * abs(t_want)
    # fixed-order reductions, no atomics: the second call is bitwise the first (into another buffer, with other stale contents)
    tr2 = torch.zeros(1, dtype=torch.float64, device="cuda")
    c2 = ops.gemm_f64(a, b, alpha, diag, out=torch.full_like(c, 7.0), trace=tr2)
    assert torch.equal(c2, c) and torch.equal(tr2, tr)


def test_gemm_f64_propagates_non_finite_values_and_refuses_bad_arguments():
    from dxmi_hip import DxmiError, ops
    a = torch.eye(32, dtype=torch.float64, device="cuda")
    b = torch.ones(32, 32, dtype=torch.float64, device="cuda")
    b[5, 7], b[9, 2] = float("nan"), float("inf")
    c = ops.gemm_f64(a, b).cpu()
    # I @ b as arithmetic: 0 * NaN and 0 * inf are NaN, so column 7 is NaN and column 2 is NaN around its one inf
    assert torch.isnan(c[:, 7]).all() and c[9, 2] == float("inf") and torch.isnan(c[:, 2]).sum() == 31
    assert torch.isfinite(c).sum() == 32 * 30 and (c[:, [0, 1, 3, 31]] == 1.0).all()
    with pytest.raises(DxmiError, match="alias"):
        ops.gemm_f64(a, b, out=a)
    with pytest.raises(DxmiError, match="multiple of 16"):
        ops.gemm_f64(torch.eye(24, dtype=torch.float64, device="cuda"), torch.eye(24, dtype=torch.float64, device="cuda"))
    x = torch.arange(256.0, dtype=torch.float64, device="cuda").reshape(16, 16).contiguous()
    want = 0.5 * (x + x.T)
    assert float(ops.frob_norm_f64(x).item()) == pytest.approx(float(x.norm().item()), rel=1e-14)
    assert torch.equal(ops.scale_f64(x, 0.25), 0.25 * x)
    assert torch.equal(ops.symmetrize_f64(x), want)


# ------------------------------------------------------------------------------------------ the distance
@pytest.mark.parametrize("D", [s[0] for s in SHAPES])
def test_device_distance_against_the_host_function(shape_statistics, D):
    from dxmi_hip import ops
    from pytorch_fid import fid_score
    m1, c1, m2, c2, want, model_its = shape_statistics[D]
    traces = float(np.trace(c1) + np.trace(c2))
    d1, d2 = torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda()
    tr, its, converged = ops.frechet_trace_sqrt(d1, d2)
    via_trace = float((m1 - m2).astype(np.float64) @ (m1 - m2).astype(np.float64) + np.trace(c1) + np.trace(c2) - 2 * tr)
    fid_score.last_distance_info.update(path=None, iterations=(0, 0))
    got = float(fid_score.calculate_frechet_distance_device(m1, c1, m2, c2))
    info = dict(fid_score.last_distance_info)
    print(f"D {D}: device {got:.12f} host {want:.12f} diff {got - want:.3e} = {(got - want) / traces:.3e} of the traces; "
          f"iterations {its} (model {model_its}), path {info['path']}")
    assert converged and info["path"] == "device" and info["iterations"] == its
    assert abs(its[0] - model_its[0]) <= 2 and abs(its[1] - model_its[1]) <= 2
    assert abs(via_trace - want) <= 1e-7 * traces
    assert abs(got - want) <= 1e-7 * traces
    # the statistics may already be on the device; the call is reproducible to the bit
    again = float(fid_score.calculate_frechet_distance_device(torch.from_numpy(m1).cuda(), d1, torch.from_numpy(m2), d2))
    assert again == got
    assert torch.equal(d1.cpu(), torch.from_numpy(c1)) and torch.equal(d2.cpu(), torch.from_numpy(c2))       # inputs untouched


def test_golden_d2048_on_the_device(golden):
    from pytorch_fid import fid_score
    m1, c1, m2, c2 = case_statistics("d2048")
    fid_score.last_distance_info.update(path=None, iterations=(0, 0))
    got = float(fid_score.calculate_frechet_distance_device(m1, c1, m2, c2))
    want = float(golden["d2048_fid"])
    print(f"d2048: device {got:.9f} golden {want:.9f} rel {abs(got - want) / want:.2e}, {fid_score.last_distance_info}")
    assert fid_score.last_distance_info["path"] == "device"
    assert abs(got - want) <= 1e-6 * want


def test_identical_distributions(golden):
    from pytorch_fid import fid_score
    m, s = golden["d64_mu1"], golden["d64_sigma1"]
    got = float(fid_score.calculate_frechet_distance_device(m, s, m, s))
    print(f"identical distributions: {got:.3e}, {fid_score.last_distance_info}")
    assert abs(got) < 1e-6


def test_singular_covariances_and_a_nan_entry(golden):
    from pytorch_fid import fid_score
    m1, c1, m2, c2 = case_statistics("d192_singular")
    got = float(fid_score.calculate_frechet_distance_device(m1, c1, m2, c2))
    want = float(golden["d192_singular_fid"])
    print(f"d192_singular: {got:.9f} golden {want:.9f} rel {abs(got - want) / want:.2e}, {fid_score.last_distance_info}")
    assert abs(got - want) <= 1e-6 * want                    # whichever path ran
    bad = c1.copy()
    bad[3, 5] = float("nan")
    fid_score.last_distance_info.update(path=None, iterations=(0, 0))
    try:
        value = fid_score.calculate_frechet_distance_device(m1, bad, m2, c2)
        print(f"NaN entry: the host path returned {value}")
    except (ValueError, np.linalg.LinAlgError) as e:         # the host function's own refusal of a non-finite matrix
        print(f"NaN entry: the host path raised {type(e).__name__}: {e}")
    assert fid_score.last_distance_info["path"] == "host" and fid_score.last_distance_info["iterations"] == (1, 0)


# ------------------------------------------------------------------------------------------ end to end
def test_fid_from_images_on_the_device_against_the_host():
    from fid_extractor_stub import PatchFeatures
    from pytorch_fid import fid_score
    rs = np.random.RandomState(7)
    images = torch.from_numpy(rs.randint(0, 256, (600, 3, 32, 32)).astype(np.uint8)).cuda()
    m2, s2 = ofid.activation_statistics((rs.random_sample((500, 16)) * 0.5 + 0.2).astype(np.float32))
    ext = PatchFeatures()
    host = fid_score.fid_from_images(images, ext, m2, s2, batch_size=50, dims=16, device="cuda")
    assert host == fid_score.fid_from_images(images, ext, m2, s2, batch_size=50, dims=16, device="cuda", distance="host")
    fid_score.last_distance_info.update(path=None, iterations=(0, 0))
    dev = fid_score.fid_from_images(images, ext, m2, s2, batch_size=50, dims=16, device="cuda", distance="device")
    act = fid_score.get_activations_from_tensor((images / 255.0).float(), ext, batch_size=50, dims=16, device="cuda")
    mu_h, sigma_h = fid_score.activation_statistics(act)
    mu_d, sigma_d = fid_score.activation_statistics(act, keep_on_device=True)
    assert mu_d.is_cuda and sigma_d.is_cuda and sigma_d.dtype == torch.float64
    assert np.array_equal(mu_d.cpu().numpy(), mu_h) and np.array_equal(sigma_d.cpu().numpy(), sigma_h)
    traces = float(np.trace(sigma_h) + np.trace(s2))
    print(f"fid_from_images: device {dev:.12f} host {host:.12f} diff {(dev - host) / traces:.3e} of the traces, {fid_score.last_distance_info}")
    assert fid_score.last_distance_info["path"] == "device"
    assert abs(dev - host) <= 1e-7 * traces


def test_cli_train_cifar10_with_fid(tmp_path):
    """train_cifar10.py with the in-training FID: evaluations at iterations 0 and 2, the best sampler kept as sampler.pth /
    value.pth, sampler_last.pth as before; without the two flags no sampler.pth."""
    import re
    import shutil
    stats = str(tmp_path / "stats.npz")
    rs = np.random.RandomState(3)
    m2, s2 = ofid.activation_statistics((rs.random_sample((200, 16)) * 0.5 + 0.2).astype(np.float32))
    np.savez(stats, mu=m2, sigma=s2)
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1", PWD=PKG, PYTHONPATH=TESTS + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "train_cifar10.py", "--config", "builtin:cifar10_T10", "--dataset", "builtin", "--synthetic_data", "--max_iters", "3"]
    sched = ["--training.fid_every", "2", "--training.fid_epoch", "null", "--training.n_fid_samples", "200", "--training.sampling_batchsize",
             "100"]
    fid_flags = ["--fid_extractor", "fid_extractor_stub:PatchFeatures", "--fid_stats", stats, "--fid_dims", "16"]
    try:
        r = subprocess.run(base + ["--run", "frechet_fid"] + fid_flags + sched, cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        logdir = os.path.join(PKG, "results", "cifar10", "cifar10_T10", "frechet_fid")
        scores = [float(v) for v in re.findall(r"FID score: ([-0-9.e+naif]+)", r.stdout)]
        print(r.stdout[-1500:])
        assert len(scores) == 2 and all(np.isfinite(scores))                       # iterations 0 and 2
        assert "did not converge" not in r.stdout                                 # --fid_distance device is the default, and it ran
        best = torch.load(os.path.join(logdir, "sampler.pth"), map_location="cpu")
        assert sorted(best) == ["epoch", "fid", "iter", "state_dict"] and np.isfinite(best["fid"]) and best["fid"] == min(scores)
        assert best["iter"] in (0, 2) and best["epoch"] == 0 and "log_betas" in best["state_dict"]
        assert r.stdout.count("best FID: sampler saved at") == (2 if scores[1] < scores[0] else 1)
        assert "state_dict" in torch.load(os.path.join(logdir, "value.pth"), map_location="cpu")
        last = torch.load(os.path.join(logdir, "sampler_last.pth"), map_location="cpu")
        assert last["iter"] == 3 and last["fid"] is None and len(last["state_dict"]) == len(best["state_dict"])
        r = subprocess.run(base + ["--run", "frechet_nofid"] + sched, cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        logdir = os.path.join(PKG, "results", "cifar10", "cifar10_T10", "frechet_nofid")
        assert os.path.exists(os.path.join(logdir, "sampler_last.pth")) and not os.path.exists(os.path.join(logdir, "sampler.pth"))
        assert "FID score" not in r.stdout
    finally:
        for run in ("frechet_fid", "frechet_nofid"):
            shutil.rmtree(os.path.join(PKG, "results", "cifar10", "cifar10_T10", run), ignore_errors=True)
