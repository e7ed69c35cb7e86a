"""evaluations/evaluator.py: the ADM evaluator's command line on the device.  CPU: argument parsing, the streaming .npz reader
against np.load, precomputed statistics, shape / dtype errors, loud failure without a GPU.  -m gpu: the CLI end to end on two
small generated batches with the weight-free stub extractor (tests/eval_extractor_stub.py), all five printed numbers against a
numpy restatement of the whole flow."""
import os
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


def _images(n, seed, hw=16):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(n, 4, 4, 3))
    noise = rng.integers(-20, 21, size=(n, hw, hw, 3))
    return np.clip(np.repeat(np.repeat(base, hw // 4, 1), hw // 4, 2) + noise, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ CPU
def test_parse_args():
    a = ev.parse_args(["ref.npz", "sample.npz"])
    assert (a.ref_batch, a.sample_batch, a.batch_size, a.extractor) == ("ref.npz", "sample.npz", 64, "pytorch_fid.inception:EvalInceptionV3")
    a = ev.parse_args(["r.npz", "s.npz", "--batch_size", "7", "--extractor", "m:attr"])
    assert (a.batch_size, a.extractor) == (7, "m:attr")
    with pytest.raises(SystemExit):
        ev.parse_args(["only_one.npz"])
    with pytest.raises(SystemExit):
        ev.parse_args(["r.npz", "s.npz", "--batch_size", "0"])


@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("bs", [1, 7, 64, 1000])
def test_streaming_reader_equals_np_load(tmp_path, compressed, bs):
    x = _images(53, seed=1)
    path = str(tmp_path / "b.npz")
    (np.savez_compressed if compressed else np.savez)(path, x, extra=np.arange(3))
    with ev.open_npz_array(path) as r:
        assert r.arr is None and len(r) == 53 and r.dtype == np.uint8
        parts = list(r.batches(bs))
    assert all(len(p) == min(bs, 53 - i * bs) for i, p in enumerate(parts))
    assert np.array_equal(np.concatenate(parts), np.load(path)["arr_0"])


def test_fortran_order_falls_back_to_np_load(tmp_path):
    x = np.asfortranarray(_images(9, seed=2))
    path = str(tmp_path / "f.npz")
    np.savez(path, x)
    with ev.open_npz_array(path) as r:
        assert np.array_equal(np.concatenate(list(r.batches(4))), x)


def test_precomputed_statistics(tmp_path):
    p = str(tmp_path / "ref.npz")
    mu, sigma = np.arange(4.0), np.eye(4)
    np.savez(p, _images(8, seed=3), mu=mu, sigma=sigma, mu_s=mu[:2], sigma_s=np.eye(2))
    got = ev.read_precomputed_statistics(p)
    assert [g.dtype for g in got] == [np.float64] * 4
    assert np.array_equal(got[0], mu) and np.array_equal(got[1], sigma) and got[3].shape == (2, 2)
    np.savez(p, _images(8, seed=3))
    assert ev.read_precomputed_statistics(p) is None
    np.savez(p, _images(8, seed=3), mu=mu, sigma=sigma)
    with pytest.raises(ValueError, match="mu_s"):
        ev.read_precomputed_statistics(p)


@pytest.mark.parametrize("arr,msg", [
    (np.zeros((8, 16, 16, 3), np.float32), "uint8"),
    (np.zeros((8, 16, 16), np.uint8), "NHWC"),
    (np.zeros((8, 16, 16, 4), np.uint8), "NHWC"),
    (np.zeros((3, 16, 16, 3), np.uint8), "at least 4"),
])
def test_shape_and_dtype_errors(tmp_path, arr, msg):
    p = str(tmp_path / "bad.npz")
    np.savez(p, arr)
    with ev.open_npz_array(p) as r:
        with pytest.raises(ValueError, match=msg):
            ev.check_image_batch(r)


def test_missing_arr_0(tmp_path):
    p = str(tmp_path / "none.npz")
    np.savez(p, images=np.zeros((4, 2, 2, 3), np.uint8))
    with pytest.raises(ValueError, match="arr_0"):
        with ev.open_npz_array(p):
            pass


def test_no_gpu_means_loud_failure_for_evaluator(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dxmi_hip import DxmiError
    from eval_extractor_stub import PoolSpatialFeatures
    p = str(tmp_path / "b.npz")
    np.savez(p, _images(8, seed=4))
    with pytest.raises(DxmiError):
        ev.evaluate(p, p, PoolSpatialFeatures(), 4)


def test_default_extractor_needs_its_weight_file(monkeypatch):
    from dxmi_hip import DxmiError
    from pytorch_fid.inception import EvalInceptionV3
    monkeypatch.delenv("DXMI_FID_WEIGHTS", raising=False)
    with pytest.raises(DxmiError, match="DXMI_FID_WEIGHTS"):
        EvalInceptionV3()


# ------------------------------------------------------------------------------------------------ GPU
def _np_flow(ref, sample, extractor, k=3):
    """The whole evaluator flow restated in numpy / fp64 on the stub's features (computed on the host)."""
    from pytorch_fid.fid_score import calculate_frechet_distance
    from test_eval_metrics import np_distances, np_inception_score, np_radii

    def feats(x):
        p, s = extractor(torch.from_numpy(x))
        return p.double().numpy(), s.double().numpy()
    (rp, rs), (sp, ss) = feats(ref), feats(sample)
    w = extractor.softmax_weight.double().cpu().numpy()
    stats = lambda a: (a.mean(0), np.cov(a, rowvar=False))
    fid = calculate_frechet_distance(*stats(sp), *stats(rp))
    sfid = calculate_frechet_distance(*stats(ss), *stats(rs))
    ra, rb = np_radii(rp, k), np_radii(sp, k)
    d = np_distances(rp, sp)
    return np_inception_score(sp, w), fid, sfid, (d <= ra[:, None]).any(0).mean(), (d <= rb[None, :]).any(1).mean()


@pytest.mark.gpu
def test_cli_end_to_end_with_stub_extractor(tmp_path):
    from eval_extractor_stub import PoolSpatialFeatures
    ref, sample = _images(90, seed=10), _images(70, seed=11)
    rp, sp = str(tmp_path / "ref.npz"), str(tmp_path / "sample.npz")
    np.savez(rp, ref)
    np.savez_compressed(sp, sample)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([TESTS, PKG, ROOT]))
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluations", "evaluator.py"), rp, sp, "--extractor",
                        "eval_extractor_stub:PoolSpatialFeatures", "--batch_size", "16"], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.split(":")[0] in ("Inception Score", "FID", "sFID", "Precision", "Recall")]
    assert [l.split(":")[0] for l in lines] == ["Inception Score", "FID", "sFID", "Precision", "Recall"], r.stdout
    assert "unpinned" in r.stdout
    got = [float(l.split(":", 1)[1]) for l in lines]
    want = _np_flow(ref, sample, PoolSpatialFeatures())
    print("cli:", got, "numpy:", want)
    assert got[0] == pytest.approx(want[0], rel=1e-5)
    assert got[1] == pytest.approx(want[1], rel=1e-4, abs=1e-6)
    assert got[2] == pytest.approx(want[2], rel=1e-4, abs=1e-6)
    # flags near a threshold may flip between f32 and fp64: at most one sample / reference image
    assert abs(got[3] - want[3]) <= 1.0 / 70 + 1e-12 and abs(got[4] - want[4]) <= 1.0 / 90 + 1e-12


@pytest.mark.gpu
def test_precomputed_reference_statistics_are_used(tmp_path, capsys):
    from eval_extractor_stub import PoolSpatialFeatures
    ref, sample = _images(90, seed=12), _images(80, seed=13)
    ext = PoolSpatialFeatures()
    rp, sp = str(tmp_path / "ref.npz"), str(tmp_path / "sample.npz")
    np.savez(sp, sample)
    np.savez(rp, ref)
    plain = ev.evaluate(rp, sp, ext, 8)
    # statistics stored with the batch replace the computed ones (here: the sample's own, so FID = sFID = 0 up to rounding)
    s_pool, s_spatial, S = ev.read_activations(sp, ext, 8)
    mu, sigma, mu_s, sigma_s = ev.statistics(sp, s_pool, s_spatial, S)
    np.savez(rp, ref, mu=mu, sigma=sigma, mu_s=mu_s, sigma_s=sigma_s)
    pre = ev.evaluate(rp, sp, ext, 8)
    assert pre[0] == plain[0] and pre[3:] == plain[3:]                 # IS and P / R still come from the images
    assert abs(pre[1]) < 1e-4 and abs(pre[2]) < 1e-4
