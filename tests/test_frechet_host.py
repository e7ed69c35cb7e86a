"""The Frechet distance on the device, the parts that need no GPU: the numpy float64 model of the two-stage
Newton-Schulz iteration (tests/frechet_model.py) against the host `calculate_frechet_distance`, the new command-line flags, the
refusals without a GPU, and the argument checks of csrc/frechet.hip's entry points under the host sanitizers (a stand-alone
program, run as a child process).

Bound of the model against the host function: |diff| <= 1e-7 * (tr S1 + tr S2).  Measured when this test was written (16 threads):
d2048 -4.9e-10, d64 -6.0e-10, d192_singular +1.2e-8 of the traces; the factor covers another BLAS summation order."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from frechet_model import frechet_distance_model  # noqa: E402
from oracle import fid as ofid  # noqa: E402


def case_statistics(name):
    _, dims, n1, n2, s1, s2, scale2, shift2 = next(c for c in ofid.CASES if c[0] == name)
    a1, a2 = ofid.synthetic_activations(s1, n1, dims), ofid.synthetic_activations(s2, n2, dims, scale=scale2, shift=shift2)
    return ofid.activation_statistics(a1) + ofid.activation_statistics(a2)


@pytest.mark.parametrize("name", [c[0] for c in ofid.CASES])
def test_model_matches_the_host_distance(golden_dir, name):
    from pytorch_fid.fid_score import calculate_frechet_distance
    golden = np.load(os.path.join(golden_dir, "fid_stats.npz"))
    m1, c1, m2, c2 = case_statistics(name)
    assert np.array_equal(m1, golden[f"{name}_mu1"]) and np.isclose(np.trace(c1), golden[f"{name}_trace1"], rtol=1e-13)
    want = float(calculate_frechet_distance(m1, c1, m2, c2))
    got, (k1, k2), converged = frechet_distance_model(m1, c1, m2, c2)
    traces = float(np.trace(c1) + np.trace(c2))
    print(f"{name}: model {got:.12f} host {want:.12f} diff {got - want:.3e} = {(got - want) / traces:.3e} of the traces, "
          f"iterations {k1} + {k2}")
    assert converged and 1 <= k1 <= 100 and 1 <= k2 <= 100
    assert abs(got - want) <= 1e-7 * traces
    assert abs(want - float(golden[f"{name}_fid"])) <= 1e-9 * float(golden[f"{name}_fid"])


def test_model_on_identical_distributions(golden_dir):
    g = np.load(os.path.join(golden_dir, "fid_stats.npz"))
    got, _, converged = frechet_distance_model(g["d64_mu1"], g["d64_sigma1"], g["d64_mu1"], g["d64_sigma1"])
    assert converged and abs(got) < 1e-6


def test_model_ends_on_a_non_finite_input():
    s = np.eye(16)
    s[3, 5] = float("nan")
    got, (k1, k2), converged = frechet_distance_model(np.zeros(16), s, np.zeros(16), np.eye(16))
    assert not converged and (k1, k2) == (1, 0) and got != got


def test_parse_args_accepts_the_fid_flags():
    import train_cifar10
    import train_image_large
    base = ["--config", "builtin:cifar10_T10", "--dataset", "builtin"]
    args, unknown = train_cifar10.parse_args(base)
    assert (args.fid_extractor, args.fid_stats, args.fid_dims, args.fid_distance) == (None, None, 2048, "device") and unknown == []
    args, unknown = train_cifar10.parse_args(base + ["--fid_extractor", "fid_extractor_stub:PatchFeatures", "--fid_stats", "s.npz", "--fid_dims",
                                                     "16", "--fid_distance", "host", "--training.fid_every", "2"])
    assert (args.fid_extractor, args.fid_stats, args.fid_dims, args.fid_distance) == ("fid_extractor_stub:PatchFeatures", "s.npz", 16, "host")
    assert unknown == ["--training.fid_every", "2"]
    with pytest.raises(SystemExit):
        train_cifar10.parse_args(base + ["--fid_distance", "scipy"])
    large = ["--config", "builtin:imagenet64_T10", "--dataset", "builtin", "--run", "r"]
    assert train_image_large.parse_args(large)[0].fid_distance == "host"              # unchanged behaviour by default
    assert train_image_large.parse_args(large + ["--fid_distance", "device"])[0].fid_distance == "device"


def test_fid_every_and_fid_epoch_exclude_each_other():
    import train_cifar10
    load = lambda over: train_cifar10.load_config("builtin:cifar10_T10", "builtin", {"training": over})
    assert train_cifar10.check_fid_schedule(load({})) == (None, 1)                     # the built-in config: every epoch
    assert train_cifar10.check_fid_schedule(load({"fid_every": 2, "fid_epoch": None})) == (2, None)
    assert train_cifar10.check_fid_schedule(load({"fid_epoch": None})) == (None, None)
    with pytest.raises(ValueError, match="cannot set both fid_epoch and fid_every"):
        train_cifar10.check_fid_schedule(load({"fid_every": 100}))


def test_no_gpu_means_loud_failure_for_the_device_distance(golden_dir):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dxmi_hip import DxmiError, ops
    from pytorch_fid.fid_score import calculate_frechet_distance_device, fid_from_images
    g = np.load(os.path.join(golden_dir, "fid_stats.npz"))
    with pytest.raises(DxmiError):
        calculate_frechet_distance_device(g["d64_mu1"], g["d64_sigma1"], g["d64_mu2"], g["d64_sigma2"])
    with pytest.raises(DxmiError):
        ops.gemm_f64(torch.eye(16, dtype=torch.float64), torch.eye(16, dtype=torch.float64))
    with pytest.raises(DxmiError):
        ops.frechet_trace_sqrt(torch.eye(16, dtype=torch.float64), torch.eye(16, dtype=torch.float64))
    with pytest.raises(ValueError, match="distance"):
        fid_from_images(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), None, None, None, distance="gpu")


def test_frechet_workspace_plan_is_host_side():
    from dxmi_hip import _lib
    lib = _lib.load()
    assert lib.dxmi_frechet_workspace_bytes(2048) >= 256 * 8 and lib.dxmi_frechet_workspace_bytes(16) > 0
    assert [lib.dxmi_frechet_workspace_bytes(n) for n in (0, -16, 24, 4112)] == [0, 0, 0, 0]


def test_frechet_arguments_under_address_and_ub_sanitizers():
    """`make asan_frechet` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_frechet.c, a program with its own main, against it and a no-device HIP runtime stub.  Null pointers,
    n % 16 != 0, n <= 0, n > 4096, aliased and misaligned matrices must each come back as DXMI_EINVAL with the message of their
    check: no crash, no sanitizer report.  The program runs as a child process; nothing is loaded into python.  A host-only build:
    machines without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_frechet"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_frechet")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") >= 80
