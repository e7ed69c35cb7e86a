"""GPU: dxmi_image_batch (csrc/image_batch.hip) and dxmi_hip.data.ImageStore on the device.  The expected values are the reference's
two normalisation expressions over byte values, evaluated on the CPU (dxmi_hip.data.form_batch; tests/test_image_store_host.py holds
them to numpy's `arr.astype(np.float32) / 127.5 - 1` and to ToTensor's `.div(255)`, `2 * x - 1` bit for bit): every comparison here
is torch.equal, there is no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dxmi_hip.data import NORM_ADM, NORM_TOTENSOR, ImageStore, form_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusion-by-maxentirl_amd")
FAST = [(32, 32), (64, 64), (16, 16)]
SCALAR = [(5, 7), (8, 12), (16, 24)]            # W % 16 != 0; 5x7x3 rows start at odd addresses


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def _store(H, W, C, rows=9):
    """uint8 [rows, H, W, C]: arange % 256 xor-mixed with seeded random bytes over the second half, so every byte value occurs."""
    n = rows * H * W * C
    a = (np.arange(n) % 256).astype(np.uint8)
    r = np.random.default_rng(H * 1000 + W * 10 + C).integers(0, 256, n, dtype=np.uint8)
    a[n // 2:] ^= r[n // 2:]
    a[:256] = np.arange(256, dtype=np.uint8)
    return torch.from_numpy(a.reshape(rows, H, W, C))


def _case(B):
    idx = torch.tensor([0, 8, 3, 8, 5, 1, 0][:B] if B > 1 else [8])
    flip = torch.tensor([1, 0, 1, 1, 0, 0, 1][:B], dtype=torch.uint8)
    return idx, flip


@pytest.mark.parametrize("norm", [NORM_ADM, NORM_TOTENSOR])
@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("hw", FAST + SCALAR)
def test_kernel_equals_cpu_expressions(ops, hw, C, B, norm):
    store = _store(*hw, C)
    assert len(np.unique(store.numpy())) == 256
    idx, flip = _case(B)
    sd, idd, fd = store.to(DEV), idx.to(DEV), flip.to(DEV)
    got = ops.image_batch(sd, idd, fd, norm)
    assert got.shape == (B, C) + hw and got.dtype == torch.float32
    assert torch.equal(got.cpu(), form_batch(store[idx], flip, norm))
    assert torch.equal(ops.image_batch(sd, idd, None, norm).cpu(), form_batch(store[idx], None, norm))               # flip = NULL
    assert torch.equal(ops.image_batch(sd, None, fd, norm).cpu(), form_batch(store[:B], flip, norm))                 # idx = NULL


@pytest.mark.parametrize("hw", [(16, 16), (5, 7)])
def test_out_of_range_rows_are_nan(ops, hw):
    store = _store(*hw, 3)
    idx = torch.tensor([2, -1, 4, 9, 8])
    flip = torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8)
    got = ops.image_batch(store.to(DEV), idx.to(DEV), flip.to(DEV), NORM_ADM).cpu()
    assert torch.isnan(got[1]).all() and torch.isnan(got[3]).all()
    good = [0, 2, 4]
    assert torch.equal(got[good], form_batch(store[idx[good]], flip[good], NORM_ADM))


def test_reproducible_and_out_in_place(ops):
    store = _store(32, 32, 3).to(DEV)
    idx, flip = (t.to(DEV) for t in _case(7))
    a = ops.image_batch(store, idx, flip, NORM_TOTENSOR)
    out = torch.full((7, 3, 32, 32), float("nan"), device=DEV)
    ret = ops.image_batch(store, idx, flip, NORM_TOTENSOR, out=out)
    assert ret is out and torch.equal(a, out)


def test_wrapper_refusals(ops):
    from dxmi_hip import DxmiError
    store = _store(16, 16, 3)
    idx, flip = _case(7)
    sd, idd, fd = store.to(DEV), idx.to(DEV), flip.to(DEV)
    with pytest.raises(DxmiError):
        ops.image_batch(store, idx, flip, NORM_ADM)                                  # CPU tensors
    with pytest.raises(AssertionError):
        ops.image_batch(sd, idd.int(), fd, NORM_ADM)                                 # int32 indices
    with pytest.raises(AssertionError):
        ops.image_batch(sd[:, :, ::2], idd, fd, NORM_ADM)                            # non-contiguous store
    with pytest.raises(AssertionError):
        ops.image_batch(sd.float(), idd, fd, NORM_ADM)                               # float store
    with pytest.raises(AssertionError):
        ops.image_batch(sd, idd, fd, NORM_ADM, out=torch.empty(7, 3, 16, 8, device=DEV))      # mismatched out
    with pytest.raises(AssertionError):
        ops.image_batch(sd, idd, fd[:3], NORM_ADM)                                   # idx and flip of different lengths
    with pytest.raises(AssertionError):
        ops.image_batch(sd, idd[:0], None, NORM_ADM)                                 # B = 0
    with pytest.raises(AssertionError):
        ops.image_batch(sd, idd, fd, 2)                                              # unknown norm
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def labelled(tmp_path_factory):
    """41 images of 16 x 16 with labels, and the CPU store's batches of two epochs for world = 2, rank = 1 (computed once)."""
    arr = np.random.default_rng(3).integers(0, 256, (41, 16, 16, 3), dtype=np.uint8)
    lab = np.random.default_rng(4).integers(0, 1000, 41).astype(np.int64)
    p = str(tmp_path_factory.mktemp("store") / "img.npz")
    np.savez(p, arr, lab)
    kw = dict(batch_size=4, rank=1, world=2, seed=11, class_cond=True)
    cpu = ImageStore(p, "cpu", NORM_ADM, **kw)
    want = [list(cpu.epoch(e)) for e in (0, 1)]
    assert len(want[0]) == 5
    return p, kw, want


@pytest.mark.parametrize("resident", ["device", "host"])
def test_store_on_the_device_equals_cpu_store(ops, labelled, resident):
    p, kw, want = labelled
    s = ImageStore(p, DEV, NORM_ADM, resident=resident, **kw)
    assert s.resident == resident
    for e in (0, 1):
        got = list(s.epoch(e))
        assert len(got) == len(want[e])
        for (x, y), (xr, yr) in zip(got, want[e]):
            assert x.is_cuda and y.is_cuda and torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)
    it = s.batches()                                   # the infinite form crosses the epoch boundary with the same batches
    flat = want[0] + want[1]
    for k in range(7):
        x, cond = next(it)
        assert torch.equal(x.cpu(), flat[k][0]) and torch.equal(cond["y"].cpu(), flat[k][1])
    s.close()


def test_real_data_consistency_training_step(ops, labelled, tmp_path):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.train_util import CMTrainLoop
    from test_hip_cm_train import build
    p, kw, want = labelled
    store = ImageStore(p, DEV, NORM_ADM, **kw)
    seen = []

    class Recording(KarrasDenoiser):
        def consistency_losses(self, model, x_start, num_scales, **k):
            seen.append(x_start.detach().cpu().clone())
            return super().consistency_losses(model, x_start, num_scales, **k)

    online = build()
    online.train()
    loop = CMTrainLoop(model=online, target_model=build(None, "target:"), teacher_model=None, teacher_diffusion=None,
                       training_mode="consistency_training", ema_scale_fn=lambda step: (0.9, 6), total_training_steps=2,
                       diffusion=Recording(sigma_data=0.5, weight_schedule="uniform", distillation=True, loss_norm="l2"),
                       data=store.batches(), batch_size=4, microbatch=2, lr=1e-4, ema_rate="0.999,0.9", log_interval=1, save_interval=-1,
                       resume_checkpoint="", use_fp16=True, lr_anneal_steps=2, log_dir=str(tmp_path))
    loop.run_loop()
    assert loop.global_step == 2 and len(seen) == 4                   # two steps of two microbatches, none skipped
    assert loop.logged and np.isfinite(loop.logged[-1]["loss"])
    for k in range(2):
        assert torch.equal(torch.cat(seen[2 * k:2 * k + 2]), want[0][k][0])
    store.close()


def _run(cmd, timeout):
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1", RANK="0")
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable] + cmd, cwd=PKG, env=env, capture_output=True, text=True,
                          timeout=timeout + 60)


def test_cli_cm_train_on_an_array_file(ops, tmp_path):
    arr = np.random.default_rng(5).integers(0, 256, (48, 16, 16, 3), dtype=np.uint8)
    lab = np.random.default_rng(6).integers(0, 1000, 48).astype(np.int64)
    np.savez(tmp_path / "tiny.npz", arr, lab)
    shrunk = dict(image_size=16, num_channels=64, num_res_blocks=1, channel_mult="1,2", attention_resolutions="8", num_head_channels=64,
                  class_cond=True, resblock_updown=True)
    r = _run(["cm_train.py", "--data_npz", str(tmp_path / "tiny.npz"), "--training_mode", "consistency_training", "--max_iters", "2",
              "--batch_size", "4", "--microbatch", "2", "--use_fp16", "True", "--start_scales", "6", "--end_scales", "6",
              "--save_interval", "2", "--log_interval", "1", "--ema_rate", "0.999,0.9", "--log_dir", str(tmp_path / "run")]
             + [a for k, v in shrunk.items() for a in (f"--{k}", str(v))], 600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"data: {tmp_path / 'tiny.npz'}: 48 images 16x16x3, labels yes, resident device, 12 batches of 4 per epoch" in r.stdout, r.stdout
    assert "target_model000002.pt" in os.listdir(tmp_path / "run")


def test_cli_train_cifar10_on_an_array_file(ops, tmp_path):
    arr = np.random.default_rng(7).integers(0, 256, (40, 32, 32, 3), dtype=np.uint8)
    np.savez(tmp_path / "tiny32.npz", arr)
    r = _run(["train_cifar10.py", "--config", "builtin:cifar10_T10", "--dataset", "builtin", "--run", "t", "--data_npz",
              str(tmp_path / "tiny32.npz"), "--max_iters", "3", "--training.batchsize", "8"], 600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"data: {tmp_path / 'tiny32.npz'}: 40 images 32x32x3, labels no, resident device, 5 batches of 8 per epoch" in r.stdout, r.stdout
