"""Host side of the EDM DSM training: the torch restatement of KarrasDenoiser.training_losses / get_weightings against the
reference's values (tests/golden/edm_dsm.npz, make_golden_dsm.py), the CPU update_ema loop, the noise-level sampler and the
TrainLoop helpers.  No GPU."""
import os

import numpy as np
import pytest
import torch

SCHEDULES = ("snr", "snr+1", "karras", "truncated-snr", "uniform")


def analytic(x_in, t, **kw):
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "edm_dsm.npz"), allow_pickle=False)


@pytest.mark.parametrize("ws", SCHEDULES)
def test_training_losses_torch_path_vs_reference(g, ws):
    from models.cm.karras_diffusion import KarrasDenoiser
    d = KarrasDenoiser(sigma_data=0.5, weight_schedule=ws)
    t = d.training_losses(analytic, torch.from_numpy(g["x_start"]), torch.from_numpy(g["sigmas"]), noise=torch.from_numpy(g["noise"]))
    assert set(t) == {"xs_mse", "mse", "loss"} and t["loss"] is t["mse"]
    np.testing.assert_allclose(t["xs_mse"].numpy(), g[f"analytic.{ws}.xs_mse"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(t["mse"].numpy(), g[f"analytic.{ws}.mse"], rtol=1e-6, atol=0)


def test_training_losses_distillation_scalings(g):
    from models.cm.karras_diffusion import KarrasDenoiser
    d = KarrasDenoiser(sigma_data=0.5, weight_schedule="karras", distillation=True)
    t = d.training_losses(analytic, torch.from_numpy(g["x_start"]), torch.from_numpy(g["sigmas"]), noise=torch.from_numpy(g["noise"]))
    np.testing.assert_allclose(t["xs_mse"].numpy(), g["analytic_distill.karras.xs_mse"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(t["mse"].numpy(), g["analytic_distill.karras.mse"], rtol=1e-6, atol=0)


def test_get_weightings():
    from models.cm.karras_diffusion import get_weightings
    s = torch.tensor([0.002, 0.5, 1.0, 3.0])
    snr = s ** -2
    assert torch.equal(get_weightings("snr", snr, 0.5), snr)
    assert torch.equal(get_weightings("snr+1", snr, 0.5), snr + 1)
    assert torch.equal(get_weightings("karras", snr, 0.5), snr + 4.0)
    assert torch.equal(get_weightings("truncated-snr", snr, 0.5), torch.clamp(snr, min=1.0))
    assert torch.equal(get_weightings("uniform", snr, 0.5), torch.ones(4))
    with pytest.raises(NotImplementedError):
        get_weightings("lpips", snr, 0.5)


def test_update_ema_cpu_loop_vs_reference(g):
    from models.cm.nn import update_ema
    for k, rate in enumerate(g["ema.rates"]):
        tgt = [torch.from_numpy(g[f"ema.{k}.before.{i}"]).clone() for i in range(4)]
        for it in range(3):
            update_ema(tgt, [torch.from_numpy(g[f"ema.src.{it}.{i}"]) for i in range(4)], rate=float(rate))
        for i in range(4):
            assert torch.equal(tgt[i], torch.from_numpy(g[f"ema.{k}.after.{i}"]))


def test_lognormal_sampler():
    from models.cm.resample import LogNormalSampler
    s, w = LogNormalSampler(generator=torch.Generator().manual_seed(0)).sample(20000, "cpu")
    assert s.shape == (20000,) and s.dtype == torch.float32 and torch.equal(w, torch.ones(20000))
    ls = s.log()
    assert abs(ls.mean().item() + 1.2) < 0.05 and abs(ls.std().item() - 1.2) < 0.05


def test_trainloop_helpers():
    from models.cm.train_util import TrainLoop, parse_resume_step_from_filename
    assert parse_resume_step_from_filename("/a/b/model000123.pt") == 123
    assert parse_resume_step_from_filename("/a/b/ema_0.999_000123.pt") == 0
    with pytest.raises(ValueError):
        TrainLoop(model=torch.nn.Linear(2, 2), diffusion=None, data=None, batch_size=1, microbatch=-1, lr=1e-4, ema_rate="0.999",
                  log_interval=1, save_interval=1, resume_checkpoint="")


def test_ema_update_validates_the_whole_list_before_launching():
    """A null EMA tensor past the first DXMI_MT_MAX-tensor launch is refused before anything is launched (no GPU needed: the
    validation is host code, and no launch is reached)."""
    import ctypes
    from dxmi_hip import _lib
    if torch.cuda.is_available():
        pytest.skip("host-only check with placeholder pointers: CPU boxes only")
    lib = _lib.load()
    n = 70
    src = (ctypes.c_void_p * n)(*[0x1000 * (i + 1) for i in range(n)])
    ema = (ctypes.c_void_p * n)(*[0x100000 + 0x1000 * i if i != 66 else 0 for i in range(n)])
    numel = (ctypes.c_int64 * n)(*([8] * n))
    rates = (ctypes.c_double * 1)(0.999)
    assert lib.dxmi_ema_update(ema, src, numel, n, 1, rates, None, None) != 0
    msg = lib.dxmi_last_error().decode()
    assert "null EMA tensor" in msg and "tensor 66" in msg, msg
