"""Host side of consistency distillation / consistency training: the torch path of KarrasDenoiser.consistency_losses against the
reference's values (tests/golden/cm_train.npz, make_golden_cd.py), the time-level table, create_ema_and_scales_fn, and
CMTrainLoop's bookkeeping (target EMA, counters, save / resume) on a small nn.Module.  No GPU."""
import os

import numpy as np
import pytest
import torch

NORMS = ("l1", "l2", "l2-32")
MODES = ("cd", "ct")
EMA_PAIRS = {"fixed_fixed": dict(target_ema_mode="fixed", start_ema=0.95, scale_mode="fixed", start_scales=40, end_scales=40),
             "fixed_progressive": dict(target_ema_mode="fixed", start_ema=0.9, scale_mode="progressive", start_scales=2, end_scales=150),
             "adaptive_progressive": dict(target_ema_mode="adaptive", start_ema=0.95, scale_mode="progressive", start_scales=2,
                                          end_scales=150),
             "fixed_progdist": dict(target_ema_mode="fixed", start_ema=0.0, scale_mode="progdist", start_scales=16, end_scales=16)}


def online_fn(x_in, t, **kw):
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


def target_fn(x_in, t, **kw):
    return torch.tanh(0.5 * x_in - 2e-3 * t[:, None, None, None] + 0.1)


def teacher_fn(x_in, t, **kw):
    return 0.8 * torch.tanh(0.9 * x_in + 5e-4 * t[:, None, None, None])


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "cm_train.npz"), allow_pickle=False)


def _diffusions(norm):
    from models.cm.karras_diffusion import KarrasDenoiser
    student = KarrasDenoiser(sigma_data=0.5, weight_schedule="karras", distillation=True, loss_norm=norm)
    return student, KarrasDenoiser(sigma_data=0.5, weight_schedule="karras", distillation=False)


@pytest.mark.parametrize("S", [6, 18])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("mode", MODES)
def test_consistency_losses_torch_path_vs_reference(g, mode, norm, S):
    student, teacher_diffusion = _diffusions(norm)
    x0, noise, idx = torch.from_numpy(g["x_start"]), torch.from_numpy(g["noise"]), torch.from_numpy(g[f"indices.{S}"])
    cd = mode == "cd"
    seen = []

    def tgt(x_in, t, **kw):
        seen.append((x_in.clone(), t.clone()))
        return target_fn(x_in, t)
    terms = student.consistency_losses(online_fn, x0, S, target_model=tgt, teacher_model=teacher_fn if cd else None,
                                       teacher_diffusion=teacher_diffusion if cd else None, noise=noise, indices=idx)
    assert set(terms) == {"loss"} and terms["loss"].shape == (6,)
    np.testing.assert_allclose(terms["loss"].numpy(), g[f"analytic.{mode}.{norm}.{S}.loss"], rtol=1e-6, atol=0)
    # the target saw c_in(t2) x_t2 at 250 ln(t2): x_t2 of the fixture under the student's c_in
    t2 = torch.from_numpy(g[f"analytic.{mode}.{norm}.{S}.t2"])
    c_in = student.get_scalings_for_boundary_condition(t2)[2]
    np.testing.assert_allclose(seen[0][0].numpy(), (c_in[:, None, None, None] * torch.from_numpy(g[f"analytic.{mode}.{norm}.{S}.x_t2"])).numpy(),
                               rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(seen[0][1].numpy(), (250 * torch.log(t2 + 1e-44)).numpy(), rtol=1e-6)


def test_consistency_losses_draws_the_reference_indices(g):
    """indices=None: th.randint(0, num_scales - 1, (N,)) from the global generator, or from `generator`."""
    student, _ = _diffusions("l2")
    x0, noise = torch.from_numpy(g["x_start"]), torch.from_numpy(g["noise"])
    for S in (6, 18):
        torch.manual_seed(int(g[f"seed.{S}"]))
        a = student.consistency_losses(online_fn, x0, S, target_model=target_fn, noise=noise)["loss"]
        np.testing.assert_allclose(a.numpy(), g[f"analytic.ct.l2.{S}.loss"], rtol=1e-6, atol=0)
        b = student.consistency_losses(online_fn, x0, S, target_model=target_fn, noise=noise,
                                       generator=torch.Generator().manual_seed(int(g[f"seed.{S}"])))["loss"]
        assert torch.equal(a, b)


@pytest.mark.parametrize("S", [6, 18])
def test_time_levels_bit_equal_to_the_reference(g, S):
    """Built on the host with the reference's expression: bit-identical on the CPU that wrote the fixture, within 1 ulp of pow
    on another (the remark DESIGN 5.10 makes for the sigma tables)."""
    from models.cm.karras_diffusion import cd_levels
    lv = cd_levels(S, 0.002, 80.0, 7.0)
    assert lv.table.dtype == torch.float32 and lv.table.shape == (S,) and cd_levels(S, 0.002, 80.0, 7.0) is lv
    idx = torch.from_numpy(g[f"indices.{S}"])
    for key, got in (("t", lv.table[idx]), ("t2", lv.table[idx + 1])):
        ref = torch.from_numpy(g[f"analytic.cd.l2.{S}.{key}"])
        ulp = torch.abs(torch.nextafter(ref, ref * 2) - ref)
        assert (torch.abs(got - ref) <= ulp).all(), (key, got, ref)
    assert (torch.from_numpy(g[f"analytic.cd.l2.{S}.t2"]) == lv.table[S - 1]).any()       # the fixture reaches the boundary level
    assert float(lv.table[0]) == pytest.approx(80.0, rel=1e-6) and float(lv.table[-1]) == pytest.approx(0.002, rel=1e-6)
    with pytest.raises(ValueError):
        cd_levels(1, 0.002, 80.0, 7.0)


def test_fixture_conditions(g, golden_dir):
    """The fixture's own conditions, from the stored arrays: distiller and target apart by at least half their size (the loss must
    not sit in the bf16 noise of the nets), and the boundary level present."""
    plain = np.load(os.path.join(golden_dir, "cm_train_plain.npz"), allow_pickle=False)
    for src, tag in ((g, "unet"), (plain, "unet_plain")):
        assert float(src[f"{tag}.target_out_scale"]) >= 1.0
        for mode in MODES:
            for norm in NORMS:
                d, a, b = src[f"{tag}.{mode}.{norm}.sep"]
                assert d >= 0.5 * max(a, b), (tag, mode, norm, d, a, b)
    assert (g["indices.6"] == 4).any() and (g["indices.18"] == 16).any()


@pytest.mark.parametrize("name", sorted(EMA_PAIRS))
def test_create_ema_and_scales_fn_vs_reference(g, name):
    from models.cm.script_util import create_ema_and_scales_fn
    fn = create_ema_and_scales_fn(total_steps=1000, distill_steps_per_iter=50, **EMA_PAIRS[name])
    for s, ema, sc in zip(g["ema_scales.steps"], g[f"ema_scales.{name}.ema"], g[f"ema_scales.{name}.scales"]):
        got = fn(int(s))
        assert isinstance(got[0], float) and isinstance(got[1], int)
        assert got[1] == int(sc) and got[0] == pytest.approx(float(ema), rel=1e-12, abs=0), (name, s, got)


def test_unknown_ema_mode_pair_and_defaults():
    from models.cm.script_util import cm_train_defaults, create_ema_and_scales_fn, create_model_and_diffusion, model_and_diffusion_defaults
    for pair in (("adaptive", "fixed"), ("fixed", "nope"), ("adaptive", "progdist")):
        with pytest.raises(NotImplementedError):
            create_ema_and_scales_fn(pair[0], 0.9, pair[1], 2, 10, 100, 10)(0)
    d = cm_train_defaults()
    assert d == dict(teacher_model_path="", teacher_dropout=0.1, training_mode="consistency_distillation", target_ema_mode="fixed",
                     scale_mode="fixed", total_training_steps=600000, start_ema=0.0, start_scales=40, end_scales=40,
                     distill_steps_per_iter=50000, loss_norm="l2")
    kw = dict(model_and_diffusion_defaults(), image_size=64, num_channels=32, num_res_blocks=1, attention_resolutions="8", distillation=True)
    _, diffusion = create_model_and_diffusion(**kw)
    assert diffusion.distillation is True


def test_refusals():
    from models.cm.karras_diffusion import KarrasDenoiser
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="Must have a target model"):
        KarrasDenoiser().consistency_losses(online_fn, x, 6)
    with pytest.raises(NotImplementedError, match="LPIPS"):
        KarrasDenoiser(loss_norm="lpips")
    d = KarrasDenoiser()
    d.loss_norm = "lpips"                    # set on the object, as the reference's callers do
    with pytest.raises(NotImplementedError, match="no LPIPS weights"):
        d.consistency_losses(online_fn, x, 6, target_model=target_fn)
    d.loss_norm = "l3"
    with pytest.raises(ValueError):
        d.consistency_losses(online_fn, x, 6, target_model=target_fn)
    with pytest.raises(NotImplementedError, match="progdist"):
        d.progdist_losses(online_fn, x, 6)


# ------------------------------------------------------------------------------------------ CMTrainLoop on the torch path
class _Tiny(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(3, 3, generator=gen) * 0.3)
        self.b = torch.nn.Parameter(torch.randn(3, generator=gen) * 0.1)

    def forward(self, x, t):
        return torch.tanh(torch.einsum("oc,nchw->nohw", self.a, x) + self.b[None, :, None, None] + 1e-3 * t[:, None, None, None])


class _FixedDraws:
    """KarrasDenoiser whose consistency_losses takes noise and indices of each call from fixed lists."""

    def __init__(self, noises, indices, start=0, norm="l2"):
        from models.cm.karras_diffusion import KarrasDenoiser
        self.d = KarrasDenoiser(sigma_data=0.5, weight_schedule="uniform", distillation=True, loss_norm=norm)
        self.noises, self.indices, self.i = noises, indices, start

    def consistency_losses(self, model, x_start, num_scales, **kw):
        n, idx = self.noises[self.i].to(x_start.device), self.indices[self.i].to(x_start.device)
        self.i += 1
        return self.d.consistency_losses(model, x_start, num_scales, noise=n, indices=idx, **kw)


def _data(steps=4):
    gen = torch.Generator().manual_seed(99)
    x = [torch.rand(4, 3, 8, 8, generator=gen) * 2 - 1 for _ in range(steps)]
    noise = [torch.randn(4, 3, 8, 8, generator=gen) for _ in range(steps)]
    idx = [torch.randint(0, 5, (4,), generator=gen) for _ in range(steps)]
    return x, noise, idx


RATES = [0.9, 0.5, 0.95, 0.7, 0.8]


def _loop(tmp, mode, resume="", start=0, use_fp16=False):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.train_util import CMTrainLoop
    x, noise, idx = _data()
    cd = mode == "consistency_distillation"
    tl = CMTrainLoop(model=_Tiny(1), target_model=_Tiny(2), teacher_model=_Tiny(3) if cd else None,
                     teacher_diffusion=KarrasDenoiser(weight_schedule="uniform") if cd else None, training_mode=mode,
                     ema_scale_fn=lambda step: (RATES[step], 6), total_training_steps=4, diffusion=_FixedDraws(noise, idx, start),
                     data=None, batch_size=4, microbatch=4, lr=1e-2, ema_rate="0.9", log_interval=2, save_interval=2,
                     resume_checkpoint=resume, use_fp16=use_fp16, log_dir=str(tmp))
    # the loop's optimiser is the device RAdam; on the CPU torch's own RAdam (its base class, same state dict) stands in for it
    opt = torch.optim.RAdam(tl.mp_trainer.master_params, lr=1e-2)
    if resume:
        opt.load_state_dict(tl.opt.state_dict())
    tl.opt = opt
    return tl


@pytest.mark.parametrize("use_fp16", [False, True])
@pytest.mark.parametrize("mode", ["consistency_distillation", "consistency_training"])
def test_cmtrainloop_target_ema_counters_save_resume(tmp_path, mode, use_fp16):
    x, _, _ = _data()
    tl = _loop(tmp_path, mode, use_fp16=use_fp16)
    assert tl.step == 0 and tl.global_step == 0 and tl.target_model.training
    assert not any(p.requires_grad for p in tl.target_model.parameters())
    flat = lambda ps: torch.cat([p.detach().reshape(-1) for p in ps]).double()
    # the target's parameters in the order of its masters
    tgt_flat = lambda loop: flat(loop.target_model_master_params)
    rec = tgt_flat(tl).clone()
    mag = rec.abs()                  # the two terms of an update may cancel: the rounding bound is on their magnitudes
    masters = []
    for k in range(3):
        assert tl.run_step(x[k], {})
        assert tl.step == k + 1 and tl.global_step == k + 1
        masters.append(flat(tl.mp_trainer.master_params).clone())
        rate = RATES[k]                          # the rate of the step's global_step BEFORE it advanced (reference :392-398)
        rec = np.float32(rate).astype(np.float64) * rec + np.float32(1 - rate).astype(np.float64) * masters[-1]
        mag = np.float32(rate).astype(np.float64) * mag + np.float32(1 - rate).astype(np.float64) * masters[-1].abs()
        assert ((tgt_flat(tl) - rec).abs() <= 12 * 2.0 ** -24 * mag + 1e-30).all()
        # masters -> the target network's own parameters
        named = dict(tl.target_model.named_parameters())
        assert ((flat([named["a"]]) - (tgt_flat(tl)[:9] if not use_fp16 else tgt_flat(tl)[3:])).abs() <= 1e-12).all()
        if k == 1:
            tl.save()
            lg = tl.mp_trainer.lg_loss_scale
    assert tl._kv["step"] == 3
    files = sorted(os.listdir(tmp_path))
    want = ["ema_0.9_000002.pt", "model000002.pt", "opt000002.pt", "target_model000002.pt"]
    if mode == "consistency_distillation":
        want.append("teacher_model000002.pt")
    assert files == sorted(want)
    sd = torch.load(tmp_path / "target_model000002.pt")
    assert set(sd) == {"a", "b"}

    tr = _loop(tmp_path, mode, resume=str(tmp_path / "model000002.pt"), start=2, use_fp16=use_fp16)
    assert tr.global_step == 2 and tr.step == 2 and tr.resume_step == 2
    for k in ("a", "b"):
        assert torch.equal(dict(tr.target_model.named_parameters())[k].detach(), sd[k])
    if mode == "consistency_distillation":
        te = torch.load(tmp_path / "teacher_model000002.pt")
        assert all(torch.equal(dict(tr.teacher_model.named_parameters())[k].detach(), te[k]) for k in ("a", "b"))
        assert not tr.teacher_model.training
    tr.mp_trainer.lg_loss_scale = lg            # the reference does not checkpoint the loss scale
    assert tr.run_step(x[2], {})
    assert tr.global_step == 3
    assert torch.equal(flat(tr.mp_trainer.master_params), masters[2])
    assert torch.equal(tgt_flat(tr), tgt_flat(tl))


def test_resume_from_a_later_checkpoint_finds_the_first_saves_teacher(tmp_path):
    """teacher_model%06d.pt is written with the first save only; a resume from a later checkpoint reads that file."""
    x, _, _ = _data()
    tl = _loop(tmp_path, "consistency_distillation")
    saved_teacher = {k: v.detach().clone() for k, v in tl.teacher_model.state_dict().items()}
    for k in range(4):
        assert tl.run_step(x[k], {})
        if k in (1, 3):
            tl.save()
    names = sorted(f for f in os.listdir(tmp_path) if f.startswith("teacher_model"))
    assert names == ["teacher_model000002.pt"] and "target_model000004.pt" in os.listdir(tmp_path)
    torch.save({k: v + 1.0 for k, v in saved_teacher.items()}, tmp_path / "teacher_model000002.pt")      # told apart from _Tiny(3)
    tr = _loop(tmp_path, "consistency_distillation", resume=str(tmp_path / "model000004.pt"), start=4)
    assert tr.global_step == 4
    for k, v in tr.teacher_model.state_dict().items():
        assert torch.equal(v, saved_teacher[k] + 1.0)
    tgt = torch.load(tmp_path / "target_model000004.pt")
    assert all(torch.equal(dict(tr.target_model.named_parameters())[k].detach(), tgt[k]) for k in ("a", "b"))


def test_cmtrainloop_run_loop_and_refusals(tmp_path):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.train_util import CMTrainLoop
    x, _, _ = _data()
    tl = _loop(tmp_path, "consistency_training")
    tl.data = iter([(b, {}) for b in x] * 2)
    tl.lr_anneal_steps = 3                      # the reference's condition: runs until BOTH step and global_step reach their ends
    tl.run_loop()
    assert tl.global_step == 4 and tl.step == 4
    assert {"target_model000002.pt", "target_model000004.pt", "model000004.pt", "progress.jsonl"} <= set(os.listdir(tmp_path))
    assert [r["step"] for r in tl.logged] == [2, 4] and all(np.isfinite(r["loss"]) for r in tl.logged)
    kw = dict(model=_Tiny(1), target_model=_Tiny(2), teacher_model=None, teacher_diffusion=None, ema_scale_fn=lambda s: (0.9, 6),
              total_training_steps=1, diffusion=KarrasDenoiser(), data=None, batch_size=4, microbatch=-1, lr=1e-3, ema_rate="0.9",
              log_interval=1, save_interval=1, resume_checkpoint="", log_dir=str(tmp_path))
    with pytest.raises(NotImplementedError):
        CMTrainLoop(training_mode="progdist", **kw)
    with pytest.raises(ValueError):
        CMTrainLoop(training_mode="something", **kw)
    with pytest.raises(ValueError):
        CMTrainLoop(training_mode="consistency_distillation", **kw)      # no teacher
