"""Host side of progressive distillation: the level table of KarrasDenoiser.progdist_losses and its torch path against the
reference's values (tests/golden/pd_train.npz, make_golden_pd.py), CMTrainLoop(training_mode="progdist")'s phase bookkeeping and
constructor resume arithmetic on a small nn.Module, the refusals, the sampler's schedule, and the C entry points of
csrc/pd_train.hip under the host sanitizers.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS = ("l1", "l2")
SCALES = (1, 2, 6)


def online_fn(x_in, t, **kw):
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


def teacher_fn(x_in, t, **kw):
    return 0.8 * torch.tanh(0.9 * x_in + 5e-4 * t[:, None, None, None])


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "pd_train.npz"), allow_pickle=False)


def _diffusions(norm, ws="karras"):
    from models.cm.karras_diffusion import KarrasDenoiser
    return (KarrasDenoiser(sigma_data=0.5, weight_schedule=ws, distillation=False, loss_norm=norm),
            KarrasDenoiser(sigma_data=0.5, weight_schedule=ws, distillation=False))


# ------------------------------------------------------------------------------------------ level table
@pytest.mark.parametrize("S", SCALES)
def test_level_table_is_the_references_bit_for_bit(g, S):
    from models.cm.karras_diffusion import PDLevels, pd_levels
    lv = pd_levels(S, 0.002, 80.0, 7.0)
    assert lv is pd_levels(S, 0.002, 80.0, 7.0) and isinstance(lv, PDLevels)                 # memoised
    assert lv.table.dtype == torch.float32 and lv.table.shape == (2 * S + 1,) and lv.num_scales == S
    idx = torch.from_numpy(g[f"indices.{S}"])
    assert idx.min() >= 0 and idx.max() <= S - 1
    t, t2, t3 = lv.levels(idx)
    for norm in NORMS:
        for name, got in (("t", t), ("t2", t2), ("t3", t3)):
            assert torch.equal(got, torch.from_numpy(g[f"analytic.{norm}.{S}.{name}"])), (norm, name)
    # layout: coarse ladder first (t3 of index i is t of index i + 1), then the half steps, strictly between their neighbours
    tab = lv.table
    assert torch.equal(tab[idx + 1], t3) and torch.equal(tab[S + 1 + idx], t2)
    assert float(tab[0]) == pytest.approx(80.0, rel=1e-6) and float(tab[S]) == pytest.approx(0.002, rel=1e-5)
    assert (tab[:S] > tab[S + 1:]).all() and (tab[S + 1:] > tab[1:S + 1]).all()


def test_golden_conditions(g):
    """The conditions make_golden_pd.py asserted, again from the stored arrays."""
    idx = g["indices.6"]
    assert (idx == 0).any() and (idx == 5).any()
    for norm in NORMS:
        assert abs(float(g[f"analytic.{norm}.6.t3"].min()) - 0.002) < 1e-6
    for tag in ("unet", "unet_plain"):
        assert 1.0 <= float(g[f"{tag}.teacher_out_scale"]) <= 16.0
        for norm in NORMS:
            sep = g[f"{tag}.{norm}.sep"]
            assert sep[0] >= 0.5 * max(sep[1], sep[2]), (tag, norm, sep)
    from models.cm.karras_diffusion import pd_levels
    for S in SCALES:
        tab = pd_levels(S, 0.002, 80.0, 7.0).table.double()
        t, t3, t2 = tab[:S], tab[1:S + 1], tab[S + 1:]
        amp = float(((t / t2) * (t3 - t2).abs() / (t3 - t).abs()).max())
        assert amp <= 1.0 and amp == pytest.approx(float(g[f"amp.{S}"]), rel=1e-5)


def test_num_scales_below_one_is_refused():
    from models.cm.karras_diffusion import PDLevels
    with pytest.raises(ValueError, match="num_scales"):
        PDLevels(0, 0.002, 80.0, 7.0)


# ------------------------------------------------------------------------------------------ torch path
@pytest.mark.parametrize("S", SCALES)
@pytest.mark.parametrize("norm", NORMS)
def test_progdist_losses_torch_path_vs_reference(g, norm, S):
    student, teacher_diffusion = _diffusions(norm)
    x0, noise, idx = torch.from_numpy(g["x_start"]), torch.from_numpy(g["noise"]), torch.from_numpy(g[f"indices.{S}"])
    seen = []

    def teacher(x_in, t, **kw):
        seen.append((x_in.clone(), t.clone()))
        return teacher_fn(x_in, t)
    terms = student.progdist_losses(online_fn, x0, S, teacher_model=teacher, teacher_diffusion=teacher_diffusion, noise=noise, indices=idx)
    assert set(terms) == {"loss"} and terms["loss"].shape == (6,)
    np.testing.assert_allclose(terms["loss"].numpy(), g[f"analytic.{norm}.{S}.loss"], rtol=1e-6, atol=0)
    # two teacher evaluations, at 250 ln(t) and 250 ln(t2)
    assert len(seen) == 2
    for (_, tm), name in zip(seen, ("t", "t2")):
        lv = torch.from_numpy(g[f"analytic.{norm}.{S}.{name}"])
        np.testing.assert_allclose(tm.numpy(), (250 * torch.log(lv)).numpy(), rtol=1e-6)
    # the index draw of the reference, reproduced from its seed through the call's own randint
    torch.manual_seed(int(g[f"seed.{S}"]))
    drawn = student.progdist_losses(online_fn, x0, S, teacher_model=teacher_fn, teacher_diffusion=teacher_diffusion, noise=noise)
    np.testing.assert_allclose(drawn["loss"].numpy(), g[f"analytic.{norm}.{S}.loss"], rtol=1e-6, atol=0)
    gen = torch.Generator().manual_seed(int(g[f"seed.{S}"]))
    drawn = student.progdist_losses(online_fn, x0, S, teacher_model=teacher_fn, teacher_diffusion=teacher_diffusion, noise=noise,
                                    generator=gen)
    np.testing.assert_allclose(drawn["loss"].numpy(), g[f"analytic.{norm}.{S}.loss"], rtol=1e-6, atol=0)


def test_torch_path_target_and_gradient(g):
    """target_x of the fixture is what the torch path compares the student against: the l2 loss restated from it, and a gradient
    that reaches the student only."""
    student, teacher_diffusion = _diffusions("l2")
    x0, noise, idx = torch.from_numpy(g["x_start"]), torch.from_numpy(g["noise"]), torch.from_numpy(g["indices.6"])
    w = torch.nn.Parameter(torch.tensor(0.7))
    loss = student.progdist_losses(lambda x_in, t, **kw: torch.tanh(w * x_in + 1e-3 * t[:, None, None, None]), x0, 6,
                                   teacher_model=teacher_fn, teacher_diffusion=teacher_diffusion, noise=noise, indices=idx)["loss"]
    t = torch.from_numpy(g["analytic.l2.6.t"])
    x_t = x0 + noise * t[:, None, None, None]
    den = student.denoise(online_fn, x_t, t)[1]
    ref = ((den - torch.from_numpy(g["analytic.l2.6.target_x"])) ** 2).mean(dim=[1, 2, 3]) * (t ** -2 + 4.0)
    np.testing.assert_allclose(loss.detach().numpy(), ref.numpy(), rtol=1e-5)
    loss.mean().backward()
    assert w.grad is not None and torch.isfinite(w.grad) and w.grad != 0


def test_loss_refusals():
    from models.cm.karras_diffusion import KarrasDenoiser
    x = torch.zeros(2, 3, 16, 16)
    d = KarrasDenoiser()
    with pytest.raises(NotImplementedError, match="teacher"):
        d.progdist_losses(online_fn, x, 6)
    with pytest.raises(NotImplementedError, match="teacher"):
        d.progdist_losses(online_fn, x, 6, teacher_model=teacher_fn)
    d.loss_norm = "l2-32"                    # the reference's progdist has no such norm (its else branch)
    with pytest.raises(ValueError, match="Unknown loss norm"):
        d.progdist_losses(online_fn, x, 6, teacher_model=teacher_fn, teacher_diffusion=KarrasDenoiser())
    d.loss_norm = "lpips"
    with pytest.raises(NotImplementedError, match="no LPIPS weights"):
        d.progdist_losses(online_fn, x, 6, teacher_model=teacher_fn, teacher_diffusion=KarrasDenoiser())


# ------------------------------------------------------------------------------------------ sampler, host side
def test_sampler_schedule_and_refusals(g):
    from dxmi_hip import ops
    from models.cm import karras_diffusion as kd
    assert kd.karras_nfe("progdist", 1) == 1 and kd.karras_nfe("progdist", 3) == 3
    den = kd.KarrasDenoiserFn(kd.KarrasDenoiser(), online_fn)
    for steps in (1, 3):
        sig = kd.get_sigmas_karras(steps + 1, 0.002, 80.0, 7.0)
        assert torch.equal(sig, torch.from_numpy(g[f"sample.{steps}.sigmas"]))
        sch = kd._schedule(sig[:-1], "euler", den, 80.0, 0.0, 0.0, float("inf"), 1.0)
        assert sch.nfe == steps and len(sch.launches) == steps + 1
        assert [l["mode"] for l in sch.launches] == [ops.KARRAS_FIRST] + [ops.KARRAS_EULER] * steps
        assert sch.launches[-1]["last"] and all(l["draw"] is None for l in sch.launches)
        assert torch.equal(sch.eval_sigmas, sig[:steps])                     # every evaluation at a non-zero sigma
        assert float(sch.sigmas[-1]) == pytest.approx(0.002, rel=1e-5)       # the last step ends at sigma_min, not at 0
        assert "sigma_hat" not in sch.callback_info(1, None, None)
    # karras_sample itself keeps its refusal of this sampler name and points at the entry point that serves it
    with pytest.raises(NotImplementedError, match="progdist_sample"):
        kd.karras_sample(kd.KarrasDenoiser(), online_fn, (1, 3, 8, 8), 4, sampler="progdist")
    with pytest.raises(NotImplementedError, match="distillation=False"):
        kd.progdist_sample(kd.KarrasDenoiser(distillation=True), online_fn, (1, 3, 8, 8), 4)
    with pytest.raises(ValueError, match="at least one step"):
        kd.sample_progdist(den, torch.zeros(1, 3, 8, 8), torch.tensor([80.0, 0.0]))


def test_cm_train_flags_for_progdist():
    import cm_train
    a = cm_train.parse_args(["--training_mode", "progdist", "--synthetic_data", "True", "--teacher_model_path", "t.pt"])
    assert (a.target_ema_mode, a.scale_mode) == ("fixed", "progdist") and a.teacher_model_path == "t.pt"
    a = cm_train.parse_args(["--synthetic_data", "True"])
    assert a.scale_mode == "fixed"


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
    """KarrasDenoiser whose progdist_losses takes noise and indices of each call from fixed lists, and records the num_scales and
    the teacher diffusion of each call."""

    def __init__(self, noises, indices, start=0):
        from models.cm.karras_diffusion import KarrasDenoiser
        self.d = KarrasDenoiser(sigma_data=0.5, weight_schedule="uniform", distillation=False, loss_norm="l2")
        self.noises, self.indices, self.i, self.seen = noises, indices, start, []

    def __getattr__(self, name):
        return getattr(self.d, name)

    def progdist_losses(self, model, x_start, num_scales, **kw):
        n, idx = self.noises[self.i], self.indices[self.i] % num_scales
        self.i += 1
        self.seen.append((num_scales, kw["teacher_diffusion"], [p.detach().clone() for p in kw["teacher_model"].parameters()]))
        return self.d.progdist_losses(model, x_start, num_scales, noise=n, indices=idx, **kw)


STEPS = 9
LR = 1e-2


def _data():
    gen = torch.Generator().manual_seed(99)
    x = [torch.rand(4, 3, 8, 8, generator=gen) * 2 - 1 for _ in range(STEPS)]
    noise = [torch.randn(4, 3, 8, 8, generator=gen) for _ in range(STEPS)]
    idx = [torch.randint(0, 4, (4,), generator=gen) for _ in range(STEPS)]
    return x, noise, idx


def _scale_fn():
    from models.cm.script_util import create_ema_and_scales_fn
    return create_ema_and_scales_fn(target_ema_mode="fixed", start_ema=0.0, scale_mode="progdist", start_scales=4, end_scales=4,
                                    total_steps=100, distill_steps_per_iter=2)


def _loop(tmp, resume="", start=0, use_fp16=False, target=None, **over):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.train_util import CMTrainLoop
    _, noise, idx = _data()
    kw = dict(model=_Tiny(1), target_model=target, teacher_model=_Tiny(3), teacher_diffusion=KarrasDenoiser(weight_schedule="uniform"),
              training_mode="progdist", ema_scale_fn=_scale_fn(), total_training_steps=8, diffusion=_FixedDraws(noise, idx, start),
              data=None, batch_size=4, microbatch=4, lr=LR, ema_rate="0.9,0.5", log_interval=2, save_interval=100,
              resume_checkpoint=resume, use_fp16=use_fp16, lr_anneal_steps=2, log_dir=str(tmp))
    kw.update(over)
    tl = CMTrainLoop(**kw)
    # the loop's optimiser is the device RAdam; on the CPU torch's own RAdam (its base class, same state dict) stands in for it
    opt = torch.optim.RAdam(tl.mp_trainer.master_params, lr=LR)
    if resume:
        opt.load_state_dict(tl.opt.state_dict())
    tl.opt = opt
    return tl


def _flat(ps):
    return torch.cat([p.detach().reshape(-1) for p in ps])


@pytest.mark.parametrize("use_fp16", [False, True])
def test_cmtrainloop_progdist_phases_counters_save_resume(tmp_path, use_fp16):
    """Two phase changes (num_scales 4 -> 2 at global step 2, 2 -> 1 at 6).  The reference's bookkeeping (:388-442): the reset runs
    after the EMA updates of the FIRST step at the new num_scales and before the counters advance."""
    x, _, _ = _data()
    fn = _scale_fn()
    assert [fn(s)[1] for s in range(9)] == [4, 4, 2, 2, 2, 2, 1, 1, 1] and all(fn(s)[0] == 1.0 for s in range(9))
    tl = _loop(tmp_path, use_fp16=use_fp16)
    teacher0 = [p.detach().clone() for p in tl.teacher_model.parameters()]
    assert tl.step == 0 and tl.global_step == 0 and tl.lr_anneal_steps == 2 and tl.target_model is None
    assert not tl.teacher_model.training and not any(p.requires_grad for p in tl.teacher_model.parameters())
    # (step, global_step, lr_anneal_steps) after each run_step
    want = [(1, 1, 2), (2, 2, 2), (1, 3, 4), (2, 4, 4), (3, 5, 4), (4, 6, 4), (1, 7, 4), (2, 8, 4)]
    masters, students, lg = {}, {}, {}
    for k in range(8):
        opt_before = tl.opt
        assert tl.run_step(x[k], {})
        assert (tl.step, tl.global_step, tl.lr_anneal_steps) == want[k], k
        assert tl.opt.param_groups[0]["lr"] == pytest.approx(LR * (1 - tl.step / tl.lr_anneal_steps))
        masters[k] = _flat(tl.mp_trainer.master_params).clone()
        students[k] = _flat(tl.model.parameters()).clone()
        if k in (2, 6):         # the step that met a new num_scales: the student became the teacher, training restarted
            for pt, ps in zip(tl.teacher_model.parameters(), tl.model.parameters()):
                assert torch.equal(pt.detach(), ps.detach())
            assert tl.opt is not opt_before and type(tl.opt) is type(opt_before) and len(tl.opt.state) == 0
            assert len(tl.ema_params) == 2
            for ema in tl.ema_params:
                assert torch.equal(_flat(ema), masters[k]) and all(e.data_ptr() != m.data_ptr() for e, m in
                                                                   zip(ema, tl.mp_trainer.master_params))
            assert not tl.teacher_model.training and not any(p.requires_grad for p in tl.teacher_model.parameters())
        else:
            assert tl.opt is opt_before and len(tl.opt.state) > 0
            assert not torch.equal(_flat(tl.ema_params[0]), masters[k])
        if tl.global_step in (2, 3, 4, 7):
            tl.save()
            lg[tl.global_step] = tl.mp_trainer.lg_loss_scale
    # the teacher each step distilled from, and under which diffusion: the given teacher under teacher_diffusion while num_scales
    # is the first one; from then on teacher_model (the student copied at the reset that FOLLOWS the first step of a phase) under the
    # student's own diffusion
    seen = tl.diffusion.seen
    assert [s[0] for s in seen] == [4, 4, 2, 2, 2, 2, 1, 1]
    assert all(s[1] is tl.teacher_diffusion for s in seen[:2]) and all(s[1] is tl.diffusion for s in seen[2:])
    for k in (0, 1, 2):
        assert all(torch.equal(a, b) for a, b in zip(seen[k][2], teacher0))
    for k in (3, 4, 5, 6):
        assert torch.equal(_flat(seen[k][2]), students[2])
    assert torch.equal(_flat(seen[7][2]), students[6]) and not torch.equal(students[6], students[2])
    # teacher_model%06d.pt with EVERY save, and it is the teacher of that step
    files = set(os.listdir(tmp_path))
    for s in (2, 3, 4, 7):
        assert {f"teacher_model{s:06d}.pt", f"model{s:06d}.pt", f"opt{s:06d}.pt", f"ema_0.9_{s:06d}.pt", f"ema_0.5_{s:06d}.pt"} <= files
    assert not any(f.startswith("target_model") for f in files)
    te2, te3, te7 = (torch.load(tmp_path / f"teacher_model{s:06d}.pt") for s in (2, 3, 7))
    assert all(torch.equal(te2[k], v) for k, v in zip(("a", "b"), teacher0))
    assert not torch.equal(te3["a"], te2["a"]) and not torch.equal(te7["a"], te3["a"])

    # the constructor's resume arithmetic (:305-318): (step, lr_anneal_steps) of the resumed global step
    for s, (step, anneal) in {2: (0, 2), 3: (1, 4), 4: (2, 4), 7: (1, 4)}.items():
        tr = _loop(tmp_path, resume=str(tmp_path / f"model{s:06d}.pt"), start=s, use_fp16=use_fp16)
        assert (tr.global_step, tr.step, tr.lr_anneal_steps) == (s, step, anneal), s
        te = torch.load(tmp_path / f"teacher_model{s:06d}.pt")        # the file of the resumed step, not the first one found
        assert all(torch.equal(dict(tr.teacher_model.named_parameters())[k].detach(), te[k]) for k in ("a", "b"))
        if s in (2, 4):         # continues with the uninterrupted run, bit for bit, across the reset (2) and inside a phase (4)
            tr.mp_trainer.lg_loss_scale = lg[s]     # the reference does not checkpoint the loss scale
            for k in (s, s + 1):
                assert tr.run_step(x[k], {})
                assert (tr.step, tr.global_step, tr.lr_anneal_steps) == want[k]
                assert torch.equal(_flat(tr.mp_trainer.master_params), masters[k]), (s, k)
    os.remove(tmp_path / "teacher_model000004.pt")
    with pytest.raises(FileNotFoundError, match="teacher_model000004"):
        _loop(tmp_path, resume=str(tmp_path / "model000004.pt"), start=4, use_fp16=use_fp16)


def test_cmtrainloop_progdist_target_model_is_a_bystander(tmp_path):
    x, _, _ = _data()
    tl = _loop(tmp_path, target=_Tiny(2))
    before = [p.detach().clone() for p in tl.target_model.parameters()]
    assert not tl.target_model.training
    for k in range(3):
        assert tl.run_step(x[k], {})
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, tl.target_model.parameters())) and not tl.target_model.training
    tl.save()
    sd = torch.load(tmp_path / "target_model000003.pt")
    assert all(torch.equal(sd[k], v) for k, v in zip(("a", "b"), before))


def test_cmtrainloop_progdist_refusals(tmp_path):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.train_util import CMTrainLoop
    with pytest.raises(NotImplementedError, match="use_graph"):
        _loop(tmp_path, use_graph=True, use_fp16=True)
    with pytest.raises(NotImplementedError, match="teacher"):
        _loop(tmp_path, teacher_model=None)
    with pytest.raises(NotImplementedError, match="teacher"):
        _loop(tmp_path, teacher_diffusion=None)
    tl = _loop(tmp_path)
    tl.diffusion = KarrasDenoiser(loss_norm="l2-32")
    with pytest.raises(ValueError, match="Unknown loss norm"):
        tl.run_step(_data()[0][0], {})
    assert CMTrainLoop is type(tl)


# ------------------------------------------------------------------------------------------ host sanitizers
def test_pd_entry_points_under_address_and_ub_sanitizers():
    """`make asan_pd` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_pd.c, a program with its own main, against it and a no-device HIP runtime stub.  Null, misaligned and
    out-of-range arguments of the four dxmi_pd_* entry points must each come back as DXMI_EINVAL with the message of their check: no
    crash, no sanitizer report.  The program runs as a child process; nothing is loaded into python.  A host-only build: machines
    without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_pd"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_pd")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") >= 55
