"""CPU: the host side of the Karras samplers (models.cm.karras_diffusion.karras_sample and friends).

The schedule tables are checked against the reference's own run (tests/golden/karras_sample.npz, written by
make_golden_karras.py): the sigma ladder, sigma_hat and every evaluation's noise level bit for bit; the time input
250 ln(sigma + 1e-44) and the ancestral split to one ulp, because torch's CPU log and pow(., 0.5) kernels round differently
by one ulp on different CPU instruction sets (the fixture's machine and the test's need not match).  Also checked: the launch
plan against the reference's network-call count and draw sequence, the C-ABI entry point's argument checks (they run
before any device call), and the generate_large.py flags."""
import ctypes
import os

import numpy as np
import pytest
import torch

EINVAL = -1       # DXMI_EINVAL
CASES = {
    "heun6": dict(sampler="heun", steps=6),
    "heun6_churn": dict(sampler="heun", steps=6, s_churn=10.0, s_tmin=0.05, s_tmax=10.0, s_noise=1.007),
    "dpm4_churn": dict(sampler="dpm", steps=4, s_churn=2.0, s_noise=1.007),
    "euler8": dict(sampler="euler", steps=8),
    "ancestral8": dict(sampler="ancestral", steps=8),
    "heun40": dict(sampler="heun", steps=40, s_churn=40.0, s_tmin=0.05, s_tmax=50.0),
}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "karras_sample.npz"))


def schedule(case):
    from models.cm.karras_diffusion import KarrasDenoiser, KarrasSchedule, get_sigmas_karras
    p = dict(CASES[case])
    sampler, steps = p.pop("sampler"), p.pop("steps")
    return KarrasSchedule(get_sigmas_karras(steps, 0.002, 80.0, 7.0), sampler, KarrasDenoiser(sigma_data=0.5), x_scale=80.0, **p)


def f32(t):
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32))


def bits(t):
    return f32(t).view(np.uint32)


@pytest.mark.parametrize("case", list(CASES))
def test_schedule_tables_bitwise(gold, case):
    from dxmi_hip import ops
    sch = schedule(case)
    np.testing.assert_array_equal(bits(sch.sigmas), bits(gold[f"{case}.sigmas"]))
    np.testing.assert_array_equal(bits(sch.sigma_hat), bits(gold[f"{case}.sigma_hat"]))
    np.testing.assert_array_equal(bits(sch.eval_sigmas), bits(gold[f"{case}.eval_sigma"]))
    # row k precedes evaluation k + 1: its time input is the one the reference's denoise() handed to the model
    np.testing.assert_array_max_ulp(f32(sch.table[:sch.nfe, ops.KT_T]), f32(gold[f"{case}.eval_t"]), maxulp=1)
    # the divisor of d after evaluation k is the noise level of evaluation k
    np.testing.assert_array_equal(bits(sch.table[1:, ops.KT_SIGMA]), bits(gold[f"{case}.eval_sigma"]))
    if CASES[case]["sampler"] == "ancestral":
        np.testing.assert_array_max_ulp(f32(sch.sigma_up), f32(gold[f"{case}.sigma_up"]), maxulp=1)
        np.testing.assert_array_max_ulp(f32(sch.sigma_down), f32(gold[f"{case}.sigma_down"]), maxulp=1)
        assert torch.equal(sch.table[1:, ops.KT_SIGMA_UP], sch.sigma_up)
        assert torch.equal(sch.table[1:, ops.KT_DT], sch.sigma_down - sch.sigmas[:-1])


def test_scalings_follow_get_scalings():
    from dxmi_hip import ops
    from models.cm.karras_diffusion import KarrasDenoiser
    sch = schedule("heun6_churn")
    diff = KarrasDenoiser(sigma_data=0.5)
    for k in range(1, sch.nfe + 1):
        s = sch.table[k, ops.KT_SIGMA].reshape(1)
        c_skip, c_out, _ = diff.get_scalings(s)
        assert torch.equal(sch.table[k, ops.KT_CSKIP].reshape(1), c_skip) and torch.equal(sch.table[k, ops.KT_COUT].reshape(1), c_out)
    for k in range(sch.nfe):
        c_in = diff.get_scalings(sch.eval_sigmas[k].reshape(1))[2]
        assert torch.equal(sch.table[k, ops.KT_CIN].reshape(1), c_in)
    assert sch.table[0, ops.KT_XSCALE] == 80.0


@pytest.mark.parametrize("case", list(CASES))
def test_nfe_and_draw_sequence(gold, case):
    from models.cm.karras_diffusion import karras_nfe
    sch = schedule(case)
    sampler, steps = CASES[case]["sampler"], CASES[case]["steps"]
    assert sch.nfe == karras_nfe(sampler, steps) == len(gold[f"{case}.eval_sigma"])
    assert sch.nfe == {"heun": 2 * steps - 1, "dpm": 2 * steps, "euler": steps, "ancestral": steps}[sampler]
    draws = [l["draw"] for l in sch.launches if l["draw"] is not None]
    if f"{case}.draws" in gold.files:
        assert 1 + len(draws) == len(gold[f"{case}.draws"]) == len(gold[f"{case}.analytic.draws"])   # x_T, then one eps / z per step
    kinds = {"heun": "eps", "dpm": "eps", "ancestral": "z"}
    assert draws == ([(kinds[sampler], i) for i in range(steps)] if sampler in kinds else [])


LOOP_CASES = [("heun", 4, 0.0), ("heun", 4, 40.0), ("dpm", 3, 0.0), ("euler", 3, 0.0), ("ancestral", 4, 0.0)]


@pytest.mark.parametrize("with_callback", [False, True])
@pytest.mark.parametrize("with_generator", [True, False])
@pytest.mark.parametrize("sampler,steps,s_churn", LOOP_CASES)
def test_launch_loop_draws_stages_and_callbacks(monkeypatch, sampler, steps, s_churn, with_generator, with_callback):
    """The launch loop on the host alone (the stage kernel is replaced by a recorder, so no device is needed): a generator is
    called in the reference's order and number (randn for x_T, one randn_like per heun / dpm step even at gamma = 0, one per
    ancestral step, the last included, none for euler); the launches are the schedule's, row by row; a launch gets noise exactly
    when its draw is used, and without a generator all of them share one buffer; `denoised` is asked for exactly on the launches
    that fire the callback, whose dict has the reference's keys (no sigma_hat for euler, :566-574)."""
    from dxmi_hip import ops
    import models.cm.karras_diffusion as kd
    from test_cm_sample_host import CountingGenerator
    shape = (2, 3, 8, 8)
    sch = kd.KarrasSchedule(kd.get_sigmas_karras(steps, 0.002, 80.0, 7.0), sampler, kd.KarrasDenoiser(sigma_data=0.5), x_scale=80.0,
                            s_churn=s_churn)
    stages, infos = [], []
    monkeypatch.setattr(ops, "karras_stage", lambda mode, last, tab, row, x, **k: stages.append((mode, last, row, k.get("noise"),
                                                                                                  k.get("denoised"))))
    monkeypatch.setattr(sch, "device_table", lambda device: sch.table)
    gen = CountingGenerator() if with_generator else None
    kd._run_stages(sch, kd.KarrasDenoiserFn(kd.KarrasDenoiser(sigma_data=0.5), lambda x, t: x), None, shape, torch.device("cpu"), gen,
                   callback=infos.append if with_callback else None)

    draws = {"heun": steps, "dpm": steps, "euler": 0, "ancestral": steps}[sampler]
    if with_generator:
        assert gen.calls == [("randn", shape)] + [("randn_like", shape)] * draws
    assert len([l for l in sch.launches if l["draw"] is not None]) == draws
    assert [(m, l, r) for m, l, r, _, _ in stages] == [(l["mode"], l["last"], k) for k, l in enumerate(sch.launches)]

    def used(l):
        if l["draw"] is None:
            return False
        kind, i = l["draw"]
        return sch.gamma[i] > 0 if kind == "eps" else float(sch.sigma_up[i]) != 0.0
    assert [n is not None for _, _, _, n, _ in stages] == [used(l) for l in sch.launches]
    n_used = sum(used(l) for l in sch.launches)
    assert n_used == {("heun", 0.0): 0, ("heun", 40.0): steps, ("dpm", 0.0): 0, ("euler", 0.0): 0,
                      ("ancestral", 0.0): steps - 1}[sampler, s_churn]      # the last ancestral z has sigma_up = 0
    if not with_generator:
        assert len({id(n) for _, _, _, n, _ in stages if n is not None}) == min(n_used, 1)

    fired = [l["cb"] is not None for l in sch.launches]
    assert [d is not None for *_, d in stages] == ([False] * len(fired) if not with_callback else fired)
    if with_callback:
        keys = {"x", "i", "sigma", "denoised"} | (set() if sampler == "euler" else {"sigma_hat"})
        assert [set(i) for i in infos] == [keys] * steps and [i["i"] for i in infos] == list(range(steps))
        assert all(tuple(i["x"].shape) == shape and tuple(i["denoised"].shape) == shape for i in infos)
        assert all(torch.equal(i["sigma"], sch.sigmas[i["i"]]) for i in infos)
    else:
        assert infos == []


def test_churn_window_turns_gamma_off():
    sch = schedule("heun6_churn")
    sig = sch.sigmas[:-1]
    for i, g in enumerate(sch.gamma):
        inside = 0.05 <= float(sig[i]) <= 10.0
        assert (g > 0) == inside
    assert any(g == 0 for g in sch.gamma) and any(g > 0 for g in sch.gamma)


def test_unsupported_samplers_and_distillation():
    from models.cm.karras_diffusion import KarrasDenoiser, karras_sample, sample_heun
    diff = KarrasDenoiser()
    for s in ("onestep", "multistep", "progdist"):
        with pytest.raises(NotImplementedError, match="consistency-distilled"):
            karras_sample(diff, lambda x, t: x, (1, 3, 8, 8), 4, sampler=s)
    with pytest.raises(ValueError):
        karras_sample(diff, lambda x, t: x, (1, 3, 8, 8), 4, sampler="lms")
    with pytest.raises(NotImplementedError, match="distillation"):
        karras_sample(KarrasDenoiser(distillation=True), lambda x, t: x, (1, 3, 8, 8), 4)
    with pytest.raises(TypeError, match="KarrasDenoiserFn"):
        sample_heun(lambda x, s: x, torch.zeros(1, 3, 8, 8), torch.ones(3), None)


def test_cpu_device_is_refused():
    from dxmi_hip._lib import DxmiError
    from models.cm.karras_diffusion import KarrasDenoiser, karras_sample
    with pytest.raises(DxmiError, match="HIP device path"):
        karras_sample(KarrasDenoiser(), lambda x, t: x, (1, 3, 8, 8), 4, device="cpu")


def test_stage_entry_rejects_bad_arguments():
    """dxmi_karras_stage validates before it touches the device: NULL pointers, N <= 0, bad CHW, unknown mode."""
    from dxmi_hip import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(16)                 # never dereferenced: every call below fails its argument check
    null = ctypes.c_void_p(0)

    def call(mode=ops.KARRAS_EULER, last=0, tab=p, x=p, x2=p, d=p, F=p, noise=null, x_in=p, t=p, out=p, N=2, CHW=768):
        return lib.dxmi_karras_stage(mode, last, tab, 0, x, x2, d, F, noise, x_in, t, out, null, N, CHW, null)
    assert call(mode=6) == EINVAL and b"unknown mode" in lib.dxmi_last_error()
    assert call(mode=-1) == EINVAL
    assert call(N=0) == EINVAL and call(N=-3) == EINVAL
    assert call(CHW=770) == EINVAL and b"multiple of 4" in lib.dxmi_last_error()
    assert call(CHW=0) == EINVAL
    assert call(tab=null) == EINVAL and call(x=null) == EINVAL
    assert call(F=null) == EINVAL
    assert call(mode=ops.KARRAS_PRED, x2=null) == EINVAL
    assert call(mode=ops.KARRAS_HEUN_CORR, d=null) == EINVAL
    assert call(mode=ops.KARRAS_PRED, last=1) == EINVAL
    assert call(mode=ops.KARRAS_FIRST, last=1) == EINVAL
    assert call(last=1, out=null) == EINVAL
    assert call(x_in=null) == EINVAL and call(t=null) == EINVAL
    assert call(mode=ops.KARRAS_PRED, noise=p) == EINVAL


# ------------------------------------------------------------------------------------------------ generate_large.py flags
def test_cli_flags_parse():
    import generate_large as g
    a, _ = g.parse_args(["--log_dir", "d", "--n_sample", "4"])
    assert a.karras_sampler is None and a.pretrained is None and a.karras_steps is None
    a, _ = g.parse_args(["--log_dir", "d", "--n_sample", "4", "--karras_sampler", "dpm"])
    assert (a.karras_steps, a.rho, a.s_churn, a.s_tmin, a.s_tmax, a.s_noise) == (40, 7.0, 0.0, 0.0, float("inf"), 1.0)
    a, _ = g.parse_args(["--log_dir", "d", "--n_sample", "4", "--karras_sampler", "heun", "--karras_steps", "18", "--rho", "5",
                         "--s_churn", "3", "--s_tmin", "0.05", "--s_tmax", "50", "--s_noise", "1.003"])
    assert (a.karras_steps, a.rho, a.s_churn, a.s_tmin, a.s_tmax, a.s_noise) == (18, 5.0, 3.0, 0.05, 50.0, 1.003)
    with pytest.raises(SystemExit):
        g.parse_args(["--log_dir", "d", "--n_sample", "4", "--karras_sampler", "multistep"])


def test_cli_guidance_conflict_and_stray_flags():
    import generate_large as g
    with pytest.raises(SystemExit):
        g.parse_args(["--log_dir", "d", "--n_sample", "4", "--karras_sampler", "heun", "--guidance_scale", "1.5"])
    with pytest.raises(SystemExit):
        g.parse_args(["--log_dir", "d", "--n_sample", "4", "--s_churn", "3"])
    with pytest.raises(SystemExit):
        g.parse_args(["--log_dir", "d", "--n_sample", "4", "--pretrained", "w.pt"])


def test_cli_pretrained_resolution():
    import configs_builtin
    import generate_large as g
    cfg = configs_builtin.get("imagenet64_T10")
    base = ["--log_dir", "logs/run", "--n_sample", "4", "--karras_sampler", "heun"]
    a, _ = g.parse_args(base + ["--pretrained", "w.pt"])
    assert g.resolve_weights(a, cfg) == ("w.pt", "plain")
    a, _ = g.parse_args(base + ["--pretrained"])
    assert g.resolve_weights(a, cfg) == (cfg.training.pretrained_path, "plain")
    a, _ = g.parse_args(base)
    assert g.resolve_weights(a, cfg) == (os.path.join("logs/run", "sampler.pth"), "sampler")
    a, _ = g.parse_args(base + ["--synthetic", "imagenet64_T10"])
    assert g.resolve_weights(a, cfg) == (None, None)
    cfg.training.pretrained_path = None
    a, _ = g.parse_args(base + ["--pretrained"])
    with pytest.raises(ValueError):
        g.resolve_weights(a, cfg)
