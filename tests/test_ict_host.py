"""Host side of improved consistency training (Song and Dhariwal 2023, "Improved Techniques for Training Consistency Models"): the
doubling curriculum of create_ema_and_scales_fn, the discretised lognormal level sampler, the pseudo-Huber norm and the 1 / (t - t2)
weighting on the torch path of KarrasDenoiser.consistency_losses, and the flags of cm_train.py.  The reference tree has none of it:
the ground truth is the paper's formulas in float64, written out here.  No GPU.

Bound of the loss values.  u = 2^-24.  Every element of distiller - target comes out of about ten fp32 operations on the four
products c_out F, c_skip x_t (online, target) and on the analytic nets' tanh (Lipschitz 1 in an argument of relative error 3 u), so
it lies within d_e = 64 u (M_e + 1) of float64, M_e the sum of the four products' magnitudes.  Then s = sum(df^2) is within
dS = sum(2 |df| d_e + d_e^2) + 64 u s, the metric L = s / (sqrt(s + c^2) + c) (dL/ds = 1 / (2 sqrt(s + c^2))) within
dS / (2 sqrt(s + c^2)) + 8 u L, and the weight (two to three roundings) within 4 u."""
import math

import numpy as np
import pytest
import torch

U = 2.0 ** -24
SMIN32 = float(np.float32(0.002))      # sigma_min as the fp32 scalar the torch path's fp32 tensors meet


def online_fn(x_in, t, **kw):          # the analytic nets of tests/test_cm_train_host.py
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


def target_fn(x_in, t, **kw):
    return torch.tanh(0.5 * x_in - 2e-3 * t[:, None, None, None] + 0.1)


def teacher_fn(x_in, t, **kw):
    return 0.8 * torch.tanh(0.9 * x_in + 5e-4 * t[:, None, None, None])


# ------------------------------------------------------------------------------------------ curriculum
def test_ict_curriculum_table():
    from models.cm.script_util import create_ema_and_scales_fn
    fn = create_ema_and_scales_fn("fixed", 0.0, "ict", 10, 1280, 600000, 50000)
    want = {0: 11, 74999: 11, 75000: 21, 149999: 21, 150000: 41, 300000: 161, 524999: 641, 525000: 1281, 599999: 1281, 600000: 1281,
            10 ** 9: 1281}
    for step, scales in want.items():
        got = fn(step)
        assert isinstance(got[0], float) and isinstance(got[1], int)
        assert got == (0.0, scales), (step, got)
    # the formula itself, step by step on a small schedule
    for start, end, total in ((2, 8, 6), (3, 50, 40), (10, 10, 7), (2, 64, 1000)):
        fn = create_ema_and_scales_fn("fixed", 0.25, "ict", start, end, total, 1)
        kp = max(1, total // (int(math.floor(math.log2(end // start))) + 1))
        for k in range(2 * total + 3):
            assert fn(k) == (0.25, min(start * 2 ** (k // kp), end) + 1), (start, end, total, k)
    assert [create_ema_and_scales_fn("fixed", 0.0, "ict", 2, 8, 6, 1)(k)[1] for k in range(6)] == [3, 3, 5, 5, 9, 9]


def test_ict_curriculum_k_prime_clamps_and_unknown_pairs_raise():
    from models.cm.script_util import create_ema_and_scales_fn
    for total in (0, 1, 2):                       # total_steps // 3 = 0: K' = 1, one doubling per step
        fn = create_ema_and_scales_fn("fixed", 0.0, "ict", 2, 8, total, 1)
        assert [fn(k)[1] for k in range(5)] == [3, 5, 9, 9, 9]
    for pair in (("adaptive", "ict"), ("fixed", "nope"), ("adaptive", "fixed")):
        with pytest.raises(NotImplementedError):
            create_ema_and_scales_fn(pair[0], 0.9, pair[1], 2, 10, 100, 10)
    with pytest.raises(ValueError):
        create_ema_and_scales_fn("fixed", 0.0, "ict", 8, 2, 100, 10)


# ------------------------------------------------------------------------------------------ sampler
def _pmf64(S, p_mean=-1.1, p_std=2.0):
    from models.cm.karras_diffusion import cd_levels
    t = [float(v) for v in cd_levels(S, 0.002, 80.0, 7.0).table]
    e = [math.erf((math.log(v) - p_mean) / (math.sqrt(2) * p_std)) for v in t]
    p = np.array([e[i] - e[i + 1] for i in range(S - 1)], dtype=np.float64)
    return p / p.sum()


@pytest.mark.parametrize("S", [3, 11, 1281])
def test_sampler_pmf_and_cdf(S):
    from models.cm.resample import DiscreteLogNormalSampler
    smp = DiscreteLogNormalSampler(0.002, 80.0, 7.0)
    tab = smp.cdf(S)
    assert smp.cdf(S) is tab and tab.num_scales == S                       # memoised per S
    p = _pmf64(S)
    assert tab.pmf.dtype == torch.float64 and tab.pmf.shape == (S - 1,)
    # a difference of two erf values near +-1 carries the absolute error of one of them: 2^-52
    np.testing.assert_allclose(tab.pmf.numpy(), p, rtol=0, atol=4 * 2.0 ** -52)
    assert abs(float(tab.pmf.sum()) - 1.0) <= S * 2.0 ** -52 and (tab.pmf > 0).all()
    cdf = tab.table
    assert cdf.dtype == torch.float32 and cdf.shape == (S - 1,)
    assert float(cdf[-1]) == 1.0 and (cdf[1:] >= cdf[:-1]).all() and float(cdf[0]) > 0
    np.testing.assert_allclose(cdf.numpy().astype(np.float64)[:-1], np.cumsum(p)[:-1], rtol=2 * U, atol=0)
    if S in (11, 1281):                                                    # the defaults leave every bin reachable in fp32
        assert (cdf[1:] > cdf[:-1]).all()


def test_sampler_other_parameters_change_the_table_and_bad_ones_raise():
    from models.cm.resample import DiscreteLogNormalSampler
    a = DiscreteLogNormalSampler(0.002, 80.0, 7.0).cdf(11).pmf
    b = DiscreteLogNormalSampler(0.002, 80.0, 7.0, p_mean=-0.5, p_std=1.0).cdf(11).pmf
    np.testing.assert_allclose(b.numpy(), _pmf64(11, -0.5, 1.0), rtol=0, atol=4 * 2.0 ** -52)
    assert not torch.equal(a, b)
    for kw in (dict(p_std=0.0), dict(p_std=-1.0), dict(p_mean=float("nan"))):
        with pytest.raises(ValueError):
            DiscreteLogNormalSampler(0.002, 80.0, 7.0, **kw)


@pytest.mark.parametrize("S", [3, 11, 1281])
def test_sampler_draw_is_searchsorted_right(S):
    from models.cm.resample import DiscreteLogNormalSampler
    smp = DiscreteLogNormalSampler(0.002, 80.0, 7.0)
    cdf32 = smp.cdf(S).table.numpy()
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    u = torch.rand(4096, generator=torch.Generator().manual_seed(S))
    u[0], u[1] = 0.0, float(below_one)
    u[2:2 + min(S - 1, 512)] = torch.from_numpy(cdf32[:512].copy())        # u on a CDF entry: side="right" goes past it
    u[u >= 1] = float(below_one)                                            # the last CDF entry is 1: rand() never is
    got = smp.indices_from_uniform(S, u)
    assert got.dtype == torch.int64 and got.shape == (4096,)
    assert np.array_equal(got.numpy(), np.searchsorted(cdf32, u.numpy(), side="right"))
    assert int(got.min()) >= 0 and int(got.max()) <= S - 2
    assert int(got[0]) == 0 and int(got[1]) == S - 2
    # sample_indices is that on rand(N) of the generator
    idx = smp.sample_indices(S, 4096, "cpu", torch.Generator().manual_seed(5))
    u5 = torch.rand(4096, generator=torch.Generator().manual_seed(5))
    assert np.array_equal(idx.numpy(), np.searchsorted(cdf32, u5.numpy(), side="right"))
    assert int(idx.min()) >= 0 and int(idx.max()) <= S - 2


def test_sampler_generator_seed_repeats_and_frequencies_follow_the_pmf():
    from models.cm.resample import DiscreteLogNormalSampler
    smp = DiscreteLogNormalSampler(0.002, 80.0, 7.0)
    a = smp.sample_indices(11, 1000, "cpu", torch.Generator().manual_seed(7))
    b = smp.sample_indices(11, 1000, "cpu", torch.Generator().manual_seed(7))
    c = smp.sample_indices(11, 1000, "cpu", torch.Generator().manual_seed(8))
    assert torch.equal(a, b) and not torch.equal(a, c)
    n = 200000
    idx = smp.sample_indices(11, n, "cpu", torch.Generator().manual_seed(1))
    freq = np.bincount(idx.numpy(), minlength=10) / n
    p = _pmf64(11)
    assert (np.abs(freq - p) <= 6 * np.sqrt(p * (1 - p) / n) + 1e-7).all()      # six binomial standard deviations per bin
    torch.manual_seed(3)                                                         # no generator: the global one
    d = smp.sample_indices(11, 64, "cpu")
    torch.manual_seed(3)
    assert torch.equal(d, smp.sample_indices(11, 64, "cpu"))


# ------------------------------------------------------------------------------------------ the torch path of the loss
def _scal64(s, sd=0.5):
    """get_scalings_for_boundary_condition in float64."""
    e = lambda v: v[:, None, None, None]
    return (e(sd ** 2 / ((s - SMIN32) ** 2 + sd ** 2)), e((s - SMIN32) * sd / (s ** 2 + sd ** 2) ** 0.5), e(1 / (s ** 2 + sd ** 2) ** 0.5))


def _edm_scal64(s, sd=0.5):
    e = lambda v: v[:, None, None, None]
    return e(sd ** 2 / (s ** 2 + sd ** 2)), e(s * sd / (s ** 2 + sd ** 2) ** 0.5), e(1 / (s ** 2 + sd ** 2) ** 0.5)


def _loss64(x0, noise, idx, S, cd, ws, c):
    """consistency_losses with the pseudo-Huber norm in float64 -> (loss, bound)."""
    from models.cm.karras_diffusion import cd_levels
    tab = cd_levels(S, 0.002, 80.0, 7.0).table.double()
    t, t2 = tab[idx], tab[idx + 1]
    e = lambda v: v[:, None, None, None]
    x0, noise = x0.double(), noise.double()
    tm = lambda s: 250 * torch.log(s)
    x_t = x0 + noise * e(t)
    cs_s, cs_o, cs_i = _scal64(t)
    F = online_fn(cs_i * x_t, tm(t))
    if cd:                                                     # Heun through the teacher (EDM scalings)
        den = lambda x, s: (lambda k, o, i: o * teacher_fn(i * x, tm(s)) + k * x)(*_edm_scal64(s))
        d = (x_t - den(x_t, t)) / e(t)
        samples = x_t + d * e(t2 - t)
        nd = (samples - den(samples, t2)) / e(t2)
        x_t2 = x_t + (d + nd) * e((t2 - t) / 2)
    else:                                                      # Euler with denoiser = x_start
        x_t2 = x_t + (x_t - x0) / e(t) * e(t2 - t)
    ct_s, ct_o, ct_i = _scal64(t2)
    Ft = target_fn(ct_i * x_t2, tm(t2))
    df = (cs_o * F + cs_s * x_t) - (ct_o * Ft + ct_s * x_t2)
    Me = (cs_o * F).abs() + (cs_s * x_t).abs() + (ct_o * Ft).abs() + (ct_s * x_t2).abs()
    w = {"ict": 1 / (t - t2), "karras": t ** -2 + 1 / 0.25, "uniform": torch.ones_like(t)}[ws]
    s = (df ** 2).flatten(1).sum(1)
    root = torch.sqrt(s + c ** 2)
    L = s / (root + c)
    assert torch.allclose(L, root - c, rtol=1e-9, atol=1e-13)              # the two forms agree where float64 can tell
    de = 64 * U * (Me + 1)
    dS = (2 * df.abs() * de + de ** 2).flatten(1).sum(1) + 64 * U * s
    return w * L, w * (dS / (2 * root) + 8 * U * L) + 4 * U * w * L


@pytest.mark.parametrize("ws", ["ict", "karras", "uniform"])
@pytest.mark.parametrize("huber_c", [None, 0.3])
@pytest.mark.parametrize("mode", ["cd", "ct"])
def test_pseudo_huber_torch_path_vs_float64(golden_dir, mode, huber_c, ws):
    import os
    from models.cm.karras_diffusion import KarrasDenoiser
    g = np.load(os.path.join(golden_dir, "cm_train.npz"), allow_pickle=False)
    cd = mode == "cd"
    student = KarrasDenoiser(sigma_data=0.5, weight_schedule=ws, distillation=True, loss_norm="pseudo-huber", huber_c=huber_c)
    td = KarrasDenoiser(sigma_data=0.5, weight_schedule="karras", distillation=False)
    x0, noise = torch.from_numpy(g["x_start"]), torch.from_numpy(g["noise"])
    c = 0.00054 * math.sqrt(x0[0].numel()) if huber_c is None else huber_c
    for S in (6, 18):
        idx = torch.from_numpy(g[f"indices.{S}"])
        assert (idx == S - 2).any()                                         # the boundary level is among them
        got = student.consistency_losses(online_fn, x0, S, target_model=target_fn, teacher_model=teacher_fn if cd else None,
                                         teacher_diffusion=td if cd else None, noise=noise, indices=idx)
        assert set(got) == {"loss"} and got["loss"].shape == (6,) and got["loss"].dtype == torch.float32
        ref, bound = _loss64(x0, noise, idx, S, cd, ws, c)
        err = (got["loss"].double() - ref).abs()
        print(f"{mode} {ws} c={c:.4g} S={S}: worst |err| / bound {float((err / bound).max()):.3e}, worst relative {float((err / ref).max()):.3e}")
        assert (err <= bound).all(), (err / bound)
        assert (bound <= 1e-2 * ref).all()                                  # the bound is no vacuous one at these operands


def test_pseudo_huber_gradient_reaches_the_online_net_only():
    from models.cm.karras_diffusion import KarrasDenoiser
    a = torch.nn.Parameter(torch.tensor(0.7))
    b = torch.nn.Parameter(torch.tensor(0.5))
    online = lambda x_in, t, **kw: torch.tanh(a * x_in)
    target = lambda x_in, t, **kw: torch.tanh(b * x_in + 0.1)
    gen = torch.Generator().manual_seed(0)
    x0 = torch.rand(4, 3, 8, 8, generator=gen) * 2 - 1
    d = KarrasDenoiser(weight_schedule="ict", distillation=True, loss_norm="pseudo-huber")
    loss = d.consistency_losses(online, x0, 11, target_model=target, generator=gen)["loss"]
    loss.mean().backward()
    assert a.grad is not None and torch.isfinite(a.grad) and float(a.grad) != 0 and b.grad is None


def test_index_sampler_draws_the_indices_of_consistency_losses():
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.resample import DiscreteLogNormalSampler
    smp = DiscreteLogNormalSampler(0.002, 80.0, 7.0)
    gen = torch.Generator().manual_seed(0)
    x0 = torch.rand(6, 3, 8, 8, generator=gen) * 2 - 1
    noise = torch.randn(6, 3, 8, 8, generator=gen)
    d = KarrasDenoiser(weight_schedule="ict", distillation=True, loss_norm="pseudo-huber")
    a = d.consistency_losses(online_fn, x0, 11, target_model=target_fn, noise=noise, index_sampler=smp,
                             generator=torch.Generator().manual_seed(4))["loss"]
    idx = smp.sample_indices(11, 6, "cpu", torch.Generator().manual_seed(4))
    b = d.consistency_losses(online_fn, x0, 11, target_model=target_fn, noise=noise, indices=idx)["loss"]
    assert torch.equal(a, b)
    c = d.consistency_losses(online_fn, x0, 11, target_model=target_fn, noise=noise, indices=idx, index_sampler=smp)["loss"]
    assert torch.equal(a, c)                                                 # given indices win over the sampler
    torch.manual_seed(int(1))                                                # no sampler: the randint draw, unchanged
    e = d.consistency_losses(online_fn, x0, 11, target_model=target_fn, noise=noise)["loss"]
    torch.manual_seed(int(1))
    f = d.consistency_losses(online_fn, x0, 11, target_model=target_fn, noise=noise, indices=torch.randint(0, 10, (6,)))["loss"]
    assert torch.equal(e, f)


def test_refusals():
    from models.cm.karras_diffusion import KarrasDenoiser, get_weightings
    x = torch.zeros(2, 3, 8, 8)
    kw = dict(target_model=target_fn, indices=torch.tensor([0, 4]))
    for norm in ("l1", "l2", "l2-32"):                                       # ict goes with pseudo-huber only
        with pytest.raises(NotImplementedError, match="pseudo-huber"):
            KarrasDenoiser(weight_schedule="ict", loss_norm=norm).consistency_losses(online_fn, x, 6, **kw)
    with pytest.raises(NotImplementedError, match="pseudo-huber"):
        KarrasDenoiser(weight_schedule="ict").training_losses(online_fn, x, torch.ones(2))
    with pytest.raises(NotImplementedError, match="pseudo-huber"):
        get_weightings("ict", torch.ones(2), 0.5)
    td = KarrasDenoiser()
    with pytest.raises(NotImplementedError, match="pseudo-huber"):
        KarrasDenoiser(weight_schedule="ict", loss_norm="l2").progdist_losses(online_fn, x, 4, teacher_model=teacher_fn, teacher_diffusion=td,
                                                                              indices=torch.tensor([0, 3]))
    with pytest.raises(ValueError, match="Unknown loss norm"):               # as l2-32 is refused there
        KarrasDenoiser(loss_norm="pseudo-huber").progdist_losses(online_fn, x, 4, teacher_model=teacher_fn, teacher_diffusion=td,
                                                                 indices=torch.tensor([0, 3]))
    with pytest.raises(ValueError, match="Unknown loss norm"):
        KarrasDenoiser(loss_norm="l2-32").progdist_losses(online_fn, x, 4, teacher_model=teacher_fn, teacher_diffusion=td,
                                                          indices=torch.tensor([0, 3]))
    for c in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="huber_c"):
            KarrasDenoiser(loss_norm="pseudo-huber", huber_c=c)
        d = KarrasDenoiser(loss_norm="pseudo-huber")
        d.huber_c = c                                                        # set on the object afterwards, as loss_norm is
        with pytest.raises(ValueError, match="huber_c"):
            d.consistency_losses(online_fn, x, 6, **kw)
    ok = KarrasDenoiser(loss_norm="pseudo-huber", huber_c=0.1).consistency_losses(online_fn, x, 6, **kw)["loss"]
    assert torch.isfinite(ok).all()


def test_target_ema_rate_zero_is_a_copy():
    """0 * target + source is not: a source of -0 would become +0 and a non-finite target NaN."""
    from models.cm.nn import update_ema
    src = [torch.tensor([-0.0, 1.5, -3.25e-40, 0.0]), torch.tensor([2.0])]
    tgt = [torch.tensor([1.0, float("inf"), float("nan"), -0.0]), torch.tensor([-7.0])]
    update_ema(tgt, src, rate=0.0)
    for a, b in zip(tgt, src):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    update_ema(tgt, [torch.zeros(4), torch.zeros(1)], rate=0.5)                # any other rate: the reference's recursion
    assert torch.equal(tgt[1], torch.tensor([1.0]))


# ------------------------------------------------------------------------------------------ cm_train.py
def test_cli_ict_flag():
    import cm_train
    args = cm_train.parse_args(["--ict", "True", "--synthetic_data", "True"])
    assert args.training_mode == "consistency_training"
    assert (args.loss_norm, args.weight_schedule, args.scale_mode, args.target_ema_mode) == ("pseudo-huber", "ict", "ict", "fixed")
    assert (args.start_ema, args.start_scales, args.end_scales, args.index_sampler) == (0.0, 10, 1280, "lognormal")
    assert args.huber_c == 0.0 and (args.p_mean, args.p_std) == (-1.1, 2.0)
    same = cm_train.parse_args(["--ict", "True", "--training_mode", "consistency_training", "--synthetic_data", "True", "--huber_c", "0.03"])
    assert same.loss_norm == "pseudo-huber" and same.huber_c == 0.03
    for mode in ("consistency_distillation", "progdist"):
        with pytest.raises(SystemExit):
            cm_train.parse_args(["--ict", "True", "--training_mode", mode, "--synthetic_data", "True"])
    plain = cm_train.parse_args(["--synthetic_data", "True"])                # nothing moves without the flag
    assert (plain.loss_norm, plain.weight_schedule, plain.scale_mode, plain.index_sampler, plain.ict) == ("l2", "karras", "fixed", "uniform", False)
    piece = cm_train.parse_args(["--synthetic_data", "True", "--scale_mode", "ict", "--index_sampler", "lognormal", "--p_mean", "-0.4",
                                 "--p_std", "1.5", "--loss_norm", "pseudo-huber"])
    assert (piece.scale_mode, piece.index_sampler, piece.p_mean, piece.p_std) == ("ict", "lognormal", -0.4, 1.5)
    with pytest.raises(SystemExit):
        cm_train.parse_args(["--synthetic_data", "True", "--index_sampler", "gaussian"])
    with pytest.raises(SystemExit):
        cm_train.parse_args(["--synthetic_data", "True", "--huber_c", "-1"])
    with pytest.raises(SystemExit):                                          # the pairing, refused before any net is built
        cm_train.parse_args(["--synthetic_data", "True", "--weight_schedule", "ict"])
    with pytest.raises(SystemExit):
        cm_train.parse_args(["--synthetic_data", "True", "--training_mode", "progdist", "--loss_norm", "pseudo-huber"])


# ------------------------------------------------------------------------------------------ the C entry points' argument checks
def test_huber_entry_points_refuse_malformed_arguments_before_any_launch():
    """Every check returns before the launch, so the refusals need no device: the pointers are host buffers nothing dereferences."""
    from dxmi_hip import _lib
    lib = _lib.load()
    buf = torch.zeros(4 * 768 + 8)
    p = buf.data_ptr() + (-buf.data_ptr()) % 16
    inf, nan = float("inf"), float("nan")
    good_f = [p, p, p, p, p, p, 18, p, p, 4, 768, 0.1, 0.5, 0.002, 0, 5, None]
    good_b = [p, p, p, p, p, p, p, p, 18, p, 4, 768, 0.1, 0.5, 0.002, 0, 5, None]

    def refused(fn, good, at, value, word):
        a = list(good)
        a[at] = value
        assert fn(*a) == -1, (at, value)                     # DXMI_EINVAL
        assert word in lib.dxmi_last_error(), (at, value, lib.dxmi_last_error())

    for at in (0, 1, 2, 3, 4, 5, 7, 8):
        refused(lib.dxmi_cd_huber_fwd, good_f, at, None, b"null pointer")
    for at in (0, 1, 2, 3, 4, 5, 6, 7, 9):
        refused(lib.dxmi_cd_huber_bwd, good_b, at, None, b"null pointer")
    for fn, good, (i_S, i_n, i_chw, i_c, i_ws) in ((lib.dxmi_cd_huber_fwd, good_f, (6, 9, 10, 11, 15)),
                                                  (lib.dxmi_cd_huber_bwd, good_b, (8, 10, 11, 12, 16))):
        for c in (0.0, -0.1, inf, -inf, nan):
            refused(fn, good, i_c, c, b"huber_c")
        for chw in (766, 0, -4):
            refused(fn, good, i_chw, chw, b"CHW")
        for S in (1, 0, -3):
            refused(fn, good, i_S, S, b"num_scales")
        for ws in (6, -1, 99):
            refused(fn, good, i_ws, ws, b"weight schedule")
        for n in (0, -1, 65536):
            refused(fn, good, i_n, n, b"N (")
        refused(fn, good, 2, p + 4, b"16-byte aligned")
    # DXMI_DSM_W_ICT stays unknown to every other entry point
    assert lib.dxmi_cd_loss_fwd(p, p, p, p, p, p, 18, p, 4, 3, 16, 16, 1, 0.5, 0.002, 0, 5, None) == -1
    assert b"weight schedule" in lib.dxmi_last_error()
    assert lib.dxmi_pd_loss_fwd(p, p, p, p, p, 6, p, 4, 768, 1, 0.5, 0.002, 0, 5, None) == -1
    assert b"weight schedule" in lib.dxmi_last_error()
    assert lib.dxmi_edm_dsm_loss_fwd(p, p, p, p, p, p, 4, 768, 0.5, 0.002, 0, 5, None) == -1
    assert b"weight schedule" in lib.dxmi_last_error()
