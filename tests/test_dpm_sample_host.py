"""DPM-Solver++ sampling of the DDPM teacher on the host (models/DxMI/dpm_sample.py): the table weights against float64 quadrature
of the integrals they stand for, the first-order rows against the merged DDIM / ancestral coefficients, the order of convergence on
an analytic network with a known probability-flow solution, the step spacing, the refusals, the parser of generate_cifar10.py and
dxmi_dpm_stage's argument checks under the host sanitizers (a stand-alone program, run as a child process).  No GPU.

There is no golden fixture: the reference tree has no such sampler.  The oracle is first principles in float64.
Order test, values computed when this test was written (relative error of the state after row S - 2 against the exact solution):
    order 1: 0.149 (S = 16), 0.0750 (S = 32), ratio 1.98;  order 2: 0.0451, 0.0106, ratio 4.26;  order 3: 7.98e-3, 6.2e-4, ratio 12.9."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from scipy.integrate import quad

from dxmi_hip import ops
from models.DxMI.ddpm_sample import ddpm_coefficients, ddpm_timesteps
from models.DxMI.dpm_sample import (DPMSampleSchedule, dpm_coefficients, dpm_orders, dpm_sample, dpm_timesteps, dpm_transition)
from models.DxMI.var_sampler import calc_diffusion_hyperparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODE, SDE = "dpmsolver++", "sde-dpmsolver++"


def alpha_bar64():
    """The fp32 table of calc_diffusion_hyperparams read into float64."""
    return calc_diffusion_hyperparams(1000, 1e-4, 0.02)["Alpha_bar"].to(torch.float32).numpy().astype(np.float64)


def analytic_net(x, t):
    return 0.8 * torch.tanh(0.9 * x + 1e-3 * t[:, None, None, None])


# ------------------------------------------------------------------------------------------ 1. quadrature
def lagrange(nodes, j):
    """L_j on `nodes`, written here from its definition."""
    def L(lam):
        v = 1.0
        for i, ni in enumerate(nodes):
            if i != j:
                v *= (lam - ni) / (nodes[j] - ni)
        return v
    return L


def quadrature_weights(ab, tau, algorithm, orders):
    """w_j of every row but the last by scipy quadrature of section 1's integrals -> [S - 1, 3] (zeros beyond a row's order)."""
    t = list(tau)[::-1]
    alpha, sigma = np.sqrt(ab[t]), np.sqrt(1 - ab[t])
    lam = np.log(alpha) - np.log(sigma)
    out = np.zeros((len(t) - 1, 3))
    for k in range(len(t) - 1):
        o = orders[k]
        nodes = [lam[k - j] for j in range(o)]
        lt, lp = lam[k], lam[k + 1]
        for j in range(o):
            L = lagrange(nodes, j)
            if algorithm == ODE:
                val, _ = quad(lambda u: np.exp(u) * L(u), lt, lp, epsabs=0, epsrel=1e-12)
                out[k, j] = sigma[k + 1] * val
            else:
                val, _ = quad(lambda u: np.exp(-2 * (lp - u)) * L(u), lt, lp, epsabs=0, epsrel=1e-12)
                out[k, j] = 2 * alpha[k + 1] * val
    return out


@pytest.mark.parametrize("algorithm,order", [(ODE, 1), (ODE, 2), (ODE, 3), (SDE, 1), (SDE, 2)])
@pytest.mark.parametrize("skip_type,S", [("logsnr", 10), ("uniform", 50)])
def test_exact_weights_against_quadrature(skip_type, S, algorithm, order):
    ab = alpha_bar64()
    sch = DPMSampleSchedule(S, order, algorithm, "exact", skip_type)
    assert sch.tau == dpm_timesteps(S, 1000, skip_type)
    co = dpm_coefficients(ab, sch.tau, algorithm, order, "exact")
    orders = dpm_orders(S, order)
    assert list(co["order"]) == orders and max(orders) == order
    want = quadrature_weights(ab, sch.tau, algorithm, orders)
    got = np.stack([co["w0"], co["w1"], co["w2"]], axis=1)
    scale = np.abs(want).max(axis=1, keepdims=True)
    worst = (np.abs(got[:-1] - want) / scale).max()
    print(f"{algorithm} order {order} {skip_type} S={S}: worst |w - quadrature| / max_j |w_j| = {worst:.3e}")
    assert worst <= 1e-6
    for k in range(S - 1):           # a weight beyond the row's order is exactly 0, one within it is not
        assert [got[k, j] != 0 for j in range(3)] == [j < orders[k] for j in range(3)]
    # the other scalars of section 1, restated
    t = sch.tau[::-1]
    alpha, sigma = np.sqrt(ab[t]), np.sqrt(1 - ab[t])
    h = np.diff(np.log(alpha) - np.log(sigma))
    assert (h > 0).all()
    ratio = sigma[1:] / sigma[:-1]
    if algorithm == ODE:
        assert np.allclose(co["cx"][:-1], ratio, rtol=1e-13, atol=0) and (co["s"] == 0).all()
    else:
        assert np.allclose(co["cx"][:-1], ratio * np.exp(-h), rtol=1e-13, atol=0)
        assert np.allclose(co["s"][:-1], sigma[1:] * np.sqrt(1 - np.exp(-2 * h)), rtol=1e-12, atol=0) and co["s"][-1] == 0
    assert np.allclose(co["a"], 1 / alpha, rtol=1e-15) and np.allclose(co["b"], sigma / alpha, rtol=1e-15)
    assert (co["cx"][-1], co["w0"][-1], co["w1"][-1], co["w2"][-1]) == (0, 1, 0, 0)          # the denoise row
    # the fp32 table is the float64 value rounded once
    tab = sch.table.numpy()
    assert tab.dtype == np.float32 and tab.shape == (S, ops.MT_COLS)
    for col, key in ((ops.MT_CX, "cx"), (ops.MT_W0, "w0"), (ops.MT_W1, "w1"), (ops.MT_W2, "w2"), (ops.MT_S, "s"), (ops.MT_A, "a"),
                     (ops.MT_B, "b")):
        assert np.array_equal(tab[:, col], co[key].astype(np.float32)), key
    assert tab[:, ops.MT_T].tolist() == [float(v) for v in t] and tab[:-1, ops.MT_T_NEXT].tolist() == tab[1:, ops.MT_T].tolist()
    assert tab[:, ops.MT_FLAGS].tolist() == [1.0] * (S - 1) + [3.0] and tab[:, ops.MT_ORDER].tolist() == [float(o) for o in orders]
    assert sch.draws == [algorithm == SDE] * (S - 1) + [False]


def test_orientation_row():
    """uniform S = 10, order 3, exact: the row from t = 600 to t = 500."""
    tau = ddpm_timesteps(10)
    co = dpm_coefficients(alpha_bar64(), tau, ODE, 3, "exact")
    k = tau[::-1].index(600)
    assert tau[::-1][k + 1] == 500 and co["order"][k] == 3
    assert np.allclose([co["w0"][k], co["w1"][k], co["w2"][k]], [0.2272, -0.1429, 0.0391], rtol=0, atol=5e-5)


@pytest.mark.parametrize("algorithm", [ODE, SDE])
def test_midpoint_changes_the_second_order_rows_only(algorithm):
    ab = alpha_bar64()
    order = 3 if algorithm == ODE else 2
    tau = dpm_timesteps(10)
    mid, exact = (dpm_coefficients(ab, tau, algorithm, order, st) for st in ("midpoint", "exact"))
    t = tau[::-1]
    lam = 0.5 * (np.log(ab[t]) - np.log1p(-ab[t]))
    rows2 = [k for k, o in enumerate(mid["order"]) if o == 2]
    assert rows2 and list(mid["order"]) == list(exact["order"])
    for k in range(10):
        same = all(mid[c][k] == exact[c][k] for c in ("w0", "w1", "w2"))
        assert same == (k not in rows2)
        assert all(mid[c][k] == exact[c][k] for c in ("cx", "s", "a", "b"))
    for k in rows2:
        h = lam[k + 1] - lam[k]
        r = (lam[k] - lam[k - 1]) / h
        gain = np.sqrt(ab[t[k + 1]]) * (1 - np.exp(-h if algorithm == ODE else -2 * h))
        assert np.isclose(mid["w0"][k], gain * (1 + 1 / (2 * r)), rtol=1e-13) and np.isclose(mid["w1"][k], -gain / (2 * r), rtol=1e-13)
        assert mid["w2"][k] == 0
        # both are second-order rules: their weights sum to the first-order weight
        assert np.isclose(mid["w0"][k] + mid["w1"][k], exact["w0"][k] + exact["w1"][k], rtol=1e-12)


def test_small_h_moments_are_stable():
    """Adjacent steps (h ~ 5e-3): the third-order weights against quadrature to the same 1e-6."""
    ab = alpha_bar64()
    tau = list(range(300, 306))
    for algorithm, order in ((ODE, 3), (SDE, 2)):
        co = dpm_coefficients(ab, tau, algorithm, order, "exact", lower_order_final=False)
        orders = dpm_orders(len(tau), order, False)
        want = quadrature_weights(ab, tau, algorithm, orders)
        got = np.stack([co["w0"], co["w1"], co["w2"]], axis=1)[:-1]
        assert (np.abs(got - want) <= 1e-9 * np.abs(want).max(axis=1, keepdims=True)).all()


# ------------------------------------------------------------------------------------------ 2. identities with merged code
@pytest.mark.parametrize("tau", [ddpm_timesteps(10), ddpm_timesteps(50), ddpm_timesteps(20, 1000, "quad"), dpm_timesteps(10)])
def test_first_order_rows_are_the_merged_samplers(tau):
    ab = alpha_bar64()
    rel = lambda got, want: np.abs(got - want).max() / np.abs(want).max()
    ode, ddim = dpm_coefficients(ab, tau, ODE, 1), ddpm_coefficients(ab, tau, eta=0.0)
    e = [rel(ode["cx"], ddim["c1"] * ddim["r"]), rel(ode["w0"], ddim["c0"] - ddim["c1"] * ddim["q"] * ddim["r"])]
    sde, anc = dpm_coefficients(ab, tau, SDE, 1), ddpm_coefficients(ab, tau, eta=1.0, variance="small")
    e += [rel(sde["cx"], anc["c1"] * anc["r"]), rel(sde["w0"], anc["c0"] - anc["c1"] * anc["q"] * anc["r"]), rel(sde["s"], anc["sigma"] * (anc["s"] != 0))]
    print(f"first-order rows vs ddpm_coefficients, S = {len(tau)}: worst relative differences {['%.1e' % v for v in e]}")
    assert max(e) <= 1e-12
    assert np.array_equal(sde["s"] != 0, anc["s"] != 0) and rel(sde["s"], anc["s"]) <= 1e-12
    assert rel(ode["a"], ddim["a"]) <= 1e-15 and rel(ode["b"], ddim["b"]) <= 1e-12


# ------------------------------------------------------------------------------------------ 3. order
def flow_error(order, S):
    """Relative error at tau_0 of the float64 torch path on eps(x, t) = sigma_t x / (0.25 ab_t + 1 - ab_t): data N(0, 0.25), whose
    probability-flow solution is x_t proportional to sqrt(0.25 ab_t + 1 - ab_t)."""
    ab = torch.from_numpy(alpha_bar64())
    var = lambda t: 0.25 * ab[t] + 1 - ab[t]

    def net(x, t):
        assert x.dtype == torch.float64
        a = ab[t.long()][:, None, None, None]
        return (1 - a).sqrt() * x / (0.25 * a + 1 - a)

    tau = dpm_timesteps(S)
    x_T = torch.tensor([1.0, -0.5, 2.0, 0.25], dtype=torch.float64).reshape(2, 1, 1, 2)
    seen = []
    dpm_sample(net, x_T.shape, steps=S, order=order, solver_type="exact", skip_type="logsnr", lower_order_final=True, clip_denoised=False,
               device="cpu", noise=[x_T] + [None] * S, callback=lambda d: seen.append(d))
    assert [d["i"] for d in seen] == list(range(S)) and [d["t"] for d in seen] == tau[::-1]
    got = seen[S - 2]["x"]
    assert got.dtype == torch.float64
    exact = x_T * (var(tau[0]) / var(tau[-1])).sqrt()
    return ((got - exact).abs() / exact.abs()).max().item()


def test_order_of_convergence():
    e = {(o, S): flow_error(o, S) for o in (1, 2, 3) for S in (16, 32)}
    ratio = {o: e[o, 16] / e[o, 32] for o in (1, 2, 3)}
    for o in (1, 2, 3):
        print(f"order {o}: error {e[o, 16]:.4e} (S = 16), {e[o, 32]:.4e} (S = 32), ratio {ratio[o]:.3f}")
    assert 1.6 <= ratio[1] <= 2.4
    assert ratio[2] >= 3
    assert ratio[3] >= 6
    assert e[2, 32] <= e[1, 32] / 4 and e[3, 32] <= e[2, 32] / 8


# ------------------------------------------------------------------------------------------ 4. spacing and refusals
def test_logsnr_steps():
    tau = dpm_timesteps(10)
    assert tau[:6] == [0, 5, 22, 73, 202, 410] and tau[-1] == 999 and len(tau) == 10
    assert dpm_timesteps(10, 1000, "logsnr", 1e-4, 0.02) == tau
    for S in (4, 5, 8, 10, 16, 20, 24, 32):
        tau = dpm_timesteps(S)
        assert len(tau) == S and tau[0] == 0 and tau[-1] == 999 and all(b > a for a, b in zip(tau, tau[1:]))
        assert all(isinstance(t, int) for t in tau)
        # nearest in lambda, restated by brute force (a tie: the lowest index)
        ab = alpha_bar64()
        lam = 0.5 * (np.log(ab) - np.log1p(-ab))
        assert tau == [int(np.argmin(np.abs(lam - v))) for v in np.linspace(lam[0], lam[-1], S)]
    gaps = np.diff(dpm_timesteps(10))
    assert gaps[0] < gaps[4]                   # dense where the log-SNR moves fast


def test_delegated_spacings_are_ddpm_timesteps():
    assert dpm_timesteps(10, 1000, "uniform") == ddpm_timesteps(10, 1000, "uniform")
    assert dpm_timesteps(20, 1000, "quad") == ddpm_timesteps(20, 1000, "quad")
    with pytest.raises(ValueError, match="largest S that works is 29"):
        dpm_timesteps(200, 1000, "quad")


def test_step_refusals():
    with pytest.raises(ValueError, match=r"largest S that works is (\d+)") as info:
        dpm_timesteps(50)
    largest = int(str(info.value).rsplit(" ", 1)[1])
    assert largest >= 32
    assert len(dpm_timesteps(largest)) == largest
    for S in (0, 1, 1001):
        with pytest.raises(ValueError):
            dpm_timesteps(S)
    with pytest.raises(ValueError, match="skip_type"):
        dpm_timesteps(10, 1000, "cosine")


def test_mode_refusals():
    ab, tau = alpha_bar64(), dpm_timesteps(8)
    for bad in (0, 4, -1, 2.5, True):
        with pytest.raises(ValueError, match="order"):
            dpm_coefficients(ab, tau, ODE, bad)
    with pytest.raises(ValueError, match="orders 1 and 2"):
        dpm_coefficients(ab, tau, SDE, 3)
    with pytest.raises(ValueError, match="algorithm"):
        dpm_coefficients(ab, tau, "dpmsolver", 2)
    with pytest.raises(ValueError, match="solver_type"):
        dpm_coefficients(ab, tau, ODE, 2, "heun")
    kw = dict(device="cpu")
    with pytest.raises(ValueError, match="orders 1 and 2"):
        dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, order=3, algorithm=SDE, **kw)
    with pytest.raises(ValueError, match="order"):
        dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, order=4, **kw)
    with pytest.raises(ValueError, match="algorithm"):
        dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, algorithm="unipc", **kw)
    with pytest.raises(ValueError, match="solver_type"):
        dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, solver_type="bh1", **kw)
    with pytest.raises(ValueError, match="skip_type"):
        dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, skip_type="karras", **kw)
    with pytest.raises(ValueError, match="largest S"):
        dpm_sample(analytic_net, (2, 3, 8, 8), steps=50, **kw)
    with pytest.raises(ValueError, match="7 draws"):
        dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, noise=[torch.zeros(2, 3, 8, 8)] * 6, **kw)


def test_order_pattern():
    assert dpm_orders(5, 3) == [1, 2, 3, 2, 1]
    assert dpm_orders(5, 3, lower_order_final=False) == [1, 2, 3, 3, 1]          # the denoise row is first order always
    assert dpm_orders(10, 2) == [1] + [2] * 8 + [1]
    assert dpm_orders(10, 2, False) == [1] + [2] * 8 + [1]
    assert dpm_orders(10, 1) == [1] * 10
    assert dpm_orders(2, 3) == [1, 1] and dpm_orders(3, 3) == [1, 2, 1] and dpm_orders(4, 3) == [1, 2, 2, 1]
    sch = DPMSampleSchedule(5, 3)
    assert sch.table[:, ops.MT_ORDER].tolist() == [1, 2, 3, 2, 1]
    assert [(float(r[ops.MT_W1]) != 0, float(r[ops.MT_W2]) != 0) for r in sch.table] == \
        [(False, False), (True, False), (True, True), (True, False), (False, False)]
    last = sch.table[-1]
    assert last[ops.MT_CX] == 0 and last[ops.MT_W0] == 1 and last[ops.MT_S] == 0 and int(last[ops.MT_FLAGS]) == 3 and last[ops.MT_T] == 0


def test_hip_model_is_refused_on_the_cpu():
    from dxmi_hip import DxmiError
    from models.DxMI.unet_small import Model
    net = Model(ch=32, out_ch=3, ch_mult=(1,), num_res_blocks=1, attn_resolutions=[], dropout=0.0, in_channels=3, resolution=8)
    with pytest.raises(DxmiError):
        dpm_sample(net, (1, 3, 8, 8), steps=4, device="cpu")


# ------------------------------------------------------------------------------------------ the torch path
class CountingGenerator:
    def __init__(self):
        self.randn_calls = self.randn_like_calls = 0
        self.gen = torch.Generator().manual_seed(11)

    def randn(self, *size, device=None, dtype=torch.float32):
        self.randn_calls += 1
        return torch.randn(*size, generator=self.gen)

    def randn_like(self, x):
        self.randn_like_calls += 1
        return torch.randn(x.shape, generator=self.gen)


def test_draw_counts_and_recorded_noise():
    g = CountingGenerator()
    out = dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, order=3, device="cpu", generator=g)
    assert (g.randn_calls, g.randn_like_calls) == (1, 0) and out.shape == (2, 3, 8, 8) and out.abs().max() <= 1
    g = CountingGenerator()
    a = dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, algorithm=SDE, device="cpu", generator=g)
    assert (g.randn_calls, g.randn_like_calls) == (1, 5)            # the denoise row adds no noise
    gen = torch.Generator().manual_seed(11)
    noise = [torch.randn(2, 3, 8, 8, generator=gen) for _ in range(6)] + [torch.full((2, 3, 8, 8), float("nan"))]
    assert torch.equal(dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, algorithm=SDE, device="cpu", noise=noise), a)


def test_transition_reads_no_history_where_the_weight_is_zero():
    sch = DPMSampleSchedule(6, 3, clip_denoised=True)
    gen = torch.Generator().manual_seed(2)
    x, eps = torch.randn(2, 3, 4, 4, generator=gen), torch.randn(2, 3, 4, 4, generator=gen)
    nan = torch.full_like(x, float("nan"))
    got, d0 = dpm_transition(x, eps, None, sch.table[0], (nan, nan))
    assert torch.isfinite(got).all() and d0.abs().max() <= 1
    got, _ = dpm_transition(x, eps, None, sch.table[1], (x, nan))
    assert torch.isfinite(got).all()
    got, _ = dpm_transition(x, eps, None, sch.table[2], (x, nan))
    assert torch.isnan(got).all()
    row = sch.table[2].double()
    want = row[ops.MT_CX] * x.double() + row[ops.MT_W0] * (row[ops.MT_A] * x.double() - row[ops.MT_B] * eps.double()).clamp(-1, 1) \
        + row[ops.MT_W1] * eps.double() + row[ops.MT_W2] * x.double()
    got, _ = dpm_transition(x.double(), eps.double(), None, row, (eps.double(), x.double()))
    assert (got - want).abs().max() <= 1e-14


def test_first_order_loop_is_ddim():
    """Order 1 on uniform steps and DDIM are the same map: the two torch paths agree to fp32 rounding over six transitions."""
    from models.DxMI.ddpm_sample import ddpm_sample
    gen = torch.Generator().manual_seed(5)
    noise = [torch.randn(3, 3, 8, 8, generator=gen)] + [None] * 6
    a = dpm_sample(analytic_net, (3, 3, 8, 8), steps=6, order=1, skip_type="uniform", device="cpu", noise=noise)
    b = ddpm_sample(analytic_net, (3, 3, 8, 8), steps=6, eta=0.0, device="cpu", noise=noise)
    assert (a - b).abs().max() <= 1e-4 and a.std() > 0.1


# ------------------------------------------------------------------------------------------ command line
def test_generate_cifar10_parser():
    import generate_cifar10 as gc
    base = ["--log_dir", "x", "--teacher_ckpt", "ema.pt"]
    args = gc.parse_args(base + ["--solver", "dpmpp"])
    assert (args.solver, args.ddpm_steps, args.solver_order, args.solver_type, args.no_lower_order_final, args.skip_type, args.no_clip,
            args.generator) == ("dpmpp", 10, 2, "midpoint", False, "logsnr", False, "dummy")
    args = gc.parse_args(base + ["--solver", "sde-dpmpp", "--ddpm_steps", "20", "--solver_order", "1", "--solver_type", "exact",
                                 "--no_lower_order_final", "--skip_type", "uniform", "--generator", "determ", "--no_clip"])
    assert (args.solver, args.ddpm_steps, args.solver_order, args.solver_type, args.no_lower_order_final, args.skip_type, args.no_clip,
            args.generator) == ("sde-dpmpp", 20, 1, "exact", True, "uniform", True, "determ")
    assert gc.parse_args(base + ["--solver", "dpmpp", "--solver_order", "3", "--skip_type", "logsnr", "--ddpm_steps", "6"]).solver_order == 3
    # without the new flags: the namespace of before
    args = gc.parse_args(base)
    assert (args.ddpm_steps, args.eta, args.variance, args.skip_type, args.no_clip, args.generator, args.config) == \
        (1000, 1.0, "small", "uniform", False, "dummy", None)
    assert args.solver == "ancestral" and args.solver_order is None and args.solver_type is None and not args.no_lower_order_final
    assert gc.parse_args(base + ["--solver", "ancestral", "--eta", "0", "--ddpm_steps", "50"]).eta == 0.0
    args = gc.parse_args(["--log_dir", "x", "--synthetic", "cifar10_T10"])
    assert args.teacher_ckpt is None and args.solver is None and args.solver_order is None and args.skip_type is None
    rejected = [
        ["--log_dir", "x", "--solver", "dpmpp"], ["--log_dir", "x", "--solver_order", "2"], ["--log_dir", "x", "--solver_type", "exact"],
        ["--log_dir", "x", "--no_lower_order_final"], ["--log_dir", "x", "--skip_type", "logsnr"],         # only with --teacher_ckpt
        base + ["--skip_type", "logsnr"], base + ["--solver", "ancestral", "--skip_type", "logsnr"],        # logsnr needs a dpm solver
        base + ["--solver_order", "2"], base + ["--solver_type", "exact"], base + ["--no_lower_order_final"],
        base + ["--solver", "dpmpp", "--eta", "0"], base + ["--solver", "sde-dpmpp", "--eta", "1"],
        base + ["--solver", "dpmpp", "--variance", "small"], base + ["--solver", "sde-dpmpp", "--variance", "large"],
        base + ["--solver", "sde-dpmpp", "--solver_order", "3"], base + ["--solver", "dpmpp", "--solver_order", "4"],
        base + ["--solver", "unipc"], base + ["--solver", "dpmpp", "--solver_type", "heun"],
        base + ["--solver", "dpmpp", "--ddpm_steps", "50"], base + ["--solver", "dpmpp", "--ddpm_steps", "1"],
        base + ["--solver", "dpmpp", "--guidance_scale", "1.0"],
    ]
    for flags in rejected:
        with pytest.raises(SystemExit):
            gc.parse_args(flags)
            pytest.fail(f"{flags} was accepted")


# ------------------------------------------------------------------------------------------ 5. host sanitizers
def test_dpm_stage_arguments_under_address_and_ub_sanitizers():
    """`make asan_dpm` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_dpm.c, a program with its own main, against it and a no-device HIP runtime stub.  Null, misaligned and
    out-of-range arguments must each come back as DXMI_EINVAL with the message of their check: no crash, no sanitizer report.  The
    program runs as a child process; nothing is loaded into python.  A host-only build: machines without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_dpm"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_dpm")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") >= 30
