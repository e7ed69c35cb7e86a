"""DPM-Solver++ on the EDM nets, host side (no GPU): models/cm/dpm_sample.py's coefficients against the closed forms and a float64
quadrature written here, the ladders, the table's columns against KarrasSchedule's, the order of convergence on a problem with a
known solution, the torch path on the CPU, generate_large.py's parser and dxmi_edm_dpm_stage's argument checks under the host
sanitizers.

The EDM parametrisation: alpha = 1, sigma_t = sigma, lambda = -ln sigma, h = ln(sigma_t / sigma_p).
  ODE  x' = (sigma_p / sigma_t) x + sum_j w_j D_{k-j},               w_j = sigma_p int_{lambda_t}^{lambda_p} e^lambda L_j dlambda
  SDE  x' = (sigma_p / sigma_t) e^-h x + sum_j w_j D_{k-j} + sigma_p sqrt(1 - e^-2h) z,
                                                                      w_j = 2 int_{lambda_t}^{lambda_p} e^{-2 (lambda_p - lambda)} L_j dlambda
The quadrature is Gauss-Legendre with 48 nodes on [lambda_t, lambda_p]: the integrands are an exponential times a polynomial of degree
<= 2 over h <= 1.6, which 48 nodes integrate to rounding."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from numpy.polynomial.legendre import leggauss

from dxmi_hip import ops
from models.cm.dpm_sample import (EDMDPMSchedule, edm_dpm_coefficients, edm_dpm_sample, edm_dpm_schedule, edm_dpm_transition,
                                  edm_sigmas)
from models.cm.karras_diffusion import KarrasDenoiser, KarrasSchedule, get_sigmas_karras
from models.DxMI.dpm_sample import dpm_orders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODE, SDE = "dpmsolver++", "sde-dpmsolver++"
MODES = [(ODE, 1), (ODE, 2), (ODE, 3), (SDE, 1), (SDE, 2)]
DIFFUSION = KarrasDenoiser()


def ladder64(S, skip_type="karras", **kw):
    """The fp32 ladder read into float64: what the coefficients are computed from."""
    return edm_sigmas(S, skip_type=skip_type, **kw).numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------ 1. the formulas
def test_first_order_ode_is_the_euler_step():
    """x' = x + (x - D) (sigma_p - sigma_t) / sigma_t = (sigma_p / sigma_t) x + (1 - sigma_p / sigma_t) D: sample_euler's map."""
    sig = ladder64(10)
    co = edm_dpm_coefficients(sig, ODE, 1)
    e_sum, e_cx = np.abs(co["cx"][:-1] + co["w0"][:-1] - 1).max(), np.abs(co["cx"][:-1] - sig[1:] / sig[:-1]).max()
    print(f"order-1 ODE, 10 karras steps: |cx + w0 - 1| <= {e_sum:.2e}, |cx - sigma_p / sigma_t| <= {e_cx:.2e}")
    assert e_sum <= 1e-15 and e_cx <= 1e-15
    assert (co["s"] == 0).all() and (co["w1"] == 0).all() and (co["w2"] == 0).all() and list(co["order"]) == [1] * 10


def test_first_order_sde_keeps_the_variance():
    """A state of variance sigma_t^2 around D leaves the row with variance sigma_p^2."""
    sig = ladder64(10)
    co = edm_dpm_coefficients(sig, SDE, 1)
    rel = (np.abs(co["cx"][:-1] ** 2 * sig[:-1] ** 2 + co["s"][:-1] ** 2 - sig[1:] ** 2) / sig[1:] ** 2).max()
    print(f"order-1 SDE, 10 karras steps: |cx^2 sigma_t^2 + s^2 - sigma_p^2| / sigma_p^2 <= {rel:.2e}")
    assert rel <= 1e-14
    h = np.log(sig[:-1] / sig[1:])
    assert np.allclose(co["cx"][:-1], sig[1:] / sig[:-1] * np.exp(-h), rtol=1e-13, atol=0)
    assert np.allclose(co["s"][:-1], sig[1:] * np.sqrt(1 - np.exp(-2 * h)), rtol=1e-12, atol=0) and co["s"][-1] == 0


@pytest.mark.parametrize("skip_type", ["karras", "logsnr"])
@pytest.mark.parametrize("algorithm", [ODE, SDE])
def test_midpoint_rows_are_the_closed_forms(algorithm, skip_type):
    order = 3 if algorithm == ODE else 2
    sig = ladder64(10, skip_type)
    lam = -np.log(sig)
    mid, exact = (edm_dpm_coefficients(sig, algorithm, order, st) for st in ("midpoint", "exact"))
    rows2 = [k for k, o in enumerate(mid["order"]) if o == 2]
    assert rows2 and list(mid["order"]) == list(exact["order"]) == dpm_orders(10, order)
    for k in range(10):
        assert all(mid[c][k] == exact[c][k] for c in ("w0", "w1", "w2")) == (k not in rows2)
        assert all(mid[c][k] == exact[c][k] for c in ("cx", "s"))
    for k in rows2:
        h = lam[k + 1] - lam[k]
        r = (lam[k] - lam[k - 1]) / h
        gain = 1 - np.exp(-h if algorithm == ODE else -2 * h)                  # alpha_p = 1
        assert np.isclose(mid["w0"][k], gain * (1 + 1 / (2 * r)), rtol=1e-13, atol=0)
        assert np.isclose(mid["w1"][k], -gain / (2 * r), rtol=1e-13, atol=0) and mid["w2"][k] == 0
        assert np.isclose(mid["w0"][k] + mid["w1"][k], exact["w0"][k] + exact["w1"][k], rtol=1e-12, atol=0)


def quadrature_weights(sig, algorithm, orders):
    """w_j of every row but the last by Gauss-Legendre quadrature of the docstring's integrals -> [S - 1, 3]."""
    nodes_x, nodes_w = leggauss(48)
    lam = -np.log(sig)
    out = np.zeros((len(sig) - 1, 3))
    for k in range(len(sig) - 1):
        o, lt, lp = orders[k], lam[k], lam[k + 1]
        u = 0.5 * (lp - lt) * nodes_x + 0.5 * (lp + lt)
        for j in range(o):
            L = np.ones_like(u)
            for i in range(o):
                if i != j:
                    L = L * (u - lam[k - i]) / (lam[k - j] - lam[k - i])
            f = np.exp(u) * L * sig[k + 1] if algorithm == ODE else 2 * np.exp(-2 * (lp - u)) * L
            out[k, j] = 0.5 * (lp - lt) * np.sum(nodes_w * f)
    return out


@pytest.mark.parametrize("algorithm,order", MODES)
@pytest.mark.parametrize("skip_type,S", [("karras", 10), ("logsnr", 10), ("karras", 40)])
def test_exact_weights_against_quadrature(skip_type, S, algorithm, order):
    sig = ladder64(S, skip_type)
    co = edm_dpm_coefficients(sig, algorithm, order, "exact")
    orders = dpm_orders(S, order)
    assert list(co["order"]) == orders and max(orders) == order
    want = quadrature_weights(sig, algorithm, orders)
    got = np.stack([co["w0"], co["w1"], co["w2"]], axis=1)
    worst = (np.abs(got[:-1] - want) / np.abs(want).max(axis=1, keepdims=True)).max()
    print(f"{algorithm} order {order} {skip_type} S={S}: worst |w - quadrature| / max_j |w_j| = {worst:.3e}")
    assert worst <= 1e-12
    for k in range(S - 1):           # a weight beyond the row's order is exactly 0, one within it is not
        assert [got[k, j] != 0 for j in range(3)] == [j < orders[k] for j in range(3)]
    assert (co["cx"][-1], co["w0"][-1], co["w1"][-1], co["w2"][-1], co["s"][-1]) == (0, 1, 0, 0, 0)        # the denoise row


def test_the_ddpm_coefficients_keep_their_bits():
    """multistep_coefficients is dpm_coefficients' loop moved, not rewritten: the DDPM schedule's float64 values restated here."""
    from models.DxMI.dpm_sample import dpm_coefficients, dpm_timesteps
    from models.DxMI.var_sampler import calc_diffusion_hyperparams
    ab = calc_diffusion_hyperparams(1000, 1e-4, 0.02)["Alpha_bar"].to(torch.float32).numpy().astype(np.float64)
    tau = dpm_timesteps(10)
    co = dpm_coefficients(ab, tau, ODE, 1)
    t = tau[::-1]
    alpha, sigma = np.sqrt(ab[t]), np.sqrt(1 - ab[t])
    assert np.array_equal(co["a"], 1.0 / alpha) and np.array_equal(co["b"], sigma / alpha)
    assert np.array_equal(co["cx"][:-1], sigma[1:] / sigma[:-1]) and set(co) == {"cx", "w0", "w1", "w2", "s", "a", "b", "order"}


# ------------------------------------------------------------------------------------------ 2. ladders and the table
def test_ladders():
    for S in (2, 4, 10, 40):
        assert torch.equal(edm_sigmas(S), get_sigmas_karras(S, 0.002, 80.0, 7.0)[:-1])
        assert torch.equal(edm_sigmas(S, 0.01, 50.0, 5.0), get_sigmas_karras(S, 0.01, 50.0, 5.0)[:-1])
        for skip_type in ("karras", "logsnr"):
            sig = edm_sigmas(S, skip_type=skip_type)
            assert sig.dtype == torch.float32 and sig.shape == (S,) and bool((sig[1:] < sig[:-1]).all()) and sig[-1] > 0
        log = edm_sigmas(S, skip_type="logsnr")
        assert log[0].item() == np.float32(80.0) and log[-1].item() == np.float32(0.002)
        assert np.allclose(np.diff(np.log(log.double().numpy())), np.log(0.002 / 80.0) / (S - 1), rtol=1e-5)
    for name in ("uniform", "quad"):
        with pytest.raises(ValueError, match=name):
            edm_sigmas(10, skip_type=name)
        with pytest.raises(ValueError, match=name):
            edm_dpm_schedule(DIFFUSION, 10, skip_type=name)
    for bad in (dict(steps=1), dict(steps=10, skip_type="linear"), dict(steps=10, sigma_min=0.0), dict(steps=10, sigma_min=90.0)):
        with pytest.raises(ValueError):
            edm_sigmas(**bad)


@pytest.mark.parametrize("algorithm,order", MODES)
@pytest.mark.parametrize("skip_type", ["karras", "logsnr"])
def test_table_columns(skip_type, algorithm, order):
    S = 10
    sch = EDMDPMSchedule(DIFFUSION, S, order, algorithm, "midpoint", skip_type)
    tab = sch.table
    assert tab.dtype == torch.float32 and tab.shape == (S, ops.ET_COLS)
    sig = sch.sigmas
    assert torch.equal(sig, edm_sigmas(S, skip_type=skip_type)) and torch.equal(tab[:, ops.ET_SIGMA], sig)
    assert bool((sig[1:] < sig[:-1]).all())
    # the fp32 table is the float64 value on the fp32 ladder, rounded once
    co = edm_dpm_coefficients(sig.numpy().astype(np.float64), algorithm, order, "midpoint")
    for col, key in ((ops.ET_CX, "cx"), (ops.ET_W0, "w0"), (ops.ET_W1, "w1"), (ops.ET_W2, "w2"), (ops.ET_S, "s")):
        assert np.array_equal(tab[:, col].numpy(), co[key].astype(np.float32)), key
    orders = dpm_orders(S, order)
    assert tab[:, ops.ET_ORDER].tolist() == [float(o) for o in orders]
    for k in range(S):
        assert [bool(tab[k, c] != 0) for c in (ops.ET_W1, ops.ET_W2)] == [orders[k] >= 2, orders[k] >= 3]
    assert tab[-1, [ops.ET_CX, ops.ET_W0, ops.ET_W1, ops.ET_W2, ops.ET_S]].tolist() == [0, 1, 0, 0, 0]
    assert tab[:, ops.ET_FLAGS].tolist() == [1.0] * (S - 1) + [3.0]
    assert EDMDPMSchedule(DIFFUSION, S, order, algorithm, clip_denoised=False).table[:, ops.ET_FLAGS].tolist() == [0.0] * (S - 1) + [2.0]
    assert sch.draws == [algorithm == SDE] * (S - 1) + [False] and sch.n_draws == (S - 1) * (algorithm == SDE)
    # the preconditioning: KarrasSchedule's Euler rows on the same ladder (launch 0 is FIRST, launch k + 1 follows evaluation k)
    ks = KarrasSchedule(torch.cat([sig, sig.new_zeros(1)]), "euler", DIFFUSION, x_scale=80.0)
    assert torch.equal(tab[:, ops.ET_CIN], ks.table[:S, ops.KT_CIN]) and torch.equal(tab[:, ops.ET_T], ks.table[:S, ops.KT_T])
    assert torch.equal(tab[:-1, ops.ET_CIN_NEXT], ks.table[1:S, ops.KT_CIN]) and torch.equal(tab[:-1, ops.ET_T_NEXT], ks.table[1:S, ops.KT_T])
    assert torch.equal(tab[:, ops.ET_CSKIP], ks.table[1:, ops.KT_CSKIP]) and torch.equal(tab[:, ops.ET_COUT], ks.table[1:, ops.KT_COUT])
    assert torch.equal(tab[:, ops.ET_XSCALE], ks.table[:S, ops.KT_XSCALE]) and tab[0, ops.ET_XSCALE].item() == 80.0
    assert tab[-1, ops.ET_T_NEXT] == 0 and tab[-1, ops.ET_CIN_NEXT] == 0
    c_skip, c_out, c_in = DIFFUSION.get_scalings(sig)
    assert torch.equal(tab[:, ops.ET_CSKIP], c_skip) and torch.equal(tab[:, ops.ET_COUT], c_out) and torch.equal(tab[:, ops.ET_CIN], c_in)


def test_schedule_is_memoised_and_refuses():
    a, b = edm_dpm_schedule(DIFFUSION, 10, 2), edm_dpm_schedule(KarrasDenoiser(), 10, 2)
    assert a is b and a is not edm_dpm_schedule(DIFFUSION, 10, 3) and a is not edm_dpm_schedule(KarrasDenoiser(sigma_data=1.0), 10, 2)
    assert edm_dpm_schedule(DIFFUSION, 10, 2, skip_type="logsnr", rho=3.0) is edm_dpm_schedule(DIFFUSION, 10, 2, skip_type="logsnr")
    with pytest.raises(NotImplementedError, match="distillation"):
        edm_dpm_schedule(KarrasDenoiser(distillation=True), 10)
    with pytest.raises(NotImplementedError, match="distillation"):
        edm_dpm_sample(KarrasDenoiser(distillation=True), lambda x, t: x, (1, 1, 2, 2), device="cpu")
    for bad in (dict(algorithm="unipc"), dict(solver_type="heun"), dict(order=0), dict(order=4), dict(order=True),
                dict(algorithm=SDE, order=3)):
        with pytest.raises(ValueError):
            edm_dpm_schedule(DIFFUSION, 10, **bad)
    with pytest.raises(ValueError, match="fall"):
        edm_dpm_coefficients([80.0, 1.0, 1.0, 0.002])


# ------------------------------------------------------------------------------------------ 3. order of convergence
def gaussian_net(x_in, t):
    """F of the exact denoiser of data N(0, 0.25): D(x, sigma) = 0.25 / (0.25 + sigma^2) x, in float64 from the network's inputs."""
    assert x_in.dtype == torch.float64
    s = torch.exp(t / 250.0)[:, None, None, None]
    c_skip, c_out, c_in = 0.25 / (s ** 2 + 0.25), s * 0.5 / (s ** 2 + 0.25) ** 0.5, 1 / (s ** 2 + 0.25) ** 0.5
    x = x_in / c_in
    return (0.25 / (0.25 + s ** 2) * x - c_skip * x) / c_out


def flow_error(order, S, skip_type, solver_type):
    """Relative error after row S - 2 against the probability-flow solution x(sigma) = x_T sqrt((0.25 + sigma^2) / (0.25 +
    sigma_0^2)) at sigma_min, sigma from 80 down to 0.002."""
    x0 = torch.tensor([1.0, -0.5, 2.0, 0.25], dtype=torch.float64).reshape(2, 1, 1, 2)
    seen = []
    edm_dpm_sample(DIFFUSION, gaussian_net, x0.shape, steps=S, order=order, solver_type=solver_type, skip_type=skip_type,
                   clip_denoised=False, device="cpu", noise=[x0] + [None] * S, callback=seen.append)
    sch = edm_dpm_schedule(DIFFUSION, S, order, ODE, solver_type, skip_type, True, False)
    assert [d["i"] for d in seen] == list(range(S)) and [float(d["sigma"]) for d in seen] == sch.sigmas.tolist()
    got = seen[S - 2]["x"]
    assert got.dtype == torch.float64
    s0, s1 = float(sch.sigmas[0]), float(sch.sigmas[-1])
    exact = x0 * 80.0 * np.sqrt((0.25 + s1 ** 2) / (0.25 + s0 ** 2))
    return ((got - exact).abs() / exact.abs()).max().item()


@pytest.mark.parametrize("solver_type", ["midpoint", "exact"])
@pytest.mark.parametrize("skip_type", ["logsnr", "karras"])
def test_order_of_convergence(skip_type, solver_type):
    e = {(o, S): flow_error(o, S, skip_type, solver_type) for o in (1, 2, 3) for S in (40, 80)}
    ratio = {o: e[o, 40] / e[o, 80] for o in (1, 2, 3)}
    for o in (1, 2, 3):
        print(f"{skip_type} {solver_type} order {o}: error {e[o, 40]:.4e} (S = 40), {e[o, 80]:.4e} (S = 80), ratio {ratio[o]:.3f}")
    assert ratio[1] >= 1.8 and ratio[2] >= 3.5 and ratio[3] >= 7
    assert e[3, 80] < e[2, 80] < e[1, 80]


# ------------------------------------------------------------------------------------------ 4. the torch path
def analytic_net(x_in, t, y=None):
    out = 0.8 * torch.tanh(0.9 * x_in + 1e-3 * t[:, None, None, None])
    return out if y is None else out + 0.01 * y[:, None, None, None].to(out.dtype)


@pytest.mark.parametrize("algorithm,order", [(ODE, 3), (SDE, 2)])
def test_torch_path_on_the_cpu(algorithm, order):
    S, shape = 6, (3, 3, 8, 8)
    gen = torch.Generator().manual_seed(11)
    noise = [torch.randn(shape, generator=gen) for _ in range(S + 1)]
    kw = dict(steps=S, order=order, algorithm=algorithm, device="cpu")
    seen = []
    out = edm_dpm_sample(DIFFUSION, analytic_net, shape, noise=noise, callback=seen.append, **kw)
    assert out.dtype == torch.float32 and out.shape == shape and out.abs().max() <= 1 and out.std() > 0.05
    assert [d["i"] for d in seen] == list(range(S)) and torch.equal(out, seen[-1]["x"].clamp(-1, 1))
    assert torch.equal(seen[-1]["x"], seen[-1]["pred_xstart"]) and all(d["pred_xstart"].abs().max() <= 1 for d in seen)
    wide = edm_dpm_sample(DIFFUSION, analytic_net, shape, noise=[n.double() for n in noise], **kw)
    assert wide.dtype == torch.float64
    # fp32 rounding: the state is at most 80 and every row's map has gain <= ~2 on it, six rows
    assert (out.double() - wide).abs().max() <= 1e-4, (out.double() - wide).abs().max()
    # the labels reach the network, and only the labels are taken
    y = torch.tensor([1, 5, 9])
    assert not torch.equal(edm_dpm_sample(DIFFUSION, analytic_net, shape, noise=noise, model_kwargs={"y": y}, **kw), out)
    with pytest.raises(ValueError, match="model_kwargs"):
        edm_dpm_sample(DIFFUSION, analytic_net, shape, noise=noise, model_kwargs={"cond": y}, **kw)
    for n in (noise[:-1], noise + [noise[0]]):
        with pytest.raises(ValueError, match=f"{S + 1} draws"):
            edm_dpm_sample(DIFFUSION, analytic_net, shape, noise=n, **kw)
    # without noise= the draws are torch's (ODE: x_T alone) or the generator's
    torch.manual_seed(3)
    a = edm_dpm_sample(DIFFUSION, analytic_net, shape, **kw)
    torch.manual_seed(3)
    assert torch.equal(a, edm_dpm_sample(DIFFUSION, analytic_net, shape, **kw)) and a.abs().max() <= 1


def test_transition_reads_no_history_where_the_weight_is_zero():
    sch = edm_dpm_schedule(DIFFUSION, 6, 3)
    x, F = torch.randn(2, 3, 4, 4), torch.randn(2, 3, 4, 4)
    for k in (0, 4, 5):           # order 1, 2 (lowered), 1: hist shorter than two entries is never indexed past its order
        o = int(sch.table[k, ops.ET_ORDER])
        hist = [torch.randn_like(x)] * (o - 1)
        acc, d0 = edm_dpm_transition(x, F, None, sch.table[k], hist)
        assert torch.isfinite(acc).all() and d0.abs().max() <= 1
    row = sch.table[0]
    want = row[ops.ET_CX] * x + row[ops.ET_W0] * (row[ops.ET_COUT] * F + row[ops.ET_CSKIP] * x).clamp(-1, 1)
    assert torch.equal(edm_dpm_transition(x, F, torch.randn_like(x), row)[0], want)           # s == 0: z is not read


def test_hip_unet_is_refused_on_the_cpu():
    from dxmi_hip import DxmiError
    from models.cm.script_util import create_model_and_diffusion
    net, diffusion = create_model_and_diffusion(image_size=16, class_cond=False, learn_sigma=False, num_channels=64, num_res_blocks=1,
                                                channel_mult="1,2", num_heads=4, num_head_channels=64, num_heads_upsample=-1,
                                                attention_resolutions="8", dropout=0.0, use_checkpoint=False, use_scale_shift_norm=True,
                                                resblock_updown=True, use_fp16=False, use_new_attention_order=False,
                                                weight_schedule="uniform")
    with pytest.raises(DxmiError):
        edm_dpm_sample(diffusion, net, (1, 3, 16, 16), steps=3, device="cpu")


def test_karras_sample_and_its_lists_are_as_they_were():
    from models.cm import karras_diffusion as kd
    assert kd.KARRAS_SAMPLERS == ("heun", "dpm", "euler", "ancestral")
    assert [kd.karras_nfe(s, 5) for s in ("heun", "dpm", "euler", "ancestral", "progdist")] == [9, 10, 5, 5, 5]
    with pytest.raises(ValueError):
        kd.karras_sample(DIFFUSION, analytic_net, (1, 3, 8, 8), 5, sampler="dpmpp")


# ------------------------------------------------------------------------------------------ 5. command line
def test_generate_large_parser():
    import generate_large as gl
    base = ["--log_dir", "x", "--n_sample", "4"]
    args, _ = gl.parse_args(base + ["--karras_sampler", "dpmpp"])
    assert (args.karras_sampler, args.karras_steps, args.solver_order, args.solver_type, args.skip_type, args.no_lower_order_final, args.rho,
            args.generator, args.no_graph, args.pretrained) == ("dpmpp", 10, 2, "midpoint", "karras", False, 7.0, "dummy", False, None)
    args, _ = gl.parse_args(base + ["--karras_sampler", "sde-dpmpp", "--karras_steps", "4", "--solver_order", "1", "--solver_type", "exact",
                                    "--skip_type", "logsnr", "--no_lower_order_final", "--generator", "determ", "--seed", "1", "--no_graph",
                                    "--pretrained", "w.pt"])
    assert (args.karras_sampler, args.karras_steps, args.solver_order, args.solver_type, args.skip_type, args.no_lower_order_final,
            args.generator, args.seed, args.no_graph, args.pretrained) == ("sde-dpmpp", 4, 1, "exact", "logsnr", True, "determ", 1, True, "w.pt")
    assert gl.parse_args(base + ["--karras_sampler", "dpmpp", "--solver_order", "3", "--rho", "5"])[0].rho == 5.0
    assert gl.parse_args(base + ["--karras_sampler", "dpmpp", "--pretrained"])[0].pretrained == ""
    assert gl.DPM_SAMPLERS == {"dpmpp": ODE, "sde-dpmpp": SDE}
    # the other samplers' namespaces are as they were
    args, _ = gl.parse_args(base + ["--karras_sampler", "heun"])
    assert (args.karras_steps, args.rho, args.s_churn, args.s_noise, args.solver_order, args.skip_type) == (40, 7.0, 0.0, 1.0, None, None)
    args, _ = gl.parse_args(base)
    assert args.karras_sampler is None and args.karras_steps is None and args.solver_order is None and not args.no_lower_order_final
    rejected = [
        base + ["--solver_order", "2"], base + ["--solver_type", "exact"], base + ["--skip_type", "logsnr"], base + ["--no_lower_order_final"],
        base + ["--karras_sampler", "heun", "--solver_order", "2"], base + ["--karras_sampler", "euler", "--skip_type", "karras"],
        base + ["--karras_sampler", "dpm", "--solver_type", "midpoint"], base + ["--karras_sampler", "progdist", "--no_lower_order_final"],
        base + ["--cm_sampler", "onestep", "--solver_order", "2"],
        base + ["--karras_sampler", "dpmpp", "--s_churn", "10"], base + ["--karras_sampler", "dpmpp", "--s_tmin", "0.1"],
        base + ["--karras_sampler", "sde-dpmpp", "--s_tmax", "50"], base + ["--karras_sampler", "sde-dpmpp", "--s_noise", "1.0"],
        base + ["--karras_sampler", "sde-dpmpp", "--solver_order", "3"], base + ["--karras_sampler", "dpmpp", "--solver_order", "4"],
        base + ["--karras_sampler", "dpmpp", "--skip_type", "logsnr", "--rho", "7"],
        base + ["--karras_sampler", "dpmpp", "--skip_type", "uniform"], base + ["--karras_sampler", "dpmpp", "--solver_type", "heun"],
        base + ["--karras_sampler", "dpmpp", "--karras_steps", "1"], base + ["--karras_sampler", "dpmpp", "--guidance_scale", "1.0"],
        base + ["--karras_sampler", "dpmpp", "--cm_sampler", "onestep"], base + ["--karras_sampler", "dpmpp", "--sampler_generator", "determ"],
        base + ["--karras_sampler", "unipc"],
    ]
    for flags in rejected:
        with pytest.raises(SystemExit):
            gl.parse_args(flags)
            pytest.fail(f"{flags} was accepted")


# ------------------------------------------------------------------------------------------ 6. host sanitizers
def test_edm_dpm_stage_arguments_under_address_and_ub_sanitizers():
    """`make asan_edm_dpm` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_edm_dpm.c, a program with its own main, against it and a no-device HIP runtime stub.  Null, misaligned
    and out-of-range arguments, z together with sample_index and a missing x_in on a row that is not last must each come back as
    DXMI_EINVAL with the message of their check: no crash, no sanitizer report.  The program runs as a child process; nothing is
    loaded into python.  A host-only build: machines without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_edm_dpm"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_edm_dpm")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") >= 45
