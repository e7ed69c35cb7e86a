"""UniPC on the EDM nets, host side (no GPU): models/cm/unipc_sample.py's coefficients (alpha = 1, lambda = -ln sigma) against UniPC's
linear system and the quadrature of tests/test_unipc_sample_host.py, the bit identities with the DPM-Solver++ table, the table's
columns against EDMDPMSchedule's, the order of convergence on the Gaussian-data problem of tests/test_edm_dpm_sample_host.py, the
torch path and the refusals.

Order test, measured on the project's fp32 ladders when this test was written: the error ratio from S = 40 to S = 80 with the
corrector, orders 1 / 2 / 3 (the corrected error is below the predictor's own at both S in all twelve cases):
    bh1, logsnr  4.47 / 8.77 / 8.85      bh1, karras  4.43 / 9.23 / 16.68
    bh2, logsnr  4.05 / 8.08 / 8.86      bh2, karras  4.01 / 8.51 / 16.69"""
import numpy as np
import pytest
import torch

from dxmi_hip import ops
from models.cm.dpm_sample import EDMDPMSchedule, edm_sigmas
from models.cm.karras_diffusion import KarrasDenoiser
from models.cm.unipc_sample import (EDMUniPCSchedule, edm_unipc_coefficients, edm_unipc_sample, edm_unipc_schedule,
                                    edm_unipc_transition)
from models.DxMI.dpm_sample import dpm_orders
from test_edm_dpm_sample_host import analytic_net, gaussian_net, ladder64
from test_unipc_sample_host import CV, VARIANTS, check_against_paper, check_solved_rows_against_quadrature

DIFFUSION = KarrasDenoiser()
ET_EUT = ((ops.ET_T, ops.EUT_T), (ops.ET_T_NEXT, ops.EUT_T_NEXT), (ops.ET_CX, ops.EUT_CX), (ops.ET_W0, ops.EUT_W0),
          (ops.ET_W1, ops.EUT_W1), (ops.ET_W2, ops.EUT_W2), (ops.ET_CSKIP, ops.EUT_CSKIP), (ops.ET_COUT, ops.EUT_COUT),
          (ops.ET_FLAGS, ops.EUT_FLAGS), (ops.ET_ORDER, ops.EUT_ORDER), (ops.ET_CIN, ops.EUT_CIN), (ops.ET_CIN_NEXT, ops.EUT_CIN_NEXT),
          (ops.ET_XSCALE, ops.EUT_XSCALE), (ops.ET_SIGMA, ops.EUT_SIGMA))


# ------------------------------------------------------------------------------------------ 1. the formulas
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("skip_type", ["karras", "logsnr"])
def test_closed_forms_are_unipcs_linear_system(skip_type, order, variant):
    S = 10
    sig = ladder64(S, skip_type)
    co = edm_unipc_coefficients(sig, order, variant)
    orders = dpm_orders(S, order)
    assert list(co["order"]) == orders and list(co["corr_order"]) == [0] + orders[:-2] + [0]
    check_against_paper(co, np.ones(S), -np.log(sig), orders, variant, f"EDM {skip_type} S={S} order {order} {variant}")
    if order >= 2:
        check_solved_rows_against_quadrature(co, np.ones(S), -np.log(sig), f"EDM {skip_type} S={S} order {order} {variant}")
    assert np.allclose(co["cx"][:-1], sig[1:] / sig[:-1], rtol=1e-14, atol=0) and np.allclose(co["ccx"][1:-1], sig[1:-1] / sig[:-2], rtol=1e-14,
                                                                                          atol=0)
    for k in range(S):          # a weight beyond a row's order is exactly 0, one within it is not
        assert [co[f"w{j}"][k] != 0 for j in range(3)] == [j < orders[k] for j in range(3)]
        q = co["corr_order"][k]
        assert [co[c][k] != 0 for c in CV] == [q > 0 and j <= q for j in range(4)]


def same_rows(uni, dpm, rows, pairs=ET_EUT):
    return all(torch.equal(uni.table[rows][:, u], dpm.table[rows][:, m]) for m, u in pairs)


@pytest.mark.parametrize("skip_type", ["karras", "logsnr"])
def test_identities_bit_for_bit(skip_type):
    S, rows = 10, list(range(10))
    for order in (1, 2):          # bh2 without the corrector is DPM-Solver++ 2M midpoint
        assert same_rows(EDMUniPCSchedule(DIFFUSION, S, order, "bh2", False, skip_type),
                         EDMDPMSchedule(DIFFUSION, S, order, solver_type="midpoint", skip_type=skip_type), rows)
    for variant in VARIANTS:
        assert same_rows(EDMUniPCSchedule(DIFFUSION, S, 1, variant, False, skip_type),
                         EDMDPMSchedule(DIFFUSION, S, 1, solver_type="midpoint", skip_type=skip_type), rows)
        uni, exact = EDMUniPCSchedule(DIFFUSION, S, 3, variant, True, skip_type), EDMDPMSchedule(DIFFUSION, S, 3, solver_type="exact",
                                                                                               skip_type=skip_type)
        rows3 = [k for k in range(S) if uni.coef["order"][k] == 3]
        assert len(rows3) == S - 4 and same_rows(uni, exact, rows3, [p for p in ET_EUT if p[0] != ops.ET_FLAGS])
    # the q = 1, bh2 corrector is the trapezoid alpha_k g (D_k + D_{k-1}) / 2, alpha = 1
    sch = EDMUniPCSchedule(DIFFUSION, S, 1, "bh2", True, skip_type)
    sig = ladder64(S, skip_type)
    want = (-np.expm1(-np.log(sig[:-2] / sig[1:-1])) / 2).astype(np.float32)
    assert np.array_equal(sch.table[1:-1, ops.EUT_CV0].numpy(), want) and torch.equal(sch.table[:, ops.EUT_CV0], sch.table[:, ops.EUT_CV1])
    assert not sch.table[:, [ops.EUT_CV2, ops.EUT_CV3]].any() and not sch.table[[0, -1], ops.EUT_CV0].any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_table_columns(variant):
    S = 10
    sch = EDMUniPCSchedule(DIFFUSION, S, 3, variant)
    tab = sch.table
    assert tab.dtype == torch.float32 and tab.shape == (S, ops.EUT_COLS) and torch.equal(sch.sigmas, edm_sigmas(S))
    co = edm_unipc_coefficients(sch.sigmas.numpy().astype(np.float64), 3, variant)
    for col, key in ((ops.EUT_CX, "cx"), (ops.EUT_W0, "w0"), (ops.EUT_W1, "w1"), (ops.EUT_W2, "w2"), (ops.EUT_CCX, "ccx"),
                     (ops.EUT_CV0, "cv0"), (ops.EUT_CV1, "cv1"), (ops.EUT_CV2, "cv2"), (ops.EUT_CV3, "cv3")):
        assert np.array_equal(tab[:, col].numpy(), co[key].astype(np.float32)), key
    orders = dpm_orders(S, 3)
    assert tab[:, ops.EUT_ORDER].tolist() == [float(o) for o in orders]
    assert tab[:, ops.EUT_CORDER].tolist() == [0.0] + [float(o) for o in orders[:-2]] + [0.0]
    assert tab[:, ops.EUT_FLAGS].tolist() == [1.0] + [5.0] * (S - 2) + [3.0]
    # the preconditioning's columns: EDMDPMSchedule's bits
    pre = [p for p in ET_EUT if p[0] in (ops.ET_T, ops.ET_T_NEXT, ops.ET_CSKIP, ops.ET_COUT, ops.ET_CIN, ops.ET_CIN_NEXT, ops.ET_XSCALE,
                                        ops.ET_SIGMA)]
    assert same_rows(sch, EDMDPMSchedule(DIFFUSION, S, 3), list(range(S)), pre)
    alone = EDMUniPCSchedule(DIFFUSION, S, 3, variant, corrector=False)
    assert not alone.table[:, ops.EUT_CCX:].any() and not alone.carry and sch.carry and sch.hist_slots == 4 and sch.n_draws == 0
    assert sch.x_in and sch.net_keywords == ("y",)


def test_schedule_is_memoised_and_refuses():
    a = edm_unipc_schedule(DIFFUSION, 10)
    assert a is edm_unipc_schedule(KarrasDenoiser(), 10, 3, "bh1", True) and a is not edm_unipc_schedule(DIFFUSION, 10, corrector=False)
    assert a is not edm_unipc_schedule(DIFFUSION, 10, variant="bh2") and a is not edm_unipc_schedule(KarrasDenoiser(sigma_data=1.0), 10)
    for name in ("uniform", "quad"):
        with pytest.raises(ValueError, match=name):
            edm_unipc_schedule(DIFFUSION, 10, skip_type=name)
    with pytest.raises(NotImplementedError, match="distillation"):
        edm_unipc_schedule(KarrasDenoiser(distillation=True), 10)
    with pytest.raises(NotImplementedError, match="distillation"):
        edm_unipc_sample(KarrasDenoiser(distillation=True), lambda x, t: x, (1, 1, 2, 2), device="cpu")
    for bad in (dict(order=0), dict(order=4), dict(order=True), dict(variant="bh3"), dict(steps=1), dict(skip_type="linear")):
        with pytest.raises(ValueError):
            edm_unipc_schedule(DIFFUSION, **{"steps": 10, **bad})
    with pytest.raises(ValueError, match="fall"):
        edm_unipc_coefficients([80.0, 1.0, 1.0, 0.002])
    with pytest.raises(ValueError, match="model_kwargs"):
        edm_unipc_sample(DIFFUSION, analytic_net, (1, 3, 4, 4), steps=4, device="cpu", model_kwargs={"cond": torch.zeros(1)})


# ------------------------------------------------------------------------------------------ 2. order of convergence
def flow_error(order, S, skip_type, variant, corrector):
    """tests/test_edm_dpm_sample_host.py's problem (data N(0, 0.25), sigma from 80 down to 0.002): the relative error of the
    predicted state after row S - 2 against the probability-flow solution at sigma_min."""
    x0 = torch.tensor([1.0, -0.5, 2.0, 0.25], dtype=torch.float64).reshape(2, 1, 1, 2)
    seen = []
    edm_unipc_sample(DIFFUSION, gaussian_net, x0.shape, steps=S, order=order, variant=variant, corrector=corrector, skip_type=skip_type,
                     clip_denoised=False, device="cpu", noise=[x0] + [None] * S, callback=seen.append)
    sch = edm_unipc_schedule(DIFFUSION, S, order, variant, corrector, skip_type, True, False)
    assert [d["i"] for d in seen] == list(range(S)) and [float(d["sigma"]) for d in seen] == sch.sigmas.tolist()
    got = seen[S - 2]["x"]
    assert got.dtype == torch.float64
    s0, s1 = float(sch.sigmas[0]), float(sch.sigmas[-1])
    exact = x0 * 80.0 * np.sqrt((0.25 + s1 ** 2) / (0.25 + s0 ** 2))
    return ((got - exact).abs() / exact.abs()).max().item()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("skip_type", ["logsnr", "karras"])
def test_order_of_convergence(skip_type, variant):
    e = {(o, S, c): flow_error(o, S, skip_type, variant, c) for o in (1, 2, 3) for S in (40, 80) for c in (True, False)}
    need = {1: 3.5, 2: 7, 3: 7}          # fourth order is not asked for: the low-order starting rows cap it
    for o in (1, 2, 3):
        ratio = e[o, 40, True] / e[o, 80, True]
        print(f"{variant} {skip_type} order {o}: error {e[o, 40, True]:.4e} (S = 40), {e[o, 80, True]:.4e} (S = 80), ratio {ratio:.3f}; "
              f"predictor alone {e[o, 40, False]:.4e}, {e[o, 80, False]:.4e}")
        assert ratio >= need[o]
        assert e[o, 40, True] < e[o, 40, False] and e[o, 80, True] < e[o, 80, False]


# ------------------------------------------------------------------------------------------ 3. the torch path
def test_torch_path_on_the_cpu():
    S, shape = 6, (3, 3, 8, 8)
    gen = torch.Generator().manual_seed(11)
    noise = [torch.randn(shape, generator=gen)] + [None] * S
    kw = dict(steps=S, device="cpu")
    seen = []
    out = edm_unipc_sample(DIFFUSION, analytic_net, shape, noise=noise, callback=seen.append, **kw)
    assert out.dtype == torch.float32 and out.shape == shape and out.abs().max() <= 1 and out.std() > 0.05
    assert [d["i"] for d in seen] == list(range(S)) and torch.equal(out, seen[-1]["x"].clamp(-1, 1))
    assert torch.equal(seen[-1]["x"], seen[-1]["pred_xstart"]) and all(d["pred_xstart"].abs().max() <= 1 for d in seen)
    wide = edm_unipc_sample(DIFFUSION, analytic_net, shape, noise=[noise[0].double()] + [None] * S, **kw)
    assert wide.dtype == torch.float64 and (out.double() - wide).abs().max() <= 1e-4
    alone = []
    edm_unipc_sample(DIFFUSION, analytic_net, shape, noise=noise, corrector=False, callback=alone.append, **kw)
    assert torch.equal(alone[0]["x"], seen[0]["x"]) and not torch.equal(alone[1]["x"], seen[1]["x"])
    # bh2, order 2, no corrector: edm_dpm_sample's midpoint run, bit for bit
    from models.cm.dpm_sample import edm_dpm_sample
    a = edm_unipc_sample(DIFFUSION, analytic_net, shape, noise=noise, order=2, variant="bh2", corrector=False, **kw)
    assert torch.equal(a, edm_dpm_sample(DIFFUSION, analytic_net, shape, noise=noise, order=2, solver_type="midpoint", **kw))
    y = torch.tensor([1, 5, 9])
    assert not torch.equal(edm_unipc_sample(DIFFUSION, analytic_net, shape, noise=noise, model_kwargs={"y": y}, **kw), out)
    for n in (noise[:-1], noise + [noise[0]]):
        with pytest.raises(ValueError, match=f"{S + 1} draws"):
            edm_unipc_sample(DIFFUSION, analytic_net, shape, noise=n, **kw)


def test_transition_without_a_corrected_state_runs_uncorrected():
    sch = edm_unipc_schedule(DIFFUSION, 8, 3)
    x, F, xc = torch.randn(2, 3, 4, 4), torch.randn(2, 3, 4, 4), torch.randn(2, 3, 4, 4)
    for k in range(8):
        p, q = int(sch.table[k, ops.EUT_ORDER]), int(sch.table[k, ops.EUT_CORDER])
        hist = [torch.randn_like(x)] * max(p - 1, q)
        acc, d0, b = edm_unipc_transition(x, F, sch.table[k], hist, xc)
        plain, _, b0 = edm_unipc_transition(x, F, sch.table[k], hist[:max(p - 1, 0)], None)
        assert torch.equal(b0, x) and torch.equal(b, x) == (q == 0) and torch.equal(plain, acc) == (q == 0) and d0.abs().max() <= 1


def test_karras_sample_and_dpm_sample_are_as_they_were():
    from models.cm import karras_diffusion as kd
    assert kd.KARRAS_SAMPLERS == ("heun", "dpm", "euler", "ancestral") and EDMDPMSchedule.hist_slots == 3 and not EDMDPMSchedule.carry
    with pytest.raises(ValueError):
        kd.karras_sample(DIFFUSION, analytic_net, (1, 3, 8, 8), 5, sampler="unipc")
