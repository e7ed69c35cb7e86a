"""UniPC sampling of the DDPM teacher on the host (models/DxMI/unipc_sample.py, unipc_coefficients in models/DxMI/dpm_sample.py): the
closed forms against UniPC's algorithm written here from the paper (r_k, the phi recurrence, R rho = b, numpy.linalg.solve, rho =
1/2 where the paper fixes it) and against Gauss-Legendre quadrature of the Lagrange integrals, the bit identities with the
DPM-Solver++ table, the order of convergence on the analytic network of tests/test_dpm_sample_host.py, the table, the torch path,
the refusals and the argument checks of both launches under the host sanitizers (a stand-alone program, run as a child process).
No GPU.  There is no golden fixture: the reference tree has no such sampler.

Order test, measured with the project's fp32 Alpha_bar table when this test was written (relative error of the state after row
S - 2, S = 16 / 32, with the corrector; the ratio; the predictor-only errors):
    bh1  order 1: 3.66e-02 / 7.41e-03, ratio 4.94 (alone 1.49e-01 / 7.50e-02);  order 2: 4.86e-02 / 5.00e-03, 9.72 (1.08e-01 /
         2.12e-02);  order 3: 2.17e-03 / 3.57e-05, 60.7 (7.64e-03 / 6.31e-04)
    bh2  order 1: 6.99e-02 / 1.78e-02, ratio 3.93 (1.49e-01 / 7.50e-02);  order 2: 1.74e-02 / 2.38e-03, 7.33 (2.12e-02 / 5.82e-03);
         order 3: 1.92e-03 / 5.02e-05, 38.1 (8.12e-03 / 6.16e-04)"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from numpy.polynomial.legendre import leggauss

from dxmi_hip import ops
from models.DxMI.dpm_sample import DPMSampleSchedule, dpm_orders, dpm_timesteps, unipc_dpm_coefficients
from models.DxMI.unipc_sample import UniPCSchedule, unipc_sample, unipc_sample_schedule, unipc_timesteps, unipc_transition
from test_dpm_sample_host import alpha_bar64, analytic_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("bh1", "bh2")
CV = ("cv0", "cv1", "cv2", "cv3")


def teacher_nodes(S, skip_type="logsnr"):
    """(alpha, sigma, lambda) of the S evaluations, noisiest first, and the steps, from the fp32 table read into float64."""
    ab, tau = alpha_bar64(), dpm_timesteps(S, skip_type=skip_type)
    t = tau[::-1]
    alpha, sigma = np.sqrt(ab[t]), np.sqrt(1 - ab[t])
    return alpha, sigma, np.log(alpha) - np.log(sigma), tau


# ------------------------------------------------------------------------------------------ 1. UniPC's linear system
def paper_weights(lam_prev, lam_t, alpha_t, order, variant):
    """UniPC (data prediction, multistep) of one step to lam_t from the `order` evaluations at lam_prev (newest first), written
    from the paper: x_t = (sigma_t / sigma_prev0) x - alpha_t (e^-h - 1) D_prev0 - alpha_t B(h) sum_m rho_m D1_m with D1_m =
    (D_prev_m - D_prev0) / r_m (and, for the corrector, D1 = D_t - D_prev0 with r = 1), rho the solution of R rho = b, R_{n,m} =
    r_m^n, b_n = hh phi_{n+2}(hh) (n + 1)! / B(hh), hh = -h.  rho = 1/2 where one unknown is left.
    -> (the predictor's weights on D_prev0.., the corrector's weights on D_t, D_prev0..)."""
    h = lam_t - lam_prev[0]
    rks = [(lam_prev[i] - lam_prev[0]) / h for i in range(1, order)] + [1.0]
    hh = -h
    h_phi_1 = np.expm1(hh)
    h_phi_k = h_phi_1 / hh - 1
    B_h = hh if variant == "bh1" else np.expm1(hh)
    R, b, fact = [], [], 1
    for i in range(1, order + 1):
        R.append(np.power(rks, i - 1))
        b.append(h_phi_k * fact / B_h)
        fact *= i + 1
        h_phi_k = h_phi_k / hh - 1 / fact
    R, b = np.asarray(R), np.asarray(b)
    if order == 1:
        rho_p, rho_c = np.zeros(0), np.asarray([0.5])
    else:
        rho_p = np.asarray([0.5]) if order == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
        rho_c = np.linalg.solve(R, b)

    def on_values(rho, with_t):
        """x_t's weights on the values themselves, from those on the differences."""
        w_prev = np.zeros(order)
        w_prev[0] = -alpha_t * h_phi_1
        w_t = 0.0
        for m in range(order - 1):
            c = -alpha_t * B_h * rho[m] / rks[m]
            w_prev[m + 1] += c
            w_prev[0] -= c
        if with_t:
            c = -alpha_t * B_h * rho[-1]
            w_t += c
            w_prev[0] -= c
        return w_prev, w_t

    pred, _ = on_values(rho_p, False)
    corr_prev, corr_t = on_values(rho_c, True)
    return pred, np.concatenate([[corr_t], corr_prev])


def check_against_paper(co, alpha, lam, orders, variant, label):
    S = len(lam)
    worst = 0.0
    for k in range(S - 1):
        p = orders[k]
        pred, _ = paper_weights([lam[k - i] for i in range(p)], lam[k + 1], alpha[k + 1], p, variant)
        got = np.asarray([co[f"w{j}"][k] for j in range(3)])
        want = np.concatenate([pred, np.zeros(3 - p)])
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
        if k >= 1:
            q = orders[k - 1]
            _, corr = paper_weights([lam[k - 1 - i] for i in range(q)], lam[k], alpha[k], q, variant)
            got = np.asarray([co[c][k] for c in CV])
            want = np.concatenate([corr, np.zeros(3 - q)])
            worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
            assert co["corr_order"][k] == q
    print(f"{label}: worst |closed form - linear system| / max_j |w_j| = {worst:.3e}")
    assert worst <= 1e-12
    return worst


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("S", [10, 16])
def test_closed_forms_are_unipcs_linear_system(S, order, variant):
    alpha, sigma, lam, tau = teacher_nodes(S)
    co = unipc_dpm_coefficients(alpha_bar64(), tau, order, variant)
    orders = dpm_orders(S, order)
    assert list(co["order"]) == orders and list(co["corr_order"]) == [0] + orders[:-2] + [0]
    check_against_paper(co, alpha, lam, orders, variant, f"teacher logsnr S={S} order {order} {variant}")
    assert np.allclose(co["cx"][:-1], sigma[1:] / sigma[:-1], rtol=1e-14, atol=0) and np.allclose(co["ccx"][1:-1], sigma[1:-1] / sigma[:-2],
                                                                                              rtol=1e-14, atol=0)
    assert (co["cx"][-1], co["w0"][-1], co["w1"][-1], co["w2"][-1], co["ccx"][-1], co["ccx"][0]) == (0, 1, 0, 0, 0, 0)
    for k in range(S):          # a weight beyond a row's order is exactly 0, one within it is not
        assert [co[f"w{j}"][k] != 0 for j in range(3)] == [j < orders[k] for j in range(3)]
        q = co["corr_order"][k]
        assert [co[c][k] != 0 for c in CV] == [q > 0 and j <= q for j in range(4)]


def quadrature(nodes, h, j):
    """int_0^h e^-v L_j(v) dv by Gauss-Legendre with 48 nodes (an exponential times a cubic over h <= 1.6: exact to rounding)."""
    gx, gw = leggauss(48)
    v = 0.5 * h * gx + 0.5 * h
    L = np.ones_like(v)
    for i, ni in enumerate(nodes):
        if i != j:
            L = L * (v - ni) / (nodes[j] - ni)
    return 0.5 * h * np.sum(gw * np.exp(-v) * L)


def check_solved_rows_against_quadrature(co, alpha, lam, label):
    S, worst, rows = len(lam), 0.0, 0
    for k in range(1, S - 1):
        q = int(co["corr_order"][k])
        if q >= 2:
            nodes = [lam[k] - lam[k - j] for j in range(q + 1)]
            want = np.asarray([alpha[k] * quadrature(nodes, lam[k] - lam[k - 1], j) for j in range(q + 1)])
            got = np.asarray([co[c][k] for c in CV[:q + 1]])
            worst, rows = max(worst, np.abs(got - want).max() / np.abs(want).max()), rows + 1
        if co["order"][k] == 3:
            nodes = [lam[k + 1] - lam[k - j] for j in range(3)]
            want = np.asarray([alpha[k + 1] * quadrature(nodes, lam[k + 1] - lam[k], j) for j in range(3)])
            got = np.asarray([co[f"w{j}"][k] for j in range(3)])
            worst, rows = max(worst, np.abs(got - want).max() / np.abs(want).max()), rows + 1
    print(f"{label}: {rows} solved rows, worst |w - quadrature| / max_j |w_j| = {worst:.3e}")
    assert rows and worst <= 1e-12


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("S", [10, 16])
def test_solved_rows_against_quadrature(S, order, variant):
    alpha, sigma, lam, tau = teacher_nodes(S)
    co = unipc_dpm_coefficients(alpha_bar64(), tau, order, variant)
    check_solved_rows_against_quadrature(co, alpha, lam, f"teacher S={S} order {order} {variant}")


# ------------------------------------------------------------------------------------------ 2. identities, bit for bit in fp32
MT_UT = ((ops.MT_T, ops.UT_T), (ops.MT_T_NEXT, ops.UT_T_NEXT), (ops.MT_CX, ops.UT_CX), (ops.MT_W0, ops.UT_W0), (ops.MT_W1, ops.UT_W1),
         (ops.MT_W2, ops.UT_W2), (ops.MT_A, ops.UT_A), (ops.MT_B, ops.UT_B), (ops.MT_FLAGS, ops.UT_FLAGS), (ops.MT_ORDER, ops.UT_ORDER))


def same_rows(uni, dpm, rows):
    return all(torch.equal(uni.table[rows][:, u], dpm.table[rows][:, m]) for m, u in MT_UT)


def test_predictor_rows_are_the_dpm_solver_rows():
    for S in (10, 16):
        rows = list(range(S))
        for order in (1, 2):      # bh2 without the corrector is DPM-Solver++ 2M midpoint
            assert same_rows(UniPCSchedule(S, order, "bh2", corrector=False), DPMSampleSchedule(S, order, solver_type="midpoint"), rows)
        for variant in VARIANTS:  # first order has no B(h)
            assert same_rows(UniPCSchedule(S, 1, variant, corrector=False), DPMSampleSchedule(S, 1, solver_type="midpoint"), rows)
            uni, exact = UniPCSchedule(S, 3, variant), DPMSampleSchedule(S, 3, solver_type="exact")
            rows3 = [k for k in range(S) if uni.coef["order"][k] == 3]
            assert len(rows3) == S - 4 and all(torch.equal(uni.table[rows3][:, u], exact.table[rows3][:, m]) for m, u in MT_UT[:8])
        # bh1 differs from the midpoint rule on the second-order rows, and only there
        bh1, mid = UniPCSchedule(S, 2, "bh1", corrector=False), DPMSampleSchedule(S, 2, solver_type="midpoint")
        rows2 = [k for k in range(S) if bh1.coef["order"][k] == 2]
        assert same_rows(bh1, mid, [k for k in range(S) if k not in rows2])
        assert all(bh1.table[k, ops.UT_W1] != mid.table[k, ops.MT_W1] for k in rows2)


def test_first_order_bh2_corrector_is_the_trapezoid():
    for S in (10, 16):
        alpha, sigma, lam, tau = teacher_nodes(S)
        sch = UniPCSchedule(S, 1, "bh2")
        rows = [k for k in range(S) if sch.coef["corr_order"][k] == 1]
        assert rows == list(range(1, S - 1))
        want = (alpha[rows] * -np.expm1(-(lam[rows] - lam[[k - 1 for k in rows]])) / 2).astype(np.float32)
        assert np.array_equal(sch.table[rows, ops.UT_CV0].numpy(), want) and np.array_equal(sch.table[rows, ops.UT_CV1].numpy(), want)
        assert torch.equal(sch.table[:, ops.UT_CV0], sch.table[:, ops.UT_CV1]) and not sch.table[:, [ops.UT_CV2, ops.UT_CV3]].any()


# ------------------------------------------------------------------------------------------ 3. the table
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", [1, 2, 3])
def test_table_columns(order, variant):
    S = 10
    sch = UniPCSchedule(S, order, variant)
    tab = sch.table
    assert tab.dtype == torch.float32 and tab.shape == (S, ops.UT_COLS) and sch.tau == unipc_timesteps(S) == dpm_timesteps(S)
    co = unipc_dpm_coefficients(alpha_bar64(), sch.tau, order, variant)
    for col, key in ((ops.UT_CX, "cx"), (ops.UT_W0, "w0"), (ops.UT_W1, "w1"), (ops.UT_W2, "w2"), (ops.UT_CCX, "ccx"), (ops.UT_CV0, "cv0"),
                     (ops.UT_CV1, "cv1"), (ops.UT_CV2, "cv2"), (ops.UT_CV3, "cv3"), (ops.UT_A, "a"), (ops.UT_B, "b")):
        assert np.array_equal(tab[:, col].numpy(), co[key].astype(np.float32)), key       # float64 on the fp32 table, rounded once
    orders = dpm_orders(S, order)
    assert tab[:, ops.UT_ORDER].tolist() == [float(o) for o in orders]
    assert tab[:, ops.UT_CORDER].tolist() == [0.0] + [float(o) for o in orders[:-2]] + [0.0]
    assert tab[:, ops.UT_FLAGS].tolist() == [1.0] + [5.0] * (S - 2) + [3.0]
    assert UniPCSchedule(S, order, variant, clip_denoised=False).table[:, ops.UT_FLAGS].tolist() == [0.0] + [4.0] * (S - 2) + [2.0]
    alone = UniPCSchedule(S, order, variant, corrector=False)
    assert alone.table[:, ops.UT_FLAGS].tolist() == [1.0] * (S - 1) + [3.0] and not alone.table[:, ops.UT_CORDER:ops.UT_CORDER + 1].any()
    assert not alone.table[:, ops.UT_CCX:].any() and not alone.carry and sch.carry and sch.hist_slots == 4
    assert sch.draws == [False] * S and sch.n_draws == 0
    assert tab[:, ops.UT_T].tolist() == [float(t) for t in sch.tau[::-1]] and tab[-1, ops.UT_T_NEXT] == 0
    free = UniPCSchedule(S, 3, variant, lower_order_final=False)
    assert free.table[:, ops.UT_ORDER].tolist() == [1.0, 2.0] + [3.0] * (S - 3) + [1.0]


def test_schedule_is_memoised_and_refuses():
    assert unipc_sample_schedule(10) is unipc_sample_schedule(10, 3, "bh1", True)
    assert unipc_sample_schedule(10) is not unipc_sample_schedule(10, corrector=False)
    assert unipc_sample_schedule(10) is not unipc_sample_schedule(10, variant="bh2")
    for bad in (dict(order=0), dict(order=4), dict(order=True), dict(order=2.5), dict(variant="bh3"), dict(variant="vary_coeff"),
                dict(skip_type="karras"), dict(steps=1), dict(steps=50)):
        with pytest.raises(ValueError):
            unipc_sample(analytic_net, (1, 3, 4, 4), device="cpu", **{"steps": 6, **bad})
    with pytest.raises(ValueError, match="order"):
        unipc_dpm_coefficients(alpha_bar64(), dpm_timesteps(10), 4)
    with pytest.raises(ValueError, match="variant"):
        unipc_dpm_coefficients(alpha_bar64(), dpm_timesteps(10), 3, "bh0")
    with pytest.raises(ValueError, match="rise"):
        unipc_dpm_coefficients(alpha_bar64(), [0, 500, 500, 999], 2)
    with pytest.raises(ValueError, match="7 draws"):
        unipc_sample(analytic_net, (1, 3, 4, 4), steps=6, device="cpu", noise=[torch.zeros(1, 3, 4, 4)] * 6)


# ------------------------------------------------------------------------------------------ 4. order of convergence
def flow_error(order, S, variant, corrector):
    """tests/test_dpm_sample_host.py's problem: the float64 torch path on eps(x, t) = sigma_t x / (0.25 ab_t + 1 - ab_t) (data
    N(0, 0.25)), logsnr steps, no clipping; the relative error of the predicted state after row S - 2 against the probability-flow
    solution at tau_0."""
    ab = torch.from_numpy(alpha_bar64())
    var = lambda t: 0.25 * ab[t] + 1 - ab[t]

    def net(x, t):
        assert x.dtype == torch.float64
        a = ab[t.long()][:, None, None, None]
        return (1 - a).sqrt() * x / (0.25 * a + 1 - a)

    tau = dpm_timesteps(S)
    x_T = torch.tensor([1.0, -0.5, 2.0, 0.25], dtype=torch.float64).reshape(2, 1, 1, 2)
    seen = []
    unipc_sample(net, x_T.shape, steps=S, order=order, variant=variant, corrector=corrector, skip_type="logsnr", clip_denoised=False,
                 device="cpu", noise=[x_T] + [None] * S, callback=seen.append)
    assert [d["i"] for d in seen] == list(range(S)) and [d["t"] for d in seen] == tau[::-1]
    got = seen[S - 2]["x"]
    assert got.dtype == torch.float64
    exact = x_T * (var(tau[0]) / var(tau[-1])).sqrt()
    return ((got - exact).abs() / exact.abs()).max().item()


@pytest.mark.parametrize("variant", VARIANTS)
def test_order_of_convergence(variant):
    """With the corrector order p behaves as order p + 1: the error ratio from S = 16 to 32 is at least 75 % of 2^(p+1), and the
    corrected error is below the predictor's own at both S.  (No claim at S = 10.)"""
    e = {(o, S, c): flow_error(o, S, variant, c) for o in (1, 2, 3) for S in (16, 32) for c in (True, False)}
    need = {1: 3, 2: 6, 3: 12}
    for o in (1, 2, 3):
        ratio = e[o, 16, True] / e[o, 32, True]
        print(f"{variant} order {o}: error {e[o, 16, True]:.4e} (S = 16), {e[o, 32, True]:.4e} (S = 32), ratio {ratio:.3f}; "
              f"predictor alone {e[o, 16, False]:.4e}, {e[o, 32, False]:.4e}")
        assert ratio >= need[o]
        assert e[o, 16, True] < e[o, 16, False] and e[o, 32, True] < e[o, 32, False]


# ------------------------------------------------------------------------------------------ 5. the torch path
def test_torch_path_on_the_cpu():
    S, shape = 6, (3, 3, 8, 8)
    gen = torch.Generator().manual_seed(11)
    noise = [torch.randn(shape, generator=gen)] + [None] * S
    kw = dict(steps=S, device="cpu")
    seen = []
    out = unipc_sample(analytic_net, shape, noise=noise, callback=seen.append, **kw)
    assert out.dtype == torch.float32 and out.shape == shape and out.abs().max() <= 1 and out.std() > 0.05
    assert [d["i"] for d in seen] == list(range(S)) and torch.equal(out, seen[-1]["x"].clamp(-1, 1))
    assert torch.equal(seen[-1]["x"], seen[-1]["pred_xstart"]) and all(d["pred_xstart"].abs().max() <= 1 for d in seen)
    wide = unipc_sample(analytic_net, shape, noise=[noise[0].double()] + [None] * S, **kw)
    assert wide.dtype == torch.float64 and (out.double() - wide).abs().max() <= 1e-4
    # the corrector changes the run from row 1 on, and only the corrector needs the carried state
    alone = []
    unipc_sample(analytic_net, shape, noise=noise, corrector=False, callback=alone.append, **kw)
    assert torch.equal(alone[0]["x"], seen[0]["x"]) and not torch.equal(alone[1]["x"], seen[1]["x"])
    # bh2, order 2, no corrector: dpm_sample's midpoint run, bit for bit
    from models.DxMI.dpm_sample import dpm_sample
    a = unipc_sample(analytic_net, shape, noise=noise, order=2, variant="bh2", corrector=False, **kw)
    assert torch.equal(a, dpm_sample(analytic_net, shape, noise=noise, order=2, solver_type="midpoint", **kw))
    # without noise= the one draw is torch's or the generator's
    torch.manual_seed(3)
    b = unipc_sample(analytic_net, shape, **kw)
    torch.manual_seed(3)
    assert torch.equal(b, unipc_sample(analytic_net, shape, **kw))


def test_transition_reads_what_its_weights_name():
    sch = unipc_sample_schedule(8, 3)
    x, eps, xc = torch.randn(2, 3, 4, 4), torch.randn(2, 3, 4, 4), torch.randn(2, 3, 4, 4)
    for k in range(8):
        p, q = int(sch.table[k, ops.UT_ORDER]), int(sch.table[k, ops.UT_CORDER])
        hist = [torch.randn_like(x)] * max(p - 1, q)          # shorter than three entries is never indexed past the orders
        acc, d0, b = unipc_transition(x, eps, sch.table[k], hist, xc)
        assert torch.isfinite(acc).all() and d0.abs().max() <= 1 and torch.equal(b, x) == (q == 0)
        plain, _, b0 = unipc_transition(x, eps, sch.table[k], hist[:max(p - 1, 0)], None)          # no corrected state: uncorrected
        assert torch.equal(b0, x) and torch.equal(plain, acc) == (q == 0)
    assert [int(v) for v in sch.table[:, ops.UT_CORDER]] == [0, 1, 2, 3, 3, 3, 3, 0]          # a q = 3 corrector runs at S = 8


def test_the_existing_samplers_are_as_they_were():
    from models.DxMI import dpm_sample as dp
    assert dp.ALGORITHMS == ("dpmsolver++", "sde-dpmsolver++") and DPMSampleSchedule.hist_slots == 3 and not DPMSampleSchedule.carry
    with pytest.raises(ValueError):
        dp.dpm_sample(analytic_net, (2, 3, 8, 8), steps=6, algorithm="unipc", device="cpu")


# ------------------------------------------------------------------------------------------ 6. host sanitizers
def test_unipc_stage_arguments_under_address_and_ub_sanitizers():
    """`make asan_unipc` compiles the HOST half of every source (no device code) with -fsanitize=address,undefined and links
    tests/host/cabi_malformed_unipc.c, a program with its own main, against it and a no-device HIP runtime stub.  Null, misaligned
    and out-of-range arguments of dxmi_unipc_stage and dxmi_edm_unipc_stage, xc == x and a missing x_in on a row that is not last
    must each come back as DXMI_EINVAL with the message of their check: no crash, no sanitizer report.  The program runs as a child
    process; nothing is loaded into python.  A host-only build: machines without a GPU only."""
    if torch.cuda.is_available():
        pytest.skip("host-only sanitizer build: CPU boxes only")
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no toolchain")
    csrc = os.path.join(ROOT, "diffusion-by-maxentirl_amd", "csrc")
    r = subprocess.run(["make", "-j8", "asan_unipc"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([os.path.join(csrc, "build_asan", "cabi_malformed_unipc")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "0 failure(s)" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert out.count("\nok ") + out.startswith("ok ") >= 85
