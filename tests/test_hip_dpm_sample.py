"""DPM-Solver++ sampling on the device: dxmi_dpm_stage against float64 on the same fp32 operands, history that was never written,
the history's slot addressing, its fused noise against dxmi_randn_indexed, the device control block, NaN and out-of-range handling,
the loop against a float64 loop with an analytic network, replay against eager on the shrunken HIP Model, batch invariance with the
deterministic generators, and generate_cifar10.py --solver dpmpp.

Bounds (u = 2^-24), counted from the kernel's operations on the fp32 table values K widened to float64, per element:
  stage   8 u (|cx x| + |w0| (|a x| + |b eps|) + |w1 D1| + |w2 D2| + |s z|): every term is rounded at most three times at half an
          ulp (its own product, the product or difference it enters, the running sum), and the clamp is continuous;
  D0      8 u (|a x| + |b eps|)   (pred_xstart and the written history slot)
  loop    the stage bound propagated row by row through the float64 loop.  With d(v) a bound on |device v - float64 v|:
            d(eps) = 0.72 d(x) + 8 u (0.8 (|0.9 x| + 1e-3 t) + |eps|)      the analytic network 0.8 tanh(0.9 x + 1e-3 t) has slope
                                                                          <= 0.72; its fp32 evaluation rounds the two products,
                                                                          their sum, tanh (2 ulp) and the scaling
            d(D0)  = a d(x) + b d(eps) + 8 u (|a x| + |b eps|)             the clamp has slope <= 1
            d(x')  = |cx| d(x) + |w0| (a d(x) + b d(eps)) + |w1| d(D1) + |w2| d(D2) + stage bound
          The same recursion with the clip form's bound of tests/test_hip_ddpm_sample.py gives ddpm_sample's; first-order DPM-Solver++
          and DDIM are the same map, so the two device loops may differ by the sum of the two (a table entry is one rounding away
          from its float64 value, which the 8 u per term, counted for 1.5 u of arithmetic, leaves room for)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "diffusion-by-maxentirl_amd")
STEPS = 10
ODE, SDE = "dpmsolver++", "sde-dpmsolver++"
SHAPES = [(3, 75), (2, 192), (5, 3072), (1, 5000), (1, 263347)]
SENTINEL = 123.0


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def schedule(algorithm, clip=True, steps=STEPS, order=None, **kw):
    from models.DxMI.dpm_sample import dpm_sample_schedule
    return dpm_sample_schedule(steps, (3 if algorithm == ODE else 2) if order is None else order, algorithm, clip_denoised=clip, **kw)


_OPERANDS = {}


def operands(ops, row, N, CHW, seed):
    """x, eps, z, D1, D2 (CPU fp32, computed once per key) with about half of the data prediction outside [-1, 1]:
    x = alpha_t x0 + sigma_t e, eps = e, x0 uniform in [-2, 2]; D1, D2 uniform in [-1, 1]."""
    key = (float(row[ops.MT_A]), float(row[ops.MT_B]), N, CHW, seed)
    if key not in _OPERANDS:
        gen = torch.Generator().manual_seed(seed)
        x0 = torch.rand(N, CHW, generator=gen) * 4 - 2
        e = torch.randn(N, CHW, generator=gen)
        z = torch.randn(N, CHW, generator=gen)
        d1, d2 = torch.rand(N, CHW, generator=gen) * 2 - 1, torch.rand(N, CHW, generator=gen) * 2 - 1
        a, b = float(row[ops.MT_A]), float(row[ops.MT_B])
        _OPERANDS[key] = ((x0 / a + (b / a) * e).float(), e, z, d1, d2)
    return _OPERANDS[key]


def history(k, d1, d2, fill=SENTINEL):
    """[3, N, CHW] with D_{k-1} and D_{k-2} where row k looks for them and `fill` in the slot it writes."""
    h = torch.full((3,) + tuple(d1.shape), fill)
    h[(k - 1) % 3], h[(k - 2) % 3] = d1, d2
    return h


def oracle(ops, row, x, eps, z, d1, d2):
    """float64 on the fp32 operands -> (x', D0, bound, bound of D0)."""
    K = row.double().numpy()
    x, eps, z, d1, d2 = (v.double().numpy() for v in (x, eps, z, d1, d2))
    cx, w0, w1, w2, s, a, b = (K[i] for i in (ops.MT_CX, ops.MT_W0, ops.MT_W1, ops.MT_W2, ops.MT_S, ops.MT_A, ops.MT_B))
    d0 = a * x - b * eps
    if int(K[ops.MT_FLAGS]) & ops.MT_FLAG_CLIP:
        d0 = np.clip(d0, -1, 1)
    xn = cx * x + w0 * d0 + w1 * d1 + w2 * d2 + s * z
    pbound = 8 * U * (np.abs(a * x) + np.abs(b * eps))
    bound = 8 * U * (np.abs(cx * x) + abs(w0) * (np.abs(a * x) + np.abs(b * eps)) + np.abs(w1 * d1) + np.abs(w2 * d2) + np.abs(s * z))
    return xn, d0, bound, pbound


def launch(ops, tab, row, x, eps, hist, z=None, pred=True, **kw):
    """One by-value launch on copies -> (x', t_out, out, pred_xstart, hist); out is pre-filled with 7."""
    xd, t = x.to(DEV).clone(), torch.full((x.shape[0],), -5.0, device=DEV)
    out = torch.full_like(xd, 7.0)
    p = torch.empty_like(xd) if pred else None
    hd = hist.to(DEV).clone()
    ops.dpm_stage(ops.DPM_STEP, tab, t, row=row, x=xd, eps=eps.to(DEV), z=None if z is None else z.to(DEV), hist=hd, out=out,
                  pred_xstart=p, **kw)
    torch.cuda.synchronize()
    return xd, t, out, p, hd


# ------------------------------------------------------------------------------------------ 1. the launch against float64
@pytest.mark.parametrize("algorithm", [ODE, SDE])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("N,CHW", SHAPES)
def test_stage_vs_fp64(ops, N, CHW, clip, algorithm):
    sch = schedule(algorithm, clip)
    tab = sch.device_table(DEV)
    top = 3 if algorithm == ODE else 2
    assert sch.table[:3, ops.MT_ORDER].tolist() == [1, 2, top] and sch.table[-1, ops.MT_ORDER] == 1
    worst = 0.0
    for row, neighbour in ((0, 1), (1, 2), (2, 3), (STEPS - 1, STEPS - 2)):
        K = sch.table[row]
        x, eps, z, d1, d2 = operands(ops, K, N, CHW, 100 * row + CHW)
        got, t_out, out, pred, hist = launch(ops, tab, row, x, eps, history(row, d1, d2), z)
        want, want_d0, bound, pbound = oracle(ops, K, x, eps, z, d1, d2)
        clipped = (np.abs(want_d0) >= 1).mean() if clip else (np.abs(want_d0) > 1).mean()
        assert 0.3 < clipped < 0.7, clipped
        err = np.abs(got.cpu().double().numpy() - want)
        perr = np.abs(pred.cpu().double().numpy() - want_d0)
        worst = max(worst, (err / bound).max(), (perr / pbound).max())
        print(f"({N}, {CHW}) clip {clip} {algorithm} row {row}: worst |err| / bound = {(err / bound).max():.3e}, pred_xstart "
              f"{(perr / pbound).max():.3e}")
        assert (err <= bound).all() and (perr <= pbound).all()
        # negative control, on the CPU: the neighbouring row's coefficients must not pass
        other = oracle(ops, sch.table[neighbour], x, eps, z, d1, d2)[0]
        assert (np.abs(other - want) > bound).any()
        # the written slot is D0 to the bit, the two others are as they were
        assert torch.equal(hist[row % 3], pred)
        assert torch.equal(hist[(row - 1) % 3].cpu(), d1) and torch.equal(hist[(row - 2) % 3].cpu(), d2)
        last = row == STEPS - 1
        assert torch.equal(t_out.cpu(), torch.full((N,), float(K[ops.MT_T_NEXT])))
        assert t_out[0].item() == (0.0 if last else float(sch.tau[STEPS - 2 - row]))
        assert torch.equal(out, got.clamp(-1, 1) if last else torch.full_like(out, 7.0))
        if last:
            assert torch.equal(got, pred)             # cx = 0, w0 = 1: x' = 0 x + 1 D0
        # pred_xstart is optional and changes nothing else
        bare = launch(ops, tab, row, x, eps, history(row, d1, d2), z, pred=False)
        assert bare[3] is None and all(torch.equal(u, v) for u, v in zip((got, t_out, out, hist), (bare[0], bare[1], bare[2], bare[4])))
    print(f"({N}, {CHW}) clip {clip} {algorithm}: worst ratio to the bound over the rows {worst:.3e}")


def test_first_mode_writes_the_first_time(ops):
    sch = schedule(ODE)
    t = torch.full((6,), -1.0, device=DEV)
    ops.dpm_stage(ops.DPM_FIRST, sch.device_table(DEV), t, row=0)
    assert t.tolist() == [float(sch.tau[-1])] * 6 == [999.0] * 6
    ops.dpm_stage(ops.DPM_FIRST, sch.device_table(DEV), t, row=3)
    assert t.tolist() == [float(sch.tau[-4])] * 6


# ------------------------------------------------------------------------------------------ 2. history that was never written
@pytest.mark.parametrize("algorithm", [ODE, SDE])
@pytest.mark.parametrize("N,CHW", [(3, 75), (5, 3072)])
def test_unwritten_history_is_not_read(ops, N, CHW, algorithm):
    """S = 6: the orders are 1, 2, 3, 3, 2, 1 (ODE, order 3) and 1, 2, 2, 2, 2, 1 (SDE, order 2).  Every slot a row's order does not
    name, and the slot it writes, holds NaN in one launch and 0 in the other."""
    S = 6
    sch = schedule(algorithm, steps=S)
    tab = sch.device_table(DEV)
    orders = [int(o) for o in sch.table[:, ops.MT_ORDER]]
    assert orders == ([1, 2, 3, 3, 2, 1] if algorithm == ODE else [1, 2, 2, 2, 2, 1])
    checked = 0
    for row in range(S):
        o = orders[row]
        if o == 3:
            continue
        x, eps, z, d1, d2 = operands(ops, sch.table[row], N, CHW, 7 + row)
        runs = []
        for fill in (float("nan"), 0.0):
            h = history(row, d1, d2, fill)
            for j in (1, 2):
                if j >= o:
                    h[(row - j) % 3] = fill
            if row == 0:
                assert bool(torch.isnan(h).all()) == (fill != 0.0)
            runs.append(launch(ops, tab, row, x, eps, h, z))
        a, b = runs
        for k in (0, 1, 3):          # x', t_out, pred_xstart
            assert torch.equal(a[k], b[k]) and torch.isfinite(a[k]).all()
        assert torch.equal(a[2], b[2])
        assert torch.equal(a[4][row % 3], b[4][row % 3]) and torch.isfinite(a[4][row % 3]).all()
        checked += 1
    assert checked == (4 if algorithm == ODE else 6)
    # and the control: a row of full order does read both slots
    row = 2 if algorithm == ODE else 1
    x, eps, z, d1, d2 = operands(ops, sch.table[row], N, CHW, 7 + row)
    h = history(row, d1, d2)
    h[(row - (2 if algorithm == ODE else 1)) % 3] = float("nan")
    assert torch.isnan(launch(ops, tab, row, x, eps, h, z)[0]).all()


# ------------------------------------------------------------------------------------------ 3. slot addressing
@pytest.mark.parametrize("N,CHW", [(3, 75), (5, 3072)])
def test_each_launch_writes_slot_row_mod_3_only(ops, N, CHW):
    sch = schedule(ODE)
    tab = sch.device_table(DEV)
    for row in range(7):
        x, eps, z, _, _ = operands(ops, sch.table[row], N, CHW, 50 + row)
        h = torch.full((3, N, CHW), SENTINEL)
        got = launch(ops, tab, row, x, eps, h)
        for slot in range(3):
            if slot == row % 3:
                assert torch.equal(got[4][slot], got[3]) and (got[4][slot].abs() <= 1).all()
            else:
                assert (got[4][slot] == SENTINEL).all(), (row, slot)
        # the same through the control block, where the kernel derives the slots from the row it reads there
        xd, t, out, hd = x.to(DEV).clone(), torch.empty(N, device=DEV), torch.empty(N, CHW, device=DEV), h.to(DEV).clone()
        ops.dpm_stage(ops.DPM_STEP, tab, t, row=(row + 1) % STEPS, ctl=control(row, 0, 0), x=xd, eps=eps.to(DEV), hist=hd, out=out)
        assert torch.equal(hd, got[4]) and torch.equal(xd, got[0])


# ------------------------------------------------------------------------------------------ 4. fused noise
SEED = (1 << 40) + 12345
INDEX = [5, (1 << 33) + 7, 123456, 0, 99]
MID = 4


def control(row, draw, seed):
    return torch.from_numpy(np.array([row, draw, seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32).view(np.int32)).to(DEV)


@pytest.mark.parametrize("N,CHW", [(3, 75), (5, 3072)])
def test_fused_noise_is_randn_indexed(ops, N, CHW):
    sch = schedule(SDE)
    tab = sch.device_table(DEV)
    assert sch.table[MID, ops.MT_S] != 0
    x, eps, _, d1, d2 = operands(ops, sch.table[MID], N, CHW, 9)
    h = history(MID, d1, d2)
    idx = torch.tensor(INDEX[:N], dtype=torch.int64, device=DEV)
    z = ops.randn_indexed(idx, (CHW,), SEED, 3)
    explicit = launch(ops, tab, MID, x, eps, h, z)
    fused = launch(ops, tab, MID, x, eps, h, None, sample_index=idx, seed=SEED, draw=3)
    assert all(torch.equal(u, v) for u, v in zip(explicit, fused))
    assert not torch.equal(fused[0], launch(ops, tab, MID, x, eps, h, None, sample_index=idx, seed=SEED, draw=4)[0])
    assert not torch.equal(fused[0], launch(ops, tab, MID, x, eps, h, None)[0])                 # no source: no noise
    # a row with s == 0 touches no noise: the last SDE row and every ODE row give the same with and without a source
    ode = schedule(ODE)
    for table, row in ((tab, STEPS - 1), (ode.device_table(DEV), MID)):
        a = launch(ops, table, row, x, eps, h, None, sample_index=idx, seed=SEED, draw=3)
        b = launch(ops, table, row, x, eps, h, None)
        c = launch(ops, table, row, x, eps, h, torch.full_like(x, float("nan")))
        for k in (0, 2, 3, 4):
            assert torch.equal(a[k], b[k]) and torch.equal(c[k], b[k])
        assert torch.isfinite(b[0]).all()


# ------------------------------------------------------------------------------------------ 5. the control block
@pytest.mark.parametrize("algorithm", [ODE, SDE])
def test_control_block_equals_by_value(ops, algorithm):
    sch = schedule(algorithm)
    tab = sch.device_table(DEV)
    N, CHW = 5, 3072
    idx = torch.tensor(INDEX, dtype=torch.int64, device=DEV)
    for row in (0, 1, 2, MID, STEPS - 1):
        x, eps, z, d1, d2 = operands(ops, sch.table[row], N, CHW, 60 + row)
        h = history(row, d1, d2)
        for kw in (dict(z=z.to(DEV)), dict(sample_index=idx)):
            want = launch(ops, tab, row, x, eps, h, kw.get("z"), sample_index=kw.get("sample_index"), seed=SEED, draw=2)
            xd, t, out = x.to(DEV).clone(), torch.full((N,), -5.0, device=DEV), torch.full((N, CHW), 7.0, device=DEV)
            p, hd = torch.empty_like(xd), h.to(DEV).clone()
            ops.dpm_stage(ops.DPM_STEP, tab, t, row=(row + 3) % STEPS, seed=1, draw=9, ctl=control(row, 2, SEED), x=xd, eps=eps.to(DEV),
                          hist=hd, out=out, pred_xstart=p, **kw)
            assert all(torch.equal(u, v) for u, v in zip(want, (xd, t, out, p, hd)))
    t = torch.zeros(3, device=DEV)
    ops.dpm_stage(ops.DPM_FIRST, tab, t, row=0, ctl=control(2, 0, 0))
    assert t.tolist() == [float(sch.tau[-3])] * 3


def test_out_of_range_row_in_the_control_block(ops):
    """The table sits at the start of a larger buffer of NaN-free sentinels: a read past its rows would bring 1e30 into the result
    instead of NaN, and the history is left finite where no slot may be read."""
    sch = schedule(ODE)
    big = torch.full((STEPS + 4, ops.MT_COLS), 1e30, device=DEV)
    big[:STEPS] = sch.table.to(DEV)
    tab = big[:STEPS]
    x, eps, z, d1, d2 = operands(ops, sch.table[MID], 3, 192, 41)
    for row in (STEPS, STEPS + 1, -1 & 0xFFFFFFFF, 1 << 20, 0x7FFFFFFF):
        xd, t, out = x.to(DEV).clone(), torch.zeros(3, device=DEV), torch.zeros(3, 192, device=DEV)
        hd = history(0, d1, d2).to(DEV)
        ops.dpm_stage(ops.DPM_STEP, tab, t, ctl=control(row, 0, 0), x=xd, eps=eps.to(DEV), z=z.to(DEV), hist=hd, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(xd).all() and torch.isnan(out).all() and torch.isnan(t).all()
        assert torch.isnan(hd[0]).all() and torch.equal(hd[1].cpu(), d2) and torch.equal(hd[2].cpu(), d1)
        t.zero_()
        ops.dpm_stage(ops.DPM_FIRST, tab, t, ctl=control(row, 0, 0))
        assert torch.isnan(t).all()
    assert (big[STEPS:] == 1e30).all()


@pytest.mark.parametrize("algorithm", [ODE, SDE])
def test_nan_stays_in_its_image(ops, algorithm):
    sch = schedule(algorithm)
    tab = sch.device_table(DEV)
    for row in (2, STEPS - 1):
        x, eps, z, d1, d2 = operands(ops, sch.table[row], 4, 771, 33)
        h = history(row, d1, d2)
        clean = launch(ops, tab, row, x, eps, h, z)
        bad = eps.clone()
        bad[2] = float("nan")
        got = launch(ops, tab, row, x, bad, h, z)
        last = row == STEPS - 1
        for k in (0, 2, 3) if last else (0, 3):             # x', out (written on the last row only), pred_xstart
            assert torch.isnan(got[k][2]).all()             # the clamps do not swallow it
            for n in (0, 1, 3):
                assert torch.equal(got[k][n], clean[k][n]) and torch.isfinite(got[k][n]).all()
        assert torch.isnan(got[4][row % 3][2]).all() and torch.equal(got[4][row % 3][[0, 1, 3]], clean[4][row % 3][[0, 1, 3]])
        assert torch.equal(got[1], clean[1])
        # a NaN in one image's history stays there too
        if not last:
            hb = h.clone()
            hb[(row - 1) % 3][1] = float("nan")
            got = launch(ops, tab, row, x, eps, hb, z)
            assert torch.isnan(got[0][1]).all() and torch.equal(got[0][[0, 2, 3]], clean[0][[0, 2, 3]])


def test_run_to_run_bits(ops):
    sch = schedule(SDE)
    tab = sch.device_table(DEV)
    x, eps, z, d1, d2 = operands(ops, sch.table[MID], 5, 3072, 21)
    h = history(MID, d1, d2)
    idx = torch.tensor(INDEX, dtype=torch.int64, device=DEV)
    for kw in (dict(z=z), dict(sample_index=idx, seed=SEED, draw=1)):
        a, b = launch(ops, tab, MID, x, eps, h, **kw), launch(ops, tab, MID, x, eps, h, **kw)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_malformed_calls(ops):
    from dxmi_hip import DxmiError
    sch = schedule(ODE)
    tab = sch.device_table(DEV)
    x, eps, z, d1, d2 = (v.to(DEV) for v in operands(ops, sch.table[MID], 4, 768, 2))
    t, out, hist = torch.empty(4, device=DEV), torch.empty(4, 768, device=DEV), torch.zeros(3, 4, 768, device=DEV)
    idx = torch.arange(4, device=DEV)
    step = lambda **kw: ops.dpm_stage(ops.DPM_STEP, **dict(dict(tab=tab, t_out=t, row=MID, x=x, eps=eps, z=z, hist=hist, out=out), **kw))
    bad = [lambda: step(row=STEPS), lambda: step(row=-1), lambda: step(sample_index=idx), lambda: step(eps=eps[:3]),
           lambda: step(eps=eps.double()), lambda: step(x=x.cpu()), lambda: step(out=None), lambda: step(hist=None),
           lambda: step(hist=hist[:2]), lambda: step(hist=hist.double()), lambda: step(hist=hist.cpu()), lambda: step(hist=hist[:, :, :767]),
           lambda: step(tab=tab[:, :8]), lambda: step(t_out=t[:3]), lambda: step(z=None, sample_index=idx.int()),
           lambda: step(ctl=torch.zeros(3, dtype=torch.int32, device=DEV))]
    for i, call in enumerate(bad):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"malformed call {i} was accepted")
    step()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 6. the loop, analytic network
def analytic_net(x, t):
    return 0.8 * torch.tanh(0.9 * x + 1e-3 * t[:, None, None, None])


def dpm_loop64(ops, tab, noise, stale=False):
    """The loop in float64 numpy on the fp32 table -> (the state after every row, the propagated bound after every row).  stale: the
    negative control, D_{k-1} and D_{k-2} change places from row 2 on (what a wrong slot address would read)."""
    K = tab.double().numpy()
    x = noise[0].double().numpy()
    dx = np.zeros_like(x)
    hist, dhist = [], []
    states, bounds = [], []
    for k in range(len(K)):
        cx, w0, w1, w2, s, a, b, t = (K[k][i] for i in (ops.MT_CX, ops.MT_W0, ops.MT_W1, ops.MT_W2, ops.MT_S, ops.MT_A, ops.MT_B, ops.MT_T))
        eps = 0.8 * np.tanh(0.9 * x + 1e-3 * t)
        deps = 0.72 * dx + 8 * U * (0.8 * (np.abs(0.9 * x) + 1e-3 * t) + np.abs(eps))
        d0 = a * x - b * eps
        dd0 = a * dx + b * deps + 8 * U * (np.abs(a * x) + np.abs(b * eps))
        if int(K[k][ops.MT_FLAGS]) & ops.MT_FLAG_CLIP:
            d0 = np.clip(d0, -1, 1)
        acc = cx * x + w0 * d0
        local = np.abs(cx * x) + abs(w0) * (np.abs(a * x) + np.abs(b * eps))
        dacc = abs(cx) * dx + abs(w0) * (a * dx + b * deps)
        for j, w in enumerate((w1, w2)):
            if w != 0:
                j = 1 - j if stale and len(hist) == 2 else j
                acc = acc + w * hist[j]
                local = local + np.abs(w * hist[j])
                dacc = dacc + abs(w) * dhist[j]
        if s != 0:
            z = noise[k + 1].double().numpy()
            acc = acc + s * z
            local = local + np.abs(s * z)
        x, dx = acc, dacc + 8 * U * local
        hist, dhist = [d0] + hist[:1], [dd0] + dhist[:1]
        states.append(x)
        bounds.append(dx)
    return np.stack(states), np.stack(bounds)


def ddim_loop64(dt, tab, noise):
    """ddpm_sample's clip form with eta = 0 in float64 numpy on its fp32 table (columns dt.DT_*) -> (states, propagated bounds), with
    the clip form's stage bound of tests/test_hip_ddpm_sample.py."""
    K = tab.double().numpy()
    x = noise[0].double().numpy()
    dx = np.zeros_like(x)
    states, bounds = [], []
    for k in range(len(K)):
        a, b, q, r, c0, c1, t = (K[k][i] for i in (dt.DT_A, dt.DT_B, dt.DT_Q, dt.DT_R, dt.DT_C0, dt.DT_C1, dt.DT_T))
        assert K[k][dt.DT_S] == 0 and int(K[k][dt.DT_FLAGS]) & dt.DT_FLAG_CLIP
        eps = 0.8 * np.tanh(0.9 * x + 1e-3 * t)
        deps = 0.72 * dx + 8 * U * (0.8 * (np.abs(0.9 * x) + 1e-3 * t) + np.abs(eps))
        x0c = np.clip(a * x - b * eps, -1, 1)
        dx0 = a * dx + b * deps
        eh = (x - q * x0c) * r
        local = (c0 + c1 * r * q) * (a * np.abs(x) + b * np.abs(eps)) + c1 * r * (np.abs(x) + q * np.abs(x0c)) + np.abs(c0 * x0c) + np.abs(c1 * eh)
        x, dx = c0 * x0c + c1 * eh, c0 * dx0 + c1 * r * (dx + q * dx0) + 8 * U * local
        states.append(x)
        bounds.append(dx)
    return np.stack(states), np.stack(bounds)


@pytest.mark.parametrize("algorithm,order", [(ODE, 1), (ODE, 2), (ODE, 3), (SDE, 1), (SDE, 2)])
@pytest.mark.parametrize("clip", [True, False])
def test_loop_with_analytic_network(ops, clip, algorithm, order):
    from models.DxMI.dpm_sample import dpm_sample, dpm_sample_schedule
    S, shape = 6, (4, 3, 8, 8)
    gen = torch.Generator().manual_seed(77)
    noise = [torch.randn(shape, generator=gen) for _ in range(S + 1)]
    sch = dpm_sample_schedule(S, order, algorithm, clip_denoised=clip)
    want, bound = dpm_loop64(ops, sch.table, noise)
    seen = []
    out = dpm_sample(analytic_net, shape, steps=S, order=order, algorithm=algorithm, clip_denoised=clip, device=DEV, noise=noise,
                     callback=lambda d: seen.append(d))
    torch.cuda.synchronize()
    got = torch.stack([d["x"] for d in seen]).cpu().double().numpy()
    err = np.abs(got - want)
    print(f"{algorithm} order {order} clip {clip}: loop vs float64, worst |err| {err.max():.3e}, worst |err| / propagated bound "
          f"{(err / bound).max():.3e} (bound up to {bound.max():.3e})")
    assert (err <= bound).all()
    if order > 1:          # negative control, on the CPU: the bound tells a loop that reads the wrong slot from the right one
        assert (np.abs(dpm_loop64(ops, sch.table, noise, stale=True)[0] - want) > bound).any()
    assert [d["i"] for d in seen] == list(range(S)) and [d["t"] for d in seen] == sch.tau[::-1]
    assert torch.equal(out, seen[-1]["x"].clamp(-1, 1)) and out.abs().max() <= 1 and out.std() > 0.05
    assert torch.equal(seen[-1]["x"], seen[-1]["pred_xstart"])
    if clip:
        assert all(d["pred_xstart"].abs().max() <= 1 for d in seen)
    # the torch path on the CPU states the same expressions
    cpu = dpm_sample(analytic_net, shape, steps=S, order=order, algorithm=algorithm, clip_denoised=clip, device="cpu", noise=noise)
    assert ((cpu - out.cpu()).abs().double().numpy() <= 2 * bound[-1]).all()          # each within the bound of the float64 loop


def test_first_order_loop_is_ddim(ops):
    from models.DxMI.ddpm_sample import ddpm_sample, ddpm_sample_schedule
    from models.DxMI.dpm_sample import dpm_sample, dpm_sample_schedule
    S, shape = 6, (4, 3, 8, 8)
    gen = torch.Generator().manual_seed(78)
    noise = [torch.randn(shape, generator=gen)] + [None] * S
    a_states, b_states = [], []
    a = dpm_sample(analytic_net, shape, steps=S, order=1, skip_type="uniform", clip_denoised=True, device=DEV, noise=noise,
                   callback=lambda d: a_states.append(d["x"]))
    b = ddpm_sample(analytic_net, shape, steps=S, eta=0.0, clip_denoised=True, device=DEV, noise=noise, callback=lambda d: b_states.append(d["x"]))
    torch.cuda.synchronize()
    sa, sb = dpm_sample_schedule(S, 1, skip_type="uniform"), ddpm_sample_schedule(S, 0.0)
    assert sa.tau == sb.tau
    _, bound_a = dpm_loop64(ops, sa.table, noise)
    _, bound_b = ddim_loop64(ops, sb.table, noise)
    diff = (torch.stack(a_states) - torch.stack(b_states)).abs().cpu().double().numpy()
    allowed = bound_a + bound_b
    print(f"order 1 vs DDIM over {S} transitions: worst |difference| {diff.max():.3e}, worst ratio to the allowed {(diff / allowed).max():.3e}")
    assert (diff <= allowed).all() and allowed.max() < 1e-2
    assert ((a - b).abs().cpu().double().numpy() <= allowed[-1]).all() and a.std() > 0.05


# ------------------------------------------------------------------------------------------ 7. the loop on the HIP Model
NET_KW = dict(ch=64, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[8], dropout=0.1, in_channels=3, resolution=16)
SHAPE = (4, 3, 16, 16)


@pytest.fixture(scope="module")
def net(ops):
    """The shrunken Model of tests/test_hip_ddpm_sample.py, in eval mode."""
    from models.DxMI.unet_small import Model
    from oracle.weights import formula_tensor
    m = Model(**NET_KW)
    m.load_state_dict({k: formula_tensor(k, v.shape) for k, v in m.state_dict().items()})
    return m.to(DEV).eval()


def test_replay_equals_eager_with_torch_draws(net):
    from models.DxMI.dpm_sample import dpm_sample, replay_graphs
    S = 6
    kw = dict(steps=S, order=3, device=DEV)
    torch.manual_seed(5)
    eager = dpm_sample(net, SHAPE, **kw).clone()
    assert replay_graphs(net) == []
    torch.manual_seed(5)
    replayed = dpm_sample(net, SHAPE, use_graph=True, **kw).clone()
    assert torch.isfinite(eager).all() and eager.abs().max() <= 1 and eager.std() > 0
    assert torch.equal(eager, replayed)
    graphs = replay_graphs(net)
    assert len(graphs) == 1 and graphs[0].captures == 1 and graphs[0].replays == S - 2
    again = dpm_sample(net, SHAPE, use_graph=True, **kw).clone()      # no seed in between: another x_T
    assert not torch.equal(again, replayed) and graphs[0].captures == 1 and graphs[0].replays == 2 * S - 2
    torch.manual_seed(5)
    from models.cm.random_util import get_generator
    assert torch.equal(dpm_sample(net, SHAPE, generator=get_generator("dummy"), **kw), eager)
    # replay is off with a callback, progress or noise=
    torch.manual_seed(5)
    assert torch.equal(dpm_sample(net, SHAPE, use_graph=True, callback=lambda d: None, **kw), eager)
    assert graphs[0].replays == 2 * S - 2 and len(replay_graphs(net)) == 1


def test_replay_equals_eager_with_the_deterministic_generator(net):
    from models.cm.random_util import get_generator
    from models.DxMI.dpm_sample import dpm_sample, replay_graphs
    S = 6
    gen = get_generator("determ", 64, seed=(1 << 35) + 3)
    kw = dict(steps=S, order=2, algorithm=SDE, device=DEV, generator=gen)
    gen.set_done_samples(8)
    eager = dpm_sample(net, SHAPE, **kw).clone()
    assert gen.draw == S                  # x_T and the S - 1 transitions that add noise
    before = {id(g) for g in replay_graphs(net)}
    gen.set_done_samples(8)
    first = dpm_sample(net, SHAPE, use_graph=True, **kw).clone()
    assert gen.draw == S and torch.equal(first, eager)
    new = [g for g in replay_graphs(net) if id(g) not in before]
    assert len(new) == 1 and new[0].captures == 1 and new[0].replays == S - 2
    gen.set_done_samples(8)
    second = dpm_sample(net, SHAPE, use_graph=True, **kw).clone()
    assert torch.equal(second, first) and new[0].captures == 1 and new[0].replays == 2 * S - 2
    gen.set_done_samples(12)
    assert not torch.equal(dpm_sample(net, SHAPE, use_graph=True, **kw), first)
    # bit for bit what explicit generator draws fed through noise= give
    gen.set_done_samples(8)
    noise = [gen.randn(*SHAPE, device=DEV)]
    noise += [gen.randn_like(noise[0]) for _ in range(S - 1)] + [None]
    assert torch.equal(dpm_sample(net, SHAPE, steps=S, order=2, algorithm=SDE, device=DEV, noise=noise), eager)
    # the ODE solver draws x_T alone
    gen.set_done_samples(8)
    dpm_sample(net, SHAPE, steps=S, order=2, device=DEV, generator=gen, use_graph=True)
    assert gen.draw == 1


def test_batch_invariance(net):
    from models.cm.random_util import get_generator
    from models.DxMI.dpm_sample import dpm_sample
    gen = get_generator("determ", 4, seed=9)
    kw = dict(steps=5, order=2, algorithm=SDE, device=DEV, generator=gen)
    gen.set_done_samples(0)
    whole = dpm_sample(net, (4, 3, 16, 16), **kw).clone()
    parts = []
    for b in range(2):
        gen.set_done_samples(2 * b)
        parts.append(dpm_sample(net, (2, 3, 16, 16), use_graph=True, **kw).clone())
    parts = torch.cat(parts)
    for i in range(4):
        assert torch.equal(parts[i], whole[i]), i
    assert not torch.equal(whole[0], whole[1])


# ------------------------------------------------------------------------------------------ 8. command line
def png_size(path):
    with open(path, "rb") as f:
        head = f.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">II", head[16:24])


def test_generate_cifar10_dpm_solver_cli(tmp_path):
    """A synthetic checkpoint (the built-in configuration's network as initialised, saved as a plain state dict) through
    generate_cifar10.py --solver dpmpp.  One child, under its own time limit (the full-size net: its first pack and one capture)."""
    import configs_builtin
    import dxmi_config
    torch.manual_seed(3)
    ckpt = tmp_path / "teacher.pt"
    torch.save(dxmi_config.instantiate(configs_builtin.get("cifar10_T10").sampler_net).state_dict(), ckpt)
    out = tmp_path / "run"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(PKG, "generate_cifar10.py"), "--log_dir", str(out),
                        "--teacher_ckpt", str(ckpt), "--config", "builtin:cifar10_T10", "--solver", "dpmpp", "--ddpm_steps", "6",
                        "--solver_order", "3", "--skip_type", "logsnr", "-n", "8", "--batchsize", "4", "--skip_fid", "--generator", "determ"],
                       cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "DPM-Solver++ (dpmsolver++), 6 logsnr steps, order 3" in r.stdout
    names = sorted(os.listdir(out / "generated"))
    assert names == [f"0_{i}.png" for i in range(8)]
    assert all(png_size(out / "generated" / n) == (32, 32) for n in names)
    assert len({(out / "generated" / n).read_bytes() for n in names}) > 1
