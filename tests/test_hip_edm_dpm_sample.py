"""DPM-Solver++ on the EDM nets on the device: dxmi_edm_dpm_stage against float64 on the same fp32 operands, FIRST, history that
was never written, its fused noise against dxmi_randn_indexed, the device control block and its poisoning, the loop against a
float64 loop with an analytic network, first order against sample_euler, replay against eager and batch invariance on the shrunken
HIP UNetModel, and generate_large.py --karras_sampler dpmpp / sde-dpmpp.

Bounds (u = 2^-24), counted from the kernel's operations on the fp32 table values K widened to float64, per element:
  D0      8 u (|c_skip x| + |c_out F|)   (pred_xstart and the written history slot): two products and their sum, the clamp is continuous
  stage   8 u (|cx x| + |w0| (|c_skip x| + |c_out F|) + |w1 D1| + |w2 D2| + |s z|): every term is rounded at most three times at half
          an ulp (its own product, the product or sum it enters, the running sum)
  x_in    is not bounded but exact: fp32(c_in_next) x' of the device's own x', one product
  loop    the stage bound propagated row by row through the float64 loop.  With d(v) a bound on |device v - float64 v|:
            d(x_0)  = u |x_0|                                               FIRST's one product x_T sigma_max
            d(x_in) = c_in d(x) + u |c_in x|                                one product
            d(F)    = 0.72 d(x_in) + 8 u (0.8 (|0.9 x_in| + |1e-3 t|) + |F|)   the analytic network 0.8 tanh(0.9 x_in + 1e-3 t) has slope
                                                                            <= 0.72; its fp32 evaluation rounds the two products,
                                                                            their sum, tanh (2 ulp) and the scaling
            d(D0)   = c_skip d(x) + c_out d(F) + 8 u (|c_skip x| + |c_out F|)  the clamp has slope <= 1
            d(x')   = |cx| d(x) + |w0| (c_skip d(x) + c_out d(F)) + |w1| d(D1) + |w2| d(D2) + stage bound
  euler   sample_euler's row is the same map written as den = c_out F + c_skip x, d = (x - den) / sigma, x' = x + d dt, in exact
          arithmetic x' = (1 + dt / sigma) x - (dt / sigma) den, so
            d(x')   = |1 + dt / sigma| d(x) + |dt / sigma| d(den) + 8 u (|x| + |d dt|) + |dt / sigma| 8 u (|x| + |den| + |c_skip x| + |c_out F|)
          (d is rounded in its difference and its quotient, the update in its product and its sum); the two device loops may differ
          by the sum of the two propagated bounds (a table entry is one rounding away from its float64 value, which the 8 u per
          term, counted for 1.5 u of arithmetic, leaves room for)."""
import os
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


def diffusion():
    from models.cm.karras_diffusion import KarrasDenoiser
    return KarrasDenoiser()


def schedule(algorithm, clip=True, steps=STEPS, order=None, **kw):
    from models.cm.dpm_sample import edm_dpm_schedule
    return edm_dpm_schedule(diffusion(), steps, (3 if algorithm == ODE else 2) if order is None else order, algorithm,
                            clip_denoised=clip, **kw)


_OPERANDS = {}


def operands(ops, row, N, CHW, seed):
    """x, F, z, D1, D2 (CPU fp32, computed once per key) with about half of the data prediction outside [-1, 1]:
    x = x0 + sigma e, F = (x0 - c_skip x) / c_out, x0 uniform in [-2, 2]; D1, D2 uniform in [-1, 1]."""
    key = (float(row[ops.ET_SIGMA]), N, CHW, seed)
    if key not in _OPERANDS:
        gen = torch.Generator().manual_seed(seed)
        x0 = torch.rand(N, CHW, generator=gen) * 4 - 2
        e = torch.randn(N, CHW, generator=gen)
        z = torch.randn(N, CHW, generator=gen)
        d1, d2 = torch.rand(N, CHW, generator=gen) * 2 - 1, torch.rand(N, CHW, generator=gen) * 2 - 1
        x = (x0 + float(row[ops.ET_SIGMA]) * e).float()
        F = ((x0 - float(row[ops.ET_CSKIP]) * x) / float(row[ops.ET_COUT])).float()
        _OPERANDS[key] = (x, F, z, d1, d2)
    return _OPERANDS[key]


def history(k, d1, d2, fill=SENTINEL):
    """[3, N, CHW] with D_{k-1} and D_{k-2} where row k looks for them and `fill` in the slot it writes."""
    h = torch.full((3,) + tuple(d1.shape), fill)
    h[(k - 1) % 3], h[(k - 2) % 3] = d1, d2
    return h


def oracle(ops, row, x, F, z, d1, d2):
    """float64 on the fp32 operands -> (x', D0, bound, bound of D0)."""
    K = row.double().numpy()
    x, F, z, d1, d2 = (v.double().numpy() for v in (x, F, z, d1, d2))
    cx, w0, w1, w2, s, c_skip, c_out = (K[i] for i in (ops.ET_CX, ops.ET_W0, ops.ET_W1, ops.ET_W2, ops.ET_S, ops.ET_CSKIP, ops.ET_COUT))
    d0 = c_out * F + c_skip * x
    if int(K[ops.ET_FLAGS]) & ops.ET_FLAG_CLIP:
        d0 = np.clip(d0, -1, 1)
    xn = cx * x + w0 * d0 + w1 * d1 + w2 * d2 + s * z
    pbound = 8 * U * (np.abs(c_skip * x) + np.abs(c_out * F))
    bound = 8 * U * (np.abs(cx * x) + abs(w0) * (np.abs(c_skip * x) + np.abs(c_out * F)) + np.abs(w1 * d1) + np.abs(w2 * d2) + np.abs(s * z))
    return xn, d0, bound, pbound


def launch(ops, tab, row, x, F, hist, z=None, pred=True, **kw):
    """One by-value launch on copies -> (x', t_out, out, pred_xstart, hist, x_in); out is pre-filled with 7, x_in with SENTINEL."""
    xd, t = x.to(DEV).clone(), torch.full((x.shape[0],), -5.0, device=DEV)
    out, x_in = torch.full_like(xd, 7.0), torch.full_like(xd, SENTINEL)
    p = torch.empty_like(xd) if pred else None
    hd = hist.to(DEV).clone()
    ops.edm_dpm_stage(ops.EDM_DPM_STEP, tab, t, row=row, x=xd, model_out=F.to(DEV), z=None if z is None else z.to(DEV), hist=hd,
                      x_in=x_in, out=out, pred_xstart=p, **kw)
    torch.cuda.synchronize()
    return xd, t, out, p, hd, x_in


# ------------------------------------------------------------------------------------------ 1. the launch against float64
@pytest.mark.parametrize("algorithm", [ODE, SDE])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("N,CHW", SHAPES)
def test_stage_vs_fp64(ops, N, CHW, clip, algorithm):
    sch = schedule(algorithm, clip)
    tab = sch.device_table(DEV)
    top = 3 if algorithm == ODE else 2
    assert sch.table[:3, ops.ET_ORDER].tolist() == [1, 2, top] and sch.table[-1, ops.ET_ORDER] == 1
    worst = 0.0
    for row, neighbour in ((0, 1), (1, 2), (2, 3), (STEPS - 1, STEPS - 2)):
        K = sch.table[row]
        x, F, z, d1, d2 = operands(ops, K, N, CHW, 100 * row + CHW)
        got, t_out, out, pred, hist, x_in = launch(ops, tab, row, x, F, history(row, d1, d2), z)
        want, want_d0, bound, pbound = oracle(ops, K, x, F, z, d1, d2)
        clipped = (np.abs(want_d0) >= 1).mean() if clip else (np.abs(want_d0) > 1).mean()
        assert 0.3 < clipped < 0.7, clipped
        err = np.abs(got.cpu().double().numpy() - want)
        perr = np.abs(pred.cpu().double().numpy() - want_d0)
        worst = max(worst, (err / bound).max(), (perr / pbound).max())
        print(f"({N}, {CHW}) clip {clip} {algorithm} row {row}: worst |err| / bound = {(err / bound).max():.3e}, pred_xstart "
              f"{(perr / pbound).max():.3e}")
        assert (err <= bound).all() and (perr <= pbound).all()
        # negative control, on the CPU: the neighbouring row's coefficients must not pass
        other = oracle(ops, sch.table[neighbour], x, F, z, d1, d2)[0]
        assert (np.abs(other - want) > bound).any()
        # the written slot is D0 to the bit, the two others are as they were
        assert torch.equal(hist[row % 3], pred)
        assert torch.equal(hist[(row - 1) % 3].cpu(), d1) and torch.equal(hist[(row - 2) % 3].cpu(), d2)
        last = row == STEPS - 1
        assert torch.equal(t_out.cpu(), torch.full((N,), float(K[ops.ET_T_NEXT])))
        assert t_out[0].item() == (0.0 if last else (1000 * 0.25 * torch.log(sch.sigmas[row + 1].reshape(1) + 1e-44)).item())
        assert torch.equal(out, got.clamp(-1, 1) if last else torch.full_like(out, 7.0))
        # the next evaluation's input: one fp32 product of the device's own x'; untouched on the last row
        c_next = sch.table[row, ops.ET_CIN_NEXT].to(DEV)
        assert torch.equal(x_in, torch.full_like(x_in, SENTINEL) if last else c_next * got)
        if last:
            assert torch.equal(got, pred)             # cx = 0, w0 = 1: x' = 0 x + 1 D0
        else:
            assert c_next.item() == diffusion().get_scalings(sch.sigmas[row + 1].reshape(1))[2].item()
        # pred_xstart is optional and changes nothing else
        bare = launch(ops, tab, row, x, F, history(row, d1, d2), z, pred=False)
        assert bare[3] is None and all(torch.equal(u, v) for u, v in zip((got, t_out, out, hist, x_in), (bare[0], bare[1], bare[2], bare[4], bare[5])))
    print(f"({N}, {CHW}) clip {clip} {algorithm}: worst ratio to the bound over the rows {worst:.3e}")


def test_last_row_takes_no_x_in(ops):
    sch = schedule(ODE)
    tab = sch.device_table(DEV)
    x, F, z, d1, d2 = operands(ops, sch.table[STEPS - 1], 2, 192, 5)
    want = launch(ops, tab, STEPS - 1, x, F, history(STEPS - 1, d1, d2))
    xd, t, out, hd = x.to(DEV).clone(), torch.empty(2, device=DEV), torch.empty(2, 192, device=DEV), history(STEPS - 1, d1, d2).to(DEV)
    ops.edm_dpm_stage(ops.EDM_DPM_STEP, tab, t, row=STEPS - 1, x=xd, model_out=F.to(DEV), hist=hd, out=out)
    assert torch.equal(xd, want[0]) and torch.equal(out, want[2]) and torch.equal(hd, want[4])


# ------------------------------------------------------------------------------------------ 2. FIRST
@pytest.mark.parametrize("N,CHW", SHAPES)
def test_first_mode(ops, N, CHW):
    sch = schedule(ODE)
    tab = sch.device_table(DEV)
    gen = torch.Generator().manual_seed(CHW)
    x = torch.randn(N, CHW, generator=gen)
    for row in (0, 3):
        xd, x_in, t = x.to(DEV).clone(), torch.full((N, CHW), SENTINEL, device=DEV), torch.full((N,), -1.0, device=DEV)
        guard = torch.full((3, N, CHW), SENTINEL, device=DEV)          # nothing else is written: no other pointer is handed over
        ops.edm_dpm_stage(ops.EDM_DPM_FIRST, tab, t, row=row, x=xd, x_in=x_in)
        torch.cuda.synchronize()
        K = sch.table[row]
        want_x = x * K[ops.ET_XSCALE]
        assert K[ops.ET_XSCALE].item() == np.float32(80.0)
        assert torch.equal(xd.cpu(), want_x) and torch.equal(x_in.cpu(), K[ops.ET_CIN] * want_x)
        assert torch.equal(t.cpu(), torch.full((N,), float(K[ops.ET_T]))) and (guard == SENTINEL).all()
    assert sch.table[0, ops.ET_T].item() == (1000 * 0.25 * torch.log(sch.sigmas[0].reshape(1) + 1e-44)).item()


# ------------------------------------------------------------------------------------------ 3. history that was never written
@pytest.mark.parametrize("algorithm", [ODE, SDE])
@pytest.mark.parametrize("N,CHW", [(3, 75), (5, 3072)])
def test_unwritten_history_is_not_read(ops, N, CHW, algorithm):
    """S = 6: the orders are 1, 2, 3, 3, 2, 1 (ODE, order 3) and 1, 2, 2, 2, 2, 1 (SDE, order 2).  Every slot a row's order does not
    name, and the slot it writes, holds NaN in one launch and 0 in the other."""
    S = 6
    sch = schedule(algorithm, steps=S)
    tab = sch.device_table(DEV)
    orders = [int(o) for o in sch.table[:, ops.ET_ORDER]]
    assert orders == ([1, 2, 3, 3, 2, 1] if algorithm == ODE else [1, 2, 2, 2, 2, 1])
    checked = 0
    for row in range(S):
        o = orders[row]
        if o == 3:
            continue
        x, F, z, d1, d2 = operands(ops, sch.table[row], N, CHW, 7 + row)
        runs = []
        for fill in (float("nan"), 0.0):
            h = history(row, d1, d2, fill)
            for j in (1, 2):
                if j >= o:
                    h[(row - j) % 3] = fill
            if row == 0:
                assert bool(torch.isnan(h).all()) == (fill != 0.0)
            runs.append(launch(ops, tab, row, x, F, h, z))
        a, b = runs
        for k in (0, 1, 3):          # x', t_out, pred_xstart
            assert torch.equal(a[k], b[k]) and torch.isfinite(a[k]).all()
        assert torch.equal(a[2], b[2]) and torch.equal(a[5], b[5]) and (row == S - 1 or torch.isfinite(a[5]).all())
        assert torch.equal(a[4][row % 3], b[4][row % 3]) and torch.isfinite(a[4][row % 3]).all()
        checked += 1
    assert checked == (4 if algorithm == ODE else 6)
    # and the control: a row of full order does read both slots
    row = 2 if algorithm == ODE else 1
    x, F, z, d1, d2 = operands(ops, sch.table[row], N, CHW, 7 + row)
    h = history(row, d1, d2)
    h[(row - (2 if algorithm == ODE else 1)) % 3] = float("nan")
    got = launch(ops, tab, row, x, F, h, z)
    assert torch.isnan(got[0]).all() and torch.isnan(got[5]).all()


# ------------------------------------------------------------------------------------------ 4. fused noise
SEED = (1 << 40) + 12345
INDEX = [5, (1 << 33) + 7, 123456, 0, 99]            # global indices that are neither contiguous nor ordered
MID = 4


def control(row, draw, seed):
    return torch.from_numpy(np.array([row & 0xFFFFFFFF, draw, seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32).view(np.int32)).to(DEV)


@pytest.mark.parametrize("N,CHW", [(3, 75), (5, 3072), (1, 5000)])
def test_fused_noise_is_randn_indexed(ops, N, CHW):
    sch = schedule(SDE)
    tab = sch.device_table(DEV)
    assert sch.table[MID, ops.ET_S] != 0
    x, F, _, d1, d2 = operands(ops, sch.table[MID], N, CHW, 9)
    h = history(MID, d1, d2)
    idx = torch.tensor(INDEX[:N], dtype=torch.int64, device=DEV)
    z = ops.randn_indexed(idx, (CHW,), SEED, 3)
    explicit = launch(ops, tab, MID, x, F, h, z)
    fused = launch(ops, tab, MID, x, F, h, None, sample_index=idx, seed=SEED, draw=3)
    assert all(torch.equal(u, v) for u, v in zip(explicit, fused))
    assert not torch.equal(fused[0], launch(ops, tab, MID, x, F, h, None, sample_index=idx, seed=SEED, draw=4)[0])
    assert not torch.equal(fused[0], launch(ops, tab, MID, x, F, h, None)[0])                 # no source: no noise
    # a row with s == 0 touches no noise: the last SDE row and every ODE row give the same with and without a source
    ode = schedule(ODE)
    for table, row in ((tab, STEPS - 1), (ode.device_table(DEV), MID)):
        a = launch(ops, table, row, x, F, h, None, sample_index=idx, seed=SEED, draw=3)
        b = launch(ops, table, row, x, F, h, None)
        c = launch(ops, table, row, x, F, h, torch.full_like(x, float("nan")))
        for k in (0, 2, 3, 4, 5):
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
        x, F, z, d1, d2 = operands(ops, sch.table[row], N, CHW, 60 + row)
        h = history(row, d1, d2)
        for kw in (dict(z=z.to(DEV)), dict(sample_index=idx)):
            want = launch(ops, tab, row, x, F, h, kw.get("z"), sample_index=kw.get("sample_index"), seed=SEED, draw=2)
            xd, t, out = x.to(DEV).clone(), torch.full((N,), -5.0, device=DEV), torch.full((N, CHW), 7.0, device=DEV)
            p, hd, x_in = torch.empty_like(xd), h.to(DEV).clone(), torch.full((N, CHW), SENTINEL, device=DEV)
            ops.edm_dpm_stage(ops.EDM_DPM_STEP, tab, t, row=(row + 3) % STEPS, seed=1, draw=9, ctl=control(row, 2, SEED), x=xd,
                              model_out=F.to(DEV), hist=hd, x_in=x_in, out=out, pred_xstart=p, **kw)
            assert all(torch.equal(u, v) for u, v in zip(want, (xd, t, out, p, hd, x_in)))
    x = torch.randn(3, 192)
    by_value = (x.to(DEV).clone(), torch.empty(3, 192, device=DEV), torch.zeros(3, device=DEV))
    block = (x.to(DEV).clone(), torch.empty(3, 192, device=DEV), torch.zeros(3, device=DEV))
    ops.edm_dpm_stage(ops.EDM_DPM_FIRST, tab, by_value[2], row=2, x=by_value[0], x_in=by_value[1])
    ops.edm_dpm_stage(ops.EDM_DPM_FIRST, tab, block[2], row=0, ctl=control(2, 0, 0), x=block[0], x_in=block[1])
    assert all(torch.equal(u, v) for u, v in zip(by_value, block)) and block[2].tolist() == [float(sch.table[2, ops.ET_T])] * 3


def test_out_of_range_row_in_the_control_block(ops):
    """The poisoning contract of the stage launches, not a fault: the table sits at the start of a larger buffer of NaN-free
    sentinels, so a read past its rows would bring 1e30 into the result instead of NaN; both history weights are forced to 0, so
    no slot is read, and the two slots that are not slot 0 are left as they were."""
    sch = schedule(ODE)
    big = torch.full((STEPS + 4, ops.ET_COLS), 1e30, device=DEV)
    big[:STEPS] = sch.table.to(DEV)
    tab = big[:STEPS]
    x, F, z, d1, d2 = operands(ops, sch.table[MID], 3, 192, 41)
    for row in (STEPS, STEPS + 1, -1, 1 << 20, 0x7FFFFFFF):
        xd, t, out = x.to(DEV).clone(), torch.zeros(3, device=DEV), torch.zeros(3, 192, device=DEV)
        x_in = torch.zeros(3, 192, device=DEV)
        hd = history(0, d1, d2).to(DEV)
        ops.edm_dpm_stage(ops.EDM_DPM_STEP, tab, t, ctl=control(row, 0, 0), x=xd, model_out=F.to(DEV), z=z.to(DEV), hist=hd, x_in=x_in,
                          out=out)
        torch.cuda.synchronize()
        assert torch.isnan(xd).all() and torch.isnan(out).all() and torch.isnan(t).all() and torch.isnan(x_in).all()
        assert torch.isnan(hd[0]).all() and torch.equal(hd[1].cpu(), d2) and torch.equal(hd[2].cpu(), d1)
        t.zero_()
        xd, x_in = x.to(DEV).clone(), torch.zeros(3, 192, device=DEV)
        ops.edm_dpm_stage(ops.EDM_DPM_FIRST, tab, t, ctl=control(row, 0, 0), x=xd, x_in=x_in)
        assert torch.isnan(t).all() and torch.isnan(xd).all() and torch.isnan(x_in).all()
    assert (big[STEPS:] == 1e30).all()


@pytest.mark.parametrize("algorithm", [ODE, SDE])
def test_nan_stays_in_its_image(ops, algorithm):
    sch = schedule(algorithm)
    tab = sch.device_table(DEV)
    for row in (2, STEPS - 1):
        x, F, z, d1, d2 = operands(ops, sch.table[row], 4, 771, 33)
        h = history(row, d1, d2)
        clean = launch(ops, tab, row, x, F, h, z)
        bad = F.clone()
        bad[2] = float("nan")
        got = launch(ops, tab, row, x, bad, h, z)
        last = row == STEPS - 1
        for k in (0, 2, 3) if last else (0, 3, 5):          # x', out (the last row only), pred_xstart, x_in (every other row)
            assert torch.isnan(got[k][2]).all()             # the clamps do not swallow it
            for n in (0, 1, 3):
                assert torch.equal(got[k][n], clean[k][n]) and torch.isfinite(got[k][n]).all()
        assert torch.isnan(got[4][row % 3][2]).all() and torch.equal(got[4][row % 3][[0, 1, 3]], clean[4][row % 3][[0, 1, 3]])
        assert torch.equal(got[1], clean[1])


def test_malformed_calls(ops):
    from dxmi_hip import DxmiError
    sch = schedule(ODE)
    tab = sch.device_table(DEV)
    x, F, z, d1, d2 = (v.to(DEV) for v in operands(ops, sch.table[MID], 4, 768, 2))
    t, out, hist = torch.empty(4, device=DEV), torch.empty(4, 768, device=DEV), torch.zeros(3, 4, 768, device=DEV)
    x_in, idx = torch.empty(4, 768, device=DEV), torch.arange(4, device=DEV)
    step = lambda **kw: ops.edm_dpm_stage(ops.EDM_DPM_STEP, **dict(dict(tab=tab, t_out=t, row=MID, x=x, model_out=F, z=z, hist=hist,
                                                                        x_in=x_in, out=out), **kw))
    first = lambda **kw: ops.edm_dpm_stage(ops.EDM_DPM_FIRST, **dict(dict(tab=tab, t_out=t, row=0, x=x.clone(), x_in=x_in), **kw))
    bad = [lambda: step(row=STEPS), lambda: step(row=-1), lambda: step(sample_index=idx), lambda: step(model_out=F[:3]),
           lambda: step(model_out=F.double()), lambda: step(x=x.cpu()), lambda: step(out=None), lambda: step(hist=None),
           lambda: step(hist=hist[:2]), lambda: step(hist=hist.double()), lambda: step(hist=hist[:, :, :767]),
           lambda: step(x_in=None), lambda: step(x_in=None, row=STEPS - 1, ctl=torch.zeros(4, dtype=torch.int32, device=DEV)),
           lambda: step(x_in=x_in[:3]), lambda: step(x_in=x_in.double()), lambda: step(x_in=x_in.cpu()),
           lambda: step(tab=tab[:, :8]), lambda: step(t_out=t[:3]), lambda: step(z=None, sample_index=idx.int()),
           lambda: step(ctl=torch.zeros(3, dtype=torch.int32, device=DEV)),
           lambda: first(x=None), lambda: first(x_in=None), lambda: first(x_in=x_in[:3]), lambda: first(row=STEPS)]
    for i, call in enumerate(bad):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"malformed call {i} was accepted")
    step()
    step(row=STEPS - 1, x_in=None)
    first()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 6. the loop, analytic network
def analytic_net(x_in, t):
    """|dF / dx_in| <= 0.8 * 0.9 = 0.72."""
    return 0.8 * torch.tanh(0.9 * x_in + 1e-3 * t[:, None, None, None])


def net_bound(x_in, t, F, dx_in):
    return 0.72 * dx_in + 8 * U * (0.8 * (np.abs(0.9 * x_in) + abs(1e-3 * t)) + np.abs(F))


def edm_loop64(ops, tab, noise, stale=False):
    """The loop in float64 numpy on the fp32 table -> (the state after every row, the propagated bound after every row).  stale: the
    negative control, D_{k-1} and D_{k-2} change places from row 2 on (what a wrong slot address would read)."""
    K = tab.double().numpy()
    x = noise[0].double().numpy() * K[0][ops.ET_XSCALE]
    dx = U * np.abs(x)
    hist, dhist = [], []
    states, bounds = [], []
    for k in range(len(K)):
        cx, w0, w1, w2, s, c_skip, c_out, c_in, t = (K[k][i] for i in (ops.ET_CX, ops.ET_W0, ops.ET_W1, ops.ET_W2, ops.ET_S, ops.ET_CSKIP,
                                                                        ops.ET_COUT, ops.ET_CIN, ops.ET_T))
        x_in = c_in * x
        F = 0.8 * np.tanh(0.9 * x_in + 1e-3 * t)
        dF = net_bound(x_in, t, F, c_in * dx + U * np.abs(x_in))
        d0 = c_out * F + c_skip * x
        dd0 = c_skip * dx + c_out * dF + 8 * U * (np.abs(c_skip * x) + np.abs(c_out * F))
        if int(K[k][ops.ET_FLAGS]) & ops.ET_FLAG_CLIP:
            d0 = np.clip(d0, -1, 1)
        acc = cx * x + w0 * d0
        local = np.abs(cx * x) + abs(w0) * (np.abs(c_skip * x) + np.abs(c_out * F))
        dacc = abs(cx) * dx + abs(w0) * (c_skip * dx + c_out * dF)
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


def euler_loop64(kt, tab, x0):
    """sample_euler in float64 numpy on its fp32 table (columns kt.KT_*, row 0 is FIRST) from the scaled state x0 -> (the state
    after every step, the propagated bounds), with the docstring's bound of its row."""
    K = tab.double().numpy()
    x = x0.double().numpy()
    dx = np.zeros_like(x)                      # x0 is handed over as fp32: both loops start from the same bits
    states, bounds = [], []
    for k in range(1, len(K)):
        sig, c_skip, c_out, dt = (K[k][i] for i in (kt.KT_SIGMA, kt.KT_CSKIP, kt.KT_COUT, kt.KT_DT))
        c_in, t = K[k - 1][kt.KT_CIN], K[k - 1][kt.KT_T]
        assert K[k][kt.KT_CLIP] == 1
        x_in = c_in * x
        F = 0.8 * np.tanh(0.9 * x_in + 1e-3 * t)
        dF = net_bound(x_in, t, F, c_in * dx + U * np.abs(x_in))
        raw = c_out * F + c_skip * x
        den = np.clip(raw, -1, 1)
        dden = c_skip * dx + c_out * dF
        d = (x - den) / sig
        g = abs(dt / sig)
        local = 8 * U * (np.abs(x) + np.abs(d * dt)) + g * 8 * U * (np.abs(x) + np.abs(den) + np.abs(c_skip * x) + np.abs(c_out * F))
        x, dx = x + d * dt, abs(1 + dt / sig) * dx + g * dden + local
        states.append(x)
        bounds.append(dx)
    return np.stack(states), np.stack(bounds)


@pytest.mark.parametrize("algorithm,order", [(ODE, 3), (SDE, 2)])
@pytest.mark.parametrize("clip", [True, False])
def test_loop_with_analytic_network(ops, clip, algorithm, order):
    from models.cm.dpm_sample import edm_dpm_sample, edm_dpm_schedule
    S, shape = 6, (5, 3, 32, 32)
    gen = torch.Generator().manual_seed(77)
    noise = [torch.randn(shape, generator=gen) for _ in range(S + 1)]
    sch = edm_dpm_schedule(diffusion(), S, order, algorithm, clip_denoised=clip)
    want, bound = edm_loop64(ops, sch.table, noise)
    seen = []
    out = edm_dpm_sample(diffusion(), analytic_net, shape, steps=S, order=order, algorithm=algorithm, clip_denoised=clip, device=DEV,
                         noise=noise, callback=lambda d: seen.append(d))
    torch.cuda.synchronize()
    got = torch.stack([d["x"] for d in seen]).cpu().double().numpy()
    err = np.abs(got - want)
    print(f"{algorithm} order {order} clip {clip}: loop vs float64, worst |err| {err.max():.3e}, worst |err| / propagated bound "
          f"{(err / bound).max():.3e} (bound up to {bound.max():.3e})")
    assert (err <= bound).all()
    # negative control, on the CPU: the bound tells a loop that reads the wrong slot from the right one
    assert (np.abs(edm_loop64(ops, sch.table, noise, stale=True)[0] - want) > bound).any()
    assert [d["i"] for d in seen] == list(range(S)) and [float(d["sigma"]) for d in seen] == sch.sigmas.tolist()
    assert torch.equal(out, seen[-1]["x"].clamp(-1, 1)) and out.abs().max() <= 1 and out.std() > 0.05
    assert torch.equal(seen[-1]["x"], seen[-1]["pred_xstart"])
    if clip:
        assert all(d["pred_xstart"].abs().max() <= 1 for d in seen)
    # the torch path on the CPU states the same expressions
    cpu = edm_dpm_sample(diffusion(), analytic_net, shape, steps=S, order=order, algorithm=algorithm, clip_denoised=clip, device="cpu",
                         noise=noise)
    assert ((cpu - out.cpu()).abs().double().numpy() <= 2 * bound[-1]).all()          # each within the bound of the float64 loop


# ------------------------------------------------------------------------------------------ 7. first order is sample_euler
def test_first_order_loop_is_sample_euler(ops):
    from models.cm.dpm_sample import edm_dpm_sample, edm_dpm_schedule, edm_sigmas
    from models.cm.karras_diffusion import KarrasDenoiserFn, _schedule, sample_euler
    S, shape = 6, (5, 3, 32, 32)
    gen = torch.Generator().manual_seed(78)
    noise = [torch.randn(shape, generator=gen)] + [None] * S
    a_states, b_states = [], []
    a = edm_dpm_sample(diffusion(), analytic_net, shape, steps=S, order=1, device=DEV, noise=noise, callback=lambda d: a_states.append(d["x"]))
    sigmas = torch.cat([edm_sigmas(S), torch.zeros(1)])
    x0 = noise[0] * np.float32(80.0)                                         # FIRST's product, the same bits
    den = KarrasDenoiserFn(diffusion(), analytic_net, True)
    b = sample_euler(den, x0.to(DEV), sigmas, None, callback=lambda d: b_states.append(d["x"]))       # d["x"]: the state BEFORE step i
    torch.cuda.synchronize()
    sa, sb = edm_dpm_schedule(diffusion(), S, 1), _schedule(sigmas, "euler", den, 1.0, 0.0, 0.0, float("inf"), 1.0)
    assert torch.equal(sa.sigmas, sigmas[:-1]) and torch.equal(b_states[0].cpu(), x0)
    _, bound_a = edm_loop64(ops, sa.table, noise)
    _, bound_b = euler_loop64(ops, sb.table, x0)
    diff = (torch.stack(a_states[:-1]) - torch.stack(b_states[1:])).abs().cpu().double().numpy()
    allowed = (bound_a + bound_b)[:-1]
    print(f"order 1 vs sample_euler over {S} rows: worst |difference| {diff.max():.3e}, worst ratio to the allowed {(diff / allowed).max():.3e} "
          f"(allowed up to {allowed.max():.3e})")
    assert (diff <= allowed).all() and allowed.max() < 1e-2
    assert ((a - b).abs().cpu().double().numpy() <= (bound_a + bound_b)[-1]).all() and a.std() > 0.05


# ------------------------------------------------------------------------------------------ 8. the loop on the HIP UNetModel
SHAPE = (5, 3, 16, 16)
LABELS = [3, 871, 12, 500, 999]


class Counting:
    """The network behind a call counter (dxmi_hip.graph.pack_modules finds the U-Net as `.net`)."""

    def __init__(self, net):
        self.net, self.calls, self.labels = net, 0, []

    def __call__(self, x_in, t, **kw):
        self.calls += 1
        self.labels.append(kw["y"].clone())
        return self.net(x_in, t, **kw)


@pytest.fixture(scope="module")
def unet(ops):
    """The shrunken class-conditional UNetModel of tests/test_hip_edm.py with formula weights, in eval mode."""
    from test_hip_edm import TINY_KW, build
    net, diff, _ = build(TINY_KW)
    assert net.num_classes is not None
    return net, diff


def test_replay_equals_eager_on_the_unet(unet):
    from models.cm.dpm_sample import edm_dpm_sample, replay_graphs
    net, diff = unet
    model = Counting(net)
    S = 6
    y = torch.tensor(LABELS, device=DEV)
    kw = dict(steps=S, order=3, device=DEV, model_kwargs={"y": y})
    torch.manual_seed(5)
    eager = edm_dpm_sample(diff, model, SHAPE, **kw).clone()
    assert model.calls == S and replay_graphs(model) == [] and all(torch.equal(v, y) for v in model.labels)
    assert torch.isfinite(eager).all() and eager.abs().max() <= 1 and eager.std() > 0
    model.calls = 0
    torch.manual_seed(5)
    first = edm_dpm_sample(diff, model, SHAPE, use_graph=True, **kw).clone()
    assert torch.equal(first, eager) and model.calls == 2                   # python ran for the warm-up row and the capture
    graphs = replay_graphs(model)
    assert len(graphs) == 1 and graphs[0].captures == 1 and graphs[0].replays == S - 2
    model.calls = 0
    torch.manual_seed(5)
    second = edm_dpm_sample(diff, model, SHAPE, use_graph=True, **kw).clone()
    assert torch.equal(second, eager) and model.calls == 0 and graphs[0].captures == 1 and graphs[0].replays == 2 * S - 2
    # the labels are a static buffer: other labels through the same graph give what the eager loop gives for them
    y2 = torch.tensor(LABELS[::-1], device=DEV)
    torch.manual_seed(5)
    other = edm_dpm_sample(diff, model, SHAPE, use_graph=True, **dict(kw, model_kwargs={"y": y2})).clone()
    torch.manual_seed(5)
    assert model.calls == 0 and not torch.equal(other, eager)
    assert torch.equal(other, edm_dpm_sample(diff, model, SHAPE, **dict(kw, model_kwargs={"y": y2})))
    # replay is off with a callback
    model.calls = 0
    torch.manual_seed(5)
    assert torch.equal(edm_dpm_sample(diff, model, SHAPE, use_graph=True, callback=lambda d: None, **kw), eager) and model.calls == S
    assert len(replay_graphs(model)) == 1


@pytest.mark.parametrize("kind", ["determ", "determ-indiv"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_batch_invariance_with_the_deterministic_generators(unet, use_graph, kind):
    from models.cm.dpm_sample import edm_dpm_sample
    from models.cm.random_util import get_generator
    net, diff = unet
    S = 5
    y = torch.tensor(LABELS, device=DEV)
    gen = get_generator(kind, 5, seed=(1 << 35) + 3)

    def run(done, rows):
        gen.set_done_samples(done)
        out = edm_dpm_sample(diff, net, (rows.stop - rows.start, 3, 16, 16), steps=S, order=2, algorithm=SDE, device=DEV,
                             generator=gen, model_kwargs={"y": y[rows]}, use_graph=use_graph).clone()
        assert gen.draw == S                  # x_T and the S - 1 transitions that add noise
        return out
    whole = run(0, slice(0, 5))
    parts = torch.cat([run(0, slice(0, 2)), run(2, slice(2, 5))])
    assert torch.isfinite(whole).all() and whole.abs().max() <= 1 and whole.std() > 0.05
    for i in range(5):
        assert torch.equal(parts[i], whole[i]), i
    assert not torch.equal(whole[0], whole[1])
    if use_graph:       # the replayed loop is the eager loop, bit for bit
        gen.set_done_samples(0)
        eager = edm_dpm_sample(diff, net, SHAPE, steps=S, order=2, algorithm=SDE, device=DEV, generator=gen, model_kwargs={"y": y})
        assert torch.equal(eager, whole)
    else:               # bit for bit what explicit generator draws fed through noise= give
        gen.set_done_samples(0)
        noise = [gen.randn(*SHAPE, device=DEV)]
        noise += [gen.randn_like(noise[0]) for _ in range(S - 1)] + [None]
        assert torch.equal(edm_dpm_sample(diff, net, SHAPE, steps=S, order=2, algorithm=SDE, device=DEV, noise=noise,
                                          model_kwargs={"y": y}), whole)
        # the ODE solver draws x_T alone
        gen.set_done_samples(0)
        edm_dpm_sample(diff, net, SHAPE, steps=S, order=2, device=DEV, generator=gen, model_kwargs={"y": y})
        assert gen.draw == 1


# ------------------------------------------------------------------------------------------ 9. command line
def generate_large(tmp, *flags):
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "generate_large.py", "--synthetic", "imagenet64_T10", "--log_dir",
                        str(tmp), "--n_sample", "4", *flags], cwd=PKG, env=env, capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    arr = np.load(os.path.join(tmp, "samples_4.npz"))["arr_0"]
    assert arr.shape == (4, 64, 64, 3) and arr.dtype == np.uint8
    return r.stdout, arr


def test_cli_generate_large_dpmpp(tmp_path):
    out, arr = generate_large(tmp_path, "--karras_sampler", "dpmpp", "--karras_steps", "3", "--batchsize", "2")
    assert "3 NFE/image" in out and "dpmpp" in out


def test_cli_generate_large_sde_dpmpp_is_batch_invariant(tmp_path):
    runs = []
    for bs in ("2", "4"):
        tmp = tmp_path / f"bs{bs}"
        tmp.mkdir()
        out, arr = generate_large(tmp, "--karras_sampler", "sde-dpmpp", "--karras_steps", "3", "--generator", "determ", "--seed", "1",
                                  "--batchsize", bs)
        assert "3 NFE/image" in out
        runs.append(arr)
    assert np.array_equal(runs[0], runs[1]) and len({a.tobytes() for a in runs[0]}) > 1
