"""UniPC on the device, the DDPM teacher's launch: dxmi_unipc_stage against float64 on the same fp32 operands, slots and a corrected
state that a row does not name filled with NaN, the device control block and its poisoning, xc = NULL against dxmi_dpm_stage, the
loop against a float64 loop with an analytic network, and replay against eager and batch invariance on the shrunken HIP Model.
The checks are written once for both families (a Family below says what differs) and tests/test_hip_edm_unipc_sample.py runs them
on dxmi_edm_unipc_stage.

Bounds (u = 2^-24), counted from the kernel's operations on the fp32 table values K widened to float64, per element, with |D0|
taken as the sum of its two products' magnitudes P = |p1| + |p2|:
  D0      8 u P   (pred_xstart and the written slot), as the DPM-Solver++ launches' tests count it
  xc'     8 u Mb, Mb = |ccx xc| + |cv0| P + |cv1 D1| + |cv2 D2| + |cv3 D3| on a corrected row; an uncorrected row copies x: exact
  x'      12 u M, M = |cx| Mb + |w0| P + |w1 D1| + |w2 D2| (Mb = |x| on an uncorrected row).  12 is the depth of the longest
          rounding chain of an element: D0 (two products and their sum: 2), the corrector (its product and the five running sums:
          5), cx b (1), the predictor's three sums (3), 11 roundings of half an ulp each, rounded up
  x_in    is not bounded but exact: fp32(c_in_next) x' of the device's own x', one product
  loop    the launch's bounds propagated row by row through the float64 loop, as the DPM-Solver++ loops' tests do: with d(v) a
          bound on |device v - float64 v|,
            d(D0)  = |a| d(x) + |b| d(eps) + 8 u P          (the EDM nets: c_skip, c_out, F)
            d(b)   = |ccx| d(xc) + |cv0| d(D0) + sum_j |cv_j| d(D_j) + 8 u Mb        (d(x) on an uncorrected row)
            d(x')  = |cx| d(b) + |w0| d(D0) + |w1| d(D1) + |w2| d(D2) + 12 u M
          and d(eps) from the analytic network 0.8 tanh(0.9 x_in + 1e-3 t) (slope <= 0.72, five roundings)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
STEPS = 10
MID = 5
SHAPES = [(3, 75), (2, 192), (5, 3072), (1, 5000), (1, 263347)]
SENTINEL = 123.0
ROWS = (0, 1, 2, 3, MID, STEPS - 1)


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


class Teacher:
    """What differs between the two launches: the table's columns by name, the schedule, the call and the two products of D0."""
    name, prefix, x_in = "teacher", "UT_", False

    def __init__(self, ops):
        self.ops = ops
        self.c = {n[len(self.prefix):]: getattr(ops, n) for n in dir(ops) if n.startswith(self.prefix)}

    def schedule(self, steps=STEPS, order=3, variant="bh1", corrector=True, clip=True):
        from models.DxMI.unipc_sample import unipc_sample_schedule
        return unipc_sample_schedule(steps, order, variant, corrector, clip_denoised=clip)

    def stage(self, tab, t, first=False, f=None, x_in=None, **kw):
        self.ops.unipc_stage(self.ops.UNIPC_FIRST if first else self.ops.UNIPC_STEP, tab, t, eps=f, **kw)

    def products(self, K, x, f):
        return K[self.c["A"]] * x, -K[self.c["B"]] * f

    def make(self, K, x0, e):
        """The state and the network output whose data prediction is x0."""
        a, b = float(K[self.c["A"]]), float(K[self.c["B"]])
        return (x0 / a + (b / a) * e).float(), e.float()

    def parent(self, steps, order):
        from models.DxMI.dpm_sample import dpm_sample_schedule
        sch = dpm_sample_schedule(steps, order, solver_type="midpoint")
        return sch, lambda tab, t, f=None, x_in=None, **kw: self.ops.dpm_stage(self.ops.DPM_STEP, tab, t, eps=f, **kw)


_OPERANDS = {}


def operands(fam, K, N, CHW, seed):
    """x, f, xc, D1, D2, D3 (CPU fp32, computed once per key) with about half of the data prediction outside [-1, 1]: x0 uniform in
    [-2, 2]; the corrected state a little off the predicted one; D1..D3 uniform in [-1, 1]."""
    key = (fam.name, tuple(K.tolist()), N, CHW, seed)
    if key not in _OPERANDS:
        gen = torch.Generator().manual_seed(seed)
        x0 = torch.rand(N, CHW, generator=gen) * 4 - 2
        e = torch.randn(N, CHW, generator=gen)
        x, f = fam.make(K, x0, e)
        xc = (x + 0.05 * torch.randn(N, CHW, generator=gen) * x.abs().mean()).float()
        d = [torch.rand(N, CHW, generator=gen) * 2 - 1 for _ in range(3)]
        _OPERANDS[key] = (x, f, xc, *d)
    return _OPERANDS[key]


def history(k, d, fill=SENTINEL):
    """[4, N, CHW] with D_{k-1}, D_{k-2}, D_{k-3} where row k looks for them and `fill` in the slot it writes."""
    h = torch.full((4,) + tuple(d[0].shape), fill)
    for j in range(3):
        h[(k - 1 - j) % 4] = d[j]
    return h


def oracle(fam, row, x, f, xc, d):
    """float64 on the fp32 operands -> (x', D0, xc', bound of x', bound of D0, bound of xc').  xc None: the row runs uncorrected."""
    c = fam.c
    K = row.double().numpy()
    x, f = x.double().numpy(), f.double().numpy()
    d = [v.double().numpy() for v in d]
    p1, p2 = fam.products(K, x, f)
    d0, P = p1 + p2, np.abs(p1) + np.abs(p2)
    if int(K[c["FLAGS"]]) & c["FLAG_CLIP"]:
        d0 = np.clip(d0, -1, 1)
    if xc is not None and int(K[c["FLAGS"]]) & c["FLAG_CORR"]:
        xc = xc.double().numpy()
        cv = [K[c[n]] for n in ("CV0", "CV1", "CV2", "CV3")]
        b = K[c["CCX"]] * xc + cv[0] * d0 + cv[1] * d[0] + cv[2] * d[1] + cv[3] * d[2]
        Mb = np.abs(K[c["CCX"]] * xc) + abs(cv[0]) * P + np.abs(cv[1] * d[0]) + np.abs(cv[2] * d[1]) + np.abs(cv[3] * d[2])
        bbound = 8 * U * Mb
    else:
        b, Mb, bbound = x, np.abs(x), np.zeros_like(x)
    cx, w0, w1, w2 = (K[c[n]] for n in ("CX", "W0", "W1", "W2"))
    xn = cx * b + w0 * d0 + w1 * d[0] + w2 * d[1]
    M = abs(cx) * Mb + abs(w0) * P + np.abs(w1 * d[0]) + np.abs(w2 * d[1])
    return xn, d0, b, 12 * U * M, 8 * U * P, bbound


def launch(fam, tab, row, x, f, hist, xc=None, pred=True, stage=None, **kw):
    """One launch on copies -> (x', t_out, out, pred_xstart, hist, xc', x_in); out is pre-filled with 7, x_in with SENTINEL.  The row
    goes by value unless kw holds ctl."""
    xd, t = x.to(DEV).clone(), torch.full((x.shape[0],), -5.0, device=DEV)
    out = torch.full_like(xd, 7.0)
    p = torch.empty_like(xd) if pred else None
    hd = hist.to(DEV).clone()
    extra = {}
    if stage is None:
        extra["xc"] = xcd = None if xc is None else xc.to(DEV).clone()
    else:
        xcd = None
    if fam.x_in:
        extra["x_in"] = torch.full_like(xd, SENTINEL)
    if "ctl" not in kw:
        kw["row"] = row
    (stage or fam.stage)(tab, t, x=xd, f=f.to(DEV), hist=hd, out=out, pred_xstart=p, **extra, **kw)
    torch.cuda.synchronize()
    return xd, t, out, p, hd, xcd, extra.get("x_in")


def control(row):
    return torch.from_numpy(np.array([row & 0xFFFFFFFF, 0, 0, 0], dtype=np.uint32).view(np.int32)).to(DEV)


def same(a, b):
    return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------ 1. the launch against float64
def check_stage_vs_fp64(fam, N, CHW, clip, corrector):
    c = fam.c
    sch = fam.schedule(clip=clip, corrector=corrector)
    tab = sch.device_table(DEV)
    assert sch.table[:4, c["ORDER"]].tolist() == [1, 2, 3, 3] and sch.table[-1, c["ORDER"]] == 1
    assert sch.table[:4, c["CORDER"]].tolist() == ([0, 1, 2, 3] if corrector else [0] * 4) and sch.table[MID, c["CORDER"]] == 3 * corrector
    worst = {"x": 0.0, "xc": 0.0, "pred": 0.0}
    for row in ROWS:
        K = sch.table[row]
        x, f, xc, *d = operands(fam, K, N, CHW, 100 * row + CHW)
        xc = xc if corrector else None
        got, t_out, out, pred, hist, xcn, x_in = launch(fam, tab, row, x, f, history(row, d), xc)
        want, want_d0, want_b, bound, pbound, bbound = oracle(fam, K, x, f, xc, d)
        clipped = (np.abs(want_d0) >= 1).mean() if clip else (np.abs(want_d0) > 1).mean()
        assert 0.3 < clipped < 0.7, clipped
        err = np.abs(got.cpu().double().numpy() - want)
        perr = np.abs(pred.cpu().double().numpy() - want_d0)
        ratio = {"x": (err / bound).max(), "pred": (perr / pbound).max(), "xc": 0.0}
        assert (err <= bound).all() and (perr <= pbound).all()
        corrected = corrector and 1 <= row < STEPS - 1
        if corrector:
            berr = np.abs(xcn.cpu().double().numpy() - want_b)
            if corrected:
                ratio["xc"] = (berr / bbound).max()
                assert (berr <= bbound).all() and (bbound > 0).all()
            else:
                assert torch.equal(xcn.cpu(), x)          # rows 0 and S - 1: b = x, copied
        else:
            assert xcn is None
        print(f"{fam.name} ({N}, {CHW}) clip {clip} corrector {corrector} row {row}: worst |err| / bound x' {ratio['x']:.3e}, xc' "
              f"{ratio['xc']:.3e}, pred_xstart {ratio['pred']:.3e}")
        worst = {k: max(v, ratio[k]) for k, v in worst.items()}
        # negative controls, on the CPU: a neighbouring row's coefficients, and the corrector left out, must not pass
        other = oracle(fam, sch.table[row + 1 if row < STEPS - 1 else row - 1], x, f, xc, d)[0]
        assert (np.abs(other - want) > bound).any()
        if corrected:
            assert (np.abs(oracle(fam, K, x, f, None, d)[0] - want) > bound).any()
        # the written slot is D0 to the bit, the three others are as they were
        assert torch.equal(hist[row % 4], pred)
        assert all(torch.equal(hist[(row - 1 - j) % 4].cpu(), d[j]) for j in range(3))
        last = row == STEPS - 1
        assert torch.equal(t_out.cpu(), torch.full((N,), float(K[c["T_NEXT"]])))
        assert torch.equal(out, got.clamp(-1, 1) if last else torch.full_like(out, 7.0))
        if fam.x_in:          # the next evaluation's input: one fp32 product of the device's own x'; untouched on the last row
            assert torch.equal(x_in, torch.full_like(x_in, SENTINEL) if last else sch.table[row, c["CIN_NEXT"]].to(DEV) * got)
        if last:
            assert torch.equal(got, pred)             # cx = 0, w0 = 1: x' = 0 x + 1 D0
        # pred_xstart is optional and changes nothing else
        bare = launch(fam, tab, row, x, f, history(row, d), xc, pred=False)
        assert bare[3] is None and same((got, t_out, out, hist, xcn, x_in), (bare[0], bare[1], bare[2], bare[4], bare[5], bare[6]))
    print(f"{fam.name} ({N}, {CHW}) clip {clip} corrector {corrector}: worst ratios to the bounds over the rows: x' {worst['x']:.3e}, "
          f"xc' {worst['xc']:.3e}, pred_xstart {worst['pred']:.3e}")


@pytest.mark.parametrize("corrector", [True, False])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("N,CHW", SHAPES)
def test_stage_vs_fp64(ops, N, CHW, clip, corrector):
    check_stage_vs_fp64(Teacher(ops), N, CHW, clip, corrector)


# ------------------------------------------------------------------------------------------ 2. what a row does not name is not read
def check_unread_slots_and_state(fam, N, CHW, through_ctl):
    """S = 10, order 3: predictor orders 1 2 3 3 3 3 3 3 2 1, corrector orders 0 1 2 3 3 3 3 3 3 0.  Over rows 0-8 every slot and
    the corrected state that the row's weights do not name, and the slot it writes, hold NaN in one launch and 0 in the other: the
    bits agree, and slot row % 4 alone is written."""
    c = fam.c
    sch = fam.schedule()
    tab = sch.device_table(DEV)
    for row in range(STEPS - 1):
        p, q = int(sch.table[row, c["ORDER"]]), int(sch.table[row, c["CORDER"]])
        x, f, xc, *d = operands(fam, sch.table[row], N, CHW, 7 + row)
        runs = []
        for fill in (float("nan"), 0.0):
            h = history(row, d, fill)
            for j in range(3):
                if j >= max(p - 1, q):
                    h[(row - 1 - j) % 4] = fill
            state = xc if q else torch.full_like(xc, fill)
            kw = dict(ctl=control(row)) if through_ctl else {}
            runs.append((launch(fam, tab, row, x, f, h, state, **kw), h))
        (a, ha), (b, hb) = runs
        for k in (0, 1, 2, 3, 5, 6):          # x', t_out, out, pred_xstart, xc', x_in
            assert (a[k] is None and b[k] is None) or (torch.equal(a[k], b[k]) and torch.isfinite(a[k]).all()), (row, k)
        assert torch.equal(a[4][row % 4], b[4][row % 4]) and torch.isfinite(a[4][row % 4]).all()
        for s in range(4):                    # slot row % 4 alone is written
            if s != row % 4:
                assert torch.equal(b[4][s].cpu(), hb[s]) and torch.equal(torch.isnan(a[4][s]).cpu(), torch.isnan(ha[s]))
        if row == 0:
            assert torch.isnan(ha).all()
    # and the control: a corrected row of full order does read every slot and the corrected state
    row = MID
    x, f, xc, *d = operands(fam, sch.table[row], N, CHW, 7 + row)
    for j in range(3):
        h = history(row, d)
        h[(row - 1 - j) % 4] = float("nan")
        assert torch.isnan(launch(fam, tab, row, x, f, h, xc)[0]).all()
    assert torch.isnan(launch(fam, tab, row, x, f, history(row, d), torch.full_like(xc, float("nan")))[0]).all()


@pytest.mark.parametrize("through_ctl", [False, True])
@pytest.mark.parametrize("N,CHW", [(3, 75), (5, 3072)])
def test_unread_slots_and_state_are_not_read(ops, N, CHW, through_ctl):
    check_unread_slots_and_state(Teacher(ops), N, CHW, through_ctl)


# ------------------------------------------------------------------------------------------ 3. the control block
def check_control_block(fam):
    sch = fam.schedule()
    tab = sch.device_table(DEV)
    N, CHW = 5, 3072
    for row in ROWS:
        x, f, xc, *d = operands(fam, sch.table[row], N, CHW, 60 + row)
        h = history(row, d)
        want = launch(fam, tab, row, x, f, h, xc)
        assert same(want, launch(fam, tab, row, x, f, h, xc))                                   # bits repeat from run to run
        assert same(want, launch(fam, tab, (row + 3) % STEPS, x, f, h, xc, ctl=control(row)))   # the block's row is the row
    t_a, t_b = torch.zeros(3, device=DEV), torch.zeros(3, device=DEV)
    xa, xb = torch.randn(3, 192, device=DEV), None
    xb = xa.clone()
    extra_a = dict(x=xa, x_in=torch.empty_like(xa)) if fam.x_in else {}
    extra_b = dict(x=xb, x_in=torch.empty_like(xb)) if fam.x_in else {}
    fam.stage(tab, t_a, first=True, row=2, **extra_a)
    fam.stage(tab, t_b, first=True, row=0, ctl=control(2), **extra_b)
    assert torch.equal(t_a, t_b) and t_b.tolist() == [float(sch.table[2, fam.c["T"]])] * 3 and torch.equal(xa, xb)
    if fam.x_in:
        assert torch.equal(extra_a["x_in"], extra_b["x_in"])


def test_control_block_equals_by_value(ops):
    check_control_block(Teacher(ops))


def check_poisoned_row(fam):
    """The poisoning contract of the stage launches, not a fault: the table sits at the start of a larger buffer of NaN-free
    sentinels, so a read past its rows would bring 1e30 into the result instead of NaN.  A poisoned row gives NaN in x, xc, x_in,
    out, t_out and slot 0; it reads no slot and no xc, and the three slots that are not slot 0 are left as they were."""
    sch = fam.schedule()
    big = torch.full((STEPS + 4, fam.c["COLS"]), 1e30, device=DEV)
    big[:STEPS] = sch.table.to(DEV)
    tab = big[:STEPS]
    x, f, xc, *d = operands(fam, sch.table[MID], 3, 192, 41)
    for row in (STEPS, STEPS + 1, -1, 1 << 20, 0x7FFFFFFF):
        got, t, out, pred, hd, xcn, x_in = launch(fam, tab, 0, x, f, history(0, d), xc, ctl=control(row))
        assert torch.isnan(got).all() and torch.isnan(out).all() and torch.isnan(t).all() and torch.isnan(xcn).all()
        assert x_in is None or torch.isnan(x_in).all()
        assert torch.isnan(hd[0]).all() and all(torch.equal(hd[(0 - 1 - j) % 4].cpu(), d[j]) for j in range(3))
        t = torch.zeros(3, device=DEV)
        extra = dict(x=x.to(DEV).clone(), x_in=torch.zeros(3, 192, device=DEV)) if fam.x_in else {}
        fam.stage(tab, t, first=True, ctl=control(row), **extra)
        assert torch.isnan(t).all() and all(torch.isnan(v).all() for v in extra.values())
    assert (big[STEPS:] == 1e30).all()


def test_out_of_range_row_in_the_control_block(ops):
    check_poisoned_row(Teacher(ops))


def check_nan_stays_in_its_image(fam):
    sch = fam.schedule()
    tab = sch.device_table(DEV)
    for row in (MID, STEPS - 1):
        x, f, xc, *d = operands(fam, sch.table[row], 4, 771, 33)
        h = history(row, d)
        clean = launch(fam, tab, row, x, f, h, xc)
        bad = f.clone()
        bad[2] = float("nan")
        got = launch(fam, tab, row, x, bad, h, xc)
        last = row == STEPS - 1
        for k in ((0, 2, 3) if last else (0, 3, 5) + ((6,) if fam.x_in else ())):      # x', out / xc', pred_xstart, x_in
            assert torch.isnan(got[k][2]).all()             # the clamps do not swallow it
            for n in (0, 1, 3):
                assert torch.equal(got[k][n], clean[k][n]) and torch.isfinite(got[k][n]).all()
        assert torch.isnan(got[4][row % 4][2]).all() and torch.equal(got[4][row % 4][[0, 1, 3]], clean[4][row % 4][[0, 1, 3]])
        assert torch.equal(got[1], clean[1])


def test_nan_stays_in_its_image(ops):
    check_nan_stays_in_its_image(Teacher(ops))


# ------------------------------------------------------------------------------------------ 4. no corrected state: the parent's launch
def check_without_xc_is_the_parent(fam, N, CHW):
    """bh2, order 2 (the midpoint rule): without xc the launch runs every row uncorrected, whatever its flags, and gives the bits of
    dxmi_dpm_stage / dxmi_edm_dpm_stage on the equal rows; the parent's ring has three slots, ours four."""
    c = fam.c
    uni = fam.schedule(order=2, variant="bh2", corrector=True)
    par, par_stage = fam.parent(STEPS, 2)
    assert uni.table[1:-1, c["CORDER"]].tolist() == [1.0] + [2.0] * (STEPS - 3)          # flagged corrected, run uncorrected
    tu, tp = uni.device_table(DEV), par.device_table(DEV)
    for row in (0, 1, MID, STEPS - 1):
        x, f, xc, *d = operands(fam, uni.table[row], N, CHW, 90 + row)
        a = launch(fam, tu, row, x, f, history(row, d), None)
        h3 = torch.full((3,) + tuple(x.shape), SENTINEL)
        h3[(row - 1) % 3], h3[(row - 2) % 3] = d[0], d[1]
        b = launch(fam, tp, row, x, f, h3, stage=par_stage)
        for k in (0, 1, 2, 3, 6):
            assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), (row, k)
        assert torch.equal(a[4][row % 4], b[4][row % 3]) and a[5] is None


@pytest.mark.parametrize("N,CHW", [(3, 75), (5, 3072), (1, 263347)])
def test_without_xc_is_dpm_stage(ops, N, CHW):
    check_without_xc_is_the_parent(Teacher(ops), N, CHW)


def test_malformed_calls(ops):
    from dxmi_hip import DxmiError
    fam = Teacher(ops)
    sch = fam.schedule()
    tab = sch.device_table(DEV)
    x, f, xc, *d = (v.to(DEV) for v in operands(fam, sch.table[MID], 4, 768, 2))
    t, out, hist = torch.empty(4, device=DEV), torch.empty(4, 768, device=DEV), torch.zeros(4, 4, 768, device=DEV)
    step = lambda **kw: ops.unipc_stage(ops.UNIPC_STEP, **dict(dict(tab=tab, t_out=t, row=MID, x=x, xc=xc, eps=f, hist=hist, out=out), **kw))
    bad = [lambda: step(row=STEPS), lambda: step(row=-1), lambda: step(eps=f[:3]), lambda: step(eps=f.double()), lambda: step(x=x.cpu()),
           lambda: step(out=None), lambda: step(hist=None), lambda: step(hist=hist[:3]), lambda: step(hist=hist.double()),
           lambda: step(xc=x), lambda: step(xc=xc[:3]), lambda: step(xc=xc.double()), lambda: step(xc=xc.cpu()),
           lambda: step(tab=tab[:, :8]), lambda: step(t_out=t[:3]), lambda: step(ctl=torch.zeros(3, dtype=torch.int32, device=DEV))]
    for i, call in enumerate(bad):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"malformed call {i} was accepted")
    step()
    step(xc=None)
    ops.unipc_stage(ops.UNIPC_FIRST, tab, t, row=0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 5. the loop, analytic network
def analytic_net(x_in, t, y=None):
    """|dF / dx_in| <= 0.8 * 0.9 = 0.72."""
    return 0.8 * torch.tanh(0.9 * x_in + 1e-3 * t[:, None, None, None])


def loop64(fam, tab, x_T, drop_corrector=False):
    """The loop in float64 numpy on the fp32 table -> (the predicted state after every row, the propagated bound after every row).
    drop_corrector: the negative control, every row runs uncorrected (what a launch that ignored xc would give)."""
    c = fam.c
    K = tab.double().numpy()
    x = x_T.double().numpy()
    dx = np.zeros_like(x)
    if fam.x_in:
        x = x * K[0][c["XSCALE"]]
        dx = U * np.abs(x)                                                     # FIRST's one product
    xc, dxc = None, None
    hist, dhist = [], []
    states, bounds = [], []
    for k in range(len(K)):
        R = K[k]
        t = R[c["T"]]
        if fam.x_in:
            x_in = R[c["CIN"]] * x
            dx_in = R[c["CIN"]] * dx + U * np.abs(x_in)
        else:
            x_in, dx_in = x, dx
        f = 0.8 * np.tanh(0.9 * x_in + 1e-3 * t)
        df = 0.72 * dx_in + 8 * U * (0.8 * (np.abs(0.9 * x_in) + abs(1e-3 * t)) + np.abs(f))
        p1, p2 = fam.products(R, x, f)
        P = np.abs(p1) + np.abs(p2)
        g1, g2 = (abs(R[c["A"]]), abs(R[c["B"]])) if not fam.x_in else (abs(R[c["CSKIP"]]), abs(R[c["COUT"]]))
        d0, dd0 = p1 + p2, g1 * dx + g2 * df + 8 * U * P
        if int(R[c["FLAGS"]]) & c["FLAG_CLIP"]:
            d0 = np.clip(d0, -1, 1)
        if int(R[c["FLAGS"]]) & c["FLAG_CORR"] and not drop_corrector:
            cv = [R[c[n]] for n in ("CV0", "CV1", "CV2", "CV3")]
            b, Mb = R[c["CCX"]] * xc + cv[0] * d0, np.abs(R[c["CCX"]] * xc) + abs(cv[0]) * P
            db = abs(R[c["CCX"]]) * dxc + abs(cv[0]) * dd0
            for j in range(3):
                if cv[j + 1] != 0:
                    b, Mb, db = b + cv[j + 1] * hist[j], Mb + np.abs(cv[j + 1] * hist[j]), db + abs(cv[j + 1]) * dhist[j]
            db = db + 8 * U * Mb
        else:
            b, Mb, db = x, np.abs(x), dx
        acc, M = R[c["CX"]] * b + R[c["W0"]] * d0, abs(R[c["CX"]]) * Mb + abs(R[c["W0"]]) * P
        dacc = abs(R[c["CX"]]) * db + abs(R[c["W0"]]) * dd0
        for j, n in enumerate(("W1", "W2")):
            if R[c[n]] != 0:
                acc, M, dacc = acc + R[c[n]] * hist[j], M + np.abs(R[c[n]] * hist[j]), dacc + abs(R[c[n]]) * dhist[j]
        x, dx, xc, dxc = acc, dacc + 12 * U * M, b, db
        hist, dhist = [d0] + hist[:2], [dd0] + dhist[:2]
        states.append(x)
        bounds.append(dx)
    return np.stack(states), np.stack(bounds)


def check_loop(fam, sample, S, clip):
    shape = (5, 3, 32, 32)
    gen = torch.Generator().manual_seed(77 + S)
    noise = [torch.randn(shape, generator=gen)] + [None] * S
    sch = fam.schedule(steps=S, clip=clip)
    assert max(sch.table[:, fam.c["CORDER"]].tolist()) == 3          # a q = 3 corrector runs
    want, bound = loop64(fam, sch.table, noise[0])
    seen = []
    out = sample(analytic_net, shape, steps=S, clip_denoised=clip, device=DEV, noise=noise, callback=lambda d: seen.append(d))
    torch.cuda.synchronize()
    got = torch.stack([d["x"] for d in seen]).cpu().double().numpy()
    err = np.abs(got - want)
    print(f"{fam.name} S {S} clip {clip}: loop vs float64, worst |err| {err.max():.3e}, worst |err| / propagated bound "
          f"{(err / bound).max():.3e} (bound up to {bound.max():.3e})")
    assert (err <= bound).all()
    # negative control, on the CPU: the bound tells a loop without the corrector from one with it
    assert (np.abs(loop64(fam, sch.table, noise[0], drop_corrector=True)[0] - want) > bound).any()
    assert [d["i"] for d in seen] == list(range(S))
    assert torch.equal(out, seen[-1]["x"].clamp(-1, 1)) and out.abs().max() <= 1 and out.std() > 0.05
    assert torch.equal(seen[-1]["x"], seen[-1]["pred_xstart"])
    # the torch path on the CPU states the same expressions
    cpu = sample(analytic_net, shape, steps=S, clip_denoised=clip, device="cpu", noise=noise)
    assert ((cpu - out.cpu()).abs().double().numpy() <= 2 * bound[-1]).all()          # each within the bound of the float64 loop


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("S", [6, 8])
def test_loop_with_analytic_network(ops, S, clip):
    from models.DxMI.unipc_sample import unipc_sample
    check_loop(Teacher(ops), unipc_sample, S, clip)


# ------------------------------------------------------------------------------------------ 6. the loop on the HIP Model
SHAPE = (4, 3, 16, 16)


@pytest.fixture(scope="module")
def net(ops):
    """The shrunken Model of tests/test_hip_dpm_sample.py, in eval mode."""
    from models.DxMI.unet_small import Model
    from oracle.weights import formula_tensor
    from test_hip_dpm_sample import NET_KW
    m = Model(**NET_KW)
    m.load_state_dict({k: formula_tensor(k, v.shape) for k, v in m.state_dict().items()})
    return m.to(DEV).eval()


def test_replay_equals_eager(net):
    from models.DxMI.unipc_sample import replay_graphs, unipc_sample
    S = 6
    kw = dict(steps=S, device=DEV)
    torch.manual_seed(5)
    eager = unipc_sample(net, SHAPE, **kw).clone()
    assert replay_graphs(net) == []
    torch.manual_seed(5)
    replayed = unipc_sample(net, SHAPE, use_graph=True, **kw).clone()
    assert torch.isfinite(eager).all() and eager.abs().max() <= 1 and eager.std() > 0
    assert torch.equal(eager, replayed)
    graphs = replay_graphs(net)
    assert len(graphs) == 1 and graphs[0].captures == 1 and graphs[0].replays == S - 2
    torch.manual_seed(5)
    again = unipc_sample(net, SHAPE, use_graph=True, **kw)
    assert torch.equal(again, eager) and graphs[0].captures == 1 and graphs[0].replays == 2 * S - 2
    assert again.data_ptr() == unipc_sample(net, SHAPE, use_graph=True, **kw).data_ptr()          # the returned tensor is static
    # the corrector is in the result, and the predictor alone has a graph of its own (no xc buffer)
    torch.manual_seed(5)
    alone = unipc_sample(net, SHAPE, corrector=False, use_graph=True, **kw).clone()
    torch.manual_seed(5)
    assert not torch.equal(alone, eager) and torch.equal(alone, unipc_sample(net, SHAPE, corrector=False, **kw))
    assert len(replay_graphs(net)) == 2
    # replay is off with a callback
    torch.manual_seed(5)
    assert torch.equal(unipc_sample(net, SHAPE, use_graph=True, callback=lambda d: None, **kw), eager) and graphs[0].replays == 3 * S - 2


def test_batch_invariance(net):
    from models.cm.random_util import get_generator
    from models.DxMI.unipc_sample import unipc_sample
    gen = get_generator("determ", 4, seed=9)
    kw = dict(steps=5, device=DEV, generator=gen)
    gen.set_done_samples(0)
    whole = unipc_sample(net, (4, 3, 16, 16), **kw).clone()
    assert gen.draw == 1                      # the solver draws x_T alone
    parts = []
    for b in range(2):
        gen.set_done_samples(2 * b)
        parts.append(unipc_sample(net, (2, 3, 16, 16), use_graph=True, **kw).clone())
    parts = torch.cat(parts)
    for i in range(4):
        assert torch.equal(parts[i], whole[i]), i
    assert not torch.equal(whole[0], whole[1])
