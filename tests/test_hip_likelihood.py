"""Probability-flow likelihood on the GPU: dxmi_pf_ll_stage against float64 on the same fp32 operands, input_vjp of both U-Nets
against the full backward (bit for bit, and with no parameter-gradient launch) and against float64 oracle nets, the whole loop on
the shrunken nets against an independent float64 statement of the formulas, batch independence, and eval_bpd.py end to end.

Bounds (u = 2^-24; the ones test_hip_dm_train.py states): an elementwise output within 16 u M of float64, M the sum of the
magnitudes of the operands that meet in it; a per-image sum within 64 u of the sum of its terms' magnitudes.  Network gradients:
cosine >= 0.995 and norm within 5 %.  The loop on the shrunken nets: NLL_BPD_ABS_BOUND_{EDM,DDPM}, twice the worst per-image
|bpd - bpd_oracle| measured on an MI355X (printed by the test)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffusion-by-maxentirl_amd")
SENTINEL = -12345.5
PAD = 64
# 768: one trip of the loop; 396 = 4 x 99: a partly filled trip; 105 and 111: CHW % 4 = 1 and 3 (the 4-byte aligned accesses and
# the scalar tail); 4800: three trips (a trip covers 256 lanes x 2 vectors x 4 elements = 2048)
SHAPES = [(3, 16, 16), (3, 12, 11), (3, 7, 5), (1, 37, 3), (3, 40, 40)]


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def tables(d, S):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.likelihood import edm_ll_schedule
    from models.DxMI.likelihood import ddpm_ll_schedule
    return {"edm": edm_ll_schedule(KarrasDenoiser(sigma_data=0.5), d, S).table, "ddpm": ddpm_ll_schedule(d, S, "logsnr").table}


def guarded(N, shape, fill=None):
    """A contiguous [N, *shape] device view with PAD sentinel floats before and after it -> (view, whole buffer)."""
    n = N * int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[PAD:PAD + n].view(N, *shape)
    if fill is not None:
        view.copy_(fill)
    return view, buf


def untouched(buf):
    return bool((buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all())


def operands(N, shape, seed, probe):
    gen = torch.Generator().manual_seed(seed)
    x, F1, g1, F2, g2, z = (torch.randn(N, *shape, generator=gen) for _ in range(6))
    e = z if probe == "gaussian" else torch.where(z >= 0, torch.ones_like(z), -torch.ones_like(z))
    return x, F1, g1, F2, g2, e


def isum(v):
    return v.reshape(v.shape[0], -1).sum(1)


def predict_ref(row, x, F, g, e):
    """PREDICT in float64 on fp32 operands -> {name: (value, magnitude)}."""
    K = lambda c: float(row[c])
    from dxmi_hip import ops as o
    x, F, g, e = (v.cpu().double() for v in (x, F, g, e))
    k1, Mk = K(o.PL_KA) * x + K(o.PL_KB) * F, (K(o.PL_KA) * x).abs() + (K(o.PL_KB) * F).abs()
    xt, Mx = x + K(o.PL_H) * k1, x.abs() + abs(K(o.PL_H)) * Mk
    ta, tb = K(o.PL_KA) * (e * e), K(o.PL_DB) * (e * g)
    return {"k1": (k1, Mk), "xt": (xt, Mx), "x_in": (K(o.PL_CIN_NEXT) * xt, abs(K(o.PL_CIN_NEXT)) * Mx),
            "div1": (isum(ta + tb), isum(ta.abs() + tb.abs()))}


def correct_ref(row, x, k1, F, g, e, div1, ell):
    from dxmi_hip import ops as o
    K = lambda c: float(row[c])
    x, k1, F, g, e, div1, ell = (v.cpu().double() for v in (x, k1, F, g, e, div1, ell))
    hk = K(o.PL_H) * k1
    xt, Mt = x + hk, x.abs() + hk.abs()
    k2, M2 = K(o.PL_KA2) * xt + K(o.PL_KB2) * F, abs(K(o.PL_KA2)) * Mt + (K(o.PL_KB2) * F).abs()
    xn, Mn = x + K(o.PL_HH) * (k1 + k2), x.abs() + abs(K(o.PL_HH)) * (k1.abs() + M2)
    ta, tb = K(o.PL_KA2) * (e * e), K(o.PL_DB2) * (e * g)
    div2, Md = isum(ta + tb), isum(ta.abs() + tb.abs())
    return {"x": (xn, Mn), "x_in": (K(o.PL_CIN_NEXT) * xn, abs(K(o.PL_CIN_NEXT)) * Mn),
            "ell": (ell + K(o.PL_HH) * (div1 + div2), ell.abs() + abs(K(o.PL_HH)) * (div1.abs() + Md))}


def worst(got, ref, M, k):
    return ((got.cpu().double() - ref).abs() / (k * U * M + 1e-30)).max().item()


def run_step(ops, tab, row, x, F1, g1, F2, g2, probe_kw, ctl=None, last_x_in=True, ell0=None):
    """FIRST is not run: PREDICT and CORRECT of `row` on guarded buffers -> dict of outputs and the buffers."""
    N, shape = x.shape[0], tuple(x.shape[1:])
    vec = lambda: torch.full((N + 2,), SENTINEL, dtype=torch.float32, device=DEV)
    xd, xb = guarded(N, shape, x)
    k1, k1b = guarded(N, shape)
    xt, xtb = guarded(N, shape)
    x_in, xib = guarded(N, shape)
    t, div1, ell, prior, logp, bpd = (vec() for _ in range(6))
    ell[1:N + 1] = torch.arange(N, dtype=torch.float32, device=DEV) * 3.25 - 2.0 if ell0 is None else ell0
    ell0 = ell[1:N + 1].clone()
    v = lambda a: a[1:N + 1]
    kw = dict(row=row) if ctl is None else dict(ctl=ctl)
    d = lambda a: a.to(DEV).contiguous()
    ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, v(t), x=xd, model_out=d(F1), vjp=d(g1), k1=k1, xt=xt, x_in=x_in, div1=v(div1), **kw, **probe_kw)
    pre = dict(k1=k1.clone(), xt=xt.clone(), x_in=x_in.clone(), div1=v(div1).clone(), t=v(t).clone(), x_kept=torch.equal(xd.cpu(), x))
    ops.pf_ll_stage(ops.PF_LL_CORRECT, tab, v(t), x=xd, model_out=d(F2), vjp=d(g2), k1=k1, x_in=x_in if last_x_in else None, div1=v(div1),
                    ell=v(ell), prior=v(prior), logp=v(logp), bpd=v(bpd), **kw, **probe_kw)
    torch.cuda.synchronize()
    post = dict(x=xd.clone(), x_in=x_in.clone(), ell=v(ell).clone(), prior=v(prior).clone(), logp=v(logp).clone(), bpd=v(bpd).clone(),
                t=v(t).clone(), ell0=ell0)
    clean = all(untouched(b) for b in (xb, k1b, xtb, xib)) and all(float(a[0]) == SENTINEL and float(a[-1]) == SENTINEL
                                                                   for a in (t, div1, ell, prior, logp, bpd))
    return pre, post, clean


# ------------------------------------------------------------------------------------------ the launch
@pytest.mark.parametrize("S", [2, 5])
@pytest.mark.parametrize("N", [1, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_stage_vs_fp64(ops, shape, N, S):
    d = int(np.prod(shape))
    figures = {}
    for family, tab in tables(d, S).items():
        tabd = tab.to(DEV)
        for row in sorted({0, S // 2, S - 1}):
            for probe in ("gaussian", "rademacher"):
                x, F1, g1, F2, g2, e = operands(N, shape, 11 + N + d + S + row, probe)
                pre, post, clean = run_step(ops, tabd, row, x, F1, g1, F2, g2, dict(eps=e.to(DEV)))
                assert clean and pre["x_kept"], (family, row, probe)
                K, last = tab[row], row == S - 1
                assert (pre["t"].cpu() == K[ops.PL_T_NEXT]).all() and (post["t"].cpu() == K[ops.PL_T_NEXT]).all()
                for name, (ref, M) in predict_ref(K, x, F1, g1, e).items():
                    w = worst(pre[name], ref, M, 64 if name == "div1" else 16)
                    figures[f"predict.{name}"] = max(figures.get(f"predict.{name}", 0.0), w)
                    assert w <= 1, (family, row, probe, name, w)
                cref = correct_ref(K, x, pre["k1"], F2, g2, e, pre["div1"], post["ell0"])
                if last:                 # nothing follows the last row: x_in keeps PREDICT's values
                    assert torch.equal(post["x_in"], pre["x_in"])
                    del cref["x_in"]
                for name, (ref, M) in cref.items():
                    w = worst(post[name], ref, M, 64 if name == "ell" else 16)
                    figures[f"correct.{name}"] = max(figures.get(f"correct.{name}", 0.0), w)
                    assert w <= 1, (family, row, probe, name, w)
                if not last:             # prior, logp and bpd are the last row's alone
                    assert all((post[k] == SENTINEL).all() for k in ("prior", "logp", "bpd"))
                    continue
                xn, ell = post["x"].cpu().double(), post["ell"].cpu().double()
                q = isum(xn * xn)
                pr, Mp = float(K[ops.PL_PRIOR_Q]) * q + float(K[ops.PL_PRIOR_C]), abs(float(K[ops.PL_PRIOR_Q])) * q + abs(float(K[ops.PL_PRIOR_C]))
                prior = post["prior"].cpu().double()
                logp = post["logp"].cpu().double()
                for name, w in (("prior", worst(post["prior"], pr, Mp, 64)), ("logp", worst(post["logp"], ell + prior, ell.abs() + prior.abs(), 16)),
                                ("bpd", worst(post["bpd"], logp * float(K[ops.PL_BPD_SCALE]) + 7, (logp * float(K[ops.PL_BPD_SCALE])).abs() + 7, 16))):
                    figures[f"last.{name}"] = max(figures.get(f"last.{name}", 0.0), w)
                    assert w <= 1, (family, row, probe, name, w)
    print(f"pf_ll_stage worst |err| / bound (shape {shape}, N {N}, S {S}): " + ", ".join(f"{k} {v:.3f}" for k, v in figures.items()))


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 7, 5), (1, 37, 3)])
def test_first_mode(ops, shape):
    N, d = 3, int(np.prod(shape))
    for family, tab in tables(d, 3).items():
        x = torch.randn(N, *shape, generator=torch.Generator().manual_seed(5))
        xd, xb = guarded(N, shape, x)
        x_in, xib = guarded(N, shape)
        t, ell = (torch.full((N + 2,), SENTINEL, device=DEV) for _ in range(2))
        ops.pf_ll_stage(ops.PF_LL_FIRST, tab.to(DEV), t[1:N + 1], row=0, x=xd, x_in=x_in, ell=ell[1:N + 1])
        K = tab[0]
        ref = x.double() * float(K[ops.PL_XSCALE])
        assert worst(xd, ref, ref.abs(), 16) <= 1 and worst(x_in, float(K[ops.PL_CIN]) * ref, (float(K[ops.PL_CIN]) * ref).abs(), 16) <= 1
        assert torch.equal(xd.cpu(), x * K[ops.PL_XSCALE]) and torch.equal(x_in.cpu(), K[ops.PL_CIN] * (x * K[ops.PL_XSCALE]))
        assert (t[1:N + 1].cpu() == K[ops.PL_T]).all() and (ell[1:N + 1].cpu() == K[ops.PL_LOGDET0]).all()
        assert untouched(xb) and untouched(xib) and all(float(a[0]) == SENTINEL == float(a[-1]) for a in (t, ell))
        if family == "ddpm":
            assert float(K[ops.PL_XSCALE]) > 1 and float(K[ops.PL_LOGDET0]) > 0


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 7, 5), (3, 40, 40)])
def test_fused_signs_are_the_given_signs(ops, shape):
    """The Rademacher signs made in the launch are the signs of randn_indexed's normals passed in: every output bit for bit, also
    for a global index above 2^32 and through the control block."""
    N, S, d = 4, 3, int(np.prod(shape))
    seed, draw = 0x1234_5678_9ABC, 5
    idx = torch.tensor([0, 7, (1 << 33) + 5, 123456], dtype=torch.int64, device=DEV)
    z = ops.randn_indexed(idx, shape, seed, draw)
    e = torch.where(z >= 0, torch.ones_like(z), -torch.ones_like(z))
    assert (e == 1).any() and (e == -1).any()
    tab = tables(d, S)["edm"].to(DEV)
    x, F1, g1, F2, g2, _ = operands(N, shape, 3, "rademacher")
    for row in (0, S - 1):
        given = run_step(ops, tab, row, x, F1, g1, F2, g2, dict(eps=e))
        fused = run_step(ops, tab, row, x, F1, g1, F2, g2, dict(sample_index=idx, seed=seed, draw=draw))
        ctl = torch.tensor([row, draw, seed & 0xFFFFFFFF, seed >> 32], dtype=torch.int32, device=DEV)
        block = run_step(ops, tab, (row + 1) % S, x, F1, g1, F2, g2, dict(sample_index=idx, seed=1, draw=9), ctl=ctl)
        other = run_step(ops, tab, row, x, F1, g1, F2, g2, dict(sample_index=idx, seed=seed, draw=draw + 1))
        for a, b in ((given, fused), (given, block)):
            assert a[2] and b[2]
            for part in (0, 1):
                for k in a[part]:
                    if torch.is_tensor(a[part][k]):
                        assert torch.equal(a[part][k], b[part][k]), (row, part, k)
        assert not torch.equal(other[0]["div1"], given[0]["div1"])       # another draw: other signs


def test_poisoned_row_gives_nan_and_touches_nothing_else(ops):
    N, S, shape = 3, 4, (3, 7, 5)
    tab = tables(105, S)["edm"].to(DEV)
    x, F1, g1, F2, g2, e = operands(N, shape, 9, "gaussian")
    for bad in (-1, S, 2 ** 31 - 1):
        ctl = torch.tensor([bad, 0, 0, 0], dtype=torch.int32, device=DEV)
        pre, post, clean = run_step(ops, tab, 0, x, F1, g1, F2, g2, dict(eps=e.to(DEV)), ctl=ctl)
        assert clean and pre["x_kept"]
        for part in (pre, post):
            for k, v in part.items():
                if torch.is_tensor(v) and k != "ell0":
                    assert torch.isnan(v).all(), (bad, k)
    xd, _ = guarded(N, shape, x)
    x_in, _ = guarded(N, shape)
    t, ell = (torch.zeros(N, device=DEV) for _ in range(2))
    ops.pf_ll_stage(ops.PF_LL_FIRST, tab, t, ctl=torch.tensor([S, 0, 0, 0], dtype=torch.int32, device=DEV), x=xd, x_in=x_in, ell=ell)
    assert all(torch.isnan(v).all() for v in (xd, x_in, t, ell))


@pytest.mark.parametrize("shape", [(3, 16, 16), (1, 37, 3), (3, 40, 40)])
def test_batch_independent_and_reproducible(ops, shape):
    """Seven images in one launch equal the same images in launches of three and four, and two runs are equal, bit for bit."""
    N, S, d = 7, 3, int(np.prod(shape))
    for family, tab in tables(d, S).items():
        tabd = tab.to(DEV)
        x, F1, g1, F2, g2, e = operands(N, shape, 21, "gaussian")
        whole = run_step(ops, tabd, S - 1, x, F1, g1, F2, g2, dict(eps=e.to(DEV)))
        again = run_step(ops, tabd, S - 1, x, F1, g1, F2, g2, dict(eps=e.to(DEV)))
        parts = [run_step(ops, tabd, S - 1, x[s], F1[s], g1[s], F2[s], g2[s], dict(eps=e[s].to(DEV)), ell0=whole[1]["ell0"][s])
                 for s in (slice(0, 3), slice(3, 7))]
        for part in (0, 1):
            for k, v in whole[part].items():
                if torch.is_tensor(v):
                    assert torch.equal(v, again[part][k]), (family, k)
                    assert torch.equal(v, torch.cat([parts[0][part][k], parts[1][part][k]])), (family, k)
        assert torch.isfinite(whole[1]["bpd"]).all()


def test_last_row_without_x_in_and_malformed_calls(ops):
    from dxmi_hip import DxmiError
    N, S, shape = 2, 3, (3, 16, 16)
    tab = tables(768, S)["edm"].to(DEV)
    x, F1, g1, F2, g2, e = operands(N, shape, 2, "gaussian")
    a = run_step(ops, tab, S - 1, x, F1, g1, F2, g2, dict(eps=e.to(DEV)))
    b = run_step(ops, tab, S - 1, x, F1, g1, F2, g2, dict(eps=e.to(DEV)), last_x_in=False)
    assert torch.equal(a[1]["bpd"], b[1]["bpd"]) and torch.equal(a[1]["x"], b[1]["x"])
    xd, ed = x.to(DEV), e.to(DEV)
    buf = lambda: torch.empty_like(xd)
    vec = lambda: torch.empty(N, device=DEV)
    t, div1, ell, prior, logp, bpd = (vec() for _ in range(6))
    idx = torch.arange(N, device=DEV)
    pred = dict(x=xd, model_out=buf(), vjp=buf(), k1=buf(), x_in=buf(), div1=div1)
    corr = dict(pred, ell=ell, prior=prior, logp=logp, bpd=bpd)
    bad = [lambda: ops.pf_ll_stage(3, tab, t, **pred, eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, **pred),                                   # no probe
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, **pred, eps=ed, sample_index=idx),          # two probes
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, row=S, **pred, eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, row=-1, **pred, eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab[:, :16].contiguous(), t, **pred, eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, **dict(pred, k1=None), eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, **dict(pred, x_in=None), eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, **dict(pred, k1=xd), eps=ed),              # k1 is x
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t, **dict(pred, vjp=buf()[:1]), eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_PREDICT, tab, t[:1], **pred, eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_CORRECT, tab, t, **dict(corr, bpd=None), eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_CORRECT, tab, t, row=0, **dict(corr, x_in=None), eps=ed),
           lambda: ops.pf_ll_stage(ops.PF_LL_CORRECT, tab, t, **corr, sample_index=idx.int()),
           lambda: ops.pf_ll_stage(ops.PF_LL_FIRST, tab, t, x=xd, x_in=buf()),                            # no ell
           lambda: ops.pf_ll_stage(ops.PF_LL_FIRST, tab, t, x=xd, ell=ell),
           lambda: ops.pf_ll_stage(ops.PF_LL_FIRST, tab.cpu(), t, x=xd, x_in=buf(), ell=ell)]
    for i, call in enumerate(bad):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"call {i} was accepted")
    lib = ops.load()
    p = lambda v: None if v is None else v.data_ptr()
    raw = lambda **o: lib.dxmi_pf_ll_stage(*[dict(dict(mode=1, tab=p(tab), rows=S, ctl=None, row=0, draw=0, seed=0, x=p(xd), F=p(pred["model_out"]),
                                                    g=p(pred["vjp"]), eps=p(ed), idx=None, k1=p(pred["k1"]), xt=None, x_in=p(pred["x_in"]), t=p(t),
                                                    div1=p(div1), ell=p(ell), prior=p(prior), logp=p(logp), bpd=p(bpd), N=N, CHW=768, stream=None),
                                               **o)[k] for k in ("mode", "tab", "rows", "ctl", "row", "draw", "seed", "x", "F", "g", "eps", "idx", "k1",
                                                                 "xt", "x_in", "t", "div1", "ell", "prior", "logp", "bpd", "N", "CHW", "stream")])
    for o, msg in ((dict(N=0), b"N (0)"), (dict(N=65536), b"N (65536)"), (dict(CHW=0), b"CHW (0)"), (dict(CHW=-4), b"CHW (-4)"),
                   (dict(rows=0), b"at least one row"), (dict(row=S), b"row (3)"), (dict(mode=7), b"unknown mode"),
                   (dict(tab=None), b"null pointer"), (dict(x=None), b"null pointer"), (dict(F=None), b"null pointer"),
                   (dict(eps=None), b"not neither"), (dict(idx=p(idx)), b"not both"), (dict(x=p(xd) + 4), b"16-byte aligned"),
                   (dict(t=p(t) + 2), b"4-byte aligned"), (dict(k1=p(xd)), b"none may be another"),
                   (dict(mode=2, bpd=None), b"null pointer")):
        assert raw(**o) != 0 and msg in lib.dxmi_last_error(), (o, lib.dxmi_last_error())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ input_vjp on the shrunken nets
PARAM_GRAD_OPS = ("conv2d_wgrad", "_conv2d_wgrad", "stem_conv_wgrad", "wgrad_branch", "wgrad_join", "colsum", "colsum_per_image",
                  "linear_bwd")
EDM_PLAIN = dict(class_cond=False, use_scale_shift_norm=False, resblock_updown=False)
DDPM_KW = dict(ch=64, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[8], dropout=0.1, in_channels=3, resolution=16)


def edm_net(plain, out_scale=1.0):
    from test_hip_cm_train import build
    return build(EDM_PLAIN if plain else None, "", out_scale)


def ddpm_net(out_scale=1.0):
    from models.DxMI.unet_small import Model
    from oracle.weights import formula_tensor
    net = Model(**DDPM_KW)
    sd = {k: formula_tensor(k, v.shape) for k, v in net.state_dict().items()}
    for k in ("conv_out.weight", "conv_out.bias"):
        sd[k] = sd[k] * out_scale
    net.load_state_dict(sd)
    return net.to(DEV).eval()


class _small64:
    """oracle.unet_small.forward in float64: its fp32-only timestep embedding is replaced, for the duration of the block, by the
    same expressions in float64."""

    def __enter__(self):
        from oracle import unet_small as us
        self.us, self.saved = us, us.timestep_embedding_sincos

        def te(t, dim):
            half = dim // 2
            freqs = torch.exp(torch.arange(half, dtype=torch.float64) * -(math.log(10000) / (half - 1)))
            arg = t.double()[:, None] * freqs[None, :]
            return torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
        us.timestep_embedding_sincos = te
        return us

    def __exit__(self, *a):
        self.us.timestep_embedding_sincos = self.saved


def edm_oracle(net, plain):
    """-> callable(x_in, t, y=None) in float64 on the net's weights (use inside `with _oracle64()`)."""
    from oracle import Precision, edm
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    kw = dict(num_classes=None, use_scale_shift_norm=False, resblock_updown=False) if plain else {}
    cfg = edm.EDMConfig(image_size=16, model_channels=64, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2), **kw)
    return lambda x_in, t, y=None: edm.unet_forward(sd, cfg, x_in, t, y=y, prec=Precision("fp32"))


def ddpm_oracle(net):
    from oracle import Precision
    from oracle import unet_small as us
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    cfg = us.UNetSmallConfig(ch=64, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(8,), resolution=16)
    return lambda x, t: us.forward(sd, cfg, x, t, Precision("fp32"))


def _cos(a, b):
    a, b = a.double().reshape(-1).cpu(), b.double().reshape(-1).cpu()
    return float(a @ b / (a.norm() * b.norm() + 1e-300))


def _vjp_operands():
    gen = torch.Generator().manual_seed(41)
    x, v = torch.randn(2, 3, 16, 16, generator=gen), torch.randn(2, 3, 16, 16, generator=gen)
    return x, v


def _counted(ops, monkeypatch):
    calls = {}
    for name in PARAM_GRAD_OPS:
        real = getattr(ops, name)

        def wrapped(*a, _real=real, _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


@pytest.mark.parametrize("plain", [False, True])
def test_edm_input_vjp(ops, monkeypatch, plain):
    from models.cm.unet_train import forward_with_grad, input_vjp
    from test_hip_dm_train import _oracle64
    net = edm_net(plain)
    x, v = _vjp_operands()
    t = torch.tensor([250 * math.log(0.7), 250 * math.log(9.0)], dtype=torch.float32)
    y = None if plain else torch.tensor([3, 871])
    yd = None if y is None else y.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out = forward_with_grad(net, xg, t.to(DEV), yd)
    out.backward(v.to(DEV))
    calls = _counted(ops, monkeypatch)
    F, g = input_vjp(net, x.to(DEV), t.to(DEV), v.to(DEV), yd)
    torch.cuda.synchronize()
    assert calls == {}, calls                                   # no parameter-gradient launch
    assert torch.equal(F, out.detach()) and torch.equal(g, xg.grad)
    assert not net.training and g.shape == x.shape and g.dtype == torch.float32
    monkeypatch.undo()
    calls = _counted(ops, monkeypatch)                          # the counters do see the full backward's launches
    forward_with_grad(net, x.to(DEV).requires_grad_(True), t.to(DEV), yd).backward(v.to(DEV))
    assert calls.get("conv2d_wgrad", 0) > 0 and calls.get("stem_conv_wgrad", 0) == 1 and calls.get("linear_bwd", 0) > 0
    with _oracle64():
        x64 = x.double().requires_grad_(True)
        F64 = edm_oracle(net, plain)(x64, t.double(), y)
        (g64,) = torch.autograd.grad((F64 * v.double()).sum(), x64)
    c, nr = _cos(g, g64), (g.double().cpu().norm() / g64.norm()).item()
    print(f"edm input_vjp ({'plain' if plain else 'class-conditional'}): cosine {c:.5f}, norm ratio {nr:.4f}, "
          f"output rel-L2 {((F.cpu().double() - F64).norm() / F64.norm()).item():.3e}")
    assert c >= 0.995 and abs(nr - 1) <= 0.05


def test_ddpm_input_vjp(ops, monkeypatch):
    from models.DxMI.unet_small_train import forward_with_grad, input_vjp
    net = ddpm_net()
    x, v = _vjp_operands()
    t = torch.tensor([37.0, 640.0])
    xg = x.to(DEV).requires_grad_(True)
    out = forward_with_grad(net, xg, t.to(DEV))
    out.backward(v.to(DEV))
    calls = _counted(ops, monkeypatch)
    net.train()                                                  # dropout 0.1: input_vjp runs in eval and puts train back
    F, g = input_vjp(net, x.to(DEV), t.to(DEV), v.to(DEV))
    torch.cuda.synchronize()
    assert net.training and calls == {}, calls
    net.eval()
    assert torch.equal(F, out.detach()) and torch.equal(g, xg.grad)
    monkeypatch.undo()
    calls = _counted(ops, monkeypatch)
    forward_with_grad(net, x.to(DEV).requires_grad_(True), t.to(DEV)).backward(v.to(DEV))
    assert calls.get("conv2d_wgrad", 0) > 0 and calls.get("stem_conv_wgrad", 0) == 1 and calls.get("linear_bwd", 0) > 0
    with _small64():
        x64 = x.double().requires_grad_(True)
        F64 = ddpm_oracle(net)(x64, t.double())
        (g64,) = torch.autograd.grad((F64 * v.double()).sum(), x64)
    c, nr = _cos(g, g64), (g.double().cpu().norm() / g64.norm()).item()
    print(f"ddpm input_vjp: cosine {c:.5f}, norm ratio {nr:.4f}, output rel-L2 {((F.cpu().double() - F64).norm() / F64.norm()).item():.3e}")
    assert c >= 0.995 and abs(nr - 1) <= 0.05


# ------------------------------------------------------------------------------------------ the whole loop on the shrunken nets
N_LOOP, STEPS_LOOP = 4, 3
# The inputs at which the trace term matters, established on the CPU oracle first, as GEN_SCALE / FAKE_SCALE of
# test_hip_dm_train.py were: the output layers' scales and, for the EDM net, the ladder's lower end.  On the full ladder 0.002 .. 80
# the three Heun steps put the network term of the divergence where c_in is near 1 and its own 1 % error (bf16 nets) is as large
# as what leaving c_in out changes (measured: the twin moved bpd by 1.0 - 1.7 x the error at every output scale from 2 to 128);
# from sigma = 1 up, c_in = 0.89 .. 0.0125 and every twin moves every image's bpd by at least 19.9 x the measured error.  DDPM net:
# at scale 0.25 the worst image of every twin moves by at least 54 x the measured error (the least moved image by 3.1 x: one of
# the four images has a small trace term under this probe).
EDM_OUT_SCALE, DDPM_OUT_SCALE = 8.0, 0.25
EDM_SIGMA_MIN, EDM_SIGMA_MAX = 1.0, 80.0
LOOP_Y = (3, 871, 40, 999)
NLL_BPD_ABS_MEASURED_EDM = 6.854e-4       # worst per-image |bpd - bpd_oracle| measured on an MI355X
NLL_BPD_ABS_MEASURED_DDPM = 3.165e-2
NLL_BPD_ABS_BOUND_EDM = 2 * NLL_BPD_ABS_MEASURED_EDM
NLL_BPD_ABS_BOUND_DDPM = 2 * NLL_BPD_ABS_MEASURED_DDPM


def cpu_state_dict(family, out_scale):
    """The formula weights of the shrunken net of `family`, float64 on the CPU (what edm_net / ddpm_net load)."""
    from oracle.weights import formula_tensor
    if family == "edm":
        from models.cm.script_util import create_model_and_diffusion
        from test_hip_cm_train import TINY_KW
        shapes, last = create_model_and_diffusion(**TINY_KW)[0].state_dict(), ("out.2.weight", "out.2.bias")
    else:
        from models.DxMI.unet_small import Model
        shapes, last = Model(**DDPM_KW).state_dict(), ("conv_out.weight", "conv_out.bias")
    sd = {k: formula_tensor(k, v.shape) for k, v in shapes.items()}
    for k in last:
        sd[k] = sd[k] * out_scale
    return {k: v.double() for k, v in sd.items()}


def loop_operands():
    gen = torch.Generator().manual_seed(77)
    x0 = torch.rand(N_LOOP, 3, 16, 16, generator=gen) * 2 - 1
    e, e_other = (torch.where(torch.randn(N_LOOP, 3, 16, 16, generator=gen) >= 0, 1.0, -1.0) for _ in range(2))
    return x0, e, e_other


def family_setup(family):
    """-> (nodes sigma [S + 1] float64, scalings(i) -> (c_skip, c_out, c_in), time(i), xscale, logdet0, prior_var), stated from the
    issue's formulas in float64; of the code under test it takes the node positions alone."""
    d = 768
    if family == "edm":
        from models.cm.karras_diffusion import KarrasDenoiser
        from models.cm.likelihood import edm_ll_schedule
        s, sd = edm_ll_schedule(KarrasDenoiser(sigma_data=0.5), d, STEPS_LOOP, 7.0, EDM_SIGMA_MIN, EDM_SIGMA_MAX).sigmas, 0.5
        scal = lambda i: (sd ** 2 / (s[i] ** 2 + sd ** 2), s[i] * sd / math.sqrt(s[i] ** 2 + sd ** 2), 1 / math.sqrt(s[i] ** 2 + sd ** 2))
        return s, scal, (lambda i: 250 * math.log(s[i])), 1.0, 0.0, s[-1] ** 2
    from models.DxMI.likelihood import ddpm_ll_schedule
    from models.DxMI.var_sampler import calc_diffusion_hyperparams
    tau = ddpm_ll_schedule(d, STEPS_LOOP, "logsnr").tau
    ab = calc_diffusion_hyperparams(1000, 1e-4, 0.02)["Alpha_bar"].to(torch.float32).double()[tau].tolist()
    s = [math.sqrt((1 - a) / a) for a in ab]
    scal = lambda i: (1.0, -s[i], 1 / math.sqrt(1 + s[i] ** 2))
    return s, scal, (lambda i: float(tau[i])), 1 / math.sqrt(ab[0]), -0.5 * d * math.log(ab[0]), 1 / ab[-1]


def oracle_loop(family, net64, x0, e, variant=None):
    """Heun on (x, l) in float64, written from the issue's formulas -> dict of per-image float64 results.  variant: None, or one of
    the wrong computations the test must tell from the right one: "no_div", "no_cin", "prior1"."""
    s, scal, time, xscale, logdet0, prior_var = family_setup(family)
    x, e = x0.double() * xscale, e.double()
    N, d = x.shape[0], x[0].numel()
    ell = torch.full((N,), logdet0, dtype=torch.float64)

    def drift(x, i):
        c_skip, c_out, c_in = scal(i)
        xi = (c_in * x).detach().requires_grad_(True)
        F = net64(xi, torch.full((N,), time(i), dtype=torch.float64))
        (g,) = torch.autograd.grad((F * e).sum(), xi)
        F = F.detach()
        k = ((1 - c_skip) * x - c_out * F) / s[i]
        div = isum((1 - c_skip) * e * e - c_out * (1.0 if variant == "no_cin" else c_in) * e * g) / s[i]
        return k, (torch.zeros_like(div) if variant == "no_div" else div)
    for i in range(len(s) - 1):
        h = s[i + 1] - s[i]
        k1, d1 = drift(x, i)
        k2, d2 = drift(x + h * k1, i + 1)
        x, ell = x + 0.5 * h * (k1 + k2), ell + 0.5 * h * (d1 + d2)
    pv = 1.0 if variant == "prior1" else prior_var
    prior = -isum(x * x) / (2 * pv) - 0.5 * d * math.log(2 * math.pi * pv)
    return {"delta_logp": ell, "prior_logp": prior, "bpd": -(ell + prior) / (d * math.log(2)) + 7}


def oracle_net(family, out_scale, y):
    sd = cpu_state_dict(family, out_scale)
    if family == "edm":
        from oracle import Precision, edm
        cfg = edm.EDMConfig(image_size=16, model_channels=64, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2))
        return lambda x_in, t: edm.unet_forward(sd, cfg, x_in, t, y=y, prec=Precision("fp32"))
    from oracle import Precision
    from oracle import unet_small as us
    cfg = us.UNetSmallConfig(ch=64, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(8,), resolution=16)
    return lambda x, t: us.forward(sd, cfg, x, t, Precision("fp32"))


def oracle_runs(family):
    """The oracle's result and its four wrong twins, on the CPU -> (result, {variant: per-image bpd shift})."""
    from test_hip_dm_train import _oracle64
    x0, e, e_other = loop_operands()
    scale = EDM_OUT_SCALE if family == "edm" else DDPM_OUT_SCALE
    with _oracle64(), _small64():
        net = oracle_net(family, scale, torch.tensor(LOOP_Y))
        ref = oracle_loop(family, net, x0, e)
        shifts = {v: (oracle_loop(family, net, x0, e, v)["bpd"] - ref["bpd"]).abs() for v in ("no_div", "no_cin", "prior1")}
        shifts["other_probe"] = (oracle_loop(family, net, x0, e_other)["bpd"] - ref["bpd"]).abs()
    return ref, shifts


@pytest.mark.parametrize("family", ["edm", "ddpm"])
def test_loop_vs_fp64_oracle(ops, family):
    """N = 4, steps = 3, the same x_0 and the same given probe on both sides.  The oracle's own worst per-image bpd moves by at least
    5 x the bound when (a) the divergence term is dropped, (b) c_in is left out of it, (c) another probe is drawn, (d) prior_var is
    replaced by 1: asserted on the CPU every run.  Measured on an MI355X: EDM worst |bpd - bpd_oracle| 6.854e-4 (delta_logp at most
    0.33 nats of 7.2e3, prior_logp 0.04), DDPM 3.165e-2 (delta_logp at most 16.8 nats, prior_logp 0.07); the device loop and the
    torch expressions on the same HIP net differ by at most 1.9e-6 bits/dim (0.03 of it), and are held to the launch bound
    (see below)."""
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.likelihood import edm_log_likelihood
    from models.DxMI.likelihood import ddpm_log_likelihood
    measured = NLL_BPD_ABS_MEASURED_EDM if family == "edm" else NLL_BPD_ABS_MEASURED_DDPM
    bound = NLL_BPD_ABS_BOUND_EDM if family == "edm" else NLL_BPD_ABS_BOUND_DDPM
    ref, shifts = oracle_runs(family)
    print(f"{family}: oracle bpd {ref['bpd'].tolist()}; |bpd shift| of the wrong twins, worst / least moved image: "
          + ", ".join(f"{k} {v.max().item():.4e} / {v.min().item():.4e}" for k, v in shifts.items()))
    x0, e, _ = loop_operands()
    y = torch.tensor(LOOP_Y, device=DEV)
    if family == "edm":
        net, d = edm_net(False, EDM_OUT_SCALE), KarrasDenoiser(sigma_data=0.5)
        run = lambda **kw: edm_log_likelihood(d, net, x0.to(DEV), steps=STEPS_LOOP, sigma_min=EDM_SIGMA_MIN, sigma_max=EDM_SIGMA_MAX,
                                              eps=e.to(DEV), model_kwargs={"y": y}, **kw)
    else:
        net = ddpm_net(DDPM_OUT_SCALE)
        run = lambda **kw: ddpm_log_likelihood(net, x0.to(DEV), steps=STEPS_LOOP, skip_type="logsnr", eps=e.to(DEV), **kw)
    got, fb = run(), run(_launches=False)
    torch.cuda.synchronize()
    assert got["nfe"] == 2 * STEPS_LOOP and all(got[k].shape == (N_LOOP,) for k in ("logp", "bpd", "prior_logp", "delta_logp"))
    assert torch.equal(got["logp"], got["delta_logp"] + got["prior_logp"])
    err = {k: (got[k].cpu().double() - ref[k]).abs().max().item() for k in ("bpd", "delta_logp", "prior_logp")}
    # The device loop against the torch expressions on the same HIP net.  Every elementwise operation of a stage is one rounding in
    # both, so the states, the network inputs and hence F and g are the same bits; what differs is the order of the per-image sums.
    # The launch bound of a sum is 64 u x the sum of its terms' magnitudes; over the 2 S launches those magnitudes add up to at
    # least |delta_logp|, and the last row adds the prior's.  Taking |delta_logp| + |prior_logp| for them is the tighter reading.
    # logp and bpd are elementwise: 16 u of their operands.
    scale = 1.0 / (768 * math.log(2))
    gd, gp, gl = (got[k].cpu().double().abs() for k in ("delta_logp", "prior_logp", "logp"))
    launch_bound = 64 * U * (gd + gp) * scale + 16 * U * (gl * scale + 7)
    dfb_all = (got["bpd"].cpu().double() - fb["bpd"].cpu().double()).abs()
    dfb = dfb_all.max().item()
    print(f"{family}: worst per-image |bpd - bpd_oracle| {err['bpd']:.4e} (measured {measured}, bound {bound}); delta_logp "
          f"{err['delta_logp']:.4e} of {ref['delta_logp'].abs().max().item():.4e}, prior_logp {err['prior_logp']:.4e} of "
          f"{ref['prior_logp'].abs().max().item():.4e}; device loop against the torch expressions on the same net: |bpd| {dfb:.4e}, "
          f"{(dfb_all / launch_bound).max().item():.3f} of the launch bound {launch_bound.min().item():.3e}")
    # The statistic the test bounds is the worst per-image |bpd - bpd_oracle|, so a wrong twin is told from the right computation
    # when it moves that statistic: each twin must move the worst image by at least 5 x the bound.  On the EDM net every single
    # image moves that far too.  On the DDPM net it does not: under this probe image 1 has a small trace term (its delta_logp is
    # 65 nats where the others' are 330 - 920), so dropping the divergence or redrawing the probe moves it by only 1.9 x and 1.5 x
    # the bound, while the worst image moves by 27.2 x (no divergence), 226.9 x (no c_in), 4306 x (prior_var = 1) and 30.3 x (probe).
    assert all(v.max().item() >= 5 * bound for v in shifts.values()), (shifts, bound)
    if family == "edm":
        assert all(v.min().item() >= 5 * bound for v in shifts.values()), (shifts, bound)
    assert err["bpd"] <= bound
    # delta_logp and prior_logp are bpd's two parts: each within the bound in bpd's unit
    unit = 768 * math.log(2)
    assert err["delta_logp"] <= bound * unit and err["prior_logp"] <= bound * unit
    assert (dfb_all <= launch_bound).all(), (dfb_all.tolist(), launch_bound.tolist())


# ------------------------------------------------------------------------------------------ batch and rank independence
# The input-only backward proved batch-invariant on an MI355X: six images as one batch, as two batches of three, and a 12-image
# array at --batchsize 5 and 12 gave bpd with a worst difference of 0.0 on both nets, so bpd is asserted bitwise.
@pytest.mark.parametrize("family", ["edm", "ddpm"])
def test_batch_and_rank_independence(ops, family):
    """determ: six images as one batch against two batches of three, and against two ranks of three: the probe e and the
    dequantisation noise xi of image i are the same bits, and so is every launch output whose inputs are."""
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.likelihood import dequantize_u8, edm_log_likelihood, make_probe
    from models.cm.random_util import DeterministicGenerator
    from models.DxMI.likelihood import ddpm_log_likelihood
    u8 = torch.randint(0, 256, (6, 3, 16, 16), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(DEV)
    y = torch.tensor([3, 871, 40, 999, 5, 17], device=DEV)
    if family == "edm":
        net, d = edm_net(False, EDM_OUT_SCALE), KarrasDenoiser(sigma_data=0.5)
        ll = lambda x0, rows, g: edm_log_likelihood(d, net, x0, steps=2, model_kwargs={"y": y[rows]}, generator=g)
    else:
        net = ddpm_net(DDPM_OUT_SCALE)
        ll = lambda x0, rows, g: ddpm_log_likelihood(net, x0, steps=2, skip_type="logsnr", generator=g)

    def batch(rows, done, rank=0, world=1):
        g = DeterministicGenerator(6, seed=11, rank=rank, world_size=world)
        g.set_done_samples(done)
        x0 = dequantize_u8(u8[rows], "uniform", g)
        draw = g.draw
        r = ll(x0, rows, g)
        g.draw = draw
        e, fused = make_probe("rademacher", x0.shape, x0.device, g)
        assert fused is not None
        return x0, e, r
    whole = batch(list(range(6)), 0)
    halves = [batch([0, 1, 2], 0), batch([3, 4, 5], 3)]
    ranks = [batch([0, 2, 4], 0, 0, 2), batch([1, 3, 5], 0, 1, 2)]
    order = [0, 2, 4, 1, 3, 5]
    for name, parts, rows in (("batches", halves, list(range(6))), ("ranks", ranks, order)):
        x0, e = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        assert torch.equal(x0, whole[0][rows]) and torch.equal(e, whole[1][rows]), name
        bpd = torch.cat([p[2]["bpd"] for p in parts])
        diff = (bpd - whole[2]["bpd"][rows]).abs().max().item()
        print(f"{family}: six images as one batch against two {name} of three: worst |bpd difference| {diff:.3e}")
        assert torch.equal(bpd, whole[2]["bpd"][rows]), name
    lo, hi = u8.float() / 128 - 1, (u8.float() + 1) / 128 - 1
    assert (whole[0] >= lo).all() and (whole[0] < hi).all() and torch.isfinite(whole[2]["bpd"]).all()


# ------------------------------------------------------------------------------------------ eval_bpd.py end to end
def _run_cli(args):
    return subprocess.run([sys.executable, os.path.join(PKG, "eval_bpd.py")] + args, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT])))


@pytest.mark.parametrize("family", ["edm", "ddpm"])
def test_eval_bpd_end_to_end(ops, family, tmp_path):
    """A saved shrunken checkpoint and a 12-image uint8 array, --steps 2 --batchsize 5: bpd_12.npz holds the Python entry point's
    values in global-index order, and --batchsize 12 gives the same file, bit for bit."""
    import dxmi_config
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.likelihood import dequantize_u8, edm_log_likelihood
    from models.cm.random_util import DeterministicGenerator
    from models.DxMI.likelihood import ddpm_log_likelihood
    n = 12
    arr = torch.randint(0, 256, (n, 16, 16, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(8)).numpy()
    labels = (np.arange(n, dtype=np.int64) * 83) % 1000
    data, ckpt, cfg_path = (os.path.join(tmp_path, f) for f in ("test.npz", "net.pt", "config.yaml"))
    np.savez(data, arr, labels)
    if family == "edm":
        from test_hip_cm_train import TINY_KW
        net = edm_net(False, EDM_OUT_SCALE)
        dxmi_config.save(dxmi_config.Cfg({"diffusion": dict(TINY_KW, sigma_min=0.002, sigma_max=80.0, distillation=False)}), cfg_path)
        flag, extra = "--pretrained", []
    else:
        net = ddpm_net(DDPM_OUT_SCALE)
        dxmi_config.save(dxmi_config.Cfg({"sampler_net": dict(DDPM_KW, ch_mult=[1, 2], _target_="models.DxMI.unet_small.Model")}), cfg_path)
        flag, extra = "--teacher_ckpt", ["--skip_type", "logsnr"]
    torch.save({k: v.cpu() for k, v in net.state_dict().items()}, ckpt)
    outs = {}
    for bs in (5, 12):
        out_dir = os.path.join(tmp_path, f"bs{bs}")
        r = _run_cli(["--data_npz", data, flag, ckpt, "--config", cfg_path, "--steps", "2", "--batchsize", str(bs), "--seed", "4",
                      "--out_dir", out_dir] + extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert f"over {n} images (1 repeat), NFE 4" in r.stdout and "bits/dim: " in r.stdout, r.stdout
        outs[bs] = np.load(os.path.join(out_dir, f"bpd_{n}.npz"))["arr_0"]
        assert outs[bs].shape == (n,) and outs[bs].dtype == np.float32 and np.isfinite(outs[bs]).all()
    # the Python entry point on the batches --batchsize 5 makes: images 0-4, 5-9, 10-11
    want = []
    u8 = torch.from_numpy(arr).permute(0, 3, 1, 2).contiguous().to(DEV)
    for done, rows in ((0, range(0, 5)), (5, range(5, 10)), (10, range(10, 12))):
        g = DeterministicGenerator(n, 4, rank=0, world_size=1)
        g.set_done_samples(done)
        x0 = dequantize_u8(u8[list(rows)], "uniform", g)
        if family == "edm":
            y = torch.from_numpy(labels[list(rows)]).to(DEV)
            want.append(edm_log_likelihood(KarrasDenoiser(sigma_data=0.5), net, x0, steps=2, model_kwargs={"y": y}, generator=g)["bpd"])
        else:
            want.append(ddpm_log_likelihood(net, x0, steps=2, skip_type="logsnr", generator=g)["bpd"])
    want = torch.cat(want).cpu().numpy()
    assert np.array_equal(outs[5], want)
    diff = float(np.abs(outs[5] - outs[12]).max())
    print(f"{family}: eval_bpd --batchsize 5 against --batchsize 12: worst |bpd difference| {diff:.3e}")
    assert np.array_equal(outs[5], outs[12])
