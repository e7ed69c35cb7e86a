"""Karras samplers of the EDM teacher on the device (models.cm.karras_diffusion.karras_sample, dxmi_karras_stage).

Tolerances:
  * stage kernel vs float64 on the same fp32 operands: |got - ref| <= 16 u M per element, u = 2^-24 (fp32 unit roundoff) and M
    the sum of the magnitudes of the terms the output is built from (x, d dt, the noise terms; d itself bounded by
    (|x_e| + |denoised|) / sigma).  The kernel rounds once per reference torch op, so a handful of u M is its whole error;
  * analytic-model trajectories (tanh(0.7 x_in + 1e-3 t), restated in torch here, 2 x 3 x 8 x 8) vs the reference's fp32 run,
    replaying its recorded draws: rel-L2 <= 1e-5 for every step's x and denoised and for the sample;
  * shrunken U-Net trajectories (1 x 3 x 16 x 16): the few-step policy of test_hip_edm.py::test_sampling_T4_vs_reference, rel-L2
    <= 3e-2 per step (the network runs in bf16, the reference in fp32; the fixture keeps these per-step values in fp16, whose
    relative rounding of 2^-11 is far inside the bound);
  * graph replay vs eager: bit for bit.
"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24

CASES = {
    "heun6": dict(sampler="heun", steps=6),
    "heun6_churn": dict(sampler="heun", steps=6, s_churn=10.0, s_tmin=0.05, s_tmax=10.0, s_noise=1.007),
    "dpm4_churn": dict(sampler="dpm", steps=4, s_churn=2.0, s_noise=1.007),
    "euler8": dict(sampler="euler", steps=8),
    "ancestral8": dict(sampler="ancestral", steps=8),
}


class ReplayGenerator:
    """Hands out recorded draws in order (the reference's generator interface: randn / randn_like)."""

    def __init__(self, draws):
        self.draws, self.k = torch.from_numpy(np.asarray(draws)), 0

    def _next(self, shape, device):
        v = self.draws[self.k]
        assert tuple(v.shape) == tuple(shape), (self.k, tuple(v.shape), tuple(shape))
        self.k += 1
        return v.to(device)

    def randn(self, *shape, device=None):
        return self._next(shape, device)

    def randn_like(self, x):
        return self._next(x.shape, x.device)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "karras_sample.npz"))


def analytic(x_in, t, **kw):
    return torch.tanh(0.7 * x_in + 1e-3 * t[:, None, None, None])


def build(kw, over=None):
    from models.cm.script_util import create_model_and_diffusion
    from oracle.weights import formula_tensor
    kw = dict(kw)
    kw.update(over or {})
    net, diffusion = create_model_and_diffusion(**kw)
    net.load_state_dict({k: formula_tensor(k, v.shape) for k, v in net.state_dict().items()})
    return net.to(DEV).eval(), diffusion


def tiny_kw():
    from test_hip_edm import PLAIN, TINY_KW
    return TINY_KW, PLAIN


# ------------------------------------------------------------------------------------------------------------ stage kernel
def _row(g, mode, clip=1.0):
    from dxmi_hip import ops
    from models.cm.karras_diffusion import KarrasDenoiser
    tab = torch.zeros(3, ops.KT_COLS)
    sig = torch.tensor([0.3 + 4 * torch.rand(1, generator=g).item()])
    c_skip, c_out, _ = KarrasDenoiser().get_scalings(sig)
    nxt = torch.tensor([0.05 + torch.rand(1, generator=g).item()])
    r = tab[1]
    r[ops.KT_SIGMA], r[ops.KT_CSKIP], r[ops.KT_COUT] = sig[0], c_skip[0], c_out[0]
    r[ops.KT_DT] = -sig[0] * 0.6
    r[ops.KT_SIGMA_UP], r[ops.KT_CHURN], r[ops.KT_SNOISE] = 0.37, 0.81, 1.007
    r[ops.KT_CIN] = KarrasDenoiser().get_scalings(nxt)[2][0]
    r[ops.KT_T] = 250 * torch.log(nxt)[0]
    r[ops.KT_XSCALE] = 80.0 if mode == ops.KARRAS_FIRST else 1.0
    r[ops.KT_CLIP] = clip
    return tab


def _ref_stage(mode, last, r, x, x2, d, F, noise):
    """float64 restatement of the stage (include/dxmi_hip.h) and the magnitude M of each output's terms."""
    from dxmi_hip import ops
    s, cs, co, dt = (float(r[k]) for k in (ops.KT_SIGMA, ops.KT_CSKIP, ops.KT_COUT, ops.KT_DT))
    up, churn, sn, cin = (float(r[k]) for k in (ops.KT_SIGMA_UP, ops.KT_CHURN, ops.KT_SNOISE, ops.KT_CIN))
    x, x2, d, F = (v.double() for v in (x, x2, d, F))
    nz = None if noise is None else noise.double()
    res = {}
    if mode == ops.KARRAS_FIRST:
        xn = x * float(r[ops.KT_XSCALE])
        M = xn.abs()
    else:
        xe = x2 if mode in (ops.KARRAS_HEUN_CORR, ops.KARRAS_DPM_CORR) else x
        den = co * F + cs * xe
        Mden = (co * F).abs() + (cs * xe).abs()
        if float(r[ops.KT_CLIP]):
            den = den.clamp(-1, 1)
        dd = (xe - den) / s
        Md = (xe.abs() + Mden) / s
        res["denoised"] = (den, Mden)
        if mode == ops.KARRAS_PRED:
            xn, M = xe + dd * dt, xe.abs() + Md * abs(dt)
            res["d"], res["x2"] = (dd, Md), (xn, M)
        elif mode == ops.KARRAS_HEUN_CORR:
            xn, M = x + ((d + dd) / 2) * dt, x.abs() + (d.abs() + Md) * abs(dt)
        elif mode == ops.KARRAS_DPM_CORR:
            xn, M = x + dd * dt, x.abs() + Md * abs(dt)
        else:
            xn, M = xe + dd * dt, xe.abs() + Md * abs(dt)
            if mode == ops.KARRAS_ANCESTRAL and nz is not None:
                xn, M = xn + nz * up, M + (nz * up).abs()
    if mode == ops.KARRAS_PRED:
        res["x_in"] = (cin * xn, abs(cin) * M)
        return res
    if last:
        res["out"] = (xn.clamp(-1, 1), M)
        return res
    if nz is not None and mode != ops.KARRAS_ANCESTRAL:
        xn, M = xn + (nz * sn) * churn, M + (nz * sn * churn).abs()
    res["x"] = (xn, M)
    res["x_in"] = (cin * xn, abs(cin) * M)
    return res


STAGES = [  # (mode name, last, noise)
    ("FIRST", 0, False), ("FIRST", 0, True), ("PRED", 0, False), ("HEUN_CORR", 0, True), ("HEUN_CORR", 1, False),
    ("DPM_CORR", 0, False), ("DPM_CORR", 1, False), ("EULER", 0, False), ("EULER", 1, False), ("ANCESTRAL", 0, True),
    ("ANCESTRAL", 1, True), ("ANCESTRAL", 1, False),
]


@pytest.mark.parametrize("hw", [16, 64, 256])
@pytest.mark.parametrize("stage", STAGES, ids=lambda s: f"{s[0]}-last{s[1]}-noise{int(s[2])}")
def test_stage_kernel_vs_fp64(stage, hw):
    from dxmi_hip import ops
    name, last, with_noise = stage
    mode = getattr(ops, f"KARRAS_{name}")
    for N in (1, 7):
        for clip in (1.0, 0.0):
            g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{last}/{with_noise}/{hw}/{N}/{clip}".encode()))
            shape = (N, 3, hw, hw)
            tab = _row(g, mode, clip)
            # x around +-1.5, F so that c_out F + c_skip x lands on both sides of the +-1 clamp
            x, x2, d = (1.5 * torch.randn(shape, generator=g) for _ in range(3))
            F = 3.0 * torch.randn(shape, generator=g)
            noise = torch.randn(shape, generator=g) if with_noise else None
            dev = {k: (None if v is None else v.to(DEV).contiguous()) for k, v in dict(x=x, x2=x2, d=d, F=F, noise=noise).items()}
            outs = {k: torch.full(shape, float("nan"), device=DEV) for k in ("x_in", "out", "denoised")}
            t = torch.full((N,), float("nan"), device=DEV)
            ops.karras_stage(mode, last, tab.to(DEV), 1, dev["x"], x2=dev["x2"], d=dev["d"],
                             model_out=None if mode == ops.KARRAS_FIRST else dev["F"], noise=dev["noise"],
                             x_in=None if last else outs["x_in"], t=None if last else t, out=outs["out"] if last else None,
                             denoised=None if mode == ops.KARRAS_FIRST else outs["denoised"])
            got = {"x": dev["x"], "x2": dev["x2"], "d": dev["d"], **outs}
            ref = _ref_stage(mode, last, tab[1], x, x2, d, F, noise)
            for k, (want, M) in ref.items():
                err = (got[k].cpu().double() - want).abs()
                bound = 16 * U * M + 1e-30
                worst = (err / bound).max().item()
                assert torch.isfinite(got[k]).all() and worst <= 1.0, (name, last, hw, N, clip, k, worst)
            if not last:
                assert torch.equal(t.cpu(), tab[1, ops.KT_T].expand(N))
            if mode == ops.KARRAS_PRED or last:    # the state is left alone
                assert torch.equal(dev["x"].cpu(), x)


# ------------------------------------------------------------------------------------------------------------ trajectories
def _trajectory(gold, case, diffusion, model, kw, shape, draws):
    from models.cm.karras_diffusion import karras_sample
    p = dict(CASES[case])
    sampler, steps = p.pop("sampler"), p.pop("steps")
    cb = []
    gen = ReplayGenerator(gold[draws])
    out = karras_sample(diffusion, model, shape, steps, model_kwargs=kw, device=DEV, sampler=sampler, generator=gen,
                        callback=lambda d: cb.append(d), **p)
    assert gen.k == len(gen.draws), "the sampler consumed a different number of draws than the reference"
    assert len(cb) == steps
    return out, cb


@pytest.mark.parametrize("case", list(CASES))
def test_analytic_trajectory_vs_reference(gold, case):
    from models.cm.karras_diffusion import KarrasDenoiser
    out, cb = _trajectory(gold, case, KarrasDenoiser(sigma_data=0.5), analytic, {}, (2, 3, 8, 8), f"{case}.analytic.draws")
    worst = 0.0
    for i, d in enumerate(cb):
        for k in ("x", "denoised"):
            r = rel_l2(d[k].cpu(), gold[f"{case}.analytic.{k}"][i])
            worst = max(worst, r)
            assert r <= 1e-5, (case, i, k, r)
        assert float(d.get("sigma_hat", d["sigma"])) == float(gold[f"{case}.sigma_hat"][i])
    r = rel_l2(out.cpu(), gold[f"{case}.analytic.sample"])
    print(f"{case}: analytic worst per-step rel-L2 {worst:.2e}, sample {r:.2e}")
    assert r <= 1e-5


@pytest.mark.parametrize("variant", ["unet", "unet_plain"])
@pytest.mark.parametrize("case", list(CASES))
def test_unet_trajectory_vs_reference(gold, case, variant):
    tiny, plain = tiny_kw()
    net, diffusion = build(tiny, plain if variant == "unet_plain" else None)
    kw = {"y": torch.from_numpy(gold[f"{case}.y"]).to(DEV)} if variant == "unet" else {}
    with torch.no_grad():
        out, cb = _trajectory(gold, case, diffusion, net, kw, (1, 3, 16, 16), f"{case}.draws")
    rs = []
    for i, d in enumerate(cb):
        rx = rel_l2(d["x"].cpu(), gold[f"{case}.{variant}.x"][i])
        rd = rel_l2(d["denoised"].cpu(), gold[f"{case}.{variant}.denoised"][i])
        rs.append((rx, rd))
        assert rx <= 3e-2 and rd <= 3e-2, (case, variant, i, rx, rd)
    r = rel_l2(out.cpu(), gold[f"{case}.{variant}.sample"])
    print(f"{case}/{variant}: per-step rel-L2 (x, denoised) " + " ".join(f"({a:.1e},{b:.1e})" for a, b in rs) + f"; sample {r:.2e}")
    assert r <= 3e-2


# ------------------------------------------------------------------------------------------------------------ graph replay
@pytest.mark.parametrize("case", ["heun6_churn", "ancestral8"])
def test_graph_replay_matches_eager(case):
    from models.cm.karras_diffusion import _GRAPHS, karras_sample
    tiny, _ = tiny_kw()
    p = dict(CASES[case])
    sampler, steps = p.pop("sampler"), p.pop("steps")
    y = torch.tensor([3, 871], device=DEV)
    outs = {}
    for mode in ("eager", "graph"):
        net, diffusion = build(tiny)
        torch.cuda.manual_seed(1234)
        outs[mode] = [karras_sample(diffusion, net, (2, 3, 16, 16), steps, model_kwargs={"y": y}, device=DEV, sampler=sampler,
                                    use_graph=mode == "graph", **p).clone() for _ in range(4)]
        if mode == "graph":
            (g,) = _GRAPHS[net].values()
            assert g.replays == 2 and g.captures == 1
    for i in range(4):
        assert torch.equal(outs["eager"][i], outs["graph"][i]), i
    assert not torch.equal(outs["graph"][2], outs["graph"][3])


# ------------------------------------------------------------------------------------------------------------ full size
def test_imagenet64_full_size_heun3():
    from models.cm.karras_diffusion import _GRAPHS, karras_sample
    from test_hip_edm import IMAGENET64_KW
    net, diffusion = build(IMAGENET64_KW)
    assert sum(p.numel() for p in net.parameters()) == 295_899_267
    calls = []
    net.register_forward_pre_hook(lambda m, a: calls.append(1))
    y = torch.tensor([1, 250, 500, 999], device=DEV)
    outs, nfe = [], []
    for use_graph in (False, True, True, True):       # eager, then the graph key's eager warm-up, capture, replay
        torch.cuda.manual_seed(99)
        calls.clear()
        outs.append(karras_sample(diffusion, net, (4, 3, 64, 64), 3, model_kwargs={"y": y}, device=DEV, sampler="heun",
                                  s_churn=1.0, use_graph=use_graph).clone())
        nfe.append(len(calls))
    assert nfe == [5, 5, 5, 0]                       # heun: 2 steps - 1 U-Net calls; a replay runs no python
    assert _GRAPHS[net]
    out = outs[0]
    assert torch.isfinite(out).all() and out.abs().max().item() <= 1.0
    assert out.std().item() > 0
    for o in outs[1:]:
        assert torch.equal(o, out)


# ------------------------------------------------------------------------------------------------------------ CLI
def test_cli_generate_large_karras(tmp_path):
    pkg = os.path.join(ROOT, "diffusion-by-maxentirl_amd")
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "generate_large.py", "--synthetic", "imagenet64_T10",
                        "--log_dir", str(tmp_path), "--karras_sampler", "heun", "--karras_steps", "2", "--n_sample", "4",
                        "--batchsize", "2"], cwd=pkg, env=env, capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "3 NFE/image" in r.stdout
    arr = np.load(os.path.join(tmp_path, "samples_4.npz"))["arr_0"]
    assert arr.shape == (4, 64, 64, 3) and arr.dtype == np.uint8
