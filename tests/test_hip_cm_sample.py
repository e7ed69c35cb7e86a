"""Consistency-model sampling and zero-shot editing on the device (models.cm.karras_diffusion: karras_sample's onestep /
multistep branch, iterative_colorization / _inpainting / _superres; dxmi_cm_stage).

Tolerances (u = 2^-24, the fp32 unit roundoff):
  * stage kernel vs float64 on the same fp32 operands, per element:
      |got - ref| <= 16 u M_elem + 136 u M_Q
    M_elem: the magnitudes of the element-wise terms (c_out F, c_skip x, the mask blend, z NOISE, the output); M_Q (Q edits
    only): sum_e |Q[d][e]| sum_d' |Q[d'][e]| |v_d'|, v the denoised terms (or ref for coefficient 0).  The element-wise part
    rounds once per reference torch op; each Q transform is a chain of at most 64 fp32 products and sums, in an order the
    reference's einsum does not fix: 2 x 64 + 8 roundings cover both transforms and the denoised value they act on
    (DESIGN 5.11).  The worst |err| / bound of every case is printed;
  * analytic-model runs (tanh(0.7 x_in + 1e-3 t)) vs the reference's fp32 run with its recorded draws: rel-L2 <= 1e-5 for the
    element-wise cases, <= 1e-4 for the Q edits (a per-element 136 u = 8.1e-6 of sum|Q||v|, which exceeds |out|);
  * shrunken U-Nets (bf16 on the device, fp32 in the reference, fp16 in the fixture): rel-L2 <= 3e-2 per step, as the Karras
    U-Net test;
  * graph replay vs eager: bit for bit.
"""
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest
import torch

from test_hip_karras_sample import ReplayGenerator, analytic, build, rel_l2, tiny_kw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
CASES = {   # name: (kind, ts) with steps 40
    "onestep": ("onestep", None),
    "multistep_0_22_39": ("multistep", (0, 22, 39)),
    "multistep_0_10_20": ("multistep", (0, 10, 20)),
    "colorization": ("colorization", (0, 22, 39)),
    "superres": ("superres", (0, 22, 39)),
    "inpainting": ("inpainting", (0, 10, 20)),
}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "cm_sample.npz"))


def distilled():
    from models.cm.karras_diffusion import KarrasDenoiser
    return KarrasDenoiser(sigma_data=0.5, sigma_max=80.0, sigma_min=0.002, weight_schedule="uniform", distillation=True)


# ------------------------------------------------------------------------------------------------------------ stage kernel
def _table(g, mode, last, clip, out_clamp):
    from dxmi_hip import ops
    tab = torch.zeros(3, ops.CT_COLS)
    sig = torch.tensor([0.3 + 4 * torch.rand(1, generator=g).item()])
    c_skip, c_out, _ = distilled().get_scalings_for_boundary_condition(sig)
    nxt = torch.tensor([0.05 + torch.rand(1, generator=g).item()])
    r = tab[1]
    r[ops.CT_CSKIP], r[ops.CT_COUT], r[ops.CT_NOISE] = c_skip[0], c_out[0], 0.83
    r[ops.CT_CIN] = distilled().get_scalings(nxt)[2][0]
    r[ops.CT_T] = 250 * torch.log(nxt)[0]
    r[ops.CT_XSCALE] = 80.0 if mode == ops.CM_FIRST else 1.0
    r[ops.CT_CLIP], r[ops.CT_OUTCLAMP] = clip, out_clamp
    return tab


def _patches(v):
    N, C, H, W = v.shape
    return v.reshape(N, C, H // 8, 8, W // 8, 8).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 8, W // 8, 64)


def _unpatches(p, shape):
    N, C, H, W = shape
    return p.reshape(N, C, H // 8, W // 8, 8, 8).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H, W)


def _ref_stage(mode, edit, last, r, Q, x, F, noise, ref, mask):
    """float64 restatement of dxmi_cm_stage (include/dxmi_hip.h) -> {output: (value, M_elem, M_Q)}."""
    from dxmi_hip import ops
    cs, co, nz, cin = (float(r[k]) for k in (ops.CT_CSKIP, ops.CT_COUT, ops.CT_NOISE, ops.CT_CIN))
    x, F = x.double(), F.double()
    zero = torch.zeros_like(x)
    if mode == ops.CM_FIRST:
        xn = x * float(r[ops.CT_XSCALE])
        return {"x": (xn, xn.abs(), zero), "x_in": (cin * xn, abs(cin) * xn.abs(), zero)}
    den = co * F + cs * x
    Md = (co * F).abs() + (cs * x).abs()
    if float(r[ops.CT_CLIP]):
        den = den.clamp(-1, 1)
    res = {"denoised": (den, Md, zero)}
    x0, Me, Mq = den, Md, zero
    if edit == ops.CM_EDIT_MASK:
        m, rf = mask.double(), ref.double()
        x0 = rf * m + den * (1 - m)
        Me = (rf * m).abs() + (den * (1 - m)).abs() + Md
    elif edit == ops.CM_EDIT_COLOUR:
        Qd, Qa = Q.double(), Q.double().abs()
        rf = ref.double()
        y = torch.einsum("bchw,cd->bdhw", den, Qd)
        y[:, 0] = torch.einsum("bchw,c->bhw", rf, Qd[:, 0])
        x0 = torch.einsum("bdhw,cd->bchw", y, Qd)
        S = torch.einsum("bchw,cd->bdhw", Md, Qa)
        S[:, 0] = torch.einsum("bchw,c->bhw", rf.abs(), Qa[:, 0])
        Mq = torch.einsum("bdhw,cd->bchw", S, Qa)
        Me = x0.abs()
    elif edit == ops.CM_EDIT_PATCH:
        Qd, Qa = Q.double(), Q.double().abs()
        rf = ref.double()
        y = _patches(den) @ Qd
        y[..., 0] = _patches(rf) @ Qd[:, 0]
        x0 = _unpatches(y @ Qd.T, den.shape)
        S = _patches(Md) @ Qa
        S[..., 0] = _patches(rf.abs()) @ Qa[:, 0]
        Mq = _unpatches(S @ Qa.T, den.shape)
        Me = x0.abs()
    xn, Mx = x0, Me
    if noise is not None:
        xn = x0 + noise.double() * nz
        Mx = Me + (noise.double() * nz).abs()
    if last:
        out = xn.clamp(-1, 1) if float(r[ops.CT_OUTCLAMP]) else xn
        res["out"] = (out, Mx, Mq)
    else:
        res["x"] = (xn, Mx, Mq)
        res["x_in"] = (cin * xn, abs(cin) * Mx, abs(cin) * Mq)
    return res


STAGES = [  # (mode, edit, last, noise)
    ("FIRST", "NONE", 0, False),
    ("STEP", "NONE", 0, True), ("STEP", "NONE", 1, True), ("STEP", "NONE", 1, False),
    ("STEP", "MASK", 0, True), ("STEP", "MASK", 1, True),
    ("STEP", "COLOUR", 0, True), ("STEP", "COLOUR", 1, False),
    ("STEP", "PATCH", 0, True), ("STEP", "PATCH", 1, True), ("STEP", "PATCH", 1, False),
]


@pytest.mark.parametrize("hw", [16, 64, 256])
@pytest.mark.parametrize("stage", STAGES, ids=lambda s: f"{s[0]}-{s[1]}-last{s[2]}-noise{int(s[3])}")
def test_stage_kernel_vs_fp64(stage, hw):
    from dxmi_hip import ops
    from models.cm.karras_diffusion import colour_basis, patch_basis
    name, ename, last, with_noise = stage
    mode, edit = getattr(ops, f"CM_{name}"), getattr(ops, f"CM_EDIT_{ename}")
    Q = {ops.CM_EDIT_COLOUR: colour_basis(), ops.CM_EDIT_PATCH: patch_basis()}.get(edit)
    worst_all = 0.0
    for N in ((7, 14) if edit == ops.CM_EDIT_MASK else (1, 7)):
        for clip, out_clamp in ((1.0, 1.0), (0.0, 0.0)):
            g = torch.Generator().manual_seed(zlib.crc32(f"{stage}/{hw}/{N}/{clip}".encode()))
            shape = (N, 3, hw, hw)
            tab = _table(g, mode, last, clip, out_clamp)
            x = 1.5 * torch.randn(shape, generator=g)
            F = 3.0 * torch.randn(shape, generator=g)
            ref = torch.rand(shape, generator=g) * 2 - 1
            mask = (torch.rand(shape, generator=g) > 0.5).float()
            noise = torch.randn(shape, generator=g) if with_noise else None
            d = {k: (None if v is None else v.to(DEV).contiguous()) for k, v in dict(x=x, F=F, ref=ref, noise=noise).items()}
            outs = {k: torch.full(shape, float("nan"), device=DEV) for k in ("x_in", "out", "denoised")}
            t = torch.full((N,), float("nan"), device=DEV)
            first = mode == ops.CM_FIRST
            ops.cm_stage(mode, last, tab.to(DEV), 1, d["x"], edit=edit, Q=None if Q is None else Q.to(DEV),
                         model_out=None if first else d["F"], noise=d["noise"],
                         ref=d["ref"] if edit != ops.CM_EDIT_NONE else None,
                         mask=mask.to(DEV) if edit == ops.CM_EDIT_MASK else None,
                         x_in=None if last else outs["x_in"], t=None if last else t, out=outs["out"] if last else None,
                         denoised=None if first else outs["denoised"])
            got = {"x": d["x"], **outs}
            want = _ref_stage(mode, edit, last, tab[1], Q, x, F, noise, ref, mask)
            for k, (w, Me, Mq) in want.items():
                err = (got[k].cpu().double() - w).abs()
                bound = 16 * U * Me + 136 * U * Mq + 1e-30
                worst = (err / bound).max().item()
                worst_all = max(worst_all, worst)
                assert torch.isfinite(got[k]).all() and worst <= 1.0, (stage, hw, N, clip, k, worst)
            if not last:
                assert torch.equal(t.cpu(), tab[1, ops.CT_T].expand(N))
            else:
                assert torch.equal(d["x"].cpu(), x)       # the state is left alone
    print(f"{stage} {hw}x{hw}: worst |err|/bound {worst_all:.3f}")


# ------------------------------------------------------------------------------------------------------------ trajectories
def _run_case(gold, case, diffusion, model, kw, draws, images_in=None):
    """-> (output, degraded images or None, per-evaluation denoised list)."""
    import models.cm.karras_diffusion as kd
    kind, ts = CASES[case]
    gen = ReplayGenerator(draws)
    dens = []
    if kind in ("onestep", "multistep"):
        shape = tuple(draws.shape[1:])
        out = kd.karras_sample(diffusion, model, shape, 40, model_kwargs=kw, device=DEV, sampler=kind, ts=ts, generator=gen,
                               callback=lambda d: dens.append(d["denoised"].clone()))
        imgs = None
    else:
        # the editing loops take no callback: record denoised by wrapping the stage launch
        from dxmi_hip import ops
        orig = ops.cm_stage

        def rec(*a, **k):
            if k.get("model_out") is not None:
                k["denoised"] = torch.empty_like(k["model_out"])
                orig(*a, **k)
                dens.append(k["denoised"])
            else:
                orig(*a, **k)
        ops.cm_stage = rec
        try:
            x = gen.randn(*draws.shape[1:], device=DEV) * 80.0
            fn = {"colorization": kd.iterative_colorization, "superres": kd.iterative_superres,
                  "inpainting": kd.iterative_inpainting}[kind]
            extra = {}
            if kind == "inpainting":        # the fixture's 16x16 letter mask: the letter lies outside, so group 0 keeps all
                m = torch.zeros(x.shape, device=DEV)
                m[:7] = 1.0
                extra["mask"] = m
            out, imgs = fn(kd.KarrasDenoiserFn(diffusion, model, True, kw), torch.as_tensor(images_in).to(DEV).float(), x, ts, steps=40,
                           generator=gen, **extra)
        finally:
            ops.cm_stage = orig
    assert gen.k == len(gen.draws), "the sampler consumed a different number of draws than the reference"
    return out, imgs, dens


@pytest.mark.parametrize("case", list(CASES))
def test_analytic_vs_reference(gold, case):
    p = f"{case}.analytic"
    out, imgs, dens = _run_case(gold, case, distilled(), analytic, {}, gold[f"{p}.draws"],
                                gold[f"{p}.images_in"] if f"{p}.images_in" in gold.files else None)
    tol = 1e-4 if case in ("colorization", "superres") else 1e-5
    rs = [rel_l2(dv.cpu(), gold[f"{p}.denoised"][i]) for i, dv in enumerate(dens)]
    assert len(dens) == len(gold[f"{p}.denoised"])
    r = rel_l2(out.cpu(), gold[f"{p}.out"])
    ri = rel_l2(imgs.cpu(), gold[f"{p}.images"]) if imgs is not None else 0.0
    print(f"{case}: analytic per-step denoised rel-L2 {['%.1e' % v for v in rs]}, out {r:.2e}, images {ri:.2e}")
    assert max(rs) <= tol and r <= tol and ri <= tol


@pytest.mark.parametrize("variant", ["unet", "unet_plain"])
@pytest.mark.parametrize("case", list(CASES))
def test_unet_vs_reference(gold, case, variant):
    tiny, plain = tiny_kw()
    over = dict(plain if variant == "unet_plain" else {}, distillation=True)
    net, diffusion = build(tiny, over)
    assert diffusion.distillation
    kw = {"y": torch.from_numpy(gold[f"{case}.y"]).to(DEV)} if variant == "unet" else {}
    with torch.no_grad():
        out, imgs, dens = _run_case(gold, case, diffusion, net, kw, gold[f"{case}.draws"],
                                    gold[f"{case}.images_in"] if f"{case}.images_in" in gold.files else None)
    rs = [rel_l2(dv.cpu(), gold[f"{case}.{variant}.denoised"][i]) for i, dv in enumerate(dens)]
    r = rel_l2(out.cpu(), gold[f"{case}.{variant}.out"])
    print(f"{case}/{variant}: per-step denoised rel-L2 {['%.1e' % v for v in rs]}; out {r:.2e}")
    assert len(rs) == len(gold[f"{case}.{variant}.denoised"]) and max(rs) <= 3e-2 and r <= 3e-2


# ------------------------------------------------------------------------------------------------------------ graph replay
@pytest.mark.parametrize("sampler,ts", [("onestep", None), ("multistep", (0, 10, 20))])
def test_graph_replay_matches_eager(sampler, ts):
    from models.cm.karras_diffusion import _GRAPHS, karras_sample
    tiny, _ = tiny_kw()
    y = torch.tensor([3, 871], device=DEV)
    outs = {}
    for mode in ("eager", "graph"):
        net, diffusion = build(tiny, {"distillation": True})
        torch.cuda.manual_seed(1234)
        outs[mode] = [karras_sample(diffusion, net, (2, 3, 16, 16), 40, model_kwargs={"y": y}, device=DEV, sampler=sampler,
                                    ts=ts, use_graph=mode == "graph").clone() for _ in range(4)]
        if mode == "graph":
            (g,) = _GRAPHS[net].values()
            assert g.replays == 2 and g.captures == 1
    for i in range(4):
        assert torch.equal(outs["eager"][i], outs["graph"][i]), i
    assert not torch.equal(outs["graph"][2], outs["graph"][3])


# ------------------------------------------------------------------------------------------------------------ full size
def test_imagenet64_full_size_multistep2():
    from models.cm.karras_diffusion import karras_sample
    from test_hip_edm import IMAGENET64_KW
    net, diffusion = build(IMAGENET64_KW, {"distillation": True})
    calls = []
    net.register_forward_pre_hook(lambda m, a: calls.append(1))
    y = torch.tensor([1, 999], device=DEV)
    torch.cuda.manual_seed(7)
    karras_sample(diffusion, net, (2, 3, 64, 64), 40, model_kwargs={"y": y}, device=DEV, sampler="multistep", ts=(0, 22, 39))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = karras_sample(diffusion, net, (2, 3, 64, 64), 40, model_kwargs={"y": y}, device=DEV, sampler="multistep",
                        ts=(0, 22, 39))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"ImageNet-64 full size, multistep-2, B=2: {dt * 1e3:.1f} ms")
    assert len(calls) == 4
    assert torch.isfinite(out).all() and out.abs().max().item() <= 1.0 and out.std().item() > 0


# ------------------------------------------------------------------------------------------------------------ CLI
def test_cli_generate_large_cm(tmp_path):
    pkg = os.path.join(ROOT, "diffusion-by-maxentirl_amd")
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "generate_large.py", "--synthetic", "imagenet64_T10",
                        "--log_dir", str(tmp_path), "--cm_sampler", "multistep", "--ts", "0,22,39", "--n_sample", "4",
                        "--batchsize", "2"], cwd=pkg, env=env, capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "2 NFE/image" in r.stdout
    arr = np.load(os.path.join(tmp_path, "samples_4.npz"))["arr_0"]
    assert arr.shape == (4, 64, 64, 3) and arr.dtype == np.uint8
