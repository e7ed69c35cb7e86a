"""CPU: the host side of the consistency-model samplers and editing loops (models.cm.karras_diffusion: CMSchedule,
karras_sample's onestep / multistep branch, sample_onestep, stochastic_iterative_sampler, iterative_*).

Checked against the reference's own run (tests/golden/cm_sample.npz, written by make_golden_cm.py): every evaluation's noise
level bit for bit, its time input 250 ln(sigma + 1e-44) to one ulp (torch's CPU log rounds differently by one ulp on different
CPU instruction sets), the Q bases bit for bit, the letter mask when the recorded font is present.  Also: NFE,
draw order, the distillation pairing, argument errors, the C-ABI entry's argument checks (before any device call) and the
generate_large.py flags."""
import ctypes
import os

import numpy as np
import pytest
import torch

EINVAL = -1       # DXMI_EINVAL
CASES = {   # name: (kind, ts) with steps 40
    "onestep": ("onestep", None),
    "multistep_0_22_39": ("multistep", (0, 22, 39)),
    "multistep_0_10_20": ("multistep", (0, 10, 20)),
    "colorization": ("multistep", (0, 22, 39)),
    "superres": ("multistep", (0, 22, 39)),
    "inpainting": ("multistep", (0, 10, 20)),
}
FONT_DIRS = ("/usr/share/fonts/truetype/dejavu", "/usr/share/fonts/TTF", "/usr/share/fonts/dejavu")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "cm_sample.npz"))


def diffusion(distillation=True):
    from models.cm.karras_diffusion import KarrasDenoiser
    return KarrasDenoiser(sigma_data=0.5, sigma_max=80.0, sigma_min=0.002, weight_schedule="uniform", distillation=distillation)


def schedule(case, **kw):
    from models.cm.karras_diffusion import CMSchedule, get_sigmas_karras
    kind, ts = CASES[case]
    if kind == "onestep":
        return CMSchedule("onestep", diffusion(), sigma0=float(get_sigmas_karras(40, 0.002, 80.0, 7.0)[0]), **kw)
    return CMSchedule("multistep", diffusion(), ts=ts, steps=40, **kw)


def f32(t):
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32))


def bits(t):
    return f32(t).view(np.uint32)


@pytest.mark.parametrize("case", list(CASES))
def test_schedule_tables_vs_reference(gold, case):
    from dxmi_hip import ops
    sch = schedule(case)
    np.testing.assert_array_equal(bits(sch.eval_sigmas), bits(gold[f"{case}.eval_sigma"]))
    np.testing.assert_array_max_ulp(f32(sch.table[:sch.nfe, ops.CT_T]), f32(gold[f"{case}.eval_t"]), maxulp=1)
    diff = diffusion()
    for k in range(1, sch.nfe + 1):       # boundary-condition scalings of the fp32 sigma, as denoise() with distillation
        c_skip, c_out, c_in = diff.get_scalings_for_boundary_condition(sch.eval_sigmas[k - 1].reshape(1))
        assert torch.equal(sch.table[k, ops.CT_CSKIP].reshape(1), c_skip)
        assert torch.equal(sch.table[k, ops.CT_COUT].reshape(1), c_out)
        assert torch.equal(sch.table[k - 1, ops.CT_CIN].reshape(1), c_in)


def test_noise_factors():
    from dxmi_hip import ops
    t_min_rho, t_max_rho = 0.002 ** (1 / 7), 80.0 ** (1 / 7)
    for case in ("multistep_0_22_39", "multistep_0_10_20"):
        sch = schedule(case)
        ts = CASES[case][1]
        for i in range(len(ts) - 1):
            nt = np.clip((t_max_rho + ts[i + 1] / 39 * (t_min_rho - t_max_rho)) ** 7, 0.002, 80.0)
            want = np.sqrt(nt ** 2 - 0.002 ** 2)
            assert sch.noise[i] == want and sch.table[i + 1, ops.CT_NOISE].item() == np.float32(want)
    # ts[-1] = steps - 1 leaves only the float64 residue of (t_min^(1/rho))^rho - t_min; ts ending at 20 leaves real noise
    assert schedule("multistep_0_22_39").noise[-1] < 1e-8 and schedule("multistep_0_10_20").noise[-1] > 1.0
    assert schedule("onestep").table[1, ops.CT_NOISE] == 0


def test_multistep_uses_diffusion_rho():
    """karras_sample's multistep branch takes rho from the diffusion, not from its rho argument (reference :400)."""
    from dxmi_hip._lib import DxmiError
    import models.cm.karras_diffusion as kd
    d = diffusion()
    d.rho = 5.0
    kd._CM_SCHEDULES.clear()
    with pytest.raises(DxmiError):
        kd.karras_sample(d, lambda x, t: x, (1, 3, 8, 8), 40, sampler="multistep", ts=(0, 10, 20), rho=7.0, device="cpu")
    (sch,) = kd._CM_SCHEDULES.values()
    assert sch.t[1] == (80.0 ** 0.2 + 10 / 39 * (0.002 ** 0.2 - 80.0 ** 0.2)) ** 5.0
    assert sch.table[0, 5] == 80.0 and sch.table[0, 7] == 1.0       # XSCALE = sigma_max, OUTCLAMP on


def test_q_bases_bitwise(gold):
    from models.cm.karras_diffusion import colour_basis, patch_basis
    np.testing.assert_array_equal(bits(colour_basis()), bits(gold["Q3"]))
    np.testing.assert_array_equal(bits(patch_basis()), bits(gold["Q64"]))


@pytest.mark.parametrize("case", list(CASES))
def test_nfe_and_draw_count(gold, case):
    from models.cm.karras_diffusion import cm_nfe
    sch = schedule(case)
    kind, ts = CASES[case]
    assert sch.nfe == cm_nfe(kind, ts) == len(gold[f"{case}.eval_sigma"]) == (1 if kind == "onestep" else len(ts) - 1)
    # x_T (or the editing loops' x), then one randn_like per multistep step, the last included
    assert len(gold[f"{case}.analytic.draws"]) == 1 + (0 if kind == "onestep" else sch.nfe)


class CountingGenerator:
    def __init__(self):
        self.calls = []

    def randn(self, *shape, device=None):
        self.calls.append(("randn", tuple(shape)))
        return torch.zeros(shape)

    def randn_like(self, x):
        self.calls.append(("randn_like", tuple(x.shape)))
        return torch.zeros_like(x)


def test_draw_order_with_generator(monkeypatch):
    """The launch loop calls randn once (x_T) and randn_like once per multistep step, in the reference's order; the stage
    kernel is replaced by a recorder, so no device is needed."""
    from dxmi_hip import ops
    import models.cm.karras_diffusion as kd
    stages = []
    monkeypatch.setattr(ops, "cm_stage", lambda mode, last, tab, row, x, **k: stages.append((mode, last, row, k.get("noise"))))
    for case in ("onestep", "multistep_0_10_20", "multistep_0_22_39"):
        stages.clear()
        sch = schedule(case)
        gen = CountingGenerator()
        den = kd.KarrasDenoiserFn(diffusion(), lambda x, t: x)
        monkeypatch.setattr(sch, "device_table", lambda device: sch.table)
        kd._run_stages(sch, den, None, (2, 3, 8, 8), torch.device("cpu"), gen)
        assert gen.calls == [("randn", (2, 3, 8, 8))] + [("randn_like", (2, 3, 8, 8))] * (sch.nfe if sch.sampler == "multistep" else 0)
        assert [(m, l, r) for m, l, r, _ in stages] == [(ops.CM_FIRST, False, 0)] + \
            [(ops.CM_STEP, k == sch.nfe, k) for k in range(1, sch.nfe + 1)]
        assert stages[0][3] is None and all((n is not None) == (sch.sampler == "multistep") for *_, n in stages[1:])


def test_pairing_rule():
    from models.cm.karras_diffusion import KarrasDenoiser, KarrasDenoiserFn, karras_sample, sample_heun, sample_onestep
    plain, distilled = KarrasDenoiser(), KarrasDenoiser(distillation=True)
    for s in ("onestep", "multistep", "progdist"):
        with pytest.raises(NotImplementedError, match="consistency-distilled"):
            karras_sample(plain, lambda x, t: x, (1, 3, 8, 8), 4, sampler=s, ts=(0, 2))
    with pytest.raises(NotImplementedError, match="consistency-distilled"):
        karras_sample(distilled, lambda x, t: x, (1, 3, 8, 8), 4, sampler="progdist")
    for s in ("heun", "dpm", "euler", "ancestral"):
        with pytest.raises(NotImplementedError, match="distillation"):
            karras_sample(distilled, lambda x, t: x, (1, 3, 8, 8), 4, sampler=s)
    with pytest.raises(NotImplementedError, match="distillation"):
        sample_heun(KarrasDenoiserFn(distilled, lambda x, t: x), torch.zeros(1, 3, 8, 8), torch.ones(3), None)
    with pytest.raises(NotImplementedError, match="consistency-distilled"):
        sample_onestep(KarrasDenoiserFn(plain, lambda x, t: x), torch.zeros(1, 3, 8, 8), torch.ones(3))
    # distilled samplers get past the pairing check: on the CPU they stop at the device check
    from dxmi_hip._lib import DxmiError
    with pytest.raises(DxmiError, match="HIP device path"):
        karras_sample(distilled, lambda x, t: x, (1, 3, 8, 8), 40, sampler="multistep", ts=(0, 22, 39), device="cpu")
    with pytest.raises(DxmiError, match="HIP device path"):
        sample_onestep(KarrasDenoiserFn(distilled, lambda x, t: x), torch.zeros(1, 3, 8, 8), torch.ones(3))


def test_argument_errors():
    from models.cm.karras_diffusion import (KarrasDenoiserFn, karras_sample, inpainting_mask, iterative_inpainting,
                                            iterative_superres, stochastic_iterative_sampler)
    d = diffusion()
    fn = KarrasDenoiserFn(d, lambda x, t: x)
    for ts in (None, (0,), (0, 40), (-1, 3)):
        with pytest.raises(ValueError, match="ts"):
            karras_sample(d, lambda x, t: x, (1, 3, 8, 8), 40, sampler="multistep", ts=ts)
        with pytest.raises(ValueError, match="ts"):
            stochastic_iterative_sampler(fn, torch.zeros(1, 3, 8, 8), None, None, ts)
    with pytest.raises(ValueError, match="multiples of 8"):
        iterative_superres(fn, torch.zeros(1, 3, 12, 12), torch.zeros(1, 3, 12, 12), (0, 22, 39))
    with pytest.raises(ValueError, match="mask"):
        iterative_inpainting(fn, torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), (0, 22, 39), mask=torch.ones(2, 1, 8, 8))
    with pytest.raises(ValueError, match="multiple of 7"):
        iterative_inpainting(fn, torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), (0, 22, 39))
    with pytest.raises(ValueError, match="font"):
        inpainting_mask(7, 16, None)
    with pytest.raises(FileNotFoundError):
        inpainting_mask(7, 16, "/nonexistent/arial.ttf")


def test_inpainting_mask_vs_reference(gold):
    from models.cm.karras_diffusion import inpainting_mask
    name = bytes(gold["font"]).decode()
    path = next((os.path.join(d, name) for d in FONT_DIRS if os.path.isfile(os.path.join(d, name))), None)
    if path is None:
        pytest.skip(f"the recorded font {name} is not installed")
    m = inpainting_mask(14, 256, path)
    n = 3 * 256 * 256
    g0 = np.unpackbits(gold["mask256.g0"])[:n].reshape(3, 256, 256).astype(bool)
    g1 = np.unpackbits(gold["mask256.g1"])[:n].reshape(3, 256, 256).astype(bool)
    assert g0.any() and g1.any() and not (g0 & g1).any()
    for i in range(14):
        np.testing.assert_array_equal(m[i].numpy() > 0.5, g0 if i < 7 else g1)


def test_stage_entry_rejects_bad_arguments():
    """dxmi_cm_stage validates before it touches the device."""
    from dxmi_hip import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(16)                 # never dereferenced: every call below fails its argument check
    null = ctypes.c_void_p(0)

    def call(mode=ops.CM_STEP, edit=ops.CM_EDIT_NONE, last=0, tab=p, Q=null, x=p, F=p, noise=null, ref=null, mask=null, x_in=p,
             t=p, out=null, N=2, C=3, H=16, W=16):
        return lib.dxmi_cm_stage(mode, edit, last, tab, 0, Q, x, F, noise, ref, mask, x_in, t, out, null, N, C, H, W, null)
    assert call(mode=2) == EINVAL and b"unknown mode" in lib.dxmi_last_error()
    assert call(mode=-1) == EINVAL
    assert call(edit=4) == EINVAL and b"unknown edit" in lib.dxmi_last_error()
    assert call(N=0) == EINVAL and call(C=0) == EINVAL and call(H=-1) == EINVAL and call(W=0) == EINVAL
    assert call(N=70000) == EINVAL
    assert call(C=1, H=3, W=5) == EINVAL and b"multiple of 4" in lib.dxmi_last_error()
    assert call(tab=null) == EINVAL and call(x=null) == EINVAL and call(F=null) == EINVAL
    assert call(mode=ops.CM_FIRST, last=1, out=p) == EINVAL and b"first stage cannot be the last" in lib.dxmi_last_error()
    assert call(mode=ops.CM_FIRST, edit=ops.CM_EDIT_MASK, ref=p, mask=p) == EINVAL
    assert call(mode=ops.CM_FIRST, noise=p) == EINVAL
    assert call(last=1) == EINVAL and call(x_in=null) == EINVAL and call(t=null) == EINVAL
    assert call(edit=ops.CM_EDIT_MASK, mask=p) == EINVAL and call(edit=ops.CM_EDIT_MASK, ref=p) == EINVAL
    assert call(edit=ops.CM_EDIT_COLOUR, ref=p) == EINVAL and b"needs Q" in lib.dxmi_last_error()
    assert call(edit=ops.CM_EDIT_COLOUR, ref=p, Q=p, C=4) == EINVAL and b"C = 3" in lib.dxmi_last_error()
    assert call(edit=ops.CM_EDIT_PATCH, ref=p, Q=p, H=12) == EINVAL and b"multiples of 8" in lib.dxmi_last_error()
    assert call(edit=ops.CM_EDIT_PATCH, ref=p, Q=p, W=20) == EINVAL


# ------------------------------------------------------------------------------------------------ generate_large.py flags
def test_cli_cm_flags_parse():
    import generate_large as g
    base = ["--log_dir", "d", "--n_sample", "4"]
    a, _ = g.parse_args(base)
    assert a.cm_sampler is None and a.ts is None and a.cm_steps is None
    a, _ = g.parse_args(base + ["--cm_sampler", "onestep"])
    assert (a.cm_sampler, a.cm_steps, a.ts) == ("onestep", 40, None)
    a, _ = g.parse_args(base + ["--cm_sampler", "multistep", "--ts", "0,22,39"])
    assert (a.cm_steps, a.ts) == (40, (0, 22, 39))
    a, _ = g.parse_args(base + ["--cm_sampler", "multistep", "--ts", "0,10", "--cm_steps", "18", "--pretrained", "cd.pt"])
    assert (a.cm_steps, a.ts, a.pretrained) == (18, (0, 10), "cd.pt")
    a, _ = g.parse_args(base + ["--cm_sampler", "onestep", "--pretrained"])
    assert a.pretrained == ""


@pytest.mark.parametrize("extra", [
    ["--cm_sampler", "multistep"],                                       # ts required
    ["--cm_sampler", "multistep", "--ts", "0,40"],                       # out of range for 40 steps
    ["--cm_sampler", "multistep", "--ts", "0"],                          # one index: no evaluation
    ["--cm_sampler", "multistep", "--ts", "0,a"],
    ["--cm_sampler", "onestep", "--ts", "0,22"],
    ["--cm_sampler", "onestep", "--karras_sampler", "heun"],
    ["--cm_sampler", "onestep", "--guidance_scale", "1.5"],
    ["--cm_sampler", "onestep", "--s_churn", "3"],
    ["--ts", "0,22,39"],
    ["--cm_steps", "18"],
    ["--karras_sampler", "heun", "--ts", "0,22"],
    ["--cm_sampler", "heun"],
])
def test_cli_cm_conflicts(extra):
    import generate_large as g
    with pytest.raises(SystemExit):
        g.parse_args(["--log_dir", "d", "--n_sample", "4"] + extra)
