"""LPIPS on the GPU (csrc/lpips.hip, dxmi_hip/lpips_ops.py, models/cm/lpips.py): every new launch against float64 on the same
bf16 / fp32 operands, the whole network against the fp64 restatement of tests/lpips_ref.py (exact, and with its bf16 storage
model), the lpips norm of consistency_losses on the shrunken HIP U-Nets (CD and CT), CMTrainLoop run-to-run bits, a full-size
step and malformed calls.

Bounds.  UB = 2^-8 is the unit roundoff of a bf16 store (8 significant bits, round to nearest even), U = 2^-24 of an fp32 operation.  A launch that stores bf16 is held to
(1 + 2^-6) UB |ref| (the store; the slack covers the fp32 value it rounds lying within a few U of the exact one across a rounding
boundary) + k U M for the k fp32 operations behind it on operands of magnitude M; each test states its k and M.  Whole-network
values: against the storage model only fp32 accumulation order differs, which flips individual bf16 roundings of either sign.
STORAGE_REL holds one bound per kind of case, each twice the worst figure measured on an MI355X for that kind: plain
LPIPS 9.543e-4 (N = 3, 16 -> 40; the 64 -> 224 case measured 3.112e-5), consistency training 1.229e-3, consistency distillation
5.007e-3.  The last is the sample at ladder index 4 of 6, whose target is x_t2 itself (c_out(sigma_min) = 0) and whose two images are
so close that the bf16 roundings carry 38 % of the value (the storage model's own gap to exact fp64), so a flipped rounding weighs
most there.  Against exact fp64 the bound is twice the gap the storage model itself shows on the same inputs, computed on the CPU.
Gradients: cosine >= 0.995 and norm within 5 % (the project's gradient bounds)."""
import math

import pytest
import torch
import torch.nn.functional as Fn

import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, UB = 2.0 ** -24, 2.0 ** -8
STORE = (1 + 2.0 ** -6) * UB
STORAGE_REL = {"lpips": 1.91e-3, "ct": 2.46e-3, "cd": 1.0e-2}      # device value against the bf16 storage model: twice the worst measured
MIN_TAP_SHARE = 0.05


@pytest.fixture(scope="module")
def lo():
    from dxmi_hip import lpips_ops, ops
    ops.device_check()
    return lpips_ops


@pytest.fixture(scope="module")
def lp():
    from models.cm.lpips import LPIPS
    return LPIPS(*R.formula_weights())


def _bf(t):
    return t.to(torch.bfloat16)


def _close(got, ref, tol, what):
    err = (got.double().cpu() - ref).abs()
    over = (err - tol).max().item()
    print(f"{what}: worst error {err.max().item():.3e}, worst error / bound {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert over <= 0, f"{what}: error exceeds its bound by {over:.3e}"


# ------------------------------------------------------------------------------------------------ single launches
@pytest.mark.parametrize("shape", [(3, 5, 5, 64), (2, 2, 2, 512), (1, 14, 14, 512)])
def test_tap_distance_vs_fp64(lo, shape):
    N, h, w, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    fx, fy = (_bf(torch.relu(torch.randn(shape, generator=g))) for _ in range(2))
    fx[0, 0, 1] = 0                                                   # an all-zero pixel: only eps keeps 1 / |f| finite
    wt = 0.1 + torch.rand(C, generator=g)
    gu = torch.randn(N, generator=g)
    X = fx.double().requires_grad_(True)
    ref = R.tap_distance(X.permute(0, 3, 1, 2), fy.double().permute(0, 3, 1, 2), wt)
    ref.backward(gu.double())
    d = [t.to(DEV) for t in (fx, fy, wt, gu)]
    got = lo.tap_fwd(d[0], d[1], d[2])
    # every term is >= 0, so the fp32 sum is within (number of sequential additions) U of it: at most ceil(hw / 8) pixels per lane
    # x 8 channels x 3 operations, 8 shuffle steps, 4 wave partials and at most 128 workgroup partials; the per-pixel sqrt and
    # reciprocals add 8 U
    k = math.ceil(h * w / 8) * 24 + 8 + 4 + 128 + 8
    _close(got, ref.detach(), k * U * ref.detach().abs(), f"tap forward {shape}")
    acc = lo.tap_fwd(d[0], d[1], d[2], out=got.clone(), scale=d[3])                                        # accumulate, then scale
    assert ((acc - (got + got) * d[3]).abs() <= 4 * U * (2 * got * d[3]).abs()).all()
    gb = lo.tap_bwd(d[3], d[0], d[1], d[2])
    # d fx = q a - fx k: a bf16 store of the difference of two fp32 terms, each a product of <= 8 factors and a C-term dot product
    # (log2(C) + 8 sequential additions); M = |q a| + |fx k| per element, bounded here by the pixel's largest |q a| times (1 + C |f^|)
    Xd, Yd = fx.double(), fy.double()
    nx, ny = Xd.norm(dim=3, keepdim=True), Yd.norm(dim=3, keepdim=True)
    q = 2 * wt.double() * (Xd / (nx + 1e-10) - Yd / (ny + 1e-10)) * (gu.double() / (h * w)).view(N, 1, 1, 1)
    M = (q.abs() / (nx + 1e-10)) + Xd.abs() * (Xd.abs() * q.abs()).sum(3, keepdim=True) / (nx.clamp_min(1e-300) * (nx + 1e-10) ** 2)
    _close(gb, X.grad, STORE * X.grad.abs() + 32 * U * M, f"tap backward {shape}")
    assert torch.isfinite(gb).all()
    ones = lo.tap_bwd(None, d[0], d[1], d[2])                         # no upstream: ones
    assert torch.equal(ones, lo.tap_bwd(torch.ones(N, device=DEV), d[0], d[1], d[2]))


@pytest.mark.parametrize("size", [5, 4])
def test_avgpool_vs_fp64(lo, size):
    g = torch.Generator().manual_seed(size)
    x = _bf(torch.randn(2, size, size, 24, generator=g))
    X = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    ref = Fn.avg_pool2d(X, 2, 2, 0)
    go = _bf(torch.randn(2, size // 2, size // 2, 24, generator=g))
    ref.backward(go.double().permute(0, 3, 1, 2))
    got = lo.avgpool2x2(x.to(DEV))
    # three fp32 additions of magnitude <= sum|x| and an exact scaling by 1/4, then the store
    M = Fn.avg_pool2d(X.detach().abs(), 2, 2, 0) * 4
    _close(got.permute(0, 3, 1, 2), ref.detach(), STORE * ref.detach().abs() + 3 * U * M, f"avgpool forward {size}")
    gi = lo.avgpool2x2_bwd(go.to(DEV), size, size)
    assert torch.equal(gi.cpu().double().permute(0, 3, 1, 2), X.grad)   # g / 4 is exact in bf16; zeros in the dropped row / column
    if size % 2:
        assert (gi[:, -1] == 0).all() and (gi[:, :, -1] == 0).all()


def test_relu_mask_acc(lo):
    g = torch.Generator().manual_seed(3)
    a, b = (_bf(torch.randn(2, 3, 5, 16, generator=g)) for _ in range(2))
    act = _bf(torch.relu(torch.randn(2, 3, 5, 16, generator=g)))
    assert (act == 0).any()
    ref = (a.double() + b.double()) * (act > 0)
    got = lo.relu_mask_acc(a.to(DEV), b.to(DEV), act.to(DEV)).cpu()
    _close(got, ref, STORE * ref.abs(), "masked accumulate")           # one fp32 addition (exact or within U), one store
    assert (got[act == 0] == 0).all()
    assert torch.equal(lo.relu_mask_acc(a.to(DEV), None, act.to(DEV)).cpu(), a * (act > 0))


@pytest.mark.parametrize("size,resize", [(16, 40), (64, 224), (12, None)])
def test_front_end_vs_fp64(lo, size, resize):
    g = torch.Generator().manual_seed(size)
    x = torch.rand(2, 3, size, size, generator=g)
    out = resize or size
    X = x.double().requires_grad_(True)
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (R.MEAN, R.STD))
    xi = Fn.interpolate(X, size=resize, mode="bilinear") if resize else X
    ref = (xi - mean) / std
    gz = torch.zeros(2, out, out, 16, dtype=torch.bfloat16)
    gz[..., :3] = _bf(torch.randn(2, out, out, 3, generator=g))
    gz[..., 3:] = 7.0                                                  # the padding channels must not be read
    ref.backward(gz[..., :3].double().permute(0, 3, 1, 2))
    got = lo.front_fwd(x.to(DEV), resize)
    assert got.shape == (2, out, out, 16) and (got[..., 3:] == 0).all()
    # source index and weights (6 fp32 operations on values <= 1: the weights are within 8 U size of exact), the 4-tap blend
    # (7 operations on values <= 1), minus mean, over std: <= (8 size + 16) U / std, then the store
    _close(got[..., :3].permute(0, 3, 1, 2), ref.detach(), STORE * ref.detach().abs() + (8 * size + 16) * U / 0.224, f"front end {size}->{out}")
    dx = lo.front_bwd(gz.to(DEV), size, size)
    # the transpose: each source pixel sums <= (out / size + 2)^2 weighted taps, weights within 8 U size, M = the same sum of |g|
    Xa = x.double().requires_grad_(True)
    xa = Fn.interpolate(Xa, size=resize, mode="bilinear") if resize else Xa
    (xa / std).backward(gz[..., :3].double().abs().permute(0, 3, 1, 2))
    k = (out // size + 3) ** 2 + 8 * size + 8
    _close(dx, X.grad, k * U * Xa.grad, f"front end transpose {out}->{size}")


@pytest.mark.parametrize("cin,cout", [(3, 64), (64, 128), (512, 512)])
def test_gradient_conv_vs_fp64(lo, cin, cout):
    """The data gradient of conv(Cin -> Cout) as ops.gconv on the packed w.transpose(0, 1).flip(2, 3), 6x5 maps."""
    from dxmi_hip import ops
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    gy = _bf(torch.randn(2, 6, 5, cout, generator=g))
    wb = w.to(torch.bfloat16).double()
    ref = torch.nn.grad.conv2d_input((2, cin, 6, 5), wb, gy.double().permute(0, 3, 1, 2), padding=1)
    M = torch.nn.grad.conv2d_input((2, cin, 6, 5), wb.abs(), gy.double().abs().permute(0, 3, 1, 2), padding=1)
    pk = ops.gconv_pack(w.to(DEV).transpose(0, 1).flip(2, 3).contiguous())
    out = torch.zeros(2, 6, 5, 16, dtype=torch.bfloat16, device=DEV) if cin == 3 else None
    got = ops.gconv(gy.to(DEV), pk, pad=(1, 1), relu=False, out=out)
    assert got.shape[-1] == (16 if cin == 3 else cin)
    # bf16 x bf16 products are exact in fp32; 9 cout of them are added in the MFMA's order: 9 cout U M, then the store
    _close(got[..., :cin].permute(0, 3, 1, 2), ref, STORE * ref.abs() + 9 * cout * U * M, f"gradient conv {cin}<-{cout}")
    if cin == 3:
        assert (got[..., 3:] == 0).all()


# ------------------------------------------------------------------------------------------------ the whole network
def _grad_close(got, want, what):
    got, want = got.double().cpu().flatten(1), want.flatten(1)
    cos = Fn.cosine_similarity(got, want).min().item()
    nrm = (got.norm(dim=1) / want.norm(dim=1) - 1).abs().max().item()
    print(f"{what}: worst cosine {cos:.5f}, worst norm deviation {nrm:.4f}")
    assert cos >= 0.995 and nrm <= 0.05, (what, cos, nrm)


def _value_close(got, exact, model, what, bound):
    got = got.detach().double().cpu()
    rel_m = ((got - model).abs() / model).max().item()
    rel_e = ((got - exact).abs() / exact).max().item()
    gap = ((model - exact).abs() / exact).max().item()
    print(f"{what}: against the storage model {rel_m:.3e} (bound {bound}); against exact fp64 {rel_e:.3e} (storage model's own gap {gap:.3e})")
    assert rel_m <= bound, (what, rel_m)
    assert rel_e <= 2 * gap, (what, rel_e, gap)


@pytest.mark.parametrize("N,size,resize", [(3, 16, 40), (1, 64, 224)])
def test_lpips_device_vs_fp64(lo, lp, N, size, resize):
    x, y = R.images(N, size)
    exact = R.lpips_ref(x, y, resize=resize, grad=True)
    model = R.lpips_ref(x, y, resize=resize, storage=True)
    share = exact["taps"] / exact["value"]
    assert share.min() >= MIN_TAP_SHARE, f"a tap carries {share.min():.3f} of a sample's value"
    xd = x.to(DEV).requires_grad_(True)
    v = lp(xd, y.to(DEV), resize=resize)
    assert v.shape == (N,) and v.dtype == torch.float32 and v.requires_grad
    gu = torch.linspace(0.5, 1.5, N)
    (v * gu.to(DEV)).sum().backward()
    _value_close(v, exact["value"], model["value"], f"lpips {N}x{size}->{resize}", STORAGE_REL["lpips"])
    _grad_close(xd.grad, exact["dx"] * gu.double().view(N, 1, 1, 1), f"lpips d x {N}x{size}->{resize}")
    with torch.no_grad():
        assert torch.equal(lp(xd, y.to(DEV), resize=resize), v.detach())
    with pytest.raises(NotImplementedError, match="y must not require grad"):
        lp(xd, y.to(DEV).requires_grad_(True), resize=resize)


# ------------------------------------------------------------------------------------------------ consistency_losses
def _nets(mode):
    from test_hip_cm_train import PLAIN, build
    online = build(PLAIN)
    for p in online.parameters():
        p.requires_grad_(True)
    return online, build(PLAIN, "target:", 0.9), (build(PLAIN, "teacher:") if mode == "cd" else None)


@pytest.mark.parametrize("mode", ["cd", "ct"])
def test_consistency_losses_lpips_on_hip_unets(lo, lp, monkeypatch, mode):
    from models.cm.karras_diffusion import KarrasDenoiser, cd_levels
    online, target, teacher = _nets(mode)
    student = KarrasDenoiser(distillation=True, loss_norm="lpips", lpips_loss=lp)
    td = KarrasDenoiser(distillation=False) if mode == "cd" else None
    g = torch.Generator().manual_seed(11)
    N, S = 2, 6
    x0 = (torch.rand(N, 3, 16, 16, generator=g) * 2 - 1).to(DEV)
    noise = torch.randn(N, 3, 16, 16, generator=g).to(DEV)
    idx = torch.tensor([3, 4], device=DEV)
    rec = {}
    images, bwd = lo.cd_lpips_images, lo.cd_lpips_bwd

    def rec_images(F, F_tg, x_t, x_t2, *a, **k):
        rec.update(F=F, F_tg=F_tg, x_t=x_t, x_t2=x_t2)
        return images(F, F_tg, x_t, x_t2, *a, **k)

    def rec_bwd(*a, **k):
        rec["dF"] = bwd(*a, **k)
        return rec["dF"]

    monkeypatch.setattr(lo, "cd_lpips_images", rec_images)
    monkeypatch.setattr(lo, "cd_lpips_bwd", rec_bwd)
    call = lambda: student.consistency_losses(online, x0, S, target_model=target, teacher_model=teacher, teacher_diffusion=td,
                                              noise=noise, indices=idx)["loss"]
    loss = call()
    gu = torch.tensor([0.75, 1.25], device=DEV)
    (loss * gu).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in online.parameters())
    tab = cd_levels(S, student.sigma_min, student.sigma_max, student.rho).table
    t, t2 = tab[idx.cpu()], tab[idx.cpu() + 1]
    ops64 = [rec[k].detach().cpu() for k in ("F", "F_tg", "x_t", "x_t2")]
    exact = R.cd_lpips_ref(*ops64, t, t2, sigma_min=float(torch.tensor(0.002, dtype=torch.float32)), grad=True)
    model = R.cd_lpips_ref(*ops64, t, t2, sigma_min=float(torch.tensor(0.002, dtype=torch.float32)), storage=True)
    _value_close(loss, exact["loss"], model["loss"], f"consistency_losses lpips {mode}", STORAGE_REL[mode])
    _grad_close(rec["dF"], exact["dF"] * gu.cpu().double().view(N, 1, 1, 1), f"consistency_losses lpips {mode} d F")
    with torch.no_grad():
        again = call()
    assert torch.equal(again, loss.detach()) and not again.requires_grad


def test_cmtrainloop_lpips_two_runs_bitwise(lo, lp, tmp_path):
    import test_hip_cm_train as T
    x, _, _ = T._data()

    def run(tmp):
        tl = T._loop(tmp, "consistency_training")
        tl.diffusion.d.loss_norm, tl.diffusion.d.lpips_loss = "lpips", lp
        t0 = [p.detach().clone() for p in tl.target_model_master_params]
        for k in range(3):
            assert tl.run_step(x[k], {})
        return t0, [p.detach().clone() for p in tl.mp_trainer.master_params], [p.detach().clone() for p in tl.target_model_master_params]

    t0, ma, ta = run(tmp_path / "a")
    _, mb, tb = run(tmp_path / "b")
    assert all(torch.equal(u, v) for u, v in zip(ma + ta, mb + tb))
    assert any(not torch.equal(u, v) for u, v in zip(t0, ta))            # the target moves


def test_imagenet64_full_size_cd_step_lpips(lo, lp):
    from backward_census import EDM_DSM_MODEL as kw
    from models.cm.script_util import create_model_and_diffusion
    torch.manual_seed(0)
    online, student = create_model_and_diffusion(**dict(kw, distillation=True))
    target, _ = create_model_and_diffusion(**kw)
    teacher, teacher_diffusion = create_model_and_diffusion(**kw)
    online, target, teacher = online.to(DEV).train(), target.to(DEV).train().requires_grad_(False), teacher.to(DEV).eval().requires_grad_(False)
    student.loss_norm, student.lpips_loss = "lpips", lp
    x0 = torch.rand(2, 3, 64, 64, device=DEV) * 2 - 1
    t = student.consistency_losses(online, x0, 40, model_kwargs={"y": torch.arange(2, device=DEV)}, target_model=target,
                                   teacher_model=teacher, teacher_diffusion=teacher_diffusion)
    t["loss"].mean().backward()
    assert torch.isfinite(t["loss"]).all() and t["loss"].shape == (2,)
    for p in online.parameters():
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all()
    print(f"imagenet64 CD step with lpips at 2 images: loss {t['loss'].tolist()}")


# ------------------------------------------------------------------------------------------------ malformed calls
def test_wrappers_refuse_malformed_arguments(lo):
    from dxmi_hip import DxmiError, ops
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    idx, tab = torch.zeros(2, dtype=torch.int64, device=DEV), f32(6) + 1
    img = f32(2, 3, 8, 8)
    bad = [
        lambda: lo.tap_fwd(None, bf(2, 4, 4, 64), f32(64)),                                   # null
        lambda: lo.tap_fwd(bf(2, 4, 4, 64).float(), bf(2, 4, 4, 64), f32(64)),                # dtype
        lambda: lo.tap_fwd(bf(2, 4, 4, 40), bf(2, 4, 4, 40), f32(40)),                        # C % 16
        lambda: lo.tap_fwd(bf(2, 4, 4, 1024), bf(2, 4, 4, 1024), f32(1024)),                  # C > 512
        lambda: lo.tap_fwd(bf(2, 4, 4, 64), bf(3, 4, 4, 64), f32(64)),                        # N mismatch
        lambda: lo.tap_fwd(bf(2, 4, 4, 64), bf(2, 4, 4, 64), f32(32)),                        # w
        lambda: lo.tap_fwd(bf(2, 4, 4, 64), bf(2, 4, 4, 64), f32(64), out=f32(3)),            # out
        lambda: lo.tap_fwd(bf(2, 4, 4, 64), bf(2, 4, 4, 64), f32(64).cpu()),                  # host tensor
        lambda: lo.tap_bwd(f32(3), bf(2, 4, 4, 64), bf(2, 4, 4, 64), f32(64)),                # g
        lambda: lo.tap_bwd(None, bf(2, 4, 4, 64), None, f32(64)),
        lambda: lo.tap_bwd(None, bf(2, 4, 4, 24), bf(2, 4, 4, 24), f32(24)),
        lambda: lo.avgpool2x2(None),
        lambda: lo.avgpool2x2(f32(2, 4, 4, 16)),
        lambda: lo.avgpool2x2(bf(2, 4, 4, 12)),                                               # C % 8
        lambda: lo.avgpool2x2(bf(2, 1, 4, 16)),                                               # a 1-pixel map
        lambda: lo.avgpool2x2_bwd(bf(2, 2, 2, 16), 6, 6),                                     # not the pool of a 6x6 map
        lambda: lo.avgpool2x2_bwd(bf(2, 2, 2, 16).float(), 4, 4),
        lambda: lo.relu_mask_acc(None, None, bf(2, 4, 4, 16)),
        lambda: lo.relu_mask_acc(bf(2, 4, 4, 16), bf(2, 4, 4, 8), bf(2, 4, 4, 16)),
        lambda: lo.relu_mask_acc(bf(2, 4, 4, 16), None, bf(2, 4, 4, 16).float()),
        lambda: lo.relu_mask_acc(bf(1, 1, 1, 4), None, bf(1, 1, 1, 4)),                       # numel % 8
        lambda: lo.front_fwd(None),
        lambda: lo.front_fwd(f32(2, 4, 8, 8)),                                                # 3 channels
        lambda: lo.front_fwd(img.double()),
        lambda: lo.front_fwd(img, 0),
        lambda: lo.front_bwd(bf(2, 8, 8, 8), 8, 8),                                           # 16 channels
        lambda: lo.front_bwd(bf(2, 8, 8, 16).float(), 8, 8),
        lambda: lo.front_bwd(None, 8, 8),
        lambda: lo.cd_lpips_images(None, img, img, img, idx, tab, "karras"),
        lambda: lo.cd_lpips_images(img, img.double(), img, img, idx, tab, "karras"),
        lambda: lo.cd_lpips_images(img, f32(3, 3, 8, 8), img, img, idx, tab, "karras"),
        lambda: lo.cd_lpips_images(img, img, img, img, idx[:1], tab, "karras"),
        lambda: lo.cd_lpips_images(img, img, img, None, idx, tab, "karras"),
        lambda: lo.cd_lpips_bwd(None, img, idx, tab, "karras"),
        lambda: lo.cd_lpips_bwd(f32(3), img, idx, tab, "karras"),
        lambda: lo.cd_lpips_bwd(f32(2), img, idx, tab[:1], "karras"),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(DxmiError):
            fn()
            pytest.fail(f"malformed call {i} was accepted")
    with pytest.raises(DxmiError):                       # the norm table of the fused l1 / l2 / l2-32 launch is not extended
        ops.cd_loss_fwd(img, img, img, img, idx, tab, "lpips", "karras")
    torch.cuda.synchronize()
