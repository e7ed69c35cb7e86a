"""LPIPS on the CPU: the torch path of models.cm.lpips against the fp64 restatement of tests/lpips_ref.py on formula weights
(parity with piq is unpinned: the reference imports no LPIPS), loading, and the lpips branch of consistency_losses."""
import pytest
import torch

import lpips_ref as R
from models.cm import karras_diffusion as kd
from models.cm.karras_diffusion import KarrasDenoiser, cd_levels
from models.cm.lpips import LPIPS, tap_distance

RTOL = 1e-4          # fp32 torch against fp64 over 13 layers, values (measured: DESIGN 5.15)
# d x of fp32 torch against fp64: roundoff 6e-8 per operation through 13 layers, plus ReLU masks that differ where a pre-activation
# lies within roundoff of zero (a discrete change of a few gradient paths); held two orders of magnitude inside the device path's
# bounds (cosine 0.995, norm 5 %)
GRAD_COS, GRAD_NORM = 1 - 5e-5, 5e-4
MIN_TAP_SHARE = 0.05


@pytest.fixture(scope="module")
def lp():
    return LPIPS(*R.formula_weights())


def _check_taps(ref):
    share = ref["taps"] / ref["value"]
    assert share.min() >= MIN_TAP_SHARE, f"a tap carries {share.min():.3f} of a sample's value: rescale lpips_ref.LIN_SCALE"


@pytest.mark.parametrize("size,resize", [(32, None), (16, 40)])
def test_torch_path_against_fp64(lp, size, resize):
    x, y = R.images(2, size)
    ref = R.lpips_ref(x, y, resize=resize, grad=True)
    _check_taps(ref)
    xg = x.clone().requires_grad_(True)
    v = lp(xg, y, resize=resize)
    assert v.shape == (2,) and v.dtype == torch.float32
    v.sum().backward()
    rel = ((v.double() - ref["value"]).abs() / ref["value"]).max().item()
    dx, want = xg.grad.double(), ref["dx"]
    cos = torch.nn.functional.cosine_similarity(dx.flatten(1), want.flatten(1)).min().item()
    nrm = (dx.flatten(1).norm(dim=1) / want.flatten(1).norm(dim=1) - 1).abs().max().item()
    print(f"lpips torch path {size}->{resize}: value rel {rel:.3e}, d x 1 - cos {1 - cos:.3e}, norm off {nrm:.3e}")
    assert rel <= RTOL
    assert cos >= GRAD_COS and nrm <= GRAD_NORM


def test_identical_images_give_zero(lp):
    x, _ = R.images(2, 16)
    assert torch.equal(lp(x, x.clone()), torch.zeros(2))


def test_one_pixel_tap_by_hand():
    # f^x = (0.6, 0.8), f^y = (0, 1), w = (2, 3): 2 * 0.36 + 3 * 0.04
    fx = torch.tensor([3.0, 4.0]).view(1, 2, 1, 1)
    fy = torch.tensor([0.0, 5.0]).view(1, 2, 1, 1)
    assert tap_distance(fx, fy, torch.tensor([2.0, 3.0])).item() == pytest.approx(0.84, rel=1e-6)
    # an all-zero pixel: the value is the other map's weighted unit vector, the gradient finite
    fz = torch.zeros(1, 2, 1, 1, requires_grad=True)
    v = tap_distance(fz, fy, torch.tensor([2.0, 3.0]))
    v.backward()
    assert v.item() == pytest.approx(3.0, rel=1e-6) and torch.isfinite(fz.grad).all()


def _toy(p, keep=None):
    def model(x, t, **kw):
        out = p.view(1, 3, 1, 1) * torch.tanh(x)
        if keep is not None:
            out.retain_grad()
            keep.append(out)
        return out
    return model


@pytest.mark.parametrize("resize_below", [256, 0])
def test_consistency_losses_lpips(lp, monkeypatch, resize_below):
    """CT (Euler step from x_start) with toy callables; 256: the resize branch, 0: the no-resize branch on a small image."""
    monkeypatch.setattr(kd, "LPIPS_RESIZE_BELOW", resize_below)
    N, size, S = (1, 16, 18) if resize_below else (2, 32, 18)
    g = torch.Generator().manual_seed(5)
    x0 = torch.rand(N, 3, size, size, generator=g) * 2 - 1
    noise = torch.randn(N, 3, size, size, generator=g)
    idx = torch.tensor([14, 11][:N])
    p = torch.tensor([0.9, 1.1, 0.7], requires_grad=True)
    q = torch.tensor([1.0, 0.8, 0.9])
    diff = KarrasDenoiser(distillation=True, loss_norm="lpips", lpips_loss=lp)
    keep = []
    loss = diff.consistency_losses(_toy(p, keep), x0, S, target_model=_toy(q), noise=noise, indices=idx)["loss"]
    loss.sum().backward()

    tab = cd_levels(S, diff.sigma_min, diff.sigma_max, diff.rho).table.double()
    t, t2 = tab[idx], tab[idx + 1]
    tt, tt2 = t.view(-1, 1, 1, 1), t2.view(-1, 1, 1, 1)
    x_t = x0.double() + noise.double() * tt
    x_t2 = x_t + (x_t - x0.double()) / tt * (tt2 - tt)
    c_in = lambda s: 1 / (s ** 2 + 0.25) ** 0.5
    th = torch.tanh(c_in(tt) * x_t)
    F_on = p.detach().double().view(1, 3, 1, 1) * th
    F_tg = q.double().view(1, 3, 1, 1) * torch.tanh(c_in(tt2) * x_t2)
    ref = R.cd_lpips_ref(F_on, F_tg, x_t, x_t2, t, t2, resize_below=resize_below, grad=True)
    rel = ((loss.detach().double() - ref["loss"]).abs() / ref["loss"]).max().item()
    dF, want = keep[0].grad.double().flatten(1), ref["dF"].flatten(1)
    cos = torch.nn.functional.cosine_similarity(dF, want).min().item()
    nrm = (dF.norm(dim=1) / want.norm(dim=1) - 1).abs().max().item()
    print(f"consistency_losses lpips (resize below {resize_below}): loss rel {rel:.3e}, d F 1 - cos {1 - cos:.3e}, norm off {nrm:.3e}")
    assert rel <= RTOL and cos >= GRAD_COS and nrm <= GRAD_NORM and torch.isfinite(p.grad).all()


def test_loading(tmp_path, monkeypatch):
    sd, lin = R.formula_weights()
    bare = {k[len("features."):]: v for k, v in sd.items()}
    bare["classifier.0.weight"] = torch.zeros(2, 2)          # extra keys are ignored
    x, y = R.images(1, 16)
    a = LPIPS(sd, lin)(x, y)
    assert torch.equal(LPIPS(bare, lin)(x, y), a)
    torch.save(bare, tmp_path / "vgg.pt")
    torch.save(list(lin), tmp_path / "lin.pt")               # piq's lpips_weights.pt: a list of five [1, C, 1, 1] tensors
    assert torch.equal(LPIPS.from_files(tmp_path / "vgg.pt", tmp_path / "lin.pt")(x, y), a)
    bad = dict(sd)
    bad["features.7.weight"] = torch.zeros(128, 64, 3, 3)
    with pytest.raises(ValueError, match="features.7"):
        LPIPS(bad, lin)
    with pytest.raises(ValueError):
        LPIPS(sd, lin[:4])
    with pytest.raises(ValueError):
        LPIPS(sd, [lin[0]] * 5)
    with pytest.raises(NotImplementedError):
        LPIPS(sd, lin, replace_pooling=False)
    monkeypatch.delenv("DXMI_LPIPS_VGG16", raising=False)
    monkeypatch.delenv("DXMI_LPIPS_LIN", raising=False)
    assert LPIPS.from_env() is None
    monkeypatch.setenv("DXMI_LPIPS_VGG16", str(tmp_path / "vgg.pt"))
    assert LPIPS.from_env() is None                          # one of the two is not enough
    with pytest.raises(NotImplementedError, match="DXMI_LPIPS_VGG16.*DXMI_LPIPS_LIN"):
        KarrasDenoiser(loss_norm="lpips")
    monkeypatch.setenv("DXMI_LPIPS_LIN", str(tmp_path / "lin.pt"))
    assert torch.equal(LPIPS.from_env()(x, y), a)
    assert torch.equal(KarrasDenoiser(loss_norm="lpips")._lpips()(x, y), a)
