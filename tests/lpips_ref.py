"""Shared by test_lpips_host.py and test_hip_lpips.py: seeded formula weights for VGG16 + the LPIPS linear layers, and an fp64
restatement of LPIPS (piq's LPIPS(replace_pooling=True, reduction="none")) and of the lpips branch of consistency_losses
(reference models/cm/karras_diffusion.py:221-234), written from the definition and independent of models/cm/lpips.py.

`storage=True` is the bf16 storage model of the device path: conv weights rounded to bf16, and every activation and every gradient
rounded to bf16 where the device stores one (the front end's output, every conv + ReLU output, every pool output; the gradient the
tap distance writes, the masked accumulate's output, every data-gradient conv's output, every pool backward's output)."""
import functools

import torch
import torch.nn.functional as F

CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_BEFORE = (5, 10, 17, 24)            # conv indices that follow an AvgPool2d(2, 2, 0)
TAP_AFTER = (2, 7, 14, 21, 28)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# per-tap scale of the formula linear weights, set so that every tap carries at least 5 % of every sample's value on the test
# images (checked by the tests that use them): with random VGG weights the deep taps of x and y differ less than the shallow ones
LIN_SCALE = (1.5, 2.0, 6.0, 30.0, 100.0)


def bf16r(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class _Store(torch.autograd.Function):
    """A bf16 store: the value is rounded on the way forward (fwd) and the gradient on the way back (bwd)."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return bf16r(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (bf16r(g) if ctx.bwd else g), None, None


@functools.lru_cache(maxsize=None)
def formula_weights(seed=0):
    """(vgg state dict with torchvision's key names, piq-style list of five [1, C, 1, 1] tensors), fp32, seeded."""
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for idx, cout in zip(CONV_INDICES, WIDTHS):
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5      # He
        sd[f"features.{idx}.bias"] = 0.05 * torch.randn(cout, generator=g)
        cin = cout
    lin = [(0.1 + torch.rand(1, WIDTHS[CONV_INDICES.index(i)], 1, 1, generator=g)) * s for i, s in zip(TAP_AFTER, LIN_SCALE)]
    return sd, lin


def images(N, size, seed=0):
    """x uniform in [0, 1], y = clamp(x + 0.25 randn, 0, 1)."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(N, 3, size, size, generator=g)
    y = (x + 0.25 * torch.randn(N, 3, size, size, generator=g)).clamp(0, 1)
    return x, y


def _features(x, sd, storage):
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    h = _Store.apply((x - mean) / std, storage, storage)
    taps = []
    for idx in CONV_INDICES:
        if idx in POOL_BEFORE:
            h = _Store.apply(F.avg_pool2d(_Store.apply(h, False, storage), 2, 2, 0), storage, False)
        w = sd[f"features.{idx}.weight"].double()
        w = bf16r(w) if storage else w
        h = F.relu(F.conv2d(_Store.apply(h, False, storage), w, sd[f"features.{idx}.bias"].double(), padding=1))
        h = _Store.apply(h, storage, storage)
        if idx in TAP_AFTER:
            taps.append(_Store.apply(h, False, storage))
    return taps


def tap_distance(fx, fy, w):
    """fp64 [N, C, h, w] features, w [C] -> [N]; the norm's derivative at an all-zero pixel is taken as 0."""
    nx = torch.linalg.vector_norm(fx, dim=1, keepdim=True)
    ny = torch.linalg.vector_norm(fy, dim=1, keepdim=True)
    d = (fx / (nx + 1e-10) - fy / (ny + 1e-10)) ** 2 * w.double().view(1, -1, 1, 1)
    return d.mean(dim=(2, 3)).sum(dim=1)


def lpips_ref(x, y, weights=None, resize=None, storage=False, grad=False):
    """-> dict(value [N], taps [5, N], dx [N, 3, H, W] or None), fp64."""
    sd, lin = weights if weights is not None else formula_weights()
    x = x.detach().double().requires_grad_(grad)
    y = y.detach().double()
    xi, yi = x, y
    if resize is not None:
        xi = F.interpolate(x, size=resize, mode="bilinear")
        yi = F.interpolate(y, size=resize, mode="bilinear")
    with torch.no_grad():
        fy = _features(yi, sd, storage)
    fx = _features(xi, sd, storage)
    taps = torch.stack([tap_distance(a, b, w.reshape(-1)) for a, b, w in zip(fx, fy, lin)])
    value = taps.sum(0)
    dx = None
    if grad:
        # per-sample gradients in one pass: sample n's value depends on x[n] only
        dx, = torch.autograd.grad(value.sum(), x)
    return {"value": value.detach(), "taps": taps.detach(), "dx": dx}


def cd_scalings(t, sigma_data=0.5, sigma_min=0.002):
    """get_scalings_for_boundary_condition in fp64 -> (c_skip, c_out), each [N, 1, 1, 1]."""
    t = t.double().view(-1, 1, 1, 1)
    c_skip = sigma_data ** 2 / ((t - sigma_min) ** 2 + sigma_data ** 2)
    c_out = (t - sigma_min) * sigma_data / (t ** 2 + sigma_data ** 2) ** 0.5
    return c_skip, c_out


def cd_lpips_ref(F_on, F_tg, x_t, x_t2, t, t2, weights=None, sigma_data=0.5, sigma_min=0.002, resize_below=256, storage=False,
                 grad=False):
    """The lpips branch of consistency_losses (reference :221-234) in fp64 from the two network outputs, with the karras
    weighting snr + 1 / sigma_data^2 -> dict(loss [N], dF [N, 3, H, W] or None: the gradient of sum(loss) into F_on)."""
    cs, co = cd_scalings(t, sigma_data, sigma_min)
    cs2, co2 = cd_scalings(t2, sigma_data, sigma_min)
    Fo = F_on.detach().double().requires_grad_(grad)
    dist = co * Fo + cs * x_t.double()
    targ = co2 * F_tg.double() + cs2 * x_t2.double()
    resize = 224 if F_on.shape[-1] < resize_below else None
    x01 = (dist + 1) / 2.0
    r = lpips_ref(x01, (targ + 1) / 2.0, weights, resize=resize, storage=storage, grad=grad)
    w = t.double() ** -2 + 1.0 / sigma_data ** 2
    dF = None
    if grad:      # chain rule by hand: loss_n = w_n lpips_n(x01_n), x01 = (c_out F + c_skip x_t + 1) / 2
        dF = r["dx"] * (w.view(-1, 1, 1, 1) * 0.5 * co)
    return {"loss": r["value"] * w, "dF": dF}
