"""EDM preconditioning and the Karras samplers of the EDM teacher (`models.cm.karras_diffusion`).

Reference: models/cm/karras_diffusion.py — KarrasDenoiser.__init__/get_snr/get_scalings (:33-68),
denoise (:337-351), karras_sample (:354-420), get_sigmas_karras (:423-429), get_ancestral_step (:437-444),
sample_euler_ancestral / sample_heun / sample_euler / sample_dpm (:447-640).  The consistency-distillation
losses and samplers (onestep, multistep, progdist) and the inpainting / super-resolution paths stay out of scope.

denoise() keeps the reference signature for any callable `model`; neither sampler calls it on the hot path.
OpenAIDiffusion (the DxMI few-step sampler) uses the fused dxmi_edm_precond / dxmi_edm_step_fwd kernels.
karras_sample builds its schedule ONCE on the host, in fp32 torch with the reference's expressions (tables
bit-identical to the reference's), uploads it as one small device table, and runs ONE dxmi_karras_stage launch
between two network evaluations (denoised, clamp, d, the Heun / DPM-2 / Euler / ancestral update, the next step's
churn and the next preconditioned input; the clamped sample after the last evaluation).
"""
import math
import weakref

import torch

from .nn import append_dims, append_zero


class KarrasDenoiser:
    def __init__(self, sigma_data: float = 0.5, sigma_max=80.0, sigma_min=0.002, rho=7.0, weight_schedule="karras",
                 distillation=False, loss_norm="l2"):
        self.sigma_data, self.sigma_max, self.sigma_min = sigma_data, sigma_max, sigma_min
        self.weight_schedule, self.distillation, self.loss_norm, self.rho = weight_schedule, distillation, loss_norm, rho
        if loss_norm == "lpips":
            raise NotImplementedError("LPIPS loss belongs to consistency distillation, not to the DxMI path")

    def get_snr(self, sigmas):
        return sigmas ** -2

    def get_sigmas(self, sigmas):
        return sigmas

    def get_scalings(self, sigma):
        c_skip = self.sigma_data ** 2 / (sigma ** 2 + self.sigma_data ** 2)
        c_out = sigma * self.sigma_data / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        c_in = 1 / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        return c_skip, c_out, c_in

    def get_scalings_for_boundary_condition(self, sigma):
        c_skip = self.sigma_data ** 2 / ((sigma - self.sigma_min) ** 2 + self.sigma_data ** 2)
        c_out = (sigma - self.sigma_min) * self.sigma_data / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        c_in = 1 / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        return c_skip, c_out, c_in

    def denoise(self, model, x_t, sigmas, **model_kwargs):
        scal = self.get_scalings_for_boundary_condition(sigmas) if self.distillation else self.get_scalings(sigmas)
        c_skip, c_out, c_in = [append_dims(s, x_t.ndim) for s in scal]
        rescaled_t = 1000 * 0.25 * torch.log(sigmas + 1e-44)
        model_output = model(c_in * x_t, rescaled_t, **model_kwargs)
        return model_output, c_out * model_output + c_skip * x_t


def get_sigmas_karras(n, sigma_min, sigma_max, rho=7.0, device="cpu"):
    ramp = torch.linspace(0, 1, n)
    min_inv_rho = sigma_min ** (1 / rho)
    max_inv_rho = sigma_max ** (1 / rho)
    sigmas = (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho
    return append_zero(sigmas).to(device)


def get_ancestral_step(sigma_from, sigma_to):
    sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


# ------------------------------------------------------------------------------------------------------------- Karras samplers
KARRAS_SAMPLERS = ("heun", "dpm", "euler", "ancestral")
_DISTILLED_SAMPLERS = ("onestep", "multistep", "progdist")
_GRAPHS = weakref.WeakKeyDictionary()       # model -> {graph key: StepGraph}
_SCHEDULES = {}


class KarrasDenoiserFn:
    """The reference's `denoiser(x_t, sigma)` closure of karras_sample (:404-410), as data: the device samplers fuse its
    arithmetic (scalings, clip) into their stage kernels and call only `model(c_in x, 250 ln(sigma + 1e-44), **model_kwargs)`."""

    def __init__(self, diffusion, model, clip_denoised=True, model_kwargs=None):
        if getattr(diffusion, "distillation", False):
            raise NotImplementedError("karras_sample on the device supports distillation=False only: the boundary-condition "
                                      "scalings belong to consistency-distilled models, which no config here builds")
        self.diffusion, self.model = diffusion, model
        self.clip_denoised, self.model_kwargs = bool(clip_denoised), dict(model_kwargs or {})

    def __call__(self, *a, **k):
        raise TypeError("KarrasDenoiserFn is not called directly: pass it to sample_heun / sample_dpm / sample_euler / "
                        "sample_euler_ancestral, which fuse its arithmetic into dxmi_karras_stage")


class KarrasSchedule:
    """Host schedule of one sampler over a sigma ladder, in fp32 torch with the reference's expressions (:447-640).

    Per step i: gamma (python float, as the reference), sigma_hat, churn = (sigma_hat^2 - sigma^2)^0.5, and per sampler the
    step sizes (dt; dpm: sigma_mid, dt_1, dt_2; ancestral: sigma_down, sigma_up).  `launches` is the launch sequence of
    dxmi_karras_stage: launch 0 (FIRST) precedes evaluation 1 and launch k follows evaluation k; `table` holds one row per launch
    (include/dxmi_hip.h, DXMI_KT_*)."""

    def __init__(self, sigmas, sampler, diffusion, clip_denoised=True, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0,
                 x_scale=1.0):
        from dxmi_hip import ops
        if sampler not in KARRAS_SAMPLERS:
            raise ValueError(f"unknown Karras sampler {sampler!r}; the device path runs {KARRAS_SAMPLERS}")
        sigmas = sigmas.detach().to("cpu", torch.float32)
        self.sampler, self.sigmas, self.sigma_data = sampler, sigmas, diffusion.sigma_data
        n = len(sigmas) - 1
        self.steps = n
        churned = sampler in ("heun", "dpm")
        self.gamma, sh, churn, dt, mid, dt2, down, up = [], [], [], [], [], [], [], []
        for i in range(n):
            gamma = (min(s_churn / (len(sigmas) - 1), 2 ** 0.5 - 1) if s_tmin <= sigmas[i] <= s_tmax else 0.0) if churned else 0.0
            sigma_hat = sigmas[i] * (gamma + 1)
            self.gamma.append(gamma)
            sh.append(sigma_hat)
            churn.append((sigma_hat ** 2 - sigmas[i] ** 2) ** 0.5)
            if sampler == "dpm":
                sigma_mid = ((sigma_hat ** (1 / 3) + sigmas[i + 1] ** (1 / 3)) / 2) ** 3
                mid.append(sigma_mid)
                dt.append(sigma_mid - sigma_hat)
                dt2.append(sigmas[i + 1] - sigma_hat)
            elif sampler == "ancestral":
                sigma_down, sigma_up = get_ancestral_step(sigmas[i], sigmas[i + 1])
                down.append(sigma_down)
                up.append(sigma_up)
                dt.append(sigma_down - sigmas[i])
            else:
                dt.append(sigmas[i + 1] - sigma_hat)
        st = lambda v: torch.stack(v) if v else None
        self.sigma_hat, self.churn, self.dt = st(sh), st(churn), st(dt)
        self.sigma_mid, self.dt_2, self.sigma_down, self.sigma_up = st(mid), st(dt2), st(down), st(up)

        z = torch.zeros((), dtype=torch.float32)
        L = []      # (mode, last, eval sigma, dt, sigma_up, next eval sigma, churn step, draw, callback step)

        def corr_tail(i):
            return dict(last=i == n - 1, nxt=None if i == n - 1 else sh[i + 1], churn_step=None if i == n - 1 else i + 1,
                        draw=None if i == n - 1 or not churned else ("eps", i + 1))
        L.append(dict(mode=ops.KARRAS_FIRST, last=False, sig=None, dt=z, up=z, nxt=sh[0], churn_step=0 if churned else None,
                      draw=("eps", 0) if churned else None, cb=None))
        for i in range(n):
            if sampler == "heun" and sigmas[i + 1] != 0:
                L.append(dict(mode=ops.KARRAS_PRED, last=False, sig=sh[i], dt=dt[i], up=z, nxt=sigmas[i + 1], churn_step=None,
                              draw=None, cb=i))
                L.append(dict(mode=ops.KARRAS_HEUN_CORR, sig=sigmas[i + 1], dt=dt[i], up=z, cb=None, **corr_tail(i)))
            elif sampler == "dpm":
                L.append(dict(mode=ops.KARRAS_PRED, last=False, sig=sh[i], dt=dt[i], up=z, nxt=mid[i], churn_step=None, draw=None,
                              cb=i))
                L.append(dict(mode=ops.KARRAS_DPM_CORR, sig=mid[i], dt=dt2[i], up=z, cb=None, **corr_tail(i)))
            elif sampler == "ancestral":
                L.append(dict(mode=ops.KARRAS_ANCESTRAL, last=i == n - 1, sig=sigmas[i], dt=dt[i], up=up[i],
                              nxt=None if i == n - 1 else sigmas[i + 1], churn_step=None, draw=("z", i), cb=i))
            else:   # euler, and heun's last step (sigma_{i+1} = 0: Euler, :537-539)
                L.append(dict(mode=ops.KARRAS_EULER, last=i == n - 1, sig=sh[i], dt=dt[i], up=z,
                              nxt=None if i == n - 1 else sigmas[i + 1], churn_step=None, draw=None, cb=i))
        self.launches = L
        self.nfe = len(L) - 1
        self.eval_sigmas = torch.stack([l["nxt"] for l in L if l["nxt"] is not None])      # noise level of every evaluation

        tab = torch.zeros((len(L), ops.KT_COLS), dtype=torch.float32)
        for k, l in enumerate(L):
            if l["sig"] is not None:
                c_skip, c_out, _ = diffusion.get_scalings(l["sig"].reshape(1))
                tab[k, ops.KT_SIGMA], tab[k, ops.KT_CSKIP], tab[k, ops.KT_COUT] = l["sig"], c_skip[0], c_out[0]
            tab[k, ops.KT_DT], tab[k, ops.KT_SIGMA_UP] = l["dt"], l["up"]
            if l["churn_step"] is not None:
                tab[k, ops.KT_CHURN] = churn[l["churn_step"]]
            tab[k, ops.KT_SNOISE] = s_noise
            if l["nxt"] is not None:
                s = l["nxt"].reshape(1)
                tab[k, ops.KT_CIN] = diffusion.get_scalings(s)[2][0]
                tab[k, ops.KT_T] = (1000 * 0.25 * torch.log(s + 1e-44))[0]      # denoise() (:348)
            tab[k, ops.KT_XSCALE] = x_scale
            tab[k, ops.KT_CLIP] = 1.0 if clip_denoised else 0.0
        self.table = tab
        self._dev = {}

    def device_table(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.table.to(device)
        return self._dev[key]


def _schedule(sigmas, sampler, denoiser, x_scale, s_churn, s_tmin, s_tmax, s_noise):
    key = (sampler, tuple(sigmas.detach().cpu().float().tolist()), float(denoiser.diffusion.sigma_data), denoiser.clip_denoised,
           float(s_churn), float(s_tmin), float(s_tmax), float(s_noise), float(x_scale))
    sch = _SCHEDULES.get(key)
    if sch is None:
        if len(_SCHEDULES) > 64:
            _SCHEDULES.clear()
        sch = _SCHEDULES[key] = KarrasSchedule(sigmas, sampler, denoiser.diffusion, denoiser.clip_denoised, s_churn, s_tmin,
                                               s_tmax, s_noise, x_scale)
    return sch


def _as_f32(v, device):
    v = v.to(device=device, dtype=torch.float32)
    return v if v.is_contiguous() else v.contiguous()


def _run(sch, denoiser, x0, shape, device, generator, callback=None, progress=False):
    """The launch sequence of `sch`: FIRST, then per network evaluation one dxmi_karras_stage launch.  x0: the initial state
    (scaled by the table's XSCALE), or None to draw it (generator.randn, else on the device).  -> the clamped sample (a new
    tensor, static under graph capture)."""
    from dxmi_hip import ops
    f32 = dict(dtype=torch.float32, device=device)
    tab = sch.device_table(device)
    x = torch.empty(shape, **f32)
    if x0 is not None:
        x.copy_(x0)
    elif generator is not None:
        x.copy_(generator.randn(*shape, device=device))
    else:
        x.normal_()
    two = sch.sampler in ("heun", "dpm")
    x2, d = (torch.empty(shape, **f32), torch.empty(shape, **f32)) if two else (None, None)
    x_in, t, out = torch.empty(shape, **f32), torch.empty(shape[0], **f32), torch.empty(shape, **f32)
    noise_buf = None
    model, kw = denoiser.model, denoiser.model_kwargs
    launches = range(len(sch.launches))
    if progress:
        try:
            from tqdm.auto import tqdm
            launches = tqdm(launches)
        except ImportError:
            pass
    F = None
    for k in launches:
        l = sch.launches[k]
        if k > 0:
            F = model(x_in, t, **kw)
            if F.dtype != torch.float32 or not F.is_contiguous() or F.device != x.device:
                F = _as_f32(F, device)
            assert F.shape == x.shape, f"model output {tuple(F.shape)} != sample shape {tuple(x.shape)}"
        noise = None
        if l["draw"] is not None:
            kind, i = l["draw"]
            used = sch.gamma[i] > 0 if kind == "eps" else float(sch.sigma_up[i]) != 0.0
            if generator is not None:     # the reference's draws, in its order and number (:522, :603, :477)
                draw = generator.randn_like(x)
                noise = _as_f32(draw, device) if used else None
            elif used:
                if noise_buf is None:
                    noise_buf = torch.empty(shape, **f32)
                noise = noise_buf.normal_()
        den, cb_x = None, None
        if callback is not None and l["cb"] is not None:
            den, cb_x = torch.empty(shape, **f32), x.clone()
        ops.karras_stage(l["mode"], l["last"], tab, k, x, x2=x2, d=d, model_out=F, noise=noise, x_in=None if l["last"] else x_in,
                         t=None if l["last"] else t, out=out if l["last"] else None, denoised=den)
        if den is not None:
            i = l["cb"]
            info = {"x": cb_x, "i": i, "sigma": sch.sigmas[i], "sigma_hat": sch.sigma_hat[i], "denoised": den}
            if sch.sampler == "euler":
                del info["sigma_hat"]          # the reference's euler callback has none (:566-574)
            callback(info)
    return out


def _check_sampler_args(denoiser, x):
    if not isinstance(denoiser, KarrasDenoiserFn):
        raise TypeError("the device Karras samplers take a KarrasDenoiserFn (diffusion, model, clip_denoised, model_kwargs): "
                        "they fuse the denoiser's arithmetic into dxmi_karras_stage")
    if not x.is_cuda:
        from dxmi_hip._lib import DxmiError
        raise DxmiError("the Karras samplers run only on the HIP device path (no CPU fallback)")


@torch.no_grad()
def sample_euler_ancestral(model, x, sigmas, generator, progress=False, callback=None):
    """Ancestral sampling with Euler steps (reference :447-478).  model: a KarrasDenoiserFn; x: the initial state."""
    _check_sampler_args(model, x)
    sch = _schedule(sigmas, "ancestral", model, 1.0, 0.0, 0.0, float("inf"), 1.0)
    return _run(sch, model, x, tuple(x.shape), x.device, generator, callback, progress)


@torch.no_grad()
def sample_heun(denoiser, x, sigmas, generator, progress=False, callback=None, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"),
                s_noise=1.0):
    """Algorithm 2 (Heun steps) of Karras et al. (2022) (reference :499-547).  NFE = 2 * steps - 1 (the last step is Euler)."""
    _check_sampler_args(denoiser, x)
    sch = _schedule(sigmas, "heun", denoiser, 1.0, s_churn, s_tmin, s_tmax, s_noise)
    return _run(sch, denoiser, x, tuple(x.shape), x.device, generator, callback, progress)


@torch.no_grad()
def sample_euler(denoiser, x, sigmas, generator, progress=False, callback=None):
    """Euler steps (reference :550-578).  NFE = steps."""
    _check_sampler_args(denoiser, x)
    sch = _schedule(sigmas, "euler", denoiser, 1.0, 0.0, 0.0, float("inf"), 1.0)
    return _run(sch, denoiser, x, tuple(x.shape), x.device, generator, callback, progress)


@torch.no_grad()
def sample_dpm(denoiser, x, sigmas, generator, progress=False, callback=None, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"),
               s_noise=1.0):
    """DPM-Solver-2-like midpoint steps, midpoint on a rho=3 Karras ladder (reference :581-621).  NFE = 2 * steps."""
    _check_sampler_args(denoiser, x)
    sch = _schedule(sigmas, "dpm", denoiser, 1.0, s_churn, s_tmin, s_tmax, s_noise)
    return _run(sch, denoiser, x, tuple(x.shape), x.device, generator, callback, progress)


def karras_nfe(sampler, steps):
    """Network evaluations per image: heun 2 steps - 1, dpm 2 steps, euler / ancestral steps."""
    return {"heun": 2 * steps - 1, "dpm": 2 * steps, "euler": steps, "ancestral": steps}[sampler]


def karras_sample(diffusion, model, shape, steps, clip_denoised=True, progress=False, callback=None, model_kwargs=None,
                  device=None, sigma_min=0.002, sigma_max=80, rho=7.0, sampler="heun", s_churn=0.0, s_tmin=0.0,
                  s_tmax=float("inf"), s_noise=1.0, generator=None, ts=None, use_graph=False):
    """Sample the EDM teacher with a Karras sampler on the device (reference :354-420); returns clamp(x_0, -1, 1).

    model: any callable model(x_in, t, **model_kwargs) -> [B, C, H, W] (the HIP UNetModel, or a torch function).
    RNG: with generator=None every draw is made on the device and draws whose result is unused are skipped (eps when
    gamma = 0, the last ancestral z, whose sigma_up is 0), so the stream differs from the reference's.  With a generator its
    randn / randn_like are called in the reference's order and number (x_T, one eps per heun / dpm step even at gamma = 0, one z
    per ancestral step): a generator that replays recorded draws reproduces the reference's trajectory.
    use_graph: replay the whole loop of a key (sampler, steps, sigma and churn settings, shape, device, labels given) as one
    hipGraph: the first call of a key runs eagerly, the second is captured.  The returned tensor is then STATIC: the next call
    of the same key overwrites it.  Off with callback, progress or a generator, and for model_kwargs other than `y`."""
    if sampler in _DISTILLED_SAMPLERS:
        raise NotImplementedError(f"sampler {sampler!r} needs a consistency-distilled model (`ts`, boundary-condition scalings), "
                                  "which no config here builds; the device path runs heun, dpm, euler and ancestral")
    if sampler not in KARRAS_SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r}")
    denoiser = KarrasDenoiserFn(diffusion, model, clip_denoised, model_kwargs)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        from dxmi_hip._lib import DxmiError
        raise DxmiError("karras_sample runs only on the HIP device path (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    shape = tuple(int(s) for s in shape)
    sigmas = get_sigmas_karras(steps, sigma_min, sigma_max, rho, device="cpu")
    churned = sampler in ("heun", "dpm")
    sch = _schedule(sigmas, sampler, denoiser, sigma_max, s_churn if churned else 0.0, s_tmin if churned else 0.0,
                    s_tmax if churned else float("inf"), s_noise if churned else 1.0)
    from dxmi_hip import graph as _graph
    kw = denoiser.model_kwargs
    if use_graph and callback is None and not progress and generator is None and set(kw) <= {"y"} \
            and not _graph.capturing():
        key = (sampler, steps, float(sigma_min), float(sigma_max), float(rho), float(s_churn), float(s_tmin), float(s_tmax),
               float(s_noise), bool(clip_denoised), float(diffusion.sigma_data), shape, device.index, "y" in kw)
        try:
            graphs = _GRAPHS.setdefault(model, {})
        except TypeError:        # not weak-referenceable: no cache, so no replay
            graphs = {}
        g = graphs.get(key)
        if g is None:
            from models.DxMI.trainer import _pack_modules
            if "y" in kw:
                fn = lambda y: _run(sch, KarrasDenoiserFn(diffusion, model, clip_denoised, {"y": y}), None, shape, device, None)
            else:
                fn = lambda: _run(sch, denoiser, None, shape, device, None)
            g = graphs[key] = _graph.StepGraph(fn, device, modules=_pack_modules(model), name=f"karras_sample{key}")
        with torch.no_grad():
            return g(kw["y"]) if "y" in kw else g()
    with torch.no_grad():
        return _run(sch, denoiser, None, shape, device, generator, callback, progress)
