"""The loop of the DDPM teacher's samplers (models/DxMI/ddpm_sample.py, models/DxMI/dpm_sample.py, models/DxMI/unipc_sample.py) and
of the EDM nets' multistep solvers (models/cm/dpm_sample.py, models/cm/unipc_sample.py), written once: per transition one network evaluation and one stage launch (csrc/stage_common.h),
as torch expressions on the CPU, eagerly on the device, or as ONE captured transition replayed for every row.

  sample          the dispatcher behind ddpm_sample / dpm_sample / edm_dpm_sample: checks, device resolution, eager or replay,
                  the graph cache
  replay_graphs   the StepGraphs a sampler holds for a network

The loop never asks which sampler it serves.  What differs lives on the schedule object (a _HostTable with steps, draws and
n_draws, one table row per transition):
  sampler                        the public function's name, for messages and the graph cache's key
  stage, FIRST, STEP             the launch (ops.ddpm_stage / ops.dpm_stage / ops.edm_dpm_stage) and its two modes
  T_COL                          the table column of the evaluation's time
  hist_slots                     the ring of earlier predictions the launch keeps: 0, 3 or 4 (fp32 [hist_slots, *shape], passed as
                                 hist=)
  transition(x, eps, z, row, hist)   one transition as torch expressions -> (x', pred_xstart); hist: the hist_slots - 1 predictions
                                 before this one, newest first, as far as the run has made them
  carry                          whether a second state is carried from transition to transition next to x: the launch then takes a
                                 static buffer of the state's shape as xc= (it writes it before it reads it), and the torch
                                 transition takes the carried value as a sixth argument (None on row 0) and returns it third
  graph_name(shape, mode)        the StepGraph's name
  x_in                           whether the network is evaluated on a second tensor the launch writes (the preconditioned input
                                 x_in, passed as x_in=) instead of on the state; FIRST then takes the state and x_in too
  initial(x, row), net_input(x, row)   the torch loop's share of that: the state FIRST leaves, and what the network is evaluated on
  net_keywords                   the model_kwargs the network takes (static buffers under replay); any other name is refused
  step_info(k)                   what the callback's dict says of row k besides i, x and pred_xstart
StageSchedule holds the DDPM teacher's answers to the last five, and carry = False.
"""
import weakref

import torch

from dxmi_hip import graph as _graph
from dxmi_hip._lib import DxmiError

from ..cm.karras_diffusion import _as_f32, _HostTable, _memo
from ..cm.random_util import DeterministicGenerator, DummyGenerator
from .ddpm_train import _hip_model


class StageSchedule(_HostTable):
    """A schedule of the loop with the answers of a sampler whose network reads the state itself and takes no keywords."""
    x_in, net_keywords, carry = False, (), False

    def initial(self, x, row):
        return x

    def net_input(self, x, row):
        return x

    def step_info(self, k):
        return {"t": self.tau[self.steps - 1 - k]}


def _progress(it, progress):
    if progress:
        try:
            from tqdm.auto import tqdm
            return tqdm(it)
        except ImportError:
            pass
    return it


def _evaluate(hip, net, x, t, kw):
    if hip is not None:
        return hip.forward_inference(x, t)
    eps = net(x, t, **kw)
    assert eps.shape == x.shape, f"network output {tuple(eps.shape)} != sample shape {tuple(x.shape)}"
    if eps.dtype != torch.float32 or not eps.is_contiguous() or eps.device != x.device:
        eps = _as_f32(eps, x.device)
    return eps


def _sample_torch(sch, net, shape, device, generator, noise, callback, progress, dtype, kw):
    """The transitions as torch expressions in `dtype`: the CPU path of the host tests, and what the GPU tests compare the launches
    with (a float64 network runs in float64 on the widened fp32 table)."""
    tab = sch.table.to(device=device, dtype=dtype)
    if noise is not None:
        x = noise[0].to(device=device, dtype=dtype).clone()
    elif generator is not None:
        x = generator.randn(*shape, device=device)
    else:
        x = torch.randn(shape, device=device)
    x = sch.initial(x, tab[0])
    hist, carried = [], None
    for k in _progress(range(sch.steps), progress):
        eps = net(sch.net_input(x, tab[k]), torch.full((shape[0],), float(tab[k, sch.T_COL]), device=device, dtype=dtype), **kw)
        z = None
        if sch.draws[k]:
            if noise is not None:
                z = noise[k + 1].to(device=device, dtype=dtype)
            else:
                z = generator.randn_like(x) if generator is not None else torch.randn_like(x)
        if sch.carry:
            x, pred, carried = sch.transition(x, eps, z, tab[k], hist, carried)
        else:
            x, pred = sch.transition(x, eps, z, tab[k], hist)
        hist = ([pred] + hist)[:max(sch.hist_slots - 1, 0)]
        if callback is not None:
            callback({"i": k, **sch.step_info(k), "x": x, "pred_xstart": pred})
    return x.clamp(-1, 1)


def _initial_state(x, shape, device, generator, noise):
    if noise is not None:
        x.copy_(noise[0])
    elif generator is not None:
        x.copy_(generator.randn(*shape, device=device))
    else:
        x.normal_()


def _buffers(sch, shape, device):
    """x, t, out and the keywords every transition's launch takes: out, hist where the sampler keeps one, x_in where the
    network is evaluated on it, and xc where a second state is carried."""
    f32 = dict(dtype=torch.float32, device=device)
    x, t, out = torch.empty(shape, **f32), torch.empty(shape[0], **f32), torch.empty(shape, **f32)
    kw = {"out": out}
    if sch.hist_slots:
        kw["hist"] = torch.empty((sch.hist_slots,) + shape, **f32)
    if sch.x_in:
        kw["x_in"] = torch.empty(shape, **f32)
    if sch.carry:
        kw["xc"] = torch.empty(shape, **f32)
    return x, t, out, kw


def _first(sch, tab, x, t, static):
    """The FIRST launch, and the tensor the network is evaluated on."""
    if sch.x_in:
        sch.stage(sch.FIRST, tab, t, row=0, x=x, x_in=static["x_in"])
        return static["x_in"]
    sch.stage(sch.FIRST, tab, t, row=0)
    return x


def _sample_eager(sch, hip, net, shape, device, generator, noise, callback, progress, net_kw):
    f32 = dict(dtype=torch.float32, device=device)
    tab = sch.device_table(device)
    x, t, out, static = _buffers(sch, shape, device)
    _initial_state(x, shape, device, generator, noise)
    fused = isinstance(generator, DeterministicGenerator)
    idx = generator.get_indices(shape[0], device) if fused and sch.n_draws else None
    zbuf = None
    x_net = _first(sch, tab, x, t, static)
    for k in _progress(range(sch.steps), progress):
        eps = _evaluate(hip, net, x_net, t, net_kw)
        kw = {}
        if sch.draws[k]:
            if noise is not None:
                kw["z"] = _as_f32(noise[k + 1], device)
            elif fused:       # the draw generator.randn_like(x) would make, made inside the launch
                kw.update(sample_index=idx, seed=generator.seed, draw=generator._next_draw())
            elif generator is not None:
                kw["z"] = _as_f32(generator.randn_like(x), device)
            else:
                zbuf = torch.empty(shape, **f32) if zbuf is None else zbuf
                kw["z"] = zbuf.normal_()
        pred = torch.empty(shape, **f32) if callback is not None else None
        sch.stage(sch.STEP, tab, t, row=k, x=x, eps=eps, pred_xstart=pred, **static, **kw)
        if callback is not None:
            callback({"i": k, **sch.step_info(k), "x": x.clone(), "pred_xstart": pred})
    return out


class _Replay:
    """ONE transition (network evaluation + stage launch) as a StepGraph, and the static buffers it runs on: x, t, out, the index
    vector and the history ring where the sampler keeps one.  The row, the draw number and the seed reach the captured launch
    through a host input, and the launch derives its history slots from the row, so the one captured step serves every row.  Holds
    the schedule: the captured launch reads its device table for as long as the graph lives."""

    def __init__(self, sch, hip, net, shape, device, mode, net_kw):
        self.sch, self.hip, self.net, self.mode = sch, hip, net, mode
        self.tab = sch.device_table(device)
        self.x, self.t, self.out, self.static = _buffers(sch, shape, device)
        self.x_net = self.static["x_in"] if sch.x_in else self.x
        self.net_kw = {k: torch.empty_like(v, device=device) for k, v in net_kw.items()}      # the labels: static buffers
        self.z = torch.empty(shape, dtype=torch.float32, device=device) if mode == "torch" else None
        self.idx = torch.zeros(shape[0], dtype=torch.int64, device=device) if mode == "fused" else None
        self.row = self.draw = self.seed = 0
        self.graph = _graph.StepGraph(self._step, device, modules=_graph.pack_modules(hip if hip is not None else net),
                                      name=sch.graph_name(shape, mode))

    def _control(self):
        return [self.row, self.draw & 0xFFFFFFFF, self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF]

    def _step(self):
        eps = _evaluate(self.hip, self.net, self.x_net, self.t, self.net_kw)
        kw = {}
        if self.mode == "torch":      # drawn in every transition: the captured step is the same for all rows (the last row's is unused)
            kw["z"] = self.z.normal_()
        elif self.mode == "fused":
            kw["sample_index"] = self.idx
        g = _graph.current()
        if g is not None:
            kw["ctl"] = g.host_input(torch.int32, 4, self._control)
        else:
            kw.update(row=self.row, draw=self.draw, seed=self.seed)
        self.sch.stage(self.sch.STEP, self.tab, self.t, x=self.x, eps=eps, **self.static, **kw)

    def run(self, shape, device, generator, net_kw):
        sch = self.sch
        _initial_state(self.x, shape, device, generator, None)       # None, or a deterministic generator (also when no row draws)
        for k, v in net_kw.items():
            self.net_kw[k].copy_(v)
        if self.mode == "fused":
            self.idx.copy_(generator.get_indices(shape[0], device))
            self.seed = int(generator.seed)
        _first(sch, self.tab, self.x, self.t, self.static)
        for k in range(sch.steps):
            self.row = k
            if self.mode == "fused" and sch.draws[k]:
                self.draw = generator._next_draw()
            self.graph()
        return self.out


_GRAPHS = weakref.WeakKeyDictionary()       # network -> {graph key: _Replay}


def replay_graphs(net, sampler):
    """The StepGraphs `sampler` ("ddpm_sample" / "dpm_sample") holds for `net` (their .captures / .replays count what ran)."""
    try:
        return [r.graph for key, r in _GRAPHS.get(net, {}).items() if key[0] == sampler]
    except TypeError:
        return []


def sample(sch, net, shape, device, generator, noise, callback, progress, use_graph, float64_state, model_kwargs=None):
    """The body of ddpm_sample / dpm_sample / edm_dpm_sample on the schedule `sch` (their docstrings are the contract).
    float64_state: whether the torch loop's state takes float64 from a float64 noise[0]; it is fp32 otherwise.  model_kwargs: the
    keywords of the network, of sch.net_keywords; under replay they are tensors, copied into static buffers."""
    shape = tuple(int(s) for s in shape)
    net_kw = dict(model_kwargs or {})
    extra = set(net_kw) - set(sch.net_keywords)
    if extra:
        raise ValueError(f"{sch.sampler}: model_kwargs {sorted(extra)} are not inputs of its network (it takes {sch.net_keywords})")
    if noise is not None and len(noise) != sch.steps + 1:
        raise ValueError(f"{sch.sampler}: noise must hold {sch.steps + 1} draws (x_T and one per transition), got {len(noise)}")
    hip = _hip_model(net)
    if isinstance(generator, DummyGenerator):       # it forwards to torch: the same draws as no generator
        generator = None
    device = _graph.indexed_device(torch.device("cuda") if device is None else device)
    with torch.no_grad():
        if device.type != "cuda":
            if hip is not None:
                raise DxmiError(f"{sch.sampler}: the HIP Model runs only on the device (a CPU device takes a torch callable)")
            wide = float64_state and noise is not None and noise[0].dtype == torch.float64
            dtype = torch.float64 if wide else torch.float32
            return _sample_torch(sch, net, shape, device, generator, noise, callback, progress, dtype, net_kw)
        replayable = generator is None or isinstance(generator, DeterministicGenerator)
        static_kw = all(torch.is_tensor(v) for v in net_kw.values())
        if not (use_graph and callback is None and not progress and noise is None and replayable and static_kw
                and not _graph.capturing()):
            return _sample_eager(sch, hip, net, shape, device, generator, noise, callback, progress, net_kw)
        mode = "none" if not sch.n_draws else ("fused" if isinstance(generator, DeterministicGenerator) else "torch")
        try:
            graphs = _GRAPHS.setdefault(hip if hip is not None else net, {})
        except TypeError:        # not weak-referenceable: no cache, so no replay
            return _sample_eager(sch, hip, net, shape, device, generator, noise, callback, progress, net_kw)
        # what a capture freezes: the sampler and the network (the dictionary's key), the shape and the device, the table and where
        # z comes from.  pred_xstart is never written under replay: it is the callback's
        key = (sch.sampler, id(sch), shape, device.index, mode) + tuple((k, v.dtype, tuple(v.shape)) for k, v in sorted(net_kw.items()))
        rp = _memo(graphs, key, 8, lambda: _Replay(sch, hip, net, shape, device, mode, net_kw))
        return rp.run(shape, device, generator, net_kw)
