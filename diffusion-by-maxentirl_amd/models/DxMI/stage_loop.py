"""The loop of the DDPM teacher's samplers (models/DxMI/ddpm_sample.py, models/DxMI/dpm_sample.py), written once: per transition
one network evaluation and one stage launch (csrc/stage_common.h), as torch expressions on the CPU, eagerly on the device, or as
ONE captured transition replayed for every row.

  sample          the dispatcher behind ddpm_sample / dpm_sample: checks, device resolution, eager or replay, the graph cache
  replay_graphs   the StepGraphs a sampler holds for a network

The loop never asks which sampler it serves.  What differs lives on the schedule object (a _HostTable with tau, steps, draws and
n_draws, one table row per transition):
  sampler                        the public function's name, for messages and the graph cache's key
  stage, FIRST, STEP             the launch (ops.ddpm_stage / ops.dpm_stage) and its two modes
  T_COL                          the table column of the evaluation's time
  hist_slots                     the ring of earlier predictions the launch keeps: 0, or 3 (fp32 [3, *shape], passed as hist=)
  transition(x, eps, z, row, hist)   one transition as torch expressions -> (x', pred_xstart); hist: the hist_slots - 1 predictions
                                 before this one, newest first, as far as the run has made them
  graph_name(shape, mode)        the StepGraph's name
"""
import weakref

import torch

from dxmi_hip import graph as _graph
from dxmi_hip._lib import DxmiError

from ..cm.karras_diffusion import _as_f32, _memo
from ..cm.random_util import DeterministicGenerator, DummyGenerator
from .ddpm_train import _hip_model


def _progress(it, progress):
    if progress:
        try:
            from tqdm.auto import tqdm
            return tqdm(it)
        except ImportError:
            pass
    return it


def _evaluate(hip, net, x, t):
    if hip is not None:
        return hip.forward_inference(x, t)
    eps = net(x, t)
    assert eps.shape == x.shape, f"network output {tuple(eps.shape)} != sample shape {tuple(x.shape)}"
    if eps.dtype != torch.float32 or not eps.is_contiguous() or eps.device != x.device:
        eps = _as_f32(eps, x.device)
    return eps


def _sample_torch(sch, net, shape, device, generator, noise, callback, progress, dtype):
    """The transitions as torch expressions in `dtype`: the CPU path of the host tests, and what the GPU tests compare the launches
    with (a float64 network runs in float64 on the widened fp32 table)."""
    tab = sch.table.to(device=device, dtype=dtype)
    if noise is not None:
        x = noise[0].to(device=device, dtype=dtype).clone()
    elif generator is not None:
        x = generator.randn(*shape, device=device)
    else:
        x = torch.randn(shape, device=device)
    hist = []
    for k in _progress(range(sch.steps), progress):
        eps = net(x, torch.full((shape[0],), float(tab[k, sch.T_COL]), device=device, dtype=dtype))
        z = None
        if sch.draws[k]:
            if noise is not None:
                z = noise[k + 1].to(device=device, dtype=dtype)
            else:
                z = generator.randn_like(x) if generator is not None else torch.randn_like(x)
        x, pred = sch.transition(x, eps, z, tab[k], hist)
        hist = ([pred] + hist)[:max(sch.hist_slots - 1, 0)]
        if callback is not None:
            callback({"i": k, "t": sch.tau[sch.steps - 1 - k], "x": x, "pred_xstart": pred})
    return x.clamp(-1, 1)


def _initial_state(x, shape, device, generator, noise):
    if noise is not None:
        x.copy_(noise[0])
    elif generator is not None:
        x.copy_(generator.randn(*shape, device=device))
    else:
        x.normal_()


def _buffers(sch, shape, device):
    """x, t, out and the keywords every transition's launch takes: out, and hist where the sampler keeps one."""
    f32 = dict(dtype=torch.float32, device=device)
    x, t, out = torch.empty(shape, **f32), torch.empty(shape[0], **f32), torch.empty(shape, **f32)
    kw = {"out": out}
    if sch.hist_slots:
        kw["hist"] = torch.empty((sch.hist_slots,) + shape, **f32)
    return x, t, out, kw


def _sample_eager(sch, hip, net, shape, device, generator, noise, callback, progress):
    f32 = dict(dtype=torch.float32, device=device)
    tab = sch.device_table(device)
    x, t, out, static = _buffers(sch, shape, device)
    _initial_state(x, shape, device, generator, noise)
    fused = isinstance(generator, DeterministicGenerator)
    idx = generator.get_indices(shape[0], device) if fused and sch.n_draws else None
    zbuf = None
    sch.stage(sch.FIRST, tab, t, row=0)
    for k in _progress(range(sch.steps), progress):
        eps = _evaluate(hip, net, x, t)
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
            callback({"i": k, "t": sch.tau[sch.steps - 1 - k], "x": x.clone(), "pred_xstart": pred})
    return out


class _Replay:
    """ONE transition (network evaluation + stage launch) as a StepGraph, and the static buffers it runs on: x, t, out, the index
    vector and the history ring where the sampler keeps one.  The row, the draw number and the seed reach the captured launch
    through a host input, and the launch derives its history slots from the row, so the one captured step serves every row.  Holds
    the schedule: the captured launch reads its device table for as long as the graph lives."""

    def __init__(self, sch, hip, net, shape, device, mode):
        self.sch, self.hip, self.net, self.mode = sch, hip, net, mode
        self.tab = sch.device_table(device)
        self.x, self.t, self.out, self.static = _buffers(sch, shape, device)
        self.z = torch.empty(shape, dtype=torch.float32, device=device) if mode == "torch" else None
        self.idx = torch.zeros(shape[0], dtype=torch.int64, device=device) if mode == "fused" else None
        self.row = self.draw = self.seed = 0
        self.graph = _graph.StepGraph(self._step, device, modules=_graph.pack_modules(hip if hip is not None else net),
                                      name=sch.graph_name(shape, mode))

    def _control(self):
        return [self.row, self.draw & 0xFFFFFFFF, self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF]

    def _step(self):
        eps = _evaluate(self.hip, self.net, self.x, self.t)
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

    def run(self, shape, device, generator):
        sch = self.sch
        _initial_state(self.x, shape, device, generator, None)       # None, or a deterministic generator (also when no row draws)
        if self.mode == "fused":
            self.idx.copy_(generator.get_indices(shape[0], device))
            self.seed = int(generator.seed)
        sch.stage(sch.FIRST, self.tab, self.t, row=0)
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


def sample(sch, net, shape, device, generator, noise, callback, progress, use_graph, float64_state):
    """The body of ddpm_sample / dpm_sample on the schedule `sch` (their docstrings are the contract).  float64_state: whether the
    torch loop's state takes float64 from a float64 noise[0]; it is fp32 otherwise."""
    shape = tuple(int(s) for s in shape)
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
            return _sample_torch(sch, net, shape, device, generator, noise, callback, progress, dtype)
        replayable = generator is None or isinstance(generator, DeterministicGenerator)
        if not (use_graph and callback is None and not progress and noise is None and replayable and not _graph.capturing()):
            return _sample_eager(sch, hip, net, shape, device, generator, noise, callback, progress)
        mode = "none" if not sch.n_draws else ("fused" if isinstance(generator, DeterministicGenerator) else "torch")
        try:
            graphs = _GRAPHS.setdefault(hip if hip is not None else net, {})
        except TypeError:        # not weak-referenceable: no cache, so no replay
            return _sample_eager(sch, hip, net, shape, device, generator, noise, callback, progress)
        # what a capture freezes: the sampler and the network (the dictionary's key), the shape and the device, the table and where
        # z comes from.  pred_xstart is never written under replay: it is the callback's
        key = (sch.sampler, id(sch), shape, device.index, mode)
        rp = _memo(graphs, key, 8, lambda: _Replay(sch, hip, net, shape, device, mode))
        return rp.run(shape, device, generator)
