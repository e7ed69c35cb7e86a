"""Host side of use_graph=True on TrainLoop / CMTrainLoop (models/cm/train_util.py): the constructor's refusals, a CPU model running
eagerly, the one-graph-per-key logic with StepGraph replaced by a counting stub, and the --use_graph flag of cm_train.py.  No GPU."""
import os

import pytest
import torch


class _Tiny(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(3, 3, generator=gen) * 0.3)
        self.b = torch.nn.Parameter(torch.randn(3, generator=gen) * 0.1)

    def forward(self, x, t):
        return torch.tanh(torch.einsum("oc,nchw->nohw", self.a, x) + self.b[None, :, None, None] + 1e-3 * t[:, None, None, None])


def _cm_kw(tmp, **over):
    from models.cm.karras_diffusion import KarrasDenoiser
    kw = dict(model=_Tiny(1), target_model=_Tiny(2), teacher_model=None, teacher_diffusion=None, training_mode="consistency_training",
              ema_scale_fn=lambda s: (0.9, 6), total_training_steps=4,
              diffusion=KarrasDenoiser(sigma_data=0.5, weight_schedule="uniform", distillation=True), data=None, batch_size=4,
              microbatch=2, lr=1e-2, ema_rate="0.9", log_interval=1, save_interval=100, resume_checkpoint="", use_fp16=True,
              log_dir=str(tmp))
    kw.update(over)
    return kw


def _dsm_kw(tmp, **over):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.resample import LogNormalSampler
    kw = dict(model=_Tiny(1), diffusion=KarrasDenoiser(sigma_data=0.5), data=None, batch_size=4, microbatch=2, lr=1e-2, ema_rate="0.9",
              log_interval=1, save_interval=100, resume_checkpoint="", use_fp16=True, schedule_sampler=LogNormalSampler(),
              log_dir=str(tmp))
    kw.update(over)
    return kw


def test_use_graph_is_a_keyword_and_off_by_default(tmp_path):
    from models.cm.train_util import CMTrainLoop, TrainLoop
    for loop in (TrainLoop(**_dsm_kw(tmp_path)), CMTrainLoop(**_cm_kw(tmp_path))):
        assert loop.use_graph is False and loop._graph is None
    assert TrainLoop(**_dsm_kw(tmp_path, use_graph=False)).use_graph is False


def test_use_graph_refuses_fp32_lpips_and_host_draws(tmp_path):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.resample import LogNormalSampler
    from models.cm.train_util import CMTrainLoop, TrainLoop
    with pytest.raises(NotImplementedError, match="use_graph=True needs use_fp16=True"):
        TrainLoop(**_dsm_kw(tmp_path, use_graph=True, use_fp16=False))
    with pytest.raises(NotImplementedError, match="use_graph=True needs use_fp16=True"):
        CMTrainLoop(**_cm_kw(tmp_path, use_graph=True, use_fp16=False))
    d = KarrasDenoiser(sigma_data=0.5, distillation=True)
    d.loss_norm = "lpips"                       # set on the object, as cm_train.py sets it
    with pytest.raises(NotImplementedError, match="loss_norm='lpips'"):
        CMTrainLoop(**_cm_kw(tmp_path, use_graph=True, diffusion=d))
    CMTrainLoop(**_cm_kw(tmp_path, use_graph=False, diffusion=d))           # eagerly the norm is the loss node's business
    with pytest.raises(NotImplementedError, match="draws on the device"):
        TrainLoop(**_dsm_kw(tmp_path, use_graph=True, schedule_sampler=LogNormalSampler(generator=torch.Generator().manual_seed(1))))


def test_cpu_model_with_use_graph_runs_eagerly(tmp_path):
    """As the samplers' use_graph: a model that is not on the device takes the eager path, step for step the use_graph=False run."""
    from models.cm.train_util import CMTrainLoop
    gen = torch.Generator().manual_seed(3)
    x = [torch.rand(4, 3, 8, 8, generator=gen) * 2 - 1 for _ in range(3)]
    ends = []
    for use_graph in (False, True):
        tl = CMTrainLoop(**_cm_kw(tmp_path / str(use_graph), use_graph=use_graph))
        tl.opt = torch.optim.RAdam(tl.mp_trainer.master_params, lr=1e-2)     # torch's RAdam stands in for the device one on the CPU
        assert tl.use_graph is False and tl._graph is None
        torch.manual_seed(7)
        for k in range(3):
            assert tl.run_step(x[k], {})
        assert tl.step == 3 and tl.global_step == 3
        ends.append([p.detach().clone() for p in tl.mp_trainer.master_params + tl.target_model_master_params])
        row = tl.dumpkvs()
        assert row["step"] == 3 and row["loss"] == row["loss"]
    assert all(torch.equal(a, b) for a, b in zip(*ends))


class _CountingGraph:
    """Stands in for dxmi_hip.graph.StepGraph: the first call of an instance 'captures', later ones 'replay'."""
    built, alive = [], 0

    def __init__(self, key):
        self.key, self.captures, self.replays = key, 0, 0
        _CountingGraph.built.append(key)
        _CountingGraph.alive += 1

    def __del__(self):
        _CountingGraph.alive -= 1

    def __call__(self, *args):
        if self.captures == 0:
            self.captures = 1
        else:
            self.replays += 1
        return (self.key, args)


def test_graph_key_same_key_reuses_changed_key_drops_and_rebuilds():
    import gc
    from models.cm.train_util import _KeyedStepGraph
    _CountingGraph.built, _CountingGraph.alive = [], 0
    drops = []
    kg = _KeyedStepGraph(_CountingGraph, on_drop=lambda: drops.append(kg.key))
    keys = [(0.9, 2), (0.9, 2), (0.9, 2), (0.9, 4), (0.95, 4), (0.95, 4), (0.9, 2)]
    for i, key in enumerate(keys):
        out = kg(key, i)
        assert out == (key, (i,)) and kg.key == key
        gc.collect()
        assert _CountingGraph.alive == 1                     # only the current key's graph is kept
    assert _CountingGraph.built == [(0.9, 2), (0.9, 4), (0.95, 4), (0.9, 2)]     # a key met again later is built again
    assert kg.builds == 4 and kg.captures == 4 and kg.replays == 3
    assert drops == [(0.9, 2), (0.9, 4), (0.95, 4)]          # on_drop runs before the held graph goes, not before the first build
    kg.drop()
    gc.collect()
    assert kg.graph is None and _CountingGraph.alive == 0 and drops[-1] == (0.9, 2)


def test_loop_keys_its_graph_on_the_ema_and_scales_pair(tmp_path, monkeypatch):
    """run_step's warm-up and counting and the loop's _graph_key, with the device left out (_step_replayed is replaced by a stub
    that makes its keyed call; the real one runs in tests/test_hip_cm_graph.py): the first run_step is the eager warm-up, then one
    build per change of ema_scale_fn(global_step), and a held global_step (an overflow step) keeps the graph."""
    from models.cm.train_util import CMTrainLoop, _KeyedStepGraph
    pairs = [(0.9, 2), (0.9, 4), (0.9, 4), (0.95, 5), (0.95, 5)]
    tl = CMTrainLoop(**_cm_kw(tmp_path, ema_scale_fn=lambda s: pairs[s]))
    _CountingGraph.built, _CountingGraph.alive = [], 0
    tl.use_graph, tl._graph = True, _KeyedStepGraph(_CountingGraph)
    took = iter([True, True, False, True, True, True])
    eager = []
    monkeypatch.setattr(tl, "_step_on_device", lambda b, c: eager.append(tl.global_step) or next(took))

    def replayed(batch, cond):
        tl._graph(tl._graph_key(), batch)
        return next(took)
    monkeypatch.setattr(tl, "_step_replayed", replayed)
    steps = []
    for _ in range(6):
        tl.run_step(torch.zeros(4, 3, 8, 8), {})
        steps.append(tl.global_step)
    assert eager == [0] and steps == [1, 2, 2, 3, 4, 5]      # the third call overflowed: counters held
    assert _CountingGraph.built == [(0.9, 4), (0.95, 5)]     # global_step 1, 2, 2 -> (0.9, 4); 3, 4 -> (0.95, 5)
    assert tl._graph.captures == 2 and tl._graph.replays == 3


def test_cm_train_use_graph_flag(monkeypatch):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusion-by-maxentirl_amd")
    monkeypatch.syspath_prepend(pkg)
    import cm_train
    assert cm_train.parse_args(["--synthetic_data", "True"]).use_graph is False
    assert cm_train.parse_args(["--synthetic_data", "True", "--use_graph", "True"]).use_graph is True


@pytest.mark.parametrize("name", ["Adam", "RAdam"])
def test_loaded_step_counters_are_host_tensors(name):
    """load_state_dict leaves the step counters where the graph's host producers (and every eager float(step)) read them without a
    device read: CPU tensors with the saved values.  A counter on another device is moved (_host_step_counters, which only looks at
    the tensor's device): shown here with a stand-in, since this test has no second device."""
    from dxmi_hip import optim
    p = torch.nn.Parameter(torch.zeros(5))
    src = getattr(optim, name)([p], lr=1e-3)
    src.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.ones(5), "exp_avg_sq": torch.full((5,), 2.0)}
    dst = getattr(optim, name)([torch.nn.Parameter(torch.zeros(5))], lr=1e-3)
    dst.__dict__["_dxmi_cache"] = {"stale": 1}
    dst.load_state_dict(src.state_dict())
    (st,) = dst.state.values()
    assert st["step"].device.type == "cpu" and float(st["step"]) == 3.0 and torch.equal(st["exp_avg_sq"], torch.full((5,), 2.0))
    assert "_dxmi_cache" not in dst.__dict__

    class Elsewhere:            # what _host_step_counters asks of a counter
        device = torch.device("meta")

        def cpu(self):
            return torch.tensor(7.0)
    st["step"] = Elsewhere()
    real_is_tensor = torch.is_tensor
    try:
        torch.is_tensor = lambda t: isinstance(t, Elsewhere) or real_is_tensor(t)
        optim._host_step_counters(dst)
    finally:
        torch.is_tensor = real_is_tensor
    assert real_is_tensor(st["step"]) and st["step"].device.type == "cpu" and float(st["step"]) == 7.0
