"""hipGraph replay of the EDM and consistency training steps (TrainLoop / CMTrainLoop with use_graph=True, models/cm/train_util.py)
against the eager loops on the same seeds: a replayed run must land, BIT FOR BIT, on the eager run's model parameters, target
parameters, EMA sets, RAdam moments, loss scale, counters and logged rows.  The nets are the shrunken U-Nets of
tests/test_hip_cm_train.py (16x16, 64 channels, formula weights with the salts "", "target:" and "teacher:"), batch 4 in two
microbatches of 2, use_fp16=True; the sigma, index and noise draws are torch's device RNG, reset by torch.manual_seed before each run.

The first run_step of a use_graph loop is the eager warm-up, the second captures, later ones replay; a changed
ema_scale_fn(global_step) pair captures again at once.  So over the calls AFTER the warm-up, captures = the number of distinct pairs
those calls met (the pair of the warm-up call itself is run eagerly and is counted only if a later call meets it again)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from test_hip_cm_train import PLAIN, TINY_KW, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CD, CT = "consistency_distillation", "consistency_training"


@pytest.fixture(scope="module", autouse=True)
def _device():
    from dxmi_hip import ops
    ops.device_check()


def _batches(n, cond, dev=DEV, seed=99):
    gen = torch.Generator().manual_seed(seed)
    xs = [(torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1).to(dev) for _ in range(n)]
    ys = [torch.randint(0, 1000, (4,), generator=gen).to(dev) for _ in range(n)]
    return [(x, {"y": y} if cond else {}) for x, y in zip(xs, ys)]


def make_loop(tmp, kind, use_graph, cond=False, norm="l2", dropout=0.0, ema_scale_fn=None, lr_anneal_steps=0, resume="", dev=DEV):
    from models.cm.karras_diffusion import KarrasDenoiser
    from models.cm.resample import LogNormalSampler
    from models.cm.train_util import CMTrainLoop, TrainLoop
    assert TINY_KW["class_cond"] and TINY_KW["image_size"] == 16 and TINY_KW["num_channels"] == 64
    over = dict({} if cond else PLAIN, dropout=dropout)
    mk = lambda *a: build(*a).to(dev)
    online = mk(over).train()
    online.dropout_seed = 11
    common = dict(model=online, data=None, batch_size=4, microbatch=2, lr=1e-4, ema_rate="0.999,0.9", log_interval=2, save_interval=100,
                  resume_checkpoint=resume, use_fp16=True, lr_anneal_steps=lr_anneal_steps, log_dir=str(tmp), use_graph=use_graph)
    if kind == "dsm":
        return TrainLoop(diffusion=KarrasDenoiser(sigma_data=0.5), schedule_sampler=LogNormalSampler(), **common)
    cd = kind == CD
    return CMTrainLoop(target_model=mk(over, "target:"), teacher_model=mk(dict(over, dropout=0.0), "teacher:") if cd else None,
                       teacher_diffusion=KarrasDenoiser(weight_schedule="uniform") if cd else None, training_mode=kind,
                       ema_scale_fn=ema_scale_fn or (lambda step: (0.9, 6)), total_training_steps=6,
                       diffusion=KarrasDenoiser(sigma_data=0.5, weight_schedule="uniform", distillation=True, loss_norm=norm), **common)


def state(tl):
    torch.cuda.synchronize()
    c = lambda ps: [p.detach().clone() for p in ps]
    s = {"masters": c(tl.mp_trainer.master_params), "model": c(tl.model.parameters()), "lg": tl.mp_trainer.lg_loss_scale,
         "step": tl.step, "global_step": getattr(tl, "global_step", None), "logged": [dict(r) for r in tl.logged],
         "opt_step": tl.opt.step_count(), "lr": [g["lr"] for g in tl.opt.param_groups]}
    for i, ps in enumerate(tl.ema_params):
        s[f"ema{i}"] = c(ps)
    s["exp_avg"] = c([tl.opt.state[P]["exp_avg"] for P in tl.mp_trainer.master_params])
    s["exp_avg_sq"] = c([tl.opt.state[P]["exp_avg_sq"] for P in tl.mp_trainer.master_params])
    s["dropout_calls"] = tl.model.__dict__.get("_dropout_calls", 0)
    if hasattr(tl, "target_model"):
        s["target_masters"] = c(tl.target_model_master_params)
        s["target"] = c(tl.target_model.parameters())
    return s


def same_rows(a, b):
    eq = lambda u, v: u == v or (u != u and v != v)
    return len(a) == len(b) and all(set(r) == set(q) and all(eq(r[k], q[k]) for k in r) for r, q in zip(a, b))


def assert_same(a, b):
    assert set(a) == set(b)
    for k, v in a.items():
        if k == "logged":
            assert same_rows(v, b[k]), (v, b[k])
        elif isinstance(v, list) and v and torch.is_tensor(v[0]):
            assert len(v) == len(b[k]) and all(torch.equal(p, q) for p, q in zip(v, b[k])), k
        else:
            assert v == b[k], (k, v, b[k])


def run(tl, batches, seed=5, each=None, every=2):
    """run_step over `batches`, a log row after every `every` calls -> the took_step of every call.  seed None: the device
    generator goes on from where it is."""
    if seed is not None:
        torch.manual_seed(seed)
    took = []
    for k, (x, cond) in enumerate(batches):
        took.append(tl.run_step(x, cond))
        if (k + 1) % every == 0:
            tl.dumpkvs()
        if each is not None:
            each(k)
    return took


CASES = [("dsm", "l2", True), ("dsm", "l2", False)] + [(kind, norm, cond) for kind in (CD, CT) for norm in ("l2", "l2-32")
                                                      for cond in (True, False)]


@pytest.mark.parametrize("kind,norm,cond", CASES)
def test_replayed_steps_equal_eager_bitwise(tmp_path, kind, norm, cond):
    batches = _batches(5, cond)
    te = make_loop(tmp_path / "e", kind, False, cond, norm)
    assert all(run(te, batches))
    tg = make_loop(tmp_path / "g", kind, True, cond, norm)
    assert all(run(tg, batches))
    assert tg._graph.captures == 1 and tg._graph.replays == 3 and te._graph is None
    se, sg = state(te), state(tg)
    assert se["step"] == 5 and len(se["logged"]) == 2 and "loss" in se["logged"][0] and se["opt_step"] == 5.0
    assert_same(se, sg)


def test_overflow_steps_are_skipped_on_the_device(tmp_path):
    """lg_loss_scale = 129.5: 2^129.5 and 2^128.5 are inf in fp32, and for many steps after them the squared gradients are, so the
    first six steps all overflow.  Under replay nothing on the host gates the EMAs: the launches take the device flag.  Then the
    scale is set to 20 on the host (the graph reads it per replay) and two steps are taken."""
    batches = _batches(8, False)
    ends, tooks = [], []
    for use_graph in (False, True):
        tl = make_loop(tmp_path / str(use_graph), CT, use_graph)
        tl.mp_trainer.lg_loss_scale = 129.5
        first = {}

        def each(k, tl=tl, first=first, use_graph=use_graph):
            if k == 0 and use_graph:
                first.update(state(tl))         # after the eager warm-up step, itself skipped (the optimiser state exists now)
            if k == 5:
                if use_graph:                   # five more skipped steps, four of them replayed: nothing has moved
                    now = state(tl)
                    for key in ("masters", "ema0", "ema1", "target_masters", "target", "exp_avg", "exp_avg_sq"):
                        assert all(torch.equal(a, b) for a, b in zip(first[key], now[key])), key
                    assert now["global_step"] == 0 and now["step"] == 0 and now["opt_step"] == 0.0 and now["lg"] == 123.5
                tl.mp_trainer.lg_loss_scale = 20.0
        tooks.append(run(tl, batches, each=each))
        ends.append(state(tl))
        if use_graph:
            assert tl._graph.replays == 6
    assert tooks[0] == tooks[1] == [False] * 6 + [True] * 2
    assert ends[0]["global_step"] == 2 and ends[0]["opt_step"] == 2.0     # global_step lags the 8 calls by the 6 skipped ones
    assert_same(ends[0], ends[1])


def test_key_change_recaptures(tmp_path):
    """scale_mode progressive, 2 -> 6 scales over 6 steps: num_scales (and with target_ema_mode adaptive the EMA rate) changes
    at almost every step; every change drops the graph and captures the next one."""
    from models.cm.script_util import create_ema_and_scales_fn
    fn = create_ema_and_scales_fn(target_ema_mode="adaptive", start_ema=0.9, scale_mode="progressive", start_scales=2, end_scales=6,
                                  total_steps=6, distill_steps_per_iter=0)
    batches = _batches(6, False)
    te = make_loop(tmp_path / "e", CT, False, ema_scale_fn=fn)
    assert all(run(te, batches))
    tg = make_loop(tmp_path / "g", CT, True, ema_scale_fn=fn)
    assert all(run(tg, batches))
    pairs = [fn(s) for s in range(6)]                       # every step was taken: call k ran at global_step k
    assert len({p[1] for p in pairs}) >= 4 and len({p[0] for p in pairs}) >= 4
    after_warmup = pairs[1:]
    assert tg._graph.captures == len(set(after_warmup)) == tg._graph.builds
    assert tg._graph.replays == 5 - tg._graph.captures and tg._graph.replays >= 1
    assert tg._graph.key == pairs[5]
    assert_same(state(te), state(tg))


def test_lr_anneal_reaches_the_replayed_optimiser(tmp_path):
    batches = _batches(5, False)
    te, tg = make_loop(tmp_path / "e", "dsm", False, lr_anneal_steps=5), make_loop(tmp_path / "g", "dsm", True, lr_anneal_steps=5)
    assert all(run(te, batches)) and all(run(tg, batches))
    se, sg = state(te), state(tg)
    assert se["lr"] == [0.0] and tg._graph.replays == 3
    assert_same(se, sg)
    fixed = make_loop(tmp_path / "f", "dsm", False)         # the anneal is visible in the parameters: lr held would end elsewhere
    assert all(run(fixed, batches))
    assert not all(torch.equal(a, b) for a, b in zip(state(fixed)["masters"], se["masters"]))


@pytest.mark.parametrize("kind", ["dsm", CT])
def test_dropout_seeds_are_host_inputs(tmp_path, kind):
    batches = _batches(5, True)
    te = make_loop(tmp_path / "e", kind, False, True, dropout=0.1)
    assert all(run(te, batches))
    tg = make_loop(tmp_path / "g", kind, True, True, dropout=0.1)
    assert all(run(tg, batches))
    assert tg._graph.replays == 3
    from models.cm.unet import ResBlock
    sites = sum(isinstance(m, ResBlock) for m in tg.model.modules())       # one dropout site per ResBlock
    assert sites > 0
    assert te.model._dropout_calls == tg.model._dropout_calls == 5 * 2 * sites
    if kind == CT:                                          # the target drew nothing: it read the online forward's device words
        assert "_dropout_calls" not in te.target_model.__dict__ and "_dropout_calls" not in tg.target_model.__dict__
        on, tgt = tg.model.dropout_seeds_used, tg.target_model.dropout_seeds_used
        assert len(on) == sites and all(torch.is_tensor(s) and s.is_cuda for s in on)
        assert [s.data_ptr() for s in on] == [s.data_ptr() for s in tgt]
    assert_same(state(te), state(tg))
    nodrop = make_loop(tmp_path / "n", kind, False, True)
    assert all(run(nodrop, batches))
    assert not all(torch.equal(a, b) for a, b in zip(state(nodrop)["masters"], state(te)["masters"]))


def test_resume_of_a_replayed_run(tmp_path):
    batches = _batches(5, False)
    te = make_loop(tmp_path / "e", CT, False)
    assert all(run(te, batches, every=1))
    tg = make_loop(tmp_path / "g", CT, True)
    assert all(run(tg, batches[:3], every=1))
    assert tg._graph.replays == 1 and tg.global_step == 3
    tg.save()
    tr = make_loop(tmp_path / "g", CT, True, resume=str(tmp_path / "g" / "model000003.pt"))
    assert tr.global_step == 3 and tr.step == 3 and tr.opt.step_count() == 3.0
    # the checkpoint was mapped to the device; the step counters, which the graph's host producers read, are back on the host
    assert all(st["step"].device.type == "cpu" for st in tr.opt.state.values())
    tr.mp_trainer.lg_loss_scale = tg.mp_trainer.lg_loss_scale       # the reference does not checkpoint the loss scale
    tr.logged = list(tg.logged)
    assert all(run(tr, batches[3:], seed=None, every=1))            # warm-up call, then the capture
    assert tr._graph.captures == 1
    assert_same(state(te), state(tr))


def _two_ranks(tmp_path, backend):
    """Two fresh interpreters, one per rank, each under its own time limit (tests/_cm_graph_worker.py) -> rank 0's result line."""
    import json
    here = os.path.dirname(os.path.abspath(__file__))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   DXMI_TEST_BACKEND=backend)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(here, "_cm_graph_worker.py"),
                                       str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=330) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-3000:]
    return json.loads([ln for ln in outs[0][0].splitlines() if ln.startswith("{")][-1])


def _check_two_ranks(line):
    assert line["world"] == 2 and line["replays"] == 3 and line["cuts"] == 1
    assert line["ranks_identical"] and line["graph_equals_eager"]


def test_two_ranks_replay_equals_eager(tmp_path):
    """Five consistency_training steps (three of them replayed) on two ranks, eager and with use_graph (the gradient exchange is a
    cut of the graph): the ranks end on identical parameters, and the replayed run on the eager run's."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    _check_two_ranks(_two_ranks(tmp_path, "nccl"))


def test_two_ranks_on_one_gpu_gloo(tmp_path):
    """The same two-rank run where there is one GPU: both processes share cuda:0 and all-reduce their (different) gradients over
    gloo at the graph's cut, as tests/test_hip_graph.py does for the DxMI steps."""
    _check_two_ranks(_two_ranks(tmp_path, "gloo"))
