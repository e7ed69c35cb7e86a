"""Rank process of tests/test_hip_ddpm_train.py::test_two_ranks_on_one_gpu: two fresh interpreters share cuda:0 and exchange their
(different) gradients over gloo; each runs DDPMTrainLoop eagerly and replayed on its own data and counts the collectives per step."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "diffusion-by-maxentirl_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    import test_hip_ddpm_train as td
    calls = [0]
    real = dist.all_reduce

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    dist.all_reduce = counted
    steps = 5
    runs = {}
    for mode in ("eager", "graph"):
        loop, per_step = td.run_loop(mode == "graph", steps, tmp=tempfile.mkdtemp(prefix="ddpm_rank_"), seed=20 + rank, rates="0.9", counter=calls)
        runs[mode] = (loop, per_step)
    le, lg = runs["eager"][0], runs["graph"][0]
    out = {"world": dist.get_world_size(), "eager_collectives": runs["eager"][1], "graph_collectives": runs["graph"][1],
           "captures": lg.captures, "replays": lg.replays,
           "params_equal": all(torch.equal(a, b) for a, b in zip(le.params, lg.params)),
           "cuts": [kind for kind, _ in lg._graph.segments].count("eager")}
    chk = torch.stack([p.detach().double().sum() for p in lg.params] + [p.detach().double().abs().sum() for p in lg.params])
    allc = [torch.zeros_like(chk) for _ in range(dist.get_world_size())]
    dist.all_gather(allc, chk)
    out["ranks_identical"] = all(torch.equal(allc[0], c) for c in allc)
    # the ranks saw different data: their local losses differ
    ls = torch.tensor([lg.logged[-1]["loss"]], device="cuda:0", dtype=torch.float64)
    alll = [torch.zeros_like(ls) for _ in range(dist.get_world_size())]
    dist.all_gather(alll, ls)
    out["losses_differ"] = not torch.equal(alll[0], alll[-1])
    if rank == 0:
        print(json.dumps(out))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
