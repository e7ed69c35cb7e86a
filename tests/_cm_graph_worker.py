"""Rank process of the two-rank tests of tests/test_hip_cm_graph.py: five consistency_training steps of CMTrainLoop on this rank's
own batches, eagerly and with use_graph=True (three of the five replayed), in a group of two: nccl (= RCCL), one GPU per rank, or
with DXMI_TEST_BACKEND=gloo both ranks on cuda:0."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "diffusion-by-maxentirl_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    rank, tmp = int(os.environ["RANK"]), sys.argv[1]
    backend = os.environ.get("DXMI_TEST_BACKEND", "nccl")
    if backend == "gloo":       # two ranks on ONE GPU (RCCL refuses that): real collectives, moved through the host
        dev = "cuda:0"
        torch.cuda.set_device(0)
        dist.init_process_group("gloo")
    else:
        dev = f"cuda:{rank}"
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", rank))
    import test_hip_cm_graph as t
    batches = t._batches(5, False, dev=dev, seed=99 + rank)
    ends = []
    for use_graph in (False, True):
        tl = t.make_loop(os.path.join(tmp, f"{use_graph}.{rank}"), t.CT, use_graph, dev=dev)
        assert all(t.run(tl, batches, seed=5 + rank))
        ends.append((t.state(tl), tl))
    (se, _), (sg, tg) = ends
    flat = lambda s: torch.cat([p.reshape(-1) for p in s["masters"] + s["target_masters"]])
    mine = flat(sg)
    other = mine.clone()
    dist.broadcast(other, 0)
    same = torch.tensor([float(torch.equal(mine, other)), float(torch.equal(mine, flat(se)) and se["lg"] == sg["lg"]
                                                                 and se["global_step"] == sg["global_step"] == 5)], device=dev)
    dist.all_reduce(same, op=dist.ReduceOp.MIN)
    cuts = sum(1 for kind, _ in tg._graph.graph.segments if kind == "eager")
    if rank == 0:
        print(json.dumps({"world": dist.get_world_size(), "replays": tg._graph.replays, "cuts": cuts,
                          "ranks_identical": bool(same[0] == 1), "graph_equals_eager": bool(same[1] == 1)}))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
