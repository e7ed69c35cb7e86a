"""Child process of tests/test_hip_ict.py::test_cmtrainloop_ict_replayed_equals_eager: six steps of improved consistency training
(CMTrainLoop with the ("fixed", "ict") curriculum 3, 3, 5, 5, 9, 9 levels, target EMA 0, the discretised lognormal level sampler)
eagerly and with use_graph=True on the same seed; prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "diffusion-by-maxentirl_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    tmp = sys.argv[1]
    import test_hip_cm_graph as t
    import test_hip_ict as ict
    batches = t._batches(6, False)
    te = ict.make_ict_loop(os.path.join(tmp, "eager"), False)
    assert all(t.run(te, batches))
    tg = ict.make_ict_loop(os.path.join(tmp, "graph"), True)
    assert all(t.run(tg, batches))
    se, sg = t.state(te), t.state(tg)
    t.assert_same(se, sg)                      # parameters, masters, target, EMA sets, RAdam moments, loss scale, counters, log rows
    bits = lambda ps: torch.cat([p.detach().reshape(-1).view(torch.int32) for p in ps])
    print(json.dumps({"captures": tg._graph.captures, "builds": tg._graph.builds, "replays": tg._graph.replays,
                      "global_step": tg.global_step, "key": list(tg._graph.key), "graph_equals_eager": True,
                      "target_is_online": bool(torch.equal(bits(tg.target_model.parameters()), bits(tg.model.parameters()))
                                               and torch.equal(bits(te.target_model.parameters()), bits(te.model.parameters())))}))


if __name__ == "__main__":
    main()
