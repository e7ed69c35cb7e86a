"""Device time of the evaluator's precision / recall kernels (csrc/eval_metrics.hip) at the ADM evaluator's sizes:
k-NN radii (k = 3) at N = 10 000 and 50 000, D = 2048, and membership at 10 000 x 50 000, D = 2048; plus the Inception Score
stage at 50 000 x 2048 x 1008.  Prints one JSON line per case: median ms over the timed repeats (device events around each call,
after one warm-up call) and the fraction of the 155 TFLOP/s f32-MFMA rate (MI355X_MICROARCH.md) the algorithmic FLOP reach.
    python tools/eval_pr_time.py [--reps 3] [--out results/eval_pr_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))
from dxmi_hip import ops  # noqa: E402

PEAK = 155e12


def features(N, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.relu(torch.randn(N, D, device="cuda", generator=g))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops.device_check()
    D = 2048
    ref, sample = features(10000, D, 1), features(50000, D, 2)
    rows = []
    for name, x in (("radii_10000", ref), ("radii_50000", sample)):
        N = x.shape[0]
        ms = timed(lambda: ops.knn_radii(x, 3), a.reps)
        rows.append(dict(case=name, N=N, D=D, ms=ms, tflop=2.0 * N * N * D / 1e12, floor_ms=2.0 * N * N * D / PEAK * 1e3))
    ra, rb = ops.knn_radii(ref, 3), ops.knn_radii(sample, 3)
    ms = timed(lambda: ops.pr_membership(ref, ra, sample, rb), a.reps)
    rows.append(dict(case="membership_10000x50000", N=10000 * 50000, D=D, ms=ms, tflop=2.0 * 10000 * 50000 * D / 1e12,
                     floor_ms=2.0 * 10000 * 50000 * D / PEAK * 1e3))
    w = torch.randn(1008, D, device="cuda") * 0.02
    ms = timed(lambda: ops.inception_score_kl(sample, w), a.reps)
    rows.append(dict(case="inception_score_50000x1008", N=50000, D=D, ms=ms, tflop=2.0 * 50000 * D * 1008 / 1e12,
                     floor_ms=2.0 * 50000 * D * 1008 / PEAK * 1e3))
    total = sum(r["ms"] for r in rows[:3])
    for r in rows:
        r["frac_of_f32_mfma_peak"] = r["floor_ms"] / r["ms"]
        print(json.dumps(r))
    print(json.dumps(dict(case="precision_recall_total", ms=total, floor_ms=sum(r["floor_ms"] for r in rows[:3]))))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
