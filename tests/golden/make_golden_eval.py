"""Generate tests/golden/eval_metrics.npz by running the reference ADM evaluator's own metric code (evaluations/evaluator.py of the
reference checkout) on seeded synthetic features.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py --reference <path of the reference checkout>

CPU only; nothing is written into the reference and no source is copied: the fixture holds inputs and outputs only.
The evaluator imports TensorFlow (not installable here) and `requests`; both are stubbed in sys.modules, `np.bool` (removed in
numpy 2) is shimmed, and ManifoldEstimator / Evaluator are built without __init__ with numpy stand-ins for the two TF graphs:
  * DistanceBlock: the reference graph's fp16 distances max(|u|^2 - 2 u.v + |v|^2, 0), the fp32 retry when any is non-finite,
    and its less_thans broadcasting;
  * the softmax session: softmax(acts @ W) in float32.
The reference's manifold_radii, evaluate_pr, compute_prec_recall, compute_inception_score and FIDStatistics.frechet_distance then
run unchanged.  The features are small non-negative integers (pool3 is non-negative), so every distance is an integer below 2048:
exact in fp16, f32 and fp64 alike.  Before writing, the generator checks that an fp64 computation gives the same radii and the
same flags as the fp16 stand-in.  The fixture therefore pins the CONTRACT (which order statistic, that the self-distance and
duplicates count, which mean is the precision, how splits are taken), not fp16 rounding.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "eval_metrics.npz")

# (name, NA, NB, D, k, duplicate rows in A): sizes that are not multiples of any tile, one below one tile, duplicates, two k
PR_CASES = [
    ("basic", 300, 257, 16, 3, 0),
    ("dups", 200, 131, 16, 3, 40),
    ("small", 50, 37, 24, 5, 0),
    ("k5", 260, 390, 24, 5, 12),
]
IS_CASE = dict(N=10300, D=8, C=12)        # splits of 5000: 5000, 5000, 300


def pr_inputs(seed, NA, NB, D, dups):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 6, size=(NA, D)).astype(np.float32)
    b = rng.integers(0, 6, size=(NB, D)).astype(np.float32)
    if dups:
        src = rng.choice(NA, size=dups, replace=False)
        dst = rng.choice(np.setdiff1d(np.arange(NA), src), size=dups, replace=False)
        a[dst] = a[src]
    return a, b


def is_inputs(seed, N, D, C):
    rng = np.random.default_rng(seed)
    pool = rng.random((N, D), dtype=np.float32) * 2.0
    w = (rng.standard_normal((D, C)) * 0.7).astype(np.float32)
    return pool, w


def load_reference(ref):
    sys.dont_write_bytecode = True
    tf = types.ModuleType("tensorflow")
    tfc = types.ModuleType("tensorflow.compat")
    tfv1 = types.ModuleType("tensorflow.compat.v1")
    tf.compat, tfc.v1 = tfc, tfv1
    sys.modules.update({"tensorflow": tf, "tensorflow.compat": tfc, "tensorflow.compat.v1": tfv1,
                        "requests": types.ModuleType("requests")})
    if not hasattr(np, "bool"):
        np.bool = bool
    sys.path.insert(0, os.path.join(ref, "evaluations"))
    import evaluator
    return evaluator


def distances16(U, V):
    def block(U, V, dt):
        U, V = U.astype(dt), V.astype(dt)
        nu = np.sum(np.square(U), 1, dtype=dt).reshape(-1, 1)
        nv = np.sum(np.square(V), 1, dtype=dt).reshape(1, -1)
        return np.maximum(nu - dt(2) * (U @ V.T) + nv, dt(0))
    d = block(U, V, np.float16)
    if not np.isfinite(d).all():
        d = block(U, V, np.float32)
    return d.astype(np.float32)


class NumpyDistanceBlock:
    def pairwise_distances(self, U, V):
        return distances16(U, V)

    def less_thans(self, batch_1, radii_1, batch_2, radii_2):
        d = distances16(batch_1, batch_2)[..., None]
        return np.any(d <= radii_2, axis=1), np.any(d <= radii_1[:, None], axis=0)


class SoftmaxSession:
    def __init__(self, w):
        self.w = w

    def run(self, _fetch, feed_dict):
        (acts,) = feed_dict.values()
        z = acts.astype(np.float32) @ self.w
        z = z - z.max(1, keepdims=True)
        e = np.exp(z)
        return (e / e.sum(1, keepdims=True)).astype(np.float32)


def fp64_radii(x, k):
    x = x.astype(np.float64)
    n = (x * x).sum(1)
    d = np.maximum(n[:, None] + n[None, :] - 2 * x @ x.T, 0)
    return np.partition(d, k, axis=1)[:, k]


def fp64_flags(a, ra, b, rb):
    a, b = a.astype(np.float64), b.astype(np.float64)
    d = np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * a @ b.T, 0)
    return (d <= rb[None, :]).any(1), (d <= ra[:, None]).any(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (its evaluations/evaluator.py is imported)")
    a = ap.parse_args()
    ev = load_reference(a.reference)
    out = {}
    for ci, (name, NA, NB, D, k, dups) in enumerate(PR_CASES):
        fa, fb = pr_inputs(1000 + ci, NA, NB, D, dups)
        me = ev.ManifoldEstimator.__new__(ev.ManifoldEstimator)
        me.distance_block = NumpyDistanceBlock()
        me.row_batch_size, me.col_batch_size = 97, 89          # several reference blocks per set
        me.nhood_sizes, me.num_nhoods, me.clamp_to_percentile, me.eps = (k,), 1, None, 1e-5
        evl = ev.Evaluator.__new__(ev.Evaluator)
        evl.manifold_estimator = me
        ra, rb = me.manifold_radii(fa), me.manifold_radii(fb)
        pr = me.evaluate_pr(fa, ra, fb, rb)
        prec, rec = evl.compute_prec_recall(fa, fb)
        # the fp16 stand-in and fp64 agree exactly on these integer features
        ra64, rb64 = fp64_radii(fa, k), fp64_radii(fb, k)
        assert np.array_equal(ra[:, 0].astype(np.float64), ra64) and np.array_equal(rb[:, 0].astype(np.float64), rb64), name
        a_in_b, b_in_a = fp64_flags(fa, ra64, fb, rb64)
        assert prec == float(pr[0][0]) == b_in_a.mean() and rec == float(pr[1][0]) == a_in_b.mean(), name
        stats = [ev.FIDStatistics(np.mean(x, axis=0), np.cov(x, rowvar=False)) for x in (fa, fb)]
        out.update({f"{name}/a": fa, f"{name}/b": fb, f"{name}/k": np.int32(k), f"{name}/radii_a": ra[:, 0], f"{name}/radii_b": rb[:, 0],
                    f"{name}/precision": np.float64(prec), f"{name}/recall": np.float64(rec),
                    f"{name}/fid": np.float64(stats[1].frechet_distance(stats[0]))})
        print(f"{name}: NA {NA} NB {NB} D {D} k {k}: precision {prec:.6f} recall {rec:.6f}")
    pool, w = is_inputs(7, **IS_CASE)
    evl = ev.Evaluator.__new__(ev.Evaluator)
    evl.sess, evl.softmax, evl.softmax_input, evl.softmax_batch_size = SoftmaxSession(w), "softmax", "acts", 512
    score = evl.compute_inception_score(pool)
    out.update({"is/pool": pool, "is/w": w, "is/score": np.float64(score)})
    print(f"inception score {score:.6f}")
    out["cases"] = np.array([c[0] for c in PR_CASES])
    np.savez(OUT, **out)
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
