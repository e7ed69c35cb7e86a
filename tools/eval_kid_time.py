"""Device time of the evaluator's KID and density / coverage kernels (csrc/eval_metrics.hip) at the ADM evaluator's
sizes, D = 2048, in one process with the legs of a comparison alternating (one call of each per round, the median over the rounds;
device events around each call, after one warm-up call of every leg, as tools/eval_pr_time.py times):

    counts / membership     dxmi_dc_counts at 10 000 x 50 000 against dxmi_pr_membership at the same sizes (the same K loop; the
                            epilogues differ)
    kid_full_10000x50000    the KID launch over all rows of the same two sets, beside them: X.X, Y.Y (upper tiles) and X.Y; the
                            X.Y part is `xy_share_of_flop` of its algorithmic FLOP
    kid_protocol            100 subsets of 1000 rows as ONE launch against the same subsets as 100 single-subset calls
    kid_full_50000x50000    the estimate over all rows at 50 000 x 50 000
    kid_vs_fid (--bias)     KID and FID of one synthetic generator at 10 000 and at 50 000 samples against a 50 000-row reference:
                            the bias of FID in the sample count, in numbers (full-rank features relu(z M), not Inception features)

Prints one JSON line per case: median ms, the algorithmic TFLOP, the floor at the 155 TFLOP/s f32-MFMA rate (MI355X_MICROARCH.md)
and floor / ms.  A call's time includes its launches' host side; nothing here is a kernel-trace time.
    python tools/eval_kid_time.py [--reps 5] [--bias] [--out results/eval_kid_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))
from dxmi_hip import ops  # noqa: E402
from evaluations import evaluator as ev  # noqa: E402

PEAK = 155e12


def features(N, D, seed, shift=0.0, latent=64):
    """relu(z M) with one projection for every set (overlapping manifolds), the sample sets shifted in z."""
    g = torch.Generator(device="cuda").manual_seed(7)
    M = torch.randn(latent, D, device="cuda", generator=g) / latent ** 0.5
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.relu((torch.randn(N, latent, device="cuda", generator=g) + shift) @ M).contiguous()


def timed_alternating(legs, reps):
    """legs: {name: fn}; one warm-up call each, then `reps` rounds of one call of each leg in turn -> {name: median ms}."""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {name: (sorted(t)[len(t) // 2], min(t), max(t)) for name, t in ts.items()}


def kid_flop(S, mx, my, D):
    return 2.0 * D * S * (mx * (mx + 1) / 2 + my * (my + 1) / 2 + mx * my)


def row(case, t, flop, **kw):
    ms, lo, hi = t
    return dict(case=case, ms=ms, ms_min=lo, ms_max=hi, tflop=flop / 1e12, floor_ms=flop / PEAK * 1e3, frac_of_f32_mfma_peak=flop / PEAK * 1e3 / ms, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bias", action="store_true", help="also KID and FID of one generator at 10 000 and 50 000 samples")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops.device_check()
    D = 2048
    ref10, ref50, sample = features(10000, D, 1), features(50000, D, 3), features(50000, D, 2, shift=0.25)
    rows = []
    # ---- counts against membership, and the KID kernel on the same pairs
    ra, rb = ops.knn_radii(ref10, 5), ops.knn_radii(sample, 3)
    t = timed_alternating({"member": lambda: ops.pr_membership(ref10, ra, sample, rb), "counts": lambda: ops.dc_counts(ref10, ra, sample),
                           "kid": lambda: ops.kid_sums(ref10, sample)}, a.reps)
    pair_flop = 2.0 * 10000 * 50000 * D
    rows.append(row("membership_10000x50000", t["member"], pair_flop))
    rows.append(row("dc_counts_10000x50000", t["counts"], pair_flop, ratio_to_membership=t["counts"][0] / t["member"][0]))
    rows.append(row("kid_full_10000x50000", t["kid"], kid_flop(1, 10000, 50000, D), xy_share_of_flop=pair_flop / kid_flop(1, 10000, 50000, D)))
    # ---- the protocol: 100 subsets of 1000 in one launch against 100 launches
    ix, iy = ev.kid_subset_indices(10000, 50000, 100, 1000, seed=0)
    ix, iy = torch.from_numpy(ix).cuda(), torch.from_numpy(iy).cuda()
    singles = [(ix[s:s + 1].contiguous(), iy[s:s + 1].contiguous()) for s in range(100)]

    def one_by_one():
        return [ops.kid_sums(ref10, sample, i, j) for i, j in singles]
    t = timed_alternating({"batched": lambda: ops.kid_sums(ref10, sample, ix, iy), "singles": one_by_one}, a.reps)
    assert torch.equal(torch.cat(one_by_one()), ops.kid_sums(ref10, sample, ix, iy))
    rows.append(row("kid_protocol_100x1000_one_launch", t["batched"], kid_flop(100, 1000, 1000, D)))
    rows.append(row("kid_protocol_100x1000_100_launches", t["singles"], kid_flop(100, 1000, 1000, D), ratio_to_one_launch=t["singles"][0] / t["batched"][0]))
    # ---- all rows at 50 000 x 50 000
    t = timed_alternating({"kid": lambda: ops.kid_sums(ref50, sample)}, max(2, a.reps // 2))
    rows.append(row("kid_full_50000x50000", t["kid"], kid_flop(1, 50000, 50000, D)))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.bias:
        from pytorch_fid.fid_score import activation_statistics, calculate_frechet_distance_device
        # full-rank features (latent = D): FID's bias in the sample count grows with the rank of the covariance
        ref = features(50000, D, 5, latent=D)
        mu_r, sig_r = activation_statistics(ref)
        same = features(50000, D, 4, latent=D)           # the reference's own distribution: the true distance is 0
        for name, gen in (("same_distribution", same), ("shifted", features(50000, D, 6, shift=0.25, latent=D))):
            for n in (10000, 50000):
                x = gen[:n].contiguous()
                mu, sig = activation_statistics(x)
                fid = float(calculate_frechet_distance_device(mu, sig, mu_r, sig_r))
                kid, kid_std = ev.kernel_inception_distance(ref, x)
                kid_all, _ = ev.kernel_inception_distance(ref, x, subsets=0)
                r = dict(case=f"kid_vs_fid_{name}_{n}", samples=n, fid=fid, kid=kid, kid_std=kid_std, kid_all_rows=kid_all)
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
