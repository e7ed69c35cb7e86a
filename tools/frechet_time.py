"""Time of the Frechet distance on the device against the host function, one JSON line per case:

  distance_d2048   calculate_frechet_distance_device on the d2048 statistics of oracle/fid.py (N 2341 / 2500, D 2048): wall clock
                   around the call, which ends in the readback of its last trace; warm, median of --reps; from numpy statistics
                   (two 33 MB uploads inside the call) and from statistics already on the device; the host
                   calculate_frechet_distance on the same statistics and machine, alternating with the device calls
  gemm_f64_n2048   dxmi_gemm_f64 alone at n = 2048 (device events, median of 20): ms and TFLOP/s (2 n^3 FLOP).  MI355X_MICROARCH.md gives
                   no fp64 matrix peak: the rate is reported as it is
  cifar_eval_<n>   one full in-training evaluation of train_cifar10.py (FidEvaluator: n images from the cifar10_T10 sampler at random
                   initialisation, quantise, InceptionV3 pool3 features on default-initialised weights, statistics, distance) with
                   --fid_distance host against device, n = 200 and 10 000; no checkpoint is written (--skip_eval leaves these out)

    python tools/frechet_time.py [--reps 5] [--skip_eval] [--out results/frechet_time.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "diffusion-by-maxentirl_amd")):
    sys.path.insert(0, p)
from dxmi_hip import ops  # noqa: E402
from oracle import fid as ofid  # noqa: E402
from pytorch_fid import fid_score  # noqa: E402


def median(ts):
    return sorted(ts)[len(ts) // 2]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def d2048_statistics():
    _, dims, n1, n2, s1, s2, scale2, shift2 = next(c for c in ofid.CASES if c[0] == "d2048")
    a1, a2 = ofid.synthetic_activations(s1, n1, dims), ofid.synthetic_activations(s2, n2, dims, scale=scale2, shift=shift2)
    (m1, c1), (m2, c2) = ofid.activation_statistics(a1), ofid.activation_statistics(a2)
    return m1.astype(np.float64), c1, m2.astype(np.float64), c2


def distance_case(reps):
    m1, c1, m2, c2 = d2048_statistics()
    d1, d2 = torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda()
    dev_np = lambda: fid_score.calculate_frechet_distance_device(m1, c1, m2, c2)
    dev_dev = lambda: fid_score.calculate_frechet_distance_device(m1, d1, m2, d2)
    host = lambda: fid_score.calculate_frechet_distance(m1, c1, m2, c2)
    dev_np(), dev_dev()                                   # warm-up: code objects, workspaces
    t_np, t_dev, t_host, values = [], [], [], {}
    for _ in range(reps):                                 # alternating: the three share whatever else the machine is doing
        t, values["device_numpy_in"] = wall(dev_np)
        t_np.append(t)
        t, values["device"] = wall(dev_dev)
        t_dev.append(t)
        info = dict(fid_score.last_distance_info)
        t, values["host"] = wall(host)
        t_host.append(t)
    return dict(case="distance_d2048", reps=reps, device_s=median(t_dev), device_min_s=min(t_dev), device_max_s=max(t_dev),
                device_numpy_in_s=median(t_np), host_s=median(t_host), host_min_s=min(t_host), host_max_s=max(t_host),
                host_threads=torch.get_num_threads(), speedup=median(t_host) / median(t_dev), path=info["path"],
                iterations=list(info["iterations"]), gemms=3 * sum(info["iterations"]) + 2, fid_device=float(values["device"]),
                fid_host=float(values["host"]))


def gemm_case(n=2048, reps=20):
    g = torch.Generator(device="cuda").manual_seed(1)
    a, b = (torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g) for _ in range(2))
    c = torch.empty_like(a)
    for _ in range(3):
        ops.gemm_f64(a, b, out=c)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.gemm_f64(a, b, out=c)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = median(ts)
    return dict(case=f"gemm_f64_n{n}", ms=ms, min_ms=min(ts), max_ms=max(ts), tflops=2.0 * n ** 3 / (ms * 1e-3) / 1e12)


def eval_cases(out):
    import train_cifar10
    cfg = train_cifar10.load_config("builtin:cifar10_T10", "builtin", {})
    import dxmi_config
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    net = dxmi_config.instantiate(cfg.sampler_net)
    sampler = dxmi_config.instantiate(cfg.sampler, net=net).to(device)
    from dxmi_hip import graph as hip_graph
    sampler.use_graph = hip_graph.default_enabled()
    m1, c1, _, _ = d2048_statistics()
    with tempfile.TemporaryDirectory() as tmp:
        stats = os.path.join(tmp, "stats.npz")
        np.savez(stats, mu=m1, sigma=c1)

        class Holder:                                     # FidEvaluator reads trainer.sampler.net / trainer.v only when it saves
            v = None
        Holder.sampler = sampler
        evs = {}
        for distance in ("host", "device"):
            args = argparse.Namespace(fid_extractor="pytorch_fid.inception:InceptionV3", fid_stats=stats, fid_dims=2048, fid_distance=distance)
            evs[distance] = train_cifar10.FidEvaluator(args, cfg, Holder, sampler, tmp, device, rank=1, world=1)      # rank 1: no file
        for distance in ("host", "device"):               # warm-up: graph capture of sample(100), packed Inception weights
            evs[distance].n_batches = 2
            evs[distance](0, 0)
        for n in (200, 10000):
            row = dict(case=f"cifar_eval_{n}", n_images=n)
            for distance in ("host", "device"):
                evs[distance].n_batches = n // cfg.training.sampling_batchsize
                t, fid = wall(lambda: evs[distance](0, 0))
                row[f"{distance}_s"], row[f"fid_{distance}"] = t, float(fid)
                if distance == "device":
                    row["path"], row["iterations"] = fid_score.last_distance_info["path"], list(fid_score.last_distance_info["iterations"])
            out(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip_eval", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops.device_check()
    rows = []

    def out(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)

    out(gemm_case())
    out(distance_case(a.reps))
    if not a.skip_eval:
        eval_cases(out)


if __name__ == "__main__":
    main()
