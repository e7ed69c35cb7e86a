"""Throughput of the EDM teacher's Heun sampler (karras_sample, hipGraph replay) next to the DxMI sampler on the same net.

In ONE process, alternating the two: Heun, 40 steps (79 network evaluations per image), and OpenAIDiffusion T=10 (10), both on
the full-size ImageNet-64 U-Net (295.9 M parameters, fp16 config, synthetic weights) at the same batch.  Prints images/s and
ms per network evaluation (NFE) for each, the median over --rounds, and one JSON line.

    python tools/karras_sample_time.py [--batch 100] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/karras_sample_time.py --only heun --rounds 1
      (the stage kernels' share: karras_stage_kernel against the total kernel time, from the run's database or, with
       --output-format csv, from its kernel_stats.csv, which tools/kstats.py reads)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("heun", "dxmi"), default=None)
    a = ap.parse_args()

    import configs_builtin
    from models.cm.karras_diffusion import karras_nfe, karras_sample
    from models.cm.script_util import create_model_and_diffusion
    from models.DxMI.openai_diffusion import OpenAIDiffusion
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    cfg = configs_builtin.get("imagenet64_T10")
    unet, diffusion = create_model_and_diffusion(**cfg.diffusion)
    dxmi = OpenAIDiffusion(unet, diffusion, **cfg.sampler)
    unet.to(dev)
    if cfg.diffusion.use_fp16:
        unet.convert_to_fp16()
    dxmi.eval()
    dxmi.use_graph = True
    B, shape = a.batch, (a.batch,) + tuple(cfg.sampler.sample_shape)
    y = torch.randint(0, 1000, (B,), device=dev)

    def heun():
        return karras_sample(diffusion, unet, shape, a.steps, model_kwargs={"y": y}, device=dev, sampler="heun", use_graph=True)

    def oad():
        return dxmi.sample(B, device=dev, i_class=y)["sample"]

    runs = {"heun": (heun, karras_nfe("heun", a.steps)), "dxmi": (oad, cfg.sampler.n_timesteps)}
    if a.only:
        runs = {a.only: runs[a.only]}
    for fn, _ in runs.values():           # eager first call, then the capture
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (fn, _) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
            assert torch.isfinite(out).all()
    res = {"batch": B}
    for k, (_, nfe) in runs.items():
        t = statistics.median(times[k])
        res[k] = {"nfe": nfe, "s_per_batch": round(t, 4), "images_per_s": round(B / t, 2), "ms_per_nfe": round(1e3 * t / nfe, 3),
                  "rounds_s": [round(v, 4) for v in times[k]]}
        print(f"{k:5s}: {nfe:3d} NFE  {t * 1e3:9.1f} ms/batch  {B / t:8.2f} images/s  {1e3 * t / nfe:7.2f} ms/NFE")
    if len(runs) == 2:
        res["ms_per_nfe_ratio_heun_over_dxmi"] = round(res["heun"]["ms_per_nfe"] / res["dxmi"]["ms_per_nfe"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
