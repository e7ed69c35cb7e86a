"""Throughput of the consistency-model samplers and zero-shot super-resolution next to the DxMI sampler on the same net, and
the time of one dxmi_cm_stage launch per edit kind.

In ONE process, alternating: onestep (1 network evaluation per image), multistep with --ts (len(ts) - 1), iterative_superres
with the same ts (not graph-replayed: the editing loops run eagerly), and OpenAIDiffusion T=4 (the imagenet64_T4 sampler
config), all on the full-size ImageNet-64 U-Net (295.9 M parameters, fp16 config, synthetic weights, distillation=True for the
consistency samplers) at the same batch.  Prints ms per batch and per network evaluation (NFE), the median over --rounds.
Then, unless --no_stage, times dxmi_cm_stage alone at the batch's shape for every edit kind (median of 200 launches, events)
against its HBM floor (bytes moved / 8 TB/s).  One JSON line at the end.

    python tools/cm_sample_time.py [--batch 100] [--rounds 3] [--ts 0,22,39]
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/cm_sample_time.py --rounds 1 --no_stage
      (the stage kernels' share: cm_*_kernel against the total kernel time, from the run's kernel_stats)
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

HBM_BYTES_PER_S = 8.0e12


def stage_times(B, shape, dev):
    """Median time of one non-last dxmi_cm_stage launch per edit kind; -> {kind: (us, floor_us)}."""
    from dxmi_hip import ops
    from models.cm.karras_diffusion import colour_basis, patch_basis
    shape = (B,) + tuple(shape)
    g = torch.Generator(device=dev).manual_seed(0)
    x, F, z, ref = (torch.randn(shape, device=dev, generator=g) for _ in range(4))
    mask = (torch.rand(shape, device=dev, generator=g) > 0.5).float()
    x_in, t = torch.empty_like(x), torch.empty(B, device=dev)
    tab = torch.zeros(2, ops.CT_COLS, device=dev)
    tab[1] = torch.tensor([0.1, 0.5, 0.8, 0.7, 20.0, 1.0, 1.0, 0.0])
    kinds = {"none": (ops.CM_EDIT_NONE, None, None, None), "mask": (ops.CM_EDIT_MASK, None, ref, mask),
             "colour": (ops.CM_EDIT_COLOUR, colour_basis().to(dev), ref, None),
             "patch": (ops.CM_EDIT_PATCH, patch_basis().to(dev), ref, None)}
    n = x.numel() * 4
    res = {}
    for name, (edit, Q, r, m) in kinds.items():
        # reads x, F, z (+ ref, + mask); writes x, x_in
        moved = n * (5 + (r is not None) + (m is not None))
        for _ in range(10):
            ops.cm_stage(ops.CM_STEP, False, tab, 1, x, edit=edit, Q=Q, model_out=F, noise=z, ref=r, mask=m, x_in=x_in, t=t)
        ts = []
        for _ in range(200):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.cm_stage(ops.CM_STEP, False, tab, 1, x, edit=edit, Q=Q, model_out=F, noise=z, ref=r, mask=m, x_in=x_in, t=t)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        res[name] = {"us": round(statistics.median(ts), 2), "hbm_floor_us": round(moved / HBM_BYTES_PER_S * 1e6, 2),
                     "mbytes": round(moved / 1e6, 1)}
        print(f"dxmi_cm_stage {name:6s}: {res[name]['us']:7.2f} us/launch, HBM floor {res[name]['hbm_floor_us']:6.2f} us "
              f"({res[name]['mbytes']} MB)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ts", type=str, default="0,22,39")
    ap.add_argument("--no_stage", action="store_true")
    a = ap.parse_args()
    ts = tuple(int(v) for v in a.ts.split(","))

    import configs_builtin
    from models.cm.karras_diffusion import KarrasDenoiserFn, iterative_superres, karras_sample
    from models.cm.script_util import create_model_and_diffusion
    from models.DxMI.openai_diffusion import OpenAIDiffusion
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    cfg = configs_builtin.get("imagenet64_T10")
    unet, diffusion = create_model_and_diffusion(**cfg.diffusion)
    dxmi = OpenAIDiffusion(unet, diffusion, **configs_builtin.get("imagenet64_T4").sampler)
    unet.to(dev)
    if cfg.diffusion.use_fp16:
        unet.convert_to_fp16()
    dxmi.eval()
    dxmi.use_graph = True
    _, cm_diff = create_model_and_diffusion(**cfg.diffusion)
    cm_diff.distillation = True
    B, shape = a.batch, (a.batch,) + tuple(cfg.sampler.sample_shape)
    y = torch.randint(0, 1000, (B,), device=dev)
    images = torch.rand(shape, device=dev) * 2 - 1

    def onestep():
        return karras_sample(cm_diff, unet, shape, 40, model_kwargs={"y": y}, device=dev, sampler="onestep", use_graph=True)

    def multistep():
        return karras_sample(cm_diff, unet, shape, 40, model_kwargs={"y": y}, device=dev, sampler="multistep", ts=ts,
                             use_graph=True)

    def superres():
        x = torch.randn(shape, device=dev) * 80.0
        return iterative_superres(KarrasDenoiserFn(cm_diff, unet, True, {"y": y}), images, x, ts)[0]

    def oad():
        return dxmi.sample(B, device=dev, i_class=y)["sample"]

    runs = {"onestep": (onestep, 1), "multistep": (multistep, len(ts) - 1), "superres": (superres, len(ts) - 1),
            "dxmi_T4": (oad, 4)}
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
    res = {"batch": B, "ts": list(ts)}
    for k, (_, nfe) in runs.items():
        t = statistics.median(times[k])
        res[k] = {"nfe": nfe, "s_per_batch": round(t, 4), "images_per_s": round(B / t, 2), "ms_per_nfe": round(1e3 * t / nfe, 3),
                  "rounds_s": [round(v, 4) for v in times[k]]}
        print(f"{k:9s}: {nfe:3d} NFE  {t * 1e3:9.1f} ms/batch  {B / t:8.2f} images/s  {1e3 * t / nfe:7.2f} ms/NFE")
    res["ms_per_nfe_ratio_multistep_over_dxmi_T4"] = round(res["multistep"]["ms_per_nfe"] / res["dxmi_T4"]["ms_per_nfe"], 4)
    if not a.no_stage:
        res["stage"] = stage_times(B, cfg.sampler.sample_shape, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
