"""The bits of the DDPM teacher's samplers, as SHA-256 digests: single dxmi_ddpm_stage / dxmi_dpm_stage launches on seeded operands,
then one ddpm_sample and one dpm_sample run, eager and replayed.  Two builds of the library (DXMI_LIB names another one, dxmi_hip/
_lib.py) compute the same thing exactly when the two outputs are byte-identical.

    python tools/stage_bits.py [--out FILE]

Launches: per schedule and shape the rows 0, 1, 2 and the last run one after the other, each on fresh copies of that row's operands,
and every output tensor (x', t_out, out, pred_xstart, and dxmi_dpm_stage's whole history ring) goes into a digest of its own,
  z      by value, the noise given
  fused  by value, the noise made in the launch (sample_index, seed, draw)
  ctl    the same launch with row, draw and seed read from the control block
DDPM: {clip, linear} x {small, large} and one eta = 0 schedule; DPM: ODE order 3 and SDE order 2, x {clip, no clip}; 10 steps;
[N, CHW] = [3, 75], [5, 3072], [1, 263347] (the last one: a second trip of the grid-stride loop, the unaligned path and the tail).
Samplers: the analytic network 0.8 tanh(0.9 x + 1e-3 t) at [4, 3, 8, 8], 10 steps, generator "determ".  Prints one JSON document.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
STEPS = 10
ROWS = (0, 1, 2, STEPS - 1)
SHAPES = ((3, 75), (5, 3072), (1, 263347))
SEED, DRAW = (1 << 40) + 12345, 3
INDEX = [5, (1 << 33) + 7, 123456, 0, 99]


def operands(N, CHW, seed, hist):
    gen = torch.Generator().manual_seed(seed)
    x, eps, z = (torch.randn(N, CHW, generator=gen) for _ in range(3))
    h = torch.rand(3, N, CHW, generator=gen) * 2 - 1 if hist else None
    return x, eps, z, h


def control(row, draw, seed):
    return torch.from_numpy(np.array([row, draw, seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32).view(np.int32)).to(DEV)


def stage_digests(ops, stage, step, tab, N, CHW, mode, hist):
    names = ("x", "t_out", "out", "pred_xstart") + (("hist",) if hist else ())
    sums = {k: hashlib.sha256() for k in names}
    idx = torch.tensor(INDEX[:N], dtype=torch.int64, device=DEV)
    for row in ROWS:
        x, eps, z, h = operands(N, CHW, 1000 * row + CHW, hist)
        got = {"x": x.to(DEV), "t_out": torch.full((N,), -5.0, device=DEV), "out": torch.full((N, CHW), 7.0, device=DEV),
               "pred_xstart": torch.full((N, CHW), 9.0, device=DEV)}
        kw = {"hist": h.to(DEV)} if hist else {}
        got.update(kw)
        if mode == "z":
            kw.update(row=row, z=z.to(DEV))
        elif mode == "fused":
            kw.update(row=row, sample_index=idx, seed=SEED, draw=DRAW + row)
        else:
            kw.update(ctl=control(row, DRAW + row, SEED), sample_index=idx)
        stage(step, tab, got["t_out"], x=got["x"], eps=eps.to(DEV), out=got["out"], pred_xstart=got["pred_xstart"], **kw)
        torch.cuda.synchronize()
        for k in names:
            sums[k].update(got[k].cpu().numpy().tobytes())
    return {k: v.hexdigest() for k, v in sums.items()}


def launches(ops):
    from models.DxMI.ddpm_sample import ddpm_sample_schedule
    from models.DxMI.dpm_sample import dpm_sample_schedule
    ddpm = {f"ddpm_{'clip' if clip else 'linear'}_{var}": ddpm_sample_schedule(STEPS, 1.0 if var == "large" else 0.7, var,
                                                                               clip_denoised=clip)
            for clip in (True, False) for var in ("small", "large")}
    ddpm["ddpm_clip_eta0"] = ddpm_sample_schedule(STEPS, 0.0)
    dpm = {f"dpm_{name}_{'clip' if clip else 'noclip'}": dpm_sample_schedule(STEPS, order, alg, clip_denoised=clip)
           for name, order, alg in (("ode3", 3, "dpmsolver++"), ("sde2", 2, "sde-dpmsolver++")) for clip in (True, False)}
    out = {}
    for stage, step, schedules, hist in ((ops.ddpm_stage, ops.DDPM_STEP, ddpm, False), (ops.dpm_stage, ops.DPM_STEP, dpm, True)):
        for name, sch in schedules.items():
            for N, CHW in SHAPES:
                for mode in ("z", "fused", "ctl"):
                    out[f"{name} [{N}, {CHW}] {mode}"] = stage_digests(ops, stage, step, sch.device_table(DEV), N, CHW, mode, hist)
    return out


def analytic_net(x, t):
    return 0.8 * torch.tanh(0.9 * x + 1e-3 * t[:, None, None, None])


def samplers():
    from models.cm.random_util import get_generator
    from models.DxMI import ddpm_sample, dpm_sample
    out = {}
    runs = (("ddpm_sample", ddpm_sample.ddpm_sample, ddpm_sample.replay_graphs, {}),
            ("dpm_sample", dpm_sample.dpm_sample, dpm_sample.replay_graphs, dict(algorithm="sde-dpmsolver++", order=2)))
    for name, fn, graphs, kw in runs:
        for use_graph in (False, True):
            gen = get_generator("determ", 64, 7)
            x = fn(analytic_net, (4, 3, 8, 8), steps=STEPS, device=DEV, generator=gen, use_graph=use_graph, **kw)
            torch.cuda.synchronize()
            out[f"{name} {'replay' if use_graph else 'eager'}"] = hashlib.sha256(x.cpu().numpy().tobytes()).hexdigest()
        out[f"{name} replays"] = sum(g.replays for g in graphs(analytic_net))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from dxmi_hip import ops
    ops.device_check()
    text = json.dumps({"launches": launches(ops), "samplers": samplers()}, indent=1, sort_keys=True)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
