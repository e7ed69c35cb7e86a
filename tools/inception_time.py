"""Throughput of the FID / evaluator InceptionV3 in both precisions on one MI355X: images/s of the bf16 and the fp32
program at batch 50 and 250 from 32x32 inputs (resize to 299 included; formula weights), and the per-launch time of the five conv
shapes that carry the most FLOP at batch 50, again in both precisions.  Device events around `inner` back-to-back calls after a
warm-up call, median over `reps` such groups.  One JSON line per case; the fp32 rows carry the arithmetic floor (11.5 GFLOP per
image, 157 TFLOP/s f32 matrix peak) and the fp32 / bf16 time ratio (the two MFMA rates differ by 16).
    python tools/inception_time.py [--reps 5] [--batches 50,250] [--out results/inception_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))
sys.path.insert(0, ROOT)
from dxmi_hip import inception_f32_ops, ops  # noqa: E402
from pytorch_fid.inception import InceptionV3  # noqa: E402

PEAK_F32 = 157.3e12


def formula_state_dict(model):
    """He-scaled conv weights, BatchNorm statistics near identity: activations stay O(1) through the net (seeded torch draws)."""
    g = torch.Generator().manual_seed(0)
    sd = {}
    for name, c in model._convs():
        fan_in = c.conv.weight[0].numel()
        n = c.bn.weight.numel()
        sd[name + ".conv.weight"] = torch.randn(c.conv.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5
        sd[name + ".bn.weight"] = 1.0 + 0.2 * (2 * torch.rand(n, generator=g) - 1)
        sd[name + ".bn.bias"] = 0.1 * (2 * torch.rand(n, generator=g) - 1)
        sd[name + ".bn.running_mean"] = 0.1 * (2 * torch.rand(n, generator=g) - 1)
        sd[name + ".bn.running_var"] = 1.0 + 0.3 * torch.rand(n, generator=g)
        sd[name + ".bn.num_batches_tracked"] = torch.tensor(0)
    return sd


def timed(fn, reps, inner=1):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return sorted(ts)[len(ts) // 2]


def conv_shapes(model, x):
    """Every gconv launch of one fp32 forward: (N, IH, IW, Cin, Cout, KH, KW, stride, pad) -> [launches, FLOP of all of them]."""
    seen, real = {}, inception_f32_ops.gconv

    def spy(x, pk, stride=(1, 1), pad=(0, 0), relu=True, out=None, coff=0):
        out = real(x, pk, stride=stride, pad=pad, relu=relu, out=out, coff=coff)
        N, IH, IW, _ = x.shape
        key = (N, IH, IW, pk.Cin, pk.Cout, pk.KH, pk.KW, tuple(stride), tuple(pad))
        e = seen.setdefault(key, [0, 0.0])
        e[0] += 1
        e[1] += 2.0 * N * out.shape[1] * out.shape[2] * pk.Cout * pk.Cin * pk.KH * pk.KW
        return out
    inception_f32_ops.gconv = spy
    try:
        model(x)
    finally:
        inception_f32_ops.gconv = real
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="50,250")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops.device_check()
    model = InceptionV3()
    model.load_fid_weights(formula_state_dict(model))
    model = model.cuda()
    rows = []
    for B in (int(v) for v in a.batches.split(",")):
        x = torch.rand(B, 3, 32, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
        ms = {}
        for prec in ("bf16", "fp32"):
            model.precision = prec
            ms[prec] = timed(lambda: model(x), a.reps)
        if B == 50:
            shapes = conv_shapes(model, x)                         # model.precision is fp32 here
            flop_per_image = sum(e[1] for e in shapes.values()) / B
        for prec in ("bf16", "fp32"):
            r = dict(case=f"forward_{prec}_b{B}", batch=B, ms=ms[prec], images_per_s=B / ms[prec] * 1e3)
            if prec == "fp32":
                r.update(floor_ms=B * 11.5e9 / PEAK_F32 * 1e3, ratio_to_bf16=ms["fp32"] / ms["bf16"])
            rows.append(r)
    rows.append(dict(case="conv_flop_per_image", gflop=flop_per_image / 1e9, conv_launches=sum(e[0] for e in shapes.values())))
    g = torch.Generator(device="cuda").manual_seed(1)
    for key, (count, flop) in sorted(shapes.items(), key=lambda kv: -kv[1][1])[:5]:
        N, IH, IW, Cin, Cout, KH, KW, stride, pad = key
        w = torch.randn(Cout, Cin, KH, KW, device="cuda", generator=g) * (2.0 / (Cin * KH * KW)) ** 0.5
        x32 = torch.zeros(N, IH, IW, -(-Cin // inception_f32_ops.GRANULE) * inception_f32_ops.GRANULE, device="cuda")
        x32[..., :Cin] = torch.randn(N, IH, IW, Cin, device="cuda", generator=g)
        one = flop / count
        t32 = timed(lambda pk=inception_f32_ops.gconv_pack(w): inception_f32_ops.gconv(x32, pk, stride=stride, pad=pad), a.reps, inner=10)
        x16 = torch.zeros(N, IH, IW, -(-Cin // 16) * 16, dtype=torch.bfloat16, device="cuda")
        x16[..., :Cin] = x32[..., :Cin].to(torch.bfloat16)
        t16 = timed(lambda pk=ops.gconv_pack(w): ops.gconv(x16, pk, stride=stride, pad=pad), a.reps, inner=10)
        rows.append(dict(case=f"conv_{IH}x{IW}x{Cin}->{Cout}_k{KH}x{KW}_s{stride[0]}", batch=N, launches_per_forward=count, gflop=one / 1e9,
                         fp32_ms=t32, fp32_tflops=one / t32 / 1e9, fp32_floor_ms=one / PEAK_F32 * 1e3, bf16_ms=t16, ratio_to_bf16=t32 / t16))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
