"""GPU box: same-box A/B of conv_ws8_kernel builds, arms alternated.

  python tools/conv_ws8_ab.py [--rounds R] [--out FILE.json] label=LIB[:DBG] ...

Every arm is a library build (tools/build_variant.sh) selected through DXMI_LIB, optionally with the timing-only ablation bits
of a diagnostic build (DXMI_CONV_WS8_DBG: 1 no weight stream, 2 no halo stream, 4 no step barriers — wrong results).  Each
round runs every arm once, each in a fresh process, in the order given; a process times graph-captured launches of 256 images at
the four shapes the CIFAR-10 net runs on this kernel.  The table is the best round per arm and shape, in microseconds."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["256->256 +res", "256->256 GN out", "256+256->256 GN out", "up 4x4->8x8 256->256"]


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "diffusion-by-maxentirl_amd")]
    import torch
    from dxmi_hip import ops
    dev, N, C = "cuda:0", 256, 256
    torch.manual_seed(0)

    def graph_time(fn, n=20):
        for _ in range(3): fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(n): fn()
        best = 1e9
        for _ in range(5):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / n * 1e3)
        return best

    rnd = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
    x8, x8b, x4, r = rnd(N, 8, 8, C), rnd(N, 8, 8, C), rnd(N, 4, 4, C), rnd(N, 8, 8, C)
    pw = ops.pack_conv_weight(torch.randn(C, C, 3, 3, device=dev) * 0.03)
    pw2 = ops.pack_conv_weight(torch.randn(C, 2 * C, 3, 3, device=dev) * 0.02)
    b, v = torch.randn(C, device=dev), torch.randn(N, C, device=dev)
    gn = (torch.ones(C, device=dev), torch.zeros(C, device=dev), 32, 1e-6, True, False)
    out = torch.empty(N, 8, 8, C, device=dev, dtype=torch.bfloat16)
    fns = [lambda: ops.conv2d(x8, pw, bias=b, addvec=v, residual=r, out=out),
           lambda: ops.conv2d(x8, pw, bias=b, addvec=v, fuse_gn=gn),
           lambda: ops.conv2d(x8, pw2, in1=x8b, bias=b, addvec=v, fuse_gn=gn),
           lambda: ops.conv2d(x4, pw, bias=b, upsample=True, out=out)]
    assert fns[1]()[1] is not None, "the fused GroupNorm output is not available in this build"
    print("AB " + json.dumps([round(graph_time(f), 2) for f in fns]), flush=True)


def main(argv):
    rounds, out, arms = 3, None, []
    it = iter(argv)
    for a in it:
        if a == "--rounds": rounds = int(next(it))
        elif a == "--out": out = next(it)
        else:
            label, spec = a.split("=", 1)
            lib, _, dbg = spec.partition(":")
            arms.append((label, os.path.abspath(lib), dbg))
    if not arms:
        sys.exit(__doc__)
    runs = {label: [] for label, _, _ in arms}
    for _ in range(rounds):
        for label, lib, dbg in arms:
            env = dict(os.environ, DXMI_LIB=lib)
            env.pop("DXMI_CONV_WS8_DBG", None)
            if dbg: env["DXMI_CONV_WS8_DBG"] = dbg
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=240)
            line = [l for l in p.stdout.splitlines() if l.startswith("AB ")]
            if p.returncode != 0 or not line:
                sys.exit(f"arm {label} failed (exit {p.returncode}); no further arm is started\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[label].append(json.loads(line[0][3:]))
            print(label, runs[label][-1], flush=True)
    print(f"\n{'arm':<16}" + "".join(f"{s:>24}" for s in SHAPES))
    for label, _, _ in arms:
        print(f"{label:<16}" + "".join(f"{min(r[i] for r in runs[label]):>24.1f}" for i in range(len(SHAPES))))
    if out:
        with open(out, "w") as f:
            json.dump({"shapes": SHAPES, "unit": "us per launch, graph-captured, N=256", "runs": runs}, f, indent=1)


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main(sys.argv[1:])
