"""Bits of the wave-specialised 3x3 conv kernels: python tools/conv_ws_bits.py OUT.json

For a fixed case list: one ops.conv2d per case on seeded operands, recorded as the kernel id the library names for the descriptor
and the SHA-256 of every output (the raw tensor, the GroupNorm block statistics, the fused GroupNorm output, where the case asks
for them).  Run against two builds of the library (DXMI_LIB=<other libdxmi_hip.so> selects one), the two OUT.json are byte-identical
exactly when both compute the same bits with the same kernels.  Small-grid re-routing is off (conv_ws_min_tiles 0), so every case
stays in the family.

Cases (kernel: what it reaches):
  conv_ws_kernel<16> / <32> (16x16 / 32x32 maps): 64, 128 and 256 channels in (64 = two chunks is below the family's four-chunk
    minimum and runs the generic kernel: its id says so; 128 / 256 = 12 / 24 groups per tile); a virtual concat (128 + 64); Cout 192
    (half-empty last cout tile: clamped weight fragments, masked residual pieces) with a residual and statistics; a residual;
    an activation mask with LeakyReLU; statistics; and one launch of more tiles than the 256 workgroups (130 / 33 images x 2 cout
    tiles = 260 / 264) with bias, per-image vector, residual and statistics: tile switch, ahead-of-time group 0, loader-side
    residual DMAs and table refetch.
  conv_ws_gn_kernel<16>: SiLU on and off, and 260 tiles.
  conv_ws8_kernel<false> / <true> (8x8 maps): N = 4 and N = 5 (a tile whose images run past the batch), the 4x4 -> 8x8 upsample, a
    residual, 260 tiles with a residual; the fused GroupNorm form with N = 4 (SiLU), N = 5 (no SiLU) and 260 tiles.
  conv_ws_up_kernel<32> / <16>: tests/test_hip_conv_ws_up.py's two map sizes (16x16 -> 32x32, 8x8 -> 16x16), each with bias,
    per-image vector, residual and statistics, and with more tiles than workgroups (17 / 129 images)."""
import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diffusion-by-maxentirl_amd"), os.path.join(ROOT, "tests")]
import torch
from dxmi_hip import ops
from forward_bounds import launch_conv

DEV = "cuda:0"


def case(name, H, N, C0, Cout, C1=0, bias=True, vec=False, res=False, mask=False, act=0, stats=False, ups=False, gn=None):
    return dict(name=name, H=H, N=N, C0=C0, C1=C1, Cout=Cout, bias=bias, vec=vec, res=res, mask=mask, act=act, stats=stats, ups=ups, gn=gn)


def family(tag, H, big):
    return [case(f"{tag}_c64", H, 2, 64, 128), case(f"{tag}_c128", H, 2, 128, 128, vec=True), case(f"{tag}_c256", H, 2, 256, 128, bias=False),
            case(f"{tag}_concat", H, 2, 128, 128, C1=64), case(f"{tag}_cout192_res_stats", H, 3, 128, 192, res=True, stats=True),
            case(f"{tag}_res", H, 2, 128, 128, res=True), case(f"{tag}_mask_leaky", H, 2, 128, 128, mask=True, act=ops.ACT_LEAKY02),
            case(f"{tag}_stats", H, 2, 128, 256, vec=True, stats=True),
            case(f"{tag}_two_tiles", H, big, 128, 256, vec=True, res=True, stats=True)]


CASES = (family("ws16", 16, 130) + family("ws32", 32, 33) + [
    case("gn16_silu", 16, 2, 128, 128, vec=True, gn=True), case("gn16_plain", 16, 3, 256, 256, gn=False),
    case("gn16_two_tiles", 16, 130, 128, 256, vec=True, gn=True),
    case("ws8_n4", 8, 4, 128, 128, vec=True), case("ws8_n5", 8, 5, 128, 128, vec=True), case("ws8_ups", 8, 4, 128, 128, ups=True),
    case("ws8_n5_res", 8, 5, 256, 128, res=True), case("ws8_two_tiles", 8, 260, 128, 256, vec=True, res=True),
    case("ws8gn_n4_silu", 8, 4, 128, 128, vec=True, gn=True), case("ws8gn_n5_plain", 8, 5, 128, 256, gn=False),
    case("ws8gn_two_tiles", 8, 260, 128, 256, vec=True, gn=True),
    case("up32", 32, 3, 256, 256, vec=True, res=True, stats=True, ups=True), case("up32_two_tiles", 32, 17, 128, 256, vec=True, res=True, stats=True, ups=True),
    case("up16", 16, 3, 256, 256, vec=True, res=True, stats=True, ups=True), case("up16_two_tiles", 16, 129, 128, 256, vec=True, res=True, stats=True, ups=True)])


def sha(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run(i, c):
    g = torch.Generator().manual_seed(9000 + i)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(DEV)
    f32 = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    H, N, Cin, Cout = c["H"], c["N"], c["C0"] + c["C1"], c["Cout"]
    IH = H // 2 if c["ups"] else H
    x0 = bf(N, IH, IH, c["C0"])
    kw = dict(in1=bf(N, IH, IH, c["C1"]) if c["C1"] else None, upsample=c["ups"], act=c["act"])
    pw = ops.pack_conv_weight(f32(Cout, Cin, 3, 3, scale=1 / math.sqrt(9 * Cin)))
    if c["bias"]:
        kw["bias"] = f32(Cout, scale=0.1)
    if c["vec"]:
        kw["addvec"] = f32(N, Cout, scale=0.3)
    if c["res"]:
        kw["residual"] = bf(N, H, H, Cout)
    if c["mask"]:
        kw.update(mask_src=bf(N, H, H, Cout), mask_slope=0.2)
    row = {"name": c["name"]}
    if c["gn"] is not None:
        kw.update(fuse_gn=(1 + f32(Cout, scale=0.3), f32(Cout, scale=0.3), Cout // 8, 1e-6, c["gn"], False), gn_ws=True)
        (raw, y), kid = launch_conv(ops, x0, pw, **kw)
        row.update(out=sha(raw), gn_out=sha(y))
    elif c["stats"]:
        (raw, st), kid = launch_conv(ops, x0, pw, want_stats=True, **kw)
        row.update(out=sha(raw), gn_stats=sha(st.buf) if st is not None else None)
    else:
        raw, kid = launch_conv(ops, x0, pw, **kw)
        row.update(out=sha(raw))
    torch.cuda.synchronize()
    row["kernel_id"] = kid
    return row


def main():
    ops.device_check()
    ops.set_tuning("conv_ws_min_tiles", 0)
    rows = []
    for i, c in enumerate(CASES):
        rows.append(run(i, c))
        print(rows[-1]["name"], rows[-1]["kernel_id"], rows[-1]["out"] and rows[-1]["out"][:16], flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "conv_ws_bits.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:      # one case per line
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
