"""Host only: brute-force of the 16-byte-slot swizzle of conv_ws8_kernel's halo image (csrc/conv_ws8.hip).

An MFMA wave's B operand is one ds_read_b128 per lane: lane = 16 kg + px reads channel piece kg (16 B) of the pixel
(row (px >> 3) + ky + 2 nb, column (px & 7) + kx - 1) of its image.  A ds_read_b128 is served in four groups of 16 lanes (the
table below); a group is conflict free when its 16 lanes hit 16 different 16-byte columns of the 256-byte LDS row (or the same
address).  A layout is (row pitch in pixels, slot(piece, column, halo row)); the linear family slot = piece ^ F with
F = (m0 . v) | (m1 . v) << 1 over v = (column bits 0..2, halo-row bit 0) is searched completely.

  python tools/ws8_swizzle.py        prints the conflict-free members for pitch 10 (the old image), 9 and 8, and checks the
                                     layout the kernel uses (pitch 8, F = (column & 4) >> 1, lanes outside columns 0..7
                                     redirected to a zero strip with the low address bits of the slot they replace)
"""
import itertools
import sys

GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
          list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
GROUPS += [[l + 32 for l in g] for g in GROUPS]


def parity(x):
    return bin(x).count("1") & 1


def F_linear(m0, m1):
    def F(col, hy):
        v = (col & 7) | ((hy & 1) << 3)
        return parity(m0 & v) | (parity(m1 & v) << 1)
    return F


def conflicts(pitch, F, strip):
    """worst number of distinct addresses on one 16-byte column within a lane group, over the nine taps and four row pairs.
    pitch 10 / 9: halo column hx = column + 1 is stored (pitch 9: column 8 is the next row's column -1);
    pitch 8 (strip=True): columns -1 and 8 read a zero strip at the same (column & 3, slot) position."""
    worst = 1
    for ky, kx, nb in itertools.product(range(3), range(3), range(4)):
        for grp in GROUPS:
            cols = {}
            for lane in grp:
                px, kg = lane & 15, lane >> 4
                hy = (px >> 3) + ky + 2 * nb
                col = (px & 7) + kx - 1
                if pitch == 8:
                    slot = kg ^ F(col, hy)
                    inside = 0 <= col < 8
                    assert inside or strip
                    base = 0 if inside else 1 << 20                    # strip: another region, same low bits
                    a = base + hy * 512 + (col & (7 if inside else 3)) * 64 + slot * 16
                else:
                    hx = col + 1
                    if pitch == 9 and hx == 9: hx, hy = 0, hy + 1       # the shared pad slot
                    a = (hy * pitch + hx) * 64 + (kg ^ F(hx, hy)) * 16
                cols.setdefault((a >> 4) & 15, set()).add(a)
            worst = max(worst, max(len(s) for s in cols.values()))
    return worst


def main():
    ok = True
    old = conflicts(10, lambda hx, hy: hx & 2, False)
    print(f"pitch 10, slot = piece ^ (hx & 2) (the image before this change): worst {old}-way")
    ok &= old == 1
    for pitch in (10, 9, 8):
        free, free_rowless = [], []
        for m0, m1 in itertools.product(range(16), repeat=2):
            if conflicts(pitch, F_linear(m0, m1), True) == 1:
                free.append((m0, m1))
                if not ((m0 | m1) & 8): free_rowless.append((m0, m1))
        print(f"pitch {pitch}: {len(free)} of 256 linear swizzles are conflict free, {len(free_rowless)} of them without the row bit")
        if pitch == 8: print("   without the row bit, (m0, m1) over column bits 0..2:", free_rowless)
    new = conflicts(8, lambda col, hy: (col & 4) >> 1, True)
    print(f"pitch 8, slot = piece ^ ((column & 4) >> 1), zero strip for columns -1 and 8 (the kernel's image): worst {new}-way")
    ok &= new == 1
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
