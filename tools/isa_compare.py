"""Compares the gfx950 device code two trees compile from the same HIP sources: python tools/isa_compare.py OLD_TREE NEW_TREE
[-o OUT.json] [source.hip ...]

Host only (hipcc cross-compiles; no GPU).  Each listed source of <tree>/diffusion-by-maxentirl_amd/csrc (default: the ten
wave-specialised sources) is compiled to device-only assembly, `hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S`
plus -D flags given with -D.  Per source the tool reports
  * whether the two assembly files are identical once the .ident / .file lines and the hash in the compilation unit's
    __hip_cuid_<hash> symbol (a hash of the source text) are dropped;
  * per kernel symbol the resource metadata of both sides (VGPR, SGPR, AGPR, spills, private segment, fixed LDS) and whether
    they are equal;
  * per kernel the instruction count per mnemonic where the two sides differ;
  * per kernel the number of differing lines after register names are normalised (v12, s[4:5], a3 -> v, s, a), and for each
    differing hunk the label it follows and its distance from the kernel's first line, so that it can be found in the listing.
It compares two builds and looks for no particular instruction."""
import argparse
import collections
import difflib
import json
import os
import re
import subprocess
import sys
import tempfile

SOURCES = ["conv_ws.hip", "conv_ws8.hip", "conv_ws_up.hip", "conv_sm.hip", "conv1x1_rw.hip", "conv1x1_rw8.hip", "conv_head.hip",
           "conv_wgrad.hip", "attention.hip", "attn_block.hip"]
META = {"vgpr": ".vgpr_count", "sgpr": ".sgpr_count", "agpr": ".agpr_count", "vgpr_spill": ".vgpr_spill_count",
        "sgpr_spill": ".sgpr_spill_count", "private_segment": ".private_segment_fixed_size", "lds": ".group_segment_fixed_size"}
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")


def compile_asm(tree, src, defs, out):
    csrc = os.path.join(tree, "diffusion-by-maxentirl_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, *defs, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                       cwd=csrc, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit(f"{tree}: {src} does not compile\n{r.stderr}")
    with open(out) as f:      # __hip_cuid_<hash>: the compilation unit's id symbol, a hash of the source file
        return [CUID.sub("__hip_cuid", l.rstrip("\n")) for l in f if not l.lstrip().startswith((".ident", ".file"))]


def metadata(lines):
    """kernel symbol -> resource fields, from the amdhsa.kernels metadata at the end of the file"""
    kernels, cur = {}, {}
    for l in lines:
        s = l.strip().lstrip("- ")
        for key, tag in META.items():
            if s.startswith(tag + ":"):
                cur[key] = int(s.split(":")[1])
        if s.startswith(".name:"):
            cur["name"] = s.split(":", 1)[1].strip()
        if s.startswith(".wavefront_size:") and "name" in cur:     # last field of a kernel's entry (sorted keys)
            kernels[cur.pop("name")] = cur
            cur = {}
    return kernels


def bodies(lines):
    """kernel symbol -> its lines (comments dropped) between the symbol's label and s_endpgm's .Lfunc_end"""
    out, name, body = {}, None, []
    for l in lines:
        code = l.split(";")[0].rstrip()
        if not code.strip():
            continue
        m = re.match(r"^(\w+):", code)
        if m and not code.startswith(".L"):
            name, body = m.group(1), []
            continue
        if name and code.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if name and (code.startswith(".L") or not code.strip().startswith(".")):      # labels and instructions, no directives
            body.append(code.strip())
    return out


def mnemonics(body):
    return collections.Counter(l.split()[0] for l in body if not l.endswith(":"))


def hunks(a, b):
    na, nb = [REG.sub(r"\1", l) for l in a], [REG.sub(r"\1", l) for l in b]
    res, n = [], 0
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, na, nb, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        label = next((a[i] for i in range(i1 - 1, -1, -1) if a[i].endswith(":")), "(kernel entry)")
        n += max(i2 - i1, j2 - j1)
        res.append({"old_line": i1, "of": len(a), "after_label": label, "old": a[i1:i2][:6], "new": b[j1:j2][:6]})
    return n, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("sources", nargs="*", default=SOURCES)
    ap.add_argument("-o", "--out")
    ap.add_argument("-D", dest="defs", action="append", default=[])
    a = ap.parse_intermixed_args()
    defs = ["-D" + d for d in a.defs]
    report, ok = {}, True
    with tempfile.TemporaryDirectory() as tmp:
        for src in a.sources:
            old = compile_asm(a.old, src, defs, os.path.join(tmp, "old.s"))
            new = compile_asm(a.new, src, defs, os.path.join(tmp, "new.s"))
            row = report[src] = {"identical": old == new, "asm_lines": [len(old), len(new)], "kernels": {}}
            mo, mn, bo, bn = metadata(old), metadata(new), bodies(old), bodies(new)
            for k in sorted(set(mo) | set(mn)):
                co, cn = mnemonics(bo.get(k, [])), mnemonics(bn.get(k, []))
                ndiff, hs = (0, []) if row["identical"] else hunks(bo.get(k, []), bn.get(k, []))
                row["kernels"][k] = {"metadata_old": mo.get(k), "metadata_new": mn.get(k), "metadata_equal": mo.get(k) == mn.get(k),
                                     "instructions": [sum(co.values()), sum(cn.values())],
                                     "mnemonic_counts_differ": {m: [co[m], cn[m]] for m in sorted(set(co) | set(cn)) if co[m] != cn[m]},
                                     "differing_lines": ndiff, "hunks": hs}
                ok = ok and mo.get(k) == mn.get(k)
            print(f"{src}: {'identical' if row['identical'] else 'DIFFERS'}", flush=True)
            for k, v in row["kernels"].items():
                m = v["metadata_new"] or {}
                print(f"  {k}: vgpr {m.get('vgpr')} sgpr {m.get('sgpr')} agpr {m.get('agpr')} spills {m.get('vgpr_spill')}/{m.get('sgpr_spill')} "
                      f"private {m.get('private_segment')} lds {m.get('lds')} | metadata {'equal' if v['metadata_equal'] else 'DIFFERS'}, "
                      f"{v['differing_lines']} differing lines in {len(v['hunks'])} hunks, mnemonic counts {v['mnemonic_counts_differ'] or 'equal'}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
