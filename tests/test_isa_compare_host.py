"""tools/isa_compare.py on two hand-written listings (host only, no compiler): the metadata fields per kernel, the kernel bodies
without directives and comments, and the differing lines once register names are normalised."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(ROOT, "tools", "isa_compare.py"))
isa = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa)

LISTING = """\t.text
\t.globl\tkern_a
\t.type\tkern_a,@function
kern_a:                                 ; @kern_a
; %bb.0:
\ts_load_dword s4, s[0:1], 0x0
\tv_mov_b32_e32 v1, 0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tv_add_u32_e32 v1, v1, v0            ; a comment
\ts_cmp_lt_i32 s5, s4
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
\t.section\t.rodata
.Lfunc_end0:
\t.size\tkern_a, .Lfunc_end0-kern_a
\t.amdgpu_metadata
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .name:           p
        .size:           8
    .group_segment_fixed_size: 64
    .name:           kern_a
    .private_segment_fixed_size: 12
    .sgpr_count:     10
    .sgpr_spill_count: 1
    .symbol:         kern_a.kd
    .vgpr_count:     2
    .vgpr_spill_count: 3
    .wavefront_size: 64
"""


def test_metadata_and_bodies():
    lines = LISTING.splitlines()
    assert isa.metadata(lines) == {"kern_a": {"agpr": 0, "lds": 64, "private_segment": 12, "sgpr": 10, "sgpr_spill": 1, "vgpr": 2,
                                              "vgpr_spill": 3}}
    body = isa.bodies(lines)["kern_a"]
    assert body == ["s_load_dword s4, s[0:1], 0x0", "v_mov_b32_e32 v1, 0", ".LBB0_1:", "v_add_u32_e32 v1, v1, v0", "s_cmp_lt_i32 s5, s4",
                    "s_cbranch_scc1 .LBB0_1", "s_endpgm"]
    assert isa.mnemonics(body)["s_cmp_lt_i32"] == 1 and ".LBB0_1:" not in isa.mnemonics(body)


def test_register_names_do_not_count_and_a_flipped_branch_does():
    old = isa.bodies(LISTING.splitlines())["kern_a"]
    renamed = isa.bodies(LISTING.replace("v1", "v7").replace("s[0:1]", "s[2:3]").splitlines())["kern_a"]
    assert isa.hunks(old, renamed) == (0, [])
    flipped = isa.bodies(LISTING.replace("s_cmp_lt_i32", "s_cmp_ge_i32").replace("s_cbranch_scc1", "s_cbranch_scc0").splitlines())["kern_a"]
    n, hs = isa.hunks(old, flipped)
    assert n == 2 and len(hs) == 1 and hs[0]["after_label"] == ".LBB0_1:" and hs[0]["old"] == ["s_cmp_lt_i32 s5, s4", "s_cbranch_scc1 .LBB0_1"]
