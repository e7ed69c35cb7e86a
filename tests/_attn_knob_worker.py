"""Child process of test_hip_forward_edges.py::test_attention_switchable_variants: the attention dispatch switches of
csrc/attention.hip (DXMI_ATTN_PF, DXMI_ATTN_GENERIC, DXMI_ATTN64, DXMI_ATTN_XCD) are read into statics once per process, so every
variant needs an interpreter of its own.  The parent sets the environment; argv[1] names the reduced table to run.  Every result is
judged by forward_bounds.attention_case (element-wise fp64 bound, two identical launches, image N - 1 alone); one JSON line of
the worst |err| / bound per tag is printed.  A result out of bound raises: the return code is then not 0."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "diffusion-by-maxentirl_amd")):
    sys.path.insert(0, p)

# table -> (the environment the parent must have set, rows (N, T, heads, D, kind, want_lse))
TABLES = {
    # attention_kernel<64, true>: block kb + 1 fetched while kb is computed, on the ragged and single-block rows of the narrow head
    "pf1_d64": ({"DXMI_ATTN_PF": "1"}, "attention_kernel<64, true>",
                [(1, 1, 1, 64, "below_zero", False), (3, 33, 1, 64, "below_zero", True), (3, 64, 3, 64, "below_zero", False),
                 (7, 65, 3, 64, "below_zero", True), (2, 129, 1, 64, "peaked", False), (2, 200, 2, 64, "below_zero", True),
                 (1, 321, 1, 64, "peaked", True), (1, 321, 1, 64, "below_zero", False)]),
    # attention_kernel<128, false>: the wide head without the prefetch
    "pf0_d128": ({"DXMI_ATTN_PF": "0"}, "attention_kernel<128, false>",
                 [(1, 64, 2, 128, "below_zero", False), (2, 65, 2, 128, "below_zero", True), (1, 130, 2, 128, "peaked", True),
                  (3, 200, 2, 128, "below_zero", False), (3, 200, 2, 128, "peaked", False)]),
    # the generic kernel where the default route has a kernel of its own: T = C = 256 single head, and D = 64 at T % 256 == 0
    "generic": ({"DXMI_ATTN_GENERIC": "1", "DXMI_ATTN64": "0"}, "generic at T256",
                [(3, 256, 1, 256, "peaked", True), (1, 256, 1, 256, "below_zero", False), (3, 256, 3, 64, "peaked", True),
                 (1, 256, 1, 64, "below_zero", False), (1, 512, 2, 64, "peaked", True)]),
    # hardware block order: grids of 1, 3, 9, 21 and 8 workgroups on the three kernels that take the permutation
    "xcd0": ({"DXMI_ATTN_XCD": "0"}, "hardware block order",
             [(1, 1, 1, 64, "below_zero", False), (3, 33, 1, 64, "below_zero", True), (7, 65, 3, 64, "below_zero", False),
              (2, 200, 2, 64, "peaked", True), (3, 256, 3, 64, "peaked", True), (3, 200, 2, 128, "below_zero", False),
              (1, 65, 1, 256, "below_zero", True)]),
}


def main():
    env, tag, rows = TABLES[sys.argv[1]]
    for k in ("DXMI_ATTN_PF", "DXMI_ATTN_GENERIC", "DXMI_ATTN64", "DXMI_ATTN_XCD"):
        assert os.environ.get(k) == env.get(k), f"{k}={os.environ.get(k)!r}: table {sys.argv[1]} wants {env.get(k)!r}"
    from dxmi_hip import ops
    from forward_bounds import FwdChecker, attention_case
    ops.device_check()
    ck = FwdChecker()
    for N, T, heads, D, kind, want_lse in rows:
        _, res = attention_case(ops, N, T, heads, D, kind, tag, want_lse=want_lse, check=ck)
        if want_lse:       # every kernel these tables reach keeps the row log-sum-exp, but for the single-head 256 x 256 shape's query
            assert (res[1] is not None) == bool(ops.load().dxmi_attention_fwd_lse_supported(T, heads * D, heads))
    print(json.dumps(ck.report()))


if __name__ == "__main__":
    main()
