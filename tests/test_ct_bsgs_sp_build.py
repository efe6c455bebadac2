"""CPU-side checks of the special-prime baby-step / giant-step transform: the entries are declared, exported and wrapped;
the two new kernels compile for gfx950 without private memory and with the waves per SIMD of the kernels they are built
from; no kernel of the file went missing and the two kernels that gained an argument kept their resources; the example is
plain C (no GPU needed)."""
import os
import re

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)
from test_ct_bsgs_build import KERNELS_BEFORE

ENTRIES = ("se_amd_ct_galois_many_ext_sp_device", "se_amd_ct_mul_plain_sum_ext_sp_device", "se_amd_ct_mod_down_sp_device",
           "se_amd_ct_galois_accum_sp_device", "se_amd_bsgs_create_sp", "se_amd_ct_bsgs_sp_device")
METHODS = ("ct_galois_many_ext_sp", "ct_mul_plain_sum_ext_sp", "ct_mod_down_sp", "ct_galois_accum_sp", "bsgs_plan_sp",
           "ct_bsgs_sp")

# (scratch bytes, waves per SIMD) of the two kernels that serve the new entries as well, from the same report on the
# parent commit: k_ct_mul_plain_sum 64 VGPRs; k_ct_rescale<10 .. 14> 95 / 101 / 131 / 125 / 127 VGPRs
PARENT = {"k_ct_mul_plain_sum": (0, 8), "k_ct_rescale<10>": (0, 5), "k_ct_rescale<11>": (0, 4), "k_ct_rescale<12>": (0, 3),
          "k_ct_rescale<13>": (0, 4), "k_ct_rescale<14>": (0, 4)}


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    assert "Out of scope: the special-prime family (it has no many form" not in text
    assert "Out of scope: the MANY form on the special-prime key" not in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+se_amd_bsgs_create_sp\s*\([^;]*se_amd_bsgs\s*\*\*\s*out\s*\)", text)


def test_new_kernels_use_no_scratch_and_keep_their_siblings_waves():
    """k_ct_galois_many_ext_sp<logn> is one pass of k_ct_galois_sum_sp<logn> with kManyExtGroup = 2 accumulator pairs;
    k_ct_galois_accum_sp<logn> is k_ct_galois_sp<logn> with the element loop inside each pass.  Each holds at least the
    waves per SIMD the same report gives its sibling, without scratch.  As built, logn 12 / 13 / 14: many_ext 123 / 124 /
    124 VGPRs beside the sum form's 122 / 115 / 126; accum_sp 122 / 119 / 121 beside the single rotation's 113 / 97 / 97;
    4 waves per SIMD each.  k_ct_mod_down_sp<logn> has the rows of k_ct_rescale<logn>: 131 / 125 / 127 VGPRs, 3 / 4 / 4
    waves."""
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    for logn in (12, 13, 14):
        for k, sibling in ((f"k_ct_galois_many_ext_sp<{logn}>", f"k_ct_galois_sum_sp<{logn}>"),
                           (f"k_ct_galois_accum_sp<{logn}>", f"k_ct_galois_sp<{logn}>"),
                           (f"k_ct_mod_down_sp<{logn}>", f"k_ct_rescale<{logn}>")):
            assert k in rows and sibling in rows, (k, sorted(rows))
            vgpr, scratch, occ = rows[k]
            print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD; {sibling}: {rows[sibling]}")
            assert scratch == 0, (k, scratch)
            assert occ >= rows[sibling][2], (k, rows[k], rows[sibling])


def test_no_kernel_went_missing_and_the_shared_ones_keep_their_resources():
    """Every kernel of the file before this block is still there.  k_ct_mul_plain_sum (now with the row -> prime map in its
    argument block) and k_ct_rescale<logn> (whose sibling k_ct_mod_down_sp takes the dropped row's prime from its arguments)
    keep the scratch and the waves per SIMD of the parent commit: 0 bytes and 8 waves (64 VGPRs); 0 bytes and 5 / 4 / 3 / 4
    / 4 waves for logn 10 .. 14."""
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    before = (list(KERNELS_BEFORE) + ["k_ct_mul_plain_sum"]
              + [f"{k}<{logn}>" for k in ("k_ct_galois_accum", "k_bsgs_permute") for logn in range(10, 15)])
    missing = [k for k in before if k not in rows]
    assert not missing, missing
    for k, (scratch, occ) in PARENT.items():
        print(f"{k}: {rows[k]}")
        assert rows[k][1] == scratch and rows[k][2] == occ, (k, rows[k])
    assert rows["k_ct_mul_plain_sum"][0] == 64, rows["k_ct_mul_plain_sum"]


def test_matvec_bsgs_fresh_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "matvec_bsgs_fresh_roundtrip.c"), tmp_path, hip=True)
