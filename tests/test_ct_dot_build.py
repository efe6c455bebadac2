"""CPU-side checks of the grouped product sums: the entries are declared, exported and wrapped; the new kernels compile for
gfx950 without private memory, the fused one at the family's 4 waves per SIMD; no kernel of the file went missing or
gained scratch and the special-prime key switch kept its waves; the example is plain C (no GPU needed)."""
import os

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_ct_mul_sum_device", "se_amd_ct_dot_sp_device")
METHODS = ("ct_mul_sum", "ct_dot_sp")

_SP = (12, 13, 14)
_ALL = range(10, 15)
# every kernel ct_ops.hip had on the parent commit
BEFORE = (
    ["k_ct_lincomb<false>", "k_ct_lincomb<true>", "k_ct_lincomb_sum", "k_ct_mul_plain", "k_ct_mul", "k_relin_key_rows",
     "k_ct_mul_plain_sum", "k_lintrans_fold"]
    + [f"{k}<{logn}>" for k in ("k_ct_rescale", "k_ct_relin", "k_ct_galois", "k_ct_lintrans", "k_ct_galois_accum",
                                "k_bsgs_permute", "k_evk_diag_switch_sp") for logn in _ALL]
    + [f"{k}<{logn}>" for k in ("k_ct_mod_down_sp", "k_ct_galois_sp", "k_ct_relin_sp", "k_ct_switch_sp",
                                "k_ct_switch_sum_sp", "k_ct_lintrans_sp", "k_ct_galois_sum_sp",
                                "k_ct_galois_many_ext_sp", "k_ct_galois_accum_sp") for logn in _SP]
    + [f"k_ct_galois_hoist<{logn}, {s}>" for logn in _ALL for s in ("true", "false")]
    + [f"{k}<{logn}, {s}>" for k in ("k_evk_diag", "k_evk_diag_sp") for logn in _ALL for s in ("true", "false")])


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    assert "NOT the modular sum of" in text and "se_amd_ct_mul_sum_device followed by se_amd_ct_relin_sp_device" in text


def test_new_kernels_use_no_scratch_and_the_fused_one_keeps_four_waves():
    """k_ct_mul_sum is k_ct_mul with the pair loop inside and three 64-bit accumulator quads; k_ct_dot_sp<logn> is
    k_ct_relin_sp<logn> with every row it would load formed in registers, a quad at a time.  As built, logn 12 / 13 / 14:
    95 / 120 / 122 VGPRs beside the relinearisation's 113 / 115 / 119; k_ct_mul_sum 66 beside k_ct_mul's 45; no scratch
    anywhere."""
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    assert "k_ct_mul_sum" in rows, sorted(rows)
    print(f"k_ct_mul_sum: {rows['k_ct_mul_sum']}; k_ct_mul: {rows['k_ct_mul']}")
    assert rows["k_ct_mul_sum"][1] == 0
    for logn in _SP:
        k = f"k_ct_dot_sp<{logn}>"
        assert k in rows, (k, sorted(rows))
        vgpr, scratch, occ = rows[k]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD; k_ct_relin_sp<{logn}>: "
              f"{rows[f'k_ct_relin_sp<{logn}>']}")
        assert scratch == 0 and occ >= 4, (k, rows[k])


def test_no_kernel_went_missing_or_gained_scratch_and_the_key_switch_keeps_its_waves():
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    assert len(BEFORE) == len(set(BEFORE)) == len(rows) - 4          # the parent's kernels and the four new ones
    missing = [k for k in BEFORE if k not in rows]
    assert not missing, missing
    spilled = {k: rows[k] for k in BEFORE if rows[k][1] != 0}
    assert not spilled, spilled
    for logn in _SP:
        for k in (f"k_ct_relin_sp<{logn}>", f"k_ct_galois_sp<{logn}>"):
            print(f"{k}: {rows[k]}")
            assert rows[k][2] == 4, (k, rows[k])


def test_dot_product_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "dot_product_roundtrip.c"), tmp_path, hip=True)
