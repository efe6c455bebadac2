"""CPU-side checks of the ciphertext products (tensor, relinearisation key, degree-2 decrypt): the entries are declared,
exported and wrapped, the new kernels compile for gfx950 without private memory, and the product example is plain C
(no GPU needed)."""
import os
import re

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_ct_mul_device", "se_amd_decrypt3_level_device", "se_amd_decrypt3_level_keyed_device",
           "se_amd_gen_relin_key", "se_amd_set_relin_key", "se_amd_ct_relin_device")
METHODS = ("ct_mul", "decrypt3_level", "decrypt3_level_keyed", "gen_relin_key", "set_relin_key", "ct_relin")
CT_KERNELS = ("k_ct_mul", "k_relin_key_rows") + tuple(
    f"{k}<{logn}{flag}>" for k, flag in (("k_ct_relin", ""), ("k_evk_diag", ", false")) for logn in range(10, 15))
DECRYPT3_KERNELS = tuple(f"{k}<{logn}>" for k in ("k_decrypt3_full", "k_decrypt3_full_keyed") for logn in range(10, 15))


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)


def test_digit_width_is_in_the_header():
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    assert re.search(r"^#define\s+SE_AMD_RELIN_DIGIT_BITS\s+15\s*$", text, flags=re.M)


def check_no_scratch(source, kernels):
    rows = resource_rows(source)
    assert rows, f"tools/resource_usage.py gave no table for {source}"
    for k in kernels:
        assert k in rows, (k, sorted(rows))
        vgpr, scratch, occ = rows[k]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD")
        assert scratch == 0, (k, rows[k])
    return rows


def test_ct_ops_kernels_use_no_scratch():
    """The tensor kernel, every degree of the relinearisation kernel (two 16-value accumulators, the coefficient
    tile, the digit tile and two key rows per thread) and the key plumbing stay in registers -- and so does every kernel
    the file already had."""
    rows = check_no_scratch("ct_ops", CT_KERNELS)
    for k, (_, scratch, _) in rows.items():
        assert scratch == 0, (k, scratch)


def test_decrypt3_kernels_exist_without_scratch():
    """The degree-2 twins of the full-modulus decrypt exist for every degree, and the template flag costs the existing
    twins no private memory."""
    check_no_scratch("encode_encrypt", DECRYPT3_KERNELS + tuple(k.replace("decrypt3", "decrypt") for k in DECRYPT3_KERNELS))


def test_ct_product_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "ct_product_roundtrip.c"), tmp_path, hip=True)
