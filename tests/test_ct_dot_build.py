"""CPU-side checks of the grouped product sums: the entries are declared, exported and wrapped (what the kernels compile to:
tests/test_ct_ops_build.py); the example is plain C (no GPU needed)."""
import os

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_ct_mul_sum_device", "se_amd_ct_dot_sp_device")
METHODS = ("ct_mul_sum", "ct_dot_sp")


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    assert "NOT the modular sum of" in text and "se_amd_ct_mul_sum_device followed by se_amd_ct_relin_sp_device" in text


def test_dot_product_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "dot_product_roundtrip.c"), tmp_path, hip=True)
