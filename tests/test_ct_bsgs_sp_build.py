"""CPU-side checks of the special-prime baby-step / giant-step transform: the entries are declared, exported and wrapped
(what the kernels compile to: tests/test_ct_ops_build.py); the example is plain C (no GPU needed)."""
import os
import re

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_ct_galois_many_ext_sp_device", "se_amd_ct_mul_plain_sum_ext_sp_device", "se_amd_ct_mod_down_sp_device",
           "se_amd_ct_galois_accum_sp_device", "se_amd_bsgs_create_sp", "se_amd_ct_bsgs_sp_device")
METHODS = ("ct_galois_many_ext_sp", "ct_mul_plain_sum_ext_sp", "ct_mod_down_sp", "ct_galois_accum_sp", "bsgs_plan_sp",
           "ct_bsgs_sp")


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    assert "Out of scope: the special-prime family (it has no many form" not in text
    assert "Out of scope: the MANY form on the special-prime key" not in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+se_amd_bsgs_create_sp\s*\([^;]*se_amd_bsgs\s*\*\*\s*out\s*\)", text)


def test_matvec_bsgs_fresh_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "matvec_bsgs_fresh_roundtrip.c"), tmp_path, hip=True)
