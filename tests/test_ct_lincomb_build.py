"""CPU-side checks of the key-free weighted sum of ciphertexts: the two entries are declared, exported and wrapped, and
the aggregation example is plain C (no GPU needed).  What the kernels compile to: tests/test_ct_ops_build.py."""
import os

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)

LINCOMB_ENTRIES = ("se_amd_ct_lincomb_device", "se_amd_set_lincomb_split")


def test_header_declares_lincomb_entries(pkg):
    assert_entries(pkg, LINCOMB_ENTRIES)


def test_library_exports_lincomb_entries(pkg):
    assert_entries(pkg, LINCOMB_ENTRIES)


def test_context_has_the_methods(pkg):
    assert_entries(pkg, (), methods=("ct_lincomb", "set_lincomb_split"))


def test_aggregate_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "aggregate_roundtrip.c"), tmp_path, hip=True)
