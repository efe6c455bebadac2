"""CPU-side checks of the key-free weighted sum of ciphertexts: the two entries are declared, exported and wrapped, the
ct_ops kernels compile for gfx950 without private memory, and the aggregation example is plain C (no GPU needed)."""
import os

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)

LINCOMB_ENTRIES = ("se_amd_ct_lincomb_device", "se_amd_set_lincomb_split")
LINCOMB_KERNELS = ("k_ct_lincomb<false>", "k_ct_lincomb<true>", "k_ct_lincomb_sum")


def test_header_declares_lincomb_entries(pkg):
    assert_entries(pkg, LINCOMB_ENTRIES)


def test_library_exports_lincomb_entries(pkg):
    assert_entries(pkg, LINCOMB_ENTRIES)


def test_context_has_the_methods(pkg):
    assert_entries(pkg, (), methods=("ct_lincomb", "set_lincomb_split"))


def test_lincomb_kernels_use_no_scratch():
    """A wave-uniform entry loop and 16-byte accesses: nothing of these kernels lives in private memory."""
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    for k in LINCOMB_KERNELS:
        assert k in rows, (k, sorted(rows))
        vgpr, scratch, occ = rows[k]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD")
        assert scratch == 0, (k, rows[k])


def test_aggregate_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "aggregate_roundtrip.c"), tmp_path, hip=True)
