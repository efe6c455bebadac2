"""CPU-side checks of the switch-key ring: the entries are declared, exported and wrapped (what the kernels compile to:
tests/test_ct_ops_build.py); the example is plain C (no GPU needed)."""
import os

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_gen_switch_keys_sp", "se_amd_set_switch_keyring_sp", "se_amd_ct_switch_keyed_sp_device",
           "se_amd_ct_switch_sum_keyed_sp_device")
METHODS = ("gen_switch_keys_sp", "set_switch_keyring_sp", "ct_switch_keyed_sp", "ct_switch_sum_keyed_sp")


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    assert "needs BOTH secrets" in text               # who can run the generator is said plainly


def test_fleet_sum_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "fleet_sum_roundtrip.c"), tmp_path, hip=True)
