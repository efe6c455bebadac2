"""CPU-side checks of the switch-key ring: the entries are declared, exported and wrapped; the two new kernels compile for
gfx950 without private memory at the family's 4 waves per SIMD; no kernel of the file went missing or gained scratch and
the special-prime key switch kept its waves; the example is plain C (no GPU needed)."""
import os

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)
from test_ct_bsgs_build import KERNELS_BEFORE

ENTRIES = ("se_amd_gen_switch_keys_sp", "se_amd_set_switch_keyring_sp", "se_amd_ct_switch_keyed_sp_device",
           "se_amd_ct_switch_sum_keyed_sp_device")
METHODS = ("gen_switch_keys_sp", "set_switch_keyring_sp", "ct_switch_keyed_sp", "ct_switch_sum_keyed_sp")

# every kernel ct_ops.hip had on the parent commit
BEFORE = (list(KERNELS_BEFORE) + ["k_ct_mul_plain_sum"]
          + [f"{k}<{logn}>" for k in ("k_ct_galois_accum", "k_bsgs_permute") for logn in range(10, 15)]
          + [f"{k}<{logn}>" for k in ("k_ct_galois_many_ext_sp", "k_ct_galois_accum_sp", "k_ct_mod_down_sp")
             for logn in (12, 13, 14)])


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    assert "needs BOTH secrets" in text               # who can run the generator is said plainly


def test_new_kernels_use_no_scratch_at_four_waves():
    """k_ct_switch_sp<logn> and k_ct_switch_sum_sp<logn> are k_ct_relin_sp<logn> with the record loop inside each pass and
    the key pointer taken per record.  As built, logn 12 / 13 / 14: 101 / 117 / 120 and 117 / 121 / 120 VGPRs beside the
    relinearisation's 113 / 115 / 119; no scratch, 4 waves per SIMD each."""
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    for logn in (12, 13, 14):
        for k in (f"k_ct_switch_sp<{logn}>", f"k_ct_switch_sum_sp<{logn}>"):
            assert k in rows, (k, sorted(rows))
            vgpr, scratch, occ = rows[k]
            print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD; k_ct_relin_sp<{logn}>: "
                  f"{rows[f'k_ct_relin_sp<{logn}>']}")
            assert scratch == 0 and occ >= 4, (k, rows[k])
    for logn in range(10, 15):
        k = f"k_evk_diag_switch_sp<{logn}>"
        assert k in rows and rows[k][1] == 0, (k, rows.get(k))


def test_no_kernel_went_missing_or_gained_scratch_and_the_key_switch_keeps_its_waves():
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    missing = [k for k in BEFORE if k not in rows]
    assert not missing, missing
    spilled = {k: rows[k] for k in BEFORE if rows[k][1] != 0}
    assert not spilled, spilled
    for logn in (12, 13, 14):
        for k in (f"k_ct_relin_sp<{logn}>", f"k_ct_galois_sp<{logn}>"):
            print(f"{k}: {rows[k]}")
            assert rows[k][2] == 4, (k, rows[k])


def test_fleet_sum_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "fleet_sum_roundtrip.c"), tmp_path, hip=True)
