"""CPU-side checks of the special-prime key switch (se_amd_ct_relin_sp_device, se_amd_ct_galois_sp_device, their keys,
se_amd_ct_drop_primes_device): the entries are declared, exported and wrapped (what the kernels compile to:
tests/test_ct_ops_build.py), the example is plain C, and the CPU simulation of a rotation at the fresh scale stays far
inside the reference's 0.1 (no GPU needed)."""
import os

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_gen_relin_key_sp", "se_amd_set_relin_key_sp", "se_amd_gen_galois_keys_sp",
           "se_amd_set_galois_keys_sp", "se_amd_ct_relin_sp_device", "se_amd_ct_galois_sp_device",
           "se_amd_ct_drop_primes_device")
METHODS = ("gen_relin_key_sp", "set_relin_key_sp", "gen_galois_keys_sp", "set_galois_keys_sp", "ct_relin_sp",
           "ct_galois_sp", "ct_drop_primes")


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)


def test_rotate_fresh_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "rotate_fresh_roundtrip.c"), tmp_path, hip=True)


def test_noise_tool_centred_digits_keep_a_fresh_rotation_inside_the_acceptance():
    """tools/ct_keyswitch_sp_noise_sim.py at 4096 x 3, L = 2: a fresh record rotated at scale 2^25 without lift or
    rescale decodes within 0.1 of the rolled values (the simulation gives 6.3e-4, key-switch coefficients up to 337),
    and the centred digits of the definition beat canonical digits in [0, q_j) (2.0e-2, 674)."""
    from oracle import pyoracle
    pyoracle.build(ref=False)
    from tools import ct_keyswitch_sp_noise_sim as sim
    cen, can = sim.rotation(4096, 3, 2, centre=True), sim.rotation(4096, 3, 2, centre=False)
    print(cen, can)
    assert cen["slot_error"] < 0.1
    assert cen["slot_error"] < can["slot_error"]
    assert cen["key_switch_max"] < can["key_switch_max"]
