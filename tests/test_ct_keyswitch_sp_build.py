"""CPU-side checks of the special-prime key switch (se_amd_ct_relin_sp_device, se_amd_ct_galois_sp_device, their keys,
se_amd_ct_drop_primes_device): the entries are declared, exported and wrapped, the two kernels compile for gfx950 without
private memory at the family's occupancy and cost the digit kernels nothing, the example is plain C, and the CPU
simulation of a rotation at the fresh scale stays far inside the reference's 0.1 (no GPU needed)."""
import os

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_gen_relin_key_sp", "se_amd_set_relin_key_sp", "se_amd_gen_galois_keys_sp",
           "se_amd_set_galois_keys_sp", "se_amd_ct_relin_sp_device", "se_amd_ct_galois_sp_device",
           "se_amd_ct_drop_primes_device")
METHODS = ("gen_relin_key_sp", "set_relin_key_sp", "gen_galois_keys_sp", "set_galois_keys_sp", "ct_relin_sp",
           "ct_galois_sp", "ct_drop_primes")
# Waves per SIMD the committed build reaches (tools/resource_usage.py ct_ops: 113 / 115 / 119 VGPRs for k_ct_relin_sp,
# 113 / 97 / 97 for k_ct_galois_sp at n = 4096 / 8192 / 16384): the family's 4 everywhere.
SP_WAVES = {f"{k}<{logn}>": 4 for k in ("k_ct_relin_sp", "k_ct_galois_sp") for logn in (12, 13, 14)}
SP_DIAG_KERNELS = tuple(f"k_evk_diag_sp<{logn}, {flag}>" for logn in range(10, 15) for flag in ("true", "false"))
# the digit key-switch kernels' floor (tests/test_ct_galois_build.py): the new code shares their helpers
DIGIT_WAVES = {f"{k}<{logn}>": 4 for k in ("k_ct_relin", "k_ct_galois") for logn in range(10, 15)}
# every kernel ct_ops.hip had before this one: all at 0 bytes of scratch
BEFORE = (("k_ct_lincomb_sum", "k_ct_mul_plain", "k_ct_mul", "k_relin_key_rows", "k_lintrans_fold",
           "k_ct_lincomb<false>", "k_ct_lincomb<true>") +
          tuple(f"{k}<{logn}>" for k in ("k_ct_rescale", "k_ct_relin", "k_ct_galois", "k_ct_lintrans")
                for logn in range(10, 15)) +
          tuple(f"k_ct_galois_hoist<{logn}, {flag}>" for logn in range(10, 15) for flag in ("true", "false")) +
          tuple(f"k_evk_diag<{logn}, {flag}>" for logn in range(10, 15) for flag in ("true", "false")))


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)


def test_special_prime_kernels_use_no_scratch_and_keep_the_occupancy():
    """Both kernels exist for LOGN 12 .. 14 (a context with a special prime has np >= 2, which the default chains give
    from n = 4096 on) with 0 bytes of scratch and 4 waves per SIMD; the diagonal kernel of the key generator exists for
    every degree; every kernel the file had before is still at 0 scratch and the ten digit key-switch instantiations
    are still at their floor of 4 waves per SIMD."""
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    assert len(SP_WAVES) == 6 and len(DIGIT_WAVES) == 10
    for k, waves in SP_WAVES.items():
        assert k in rows, (k, sorted(rows))
        vgpr, scratch, occ = rows[k]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD")
        assert scratch == 0 and occ == waves, (k, rows[k])
    for k in SP_DIAG_KERNELS:
        assert k in rows and rows[k][1] == 0, k
    assert not [k for k in rows if k.startswith(("k_ct_relin_sp<1", "k_ct_galois_sp<1")) and k not in SP_WAVES]
    for k in BEFORE:
        assert k in rows, (k, sorted(rows))
        assert rows[k][1] == 0, (k, rows[k])
    for k, (_, scratch, _) in rows.items():
        assert scratch == 0, (k, scratch)
    for k, waves in DIGIT_WAVES.items():
        assert rows[k][2] >= waves, (k, rows[k], waves)


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
