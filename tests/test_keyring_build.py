"""CPU-side checks of the key-ring feature: the five entries are declared and exported, and the keyed twins of the
encryption / decrypt kernels keep the register budgets of the unkeyed kernels (no GPU needed)."""
import pytest

from build_support import assert_entries, pkg, resource_rows  # noqa: F401  (pkg is a fixture)

KEYRING_ENTRIES = ("se_amd_set_secret_keyring", "se_amd_set_public_keyring", "se_amd_encrypt_sym_keyed_device",
                   "se_amd_encrypt_asym_keyed_device", "se_amd_decrypt_decode_keyed_device")


def test_header_declares_keyring_entries(pkg):
    assert_entries(pkg, KEYRING_ENTRIES)


def test_library_exports_keyring_entries(pkg):
    assert_entries(pkg, KEYRING_ENTRIES)


@pytest.fixture(scope="module")
def rows():
    r = resource_rows("encode_encrypt")
    assert r, "tools/resource_usage.py gave no table for encode_encrypt"
    return r


def test_keyed_kernels_keep_the_unkeyed_budgets(rows):
    """Every keyed twin (key base in SGPRs) uses the registers, scratch and occupancy of its unkeyed kernel."""
    twins = []
    for logn in range(10, 15):
        for mode in (0, 1):
            twins += [(f"k_encode_encrypt<{logn}, {mode}>", f"k_encode_encrypt_keyed<{logn}, {mode}>"),
                      (f"k_encode_encrypt_general<{logn}, {mode}>", f"k_encode_encrypt_general_keyed<{logn}, {mode}>")]
        twins += [(f"k_ntt_fuse<{logn}, 0>", f"k_ntt_fuse_keyed<{logn}, 0>"),
                  (f"k_decrypt_decode<{logn}>", f"k_decrypt_decode_keyed<{logn}>")]
    for plain, keyed in twins:
        assert keyed in rows, keyed
        pv, ps, po = rows[plain]
        kv, ks, ko = rows[keyed]
        assert ko >= po, (keyed, rows[keyed], rows[plain])
        assert ks <= ps, (keyed, rows[keyed], rows[plain])
        if "general" not in plain:   # the general (list-walking) forms: only occupancy and spills matter
            assert kv <= pv, (keyed, rows[keyed], rows[plain])


def test_keyed_kernels_within_the_issue_budgets(rows):
    vg, sc, occ = rows["k_encode_encrypt_keyed<12, 0>"]
    assert vg <= 128 and occ >= 4 and sc <= 96         # scratch only in the pair form's exact redo
    assert rows["k_encode_encrypt_keyed<12, 1>"][0] <= 168
    assert rows["k_encode_encrypt_keyed<13, 1>"][0] <= 128
    for k in ("k_ntt_fuse_keyed<12, 0>", "k_ntt_fuse_keyed<14, 0>", "k_encode_encrypt_keyed<14, 0>"):
        assert rows[k][1] == 0, (k, rows[k])
    for k in ("k_ring_secret_ntt<12>", "k_ring_secret_ntt<14>", "k_key_sanitize", "k_key_reject", "k_ring_pairs"):
        assert k in rows and rows[k][1] == 0, k
