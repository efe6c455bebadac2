"""CPU-side checks of the key-ring feature: the five entries are declared and exported, and the keyed twins of the
encryption / decrypt kernels keep the register budgets of the unkeyed kernels (no GPU needed)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEYRING_ENTRIES = ("se_amd_set_secret_keyring", "se_amd_set_public_keyring", "se_amd_encrypt_sym_keyed_device",
                   "se_amd_encrypt_asym_keyed_device", "se_amd_decrypt_decode_keyed_device")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.load_package()
    p.build_library()
    return p


def test_header_declares_keyring_entries():
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for nm in KEYRING_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % nm, text), nm


def test_library_exports_keyring_entries(pkg):
    L = pkg.lib()
    for nm in KEYRING_ENTRIES:
        assert nm in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, nm), nm


@pytest.fixture(scope="module")
def rows():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "encode_encrypt"],
                         capture_output=True, text=True, timeout=1200).stdout
    r = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if len(f) >= 6:
            r[" ".join(f[:-5]).replace("seamd::", "")] = (int(f[-5]), int(f[-3]), int(f[-2]))   # VGPR, scratch, occ
    assert r, out
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
