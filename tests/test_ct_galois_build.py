"""CPU-side checks of the slot rotations (Galois elements, Galois keys, the automorphism fused with its key switch): the
entries are declared, exported and wrapped, the two host-only entries agree with Python integers and with the oracle's
transforms, the new kernels compile for gfx950 without private memory, and the slot-sum example is plain C (no GPU
needed)."""
import os

import numpy as np
import pytest

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)
from vectors import sigma_coeff

ENTRIES = ("se_amd_galois_element", "se_amd_galois_table", "se_amd_gen_galois_keys", "se_amd_set_galois_keys",
           "se_amd_ct_galois_device")
METHODS = ("gen_galois_keys", "set_galois_keys", "ct_galois")
DEGREES = (1024, 2048, 4096, 8192, 16384)
GALOIS_KERNELS = tuple(
    f"{k}<{logn}{flag}>" for k, flag in (("k_ct_galois", ""), ("k_evk_diag", ", true")) for logn in range(10, 15))
RELIN_KERNELS = tuple(f"k_ct_relin<{logn}>" for logn in range(10, 15))
# Waves per SIMD of the two key-switch kernels before they shared their device code (tools/resource_usage.py ct_ops on
# that commit: 106 / 107 / 107 / 109 / 114 VGPRs for k_ct_relin, 124 / 125 / 125 / 106 / 105 for k_ct_galois): the
# floor the shared helpers must not cost a wave of.
KEY_SWITCH_WAVES = {f"{k}<{logn}>": 4 for k in ("k_ct_relin", "k_ct_galois") for logn in range(10, 15)}


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    assert callable(pkg.galois_element) and callable(pkg.galois_table)


@pytest.mark.parametrize("n", DEGREES)
def test_galois_element(pkg, n):
    """3^(step mod n/2) mod 2n for steps on both sides of zero and of the period; step 0 and step n/2 give 1."""
    for s in (0, 1, -1, n // 4, n // 2, 5):
        assert pkg.galois_element(n, s) == pow(3, s % (n // 2), 2 * n), s
    assert pkg.galois_element(n, 0) == 1 == pkg.galois_element(n, n // 2)
    assert (pkg.galois_element(n, 1) * pkg.galois_element(n, -1)) % (2 * n) == 1


def test_galois_element_refuses_a_bad_degree(pkg):
    for n in (0, 512, 3000, 4097, 32768):
        with pytest.raises(pkg.SealEmbeddedAmdError):
            pkg.galois_element(n, 1)


@pytest.mark.parametrize("shape", [(1024, 1), (4096, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_galois_table_is_the_automorphism_in_ntt_form(pkg, shape):
    """o.ntt(sigma_coeff(a)) == o.ntt(a)[src] for a random a, on the first and last prime, for 3, 3^-1, 3^5, n + 1 and
    2n - 1; src is a permutation."""
    from oracle import pyoracle
    pyoracle.build(ref=False)
    n, npr = shape
    o = pyoracle.Oracle(n, npr)
    rng = np.random.default_rng(n)
    for g in (3, pow(3, -1, 2 * n), pow(3, 5, 2 * n), n + 1, 2 * n - 1):
        src = pkg.galois_table(n, g)
        assert src.dtype == np.uint16 and sorted(src.tolist()) == list(range(n)), g
        for j in sorted({0, npr - 1}):
            q = int(o.q[j])
            a = rng.integers(0, q, n, dtype=np.uint32)
            a[:3] = [0, 1, q - 1]
            assert (o.ntt(sigma_coeff(a, g, q), j) == o.ntt(a, j)[src.astype(np.int64)]).all(), (g, j)


def test_galois_table_identity_and_refusals(pkg):
    n = 2048
    assert (pkg.galois_table(n, 1) == np.arange(n)).all()
    for g in (0, 2, n, 2 * n, 2 * n + 1, 0xFFFFFFFF):
        with pytest.raises(pkg.SealEmbeddedAmdError):
            pkg.galois_table(n, g)
    with pytest.raises(pkg.SealEmbeddedAmdError):
        pkg.galois_table(3000, 3)


def test_ct_ops_kernels_use_no_scratch():
    """The fused automorphism + key switch and the Galois diagonal exist for every degree and stay in registers, and
    so does every other kernel of the file -- the relinearisation kernel they share the key switch with among them; that
    sharing costs neither of the two kernels a wave per SIMD at any degree."""
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    for k in GALOIS_KERNELS + RELIN_KERNELS:
        assert k in rows, (k, sorted(rows))
        vgpr, scratch, occ = rows[k]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD")
    for k, (_, scratch, _) in rows.items():
        assert scratch == 0, (k, scratch)
    assert len(KEY_SWITCH_WAVES) == 10
    for k, waves in KEY_SWITCH_WAVES.items():
        assert rows[k][2] >= waves, (k, rows[k], waves)


def test_slot_sum_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "slot_sum_roundtrip.c"), tmp_path, hip=True)
