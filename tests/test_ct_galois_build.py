"""CPU-side checks of the slot rotations (Galois elements, Galois keys, the automorphism fused with its key switch): the
entries are declared, exported and wrapped, the two host-only entries agree with Python integers and with the oracle's
transforms, and the slot-sum example is plain C (no GPU needed).  What the kernels compile to:
tests/test_ct_ops_build.py."""
import os

import numpy as np
import pytest

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)
from vectors import sigma_coeff

ENTRIES = ("se_amd_galois_element", "se_amd_galois_table", "se_amd_gen_galois_keys", "se_amd_set_galois_keys",
           "se_amd_ct_galois_device")
METHODS = ("gen_galois_keys", "set_galois_keys", "ct_galois")
DEGREES = (1024, 2048, 4096, 8192, 16384)


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


def test_slot_sum_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "slot_sum_roundtrip.c"), tmp_path, hip=True)
