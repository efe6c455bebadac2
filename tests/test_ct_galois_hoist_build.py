"""CPU-side checks of the hoisted rotations (many rotations of a record from one digit decomposition): the two entries
are declared, exported and wrapped (what the kernel compiles to: tests/test_ct_ops_build.py), the moving-sum example is
plain C, and the algebra the definition rests on -- sigma applied to a TRANSFORMED digit is the permutation src_g of the
transform of sigma applied to the integer digit -- holds with the oracle and Python integers (no GPU needed)."""
import os

import numpy as np
import pytest

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)
from vectors import galois_image, sigma_coeff

ENTRIES = ("se_amd_ct_galois_many_device", "se_amd_ct_galois_sum_device")
METHODS = ("ct_galois_many", "ct_galois_sum")


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)


def test_moving_sum_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "moving_sum_roundtrip.c"), tmp_path, hip=True)


def test_permuted_transform_is_the_transform_of_the_rotated_digit(pkg):
    """1024 x 1: for g in 3, 3^-1, n + 1, 2n - 1 and both 15-bit digit rows D of a coefficient row,
    o.ntt(D)[src_g] == o.ntt(sigma_int(D) mod q), sigma_int on the integers with its signs.  The coefficient row holds
    0, 1, 2^15 - 1 (low digit 2^15 - 1, high digit 0), 2^15, and the full-range q - 1, each on negated and on kept
    positions of every element that keeps more than the constant coefficient (2n - 1 negates all the others; the
    constant one holds 0), so the low digit row holds 0, 1, 2^15 - 1 and the low digit of q - 1 on both kinds."""
    from oracle import pyoracle
    pyoracle.build(ref=False)
    n = 1024
    o = pyoracle.Oracle(n, 1)
    q = int(o.q[0])
    rng = np.random.default_rng(1024)
    elts = (3, pow(3, -1, 2 * n), n + 1, 2 * n - 1)
    edges = np.array([0, 1, (1 << 15) - 1, 1 << 15, q - 1], dtype=np.uint32)
    c = rng.integers(1, q, n, dtype=np.uint32)
    for start in (0, 100, n // 2, n // 2 + 101, n - 11):     # twice, 5 apart wraps to 6: even and odd indices
        c[start:start + 5] = edges
        c[start + 6:start + 11] = edges
    digits = (c & np.uint32(0x7FFF), c >> np.uint32(15))
    assert (digits[0].astype(np.uint64) + (digits[1].astype(np.uint64) << np.uint64(15)) == c).all()
    for g in elts:
        _, neg = galois_image(n, g)
        for v in edges:
            at = c == v
            assert (at & neg).any(), (g, int(v))
            assert (at & ~neg).any() or g == 2 * n - 1, (g, int(v))
        assert c[0] == 0 and not neg[0]
        src = pkg.galois_table(n, g).astype(np.int64)
        for t, D in enumerate(digits):
            rotated = sigma_coeff(D.astype(np.int64), g)                   # integers in (-2^15, 2^15)
            assert np.abs(rotated).max() < (1 << 15)
            assert (o.ntt(D, 0)[src] == o.ntt((rotated % q).astype(np.uint32), 0)).all(), (g, t)
