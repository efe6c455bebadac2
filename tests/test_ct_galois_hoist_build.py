"""CPU-side checks of the hoisted rotations (many rotations of a record from one digit decomposition): the two entries
are declared, exported and wrapped, every instantiation of the kernel compiles for gfx950 without private memory and
keeps the waves per SIMD it was built with, the moving-sum example is plain C, and the algebra the definition rests on
-- sigma applied to a TRANSFORMED digit is the permutation src_g of the transform of sigma applied to the integer digit
-- holds with the oracle and Python integers (no GPU needed)."""
import os

import numpy as np
import pytest

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)
from vectors import galois_image, sigma_coeff

ENTRIES = ("se_amd_ct_galois_many_device", "se_amd_ct_galois_sum_device")
METHODS = ("ct_galois_many", "ct_galois_sum")
# Waves per SIMD of k_ct_galois_hoist<logn, SUM> as built (tools/resource_usage.py ct_ops): the sum form carries one
# accumulator pair like its siblings k_ct_relin / k_ct_galois and keeps their 4 (107 / 122 / 121 / 127 / 111 VGPRs for
# logn 10 .. 14); the many form carries kHoistGroup = 2 pairs, 139 / 154 / 153 / 159 VGPRs and 3 waves for logn 10 .. 13,
# and at logn 14, where the workgroup of 1024 threads is 4 waves per SIMD by itself, 128 VGPRs with the coefficients of
# the input row parked in LDS.  A floor: fewer waves than these is a regression, scratch at any degree is one too.
HOIST_WAVES = {f"k_ct_galois_hoist<{logn}, true>": 4 for logn in range(10, 15)}
HOIST_WAVES.update({f"k_ct_galois_hoist<{logn}, false>": 3 for logn in range(10, 14)})
HOIST_WAVES["k_ct_galois_hoist<14, false>"] = 4


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)


def test_hoist_kernels_use_no_scratch_and_keep_their_waves():
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    assert len(HOIST_WAVES) == 10
    for k, waves in HOIST_WAVES.items():
        assert k in rows, (k, sorted(rows))
        vgpr, scratch, occ = rows[k]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD")
        assert scratch == 0, (k, scratch)
        assert occ >= waves, (k, rows[k], waves)


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
