"""CPU-side checks of the full-modulus decrypt: the entries are declared and exported, the k_decrypt_full kernels exist
for every degree within their scratch budgets, and the host's recombination constants are exact (no GPU needed)."""
import os

import pytest

import vectors as V
from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)
from gpu_support import SE_ERR_INVALD_ARGUMENT

FULL_ENTRIES = ("se_amd_decrypt_full_device", "se_amd_decrypt_full_keyed_device")
SHAPES = V.ALL_SHAPES + [(16384, 13), (4096, 2), (4096, 1), (8192, 3)]


def test_header_declares_full_entries(pkg):
    assert_entries(pkg, FULL_ENTRIES)


def test_library_exports_full_entries(pkg):
    assert_entries(pkg, FULL_ENTRIES, methods=("decrypt_full", "decrypt_full_keyed"))


@pytest.fixture(scope="module")
def rows():
    r = resource_rows("encode_encrypt")
    assert r, "tools/resource_usage.py gave no table for encode_encrypt"
    return r


def test_full_kernels_exist_within_their_scratch_budget(rows):
    """No private-memory traffic in the prime loop: zero scratch for n <= 8192; at n = 16384 (1024 threads, 128 VGPRs
    per thread) at most the 96 bytes this project accepts for a cold spilling branch."""
    for logn in range(10, 15):
        plain, keyed = f"k_decrypt_full<{logn}>", f"k_decrypt_full_keyed<{logn}>"
        assert plain in rows and keyed in rows, (plain, sorted(rows))
        pv, ps, po = rows[plain]
        kv, ks, ko = rows[keyed]
        print(f"{plain}: {pv} VGPRs, {ps} B scratch, {po} waves/SIMD; keyed {kv} / {ks} / {ko}")
        if logn <= 13:
            assert ps == 0, (plain, rows[plain])
        else:
            assert ps <= 96, (plain, rows[plain])
            assert pv <= 128, (plain, rows[plain])
        assert kv <= pv and ks <= ps and ko >= po, (keyed, rows[keyed], rows[plain])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_crt_constants_are_exact(pkg, shape):
    """inv[j] . (q_0 ... q_{j-1}) = 1 (mod q_j) and the Shoup companion is floor(inv . 2^32 / q_j), in Python ints."""
    n, npr = shape
    q = [int(x) for x in pkg.host_tables(n, npr)["q"]]
    inv, sh = pkg.crt_constants(n, npr)
    assert len(inv) == npr and int(inv[0]) == 0 and int(sh[0]) == 0
    Q = 1
    for j in range(npr):
        if j:
            assert 0 < int(inv[j]) < q[j]
            assert Q * int(inv[j]) % q[j] == 1, j
            assert int(sh[j]) == (int(inv[j]) << 32) // q[j], j
        Q *= q[j]
    # the kernel's width assumptions: two primes stay below 2^60, three below 2^90 (the 128-bit step of the third prime)
    if npr >= 2:
        assert q[0] * q[1] < 2 ** 60
    if npr >= 3:
        assert q[0] * q[1] * q[2] < 2 ** 90
    if npr >= 4:
        assert q[0] * q[1] * q[2] > 2 ** 65      # from the fourth prime on an int64 is its own centred representative


def test_crt_constants_reject_unsupported_shapes(pkg):
    import numpy as np
    L = pkg.lib()
    buf = np.zeros(16, np.uint32)
    assert L.se_amd_crt_constants(4096, 4, buf.ctypes.data, None) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_crt_constants(1000, 1, buf.ctypes.data, None) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_crt_constants(4096, 3, None, None) == SE_ERR_INVALD_ARGUMENT


def test_roundtrip_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "batch_roundtrip.c"), tmp_path, hip=True)
