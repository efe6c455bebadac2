"""CPU-side checks of the rescale, the plaintext product and the level-aware decrypt: the entries are declared, exported
and wrapped, the rescale constants are exact, and the weighted-average example is plain C (no GPU needed).  What the
ct_ops kernels compile to: tests/test_ct_ops_build.py."""
import os

import numpy as np
import pytest

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)
from gpu_support import SE_ERR_INVALD_ARGUMENT

ENTRIES = ("se_amd_ct_rescale_device", "se_amd_ct_mul_plain_device", "se_amd_decrypt_level_device",
           "se_amd_decrypt_level_keyed_device", "se_amd_rescale_constants")
METHODS = ("ct_rescale", "ct_mul_plain", "decrypt_level", "decrypt_level_keyed")


def test_header_declares_the_entries(pkg):
    assert_entries(pkg, ENTRIES)


def test_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES)


def test_context_has_the_methods(pkg):
    assert_entries(pkg, (), methods=METHODS)


@pytest.mark.parametrize("shape", [(4096, 2), (4096, 3), (8192, 6), (16384, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rescale_constants_are_exact(pkg, shape):
    """inv[j] . q_last = 1 (mod q_j) and the Shoup companion is floor(inv . 2^32 / q_j), in Python ints; nothing is
    written beyond the primes - 1 entries."""
    n, primes = shape
    q = [int(x) for x in pkg.host_tables(n, primes)["q"]]
    inv = np.full(primes + 2, 0xABABABAB, np.uint32)
    sh = np.full(primes + 2, 0xCDCDCDCD, np.uint32)
    L = pkg.lib()
    assert L.se_amd_rescale_constants(n, primes, inv.ctypes.data, sh.ctypes.data) == 0
    for j in range(primes - 1):
        assert 0 < int(inv[j]) < q[j]
        assert int(inv[j]) * q[-1] % q[j] == 1, j
        assert int(sh[j]) == (int(inv[j]) << 32) // q[j], j
    assert (inv[primes - 1:] == 0xABABABAB).all() and (sh[primes - 1:] == 0xCDCDCDCD).all()
    # the Shoup companion is optional, and the wrapper returns the same numbers
    alone = np.zeros(primes - 1, np.uint32)
    assert L.se_amd_rescale_constants(n, primes, alone.ctypes.data, None) == 0
    assert (alone == inv[:primes - 1]).all()
    wi, ws = pkg.rescale_constants(n, primes)
    assert (wi == inv[:primes - 1]).all() and (ws == sh[:primes - 1]).all()


def test_rescale_constants_reject_bad_arguments(pkg):
    L = pkg.lib()
    buf = np.zeros(16, np.uint32)
    assert L.se_amd_rescale_constants(4096, 1, buf.ctypes.data, None) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_rescale_constants(4096, 0, buf.ctypes.data, None) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_rescale_constants(4096, 4, buf.ctypes.data, None) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_rescale_constants(1000, 2, buf.ctypes.data, None) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_rescale_constants(4096, 3, None, None) == SE_ERR_INVALD_ARGUMENT
    assert not buf.any()


def test_weighted_average_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "weighted_average_roundtrip.c"), tmp_path, hip=True)
