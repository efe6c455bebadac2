"""CPU-side checks of the full-modulus decrypt: the entries are declared and exported, the k_decrypt_full kernels exist
for every degree within their scratch budgets, and the host's recombination constants are exact (no GPU needed)."""
import os
import re
import subprocess
import sys

import pytest

import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ENTRIES = ("se_amd_decrypt_full_device", "se_amd_decrypt_full_keyed_device")
SHAPES = V.ALL_SHAPES + [(16384, 13), (4096, 2), (4096, 1), (8192, 3)]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.load_package()
    p.build_library()
    return p


def test_header_declares_full_entries():
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for nm in FULL_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % nm, text), nm


def test_library_exports_full_entries(pkg):
    L = pkg.lib()
    for nm in FULL_ENTRIES:
        assert nm in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, nm), nm
    ctx_cls = pkg.Context
    assert hasattr(ctx_cls, "decrypt_full") and hasattr(ctx_cls, "decrypt_full_keyed")


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
    assert L.se_amd_crt_constants(4096, 4, buf.ctypes.data, None) == -22
    assert L.se_amd_crt_constants(1000, 1, buf.ctypes.data, None) == -22
    assert L.se_amd_crt_constants(4096, 3, None, None) == -22


def test_roundtrip_example_compiles_as_plain_c(tmp_path):
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-c",
                    os.path.join(ROOT, "examples", "batch_roundtrip.c"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", str(tmp_path / "batch_roundtrip.o")],
                   check=True)
