"""CPU-side checks of the linear transforms (plaintext-weighted sums of hoisted rotations): the three entries are
declared, exported and wrapped (what the kernels compile to: tests/test_ct_ops_build.py), the matrix-vector example is
plain C, and the identity the plan rests on -- a weight that does not depend on the key row can be folded into the key --
holds with the oracle and Python integers (no GPU needed)."""
import os
import re

import numpy as np

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_lintrans_create", "se_amd_ct_lintrans_device")      # declared `int name(`
DESTROY = "se_amd_lintrans_destroy"                                    # declared `void name(`
METHODS = ("lintrans_plan", "ct_lintrans")


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bvoid\s+%s\s*\(\s*se_amd_lintrans\s*\*" % DESTROY, text)
    assert re.search(r"typedef\s+struct\s+se_amd_lintrans\s+se_amd_lintrans\s*;", text)
    assert DESTROY in pkg.EXPORTED_SYMBOLS and hasattr(pkg.lib(), DESTROY)


def test_matvec_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "matvec_roundtrip.c"), tmp_path, hip=True)


def test_a_weight_folds_into_the_key(pkg):
    """1024 x 1, for R = 2 transformed digit rows F_r (the oracle's NTT of 15-bit digits), random key rows gk_r, a random
    permutation src and weights d that hold 0, 1, q - 1 and random words:
        sum_r F_r[src] . ((gk_r . d) mod q)  ==  d . sum_r F_r[src] . gk_r      (mod q),
    in Python integers.  Edge words of gk_r (0, 1, q - 1) meet every edge weight."""
    from oracle import pyoracle
    pyoracle.build(ref=False)
    n = 1024
    o = pyoracle.Oracle(n, 1)
    q = int(o.q[0])
    rng = np.random.default_rng(4242)
    edges = [0, 1, q - 1]
    c = rng.integers(0, q, n, dtype=np.uint32)
    F = [o.ntt(c & np.uint32(0x7FFF), 0), o.ntt(c >> np.uint32(15), 0)]
    gk = [rng.integers(0, q, n, dtype=np.uint32) for _ in F]
    d = rng.integers(0, q, n, dtype=np.uint32)
    for a, dv in enumerate(edges):                 # positions 3 a + b: weight edge a on key edge b (both rows)
        for b, kv in enumerate(edges):
            d[3 * a + b] = dv
            for row in gk:
                row[3 * a + b] = kv
    src = rng.permutation(n)
    assert sorted(src.tolist()) == list(range(n))
    Fi = [[int(v) for v in f[src]] for f in F]
    gi = [[int(v) for v in row] for row in gk]
    di = [int(v) for v in d]
    for k in range(n):
        folded = sum(Fi[r][k] * ((gi[r][k] * di[k]) % q) for r in range(len(F))) % q
        plain = (di[k] * (sum(Fi[r][k] * gi[r][k] for r in range(len(F))) % q)) % q
        assert folded == plain, k
    # an unreduced weight word folds like its residue (the fold kernel reduces it once)
    big = rng.integers(q, 1 << 32, n, dtype=np.uint64)
    for k in range(0, n, 37):
        w = int(big[k])
        assert (gi[0][k] * (w % q)) % q == (gi[0][k] * w) % q
