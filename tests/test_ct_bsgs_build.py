"""CPU-side checks of the baby-step / giant-step linear transforms: the entries are declared, exported and wrapped (what
the kernels compile to: tests/test_ct_ops_build.py), the example is plain C, and the identity the plan rests on,
sigma_gamma(d' . z) = d . sigma_gamma(z) for d' = d permuted by gamma^-1, holds in Python integers (no GPU needed)."""
import os
import re

import numpy as np

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)
from ct_model import inverse_element

ENTRIES = ("se_amd_ct_mul_plain_sum_device", "se_amd_ct_galois_accum_device", "se_amd_bsgs_create",
           "se_amd_ct_bsgs_device")                                   # declared `int name(`
DESTROY = "se_amd_bsgs_destroy"                                       # declared `void name(`
WORKSPACE = "se_amd_bsgs_workspace_bytes"                             # declared `size_t name(`
METHODS = ("ct_mul_plain_sum", "ct_galois_accum", "bsgs_plan", "ct_bsgs", "bsgs_workspace_bytes")


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bvoid\s+%s\s*\(\s*se_amd_bsgs\s*\*" % DESTROY, text)
    assert re.search(r"\bsize_t\s+%s\s*\(\s*const\s+se_amd_bsgs\s*\*" % WORKSPACE, text)
    assert re.search(r"typedef\s+struct\s+se_amd_bsgs\s+se_amd_bsgs\s*;", text)
    for nm in (DESTROY, WORKSPACE):
        assert nm in pkg.EXPORTED_SYMBOLS and hasattr(pkg.lib(), nm), nm
    assert callable(getattr(pkg.BsgsPlan, "close", None))


def test_matvec_bsgs_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "matvec_bsgs_roundtrip.c"), tmp_path, hip=True)


def test_a_diagonal_pre_rotated_by_the_inverse_commutes_with_the_giant_step(pkg):
    """1024 x 1, in Python integers.  For gamma in {3, n + 1, 2n - 1, 3^-1}: src_gamma o src_{gamma^-1} is the identity
    (both ways), and with d'[k] = d[src_{gamma^-1}(k)], sigma_gamma(x)[k] = x[src_gamma(k)] on NTT-form rows,
        sigma_gamma(d' . z) == d . sigma_gamma(z)      (mod q)
    for random rows d and z that hold 0, 1 and q - 1, every edge word of d meeting every edge word of z."""
    from oracle import pyoracle
    pyoracle.build(ref=False)
    n = 1024
    q = int(pyoracle.Oracle(n, 1).q[0])
    rng = np.random.default_rng(2323)
    edges = [0, 1, q - 1]
    for gamma in (3, n + 1, 2 * n - 1, inverse_element(n, 3)):
        inv = inverse_element(n, gamma)
        src, src_inv = (pkg.galois_table(n, g).astype(np.int64) for g in (gamma, inv))
        assert sorted(src.tolist()) == list(range(n))
        assert (src[src_inv] == np.arange(n)).all() and (src_inv[src] == np.arange(n)).all(), gamma
        d = [int(v) for v in rng.integers(0, q, n)]
        z = [int(v) for v in rng.integers(0, q, n)]
        for a, dv in enumerate(edges):               # position k = 3 a + b: d[k] = edge a meets sigma(z)[k] = edge b
            for b, zv in enumerate(edges):
                d[3 * a + b] = dv
                z[int(src[3 * a + b])] = zv
        dp = [d[int(src_inv[k])] for k in range(n)]
        prod = [(dp[k] * z[k]) % q for k in range(n)]
        lhs = [prod[int(src[k])] for k in range(n)]
        rhs = [(d[k] * z[int(src[k])]) % q for k in range(n)]
        assert lhs == rhs, gamma
        assert {(d[k], z[int(src[k])]) for k in range(9)} == {(a, b) for a in edges for b in edges}
