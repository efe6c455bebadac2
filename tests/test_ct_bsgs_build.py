"""CPU-side checks of the baby-step / giant-step linear transforms: the entries are declared, exported and wrapped, the
two new kernels compile for gfx950 without private memory -- the accumulate kernel with the waves per SIMD of the single
rotation it repeats -- and no kernel of the file went missing, the example is plain C, and the identity the plan rests
on, sigma_gamma(d' . z) = d . sigma_gamma(z) for d' = d permuted by gamma^-1, holds in Python integers (no GPU needed)."""
import os
import re

import numpy as np

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)
from ct_model import inverse_element

ENTRIES = ("se_amd_ct_mul_plain_sum_device", "se_amd_ct_galois_accum_device", "se_amd_bsgs_create",
           "se_amd_ct_bsgs_device")                                   # declared `int name(`
DESTROY = "se_amd_bsgs_destroy"                                       # declared `void name(`
WORKSPACE = "se_amd_bsgs_workspace_bytes"                             # declared `size_t name(`
METHODS = ("ct_mul_plain_sum", "ct_galois_accum", "bsgs_plan", "ct_bsgs", "bsgs_workspace_bytes")

# the kernels of kernels/ct_ops.hip before this block was added
KERNELS_BEFORE = (
    ["k_ct_lincomb<false>", "k_ct_lincomb<true>", "k_ct_lincomb_sum", "k_ct_mul_plain", "k_ct_mul", "k_relin_key_rows",
     "k_lintrans_fold"]
    + [f"{k}<{logn}>" for k in ("k_ct_rescale", "k_ct_relin", "k_ct_galois", "k_ct_lintrans") for logn in range(10, 15)]
    + [f"{k}<{logn}>" for k in ("k_ct_galois_sp", "k_ct_relin_sp", "k_ct_lintrans_sp", "k_ct_galois_sum_sp")
       for logn in range(12, 15)]
    + [f"k_ct_galois_hoist<{logn}, {s}>" for logn in range(10, 15) for s in ("true", "false")]
    + [f"{k}<{logn}, {s}>" for k in ("k_evk_diag", "k_evk_diag_sp") for logn in range(10, 15) for s in ("true", "false")])


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


def test_bsgs_kernels_use_no_scratch_and_keep_the_rotations_waves():
    """k_ct_galois_accum<logn> is k_ct_galois<logn> with the element loop inside: ONE accumulator pair across the
    elements, sigma(c0) added to it, so it holds at least the waves per SIMD the same report gives the single rotation,
    without scratch.  As built: 118 / 119 / 120 / 122 / 108 VGPRs for logn 10 .. 14 beside the rotation's 124 / 125 / 125 /
    102 / 105, 4 waves per SIMD each.  k_ct_mul_plain_sum: 64 VGPRs (a tile of four records, 64-bit sums), 8 waves."""
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    for logn in range(10, 15):
        k, sibling = f"k_ct_galois_accum<{logn}>", f"k_ct_galois<{logn}>"
        assert k in rows and sibling in rows, (k, sorted(rows))
        vgpr, scratch, occ = rows[k]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD; {sibling}: {rows[sibling]}")
        assert scratch == 0, (k, scratch)
        assert occ >= rows[sibling][2], (k, rows[k], rows[sibling])
    assert "k_ct_mul_plain_sum" in rows, sorted(rows)
    vgpr, scratch, occ = rows["k_ct_mul_plain_sum"]
    print(f"k_ct_mul_plain_sum: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD")
    assert scratch == 0
    missing = [k for k in KERNELS_BEFORE if k not in rows]
    assert not missing, missing


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
