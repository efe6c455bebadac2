"""CPU-side checks of the hoisted rotations on the special-prime key (se_amd_ct_galois_sum_sp_device,
se_amd_lintrans_create_sp, se_amd_ct_lintrans_sp_device): the entries are declared, exported and wrapped (what the kernels
compile to: tests/test_ct_ops_build.py), the example is plain C, the definition has the two properties the header states,
and the CPU simulation of a moving sum and of a matrix-vector product on fresh records stays inside the reference's 0.1
(no GPU needed)."""
import os

import numpy as np

from build_support import ROOT, assert_entries, compile_only, pkg  # noqa: F401  (pkg is a fixture)
from ct_model import edge_row, galois_sp_expect, hoist_sp_expect, sum_of_single_calls

ENTRIES = ("se_amd_ct_galois_sum_sp_device", "se_amd_lintrans_create_sp", "se_amd_ct_lintrans_sp_device")
METHODS = ("ct_galois_sum_sp", "lintrans_plan_sp", "ct_lintrans_sp")


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)


def test_matvec_fresh_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "matvec_fresh_roundtrip.c"), tmp_path, hip=True)


def test_model_one_element_is_the_single_entry_and_two_are_not_two_calls():
    """The definition (hoist_sp_expect of tests/ct_model.py) at 4096 x 3, L = 2, one record whose c1 rows hold 0, 1,
    (q - 1)/2, (q + 1)/2 and q - 1 on negated and on kept positions, random key words: with one element it equals the
    definition of se_amd_ct_galois_sp_device bit for bit (centring commutes with sigma), for both elements; with the
    elements {3, n + 1} it differs from the sum of the two single key switches in at least one word of each half (one
    rounding, not two).  All-ones weights with an all-ones diag0 give the sum form with add_input."""
    from oracle import pyoracle
    pyoracle.build(ref=False)
    n, npr, L = 4096, 3, 2
    o = pyoracle.Oracle(n, npr)
    q = o.q
    rng = np.random.default_rng(4096 * 3 + 17)
    elts = [3, n + 1]
    keys = [tuple(np.stack([np.stack([rng.integers(0, q[i], n, dtype=np.uint32) for i in range(npr)])
                            for _ in range(npr - 1)]) for _ in range(2)) for _ in elts]
    c0 = np.stack([rng.integers(0, q[j], n, dtype=np.uint32) for j in range(L)])[None]
    c1 = np.stack([edge_row(o, j, rng, elts, edges="centring") for j in range(L)])[None]
    for g, key in zip(elts, keys):
        h0, h1, info = hoist_sp_expect(o, c0, c1, [g], [key])
        e0, e1 = galois_sp_expect(o, c0, c1, g, *key)
        assert (h0 == e0).all() and (h1 == e1).all(), g
        assert len(info) == 1 and info[0]["delta"][0].shape == (n,) and len(info[0]["D"]) == L
    h0, h1, _ = hoist_sp_expect(o, c0, c1, elts, keys)
    s0, s1 = sum_of_single_calls(o, c0, c1, elts, keys)
    differ = int((h0 != s0).sum()), int((h1 != s1).sum())
    print(f"words that differ from the sum of two single key switches: {differ} of {h0.size}")
    assert differ[0] > 0 and differ[1] > 0
    # all-ones weights and an all-ones diag0 are the sum form with add_input
    ones = np.ones((len(elts), npr, n), dtype=np.uint32)
    a0, a1, _ = hoist_sp_expect(o, c0, c1, elts, keys, w0=1)
    w0_, w1_, _ = hoist_sp_expect(o, c0, c1, elts, keys, weights=ones, w0=ones[0])
    assert (a0 == w0_).all() and (a1 == w1_).all()


def test_noise_tool_moving_sum_and_matvec_on_fresh_records_stay_inside_the_acceptance():
    """tools/ct_keyswitch_sp_noise_sim.py at the shapes the GPU tests use, 4096 x 3 with L = 2 and 8192 x 6 with L = 5: a
    moving sum of a fresh record and its 7 rotations in one call, decoded at Delta, and an 8 x 8 matrix-vector product
    with diagonals encoded at Delta, no lift and one rescale, both decode within the reference's 0.1 (the simulation
    gives 1.1e-3 and 3.5e-3 for the sum, 3.4e-3 and 8.9e-3 for the product; the table of INTEGRATION section 4l holds
    every figure), so both shapes stay in the GPU test.  The single rounding is not worse than 7 roundings: a division by P adds -(delta_0 + delta_1 s)
    / P to the decrypted value, every coefficient of delta_k / P uniform in (-1/2, 1/2], so 7 independent divisions add a
    term of 7^(1/2) times the root mean square of one (in the matrix-vector product each of them is multiplied by its
    diagonal on top); the root mean squares over the coefficients are compared.  The largest key-switch coefficient and
    the slot error of both forms are printed, not ordered: the term both forms share, sum_j D_j e_j / P, dominates them."""
    from oracle import pyoracle
    pyoracle.build(ref=False)
    from tools import ct_keyswitch_sp_noise_sim as sim
    for n, npr, L in ((4096, 3, 2), (8192, 6, 5)):
        for row in (sim.moving_sum(n, npr, L, 7), sim.matvec(n, npr, L)):
            print(row)
            assert row["slot_error"] < 0.1, row
            assert row["rounding_rms"] <= row["rounding_rms_single"], row
