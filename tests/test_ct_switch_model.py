"""The host model of the switch-key ring (tests/ct_model_switch.py) checked on the CPU at 4096 x 3, L = 2: its pieces
against the special-prime definitions of tests/ct_model.py and against one another, the exact identity of a switching
key, and the noise simulation tools/ct_switch_noise_sim.py against the reference's 0.1.  The GPU module holds the kernels
to this model."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vectors as V
from ct_model import add_mod, centred, key_errors, key_switch_sp, rand_slab, relin_sp_expect, sp_key, switch_quotient
from ct_model_switch import random_ring, sum_of_single_switches, switch_expect, switch_sum_expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NP, L = 4096, 3, 2


@pytest.fixture(scope="module")
def o():
    from oracle import pyoracle
    pyoracle.build(ref=False)
    return pyoracle.Oracle(N, NP)


@pytest.fixture(scope="module")
def case(o):
    """B = 4 random records at level 2, a ring of K = 3 random keys, key indices that use every key, and the single
    switches of all records (computed once, left unchanged)."""
    rng = np.random.default_rng(4096 * 3 + 17)
    wk0, wk1 = random_ring(rng, o.q, 3, N)
    c0, c1 = rand_slab(rng, o.q, 4, N, L), rand_slab(rng, o.q, 4, N, L)
    key_idx = np.array([2, 0, 1, 2], dtype=np.uint32)
    return dict(wk0=wk0, wk1=wk1, c0=c0, c1=c1, key_idx=key_idx, single=switch_expect(o, c0, c1, key_idx, wk0, wk1))


def test_model_imports_neither_torch_nor_pytest():
    code = ("import sys; sys.path[:0] = [%r, %r]; import ct_model_switch; "
            "assert not {'torch', 'pytest', 'seal_embedded_amd'} & set(sys.modules)" % (os.path.join(ROOT, "tests"), ROOT))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_switch_is_the_relinearisation_of_c0_0_c1_under_the_records_key(o, case):
    s0, s1 = case["single"]
    zero = np.zeros_like(case["c1"])
    for b, k in enumerate(case["key_idx"]):
        e0, e1 = relin_sp_expect(o, case["c0"][b:b + 1], zero[b:b + 1], case["c1"][b:b + 1], case["wk0"][k], case["wk1"][k])
        assert (s0[b] == e0[0]).all() and (s1[b] == e1[0]).all(), b


def test_singleton_rows_are_single_switches_and_an_empty_row_is_zero(o, case):
    rows = [[b] for b in range(4)] + [[]]
    r0, r1, info = switch_sum_expect(o, case["c0"], case["c1"], case["key_idx"], rows, case["wk0"], case["wk1"])
    assert (r0[:4] == case["single"][0]).all() and (r1[:4] == case["single"][1]).all()
    assert not r0[4].any() and not r1[4].any() and not info[4]["delta"][0].any()


def test_a_row_of_two_is_not_the_sum_of_two_switches_and_differs_by_the_carry(o, case):
    """delta_row = centred(delta_a + delta_b mod P) = delta_a + delta_b - c P with c in {-1, 0, 1}, so the row minus the
    modular sum of the two single switches is NTT_i(c P) . P^-1 = NTT_i(c mod q_i) on every prime, for both halves: in the
    coefficient domain the two differ by exactly c, wherever c != 0.  The share of such coefficients is printed."""
    c0, c1, key_idx, wk0, wk1 = (case[k] for k in ("c0", "c1", "key_idx", "wk0", "wk1"))
    P = o.q[NP - 1]
    row = [0, 1]
    r0, r1, info = switch_sum_expect(o, c0, c1, key_idx, [row], wk0, wk1)
    s0, s1 = sum_of_single_switches(o, c0, c1, key_idx, row, wk0, wk1)
    singles = [key_switch_sp(o, c1[b], wk0[key_idx[b]], wk1[key_idx[b]])["delta"] for b in row]
    for h, (r, s) in enumerate(((r0[0], s0), (r1[0], s1))):
        num = singles[0][h] + singles[1][h] - info[0]["delta"][h]
        assert (num % P == 0).all()
        c = num // P
        assert set(np.unique(c)) <= {-1, 0, 1}
        share = float((c != 0).mean())
        print(f"half {h}: {share:.4f} of the coefficients carry (|delta_a + delta_b| > P/2)")
        assert (c != 0).any() and (r != s).any()
        for i in range(L):
            q = np.uint64(o.q[i])
            diff = ((r[i].astype(np.uint64) + q - s[i].astype(np.uint64)) % q).astype(np.uint32)
            assert (centred(o.intt(diff, i), o.q[i]) == c).all(), (h, i)


def test_switching_key_identity_is_an_exact_quotient(o):
    """A key from sp_key(o, sk_to, target = NTT(s_from)): its errors recovered under s_to with the diagonal of s_from are
    small and agree on the first and the special prime (key_errors), and T - delta_0 - delta_1 * s_to is divisible by P
    (switch_quotient asserts it): the switch moves c1 . s_from under s_to up to that quotient."""
    sk_to, sk_from = V.secret_key(N, seed=5), V.secret_key(N, seed=101)
    hat = lambda sk: np.stack([o.ntt(o.expand_ternary(sk, j), j) for j in range(NP)])  # noqa: E731
    s_to, s_from = hat(sk_to), hat(sk_from)
    k0, k1 = sp_key(o, sk_to, s_from[:NP - 1], "switch-model")
    errs = key_errors(o, k0, k1, s_to, s_from[:NP - 1])
    s_nat = centred(o.expand_ternary(sk_to, 0), o.q[0])
    d = rand_slab(np.random.default_rng(9), o.q, 1, N, L)[0]
    quo = switch_quotient(o, d, k0, k1, errs, s_nat)
    print(f"max |switch term| = {int(np.abs(quo).max())}")
    # and the identity itself: ks_0 + ks_1 s_to = d s_from + quotient on every data prime
    ks0, ks1 = key_switch_sp(o, d, k0, k1)["ks"]
    zero = np.zeros(N, dtype=np.uint32)
    lhs = np.stack([o.decrypt(ks0[i], ks1[i], s_to[i], i) for i in range(L)])
    moved = np.stack([o.decrypt(zero, d[i], s_from[i], i) for i in range(L)])
    term = np.stack([o.ntt((quo % o.q[i]).astype(np.uint32), i) for i in range(L)])
    assert (lhs == add_mod(o, moved, term)).all()


def test_noise_tool_rows_of_one_and_eight_decode_within_the_references_bound():
    """tools/ct_switch_noise_sim.py at 4096 x 3, L = 2: a row of 1 and a row of 8 fresh records under 8 device keys,
    decoded under the aggregator key alone, are within the reference's 0.1 of the sums of the slot values in [-1, 1].
    As run: 7.1e-04 (m = 1) and 1.2e-03 (m = 8); both are printed, only 0.1 is asserted."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ct_switch_noise_sim as sim
    for m in (1, 8):
        r = sim.row(N, NP, L, m)
        print(f"row of {m}: slot error {r['slot_error']:.3e} (m single switches: {r['slot_error_single']:.3e}), "
              f"largest switch coefficient {r['key_switch_max']}")
        assert r["slot_error"] < 0.1 and r["slot_error_single"] < 0.1, r
