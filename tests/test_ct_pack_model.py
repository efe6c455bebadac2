"""The host model of slot packing (tests/ct_model_pack.py) checked on the CPU at 4096 x 2 (L = 1) and 4096 x 3 (L = 2): the
five facts of the header block against the special-prime definitions of tests/ct_model.py, and the exact identity of a
packed row under keys made by the oracle.  The GPU module holds the kernels to this model."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vectors as V
from ct_model import (centred, galois_sp_expect, hoist_sp_expect, key_errors, modular_sum, rand_key, rand_slab,
                      sigma_rows, sp_key, sum_of_single_calls)
from ct_model_pack import pack_expect, pack_row_quotient, single_deltas, sum_of_single_rotations
from vectors import sigma_coeff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
SHAPES = [(2, 1), (3, 2)]                                      # (np, L)
ELTS = [3, 1, N + 1, 2 * N - 1, 3]                             # the identity and a repeated element among them
B = 4


@pytest.fixture(scope="module")
def oracles():
    from oracle import pyoracle
    pyoracle.build(ref=False)
    return {npr: pyoracle.Oracle(N, npr) for npr, _ in SHAPES}


@pytest.fixture(scope="module")
def cases(oracles):
    """Per shape: B = 4 random records at level L and one random special-prime key per listed element (the repeated
    element has a key of its own per listing: the model takes the key of the element INDEX); computed once, left
    unchanged."""
    out = {}
    for npr, L in SHAPES:
        o = oracles[npr]
        rng = np.random.default_rng(4096 * npr + 23)
        keys = [None if g == 1 else (rand_key(rng, o.q, N), rand_key(rng, o.q, N)) for g in ELTS]
        keys[4] = keys[0]                                      # one installed key per element
        out[(npr, L)] = dict(o=o, L=L, keys=keys, c0=rand_slab(rng, o.q, B, N, L), c1=rand_slab(rng, o.q, B, N, L))
    return out


@pytest.fixture(params=SHAPES, ids=lambda s: f"4096x{s[0]}-L{s[1]}")
def case(cases, request):
    return cases[request.param]


def test_model_imports_neither_torch_nor_pytest():
    code = ("import sys; sys.path[:0] = [%r, %r]; import ct_model_pack; "
            "assert not {'torch', 'pytest', 'seal_embedded_amd'} & set(sys.modules)" % (os.path.join(ROOT, "tests"), ROOT))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_fact_1_a_row_of_one_rotated_entry_is_the_single_rotation(case):
    o, c0, c1, keys = (case[k] for k in ("o", "c0", "c1", "keys"))
    rows = [[(0, 0)], [(1, 2)], [(2, 3)], [(3, 4)], []]
    r0, r1, info = pack_expect(o, c0, c1, ELTS, rows, keys)
    for g, row in enumerate(rows[:4]):
        b, e = row[0]
        e0, e1 = galois_sp_expect(o, c0[b:b + 1], c1[b:b + 1], ELTS[e], *keys[e])
        assert (r0[g] == e0[0]).all() and (r1[g] == e1[0]).all(), g
    assert not r0[4].any() and not r1[4].any() and not info[4]["delta"][0].any()


@pytest.mark.parametrize("identity", [False, True], ids=["rotations", "with-identity"])
def test_fact_2_one_record_under_every_element_is_the_hoisted_sum(case, identity):
    o, c0, c1, keys = (case[k] for k in ("o", "c0", "c1", "keys"))
    b = 1
    listed = [e for e, g in enumerate(ELTS) if identity or g != 1]
    r0, r1, _ = pack_expect(o, c0, c1, ELTS, [[(b, e) for e in listed]], keys)
    rotated = [e for e in listed if ELTS[e] != 1]
    h0, h1, _ = hoist_sp_expect(o, c0[b:b + 1], c1[b:b + 1], [ELTS[e] for e in rotated], [keys[e] for e in rotated],
                                w0=1 if identity else None)
    assert (r0[0] == h0[0]).all() and (r1[0] == h1[0]).all()


def test_fact_3_identity_rows_are_plain_modular_sums(case):
    o, c0, c1, keys = (case[k] for k in ("o", "c0", "c1", "keys"))
    row = [(2, 1), (0, 1), (2, 1)]
    r0, r1, info = pack_expect(o, c0, c1, ELTS, [row], keys)
    pick = [b for b, _ in row]
    assert (r0[0] == modular_sum(o, c0[pick][:, None])[0]).all() and (r1[0] == modular_sum(o, c1[pick][:, None])[0]).all()
    assert not info[0]["delta"][0].any() and not info[0]["delta"][1].any()


def test_fact_4_a_row_of_two_rotations_differs_from_two_single_calls_by_the_carry(case):
    """delta_row = centred(delta_a + delta_b mod P) = delta_a + delta_b - c P with c in {-1, 0, 1}: in the coefficient
    domain the row minus the modular sum of the two single rotations is exactly c, on every prime and both halves -- they
    agree wherever |delta_a + delta_b| <= (P - 1)/2 and differ elsewhere, which on random slabs is somewhere."""
    o, L, c0, c1, keys = (case[k] for k in ("o", "L", "c0", "c1", "keys"))
    P = o.q[o.np - 1]
    # one record under two elements, against ct_model.sum_of_single_calls; two records, against the entry-wise sum
    for row in ([(1, 0), (1, 2)], [(0, 3), (2, 0)]):
        r0, r1, info = pack_expect(o, c0, c1, ELTS, [row], keys)
        if row[0][0] == row[1][0]:
            b = row[0][0]
            s0, s1 = sum_of_single_calls(o, c0[b:b + 1], c1[b:b + 1], [ELTS[e] for _, e in row], [keys[e] for _, e in row])
            s0, s1 = s0[0], s1[0]
            t0, t1 = sum_of_single_rotations(o, c0, c1, ELTS, row, keys)
            assert (s0 == t0).all() and (s1 == t1).all()
        else:
            s0, s1 = sum_of_single_rotations(o, c0, c1, ELTS, row, keys)
        singles = single_deltas(o, c1, ELTS, row, keys)
        for h, (r, s) in enumerate(((r0[0], s0), (r1[0], s1))):
            total = singles[0][h] + singles[1][h]
            num = total - info[0]["delta"][h]
            assert (num % P == 0).all()
            c = num // P
            assert set(np.unique(c)) <= {-1, 0, 1}
            assert ((c == 0) == (np.abs(total) <= (P - 1) // 2)).all()
            print(f"row {row}, half {h}: {float((c != 0).mean()):.4f} of the coefficients carry")
            assert (c != 0).any() and (r != s).any()
            for i in range(L):
                q = np.uint64(o.q[i])
                diff = ((r[i].astype(np.uint64) + q - s[i].astype(np.uint64)) % q).astype(np.uint32)
                assert (centred(o.intt(diff, i), o.q[i]) == c).all(), (h, i)


def test_fact_5_and_the_exact_identity_under_oracle_keys(case):
    """Keys from sp_key(o, sk, sigma_g(s_hat)): on every data prime the decryption of a packed row equals the sum of
    sigma_k of the records' decryptions plus NTT_i(pack_row_quotient), the quotient (T - delta_0 - delta_1 * s) / P being
    exact (pack_row_quotient asserts it) -- so the result is a level-L record under the same key, at the same scale."""
    o, L, c0, c1 = (case[k] for k in ("o", "L", "c0", "c1"))
    npr = o.np
    sk = V.secret_key(N, seed=5)
    s_hat = np.stack([o.ntt(o.expand_ternary(sk, j), j) for j in range(npr)])
    s_nat = centred(o.expand_ternary(sk, 0), o.q[0])
    keys, errs = [], []
    for e, g in enumerate(ELTS[:4]):
        if g == 1:
            keys.append(None)
            errs.append(None)
            continue
        target = sigma_rows(o, s_hat, g)[:npr - 1]
        k0, k1 = sp_key(o, sk, target, f"pack-model-{g}")
        keys.append((k0, k1))
        errs.append(key_errors(o, k0, k1, s_hat, target))
    elts = ELTS[:4]
    row = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 2)]
    r0, r1, info = pack_expect(o, c0, c1, elts, [row], keys)
    quo, t_max = pack_row_quotient(o, info[0], row, errs, s_nat)
    print(f"max |pack term| = {int(np.abs(quo).max())}, max |T| = {t_max}")
    for i in range(L):
        q = np.uint64(o.q[i])
        want = o.ntt((quo % o.q[i]).astype(np.uint32), i).astype(np.uint64)
        for b, e in row:
            m = o.intt(o.decrypt(c0[b, i], c1[b, i], s_hat[i], i), i)
            want = (want + o.ntt(sigma_coeff(m, elts[e], o.q[i]), i).astype(np.uint64)) % q
        assert (o.decrypt(r0[0, i], r1[0, i], s_hat[i], i) == want.astype(np.uint32)).all(), i
