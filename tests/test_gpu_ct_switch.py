"""Switch-key rings (-m gpu): se_amd_gen_switch_keys_sp, se_amd_set_switch_keyring_sp, se_amd_ct_switch_keyed_sp_device and
se_amd_ct_switch_sum_keyed_sp_device.
Every expectation is the definition in tests/ct_model_switch.py on top of tests/ct_model.py: the oracle's primitives (ntt,
intt, decrypt, fft, expand_ternary) and Python / NumPy integers, never the code under test.  Every comparison is bit-exact
except the reference's own acceptance criterion |values - expected| < 0.1 (device/test/ckks_tests_common.c:132).
Oracle(n, L) is the oracle of a level-L record of Oracle(n, np): the default chains are prefixes of one another."""
import numpy as np
import pytest

import vectors as V
from ct_model import (CASE_IDS, SHAPE_IDS, SP_CASES, centred, edge_row, galois_seeds, galois_sp_expect, key_errors,
                      rand_key, rand_slab, relin_sp_expect, sp_diagonal, switch_quotient)
from ct_model_switch import random_ring, ring_seeds, row_quotient, switch_expect, switch_sum_expect
from gpu_support import (NULL, SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched,  # noqa: F401
                         assert_zero_prefix, check_level_decrypt, dev_t, dptr, drop_records, env, expectation,
                         guarded_pair, hptr, install_galois_keys, keyed_cases, ntt_secret, run_decrypt, run_example,
                         run_galois_sp, run_relin_sp, step_elements, stream_of, unit_values)

pytestmark = pytest.mark.gpu


# ---- the runners of the two entries: one call each, two rows of sentinels behind each output, status pre-filled with 77 ----
def csr(rows):
    """Lists of record indices -> (row_ptr [G + 1], idx [max(nnz, 1)], nnz)."""
    row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    flat = [b for r in rows for b in r]
    return row_ptr, np.array(flat + [0] * (not flat), dtype=np.uint32), len(flat)


def run_switch(env, ctx, c0, c1, key_idx, primes):
    """One ct_switch_keyed_sp call on device slabs [B][primes][n] -> (out0, out1 host, status host [B])."""
    B = c0.shape[0]
    st = env["torch"].full((B,), 77, dtype=env["torch"].uint8, device=env["dev"])
    out = guarded_pair(env, ctx.n, (B, primes, ctx.n), "switch",
                       lambda a, b: ctx.ct_switch_keyed_sp(c0, c1, key_idx, a, b, primes=primes, status=st))
    return out[0], out[1], st.cpu().numpy()


def run_switch_sum(env, ctx, c0, c1, key_idx, rows, primes, row_ptr=None):
    """One ct_switch_sum_keyed_sp call with the CSR form of `rows` (row_ptr: an override of the same length)
    -> (out0, out1 host [G][primes][n], status host [G])."""
    rp, idx, _ = csr(rows)
    rp = rp if row_ptr is None else np.asarray(row_ptr, dtype=np.uint32)
    G = len(rows)
    st = env["torch"].full((G,), 77, dtype=env["torch"].uint8, device=env["dev"])
    d_rp, d_idx = dev_t(env, rp), dev_t(env, idx)
    out = guarded_pair(env, ctx.n, (G, primes, ctx.n), "switch_sum", lambda a, b: ctx.ct_switch_sum_keyed_sp(
        c0, c1, key_idx, d_rp, d_idx[:sum(len(r) for r in rows)], a, b, primes=primes, status=st))
    return out[0], out[1], st.cpu().numpy()


# ---- test 1: the definition on arbitrary slabs and ring words -------------------------------------------------------
@pytest.mark.parametrize("shape,levels,_", SP_CASES, ids=CASE_IDS)
def test_switch_arbitrary_slabs_and_ring(env, shape, levels, _):
    """Test 1: random residues for the slabs and for a ring of K = 3 keys (key words 0, 1 and q_i - 1 on a data column
    and on the special prime's); record 0 of c1 holds 0, 1, (q_j - 1)/2, (q_j + 1)/2 and q_j - 1 among random
    coefficients, record 1 is all q_j - 1; the key indices use every key.  Entry 2 against the definition; a lower level
    uses rows j < L, columns i < L and column p of the same ring; the sentinels survive.  No secret key is installed."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    B, K = 3, 3
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    q = o.q
    rng = np.random.default_rng(43 * n + npr)
    wk0, wk1 = random_ring(rng, q, K, n)
    ctx.set_switch_keyring_sp(wk0, wk1)
    key_idx = np.array([2, 0, 1], dtype=np.uint32)
    for L in levels:
        c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
        for j in range(L):
            c1[0, j] = edge_row(o, j, rng, [], edges="centring")
        c0[1] = c1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
        e0, e1 = switch_expect(o, c0, c1, key_idx, wk0, wk1)
        g0, g1, st = run_switch(env, ctx, dev_t(env, c0), dev_t(env, c1), dev_t(env, key_idx), L)
        assert (g0 == e0).all() and (g1 == e1).all() and (st == 1).all(), L
    ctx.close()


# ---- test 2: the relinearisation twin -------------------------------------------------------------------------------
def test_switch_is_relin_sp_under_the_records_ring_key(env):
    """Test 2: at 4096 x 3, L = 2, B = 3 the outputs have the bytes of ct_relin_sp(c0, 0, c1) with ring key idx[b]
    installed as the relinearisation key, record by record."""
    torch = env["torch"]
    n, npr, L, B, K = 4096, 3, 2, 3, 3
    ctx = env["pkg"].Context(n, npr)
    q = ctx.moduli()
    rng = np.random.default_rng(4096 * 3 + 9)
    wk0, wk1 = random_ring(rng, q, K, n)
    ctx.set_switch_keyring_sp(wk0, wk1)
    key_idx = np.array([1, 2, 0], dtype=np.uint32)
    c0, c1 = dev_t(env, rand_slab(rng, q, B, n, L)), dev_t(env, rand_slab(rng, q, B, n, L))
    g0, g1, st = run_switch(env, ctx, c0, c1, dev_t(env, key_idx), L)
    assert (st == 1).all()
    for b in range(B):
        ctx.set_relin_key_sp(wk0[key_idx[b]], wk1[key_idx[b]])
        r0, r1 = run_relin_sp(env, ctx, c0, torch.zeros_like(c1), c1, L)
        assert g0[b].tobytes() == r0[b].tobytes() and g1[b].tobytes() == r1[b].tobytes(), b
    ctx.close()


# ---- test 3: the sum form against the model -------------------------------------------------------------------------
SUM_ROWS = [[], [2], [3, 3], [0, 2, 5], [1] * 17, [5, 0, 3, 1]]


@pytest.mark.parametrize("shape,levels", [((4096, 3), (2, 1)), ((4096, 2), (1,))], ids=CASE_IDS)
def test_switch_sum_rows_against_the_model(env, shape, levels):
    """Test 3: B = 6 records, K = 3 keys, one call whose rows are: an empty row; a singleton, whose bytes equal entry 2's;
    a row with one record twice; a row mixing all three keys; 17 entries over the all-(q_j - 1) record, whose key holds
    q_i - 1 in every word (the lazy range: the largest product on every term); a row in non-monotone record order."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    B, K = 6, 3
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    q = o.q
    rng = np.random.default_rng(47 * n + npr)
    wk0, wk1 = random_ring(rng, q, K, n)
    wk0[1] = wk1[1] = (np.array(q, dtype=np.uint32) - 1)[None, :, None]
    ctx.set_switch_keyring_sp(wk0, wk1)
    key_idx = np.array([0, 1, 2, 2, 0, 1], dtype=np.uint32)
    assert {int(key_idx[b]) for b in SUM_ROWS[3]} == {0, 1, 2} and key_idx[1] == 1
    for L in levels:
        c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
        c0[1] = c1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
        e0, e1, _ = switch_sum_expect(o, c0, c1, key_idx, SUM_ROWS, wk0, wk1)
        d0, d1, dk = dev_t(env, c0), dev_t(env, c1), dev_t(env, key_idx)
        g0, g1, st = run_switch_sum(env, ctx, d0, d1, dk, SUM_ROWS, L)
        assert (st == 1).all(), st
        for g in range(len(SUM_ROWS)):
            assert (g0[g] == e0[g]).all() and (g1[g] == e1[g]).all(), (L, g)
        assert not g0[0].any() and not g1[0].any()
        s0, s1, _ = run_switch(env, ctx, d0, d1, dk, L)
        assert g0[1].tobytes() == s0[2].tobytes() and g1[1].tobytes() == s1[2].tobytes(), L
    ctx.close()


def test_switch_sum_row_of_two_at_16384x13(env):
    """Test 3, LOGN 14 and the long prime loop: one row of 2 records under 2 keys at 16384 x 13, L = 12."""
    from oracle.pyoracle import Oracle
    n, npr, L, B, K = 16384, 13, 12, 2, 2
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(53 * n + npr)
    wk0, wk1 = random_ring(rng, o.q, K, n)
    ctx.set_switch_keyring_sp(wk0, wk1)
    key_idx = np.array([1, 0], dtype=np.uint32)
    c0, c1 = rand_slab(rng, o.q, B, n, L), rand_slab(rng, o.q, B, n, L)
    e0, e1, _ = switch_sum_expect(o, c0, c1, key_idx, [[0, 1]], wk0, wk1)
    g0, g1, st = run_switch_sum(env, ctx, dev_t(env, c0), dev_t(env, c1), dev_t(env, key_idx), [[0, 1]], L)
    assert (st == 1).all() and (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


# ---- test 4: the delta boundary across records ----------------------------------------------------------------------
def test_switch_sum_delta_boundary_across_records(env):
    """Test 4 at 4096 x 3, L = 1: two keys whose row 0, column p of half 0 is the NTT of the constant 1 (all ones), so
    delta_0 of a row of two records is centred(D_{a,0} + D_{b,0} mod P); two records under the two keys with D_{a,0} +
    D_{b,0} = (P - 1)/2, (P + 1)/2, -(P - 1)/2, -(P + 1)/2 and 0 on the first five coefficients (reachable: q_0 - 1 >=
    (P + 1)/2), which the oracle confirms, with delta_0 = (P - 1)/2, -(P - 1)/2, -(P - 1)/2, (P - 1)/2, 0 there."""
    from oracle.pyoracle import Oracle
    n, npr, L, B, K = 4096, 3, 1, 2, 2
    o = Oracle(n, npr)
    q, p = o.q, npr - 1
    P = q[p]
    assert q[0] - 1 >= (P + 1) // 2
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(79)
    wk0, wk1 = random_ring(rng, q, K, n)
    wk0[0, 0, p] = wk0[1, 0, p] = 1
    assert (o.ntt(np.eye(1, n, 0, dtype=np.uint32)[0], p) == 1).all()
    ctx.set_switch_keyring_sp(wk0, wk1)
    key_idx = np.array([0, 1], dtype=np.uint32)
    sums = np.array([(P - 1) // 2, (P + 1) // 2, -(P - 1) // 2, -(P + 1) // 2, 0], dtype=np.int64)
    a = np.array([(q[0] - 1) // 2, (q[0] - 1) // 2, -(q[0] - 1) // 2, -(q[0] - 1) // 2, 5], dtype=np.int64)
    b = sums - a
    assert (np.abs(b) <= (q[0] - 1) // 2).all()
    c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
    for rec, vals in ((0, a), (1, b)):
        c = o.intt(c1[rec, 0], 0)
        c[:5] = vals % q[0]
        c1[rec, 0] = o.ntt(c, 0)
    rows = [[0, 1]]
    e0, e1, info = switch_sum_expect(o, c0, c1, key_idx, rows, wk0, wk1)
    assert ((info[0]["D"][0][0] + info[0]["D"][1][0])[:5] == sums).all()
    assert (info[0]["delta"][0][:5] == [(P - 1) // 2, -(P - 1) // 2, -(P - 1) // 2, (P - 1) // 2, 0]).all()
    g0, g1, st = run_switch_sum(env, ctx, dev_t(env, c0), dev_t(env, c1), dev_t(env, key_idx), rows, L)
    assert (st == 1).all() and (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


# ---- test 5: key generation, installs and their refusals ------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_switch_key_generation_and_installs(env, shape):
    """Test 5: gen_switch_keys_sp with K = 2 equals gen_keys_batch(K = np - 1, sk_to replicated, the key's block of seeds)
    plus (P mod q_j) . NTT_j(s_from_k) on column j of row j; exactly those columns differ and column p has no diagonal; the
    generator installs nothing.  SE_ERR_NO_KEY before an install; a word == q_i, a code 3 in sk_to or in one sk_from and
    K = 0 are refused; a refused install leaves the previous ring working with the same bits; a new install replaces the
    ring; the ring and the special-prime relinearisation / Galois keys are installed sets of their own."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    pkg = env["pkg"]
    n, npr = shape
    R, p, L, K, B = npr - 1, npr - 1, npr - 1, 2, 2
    o = Oracle(n, npr)
    ctx = pkg.Context(n, npr)
    sk_to = V.secret_key(n, seed=3)
    sk_from = np.stack([V.secret_key(n, seed=21), V.secret_key(n, seed=22)])
    sa, se = ring_seeds(npr, K, "switch-keygen")
    wk0, wk1 = ctx.gen_switch_keys_sp(sk_from, sk_to, sa, se)
    assert wk0.shape == (K, R, npr, n)
    for k in range(K):
        _, pk0, pk1 = ctx.gen_keys_batch(sa[k], se[k], sk_in=np.tile(sk_to, (R, 1)))
        target = np.stack(ntt_secret(o, sk_from[k]))[:R]
        exp0 = pk0.copy()
        for j in range(R):
            exp0[j, j] = (pk0[j, j].astype(np.uint64) + sp_diagonal(o, target, j)) % np.uint64(o.q[j])
        assert (wk1[k] == pk1).all() and (wk0[k] == exp0).all(), k
        assert (wk0[k] != pk0).any(axis=2).sum() == R and (wk0[k][:, p] == pk0[:, p]).all(), k
    # the generator installed nothing: no secret key, no ring
    rng = np.random.default_rng(n + npr + 1)
    c0, c1, c2 = (rand_slab(rng, o.q, B, n, L) for _ in range(3))
    d0, d1, d2 = dev_t(env, c0), dev_t(env, c1), dev_t(env, c2)
    key_idx = np.array([1, 0], dtype=np.uint32)
    dk = dev_t(env, key_idx)
    rows = [[0, 1], [1]]
    rp, idx, nnz = csr(rows)
    d_rp, d_idx = dev_t(env, rp), dev_t(env, idx)
    out0, out1 = torch.full_like(d0, SENTINEL), torch.full_like(d0, SENTINEL)
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    one = CEntry(ctx.L.se_amd_ct_switch_keyed_sp_device, ctx=ctx.h, c0=dptr(d0), c1=dptr(d1), B=B, primes=L,
                 key_idx=dptr(dk), out0=dptr(out0), out1=dptr(out1), status=dptr(st), stream=stream_of(env))
    many = CEntry(ctx.L.se_amd_ct_switch_sum_keyed_sp_device, ctx=ctx.h, c0=dptr(d0), c1=dptr(d1), B=B, primes=L,
                  key_idx=dptr(dk), G=len(rows), row_ptr=dptr(d_rp), idx=dptr(d_idx), nnz=nnz, out0=dptr(out0),
                  out1=dptr(out1), status=dptr(st), stream=stream_of(env))
    assert ctx.L.se_amd_decrypt_level_device(ctx.h, dptr(d0), dptr(d1), B, L, ctx.scale(), NULL, NULL, NULL, dptr(st),
                                             stream_of(env)) == SE_ERR_NO_KEY
    assert one() == SE_ERR_NO_KEY and many() == SE_ERR_NO_KEY
    # a refused first install installs nothing
    bad0 = wk0.copy()
    bad0[0, 0, 0, 0] = o.q[0]
    with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
        ctx.set_switch_keyring_sp(bad0, wk1)
    assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    assert one() == SE_ERR_NO_KEY and many() == SE_ERR_NO_KEY
    assert_untouched(out0, out1)
    assert_untouched(st, fill=77)
    ctx.set_switch_keyring_sp(wk0, wk1)
    want = switch_expect(o, c0[:1], c1[:1], key_idx[:1], wk0, wk1)

    def ring_works():
        g0, g1, s = run_switch(env, ctx, d0, d1, dk, L)
        assert (g0[:1] == want[0]).all() and (g1[:1] == want[1]).all() and (s == 1).all()
        return (g0, g1) + run_switch_sum(env, ctx, d0, d1, dk, rows, L)[:2]

    before = ring_works()
    bad1 = wk1.copy()
    bad1[K - 1, R - 1, p, n - 1] = o.q[p]
    for k0, k1 in ((bad0, wk1), (wk0, bad1)):                                 # a word == q_i, either half
        with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
            ctx.set_switch_keyring_sp(k0, k1)
        assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    install = CEntry(ctx.L.se_amd_set_switch_keyring_sp, ctx=ctx.h, K=K, wk0=hptr(wk0), wk1=hptr(wk1))
    install.refused([dict(K=0), dict(wk0=NULL)])
    assert all((a == b).all() for a, b in zip(before, ring_works()))          # the same bits as before
    # the generator's own refusals; nothing is written
    bad_sk = sk_to.copy()
    bad_sk[5] |= 0x03
    bad_from = sk_from.copy()
    bad_from[1, n // 4 - 1] |= 0x30
    t0, t1 = np.zeros_like(wk0), np.zeros_like(wk1)
    gen = CEntry(ctx.L.se_amd_gen_switch_keys_sp, ctx=ctx.h, K=K, sk_from=hptr(sk_from), sk_to=hptr(sk_to),
                 seeds_a=hptr(sa), seeds_e=hptr(se), wk0=hptr(t0), wk1=hptr(t1))
    gen.refused([dict(sk_to=hptr(bad_sk)), dict(sk_from=hptr(bad_from)), dict(K=0), dict(sk_from=NULL), dict(wk1=NULL)])
    assert not t0.any() and not t1.any()
    # the ring and the special-prime evaluation keys are installed sets of their own
    rel = CEntry(ctx.L.se_amd_ct_relin_sp_device, ctx=ctx.h, c0=dptr(d0), c1=dptr(d1), c2=dptr(d2), B=B, primes=L,
                 out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    assert rel() == SE_ERR_NO_KEY                                             # the ring does not serve the relinearisation
    ek = [rand_key(rng, o.q, n) for _ in range(4)]
    ctx.set_relin_key_sp(ek[0], ek[1])
    ctx.set_galois_keys_sp([3], ek[2][None], ek[3][None])
    evk = lambda: run_relin_sp(env, ctx, d0, d1, d2, L) + run_galois_sp(env, ctx, d0, d1, 3, L)  # noqa: E731
    evk_before = evk()
    assert all((a == b).all() for a, b in zip(before, ring_works()))          # installing them changed no ring result
    # a new install replaces the ring: the keys in the other order
    ctx.set_switch_keyring_sp(wk0[::-1], wk1[::-1])
    g0, g1, s = run_switch(env, ctx, d0, d1, dev_t(env, 1 - key_idx), L)
    assert (g0 == before[0]).all() and (g1 == before[1]).all() and (s == 1).all()
    g0, g1, s = run_switch(env, ctx, d0, d1, dk, L)
    swapped = switch_expect(o, c0[:1], c1[:1], 1 - key_idx[:1], wk0, wk1)
    assert (g0[:1] == swapped[0]).all() and (g1[:1] == swapped[1]).all() and (g0[0] != before[0][0]).any()
    assert all((a == b).all() for a, b in zip(evk_before, evk()))             # and the other way round
    ctx.close()


# ---- test 6: status and arguments -----------------------------------------------------------------------------------
def test_switch_status(env):
    """Test 6, status: entry 2 gives a record whose key index is >= K status 2 and zero outputs, the other records their
    results; entry 3 gives a row with a record index >= B, a member whose key index is >= K, a decreasing or an overlong
    row_ptr pair status 2 and zero rows in both slabs, and every other row its result."""
    from oracle.pyoracle import Oracle
    n, npr, L, B, K = 4096, 3, 2, 4, 2
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(83)
    wk0, wk1 = random_ring(rng, o.q, K, n)
    ctx.set_switch_keyring_sp(wk0, wk1)
    c0, c1 = rand_slab(rng, o.q, B, n, L), rand_slab(rng, o.q, B, n, L)
    d0, d1 = dev_t(env, c0), dev_t(env, c1)
    key_idx = np.array([1, K, 0, 0xFFFFFFFF], dtype=np.uint32)
    good = [0, 2]
    e0, e1 = switch_expect(o, c0[good], c1[good], key_idx[good], wk0, wk1)
    g0, g1, st = run_switch(env, ctx, d0, d1, dev_t(env, key_idx), L)
    assert list(st) == [1, 2, 1, 2]
    assert (g0[good] == e0).all() and (g1[good] == e1).all()
    assert not g0[[1, 3]].any() and not g1[[1, 3]].any()
    # rows: good | record index >= B | a member with a bad key index | good | empty
    rows = [[0, 2], [2, B], [0, 1, 2], [2, 2, 0], []]
    s0, s1, _ = switch_sum_expect(o, c0, c1, key_idx, [rows[0], rows[3]], wk0, wk1)
    g0, g1, st = run_switch_sum(env, ctx, d0, d1, dev_t(env, key_idx), rows, L)
    assert list(st) == [1, 2, 2, 1, 1]
    assert (g0[[0, 3]] == s0).all() and (g1[[0, 3]] == s1).all()
    assert not g0[[1, 2, 4]].any() and not g1[[1, 2, 4]].any()
    # row_ptr pairs: rows of [0, 2 | 2, 0] with pointers 0, 2, 1, 4, 9 (nnz = 4): good, decreasing, (1, 4) good, overlong
    rows = [[0, 2], [], [2, 0], []]
    rp = [0, 2, 1, 4, 9]
    s0, s1, _ = switch_sum_expect(o, c0, c1, key_idx, [[0, 2], [2, 2, 0]], wk0, wk1)
    g0, g1, st = run_switch_sum(env, ctx, d0, d1, dev_t(env, key_idx), rows, L, row_ptr=rp)
    assert list(st) == [1, 2, 1, 2]
    assert (g0[[0, 2]] == s0).all() and (g1[[0, 2]] == s1).all()
    assert not g0[[1, 3]].any() and not g1[[1, 3]].any()
    ctx.close()


def test_switch_arguments(env):
    """Test 6, arguments: every argument error returns -22 and writes nothing: NULL, alignment, primes outside
    [1, np - 1] (primes = np among them), B / G / nnz >= 2^32, and every entry on a context of one prime.  B = 0 resp.
    G = 0 is a successful no-op; a level-1 call writes B . n resp. G . n words and nothing behind them."""
    torch = env["torch"]
    n, npr, B, G = 4096, 3, 2, 2
    ctx = env["pkg"].Context(n, npr)
    L = ctx.L
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    ki = torch.zeros(B, dtype=torch.int32, device=env["dev"])
    rp = dev_t(env, np.array([0, 1, 2], dtype=np.uint32))
    ix = dev_t(env, np.array([1, 0], dtype=np.uint32))
    s = stream_of(env)
    f2 = CEntry(L.se_amd_ct_switch_keyed_sp_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, primes=2, key_idx=dptr(ki),
                out0=dptr(out0), out1=dptr(out1), status=dptr(st), stream=s)
    f3 = CEntry(L.se_amd_ct_switch_sum_keyed_sp_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, primes=2,
                key_idx=dptr(ki), G=G, row_ptr=dptr(rp), idx=dptr(ix), nnz=2, out0=dptr(out0), out1=dptr(out1),
                status=dptr(st), stream=s)
    key = np.zeros((2, npr - 1, npr, n), dtype=np.uint32)
    ctx.set_switch_keyring_sp(key, key)
    f2.refused([
        dict(ctx=None),
        dict(c0=NULL),                                                          # NULL mandatory pointers
        dict(c1=NULL),
        dict(key_idx=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(primes=0),                                                         # primes outside [1, np - 1]
        dict(primes=3),                                                         # primes = np
        dict(primes=4),
        dict(B=2 ** 32),                                                        # B >= 2^32
        dict(c0=dptr(c0, 4)),                                                   # alignment, each slab
        dict(c1=dptr(c1, 8)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
    ])
    f3.refused([
        dict(ctx=None),
        dict(c0=NULL),
        dict(c1=NULL),
        dict(key_idx=NULL),
        dict(row_ptr=NULL),
        dict(idx=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(primes=0),
        dict(primes=3),
        dict(B=2 ** 32),
        dict(G=2 ** 32),
        dict(nnz=2 ** 32),
        dict(c0=dptr(c0, 4)),
        dict(c1=dptr(c1, 8)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
    ])
    assert f2(B=0) == 0
    assert f3(G=0) == 0
    # a context of one prime has no prime to reserve
    one = env["pkg"].Context(1024, 1)
    k1 = np.zeros((1, 1, 1, 1024), dtype=np.uint32)
    sd = np.zeros((1, 64), dtype=np.uint8)
    sk = V.secret_key(1024, seed=3)
    f2.refused([dict(ctx=one.h, primes=1)])
    f3.refused([dict(ctx=one.h, primes=1)])
    assert L.se_amd_set_switch_keyring_sp(one.h, 1, hptr(k1), hptr(k1)) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_gen_switch_keys_sp(one.h, 1, hptr(sk), hptr(sk), hptr(sd), hptr(sd), hptr(k1),
                                       hptr(k1)) == SE_ERR_INVALD_ARGUMENT
    assert not k1.any()
    one.close()
    assert_untouched(out0, out1)
    assert_untouched(st, fill=77)
    for f in (f2, f3):
        out0.fill_(SENTINEL)
        out1.fill_(SENTINEL)
        assert f(primes=1) == 0
        for o in (out0, out1):
            assert_zero_prefix(o, B * n)
        assert bool((st == 1).all())
    ctx.close()


# ---- tests 7 and 8: real keys -----------------------------------------------------------------------------------------
KEYS = 3
KEY_IDX = np.array([0, 1, 2, 1, 2, 0], dtype=np.uint32)


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key, the TARGET key of the ring:
    K = 3 device keys, installed as the secret ring; the switching keys from each of them to the case's key, generated on
    the device and installed; the errors of every switching key, recovered with the oracle; the special-prime Galois key
    of step 1 under the case's key, installed; B = 6 records with slot values in [-1, 1] under the device keys KEY_IDX
    (keyed symmetric encryption), dropped to np - 1 primes by ct_drop_primes."""
    torch = env["torch"]
    ctx, o = case["ctx"], case["o"]
    n, npr = ctx.n, ctx.np
    B = len(KEY_IDX)
    sk_dev = np.stack([V.secret_key(n, seed=30 + k) for k in range(KEYS)])
    dev_hat = [ntt_secret(o, sk) for sk in sk_dev]
    ctx.set_secret_keyring(sk_dev)
    wk0, wk1 = ctx.gen_switch_keys_sp(sk_dev, case["sk"], *ring_seeds(npr, KEYS, "switch-e2e"))
    ctx.set_switch_keyring_sp(wk0, wk1)
    errs = [key_errors(o, wk0[k], wk1[k], case["s_hat"], np.stack(dev_hat[k][:npr - 1])) for k in range(KEYS)]
    elts = step_elements(env, n, (1,))
    gk0, gk1 = install_galois_keys(case, elts, "switch-gk", sp=True)
    vals = unit_values(B, n, 5000 + n)
    ss, sd = V.bench_seeds(B, first=300)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encrypt_sym_keyed(dev_t(env, vals), dev_t(env, KEY_IDX), dev_t(env, ss), dev_t(env, sd), c0, c1, status=st)
    torch.cuda.synchronize()
    assert bool((st == 1).all())
    case.update(wk0=wk0, wk1=wk1, errs=errs, dev_hat=dev_hat, elt=elts[0], gk0=gk0[0], gk1=gk1[0], vals=vals,
                fresh=(c0, c1), dropped=drop_records(env, ctx, c0, c1, npr - 1))


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_switch_exact_identity_with_real_keys(env, keyed_cases, shape):
    """Test 7, at L = np - 1 on fresh dropped records of two device keys: with y the oracle's centred decrypt of a record
    under its OWN key and y' that of the switched record under the target key, y' - y equals switch_quotient -- (T -
    delta_0 - delta_1 * s_to) / P with T = sum_j D_j * e_j, an exact quotient -- as integers.  For a row of two records
    under two keys, y' - (y_a + y_b) equals the quotient with T and delta of the row.  The largest term is printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    o, s_hat, ctx = c["o"], c["s_hat"], c["ctx"]
    n, npr = shape
    L = npr - 1
    lo = Oracle(n, L)
    s_nat = centred(o.expand_ternary(c["sk"], 0), o.q[0])
    pair = [0, 1]                                              # device keys 0 and 1
    l0, l1 = (x[pair] for x in c["dropped"])
    kidx = KEY_IDX[pair]
    y = [np.array(expectation(lo, l0[b], l1[b], c["dev_hat"][kidx[b]][:L])["y"], dtype=object) for b in range(2)]
    d0, d1, dk = dev_t(env, l0), dev_t(env, l1), dev_t(env, kidx)
    g0, g1, st = run_switch(env, ctx, d0, d1, dk, L)
    assert (st == 1).all()
    for b in range(2):
        k = kidx[b]
        y2 = np.array(expectation(lo, g0[b], g1[b], s_hat[:L])["y"], dtype=object)
        quo = switch_quotient(o, l1[b], c["wk0"][k], c["wk1"][k], c["errs"][k], s_nat)
        assert ((y2 - y[b]) == quo.astype(object)).all(), b
        print(f"record {b} (key {k}): max |switch term| = {int(np.abs(quo).max())}")
    r0, r1, st = run_switch_sum(env, ctx, d0, d1, dk, [[0, 1]], L)
    assert (st == 1).all()
    e0, e1, info = switch_sum_expect(o, l0, l1, kidx, [[0, 1]], c["wk0"], c["wk1"])
    assert (r0 == e0).all() and (r1 == e1).all()
    quo, t_max = row_quotient(o, info[0], [0, 1], kidx, c["errs"], s_nat)
    y2 = np.array(expectation(lo, r0[0], r1[0], s_hat[:L])["y"], dtype=object)
    assert ((y2 - (y[0] + y[1])) == quo.astype(object)).all()
    print(f"row of two: max |switch term| = {int(np.abs(quo).max())}, max |T| = {t_max}")


def test_switch_sum_end_to_end_at_the_fresh_scale(env, keyed_cases):
    """Test 8 at 4096 x 3: keyed symmetric encrypt under K = 3 device keys -> ct_drop_primes to np - 1 -> ONE
    ct_switch_sum_keyed_sp call with the rows {0 .. 5}, {0, 3}, {4} -> decrypt_level under the target key alone at scale
    Delta: the call equals its definition, the final pte / values / values_f64 equal the oracle's on the final records
    bit for bit, and the slots are within the reference's 0.1 of the sums of the values (on the expectation first;
    tools/ct_switch_noise_sim.py puts the error near 1e-3).  The regression the ring exists for: the same records summed
    by ct_lincomb WITHOUT switching and decrypted under the target key miss 0.1.  The switched sums then go unchanged into
    ct_galois_sp (step 1, the target key's Galois key) and decrypt to the rolled sums within 0.1."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    shape = (4096, 3)
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    L = npr - 1
    lo = Oracle(n, L)
    l0, l1 = c["dropped"]
    d0, d1, dk = dev_t(env, l0), dev_t(env, l1), dev_t(env, KEY_IDX)
    rows = [[0, 1, 2, 3, 4, 5], [0, 3], [4]]
    want = np.stack([c["vals"][r].astype(np.float64).sum(axis=0) for r in rows])
    r0, r1, st = run_switch_sum(env, ctx, d0, d1, dk, rows, L)
    assert (st == 1).all()
    e0, e1, _ = switch_sum_expect(o, l0, l1, KEY_IDX, rows, c["wk0"], c["wk1"])
    assert (r0 == e0).all() and (r1 == e1).all()
    check_level_decrypt(env, ctx, lo, r0, r1, c["s_hat"], L, o.scale, want, "switched sums")
    # the plain sum of records under different keys is under no key at all (ct_lincomb takes the records at np primes,
    # as they were encrypted: dropping a prime changes neither message nor scale)
    rp, idx, _ = csr(rows)
    x0, x1 = guarded_pair(env, n, (len(rows), npr, n), "lincomb", lambda a, b: ctx.ct_lincomb(
        c["fresh"][0], a, c["fresh"][1], b, row_ptr=dev_t(env, rp), idx=dev_t(env, idx)))
    plain = run_decrypt(env, ctx, dev_t(env, x0), dev_t(env, x1))
    torch.cuda.synchronize()
    for g in range(len(rows)):
        err = float(np.abs(plain["values"][g].cpu().numpy().astype(np.float64) - want[g]).max())
        print(f"row {g}: summed without switching: {err:.3e}")
        assert not err < 0.1, (g, err)
    # under one key the sums are ordinary records: a rotation with that key's Galois key
    g0, g1 = run_galois_sp(env, ctx, dev_t(env, r0), dev_t(env, r1), c["elt"], L)
    f0, f1 = galois_sp_expect(o, r0, r1, c["elt"], c["gk0"], c["gk1"])
    assert (g0 == f0).all() and (g1 == f1).all()
    check_level_decrypt(env, ctx, lo, g0, g1, c["s_hat"], L, o.scale, np.roll(want, -1, axis=1), "rolled sums")


# ---- test 9: the example --------------------------------------------------------------------------------------------
def test_fleet_sum_example(env, tmp_path):
    """examples/fleet_sum_roundtrip.c from plain gcc: 16 records under 4 device keys, dropped to np - 1, switched and
    summed in 4 groups that mix keys by one call, decrypted under the aggregator key alone within the reference's 0.1."""
    run_example("fleet_sum_roundtrip", tmp_path, ("4096", "3", "16", "4"))
