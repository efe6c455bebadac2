"""Slot packing (-m gpu): se_amd_ct_pack_sp_device.
Every expectation is the definition in tests/ct_model_pack.py on top of tests/ct_model.py: the oracle's primitives (ntt,
intt, decrypt, fft, expand_ternary) and Python / NumPy integers, never the code under test.  Every comparison is bit-exact
except the reference's own acceptance criterion |values - expected| < 0.1 (device/test/ckks_tests_common.c:132).
Oracle(n, L) is the oracle of a level-L record of Oracle(n, np): the default chains are prefixes of one another."""
import numpy as np
import pytest

from ct_model import (SHAPE_IDS, call_elements, centred, edge_row, inverse_element, key_errors, rand_key, rand_slab,
                      sigma_rows)
from ct_model_pack import csr_entries, pack_expect, pack_row_quotient
from gpu_support import (NULL, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched, assert_zero_prefix,  # noqa: F401
                         check_level_decrypt, dev_t, dptr, drop_records, env, expectation, fresh_records, guarded_pair,
                         hptr, install_galois_keys, keyed_cases, run_example, run_galois_sp, step_elements, stream_of)
from vectors import sigma_coeff

pytestmark = pytest.mark.gpu


# ---- the runners: one call each, two rows of sentinels behind each output, status pre-filled with 77 ------------------
def run_pack(env, ctx, c0, c1, elts, rows, primes, row_ptr=None):
    """One ct_pack_sp call with the CSR form of `rows`, lists of (record, element index) pairs (row_ptr: an override of
    the same length) -> (out0, out1 host [G][primes][n], status host [G])."""
    rp, idx, eidx, nnz = csr_entries(rows)
    rp = rp if row_ptr is None else np.asarray(row_ptr, dtype=np.uint32)
    G = len(rows)
    st = env["torch"].full((G,), 77, dtype=env["torch"].uint8, device=env["dev"])
    d_rp, d_idx, d_eidx = dev_t(env, rp), dev_t(env, idx), dev_t(env, eidx)
    out = guarded_pair(env, ctx.n, (G, primes, ctx.n), "pack", lambda a, b: ctx.ct_pack_sp(
        c0, c1, elts, d_eidx[:nnz], a, b, primes=primes, row_ptr=d_rp, idx=d_idx[:nnz], status=st))
    return out[0], out[1], st.cpu().numpy()


def run_pack_single(env, ctx, c0, c1, elts, eidx, primes):
    """One ct_pack_sp call in the single form: record b under elts[eidx[b]] -> (out0, out1 host [B][primes][n], status)."""
    B = c0.shape[0]
    st = env["torch"].full((B,), 77, dtype=env["torch"].uint8, device=env["dev"])
    d_eidx = dev_t(env, np.asarray(eidx, dtype=np.uint32))
    out = guarded_pair(env, ctx.n, (B, primes, ctx.n), "pack single",
                       lambda a, b: ctx.ct_pack_sp(c0, c1, elts, d_eidx, a, b, primes=primes, status=st))
    return out[0], out[1], st.cpu().numpy()


def run_sum_sp(env, ctx, c0, c1, elts, primes, add_input):
    """One ct_galois_sum_sp call on device slabs [B][primes][n]."""
    return guarded_pair(env, ctx.n, (c0.shape[0], primes, ctx.n), "sum_sp",
                        lambda a, b: ctx.ct_galois_sum_sp(c0, c1, elts, a, b, add_input=add_input, primes=primes))


# ---- the slabs and keys of tests 1 to 3 -----------------------------------------------------------------------------
B6 = 6
SLAB_CASES = [((4096, 3), (2, 1)), ((4096, 2), (1,)), ((8192, 6), (5,)), ((16384, 13), (12,))]
SLAB_IDS = [f"{n}x{npr}" for (n, npr), _ in SLAB_CASES]


@pytest.fixture(scope="module")
def slab_cases(env):
    """slab_cases(shape, levels) -> per shape, computed once: a context without a secret key; the call's elements
    (call_elements plus the identity at n = 4096, else 3 and n + 1); random special-prime Galois keys of the distinct
    elements installed, with the key words 0, 1 and q - 1 on a data column and on column p, and EVERY word of the key of
    n + 1 equal to q_i - 1; per level the slabs (B = 6 at n = 4096, else 2): record 0 of c1 holds the centring edge rows,
    record 1 is all q_j - 1."""
    from oracle.pyoracle import Oracle
    cache = {}

    def get(shape, levels):
        if shape in cache:
            return cache[shape]
        n, npr = shape
        p = npr - 1
        o = Oracle(n, npr)
        ctx = env["pkg"].Context(n, npr)
        q = o.q
        rng = np.random.default_rng(59 * n + npr)
        small = n == 4096
        elts = call_elements(n, npr) + [1] if small else [3, n + 1]
        distinct = [g for k, g in enumerate(elts) if g != 1 and g not in elts[:k]]
        gk0 = np.stack([rand_key(rng, q, n) for _ in distinct])
        gk1 = np.stack([rand_key(rng, q, n) for _ in distinct])
        for k in (gk0[0], gk1[len(distinct) - 1]):
            k[0, 0, :4] = [0, 1, q[0] - 1, q[0] - 1]
            k[0, p, :4] = [0, 1, q[p] - 1, q[p] - 1]
        if small:
            lazy = distinct.index(n + 1)
            gk0[lazy] = gk1[lazy] = (np.array(q, dtype=np.uint32) - 1)[None, :, None]
        ctx.set_galois_keys_sp(distinct, gk0, gk1)
        key_of = {g: (gk0[k], gk1[k]) for k, g in enumerate(distinct)}
        B = B6 if small else 2
        slabs = {}
        for L in levels:
            c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
            for j in range(L):
                c1[0, j] = edge_row(o, j, rng, [3, n + 1], edges="centring")   # 1 negates nothing, 2n - 1 all but index 0
            c0[1] = c1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
            slabs[L] = (c0, c1)
        cache[shape] = dict(o=o, ctx=ctx, elts=elts, keys=[key_of.get(g) for g in elts], slabs=slabs)
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()


# ---- test 1: the definition on arbitrary slabs and key words --------------------------------------------------------
@pytest.mark.parametrize("shape,levels", SLAB_CASES, ids=SLAB_IDS)
def test_pack_arbitrary_slabs_and_keys(env, slab_cases, shape, levels):
    """Test 1: random residues for the slabs and for the installed keys (key words 0, 1 and q_i - 1 on a data column and
    on column p); record 0 of c1 holds 0, 1, (q_j - 1)/2, (q_j + 1)/2 and q_j - 1 among random coefficients, record 1 is
    all q_j - 1.  At n = 4096 three rows that together use every record and every listed element, the identity and the
    repeated element among them; at 8192 x 6 (L = 5) and 16384 x 13 (L = 12) one row of two entries.  Against the
    definition; a lower level uses rows j < L, columns i < L and column p of the same keys; the sentinels survive and the
    status, pre-filled with 77, is 1.  No secret key is installed."""
    case = slab_cases(shape, levels)
    o, ctx, elts, keys = case["o"], case["ctx"], case["elts"], case["keys"]
    E = len(elts)
    if shape[0] == 4096:
        rows = [[(0, 0), (1, 1 % E)], [(2, 2 % E), (3, E - 1), (0, 3 % E)], [(4, 4 % E), (5, 5 % E), (1, 6 % E), (4, E - 1)]]
        assert {b for r in rows for b, _ in r} == set(range(B6)) and elts[E - 1] == 1
        assert {e for r in rows for _, e in r} == set(range(E))
    else:
        rows = [[(0, 0), (1, 1)]]
    for L in levels:
        c0, c1 = case["slabs"][L]
        e0, e1, _ = pack_expect(o, c0, c1, elts, rows, keys)
        g0, g1, st = run_pack(env, ctx, dev_t(env, c0), dev_t(env, c1), elts, rows, L)
        assert (st == 1).all(), st
        assert (g0 == e0).all() and (g1 == e1).all(), L


# ---- test 2: one call of every kind of row --------------------------------------------------------------------------
@pytest.mark.parametrize("shape,levels", SLAB_CASES[:2], ids=SLAB_IDS[:2])
def test_pack_rows_against_the_model(env, slab_cases, shape, levels):
    """Test 2: B = 6 records, one call whose rows are: an empty row; a singleton, whose bytes equal ct_galois_sp on that
    record; one (record, element) entry listed twice; a row mixing three elements and the identity; an identity-only row;
    a row in non-monotone record order; one record under every listed element, whose bytes equal ct_galois_sum_sp with
    the non-identity elements and add_input (fact 2); 17 entries over the all-(q_j - 1) record under the key whose every
    word is q_i - 1 (the lazy range: the largest product on every term)."""
    case = slab_cases(shape, levels)
    o, ctx, elts, keys = case["o"], case["ctx"], case["elts"], case["keys"]
    n = shape[0]
    E, ident, lazy = len(elts), elts.index(1), elts.index(n + 1)
    rot = [e for e in range(E) if elts[e] != 1]
    r = lambda k: rot[k % len(rot)]  # noqa: E731
    rows = [[], [(2, r(0))], [(3, r(2)), (3, r(2))], [(0, r(0)), (4, r(1)), (5, r(2)), (2, ident)],
            [(1, ident), (4, ident), (4, ident)], [(5, r(1)), (0, r(2)), (3, r(0)), (1, r(3))],
            [(4, e) for e in range(E)], [(1, lazy)] * 17]
    assert len({elts[e] for _, e in rows[3]}) == 4
    for L in levels:
        c0, c1 = case["slabs"][L]
        d0, d1 = dev_t(env, c0), dev_t(env, c1)
        e0, e1, _ = pack_expect(o, c0, c1, elts, rows, keys)
        g0, g1, st = run_pack(env, ctx, d0, d1, elts, rows, L)
        assert (st == 1).all(), st
        for g in range(len(rows)):
            assert (g0[g] == e0[g]).all() and (g1[g] == e1[g]).all(), (L, g)
        assert not g0[0].any() and not g1[0].any()
        s0, s1 = run_galois_sp(env, ctx, d0, d1, elts[r(0)], L)
        assert g0[1].tobytes() == s0[2].tobytes() and g1[1].tobytes() == s1[2].tobytes(), L
        h0, h1 = run_sum_sp(env, ctx, d0, d1, [elts[e] for e in rot], L, True)
        assert g0[6].tobytes() == h0[4].tobytes() and g1[6].tobytes() == h1[4].tobytes(), L


# ---- test 3: the single form ----------------------------------------------------------------------------------------
def test_pack_single_form_is_a_rotation_per_record(env, slab_cases):
    """Test 3 at 4096 x 3, L = 2 and 1: B = 6 records under six different element indices, the repeated element's second
    listing among them; record b has the bytes of ct_galois_sp with elts[eidx[b]], and the call equals the definition.
    With the identity on one record that record comes back as it is."""
    case = slab_cases(*SLAB_CASES[0])
    o, ctx, elts, keys = case["o"], case["ctx"], case["elts"], case["keys"]
    eidx = [5, 0, 6, 3, 1, 4]
    assert len(set(eidx)) == B6 and all(elts[e] != 1 for e in eidx) and elts[6] == elts[2]
    for L in SLAB_CASES[0][1]:
        c0, c1 = case["slabs"][L]
        d0, d1 = dev_t(env, c0), dev_t(env, c1)
        g0, g1, st = run_pack_single(env, ctx, d0, d1, elts, eidx, L)
        assert (st == 1).all(), st
        e0, e1, _ = pack_expect(o, c0, c1, elts, [[(b, e)] for b, e in enumerate(eidx)], keys)
        assert (g0 == e0).all() and (g1 == e1).all(), L
        for b, e in enumerate(eidx):
            s0, s1 = run_galois_sp(env, ctx, d0[b:b + 1], d1[b:b + 1], elts[e], L)
            assert g0[b].tobytes() == s0[0].tobytes() and g1[b].tobytes() == s1[0].tobytes(), (L, b)
        with_id = [elts.index(1) if b == 2 else e for b, e in enumerate(eidx)]
        i0, i1, st = run_pack_single(env, ctx, d0, d1, elts, with_id, L)
        assert (st == 1).all() and (i0[2] == c0[2]).all() and (i1[2] == c1[2]).all()
        keep = [b for b in range(B6) if b != 2]
        assert (i0[keep] == g0[keep]).all() and (i1[keep] == g1[keep]).all()


# ---- test 4: the delta boundary across entries ----------------------------------------------------------------------
def test_pack_delta_boundary_across_entries(env):
    """Test 4 at 4096 x 3, L = 1: two keys (elements 3 and n + 1) whose row 0, column p of half 0 is the NTT of the
    constant 1 (all ones), so delta_0 of a row of two entries is centred(sigma_a(D_a) + sigma_b(D_b) mod P); two records
    with sigma_a(D_a) + sigma_b(D_b) = (P - 1)/2, (P + 1)/2, -(P - 1)/2, -(P + 1)/2 and 0 on the first five coefficients
    (reachable: q_0 - 1 >= (P + 1)/2), which the model confirms, with delta_0 = (P - 1)/2, -(P - 1)/2, -(P - 1)/2,
    (P - 1)/2, 0 there.  An implementation that divides per entry rounds each entry's delta on its own and misses."""
    from oracle.pyoracle import Oracle
    n, npr, L, B = 4096, 3, 1, 2
    o = Oracle(n, npr)
    q, p = o.q, npr - 1
    P = q[p]
    assert q[0] - 1 >= (P + 1) // 2
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(97)
    elts = [3, n + 1]
    gk0 = np.stack([rand_key(rng, q, n) for _ in elts])
    gk1 = np.stack([rand_key(rng, q, n) for _ in elts])
    gk0[0, 0, p] = gk0[1, 0, p] = 1
    assert (o.ntt(np.eye(1, n, 0, dtype=np.uint32)[0], p) == 1).all()
    ctx.set_galois_keys_sp(elts, gk0, gk1)
    sums = np.array([(P - 1) // 2, (P + 1) // 2, -(P - 1) // 2, -(P + 1) // 2, 0], dtype=np.int64)
    a = np.array([(q[0] - 1) // 2, (q[0] - 1) // 2, -(q[0] - 1) // 2, -(q[0] - 1) // 2, 5], dtype=np.int64)
    b = sums - a
    assert (np.abs(b) <= (q[0] - 1) // 2).all()
    c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
    for rec, g, vals in ((0, elts[0], a), (1, elts[1], b)):
        image = sigma_coeff(centred(o.intt(c1[rec, 0], 0), q[0]), g)       # sigma_g(D) of the random record
        image[:5] = vals
        c = sigma_coeff(image, inverse_element(n, g))                      # the D whose image that is
        c1[rec, 0] = o.ntt((c % q[0]).astype(np.uint32), 0)
    rows = [[(0, 0), (1, 1)]]
    keys = [(gk0[k], gk1[k]) for k in range(2)]
    e0, e1, info = pack_expect(o, c0, c1, elts, rows, keys)
    assert ((info[0]["D"][0][0] + info[0]["D"][1][0])[:5] == sums).all()
    assert (info[0]["delta"][0][:5] == [(P - 1) // 2, -(P - 1) // 2, -(P - 1) // 2, (P - 1) // 2, 0]).all()
    g0, g1, st = run_pack(env, ctx, dev_t(env, c0), dev_t(env, c1), elts, rows, L)
    assert (st == 1).all() and (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


# ---- test 5: status -------------------------------------------------------------------------------------------------
def test_pack_status(env, slab_cases):
    """Test 5: a row with a record index >= B, an element index >= E, a decreasing or an overlong row_ptr pair gets status
    2 and zero rows in both slabs; every other row its result, an empty row zeros with status 1."""
    case = slab_cases(*SLAB_CASES[0])
    o, ctx, elts, keys = case["o"], case["ctx"], case["elts"], case["keys"]
    L, E = 2, len(elts)
    c0, c1 = case["slabs"][L]
    d0, d1 = dev_t(env, c0), dev_t(env, c1)
    # rows: good | record index >= B | element index >= E | good | empty | the largest words
    rows = [[(0, 0), (2, 7)], [(2, 1), (B6, 0)], [(0, 0), (1, E), (2, 1)], [(2, 3), (2, 3), (0, 4)], [],
            [(0xFFFFFFFF, 0)], [(0, 0xFFFFFFFF)]]
    s0, s1, _ = pack_expect(o, c0, c1, elts, [rows[0], rows[3]], keys)
    g0, g1, st = run_pack(env, ctx, d0, d1, elts, rows, L)
    assert list(st) == [1, 2, 2, 1, 1, 2, 2]
    assert (g0[[0, 3]] == s0).all() and (g1[[0, 3]] == s1).all()
    assert not g0[[1, 2, 4, 5, 6]].any() and not g1[[1, 2, 4, 5, 6]].any()
    # row_ptr pairs: entries [(0, 0), (2, 7) | (2, 3), (0, 4)] with pointers 0, 2, 1, 4, 9 (nnz = 4): good, decreasing,
    # (1, 4) good, overlong
    rows = [[(0, 0), (2, 7)], [], [(2, 3), (0, 4)], []]
    s0, s1, _ = pack_expect(o, c0, c1, elts, [rows[0], [(2, 7), (2, 3), (0, 4)]], keys)
    g0, g1, st = run_pack(env, ctx, d0, d1, elts, rows, L, row_ptr=[0, 2, 1, 4, 9])
    assert list(st) == [1, 2, 1, 2]
    assert (g0[[0, 2]] == s0).all() and (g1[[0, 2]] == s1).all()
    assert not g0[[1, 3]].any() and not g1[[1, 3]].any()


# ---- test 6: arguments ----------------------------------------------------------------------------------------------
def test_pack_arguments(env):
    """Test 6: every argument error returns -22 and writes nothing: NULL ctx, slabs, elts and eidx; exactly one of
    row_ptr / idx NULL; the single form with G != B or nnz != B; E = 0 and 65; an even element and one >= 2n; primes
    outside [1, np - 1] (primes = np among them); B, G, nnz >= 2^32; each misaligned slab; a context of one prime.
    SE_ERR_NO_KEY, with the element named, while only digit Galois keys (and a relinearisation key and a switch ring) are
    installed, and for one listed element without a key.  G = 0 is a successful no-op; a level-1 call writes G . n words
    and nothing behind them."""
    torch, pkg = env["torch"], env["pkg"]
    n, npr, B, G = 4096, 3, 2, 2
    ctx = pkg.Context(n, npr)
    L = ctx.L
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    rp = dev_t(env, np.array([0, 1, 2], dtype=np.uint32))
    ix = dev_t(env, np.array([1, 0], dtype=np.uint32))
    ex = dev_t(env, np.array([0, 1], dtype=np.uint32))
    good = np.array([3, 1], dtype=np.uint32)
    many = np.full(65, 3, dtype=np.uint32)
    even, big = np.array([3, 4], dtype=np.uint32), np.array([2 * n + 1, 3], dtype=np.uint32)
    csr_call = CEntry(L.se_amd_ct_pack_sp_device, ctx=ctx.h, a0=dptr(c0), a1=dptr(c1), nb=B, primes=2, el=hptr(good), ne=2,
                      g=G, r=dptr(rp), i=dptr(ix), e=dptr(ex), nnz=2, o0=dptr(out0), o1=dptr(out1), status=dptr(st),
                      stream=stream_of(env))
    single = dict(r=NULL, i=NULL)                           # the single form: no row_ptr, no idx
    # nothing is installed yet: the refusals come before the keys are looked at
    csr_call.refused([
        dict(ctx=None), dict(a0=NULL), dict(a1=NULL), dict(o0=NULL), dict(o1=NULL), dict(el=NULL),
        dict(e=NULL), dict(single, e=NULL),
        dict(r=NULL), dict(i=NULL),                                        # exactly one of row_ptr / idx
        dict(single, g=1), dict(single, g=3), dict(single, nnz=1), dict(single, nnz=3),
        dict(ne=0), dict(el=hptr(many), ne=65),
        dict(el=hptr(even)), dict(el=hptr(big)),
        dict(primes=0), dict(primes=3), dict(primes=4),
        dict(nb=2 ** 32), dict(g=2 ** 32), dict(nnz=2 ** 32),
        dict(a0=dptr(c0, 4)), dict(a1=dptr(c1, 8)), dict(o0=dptr(out0, 12)), dict(o1=dptr(out1, 4))])
    # a context of one prime has no prime to reserve
    one = pkg.Context(1024, 1)
    csr_call.refused([dict(ctx=one.h, primes=1)])
    one.close()
    # no key of the right family: digit Galois keys, a relinearisation key and a switch ring do not serve
    assert csr_call() == SE_ERR_NO_KEY and "element 3" in L.se_amd_last_error().decode()
    dkey = np.zeros((2, 2 * npr, npr, n), dtype=np.uint32)
    key = np.zeros((2, npr - 1, npr, n), dtype=np.uint32)
    ctx.set_galois_keys([3, 9], dkey, dkey)
    ctx.set_relin_key_sp(key[0], key[0])
    ctx.set_switch_keyring_sp(key, key)
    assert csr_call() == SE_ERR_NO_KEY and csr_call(**single) == SE_ERR_NO_KEY
    ctx.set_galois_keys_sp([9, 5], key, key)
    assert csr_call() == SE_ERR_NO_KEY
    msg = L.se_amd_last_error().decode()
    assert "special-prime" in msg and "element 3" in msg, msg
    assert_untouched(out0, out1)
    assert_untouched(st, fill=77)
    # with the key: the identity alone needs none; G = 0 is a no-op; a level-1 call writes G . n words
    ctx.set_galois_keys_sp([3, 9], key, key)
    assert csr_call(g=0) == 0
    ident, e0 = np.array([1], dtype=np.uint32), torch.zeros_like(ex)
    assert csr_call(el=hptr(ident), ne=1, e=dptr(e0), primes=1) == 0
    torch.cuda.synchronize()
    assert bool((out0.reshape(-1)[G * n:] == SENTINEL).all()) and bool((st == 1).all())
    for form in ({}, single):
        out0.fill_(SENTINEL)
        out1.fill_(SENTINEL)
        st.fill_(77)
        assert csr_call(**form, primes=1) == 0
        for o in (out0, out1):
            assert_zero_prefix(o, G * n)
        assert bool((st == 1).all())
    ctx.close()


# ---- tests 7 and 8: real keys ---------------------------------------------------------------------------------------
WIDTH = 128
RECORDS = {(4096, 3): 16, (8192, 6): 4}


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: m records (16 at 4096 x 3, 4
    at 8192 x 6) with values in [-1, 1] in the slots 0 .. 127 and zero elsewhere, encrypted fresh and dropped to np - 1
    primes by ct_drop_primes; the elements of the steps -128 k, k < m -- se_amd_galois_element rotates LEFT by a positive
    step, so step -128 k moves the slots 0 .. 127 to 128 k .. 128 k + 127 -- with k = 0 the identity; the special-prime
    Galois keys of the m - 1 others, generated on the device and installed, and their errors recovered with the oracle."""
    ctx, o = case["ctx"], case["o"]
    n, npr = ctx.n, ctx.np
    m = RECORDS[(n, npr)]
    elts = step_elements(env, n, [-WIDTH * k for k in range(m)])
    assert elts[0] == 1 and len(set(elts)) == m
    gk0, gk1 = install_galois_keys(case, elts[1:], "pack-gk", sp=True)
    s_rows = np.stack(case["s_hat"][:npr - 1])
    errs = [None] + [key_errors(o, gk0[k], gk1[k], case["s_hat"], sigma_rows(o, s_rows, g)) for k, g in enumerate(elts[1:])]
    vals = np.zeros((m, n // 2), dtype=np.float32)
    vals[:, :WIDTH] = np.random.default_rng(8000 + n).uniform(-1.0, 1.0, (m, WIDTH)).astype(np.float32)
    c0, c1 = fresh_records(env, ctx, vals, 500)
    case.update(elts=elts, keys=[None] + [(gk0[k], gk1[k]) for k in range(m - 1)], errs=errs, vals=vals,
                dropped=drop_records(env, ctx, c0, c1, npr - 1))


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_pack_exact_identity_with_real_keys(env, keyed_cases, shape):
    """Test 7, at L = np - 1 on fresh dropped records, a row of three rotated entries (one record twice, under two
    elements) and an identity entry: the device's output equals the definition, and with y_k the oracle's centred decrypt
    of record k and y' that of the packed row, y' - sum_k sigma_k(y_k) equals pack_row_quotient -- (T - delta_0 - delta_1
    * s) / P with T and the deltas of the ROW, an exact quotient -- as integers.  An implementation that divides per entry
    carries other roundings and misses.  The largest term is printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    o, s_hat, ctx, elts = c["o"], c["s_hat"], c["ctx"], c["elts"]
    n, npr = shape
    L = npr - 1
    lo = Oracle(n, L)
    s_nat = centred(o.expand_ternary(c["sk"], 0), o.q[0])
    l0, l1 = (x[:3] for x in c["dropped"])
    row = [(0, 1), (1, 2), (2, 0), (0, 3)]
    g0, g1, st = run_pack(env, ctx, dev_t(env, l0), dev_t(env, l1), elts, [row], L)
    assert (st == 1).all()
    e0, e1, info = pack_expect(o, l0, l1, elts, [row], c["keys"])
    assert (g0 == e0).all() and (g1 == e1).all()
    quo, t_max = pack_row_quotient(o, info[0], row, c["errs"], s_nat)
    y = [np.array(expectation(lo, l0[b], l1[b], s_hat[:L])["y"], dtype=object) for b in range(3)]
    y2 = np.array(expectation(lo, g0[0], g1[0], s_hat[:L])["y"], dtype=object)
    rotated = sum(sigma_coeff(y[b], elts[e]) for b, e in row)
    assert ((y2 - rotated) == quo.astype(object)).all()
    print(f"{n} x {npr}, row of four: max |pack term| = {int(np.abs(quo).max())}, max |T| = {t_max}")


def test_pack_end_to_end_at_the_fresh_scale(env, keyed_cases):
    """Test 8 at 4096 x 3: 16 records with values in [-1, 1] in the slots 0 .. 127 and zero elsewhere -> ct_drop_primes to
    np - 1 -> ONE ct_pack_sp call with the steps -128 k (fifteen keys and the identity) -> decrypt_level at scale Delta:
    the call equals its definition, the final pte / values / values_f64 equal the oracle's on the packed record bit for
    bit, and every slot is within the reference's 0.1 of the concatenation of the sixteen vectors (on the expectation
    first)."""
    from oracle.pyoracle import Oracle
    shape = (4096, 3)
    c = keyed_cases(shape)
    ctx, o, elts = c["ctx"], c["o"], c["elts"]
    n, npr = shape
    L, m = npr - 1, RECORDS[shape]
    lo = Oracle(n, L)
    l0, l1 = c["dropped"]
    row = [(k, k) for k in range(m)]
    r0, r1, st = run_pack(env, ctx, dev_t(env, l0), dev_t(env, l1), elts, [row], L)
    assert (st == 1).all()
    e0, e1, _ = pack_expect(o, l0, l1, elts, [row], c["keys"])
    assert (r0 == e0).all() and (r1 == e1).all()
    want = c["vals"][:, :WIDTH].astype(np.float64).reshape(1, m * WIDTH)
    assert want.shape[1] == n // 2
    check_level_decrypt(env, ctx, lo, r0, r1, c["s_hat"], L, o.scale, want, "sixteen records packed into one")


# ---- test 9: the example --------------------------------------------------------------------------------------------
def test_slot_pack_example(env, tmp_path):
    """examples/slot_pack_roundtrip.c from plain gcc: 16 records of 128 values, dropped to np - 1, packed into one record
    by one call under fifteen special-prime Galois keys and the identity, decrypted within the reference's 0.1."""
    run_example("slot_pack_roundtrip", tmp_path, ("4096", "3", "16"))
