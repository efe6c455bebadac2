"""Encrypted inner products (-m gpu): se_amd_ct_mul_sum_device and se_amd_ct_dot_sp_device.
Every expectation is the definition in tests/ct_model_dot.py on top of tests/ct_model.py: the oracle's primitives (ntt,
intt, decrypt, fft, expand_ternary) and Python / NumPy integers, never the code under test.  Every comparison is bit-exact
except the reference's own acceptance criterion |values - expected| < 0.1 (device/test/ckks_tests_common.c:132).
Oracle(n, L) is the oracle of a level-L record of Oracle(n, np): the default chains are prefixes of one another, and a
Context(n, L) is the context whose ct_lincomb takes level-L slabs."""
import numpy as np
import pytest

from ct_model import (CASE_IDS, SHAPE_IDS, SP_CASES, centred, edge_row, galois_seeds, key_errors, rand_key, rand_slab,
                      switch_quotient)
from ct_model_dot import csr_pairs, dot_sp_expect, mul_sum_expect, product_sum
from gpu_support import (NULL, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched, assert_zero_prefix,  # noqa: F401
                         check_level_decrypt, dev_t, dptr, drop_records, encrypt_sym, env, expectation, guarded_pair,
                         keyed_cases, rescale_records, run_decrypt, run_example, run_relin_sp, sentinel_out, stream_of,
                         take, unit_values)

pytestmark = pytest.mark.gpu


# ---- the runners of the two entries: one call each, two rows of sentinels behind each output, status pre-filled with 77 ----
def _call_args(env, rows, row_ptr, identity):
    rp, ia, ib, nnz = csr_pairs(rows)
    rp = rp if row_ptr is None else np.asarray(row_ptr, dtype=np.uint32)
    st = env["torch"].full((len(rows),), 77, dtype=env["torch"].uint8, device=env["dev"])
    d_ia, d_ib = (None, None) if identity else (dev_t(env, ia)[:nnz], dev_t(env, ib)[:nnz])
    return dev_t(env, rp), d_ia, d_ib, st


def run_mul_sum(env, ctx, a, b, rows, primes, row_ptr=None, identity=False):
    """One ct_mul_sum call on device slab pairs a = (a0, a1), b = (b0, b1) with the CSR form of `rows` (row_ptr: an
    override of the same length; identity: ia = ib = NULL) -> (T0, T1, T2 host [G][primes][n], status host [G])."""
    d_rp, d_ia, d_ib, st = _call_args(env, rows, row_ptr, identity)
    shape = (len(rows), primes, ctx.n)
    words = int(np.prod(shape))
    outs = [sentinel_out(env, words, 2 * ctx.n) for _ in range(3)]
    ctx.ct_mul_sum(a[0], a[1], b[0], b[1], d_rp, d_ia, d_ib, *outs, primes=primes, status=st)
    env["torch"].cuda.synchronize()
    return tuple(take(t, words, shape, f"mul_sum out{k}") for k, t in enumerate(outs)) + (st.cpu().numpy(),)


def run_dot(env, ctx, a, b, rows, primes, row_ptr=None, identity=False):
    """One ct_dot_sp call, as run_mul_sum -> (out0, out1 host [G][primes][n], status host [G])."""
    d_rp, d_ia, d_ib, st = _call_args(env, rows, row_ptr, identity)
    out = guarded_pair(env, ctx.n, (len(rows), primes, ctx.n), "dot_sp", lambda x, y: ctx.ct_dot_sp(
        a[0], a[1], b[0], b[1], d_rp, d_ia, d_ib, x, y, primes=primes, status=st))
    return out[0], out[1], st.cpu().numpy()


def dot_slabs(o, rng, L, B=4):
    """Two sides of B random records at level L: record 1 of both sides is all q_j - 1; record 0 of a1 is all ones (the
    NTT of the constant 1) and record 0 of b1 holds 0, 1, (q_j -+ 1)/2 and q_j - 1 among random coefficients, so T2 of the
    pair (0, 0) carries them."""
    a0, a1, b0, b1 = (rand_slab(rng, o.q, B, o.n, L) for _ in range(4))
    for s in (a0, a1, b0, b1):
        s[1] = (np.array(o.q[:L], dtype=np.uint32) - 1)[:, None]
    a1[0] = 1
    for j in range(L):
        b1[0, j] = edge_row(o, j, rng, [], edges="centring")
    return a0, a1, b0, b1


# empty | one pair | a pair twice | (0, 0) with two random pairs | 33 entries of the all-(q_j - 1) pair: the smallest row
# that passes every late-reduction boundary (8, 16, 24, 32) with the largest terms | non-monotone order with ia != ib
ROWS = [[], [(2, 3)], [(3, 2), (3, 2)], [(0, 0), (2, 1), (3, 3)], [(1, 1)] * 33, [(3, 0), (0, 2), (2, 0), (1, 3)]]


def dev_sides(env, slabs):
    d = [dev_t(env, s) for s in slabs]
    return (d[0], d[1]), (d[2], d[3])


# ---- test 1: the definition on arbitrary slabs and key words --------------------------------------------------------
@pytest.mark.parametrize("shape,levels,_", SP_CASES, ids=CASE_IDS)
def test_dot_arbitrary_slabs_and_key(env, shape, levels, _):
    """Test 1: random residues and a random key, the constructed records of dot_slabs, the rows ROWS in one call: both
    entries against the model, entry 1 also at primes = np; the sentinels survive.  No secret key is installed."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(59 * n + npr)
    k0, k1 = rand_key(rng, o.q, n), rand_key(rng, o.q, n)
    ctx.set_relin_key_sp(k0, k1)
    for L in tuple(levels) + (npr,):
        slabs = dot_slabs(o, rng, L)
        a, b = dev_sides(env, slabs)
        T = mul_sum_expect(o, *slabs, ROWS)
        g = run_mul_sum(env, ctx, a, b, ROWS, L)
        assert (g[3] == 1).all(), g[3]
        for k in range(3):
            assert (g[k] == T[k]).all(), (L, k)
        if L == npr:
            continue
        e0, e1, _info = dot_sp_expect(o, *slabs, ROWS, k0, k1)
        g0, g1, st = run_dot(env, ctx, a, b, ROWS, L)
        assert (st == 1).all(), st
        for r in range(len(ROWS)):
            assert (g0[r] == e0[r]).all() and (g1[r] == e1[r]).all(), (L, r)
        assert not g0[0].any() and not g1[0].any()
    ctx.close()


# ---- test 2: the twins ----------------------------------------------------------------------------------------------
def test_dot_twins(env):
    """Test 2 at 4096 x 3, L = 2: a row of one pair has the bytes of ct_mul -> ct_relin_sp; every row of ROWS has the
    bytes of ct_mul_sum -> ct_relin_sp and of ct_mul -> ct_lincomb (slabs 0 / 1, then slab 2) -> ct_relin_sp; ct_mul_sum
    has the bytes of ct_mul -> ct_lincomb; identity pairs equal explicit arange lists; squares with a and b the same
    pointers."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, L = 4096, 3, 2
    o = Oracle(n, npr)
    ctx, sums = env["pkg"].Context(n, npr), env["pkg"].Context(n, L)
    assert sums.moduli() == ctx.moduli()[:L]
    rng = np.random.default_rng(61)
    k0, k1 = rand_key(rng, o.q, n), rand_key(rng, o.q, n)
    ctx.set_relin_key_sp(k0, k1)
    slabs = dot_slabs(o, rng, L)
    a, b = dev_sides(env, slabs)
    g0, g1, st = run_dot(env, ctx, a, b, ROWS, L)
    T0, T1, T2, _ = run_mul_sum(env, ctx, a, b, ROWS, L)
    # entry 1, then the relinearisation
    r0, r1 = run_relin_sp(env, ctx, dev_t(env, T0), dev_t(env, T1), dev_t(env, T2), L)
    assert g0.tobytes() == r0.tobytes() and g1.tobytes() == r1.tobytes()
    # the tensor of every pair, the row sums of the slabs, the relinearisation
    rp, ia, ib, nnz = csr_pairs(ROWS)
    P3 = [torch.zeros((nnz, L, n), dtype=torch.int32, device=env["dev"]) for _ in range(3)]
    ctx.ct_mul(a[0], a[1], b[0], b[1], *P3, ia=dev_t(env, ia), ib=dev_t(env, ib), primes=L)
    d_rp, d_all = dev_t(env, rp), dev_t(env, np.arange(nnz, dtype=np.uint32))
    S01 = guarded_pair(env, n, (len(ROWS), L, n), "lincomb 0/1",
                       lambda x, y: sums.ct_lincomb(P3[0], x, P3[1], y, row_ptr=d_rp, idx=d_all))
    S2 = sentinel_out(env, len(ROWS) * L * n, 2 * n)
    sums.ct_lincomb(P3[2], S2, row_ptr=d_rp, idx=d_all)
    torch.cuda.synchronize()
    S2 = take(S2, len(ROWS) * L * n, (len(ROWS), L, n), "lincomb 2")
    assert T0.tobytes() == S01[0].tobytes() and T1.tobytes() == S01[1].tobytes() and T2.tobytes() == S2.tobytes()
    r0, r1 = run_relin_sp(env, ctx, dev_t(env, S01[0]), dev_t(env, S01[1]), dev_t(env, S2), L)
    assert g0.tobytes() == r0.tobytes() and g1.tobytes() == r1.tobytes()
    # a row of one pair: the tensor of that pair relinearised
    one = ROWS.index([(2, 3)])
    k = int(rp[one])
    r0, r1 = run_relin_sp(env, ctx, *(t[k:k + 1] for t in P3), L)
    assert g0[one].tobytes() == r0[0].tobytes() and g1[one].tobytes() == r1[0].tobytes()
    # identity pairs equal explicit lists
    rows = [[(0, 0), (1, 1)], [(2, 2)], [(3, 3)]]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(run_dot(env, ctx, a, b, rows, L, identity=True),
                                                          run_dot(env, ctx, a, b, rows, L)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(run_mul_sum(env, ctx, a, b, rows, L, identity=True),
                                                          run_mul_sum(env, ctx, a, b, rows, L)))
    # squares: a and b the same pointers
    rows = [[(0, 0), (2, 3)], [(1, 1)]]
    sq = (slabs[0], slabs[1], slabs[0], slabs[1])
    e0, e1, _ = dot_sp_expect(o, *sq, rows, k0, k1)
    s0, s1, st = run_dot(env, ctx, a, a, rows, L)
    assert (s0 == e0).all() and (s1 == e1).all() and (st == 1).all()
    T = mul_sum_expect(o, *sq, rows)
    g = run_mul_sum(env, ctx, a, a, rows, L)
    assert all((g[k] == T[k]).all() for k in range(3))
    ctx.close()
    sums.close()


# ---- test 3: edges that only the sum has ----------------------------------------------------------------------------
def test_dot_centring_edges_of_the_summed_row(env):
    """Test 3 at 4096 x 3, L = 1: key row 0, column p of half 0 all ones, so delta_0 = centred(D_0 mod P); a1 all ones on
    both records (the NTT of the constant 1), so T2 of the row {(0, 0), (1, 1)} is b1[0] + b1[1]; the two b1 records hold
    interior coefficients whose sum mod q_0 is (q_0 - 1)/2, (q_0 + 1)/2, (P - 1)/2, (P + 1)/2 and 0 on the first five.
    (In the default chain q_0 < P, so (P -+ 1)/2 lie above q_0 / 2 and centre to negative digits, which are their own
    delta.)  The model confirms D and delta there, then the device is asked.  A kernel that switches per pair, or centres
    before it sums, fails here."""
    from oracle.pyoracle import Oracle
    n, npr, L = 4096, 3, 1
    o = Oracle(n, npr)
    q0, p = o.q[0], npr - 1
    P = o.q[p]
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(67)
    k0, k1 = rand_key(rng, o.q, n), rand_key(rng, o.q, n)
    k0[0, p] = 1
    ctx.set_relin_key_sp(k0, k1)
    a0, a1, b0, b1 = (rand_slab(rng, o.q, 2, n, L) for _ in range(4))
    a1[:] = 1
    assert (o.ntt(np.eye(1, n, 0, dtype=np.uint32)[0], 0) == 1).all()
    sums = np.array([(q0 - 1) // 2, (q0 + 1) // 2, (P - 1) // 2, (P + 1) // 2, 0], dtype=np.int64)
    u = q0 // 3 + np.arange(5, dtype=np.int64)
    v = (sums - u) % q0
    edges = {0, 1, (q0 - 1) // 2, (q0 + 1) // 2, q0 - 1}
    assert not edges & set(u.tolist()) and not edges & set(v.tolist())             # each record is interior
    for rec, vals in ((0, u), (1, v)):
        c = o.intt(b1[rec, 0], 0)
        c[:5] = vals
        b1[rec, 0] = o.ntt(c, 0)
    rows = [[(0, 0), (1, 1)]]
    e0, e1, info = dot_sp_expect(o, a0, a1, b0, b1, rows, k0, k1)
    D = centred(sums.astype(np.uint32), q0)
    assert (info[0]["D"][0][:5] == D).all()
    assert (info[0]["delta"][0][:5] == centred((D % P).astype(np.uint32), P)).all()
    assert D[0] == (q0 - 1) // 2 and D[1] == -(q0 - 1) // 2
    a, b = dev_sides(env, (a0, a1, b0, b1))
    g0, g1, st = run_dot(env, ctx, a, b, rows, L)
    assert (st == 1).all() and (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


# ---- test 4: LOGN 14 and the long prime loop ------------------------------------------------------------------------
def test_dot_row_of_two_at_16384x13(env):
    """Test 4: one row of 2 pairs at 16384 x 13, L = 12, both entries against the model."""
    from oracle.pyoracle import Oracle
    n, npr, L = 16384, 13, 12
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(71 * n + npr)
    k0, k1 = rand_key(rng, o.q, n), rand_key(rng, o.q, n)
    ctx.set_relin_key_sp(k0, k1)
    slabs = tuple(rand_slab(rng, o.q, 2, n, L) for _ in range(4))
    a, b = dev_sides(env, slabs)
    rows = [[(0, 1), (1, 0)]]
    T = mul_sum_expect(o, *slabs, rows)
    g = run_mul_sum(env, ctx, a, b, rows, L)
    assert all((g[k] == T[k]).all() for k in range(3)) and (g[3] == 1).all()
    e0, e1, _ = dot_sp_expect(o, *slabs, rows, k0, k1)
    g0, g1, st = run_dot(env, ctx, a, b, rows, L)
    assert (st == 1).all() and (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


# ---- test 5: status -------------------------------------------------------------------------------------------------
def test_dot_status(env):
    """Test 5 at 4096 x 3, L = 2, Ba = 4, Bb = 3: a row with an ia >= Ba, with an ib >= Bb beside a valid ia, with
    0xFFFFFFFF, a decreasing or an overlong row_ptr pair is all zero in every output slab with status 2; an empty row is
    zero with status 1; every other row equals the model.  Both entries."""
    from oracle.pyoracle import Oracle
    n, npr, L, Ba, Bb = 4096, 3, 2, 4, 3
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(73)
    k0, k1 = rand_key(rng, o.q, n), rand_key(rng, o.q, n)
    ctx.set_relin_key_sp(k0, k1)
    slabs = (rand_slab(rng, o.q, Ba, n, L), rand_slab(rng, o.q, Ba, n, L),
             rand_slab(rng, o.q, Bb, n, L), rand_slab(rng, o.q, Bb, n, L))
    a, b = dev_sides(env, slabs)
    # good | ia >= Ba | ib >= Bb with a valid ia (3 is a record of a, not of b) | 0xFFFFFFFF | good | empty
    rows = [[(0, 2), (3, 1)], [(1, 1), (Ba, 0)], [(0, 0), (3, Bb)], [(0xFFFFFFFF, 0), (1, 0xFFFFFFFF)], [(3, 2)] * 3, []]
    good = [0, 4]
    for rows_, rp, good_, want_st in (
            (rows, None, good, [1, 2, 2, 2, 1, 1]),
            # pointers 0, 2, 1, 4, 9 over nnz = 4 pairs: good, decreasing, (1, 4) good, overlong
            ([[(0, 2), (3, 1)], [], [(2, 0), (1, 1)], []], [0, 2, 1, 4, 9], [0, 2], [1, 2, 1, 2])):
        model_rows = [rows_[g] for g in good_]
        if rp is not None:
            flat = [pr for r in rows_ for pr in r]
            model_rows = [flat[rp[g]:rp[g + 1]] for g in good_]
        T = mul_sum_expect(o, *slabs, model_rows)
        e0, e1, _ = dot_sp_expect(o, *slabs, model_rows, k0, k1)
        bad_ = [g for g in range(len(rows_)) if g not in good_]
        g = run_mul_sum(env, ctx, a, b, rows_, L, row_ptr=rp)
        assert list(g[3]) == want_st
        assert all((g[k][good_] == T[k]).all() and not g[k][bad_].any() for k in range(3))
        g0, g1, st = run_dot(env, ctx, a, b, rows_, L, row_ptr=rp)
        assert list(st) == want_st
        assert (g0[good_] == e0).all() and (g1[good_] == e1).all() and not g0[bad_].any() and not g1[bad_].any()
    ctx.close()


# ---- test 6: arguments and key sets ---------------------------------------------------------------------------------
def test_dot_arguments(env):
    """Test 6: every argument error of both entries returns -22 and writes nothing: NULL ctx, slab or row_ptr; only one of
    ia / ib NULL; both NULL with nnz != Ba or nnz != Bb; primes outside [1, np] resp. [1, np - 1] (primes = np for entry
    2, np + 1 for entry 1); Ba, Bb, G or nnz >= 2^32; a misaligned slab; entry 2 on a context of one prime.  G = 0 is a
    successful no-op; Ba = 0 gives non-empty rows status 2; a level-1 call writes G . n words per slab and nothing behind
    them."""
    torch = env["torch"]
    n, npr, B, G = 4096, 3, 2, 2
    ctx = env["pkg"].Context(n, npr)
    a0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    a1, b0, b1 = (torch.zeros_like(a0) for _ in range(3))
    outs = [torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"]) for _ in range(3)]
    st = torch.full((G,), 77, dtype=torch.uint8, device=env["dev"])
    rp = dev_t(env, np.array([0, 1, 2], dtype=np.uint32))
    ia = dev_t(env, np.array([1, 0], dtype=np.uint32))
    ib = dev_t(env, np.array([0, 1], dtype=np.uint32))
    key = np.zeros((npr - 1, npr, n), dtype=np.uint32)
    ctx.set_relin_key_sp(key, key)
    ins = dict(ctx=ctx.h, a0=dptr(a0), a1=dptr(a1), Ba=B, b0=dptr(b0), b1=dptr(b1), Bb=B, primes=2, G=G, row_ptr=dptr(rp),
               ia=dptr(ia), ib=dptr(ib), nnz=2, o0=dptr(outs[0]), o1=dptr(outs[1]))
    f1 = CEntry(ctx.L.se_amd_ct_mul_sum_device, **ins, o2=dptr(outs[2]), status=dptr(st), stream=stream_of(env))
    f2 = CEntry(ctx.L.se_amd_ct_dot_sp_device, **ins, status=dptr(st), stream=stream_of(env))

    def cases(top, o2_null=(), o2_off=()):
        """The refusals both entries share; entry 1's third output slab in its two places."""
        return [
            dict(ctx=None),                                                        # NULL ctx, slab, row_ptr
            dict(a0=NULL), dict(a1=NULL), dict(b0=NULL), dict(b1=NULL), dict(o0=NULL), dict(o1=NULL), *o2_null,
            dict(row_ptr=NULL),
            dict(ia=NULL), dict(ib=NULL),                                          # only one of ia / ib NULL
            dict(primes=0), dict(primes=top + 1),                                  # primes outside the range
            dict(Ba=2 ** 32), dict(Bb=2 ** 32), dict(G=2 ** 32), dict(nnz=2 ** 32),    # Ba, Bb, G, nnz >= 2^32
            dict(a0=dptr(a0, 4)), dict(a1=dptr(a1, 8)), dict(b0=dptr(b0, 12)), dict(b1=dptr(b1, 4)),   # alignment, each slab
            dict(o0=dptr(outs[0], 8)), dict(o1=dptr(outs[1], 12)), *o2_off,
            dict(ia=NULL, ib=NULL, nnz=3),                                         # both NULL: nnz != Ba or nnz != Bb
            dict(ia=NULL, ib=NULL, Ba=3),
            dict(ia=NULL, ib=NULL, Bb=3),
        ]

    f1.refused(cases(npr, [dict(o2=NULL)], [dict(o2=dptr(outs[2], 4))]))
    f2.refused(cases(npr - 1))
    assert f1(G=0) == 0
    assert f2(G=0) == 0
    # a context of one prime has no prime to reserve; entry 1 serves it
    one = env["pkg"].Context(1024, 1)
    f2.refused([dict(ctx=one.h, primes=1)])
    one.close()
    assert_untouched(*outs)
    assert_untouched(st, fill=77)
    # Ba = 0: the non-empty rows get status 2, zero rows
    for f, n_out in ((f1, 3), (f2, 2)):
        for o in outs:
            o.fill_(SENTINEL)
        st.fill_(77)
        assert f(Ba=0, primes=1) == 0
        torch.cuda.synchronize()
        assert st.tolist() == [2, 2]
        # a level-1 call writes G . n words per slab and nothing behind them
        assert f(primes=1) == 0
        for o in outs[:n_out]:
            assert_zero_prefix(o, G * n)
        assert st.tolist() == [1, 1]
    assert bool((outs[2] == SENTINEL).all())                                       # entry 2 has no third slab
    ctx.close()


def test_dot_key_sets(env):
    """Test 6, key sets: SE_ERR_NO_KEY from entry 2 before set_relin_key_sp, and with only a digit relinearisation key,
    special-prime Galois keys and a switch ring installed; nothing is written; entry 1 works with no key at all."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, L = 4096, 3, 2
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(79)
    slabs = tuple(rand_slab(rng, o.q, 2, n, L) for _ in range(4))
    a, b = dev_sides(env, slabs)
    rows = [[(0, 1), (1, 1)]]
    rp, ia, ib, nnz = csr_pairs(rows)
    d_rp, d_ia, d_ib = dev_t(env, rp), dev_t(env, ia), dev_t(env, ib)
    out0 = torch.full((1, L, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    st = torch.full((1,), 77, dtype=torch.uint8, device=env["dev"])
    dot = CEntry(ctx.L.se_amd_ct_dot_sp_device, ctx=ctx.h, a0=dptr(a[0]), a1=dptr(a[1]), Ba=2, b0=dptr(b[0]),
                 b1=dptr(b[1]), Bb=2, primes=L, G=1, row_ptr=dptr(d_rp), ia=dptr(d_ia), ib=dptr(d_ib), nnz=nnz,
                 out0=dptr(out0), out1=dptr(out1), status=dptr(st), stream=stream_of(env))
    assert dot() == SE_ERR_NO_KEY
    digit = np.zeros((2 * npr, npr, n), dtype=np.uint32)
    ctx.set_relin_key(digit, digit)
    ek = [rand_key(rng, o.q, n) for _ in range(2)]
    ctx.set_galois_keys_sp([3], ek[0][None], ek[1][None])
    ctx.set_switch_keyring_sp(ek[0][None], ek[1][None])
    assert dot() == SE_ERR_NO_KEY
    assert_untouched(out0, out1)
    assert_untouched(st, fill=77)
    T = mul_sum_expect(o, *slabs, rows)
    bare = env["pkg"].Context(n, npr)
    g = run_mul_sum(env, bare, a, b, rows, L)
    assert all((g[k] == T[k]).all() for k in range(3)) and (g[3] == 1).all()
    bare.close()
    ctx.set_relin_key_sp(ek[0], ek[1])
    e0, e1, _ = dot_sp_expect(o, *slabs, rows, ek[0], ek[1])
    g0, g1, s = run_dot(env, ctx, a, b, rows, L)
    assert (g0 == e0).all() and (g1 == e1).all() and (s == 1).all()
    ctx.close()


# ---- tests 7 and 8: real keys -----------------------------------------------------------------------------------------
M = 8                                                        # records per side


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: the special-prime
    relinearisation key, generated on the device and installed, with its errors recovered by the oracle; M + M fresh
    symmetric records with slot values in [-1, 1] (side a: records 0 .. M-1, side b: the rest) with the plaintexts the
    encryptor reported, and the same records dropped to np - 1 primes by ct_drop_primes."""
    ctx, o = case["ctx"], case["o"]
    n, npr = ctx.n, ctx.np
    evk0, evk1 = ctx.gen_relin_key_sp(case["sk"], *galois_seeds(npr, 1, "dot-relin-e2e", sp=True))
    ctx.set_relin_key_sp(evk0, evk1)
    sq = np.stack([((case["s_hat"][j].astype(np.uint64) ** 2) % np.uint64(o.q[j])).astype(np.uint32)
                   for j in range(npr - 1)])
    vals = unit_values(2 * M, n, 7000 + n)
    c0, c1, pte, st = encrypt_sym(env, ctx, vals, first=400)
    assert bool((st == 1).all())
    case.update(evk0=evk0, evk1=evk1, errs=key_errors(o, evk0, evk1, case["s_hat"], sq), vals=vals,
                pte=pte.cpu().numpy(), dropped=drop_records(env, ctx, c0, c1, npr - 1))


def sides_of(env, dropped):
    l0, l1 = dropped
    host = (l0[:M], l1[:M], l0[M:], l1[M:])
    return host, dev_sides(env, host)


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_dot_exact_identity_with_real_keys(env, keyed_cases, shape):
    """Test 7, at L = np - 1 on fresh dropped records: with y_a, y_b the oracle's centred decrypts, the centred decrypt of
    a row of two pairs minus sum negacyclic(y_a, y_b) equals switch_quotient's exact quotient for d = T2 of the row, as
    integers (the largest term is printed); decrypt3_level of entry 1's output reports the pte sum
    negacyclic(pte_a, pte_b) of what the encryptor reported."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    o, s_hat, ctx = c["o"], c["s_hat"], c["ctx"]
    n, npr = shape
    L = npr - 1
    lo = Oracle(n, L)
    s_nat = centred(o.expand_ternary(c["sk"], 0), o.q[0])
    host, (a, b) = sides_of(env, c["dropped"])
    row = [(0, 1), (2, 0)]
    ya = {k: expectation(lo, host[0][k], host[1][k], s_hat[:L])["y"] for k in (0, 2)}
    yb = {k: expectation(lo, host[2][k], host[3][k], s_hat[:L])["y"] for k in (0, 1)}
    g0, g1, st = run_dot(env, ctx, a, b, [row], L)
    assert (st == 1).all()
    T2 = mul_sum_expect(o, *host, [row])[2][0]
    quo = switch_quotient(o, T2, c["evk0"], c["evk1"], c["errs"], s_nat)
    y2 = np.array(expectation(lo, g0[0], g1[0], s_hat[:L])["y"], dtype=object)
    assert ((y2 - product_sum(o, ya, yb, row)) == quo.astype(object)).all()
    print(f"{n} x {npr}: row of two pairs: max |key-switch term| = {int(np.abs(quo).max())}, "
          f"log2 max |product sum| = {np.log2(float(max(abs(int(v)) for v in y2))):.2f}")
    t0, t1, t2, st = run_mul_sum(env, ctx, a, b, [row], L)
    got = run_decrypt(env, ctx, dev_t(env, t0), dev_t(env, t1), L, o.scale * o.scale, c2=dev_t(env, t2))
    pte = c["pte"]
    want = product_sum(o, {k: pte[k] for k in (0, 2)}, {k: pte[M + k] for k in (0, 1)}, row)
    assert int(got["status"][0]) == 1
    assert (got["pte"][0].cpu().numpy().astype(object) == want).all()


def test_dot_end_to_end_at_the_fresh_scale(env, keyed_cases):
    """Test 8 at 4096 x 3: 8 + 8 fresh records with slots in [-1, 1] -> ct_drop_primes -> ONE ct_dot_sp with the rows
    {0 .. 7}, {0, 3}, {4} -> ct_rescale -> decrypt_level at Delta^2 / q_1: the call equals its definition, the decrypt
    outputs equal the oracle's bit for bit and the slots are within the reference's 0.1 of the float64 inner products
    (on the expectation first).  The eager path on the same rows (ct_mul, ct_relin_sp per pair, ct_lincomb) also passes
    0.1, and its bytes differ from the one-call result on the row of 8: one rounding instead of m."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    shape = (4096, 3)
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    L = npr - 1
    l1 = Oracle(n, L - 1)
    host, (a, b) = sides_of(env, c["dropped"])
    members = [list(range(M)), [0, 3], [4]]
    rows = [[(k, k) for k in r] for r in members]
    prod = c["vals"][:M].astype(np.float64) * c["vals"][M:].astype(np.float64)
    want = np.stack([prod[r].sum(axis=0) for r in members])
    scale = o.scale * o.scale / o.q[L - 1]
    g0, g1, st = run_dot(env, ctx, a, b, rows, L)
    assert (st == 1).all()
    e0, e1, _ = dot_sp_expect(o, *host, rows, c["evk0"], c["evk1"])
    assert (g0 == e0).all() and (g1 == e1).all()
    f0, f1 = rescale_records(env, ctx, o, g0, g1, L)
    check_level_decrypt(env, ctx, l1, f0, f1, c["s_hat"], L - 1, scale, want, "inner products")
    # the eager path: the tensor of every pair, every product relinearised, then the row sums
    P3 = [torch.zeros((M, L, n), dtype=torch.int32, device=env["dev"]) for _ in range(3)]
    ctx.ct_mul(a[0], a[1], b[0], b[1], *P3, primes=L)
    r0, r1 = run_relin_sp(env, ctx, *P3, L)
    sums = env["pkg"].Context(n, L)
    rp, idx, _, _ = csr_pairs(rows)
    x0, x1 = guarded_pair(env, n, (len(rows), L, n), "lincomb", lambda x, y: sums.ct_lincomb(
        dev_t(env, r0), x, dev_t(env, r1), y, row_ptr=dev_t(env, rp), idx=dev_t(env, idx)))
    sums.close()
    assert x0[0].tobytes() != g0[0].tobytes() and x1[0].tobytes() != g1[0].tobytes()
    assert x0[2].tobytes() == g0[2].tobytes() and x1[2].tobytes() == g1[2].tobytes()   # a row of one pair: the same bits
    h0, h1 = rescale_records(env, ctx, o, x0, x1, L, "eager rescale")
    check_level_decrypt(env, ctx, l1, h0, h1, c["s_hat"], L - 1, scale, want, "eager inner products")


# ---- test 9: the example --------------------------------------------------------------------------------------------
def test_dot_product_example(env, tmp_path):
    """examples/dot_product_roundtrip.c from plain gcc: two batches of 16 records under one key, dropped to np - 1, ONE
    ct_dot_sp call whose rows are 4 groups, one rescale, decrypted at Delta^2 / q_{np-2} within the reference's 0.1."""
    run_example("dot_product_roundtrip", tmp_path, ("4096", "3", "16", "4"))
