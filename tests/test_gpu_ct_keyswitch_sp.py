"""Special-prime key switch (-m gpu): se_amd_gen/set_relin_key_sp, se_amd_gen/set_galois_keys_sp, se_amd_ct_relin_sp_device,
se_amd_ct_galois_sp_device and se_amd_ct_drop_primes_device.
Every expectation is the definition in tests/ct_model.py: the oracle's primitives (ntt, intt, decrypt, fft,
expand_ternary) and Python / NumPy integers, never the code under test.  The automorphism of an expectation is its
coefficient-domain definition pushed through o.intt and o.ntt.  Every comparison is bit-exact except the reference's own
acceptance criterion |values - expected| < 0.1 (device/test/ckks_tests_common.c:132).
Oracle(n, L) is the oracle of a level-L record of Oracle(n, np): the default chains are prefixes of one another."""
import numpy as np
import pytest

import vectors as V
from ct_model import (CASE_IDS, SHAPE_IDS, SP_CASES, centred, edge_row, galois_seeds, galois_sp_expect, key_errors,
                      key_switch_sp, rand_key, rand_slab, relin_sp_expect, sigma_rows, sigma_slab, sp_diagonal,
                      src_table, switch_quotient)
from gpu_support import (NULL, SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched,  # noqa: F401
                         assert_zero_prefix, check_level_decrypt, dev_t, dptr, drop_records, env, expectation,
                         fresh_records, hptr, install_galois_keys, keyed_cases, ntt_secret, rescale_records,
                         run_decrypt, run_example, run_galois, run_galois_sp, run_relin, run_relin_sp, sentinel_out,
                         step_elements, stream_of, take, unit_values)
from vectors import sigma_coeff

pytestmark = pytest.mark.gpu


# ---- test 1: the definition on arbitrary slabs and key words --------------------------------------------------------
@pytest.mark.parametrize("shape,levels,B", SP_CASES, ids=CASE_IDS)
def test_sp_arbitrary_slabs_and_key(env, shape, levels, B):
    """Test 1: random residues for the slabs and for the installed keys (the Galois keys of 3 and n + 1, a
    relinearisation key; key words 0, 1 and q_i - 1 on a data column and on the special prime's); record 0 of the
    switched slab holds 0, 1, (q_j - 1)/2, (q_j + 1)/2 and q_j - 1 on negated and on kept positions, record 1 is all
    q_j - 1; both entries against the definition, d0 and d1 of the relinearisation random.  A lower level uses rows
    j < L, columns i < L and column p of the same keys; the sentinels survive.  No secret key is installed."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    p = npr - 1
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    q = o.q
    rng = np.random.default_rng(41 * n + npr)
    elts = [3, n + 1]
    gk0 = np.stack([rand_key(rng, q, n) for _ in elts])
    gk1 = np.stack([rand_key(rng, q, n) for _ in elts])
    evk0, evk1 = rand_key(rng, q, n), rand_key(rng, q, n)
    for k in (gk0[0], gk1[1], evk0):
        k[0, 0, :4] = [0, 1, q[0] - 1, q[0] - 1]
        k[0, p, :4] = [0, 1, q[p] - 1, q[p] - 1]
    ctx.set_galois_keys_sp(elts, gk0, gk1)
    ctx.set_relin_key_sp(evk0, evk1)
    for L in levels:
        c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
        for j in range(L):
            c1[0, j] = edge_row(o, j, rng, elts, edges="centring")
        c0[1] = c1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
        d0, d1 = dev_t(env, c0), dev_t(env, c1)
        for k, g in enumerate(elts):
            e0, e1 = galois_sp_expect(o, c0, c1, g, gk0[k], gk1[k])
            g0, g1 = run_galois_sp(env, ctx, d0, d1, g, L)
            assert (g0 == e0).all() and (g1 == e1).all(), (L, g)
        a0, a1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
        e0, e1 = relin_sp_expect(o, a0, a1, c1, evk0, evk1)
        r0, r1 = run_relin_sp(env, ctx, dev_t(env, a0), dev_t(env, a1), d1, L)
        assert (r0 == e0).all() and (r1 == e1).all(), L
    ctx.close()


def test_sp_delta_boundary(env):
    """Test 1, the delta boundary at 4096 x 3, L = 2: the key has column p of rows 0 and 1 of half 0 equal to the NTT of
    the constant 1 (all ones), so delta_0 = centred(D_0 + D_1 mod P); the switched polynomial has D_0 + D_1 =
    (P - 1)/2, (P + 1)/2, -(P - 1)/2, -(P + 1)/2 and 0 on its first five coefficients (reachable: q_0 + q_1 > P > q_1),
    which the oracle confirms, with delta_0 = (P - 1)/2, -(P - 1)/2, -(P - 1)/2, (P - 1)/2, 0 there.  Both entries."""
    from oracle.pyoracle import Oracle
    n, npr, L, B = 4096, 3, 2, 2
    o = Oracle(n, npr)
    q, p = o.q, npr - 1
    P = q[p]
    assert q[0] + q[1] > P > q[1]
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(77)
    g = 3
    k0, k1 = rand_key(rng, q, n), rand_key(rng, q, n)
    k0[0, p] = k0[1, p] = 1
    assert (o.ntt(np.eye(1, n, 0, dtype=np.uint32)[0], p) == 1).all()
    ctx.set_galois_keys_sp([g], k0[None], k1[None])
    ctx.set_relin_key_sp(k0, k1)
    sums = np.array([(P - 1) // 2, (P + 1) // 2, -(P - 1) // 2, -(P + 1) // 2, 0], dtype=np.int64)
    a = np.array([(q[0] - 1) // 2, (q[0] - 1) // 2, -(q[0] - 1) // 2, -(q[0] - 1) // 2, 5], dtype=np.int64)
    b = sums - a
    assert (np.abs(b) <= (q[1] - 1) // 2).all()
    d = rand_slab(rng, q, B, n, L)
    for j, vals in ((0, a), (1, b)):
        c = o.intt(d[0, j], j)
        c[:5] = vals % q[j]
        d[0, j] = o.ntt(c, j)
    r = key_switch_sp(o, d[0], k0, k1)
    assert ((r["D"][0] + r["D"][1])[:5] == sums).all()
    assert (r["delta"][0][:5] == [(P - 1) // 2, -(P - 1) // 2, -(P - 1) // 2, (P - 1) // 2, 0]).all()
    a0, a1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
    e0, e1 = relin_sp_expect(o, a0, a1, d, k0, k1)
    r0, r1 = run_relin_sp(env, ctx, dev_t(env, a0), dev_t(env, a1), dev_t(env, d), L)
    assert (r0 == e0).all() and (r1 == e1).all()
    # the rotation switches sigma(c1): c1 = sigma^-1 of the constructed polynomial
    c1 = sigma_slab(o, d, pow(g, -1, 2 * n))
    assert (sigma_slab(o, c1, g) == d).all()
    e0, e1 = galois_sp_expect(o, a0, c1, g, k0, k1)
    g0, g1 = run_galois_sp(env, ctx, dev_t(env, a0), dev_t(env, c1), g, L)
    assert (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


# ---- test 2: the relinearisation twin -------------------------------------------------------------------------------
def test_galois_sp_is_relin_sp_of_the_permuted_record(env):
    """Test 2: at 4096 x 3, L = 2 the outputs have the bytes of ct_relin_sp(sigma(c0), 0, sigma(c1)) with the element's
    key words installed as the relinearisation key; sigma is an index_select along the row."""
    torch = env["torch"]
    n, npr, L, B = 4096, 3, 2, 3
    ctx = env["pkg"].Context(n, npr)
    q = ctx.moduli()
    rng = np.random.default_rng(4096 * 3 + 5)
    elts = [pow(3, 7, 2 * n), 2 * n - 1]
    gk0 = np.stack([rand_key(rng, q, n) for _ in elts])
    gk1 = np.stack([rand_key(rng, q, n) for _ in elts])
    ctx.set_galois_keys_sp(elts, gk0, gk1)
    c0, c1 = dev_t(env, rand_slab(rng, q, B, n, L)), dev_t(env, rand_slab(rng, q, B, n, L))
    for k, g in enumerate(elts):
        src = dev_t(env, src_table(n, g))
        p0, p1 = c0.index_select(2, src).contiguous(), c1.index_select(2, src).contiguous()
        ctx.set_relin_key_sp(gk0[k], gk1[k])
        r0, r1 = run_relin_sp(env, ctx, p0, torch.zeros_like(p1), p1, L)
        g0, g1 = run_galois_sp(env, ctx, c0, c1, g, L)
        assert (g0 == r0).all() and (g1 == r1).all(), g
    ctx.close()


# ---- test 3: key generation, installs and their refusals ------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_sp_key_generation(env, shape):
    """Test 3: gen_relin_key_sp and gen_galois_keys_sp for {3, 3^-1, 2n - 1} equal gen_keys_batch(K = np - 1, this key
    replicated, the block of seeds) plus (P mod q_j) . target on column j of row j; exactly those columns differ and
    column p has no diagonal; nothing installed is touched.  The calls without a key, or for an element that is not
    installed, are SE_ERR_NO_KEY; the installs and generators refuse what the digit twins refuse and the previous set
    still works.  Installing special-prime keys leaves the digit keys' results unchanged, and the other way round."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    pkg = env["pkg"]
    n, npr = shape
    R, p, L = npr - 1, npr - 1, npr - 1
    o = Oracle(n, npr)
    ctx = pkg.Context(n, npr)
    sk = V.secret_key(n, seed=3)
    s_hat = np.stack(ntt_secret(o, sk))
    elts = [3, pow(3, -1, 2 * n), 2 * n - 1]
    G = len(elts)
    # relinearisation key
    ra, re_ = galois_seeds(npr, 1, "sp-relin-keygen", sp=True)
    evk0, evk1 = ctx.gen_relin_key_sp(sk, ra, re_)
    assert evk0.shape == (R, npr, n)
    _, pk0, pk1 = ctx.gen_keys_batch(ra, re_, sk_in=np.tile(sk, (R, 1)))
    s2 = np.stack([((s_hat[j].astype(np.uint64) ** 2) % np.uint64(o.q[j])).astype(np.uint32) for j in range(R)])
    exp0 = pk0.copy()
    for j in range(R):
        exp0[j, j] = (pk0[j, j].astype(np.uint64) + sp_diagonal(o, s2, j)) % np.uint64(o.q[j])
    assert (evk1 == pk1).all() and (evk0 == exp0).all()
    assert (evk0 != pk0).any(axis=2).sum() == R and (evk0[:, p] == pk0[:, p]).all()
    # Galois keys
    sa, se = galois_seeds(npr, G, "sp-gk-keygen", sp=True)
    gk0, gk1 = ctx.gen_galois_keys_sp(sk, elts, sa, se)
    assert gk0.shape == (G, R, npr, n)
    sa, se = np.asarray(sa).reshape(G, R, 64), np.asarray(se).reshape(G, R, 64)
    for k, g in enumerate(elts):
        _, pk0, pk1 = ctx.gen_keys_batch(sa[k], se[k], sk_in=np.tile(sk, (R, 1)))
        target = sigma_rows(o, s_hat[:R], g)
        exp0 = pk0.copy()
        for j in range(R):
            exp0[j, j] = (pk0[j, j].astype(np.uint64) + sp_diagonal(o, target, j)) % np.uint64(o.q[j])
        assert (gk1[k] == pk1).all(), g
        assert (gk0[k] == exp0).all(), g
        assert (gk0[k] != pk0).any(axis=2).sum() == R and (gk0[k][:, p] == pk0[:, p]).all(), g
    # the generators installed nothing: no secret key, no special-prime key
    B = 2
    slab = torch.zeros((B, L, n), dtype=torch.int32, device=env["dev"])
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    assert ctx.L.se_amd_decrypt_level_device(ctx.h, dptr(slab), dptr(slab), B, L, ctx.scale(), NULL, NULL, NULL,
                                             dptr(st), stream_of(env)) == SE_ERR_NO_KEY
    out0, out1 = torch.full_like(slab, SENTINEL), torch.full_like(slab, SENTINEL)
    gal = CEntry(ctx.L.se_amd_ct_galois_sp_device, ctx=ctx.h, c0=dptr(slab), c1=dptr(slab), B=B, primes=L, elt=3,
                 out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    rel = CEntry(ctx.L.se_amd_ct_relin_sp_device, ctx=ctx.h, d0=dptr(slab), d1=dptr(slab), d2=dptr(slab), B=B, primes=L,
                 out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    assert gal(elt=3) == SE_ERR_NO_KEY and rel() == SE_ERR_NO_KEY
    # a refused first install installs nothing
    bad0 = gk0.copy()
    bad0[0, 0, 0, 0] = o.q[0]
    with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
        ctx.set_galois_keys_sp(elts, bad0, gk1)
    assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    bad1 = evk1.copy()
    bad1[R - 1, p, n - 1] = o.q[p]
    with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
        ctx.set_relin_key_sp(evk0, bad1)
    assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    assert gal(elt=3) == SE_ERR_NO_KEY and rel() == SE_ERR_NO_KEY
    assert_untouched(out0, out1)
    assert_untouched(st, fill=77)
    # the first two elements are installed: the third is not there
    ctx.set_galois_keys_sp(elts[:2], gk0[:2], gk1[:2])
    ctx.set_relin_key_sp(evk0, evk1)
    assert gal(elt=elts[2]) == SE_ERR_NO_KEY and gal(elt=5) == SE_ERR_NO_KEY
    rng = np.random.default_rng(n + npr)
    c0, c1, c2 = (rand_slab(rng, o.q, B, n, L) for _ in range(3))
    d0, d1, d2 = dev_t(env, c0), dev_t(env, c1), dev_t(env, c2)
    want_g = galois_sp_expect(o, c0[:1], c1[:1], elts[1], gk0[1], gk1[1])
    want_r = relin_sp_expect(o, c0[:1], c1[:1], c2[:1], evk0, evk1)

    def previous_set_works():
        g0, g1 = run_galois_sp(env, ctx, d0, d1, elts[1], L)
        assert (g0[:1] == want_g[0]).all() and (g1[:1] == want_g[1]).all()
        r0, r1 = run_relin_sp(env, ctx, d0, d1, d2, L)
        assert (r0[:1] == want_r[0]).all() and (r1[:1] == want_r[1]).all()
        assert gal(elt=elts[2]) == SE_ERR_NO_KEY
        return g0, g1, r0, r1

    sp_before = previous_set_works()
    refused = []
    for which, (k, r, i, c) in ((0, (0, 0, 0, 0)), (1, (G - 1, R - 1, npr - 1, n - 1))):
        k0, k1 = gk0.copy(), gk1.copy()
        (k0, k1)[which][k, r, i, c] = o.q[i]
        refused.append((elts, k0, k1))                                   # a word == q_i
    refused.append(([3, elts[1], 3], gk0, gk1))                          # a duplicate element
    refused.append(([3, 4, elts[2]], gk0, gk1))                          # an even element
    refused.append(([3, 2 * n + 1, elts[2]], gk0, gk1))                  # an element >= 2n
    for el, k0, k1 in refused:
        with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
            ctx.set_galois_keys_sp(el, k0, k1)
        assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value), el
    with pytest.raises(pkg.SealEmbeddedAmdError):
        ctx.set_relin_key_sp(bad1, evk1)
    previous_set_works()
    # the digit keys and the special-prime keys are installed sets of their own
    dk = [np.stack([rand_slab(rng, o.q, 1, n)[0] for _ in range(2 * npr)])[None] for _ in range(4)]
    dig = lambda: (run_galois(env, ctx, d0, d1, elts[1], L), run_relin(env, ctx, d0, d1, d2, L))
    ctx.set_galois_keys([elts[1]], dk[0], dk[1])
    ctx.set_relin_key(dk[2][0], dk[3][0])
    digit_before = dig()
    sp_now = previous_set_works()                              # installing digit keys changed no special-prime result
    assert all((a == b).all() for a, b in zip(sp_before, sp_now))
    ctx.set_galois_keys_sp(elts[:2], gk0[:2], gk1[:2])
    ctx.set_relin_key_sp(evk0, evk1)
    digit_now = dig()                                          # and the other way round
    assert all((a == b).all() for x, y in zip(digit_before, digit_now) for a, b in zip(x, y))
    # a new install replaces the whole set
    ctx.set_galois_keys_sp(elts[2:], gk0[2:], gk1[2:])
    assert gal(elt=elts[1]) == SE_ERR_NO_KEY and gal(elt=elts[2]) == 0
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(out0)) == 0 and int(torch.count_nonzero(out1)) == 0    # zero slabs rotate to zero
    # the generators' own refusals
    bad_sk = sk.copy()
    bad_sk[5] |= 0x03
    for args in ((bad_sk, elts), (sk, [3, 6, 5]), (sk, [3, 2 * n + 1, 5])):
        with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
            ctx.gen_galois_keys_sp(args[0], args[1], sa, se)
        assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
        ctx.gen_relin_key_sp(bad_sk, ra, re_)
    assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    el = np.array(elts, dtype=np.uint32)
    gen = CEntry(ctx.L.se_amd_gen_galois_keys_sp, ctx=ctx.h, sk=hptr(sk), elts=hptr(el), G=G, seeds_a=hptr(sa),
                 seeds_e=hptr(se), gk0=hptr(gk0), gk1=hptr(gk1))
    install = CEntry(ctx.L.se_amd_set_galois_keys_sp, ctx=ctx.h, elts=hptr(el), G=G, gk0=hptr(gk0), gk1=hptr(gk1))
    for Gbad in (0, 65):
        gen.refused([dict(G=Gbad)])
        install.refused([dict(G=Gbad)])
    assert ctx.L.se_amd_set_relin_key_sp(ctx.h, NULL, hptr(evk1)) == SE_ERR_INVALD_ARGUMENT
    assert ctx.L.se_amd_gen_relin_key_sp(ctx.h, hptr(sk), NULL, hptr(re_), hptr(evk0),
                                         hptr(evk1)) == SE_ERR_INVALD_ARGUMENT
    assert gal(elt=elts[2]) == 0
    ctx.close()


# ---- test 4: arguments ----------------------------------------------------------------------------------------------
def test_sp_arguments(env):
    """Every argument error returns -22 and writes nothing: the digit twins' (NULL, alignment, B >= 2^32, the element),
    primes outside [1, np - 1] (primes = np among them), and every entry on a context of one prime.  SE_ERR_NO_KEY for an
    element without a key, and for both entries when only digit keys are installed.  B = 0 is a successful no-op; a
    level-1 call writes B . n words and nothing behind them."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 2
    ctx = env["pkg"].Context(n, npr)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1, c2 = torch.zeros_like(c0), torch.zeros_like(c0)
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    L, s = ctx.L, stream_of(env)
    fg = CEntry(L.se_amd_ct_galois_sp_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, primes=2, elt=3, out0=dptr(out0),
                out1=dptr(out1), stream=s)
    fr = CEntry(L.se_amd_ct_relin_sp_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), c2=dptr(c2), B=B, primes=2,
                out0=dptr(out0), out1=dptr(out1), stream=s)
    # only digit keys installed: they do not serve these entries
    dkey = np.zeros((1, 2 * npr, npr, n), dtype=np.uint32)
    ctx.set_galois_keys([3], dkey, dkey)
    ctx.set_relin_key(dkey[0], dkey[0])
    assert fg() == SE_ERR_NO_KEY
    assert fr() == SE_ERR_NO_KEY
    key = np.zeros((1, npr - 1, npr, n), dtype=np.uint32)
    ctx.set_galois_keys_sp([3], key, key)
    ctx.set_relin_key_sp(key[0], key[0])
    fg.refused([
        dict(ctx=None),
        dict(c0=NULL),                                                 # NULL mandatory pointers
        dict(c1=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(primes=0),                                                # primes outside [1, np - 1]
        dict(primes=3),                                                # primes = np: the special prime is not data
        dict(primes=4),
        dict(B=2 ** 32),                                               # B >= 2^32
        dict(c0=dptr(c0, 4)),                                          # alignment, each slab
        dict(c1=dptr(c1, 8)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
        dict(elt=0),                                                   # an even element, one >= 2n
        dict(elt=4),
        dict(elt=2 * n),
        dict(elt=2 * n + 3),
    ])
    fr.refused([
        dict(ctx=None),
        dict(c0=NULL),
        dict(c1=NULL),
        dict(c2=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(primes=0),
        dict(primes=3),                                                # primes = np
        dict(B=2 ** 32),
        dict(c0=dptr(c0, 4)),
        dict(c1=dptr(c1, 8)),
        dict(c2=dptr(c2, 4)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
    ])
    assert fg(elt=5) == SE_ERR_NO_KEY
    assert fg(B=0) == 0
    assert fr(B=0) == 0
    # a context of one prime has no prime to reserve
    one = env["pkg"].Context(1024, 1)
    k1 = np.zeros((1, 1, 1, 1024), dtype=np.uint32)
    sd = np.zeros((1, 64), dtype=np.uint8)
    sk = V.secret_key(1024, seed=3)
    el = np.array([3], dtype=np.uint32)
    fg.refused([dict(ctx=one.h, primes=1)])
    fr.refused([dict(ctx=one.h, primes=1)])
    assert L.se_amd_set_relin_key_sp(one.h, hptr(k1), hptr(k1)) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_set_galois_keys_sp(one.h, hptr(el), 1, hptr(k1), hptr(k1)) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_gen_relin_key_sp(one.h, hptr(sk), hptr(sd), hptr(sd), hptr(k1), hptr(k1)) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_gen_galois_keys_sp(one.h, hptr(sk), hptr(el), 1, hptr(sd), hptr(sd), hptr(k1),
                                       hptr(k1)) == SE_ERR_INVALD_ARGUMENT
    assert not k1.any()
    one.close()
    assert_untouched(out0, out1)
    for f in (fg, fr):
        out0.fill_(SENTINEL)
        out1.fill_(SENTINEL)
        assert f(primes=1) == 0
        for o in (out0, out1):
            assert_zero_prefix(o, B * n)
    ctx.close()


def test_drop_primes(env):
    """ct_drop_primes equals slicing for every (primes_in, primes_out) of a 4096 x 3 context, primes_out = primes_in
    among them, in the two-slab and the one-slab form, and writes nothing behind its output; its argument errors
    return -22 and write nothing; B = 0 is a no-op.  It needs no key."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 3
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(5)
    full = [rng.integers(0, 2 ** 32, (B, npr, n), dtype=np.uint32) for _ in range(2)]
    for pin in (3, 2, 1):
        a, b = full[0][:, :pin].copy(), full[1][:, :pin].copy()
        da, db = dev_t(env, a), dev_t(env, b)
        for pout in range(1, pin + 1):
            words = B * pout * n
            o0, o1 = sentinel_out(env, words, 2 * n), sentinel_out(env, words, 2 * n)
            ctx.ct_drop_primes(da, o0, db, o1, primes_in=pin, primes_out=pout)
            torch.cuda.synchronize()
            assert (take(o0, words, (B, pout, n), "drop out0") == a[:, :pout]).all(), (pin, pout)
            assert (take(o1, words, (B, pout, n), "drop out1") == b[:, :pout]).all(), (pin, pout)
            o0 = sentinel_out(env, words, 2 * n)
            ctx.ct_drop_primes(db, o0, primes_in=pin, primes_out=pout)          # one slab
            torch.cuda.synchronize()
            assert (take(o0, words, (B, pout, n), "drop one slab") == b[:, :pout]).all(), (pin, pout)
    da, db = dev_t(env, full[0]), dev_t(env, full[1])
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    f = CEntry(ctx.L.se_amd_ct_drop_primes_device, ctx=ctx.h, in0=dptr(da), in1=dptr(db), B=B, primes_in=3, primes_out=2,
               out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    f.refused([
        dict(ctx=None),
        dict(in0=NULL),
        dict(out0=NULL),
        dict(out1=NULL),                                               # one of in1 / out1 alone
        dict(in1=NULL),
        dict(primes_out=0),                                            # 1 <= primes_out <= primes_in <= np
        dict(primes_in=2, primes_out=3),
        dict(primes_in=4),
        dict(B=2 ** 32),
        dict(in0=dptr(da, 4)),                                         # alignment
        dict(in1=dptr(db, 8)),
        dict(out0=dptr(out0, 4)),
        dict(out1=dptr(out1, 12)),
    ])
    assert f(B=0) == 0
    assert_untouched(out0, out1)
    ctx.close()


# ---- tests 5 to 7: a real key ----------------------------------------------------------------------------------------
STEPS = (1, -3)


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: the special-prime Galois
    keys of the steps 1 and -3 and the special-prime relinearisation key, installed; digit Galois keys of the same steps,
    installed; B = 4 fresh symmetric records with slot values in [-1, 1] and the same records dropped to np - 1 primes by
    ct_drop_primes (equal to the slices)."""
    ctx, sk = case["ctx"], case["sk"]
    n, npr = ctx.n, ctx.np
    elts = step_elements(env, n, STEPS)
    gk0, gk1 = install_galois_keys(case, elts, "sp-gk-e2e", sp=True)
    evk0, evk1 = ctx.gen_relin_key_sp(sk, *galois_seeds(npr, 1, "sp-relin-e2e", sp=True))
    ctx.set_relin_key_sp(evk0, evk1)
    install_galois_keys(case, elts, "sp-dgk")
    vals = unit_values(4, n, 3000 + n)
    c0, c1 = fresh_records(env, ctx, vals, 200)
    case.update(elts=elts, gk0=gk0, gk1=gk1, evk0=evk0, evk1=evk1, vals=vals,
                dropped=drop_records(env, ctx, c0, c1, npr - 1))


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_sp_exact_key_switch_identity(env, keyed_cases, shape):
    """Test 5, at L = np - 1 on fresh dropped records: with y the oracle's centred decrypt of a record, y' that of its
    rotation, D_j the centred digits of sigma(c1), e_j the key's errors recovered with the oracle, delta_k of the
    definition and T = sum_j negacyclic(D_j, e_j): T - delta_0 - negacyclic(delta_1, s) is divisible by P in every
    coefficient and y' - sigma(y) equals the quotient as integers; sigma acts on the integers."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    o, s_hat, ctx = c["o"], c["s_hat"], c["ctx"]
    n, npr = shape
    L = npr - 1
    lo = Oracle(n, L)
    s_nat = centred(o.expand_ternary(c["sk"], 0), o.q[0])
    l0, l1 = (x[:2] for x in c["dropped"])
    for k, g in enumerate(c["elts"]):
        k0, k1 = c["gk0"][k], c["gk1"][k]
        errs = key_errors(o, k0, k1, s_hat, sigma_rows(o, np.stack(s_hat[:L]), g))
        g0, g1 = run_galois_sp(env, ctx, dev_t(env, l0), dev_t(env, l1), g, L)
        for b in range(2):
            y = np.array(expectation(lo, l0[b], l1[b], s_hat[:L])["y"], dtype=object)
            y2 = np.array(expectation(lo, g0[b], g1[b], s_hat[:L])["y"], dtype=object)
            quo = switch_quotient(o, sigma_rows(o, l1[b], g), k0, k1, errs, s_nat)
            assert ((y2 - sigma_coeff(y, g)) == quo.astype(object)).all(), (g, b)
            print(f"element {g}, record {b}: max |key-switch term| = {int(np.abs(quo).max())}")


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_sp_rotation_end_to_end_at_the_fresh_scale(env, keyed_cases, shape):
    """Test 6: encrypt -> ct_drop_primes -> ct_galois_sp (step 1, then step -3 on a second pass) ->
    decrypt_level(primes = np - 1, scale = Delta) on B = 4 records with slot values in [-1, 1]: every stage equals its
    definition, the final pte / values / values_f64 equal the oracle's on the final records bit for bit, and the slots are
    within the reference's 0.1 of np.roll(vals, -s) (applied to the expectation first; the CPU simulation,
    tools/ct_keyswitch_sp_noise_sim.py, puts the error near 6e-4 and 1.5e-3).  The same unlifted records through the
    digit entry se_amd_ct_galois_device miss 0.1: the regression the special prime exists for.  The worst error is
    printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    L = npr - 1
    lo = Oracle(n, L)
    B = c["vals"].shape[0]
    l0, l1 = c["dropped"]
    d0, d1 = dev_t(env, l0), dev_t(env, l1)
    for k, (s, g) in enumerate(zip(STEPS, c["elts"])):
        g0, g1 = run_galois_sp(env, ctx, d0, d1, g, L)
        e0, e1 = galois_sp_expect(o, l0, l1, g, c["gk0"][k], c["gk1"][k])
        assert (g0 == e0).all() and (g1 == e1).all(), s
        want = np.roll(c["vals"].astype(np.float64), -s, axis=1)
        check_level_decrypt(env, ctx, lo, g0, g1, c["s_hat"], L, o.scale, want, f"step {s}")
        # the digit key switch on the same unlifted records drowns the message
        x0, x1 = run_galois(env, ctx, d0, d1, g, L)
        dig = run_decrypt(env, ctx, dev_t(env, x0), dev_t(env, x1), L, o.scale)
        for b in range(B):
            err_d = float(np.abs(dig["values"][b].cpu().numpy().astype(np.float64) - want[b]).max())
            print(f"step {s}, record {b}: digit key switch without a lift: {err_d:.3e}")
            assert not err_d < 0.1, (s, b, err_d)


@pytest.mark.parametrize("shape", [(8192, 6), (4096, 3)], ids=SHAPE_IDS)
def test_sp_product_without_the_raised_scale(env, keyed_cases, shape):
    """Test 7: ct_drop_primes -> ct_mul (squares) -> ct_relin_sp -> ct_rescale -> decrypt_level(primes = L - 1, scale =
    Delta^2 / q_{L-1}), L = np - 1, on B = 4 records with slot values in [-1, 1]: the relinearisation and the rescale
    equal their definitions, the final outputs equal the oracle's bit for bit and the slots are within 0.1 of the squared
    values, on the expectation first.  tools/ct_keyswitch_sp_noise_sim.py gives 7.3e-3 at 8192 x 6 (L = 5) and 3.3e-3 at
    4096 x 3 (L = 2), both inside 0.1, so both shapes run (8.9e-5 and 4.9e-5 without any key switch: at scale
    Delta^2 / q = 2^20 the key-switch term of a few hundred per coefficient is what is left)."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    L = npr - 1
    lo, lo1 = Oracle(n, L), Oracle(n, L - 1)
    B = c["vals"].shape[0]
    l0, l1 = c["dropped"]
    d0, d1 = dev_t(env, l0), dev_t(env, l1)
    words = B * L * n
    t = [sentinel_out(env, words, 2 * n) for _ in range(3)]
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.ct_mul(d0, d1, d0, d1, t[0], t[1], t[2], primes=L, status=st)
    torch.cuda.synchronize()
    assert bool((st == 1).all())
    m = [take(x, words, (B, L, n), "tensor") for x in t]
    qv = np.array(o.q[:L], dtype=np.uint64)[None, :, None]
    w0, w1 = l0.astype(np.uint64), l1.astype(np.uint64)
    assert (m[0] == (w0 * w0) % qv).all() and (m[1] == (2 * ((w0 * w1) % qv)) % qv).all() and (m[2] == (w1 * w1) % qv).all()
    r0, r1 = run_relin_sp(env, ctx, *(dev_t(env, x) for x in m), L)
    e0, e1 = relin_sp_expect(o, m[0][:2], m[1][:2], m[2][:2], c["evk0"], c["evk1"])
    assert (r0[:2] == e0).all() and (r1[:2] == e1).all()
    f0, f1 = rescale_records(env, ctx, lo, r0, r1, L)
    scale = o.scale * o.scale / o.q[L - 1]
    check_level_decrypt(env, ctx, lo1, f0, f1, c["s_hat"], L - 1, scale, c["vals"].astype(np.float64) ** 2, "squares")


# ---- test 8: the example --------------------------------------------------------------------------------------------
def test_rotate_fresh_example(env, tmp_path):
    """examples/rotate_fresh_roundtrip.c from plain gcc: encrypt, drop to np - 1, one rotation at the fresh scale and a
    decrypt at the same scale come back within the reference's 0.1."""
    run_example("rotate_fresh_roundtrip", tmp_path, ("4096", "3", "8", "1"))
