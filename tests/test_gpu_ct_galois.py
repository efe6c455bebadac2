"""Slot rotations (-m gpu): Galois keys (se_amd_gen_galois_keys, se_amd_set_galois_keys) and the automorphism fused with
its key switch, se_amd_ct_galois_device.
Every expectation is built from the oracle's primitives (ntt, intt, decrypt, fft, expand_ternary) and Python / NumPy
integers, never from the code under test.  The automorphism of an expectation is its coefficient-domain definition
x^k -> +-x^(k g mod n) pushed through o.intt and o.ntt, never se_amd_galois_table.  Every comparison is bit-exact except
the reference's own acceptance criterion |values - expected| < 0.1 (device/test/ckks_tests_common.c:132).
Oracle(n, L - 1) is the oracle of the level below Oracle(n, L): the default chains are prefixes of one another."""
import numpy as np
import pytest

import vectors as V
from ct_model import (CASE_IDS, GALOIS_CASES, SHAPE_IDS, digit_key_errors, digits_of, edge_row, galois_diagonal,
                      galois_expect, galois_seeds, lift_expect, negacyclic, rand_slab, random_keys, sigma_slab, src_table)
from gpu_support import (NULL, SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched,  # noqa: F401
                         assert_zero_prefix, check_headroom, check_level_decrypt, dev_t, dptr, env, expectation,
                         fresh_records, host_u32, hptr, install_galois_keys, keyed_cases, lift_records, ntt_secret,
                         rescale_records, run_example, run_galois, step_elements, stream_of, unit_values)
from vectors import sigma_coeff

pytestmark = pytest.mark.gpu

LIFT = 1 << 30


# ---- test 1: the definition on arbitrary slabs and key words --------------------------------------------------------
@pytest.mark.parametrize("shape,levels,B", GALOIS_CASES, ids=CASE_IDS)
def test_galois_arbitrary_slabs_and_key(env, shape, levels, B):
    """Test 1: random residues for both slabs and for the installed keys of the elements 3 and n + 1 (n + 1 moves no
    coefficient and negates every odd one); record 0 of c1 holds 0, 1, the digit boundaries and q - 1 on negated and on
    kept positions, record 1 is all q_j - 1; against the definition.  A lower level uses the rows r < 2L and columns
    i < L of the same keys; the sentinels behind the outputs survive.  No secret key is installed."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    q = o.q
    rng = np.random.default_rng(37 * n + npr)
    elts = [3, n + 1]
    gk0, gk1 = random_keys(rng, q, len(elts), n, npr)
    ctx.set_galois_keys(elts, gk0, gk1)
    for L in levels:
        c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
        for j in range(L):
            c1[0, j] = edge_row(o, j, rng, elts)
        c0[1] = c1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
        d0, d1 = dev_t(env, c0), dev_t(env, c1)
        for k, g in enumerate(elts):
            e0, e1 = galois_expect(o, c0, c1, g, gk0[k], gk1[k])
            g0, g1 = run_galois(env, ctx, d0, d1, g, L)
            assert (g0 == e0).all() and (g1 == e1).all(), (L, g)
    ctx.close()


# ---- test 2: the relinearisation twin -------------------------------------------------------------------------------
def test_galois_is_relin_of_the_permuted_record(env):
    """Test 2: at 4096 x 3 the outputs have the bytes of ct_relin(sigma(c0), 0, sigma(c1)) with the element's key
    installed as the relinearisation key; sigma is an index_select along the row."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 3
    R = 2 * npr
    ctx = env["pkg"].Context(n, npr)
    q = ctx.moduli()
    rng = np.random.default_rng(4096 * 3 + 2)
    elts = [pow(3, 7, 2 * n), 2 * n - 1]
    gk0 = np.stack([np.stack([rand_slab(rng, q, 1, n)[0] for _ in range(R)]) for _ in elts])
    gk1 = np.stack([np.stack([rand_slab(rng, q, 1, n)[0] for _ in range(R)]) for _ in elts])
    ctx.set_galois_keys(elts, gk0, gk1)
    c0, c1 = dev_t(env, rand_slab(rng, q, B, n)), dev_t(env, rand_slab(rng, q, B, n))
    for k, g in enumerate(elts):
        src = dev_t(env, src_table(n, g))
        p0, p1 = c0.index_select(2, src).contiguous(), c1.index_select(2, src).contiguous()
        ctx.set_relin_key(gk0[k], gk1[k])
        r0, r1 = torch.full_like(c0, SENTINEL), torch.full_like(c0, SENTINEL)
        ctx.ct_relin(p0, torch.zeros_like(p1), p1, r0, r1)
        g0, g1 = run_galois(env, ctx, c0, c1, g, npr)
        torch.cuda.synchronize()
        assert (g0 == host_u32(r0)).all() and (g1 == host_u32(r1)).all(), g
    ctx.close()


# ---- test 3: key generation, installs and their refusals ------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_galois_key_generation(env, shape):
    """Test 3: gen_galois_keys for {3, 3^-1, 2n - 1} equals gen_keys_batch(K = 2 np, this key replicated, the element's
    block of seeds) plus the diagonal from the oracle's NTT(s) and sigma in Python; exactly the diagonal columns differ;
    nothing installed in the context is touched.  ct_galois without a key, or for an element that is not installed, is
    SE_ERR_NO_KEY; an install with a word == q_i, a duplicate or an even element is refused and the previous set still
    works."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    pkg = env["pkg"]
    n, npr = shape
    R = 2 * npr
    o = Oracle(n, npr)
    ctx = pkg.Context(n, npr)
    sk = V.secret_key(n, seed=3)
    elts = [3, pow(3, -1, 2 * n), 2 * n - 1]
    G = len(elts)
    sa, se = galois_seeds(npr, G, "gk-keygen")
    gk0, gk1 = ctx.gen_galois_keys(sk, elts, sa, se)
    s_hat = ntt_secret(o, sk)
    sa, se = np.asarray(sa).reshape(G, R, 64), np.asarray(se).reshape(G, R, 64)
    for k, g in enumerate(elts):
        _, pk0, pk1 = ctx.gen_keys_batch(sa[k], se[k], sk_in=np.tile(sk, (R, 1)))
        exp0 = pk0.copy()
        for j in range(npr):
            for t in range(2):
                exp0[2 * j + t, j] = (pk0[2 * j + t, j].astype(np.uint64) + galois_diagonal(o, s_hat, g, j, t)) % np.uint64(o.q[j])
        assert (gk1[k] == pk1).all(), g
        assert (gk0[k] == exp0).all(), g
        assert (gk0[k] != pk0).any(axis=2).sum() == R, g      # exactly the diagonal columns changed
    # the generator installed nothing: no secret key, no Galois key
    B = 2
    slab = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    assert ctx.L.se_amd_decrypt_level_device(ctx.h, dptr(slab), dptr(slab), B, npr, ctx.scale(), NULL, NULL, NULL,
                                             dptr(st), stream_of(env)) == SE_ERR_NO_KEY
    out0, out1 = torch.full_like(slab, SENTINEL), torch.full_like(slab, SENTINEL)
    gal = CEntry(ctx.L.se_amd_ct_galois_device, ctx=ctx.h, c0=dptr(slab), c1=dptr(slab), B=B, primes=npr, elt=3,
                 out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    assert gal(elt=3) == SE_ERR_NO_KEY
    # a refused first install installs nothing
    bad0 = gk0.copy()
    bad0[0, 0, 0, 0] = o.q[0]
    with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
        ctx.set_galois_keys(elts, bad0, gk1)
    assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    assert gal(elt=3) == SE_ERR_NO_KEY
    assert_untouched(out0, out1)
    assert_untouched(st, fill=77)
    # the first two elements are installed: the third is not there
    ctx.set_galois_keys(elts[:2], gk0[:2], gk1[:2])
    assert gal(elt=elts[2]) == SE_ERR_NO_KEY and gal(elt=5) == SE_ERR_NO_KEY
    rng = np.random.default_rng(n + npr)
    c0, c1 = rand_slab(rng, o.q, B, n), rand_slab(rng, o.q, B, n)
    d0, d1 = dev_t(env, c0), dev_t(env, c1)
    want = galois_expect(o, c0[:1], c1[:1], elts[1], gk0[1], gk1[1])

    def previous_set_works():
        g0, g1 = run_galois(env, ctx, d0, d1, elts[1], npr)
        assert (g0[:1] == want[0]).all() and (g1[:1] == want[1]).all()
        assert gal(elt=elts[2]) == SE_ERR_NO_KEY

    previous_set_works()
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
            ctx.set_galois_keys(el, k0, k1)
        assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value), el
        previous_set_works()
    # a new install replaces the whole set
    ctx.set_galois_keys(elts[2:], gk0[2:], gk1[2:])
    assert gal(elt=elts[1]) == SE_ERR_NO_KEY and gal(elt=elts[2]) == 0
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(out0)) == 0 and int(torch.count_nonzero(out1)) == 0    # zero slabs rotate to zero
    # the generator's own refusals
    bad_sk = sk.copy()
    bad_sk[5] |= 0x03
    for args in ((bad_sk, elts), (sk, [3, 6, 5]), (sk, [3, 2 * n + 1, 5])):
        with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
            ctx.gen_galois_keys(args[0], args[1], sa, se)
        assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    el = np.array(elts, dtype=np.uint32)
    gen = CEntry(ctx.L.se_amd_gen_galois_keys, ctx=ctx.h, sk=hptr(sk), elts=hptr(el), G=G, seeds_a=hptr(sa),
                 seeds_e=hptr(se), gk0=hptr(gk0), gk1=hptr(gk1))
    install = CEntry(ctx.L.se_amd_set_galois_keys, ctx=ctx.h, elts=hptr(el), G=G, gk0=hptr(gk0), gk1=hptr(gk1))
    for Gbad in (0, 65):
        gen.refused([dict(G=Gbad)])
        install.refused([dict(G=Gbad)])
    assert gal(elt=elts[2]) == 0
    ctx.close()


# ---- test 4: arguments ----------------------------------------------------------------------------------------------
def test_galois_arguments(env):
    """The argument errors return -22 and write nothing; B = 0 is a successful no-op; a level-2 call writes B . 2 . n
    words and nothing behind them."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 2
    ctx = env["pkg"].Context(n, npr)
    key = np.zeros((1, 2 * npr, npr, n), dtype=np.uint32)
    ctx.set_galois_keys([3], key, key)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    f = CEntry(ctx.L.se_amd_ct_galois_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, primes=3, elt=3,
               out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    f.refused([
        dict(ctx=None),
        dict(c0=NULL),                                                 # NULL mandatory pointers
        dict(c1=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(primes=0),                                                # primes outside [1, np]
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
    assert f(elt=5) == SE_ERR_NO_KEY
    assert f(B=0) == 0
    assert_untouched(out0, out1)
    assert f(primes=2) == 0
    for o in (out0, out1):
        assert_zero_prefix(o, B * 2 * n)
    ctx.close()


# ---- tests 5 and 6: a real key ---------------------------------------------------------------------------------------
STEPS = (1, -3)


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: the Galois keys of the
    steps 1 and -3, installed; B = 4 fresh symmetric records with slot values in [-1, 1] and the same records lifted by
    2^30 in the test's own integers."""
    ctx, o = case["ctx"], case["o"]
    n = ctx.n
    elts = step_elements(env, n, STEPS)
    gk0, gk1 = install_galois_keys(case, elts, "gk-e2e")
    vals = unit_values(4, n, 3000 + n)
    c0, c1 = fresh_records(env, ctx, vals, 200)
    case.update(elts=elts, gk0=gk0, gk1=gk1, vals=vals, fresh=(c0, c1),
                lifted=(lift_expect(o, host_u32(c0), LIFT), lift_expect(o, host_u32(c1), LIFT)))


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_galois_exact_key_switch_identity(env, keyed_cases, shape):
    """Test 5: with y the oracle's centred decrypt of a lifted record, y' that of its rotation, D_r the digits of
    sigma(c1) and e_r the key's errors recovered with the oracle (centred INTT of gk0 + gk1 . s_hat - diagonal),
    y' - sigma(y) == sum_r negacyclic(D_r, e_r) as integers for every coefficient; sigma acts on the integers."""
    c = keyed_cases(shape)
    o, s_hat, npr, ctx = c["o"], c["s_hat"], c["o"].np, c["ctx"]
    l0, l1 = (x[:2] for x in c["lifted"])
    for k, g in enumerate(c["elts"]):
        errs = digit_key_errors(o, c["gk0"][k], c["gk1"][k], s_hat, lambda j, t: galois_diagonal(o, s_hat, g, j, t))
        g0, g1 = run_galois(env, ctx, dev_t(env, l0), dev_t(env, l1), g, npr)
        p1 = sigma_slab(o, l1, g)
        for b in range(2):
            y = np.array(expectation(o, l0[b], l1[b], s_hat)["y"], dtype=object)
            y2 = np.array(expectation(o, g0[b], g1[b], s_hat)["y"], dtype=object)
            ks = np.zeros(o.n, dtype=np.int64)
            for dig, er in zip(digits_of(o, p1[b], npr), errs):
                ks += negacyclic(dig.astype(np.int64), er)         # n . 2^15 . 64 per term: far below 2^62
            assert ((y2 - sigma_coeff(y, g)) == ks.astype(object)).all(), (g, b)
            print(f"element {g}, record {b}: max |key-switch term| = {int(np.abs(ks).max())}")


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_rotation_end_to_end(env, keyed_cases, shape):
    """Test 6: ct_lincomb with weight 2^30 -> ct_galois (step 1, then step -3 on a second pass) -> ct_rescale ->
    decrypt_level(primes = np - 1, scale = Delta 2^30 / q_last) on B = 4 records with slot values in [-1, 1]: every
    stage equals its definition, the final pte / values / values_f64 equal the oracle's on the final records bit for
    bit, and the slots are within the reference's 0.1 of np.roll(vals, -s) (applied to the expectation first; a CPU
    simulation of the same chain, tools/ct_galois_noise_sim.py, puts the error near 1e-4).  The worst error is
    printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    lo = Oracle(n, npr - 1)
    l0, l1 = lift_records(env, ctx, o, c["fresh"], LIFT)
    assert (l0 == c["lifted"][0]).all() and (l1 == c["lifted"][1]).all()
    scale = o.scale * LIFT / o.q[npr - 1]
    for k, (s, g) in enumerate(zip(STEPS, c["elts"])):
        g0, g1 = run_galois(env, ctx, dev_t(env, l0), dev_t(env, l1), g, npr)
        e0, e1 = galois_expect(o, l0[:2], l1[:2], g, c["gk0"][k], c["gk1"][k])
        assert (g0[:2] == e0).all() and (g1[:2] == e1).all(), s
        check_headroom(o, g0, g1, c["s_hat"], f"step {s}")
        f0, f1 = rescale_records(env, ctx, o, g0, g1, npr, s)
        want = np.roll(c["vals"].astype(np.float64), -s, axis=1)
        check_level_decrypt(env, ctx, lo, f0, f1, c["s_hat"], npr - 1, scale, want, f"step {s}")


# ---- test 7: the example --------------------------------------------------------------------------------------------
def test_slot_sum_example(env, tmp_path):
    """examples/slot_sum_roundtrip.c from plain gcc: packed dot products through the tensor, relin, four rotate-and-adds,
    rescale and decrypt_level come back within the reference's 0.1."""
    run_example("slot_sum_roundtrip", tmp_path, ("4096", "3", "8"))
