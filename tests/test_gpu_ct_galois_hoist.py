"""Hoisted rotations (-m gpu): se_amd_ct_galois_many_device and se_amd_ct_galois_sum_device, many rotations of a record
from one digit decomposition under the installed Galois keys.
Every expectation is written from the definition with the oracle's primitives (ntt, intt,
decrypt, fft, expand_ternary), se_amd_galois_table -- a host-only entry pinned against the coefficient-domain
automorphism by tests/test_ct_galois_build.py -- and Python / NumPy integers, never from the device code under test:
    D_{j,t}          = digits_of(c1)                                  (of c1 itself, not of sigma(c1))
    rot0[g][b][i][k] = c0[b][i][src_g(k)] + sum_r NTT_i(D_r)[src_g(k)] . gk0_g[r][i][k]   mod q_i
    rot1[g][b][i][k] =                      sum_r NTT_i(D_r)[src_g(k)] . gk1_g[r][i][k]   mod q_i.
Every comparison is bit-exact except the reference's own acceptance criterion |values - expected| < 0.1
(device/test/ckks_tests_common.c:132).  Oracle(n, L - 1) is the oracle of the level below Oracle(n, L)."""
import numpy as np
import pytest

from ct_model import (CASE_IDS, DIGIT_MASK, GALOIS_CASES, SHAPE_IDS, call_elements, digit_key_errors, digits_of,
                      edge_row, galois_diagonal, hoist_expect, lift_expect, modular_sum, negacyclic, rand_slab,
                      random_keys)
from gpu_support import (NULL, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched, assert_zero_prefix,  # noqa: F401
                         check_headroom, check_level_decrypt, dev_t, dptr, env, expectation, fresh_records, host_u32,
                         hptr, install_galois_keys, keyed_cases, lift_records, rescale_records, run_example, run_many,
                         run_sum, step_elements, stream_of, unit_values)
from vectors import sigma_coeff

pytestmark = pytest.mark.gpu

LIFT = 1 << 30
GC = 2          # kHoistGroup of kernels/ct_ops.hip: elements in flight of the many form


# ---- tests 1 and 2: the definition on arbitrary slabs and key words -------------------------------------------------
@pytest.fixture(scope="module")
def slab_cases(env):
    """slab_cases(shape, levels, B) -> per level the slabs, the expectation of the many form and what ONE many-form
    device call returned, computed once and shared by tests 1 and 2.  Random key words, no secret key installed."""
    from oracle.pyoracle import Oracle
    cache = {}

    def get(shape, levels, B):
        if shape in cache:
            return cache[shape]
        n, npr = shape
        o = Oracle(n, npr)
        ctx = env["pkg"].Context(n, npr)
        q = o.q
        rng = np.random.default_rng(41 * n + npr)
        elts = call_elements(n, npr)          # 4096 x 3: G = 7 is above GC and no multiple of it, the last group is short
        assert shape != (4096, 3) or (len(elts) > GC and len(elts) % GC != 0)
        keys = sorted(set(elts))
        key_of = {g: k for k, g in enumerate(keys)}
        gk0, gk1 = random_keys(rng, q, len(keys), n, npr)
        ctx.set_galois_keys(keys, gk0, gk1)
        per_level = {}
        for L in levels:
            c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
            for j in range(L):
                c1[0, j] = edge_row(o, j, rng, elts, starts=6)
            c0[1] = c1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
            d0, d1 = dev_t(env, c0), dev_t(env, c1)
            exp = hoist_expect(env["pkg"].galois_table, o, c0, c1, elts, key_of, gk0, gk1)
            got = run_many(env, ctx, d0, d1, elts, L)
            per_level[L] = dict(c0=c0, c1=c1, d0=d0, d1=d1, exp=exp, got=got)
        cache[shape] = dict(ctx=ctx, o=o, elts=elts, levels=per_level)
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()



@pytest.mark.parametrize("shape,levels,B", GALOIS_CASES, ids=CASE_IDS)
def test_many_arbitrary_slabs_and_key(slab_cases, shape, levels, B):
    """Test 1: random residues for both slabs and for the installed keys; record 0 of c1 holds 0, 1, the digit
    boundaries and q - 1 on negated and on kept positions, record 1 is all q_j - 1; out[e] against the definition for
    every element of the call, one of them listed twice, the last group short at 4096 x 3.  A lower level uses the rows
    r < 2L and columns i < L of the same keys; the sentinels behind the outputs survive (run_many)."""
    case = slab_cases(shape, levels, B)
    for L in levels:
        lv = case["levels"][L]
        for e, g in enumerate(case["elts"]):
            assert (lv["got"][0][e] == lv["exp"][0][e]).all(), (L, e, g, "out0")
            assert (lv["got"][1][e] == lv["exp"][1][e]).all(), (L, e, g, "out1")


@pytest.mark.parametrize("shape,levels,B", GALOIS_CASES, ids=CASE_IDS)
def test_sum_is_the_modular_sum_of_the_many_form(env, slab_cases, shape, levels, B):
    """Test 2: on the slabs of test 1 the sum form equals the modular sum of the many form's expectation and of what
    test 1's device call returned, with add_input 0 and 1, for G = 1 and for the whole element list (an element listed
    twice counts twice)."""
    case = slab_cases(shape, levels, B)
    o, ctx, elts = case["o"], case["ctx"], case["elts"]
    for L in levels:
        lv = case["levels"][L]
        for G in (1, len(elts)):
            for add in (False, True):
                want = [modular_sum(o, lv["exp"][h][:G], lv[f"c{h}"] if add else None) for h in (0, 1)]
                from_device = [modular_sum(o, lv["got"][h][:G], lv[f"c{h}"] if add else None) for h in (0, 1)]
                s0, s1 = run_sum(env, ctx, lv["d0"], lv["d1"], elts[:G], L, add)
                assert (s0 == want[0]).all() and (s1 == want[1]).all(), (L, G, add)
                assert (s0 == from_device[0]).all() and (s1 == from_device[1]).all(), (L, G, add)


# ---- test 3: arguments ----------------------------------------------------------------------------------------------
def test_hoist_arguments(env):
    """Both entries: every argument error returns its documented code and leaves the sentinel-filled outputs untouched
    (G = 0 and 65, an even element, one >= 2n, a NULL element list, an element without a key -- SE_ERR_NO_KEY with the
    element named in the text --, a NULL or misaligned slab, a level of 0 or above np, B >= 2^32); B = 0 succeeds and
    writes nothing; after a refused set_galois_keys the entries still run on the previous set."""
    torch, pkg = env["torch"], env["pkg"]
    n, npr, B = 4096, 3, 2
    ctx = pkg.Context(n, npr)
    key = np.zeros((2, 2 * npr, npr, n), dtype=np.uint32)
    ctx.set_galois_keys([3, 9], key, key)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    out0 = torch.full((2, B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    el = lambda *g: np.array(g + (0,) * (65 - len(g)), dtype=np.uint32)     # room for the G = 65 call
    good, even, big, nokey = el(3, 9), el(3, 4), el(3, 2 * n + 1), el(3, 5)
    L = ctx.L
    many = CEntry(L.se_amd_ct_galois_many_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, primes=3, elts=hptr(good),
                  G=2, out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    total = CEntry(L.se_amd_ct_galois_sum_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, primes=3, elts=hptr(good),
                   G=2, add_input=1, out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    bad_calls = [
        dict(ctx=None),
        dict(c0=NULL),                                        # NULL mandatory pointers
        dict(c1=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(elts=NULL),                                      # NULL element list
        dict(primes=0),                                       # primes outside [1, np]
        dict(primes=4),
        dict(B=2 ** 32),                                      # B >= 2^32
        dict(c0=dptr(c0, 4)),                                 # alignment, each slab
        dict(c1=dptr(c1, 8)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
        dict(G=0),                                            # G = 0, G = 65
        dict(G=65),
        dict(elts=hptr(even)),                                # an even element, one >= 2n
        dict(elts=hptr(big)),
    ]
    for f in (many, total):
        f.refused(bad_calls)
        assert f(elts=hptr(nokey)) == SE_ERR_NO_KEY
        assert "element 5" in L.se_amd_last_error().decode(), L.se_amd_last_error()
        assert f(B=0) == 0
    assert_untouched(out0, out1)
    # a refused install leaves the previous set to the hoisted entries: zero keys and zero slabs give zero rows
    bad = key.copy()
    bad[1, 0, 0, 0] = ctx.moduli()[0]
    with pytest.raises(pkg.SealEmbeddedAmdError):
        ctx.set_galois_keys([3, 9], bad, key)
    with pytest.raises(pkg.SealEmbeddedAmdError):
        ctx.set_galois_keys([3, 5, 3], np.zeros((3,) + key.shape[1:], dtype=np.uint32),
                            np.zeros((3,) + key.shape[1:], dtype=np.uint32))
    assert many(primes=2, elts=hptr(nokey)) == SE_ERR_NO_KEY                   # 5 was not installed
    assert many(primes=2) == 0                                                 # a level-2 call: 2 . B . 2 . n words
    for o in (out0, out1):
        assert_zero_prefix(o, 2 * B * 2 * n)
    out0.fill_(SENTINEL)
    out1.fill_(SENTINEL)
    assert total() == 0
    for o in (out0, out1):
        assert_zero_prefix(o, B * 3 * n)
    ctx.close()


# ---- tests 4 and 5: a real key ---------------------------------------------------------------------------------------
WINDOW = tuple(range(1, 8))          # the steps of the moving sum
STEPS = WINDOW + (-3,)               # ... and a right rotation for the many form


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: the Galois keys of the
    steps 1 .. 7 and -3, installed; B = 4 fresh symmetric records with slot values in [-1, 1] and the same records
    lifted by 2^30 in the test's own integers (the records of the rotation tests)."""
    ctx, o = case["ctx"], case["o"]
    n = ctx.n
    elts = step_elements(env, n, STEPS)
    gk0, gk1 = install_galois_keys(case, elts, "gk-hoist")
    vals = unit_values(4, n, 3000 + n)
    c0, c1 = fresh_records(env, ctx, vals, 200)
    case.update(elts=elts, key_of={g: k for k, g in enumerate(elts)}, gk0=gk0, gk1=gk1, vals=vals, fresh=(c0, c1),
                lifted=(lift_expect(o, host_u32(c0), LIFT), lift_expect(o, host_u32(c1), LIFT)))


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_hoist_exact_key_switch_identity(env, keyed_cases, shape):
    """Test 4: with y the oracle's centred decrypt of a lifted record, y' that of rot[g] from ONE many-form call with the
    steps 1 .. 7, D_r = digits_of(c1), unrotated, and e_r the key's errors recovered with the oracle (centred INTT of
    gk0 + gk1 . s_hat - diagonal),  y' - sigma(y) == sum_r negacyclic(sigma_int(D_r), e_r)  as integers for every
    coefficient, element and record; sigma_int = sigma_coeff on the integers, with its signs.
    The products run in float64, where they are exact: a term is below n . 2^15 . 64 <= 2^34 and the sum of the 2 np
    terms below 2^38, far inside the 2^53 of the format."""
    c = keyed_cases(shape)
    o, s_hat, npr, ctx = c["o"], c["s_hat"], c["o"].np, c["ctx"]
    l0, l1 = (x[:2] for x in c["lifted"])
    elts = c["elts"][:len(WINDOW)]
    g0, g1 = run_many(env, ctx, dev_t(env, l0), dev_t(env, l1), elts, npr)
    ys = [np.array(expectation(o, l0[b], l1[b], s_hat)["y"], dtype=object) for b in range(2)]
    digs = [[d.astype(np.int64) for d in digits_of(o, l1[b], npr)] for b in range(2)]
    for k, g in enumerate(elts):
        errs = [e.astype(np.float64) for e in digit_key_errors(o, c["gk0"][k], c["gk1"][k], s_hat,
                                                               lambda j, t: galois_diagonal(o, s_hat, g, j, t))]
        for b in range(2):
            y2 = np.array(expectation(o, g0[k, b], g1[k, b], s_hat)["y"], dtype=object)
            ks = np.zeros(o.n, dtype=np.float64)
            for dig, er in zip(digs[b], errs):
                sd = sigma_coeff(dig, g)
                assert np.abs(sd).max() <= DIGIT_MASK
                ks += negacyclic(sd.astype(np.float64), er)
            assert np.abs(ks).max() < 2.0 ** 52 and (ks == np.rint(ks)).all()
            assert ((y2 - sigma_coeff(ys[b], g)) == ks.astype(np.int64).astype(object)).all(), (g, b)
            print(f"element {g}, record {b}: max |key-switch term| = {int(np.abs(ks).max())}")


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_moving_sum_end_to_end(env, keyed_cases, shape):
    """Test 5: ct_lincomb with weight 2^30 -> ct_galois_sum (steps 1 .. 7, add_input) -> ct_rescale ->
    decrypt_level(primes = np - 1, scale = Delta 2^30 / q_last) on B = 4 records with slot values in [-1, 1]: every stage
    equals its definition, the final pte / values / values_f64 equal the oracle's on the final records bit for bit,
    every coefficient before the rescale is below 2^62, and the slots are within the reference's 0.1 of the moving sums
    of 8 of vals (applied to the expectation first).  The many form with the steps 1 and -3, rescaled and decrypted, is
    within 0.1 of np.roll.  The worst errors are printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    lo = Oracle(n, npr - 1)
    l0, l1 = lift_records(env, ctx, o, c["fresh"], LIFT)
    assert (l0 == c["lifted"][0]).all() and (l1 == c["lifted"][1]).all()
    scale = o.scale * LIFT / o.q[npr - 1]
    window = c["elts"][:len(WINDOW)]
    d0, d1 = dev_t(env, l0), dev_t(env, l1)
    rot = hoist_expect(env["pkg"].galois_table, o, l0, l1, c["elts"], c["key_of"], c["gk0"], c["gk1"])

    def finish(g0, g1, want_slots, what):
        """rescale and decrypt the level-np records (g0, g1) against their definitions and want_slots."""
        check_headroom(o, g0, g1, c["s_hat"], what)
        f0, f1 = rescale_records(env, ctx, o, g0, g1, npr, what)
        check_level_decrypt(env, ctx, lo, f0, f1, c["s_hat"], npr - 1, scale, want_slots, what)

    # the moving sum: one call
    s0, s1 = run_sum(env, ctx, d0, d1, window, npr, True)
    assert (s0 == modular_sum(o, rot[0][:len(WINDOW)], l0)).all(), "sum out0"
    assert (s1 == modular_sum(o, rot[1][:len(WINDOW)], l1)).all(), "sum out1"
    v64 = c["vals"].astype(np.float64)
    finish(s0, s1, sum(np.roll(v64, -s, axis=1) for s in range(len(WINDOW) + 1)), "moving sum of 8")
    # the many form: steps 1 and -3 from one call
    pick = [STEPS.index(1), STEPS.index(-3)]
    m0, m1 = run_many(env, ctx, d0, d1, [c["elts"][k] for k in pick], npr)
    for e, k in enumerate(pick):
        assert (m0[e] == rot[0][k]).all() and (m1[e] == rot[1][k]).all(), STEPS[k]
        finish(m0[e], m1[e], np.roll(v64, -STEPS[k], axis=1), f"many form, step {STEPS[k]}")


# ---- test 6: the example --------------------------------------------------------------------------------------------
def test_moving_sum_example(env, tmp_path):
    """examples/moving_sum_roundtrip.c from plain gcc: lift, ONE se_amd_ct_galois_sum_device call with the steps 1 .. 7
    and add_input, rescale and decrypt_level come back within the reference's 0.1 of the moving sums of 8."""
    run_example("moving_sum_roundtrip", tmp_path, ("4096", "3", "8"))
