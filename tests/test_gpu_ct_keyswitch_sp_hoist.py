"""Hoisted rotations on the special-prime key (-m gpu): se_amd_ct_galois_sum_sp_device, se_amd_lintrans_create_sp and
se_amd_ct_lintrans_sp_device.
Every expectation is the definition in tests/ct_model.py (hoist_sp_expect and, for the single entry, galois_sp_expect):
the oracle's primitives and Python / NumPy integers, never the code under test.  Every comparison is bit-exact except
the reference's own acceptance criterion |values - expected| < 0.1.
Oracle(n, L) is the oracle of a level-L record of Oracle(n, np): the default chains are prefixes of one another."""
import numpy as np
import pytest

import vectors as V
from ct_model import (CASE_IDS, SHAPE_IDS, SP_CASES, add_mod, centred, edge_diagonals, edge_row, hoist_sp_expect,
                      key_errors, key_switch_sp, matrix, matrix_diagonals, negacyclic, rand_key, rand_slab, sigma_rows,
                      sum_of_single_calls)
from gpu_support import (NULL, SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched,  # noqa: F401
                         assert_zero_prefix, check_level_decrypt, create_handle, creates_refused, dev_t, dptr,
                         drop_records, encode_diagonals, env, expectation, fresh_records, guarded_pair, hptr,
                         install_galois_keys, keyed_cases, periodic_values, rescale_records, run_example, run_galois_sp,
                         step_elements, stream_of, unit_values)
from vectors import sigma_coeff

pytestmark = pytest.mark.gpu


def run_sum_sp(env, ctx, c0, c1, elts, primes, add_input):
    """One ct_galois_sum_sp call on device slabs [B][primes][n]; two rows of sentinels behind each output."""
    return guarded_pair(env, ctx.n, (c0.shape[0], primes, ctx.n), "sum_sp",
                        lambda a, b: ctx.ct_galois_sum_sp(c0, c1, elts, a, b, add_input=add_input, primes=primes))


def run_lintrans_sp(env, ctx, plan, c0, c1, primes):
    return guarded_pair(env, ctx.n, (c0.shape[0], primes, ctx.n), "lintrans_sp",
                        lambda a, b: ctx.ct_lintrans_sp(plan, c0, c1, a, b, primes=primes))


@pytest.fixture(scope="module")
def slab_cases(env):
    """slab_cases(shape, B) -> per shape, computed once and shared by tests 1 and 4: a context without a secret key, random
    special-prime Galois keys of its elements installed (key words 0, 1 and q - 1 on a data column and on column p), and
    per level the slabs: record 0 of c1 holds the edge rows, record 1 is all q_j - 1."""
    from oracle.pyoracle import Oracle
    cache = {}

    def get(shape, levels, B):
        if shape in cache:
            return cache[shape]
        n, npr = shape
        p = npr - 1
        o = Oracle(n, npr)
        ctx = env["pkg"].Context(n, npr)
        q = o.q
        rng = np.random.default_rng(43 * n + npr)
        elts = [3, n + 1] if n > 4096 else [3, n + 1, 1, 2 * n - 1]
        gk0 = np.stack([rand_key(rng, q, n) for _ in elts])
        gk1 = np.stack([rand_key(rng, q, n) for _ in elts])
        for k in (gk0[0], gk1[1]):
            k[0, 0, :4] = [0, 1, q[0] - 1, q[0] - 1]
            k[0, p, :4] = [0, 1, q[p] - 1, q[p] - 1]
        ctx.set_galois_keys_sp(elts, gk0, gk1)
        slabs = {}
        for L in levels:
            c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
            for j in range(L):
                c1[0, j] = edge_row(o, j, rng, [3, n + 1], edges="centring")     # 1 negates nothing, 2n - 1 everything but index 0
            c0[1] = c1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
            slabs[L] = (c0, c1)
        cache[shape] = dict(o=o, ctx=ctx, elts=elts, keys={g: (gk0[k], gk1[k]) for k, g in enumerate(elts)},
                            slabs=slabs, rng=rng)
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()


# ---- test 1: the definition on arbitrary slabs and key words --------------------------------------------------------
@pytest.mark.parametrize("shape,levels,B", SP_CASES, ids=CASE_IDS)
def test_sum_sp_arbitrary_slabs_and_keys(env, slab_cases, shape, levels, B):
    """Test 1: random residues for the slabs and for the installed keys; the element lists [3], [3, n + 1, 3] (a repeat
    counts twice) and [1, 2n - 1], each with add_input 0 and 1, against the definition (at 16384 x 13 the one list
    [3, n + 1, 3] with add_input).  A lower level uses rows j < L, columns i < L and column p of the same keys; the
    sentinels survive.  No secret key is installed."""
    case = slab_cases(shape, levels, B)
    n, npr = shape
    o, ctx = case["o"], case["ctx"]
    runs = [([3, n + 1, 3], 1)] if n > 4096 else [(el, a) for el in ([3], [3, n + 1, 3], [1, 2 * n - 1]) for a in (0, 1)]
    for L in levels:
        c0, c1 = case["slabs"][L]
        d0, d1 = dev_t(env, c0), dev_t(env, c1)
        for elts, add in runs:
            e0, e1, _ = hoist_sp_expect(o, c0, c1, elts, [case["keys"][g] for g in elts], w0=1 if add else None)
            g0, g1 = run_sum_sp(env, ctx, d0, d1, elts, L, bool(add))
            assert (g0 == e0).all() and (g1 == e1).all(), (L, elts, add)


# ---- test 2: one element is the single entry ------------------------------------------------------------------------
def test_sum_sp_of_one_element_has_the_bytes_of_galois_sp(env):
    """Test 2: at 4096 x 3, L = 2, B = 3, for the elements 3^7 mod 2n and 2n - 1 the sum form with G = 1 and no
    add_input has the bytes of ct_galois_sp (centring commutes with sigma); with add_input it is that plus the record,
    mod q_i."""
    n, npr, L, B = 4096, 3, 2, 3
    ctx = env["pkg"].Context(n, npr)
    q = ctx.moduli()
    rng = np.random.default_rng(4096 * 3 + 7)
    elts = [pow(3, 7, 2 * n), 2 * n - 1]
    ctx.set_galois_keys_sp(elts, np.stack([rand_key(rng, q, n) for _ in elts]),
                           np.stack([rand_key(rng, q, n) for _ in elts]))
    c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
    d0, d1 = dev_t(env, c0), dev_t(env, c1)
    qv = np.array(q[:L], dtype=np.uint64)[None, :, None]
    for g in elts:
        s0, s1 = run_galois_sp(env, ctx, d0, d1, g, L)
        h0, h1 = run_sum_sp(env, ctx, d0, d1, [g], L, False)
        assert (h0 == s0).all() and (h1 == s1).all(), g
        a0, a1 = run_sum_sp(env, ctx, d0, d1, [g], L, True)
        assert (a0 == ((s0.astype(np.uint64) + c0) % qv)).all() and (a1 == ((s1.astype(np.uint64) + c1) % qv)).all(), g
    ctx.close()


# ---- test 3: one rounding, not G ------------------------------------------------------------------------------------
def test_sum_sp_rounds_once(env):
    """Test 3, the delta boundary at 4096 x 3, L = 2, elements 1 and 3: column p of both rows of half 0 of both keys is the
    NTT of the constant 1 (all ones), so the single delta_0 of element e is centred(sigma_e(D_0 + D_1) mod P) and the
    hoisted delta_0 is centred(sigma_1(S) + sigma_3(S) mod P), S = D_0 + D_1.  S is built so that on chosen coefficients x
    the two single values a = S[x] and b = sigma_3(S)[x] each lie inside (-P/2, P/2] while a + b is (P - 1)/2,
    (P + 1)/2, -(P - 1)/2, -(P + 1)/2, P - 1, -(P - 1) and 0: at and across the boundary on both sides.  Everywhere
    else |S| < P/8, so no other coefficient wraps.  The construction is confirmed on the CPU expectation first; then
    the GPU equals the definition, the sum of two ct_galois_sp outputs equals the sum of the single expectations, and the
    two differ exactly where the expectations do."""
    from oracle.pyoracle import Oracle
    n, npr, L, B = 4096, 3, 2, 1
    o = Oracle(n, npr)
    q, p = o.q, npr - 1
    P = q[p]
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(79)
    elts = [1, 3]
    keys = []
    for _ in elts:
        k0, k1 = rand_key(rng, q, n), rand_key(rng, q, n)
        k0[0, p] = k0[1, p] = 1
        keys.append((k0, k1))
    assert (o.ntt(np.eye(1, n, 0, dtype=np.uint32)[0], p) == 1).all()
    ctx.set_galois_keys_sp(elts, np.stack([k[0] for k in keys]), np.stack([k[1] for k in keys]))
    targets = np.array([(P - 1) // 2, (P + 1) // 2, -(P - 1) // 2, -(P + 1) // 2, P - 1, -(P - 1), 0], dtype=np.int64)
    wrapped = np.array([(P - 1) // 2, -(P - 1) // 2, -(P - 1) // 2, (P - 1) // 2, -1, 1, 0], dtype=np.int64)
    assert (wrapped == centred(targets % P, P)).all()
    pos, neg = V.galois_image(n, 3)
    inv = np.empty(n, dtype=np.int64)
    inv[pos] = np.arange(n)
    xs = np.arange(5, 5 + 16 * len(targets), 16)            # the chosen coefficients, and their preimages under sigma_3
    ks = inv[xs]
    assert len(set(xs) | set(ks)) == 2 * len(targets)
    S = rng.integers(-(P // 16), P // 16, n, dtype=np.int64)
    a = targets // 2
    b = targets - a
    S[xs] = a
    S[ks] = np.where(neg[ks], -b, b)
    D0 = S // 2
    D1 = S - D0
    assert np.abs(D0).max() <= (q[0] - 1) // 2 and np.abs(D1).max() <= (q[1] - 1) // 2
    c1 = np.stack([o.ntt((D % q[j]).astype(np.uint32), j) for j, D in enumerate((D0, D1))])[None]
    c0 = rand_slab(rng, q, B, n, L)
    # the construction, on the expectations
    e0, e1, info = hoist_sp_expect(o, c0, c1, elts, keys)
    assert (info[0]["D"][0] == D0).all() and (info[0]["D"][1] == D1).all()
    single = [key_switch_sp(o, sigma_rows(o, c1[0], g), *key)["delta"][0] for g, key in zip(elts, keys)]
    assert (single[0] == S).all() and (single[1] == sigma_coeff(S, 3)).all()       # no single delta wraps anywhere
    assert (single[0][xs] == a).all() and (single[1][xs] == b).all()
    assert (info[0]["delta"][0][xs] == wrapped).all()
    total = single[0] + single[1]
    assert (info[0]["delta"][0] == centred(total % P, P)).all()
    crossing = np.abs(total) > P // 2
    assert crossing[xs].tolist() == [False, True, False, True, True, True, False]
    s0, s1 = sum_of_single_calls(o, c0, c1, elts, keys)
    assert (e0 != s0).any()
    # the GPU
    d0, d1 = dev_t(env, c0), dev_t(env, c1)
    g0, g1 = run_sum_sp(env, ctx, d0, d1, elts, L, False)
    assert (g0 == e0).all() and (g1 == e1).all()
    t0, t1 = np.zeros_like(c0), np.zeros_like(c1)
    for g in elts:
        r0, r1 = run_galois_sp(env, ctx, d0, d1, g, L)
        t0[0], t1[0] = add_mod(o, t0[0], r0[0]), add_mod(o, t1[0], r1[0])
    assert (t0 == s0).all() and (t1 == s1).all()
    assert ((g0 != t0) == (e0 != s0)).all() and ((g1 != t1) == (e1 != s1)).all()
    print(f"{int(crossing.sum())} coefficients cross the boundary; {int((e0 != s0).sum())} words of out0 differ")
    ctx.close()


# ---- test 4: the linear transform -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,levels,B", SP_CASES, ids=CASE_IDS)
def test_lintrans_sp_matches_the_definition(env, slab_cases, shape, levels, B):
    """Test 4: on the slabs and keys of test 1 (B = 2 at 16384 x 13), elements [3, n + 1, 3], diagonals of arbitrary
    32-bit words with 0, 1, q_i - 1, q_i and 2^32 - 1 on data rows and on row p, with and without diag0, against the
    definition; one plan serves every level of the case.  All-ones diagonals with diag0 all ones or absent give the
    bytes of the sum form with add_input 1 or 0."""
    torch = env["torch"]
    case = slab_cases(shape, levels, B)
    n, npr = shape
    o, ctx = case["o"], case["ctx"]
    elts = [3, n + 1, 3]
    keys = [case["keys"][g] for g in elts]
    diag = edge_diagonals(case["rng"], o.q, len(elts) + 1, n)
    t_diag = dev_t(env, diag)
    ones = torch.ones((len(elts) + 1, npr, n), dtype=torch.int32, device=env["dev"])
    for with0 in (True, False):
        plan = ctx.lintrans_plan_sp(elts, t_diag[1:].contiguous(), t_diag[0].contiguous() if with0 else None)
        unit = ctx.lintrans_plan_sp(elts, ones[1:].contiguous(), ones[0].contiguous() if with0 else None)
        for L in levels:
            c0, c1 = case["slabs"][L]
            d0, d1 = dev_t(env, c0), dev_t(env, c1)
            e0, e1, _ = hoist_sp_expect(o, c0, c1, elts, keys, diag[1:], diag[0] if with0 else None)
            g0, g1 = run_lintrans_sp(env, ctx, plan, d0, d1, L)
            assert (g0 == e0).all() and (g1 == e1).all(), (L, with0)
            u0, u1 = run_lintrans_sp(env, ctx, unit, d0, d1, L)
            s0, s1 = run_sum_sp(env, ctx, d0, d1, elts, L, with0)
            assert (u0 == s0).all() and (u1 == s1).all(), (L, with0)
        plan.close()
        unit.close()


def test_lintrans_sp_plan_is_a_snapshot(env, slab_cases):
    """Test 4: after set_galois_keys_sp with other words and after the diagonals are freed, a plan gives the bytes it
    gave before; a plan made now gives others.  The shared keys are put back."""
    shape, levels, B = SP_CASES[0]
    case = slab_cases(shape, levels, B)
    n, npr = shape
    o, ctx = case["o"], case["ctx"]
    elts, L = [3, n + 1], 2
    c0, c1 = case["slabs"][L]
    d0, d1 = dev_t(env, c0), dev_t(env, c1)
    diag = edge_diagonals(np.random.default_rng(5), o.q, 3, n)
    t_diag = dev_t(env, diag)
    old = ctx.lintrans_plan_sp(elts, t_diag[1:].contiguous(), t_diag[0].contiguous())
    before = run_lintrans_sp(env, ctx, old, d0, d1, L)
    del t_diag
    env["torch"].cuda.empty_cache()
    rng = np.random.default_rng(6)
    installed = list(case["keys"])
    try:
        ctx.set_galois_keys_sp(elts, np.stack([rand_key(rng, o.q, n) for _ in elts]),
                               np.stack([rand_key(rng, o.q, n) for _ in elts]))
        after = run_lintrans_sp(env, ctx, old, d0, d1, L)
        assert (after[0] == before[0]).all() and (after[1] == before[1]).all()
        t_diag = dev_t(env, diag)
        new = ctx.lintrans_plan_sp(elts, t_diag[1:].contiguous(), t_diag[0].contiguous())
        other = run_lintrans_sp(env, ctx, new, d0, d1, L)
        assert (other[0] != before[0]).any() and (other[1] != before[1]).any()
        new.close()
    finally:
        ctx.set_galois_keys_sp(installed, np.stack([case["keys"][g][0] for g in installed]),
                               np.stack([case["keys"][g][1] for g in installed]))
        old.close()


# ---- tests 5 and 8: a real key --------------------------------------------------------------------------------------
DIM = 8
WINDOW = tuple(range(1, DIM))          # the moving sum and the matrix use the steps 1 .. 7
IDENTITY_STEPS = (1, -3)


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: the special-prime Galois
    keys of the steps 1 .. 7 and -3, installed; B = 4 fresh symmetric records with slot values in [-1, 1] and B = 4 with
    8-periodic slot values, both dropped to np - 1 primes by ct_drop_primes (equal to the slices)."""
    ctx = case["ctx"]
    n, npr, B = ctx.n, ctx.np, 4
    steps = WINDOW + (-3,)
    elts = step_elements(env, n, steps)
    gk0, gk1 = install_galois_keys(case, elts, "sp-hoist-gk", sp=True)
    sets = dict(unit=unit_values(B, n, 6000 + n), tiled=periodic_values(B, n, DIM, 7000 + n))
    dropped = {}
    for k, (name, vals) in enumerate(sets.items()):
        c0, c1 = fresh_records(env, ctx, vals, 400 + 16 * k)
        dropped[name] = drop_records(env, ctx, c0, c1, npr - 1)
    case.update(key_of={s: (elts[k], (gk0[k], gk1[k])) for k, s in enumerate(steps)}, vals=sets, dropped=dropped)


KEYED_SHAPES = [(4096, 3), (8192, 6)]


@pytest.mark.parametrize("shape", KEYED_SHAPES, ids=SHAPE_IDS)
def test_sum_sp_exact_identity_with_a_real_key(env, keyed_cases, shape):
    """Test 5, at L = np - 1 on two fresh dropped records, steps {1, -3}, add_input: with y, y' the oracle's centred
    decrypts of the input and the output, D_j the centred digits of c1, e_{e,j} the errors of element e's key recovered
    with the oracle, delta_k of the definition and T = sum_e sum_j negacyclic(sigma_e(D_j), e_{e,j}):
    T - delta_0 - negacyclic(delta_1, s) is divisible by P in every coefficient and y' - y - sum_e sigma_e(y) equals the
    quotient as integers.  The largest coefficient of the quotient is printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    o, s_hat, ctx = c["o"], c["s_hat"], c["ctx"]
    n, npr = shape
    L = npr - 1
    P = o.q[npr - 1]
    lo = Oracle(n, L)
    s_nat = centred(o.expand_ternary(c["sk"], 0), o.q[0])
    l0, l1 = (x[:2] for x in c["dropped"]["unit"])
    elts = [c["key_of"][s][0] for s in IDENTITY_STEPS]
    keys = [c["key_of"][s][1] for s in IDENTITY_STEPS]
    errs = [key_errors(o, k0, k1, s_hat, sigma_rows(o, np.stack(s_hat[:L]), g)) for g, (k0, k1) in zip(elts, keys)]
    g0, g1 = run_sum_sp(env, ctx, dev_t(env, l0), dev_t(env, l1), elts, L, True)
    e0, e1, info = hoist_sp_expect(o, l0, l1, elts, keys, w0=1)
    assert (g0 == e0).all() and (g1 == e1).all()
    for b in range(2):
        y = np.array(expectation(lo, l0[b], l1[b], s_hat[:L])["y"], dtype=object)
        y2 = np.array(expectation(lo, g0[b], g1[b], s_hat[:L])["y"], dtype=object)
        T = np.zeros(n, dtype=np.int64)
        rotated = y.copy()
        for g, err in zip(elts, errs):
            rotated = rotated + sigma_coeff(y, g)
            for Dj, ej in zip(info[b]["D"], err):
                T += negacyclic(sigma_coeff(Dj, g), ej)                     # below n . 2^29 . 64 < 2^49 per term
        num = T - info[b]["delta"][0] - negacyclic(info[b]["delta"][1], s_nat)
        assert (num % P == 0).all(), b
        quo = num // P
        assert ((y2 - rotated) == quo.astype(object)).all(), b
        print(f"{n} x {npr}, record {b}: max |key-switch term of the sum of two rotations| = {int(np.abs(quo).max())}")


@pytest.mark.parametrize("shape", KEYED_SHAPES, ids=SHAPE_IDS)
def test_moving_sum_end_to_end_at_the_fresh_scale(env, keyed_cases, shape):
    """Test 8 (a): encrypt -> ct_drop_primes -> ONE ct_galois_sum_sp (steps 1 .. 7, add_input) -> decrypt_level(np - 1,
    Delta) on B = 4 records with slot values in [-1, 1]: the stage equals its definition, the decode equals the oracle's
    on the output records bit for bit, and the slots are within the reference's 0.1 of the rolled sum, asserted on the
    expectation first (tools/ct_keyswitch_sp_noise_sim.py admits both shapes).  The worst error is printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    L = npr - 1
    lo = Oracle(n, L)
    vals = c["vals"]["unit"]
    l0, l1 = c["dropped"]["unit"]
    elts = [c["key_of"][s][0] for s in WINDOW]
    keys = [c["key_of"][s][1] for s in WINDOW]
    g0, g1 = run_sum_sp(env, ctx, dev_t(env, l0), dev_t(env, l1), elts, L, True)
    e0, e1, _ = hoist_sp_expect(o, l0, l1, elts, keys, w0=1)
    assert (g0 == e0).all() and (g1 == e1).all()
    want = sum(np.roll(vals.astype(np.float64), -s, axis=1) for s in (0,) + WINDOW)
    check_level_decrypt(env, ctx, lo, g0, g1, c["s_hat"], L, o.scale, want, "moving sum of 8 at the fresh scale")


@pytest.mark.parametrize("shape", KEYED_SHAPES, ids=SHAPE_IDS)
def test_matvec_end_to_end_without_a_lift(env, keyed_cases, shape):
    """Test 8 (b): encode_ntt of the eight diagonals of M at Delta -> lintrans_plan_sp -> ONE ct_lintrans_sp on fresh
    dropped records -> ct_rescale -> decrypt_level(np - 2, Delta^2 / q_{np-2}) on B = 4 records of 8-periodic slot values
    in [-1, 1]: every stage equals its definition (the encoded diagonals equal the oracle's), the decode equals the
    oracle's bit for bit, and the slots are within the reference's 0.1 of M x, on the expectation first.  The worst error
    is printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    L = npr - 1
    lo, lo1 = Oracle(n, L), Oracle(n, L - 1)
    vals = c["vals"]["tiled"]
    l0, l1 = c["dropped"]["tiled"]
    elts = [c["key_of"][s][0] for s in WINDOW]
    keys = [c["key_of"][s][1] for s in WINDOW]
    M = matrix(DIM)
    diag = encode_diagonals(env, ctx, o, matrix_diagonals(M, n))
    t_diag = dev_t(env, diag)
    plan = ctx.lintrans_plan_sp(elts, t_diag[1:].contiguous(), t_diag[0].contiguous())
    g0, g1 = run_lintrans_sp(env, ctx, plan, dev_t(env, l0), dev_t(env, l1), L)
    plan.close()
    e0, e1, _ = hoist_sp_expect(o, l0, l1, elts, keys, diag[1:], diag[0])
    assert (g0 == e0).all() and (g1 == e1).all(), "plan call"
    f0, f1 = rescale_records(env, ctx, lo, g0, g1, L)
    scale = o.scale * o.scale / o.q[L - 1]
    want_slots = np.tile(vals.astype(np.float64)[:, :DIM] @ M.T, (1, n // 2 // DIM))
    check_level_decrypt(env, ctx, lo1, f0, f1, c["s_hat"], L - 1, scale, want_slots, "M x on fresh records")


# ---- tests 6 and 7: installs, kinds and arguments -------------------------------------------------------------------
def test_sp_hoist_installs_and_kinds(env):
    """Test 6: with only digit keys installed the sum entry and lintrans_create_sp are SE_ERR_NO_KEY (*out stays NULL);
    an element missing from the special-prime set is SE_ERR_NO_KEY with the element named; a digit plan passed to the new
    execute entry and a special-prime plan passed to se_amd_ct_lintrans_device are -22, as is a plan of another context,
    and the sentinels are intact; se_amd_lintrans_destroy(NULL) is a no-op."""
    torch, pkg = env["torch"], env["pkg"]
    n, npr, B = 4096, 3, 2
    ctx, other = pkg.Context(n, npr), pkg.Context(n, npr)
    L, h = ctx.L, ctx.h
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    diag = torch.ones((2, npr, n), dtype=torch.int32, device=env["dev"])
    diag0 = torch.ones((npr, n), dtype=torch.int32, device=env["dev"])
    s = stream_of(env)
    good, nokey = np.array([3, 9], dtype=np.uint32), np.array([3, 5], dtype=np.uint32)
    mk = dict(ctx=h, elts=hptr(good), G=2, diag=dptr(diag), diag0=dptr(diag0), pt_primes=npr, out=None)
    mk_digit, mk_sp = CEntry(L.se_amd_lintrans_create, **mk), CEntry(L.se_amd_lintrans_create_sp, **mk)
    fs = CEntry(L.se_amd_ct_galois_sum_sp_device, ctx=h, c0=dptr(c0), c1=dptr(c1), B=B, primes=2, elts=hptr(good), G=2,
                add_input=1, out0=dptr(out0), out1=dptr(out1), stream=s)
    dkey = np.zeros((2, 2 * npr, npr, n), dtype=np.uint32)
    ctx.set_galois_keys([3, 9], dkey, dkey)
    assert fs() == SE_ERR_NO_KEY
    creates_refused(mk_sp, [{}], SE_ERR_NO_KEY)
    key = np.zeros((2, npr - 1, npr, n), dtype=np.uint32)
    ctx.set_galois_keys_sp([3, 9], key, key)
    other.set_galois_keys_sp([3, 9], key, key)
    assert fs(elts=hptr(nokey)) == SE_ERR_NO_KEY
    assert "special-prime" in L.se_amd_last_error().decode() and "element 5" in L.se_amd_last_error().decode()
    creates_refused(mk_sp, [dict(elts=hptr(nokey))], SE_ERR_NO_KEY)
    assert "element 5" in L.se_amd_last_error().decode(), L.se_amd_last_error()
    rc, digit = create_handle(mk_digit)
    assert rc == 0 and digit.value
    rc, sp = create_handle(mk_sp)
    assert rc == 0 and sp.value
    rc, foreign = create_handle(mk_sp, ctx=other.h)
    assert rc == 0 and foreign.value
    run = dict(ctx=h, plan=None, c0=dptr(c0), c1=dptr(c1), B=B, primes=2, out0=dptr(out0), out1=dptr(out1), stream=s)
    fd, fp = CEntry(L.se_amd_ct_lintrans_device, **run), CEntry(L.se_amd_ct_lintrans_sp_device, **run)
    fp.refused([dict(plan=digit)])
    fd.refused([dict(plan=sp)])
    fp.refused([dict(plan=foreign), dict(ctx=other.h, plan=sp)])
    assert_untouched(out0, out1)
    # each plan serves the entry of its kind: zero keys and zero slabs give zero rows
    for f, pl in ((fd, digit), (fp, sp)):
        out0.fill_(SENTINEL)
        out1.fill_(SENTINEL)
        assert f(plan=pl) == 0
        for o in (out0, out1):
            assert_zero_prefix(o, B * 2 * n)
    L.se_amd_lintrans_destroy(None)
    for pl in (digit, sp, foreign):
        L.se_amd_lintrans_destroy(pl)
    ctx.close()
    other.close()


def test_sp_hoist_arguments(env):
    """Test 7: every argument error returns -22 and writes nothing: NULL pointers, each alignment, B = 2^32, primes 0, np
    and np + 1, elts NULL, G = 0 and 65, an even element, an element >= 2n, pt_primes other than np, and all three
    entries on a context of one prime.  B = 0 returns 0; a level-1 call writes B . n words and nothing behind them."""
    torch, pkg = env["torch"], env["pkg"]
    n, npr, B = 4096, 3, 2
    ctx = pkg.Context(n, npr)
    L, h = ctx.L, ctx.h
    key = np.zeros((2, npr - 1, npr, n), dtype=np.uint32)
    ctx.set_galois_keys_sp([3, 9], key, key)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    diag = torch.ones((2, npr, n), dtype=torch.int32, device=env["dev"])
    diag0 = torch.ones((npr, n), dtype=torch.int32, device=env["dev"])
    s = stream_of(env)
    el = lambda *g: np.array(g + (0,) * (65 - len(g)), dtype=np.uint32)     # room for the G = 65 call
    good, even, big = el(3, 9), el(3, 4), el(3, 2 * n + 1)
    fs = CEntry(L.se_amd_ct_galois_sum_sp_device, ctx=h, c0=dptr(c0), c1=dptr(c1), B=B, primes=2, elts=hptr(good), G=2,
                add_input=1, out0=dptr(out0), out1=dptr(out1), stream=s)
    fs.refused([
        dict(ctx=None),
        dict(c0=NULL),                                               # NULL mandatory pointers
        dict(c1=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(primes=0),                                              # primes outside [1, np - 1]
        dict(primes=npr),                                            # primes = np: the special prime is not data
        dict(primes=npr + 1),
        dict(B=2 ** 32),                                             # B >= 2^32
        dict(c0=dptr(c0, 4)),                                        # alignment, each slab
        dict(c1=dptr(c1, 8)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
        dict(elts=NULL),                                             # elts NULL, G = 0, G = 65
        dict(G=0),
        dict(G=65),
        dict(elts=hptr(even)),                                       # an even element, one >= 2n
        dict(elts=hptr(big)),
    ])
    fc = CEntry(L.se_amd_lintrans_create_sp, ctx=h, elts=hptr(good), G=2, diag=dptr(diag), diag0=dptr(diag0),
                pt_primes=npr, out=None)
    creates_refused(fc, [
        dict(ctx=None),
        dict(elts=NULL),                                     # NULL elts, d_diag
        dict(diag=NULL),
        dict(G=0),                                           # G = 0, G = 65
        dict(G=65),
        dict(pt_primes=0),                                   # pt_primes must be np
        dict(pt_primes=npr - 1),
        dict(pt_primes=npr + 1),
        dict(elts=hptr(even)),                               # an even element, one >= 2n
        dict(elts=hptr(big)),
        dict(diag=dptr(diag, 4)),                            # alignment of either diagonal pointer
        dict(diag0=dptr(diag0, 8)),
    ])
    assert create_handle(fc, out=None)[0] == SE_ERR_INVALD_ARGUMENT                       # NULL out
    rc, plan = create_handle(fc)
    assert rc == 0 and plan.value
    fp = CEntry(L.se_amd_ct_lintrans_sp_device, ctx=h, plan=plan, c0=dptr(c0), c1=dptr(c1), B=B, primes=2,
                out0=dptr(out0), out1=dptr(out1), stream=s)
    fp.refused([
        dict(ctx=None),
        dict(c0=NULL),                                       # NULL slab pointers
        dict(c1=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(primes=0),                                      # primes outside [1, np - 1]
        dict(primes=npr),
        dict(primes=npr + 1),
        dict(B=2 ** 32),                                     # B >= 2^32
        dict(c0=dptr(c0, 4)),                                # alignment, each slab
        dict(c1=dptr(c1, 8)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
        dict(plan=NULL),                                     # no plan
    ])
    assert fs(B=0) == 0
    assert fp(B=0) == 0
    # a context of one prime has no prime to reserve
    one = pkg.Context(1024, 1)
    fs.refused([dict(ctx=one.h, primes=1)])
    creates_refused(fc, [dict(ctx=one.h, pt_primes=1)])
    fp.refused([dict(ctx=one.h, primes=1)])
    one.close()
    assert_untouched(out0, out1)
    for f in (fs, fp):
        out0.fill_(SENTINEL)
        out1.fill_(SENTINEL)
        assert f(primes=1) == 0
        for o in (out0, out1):
            assert_zero_prefix(o, B * n)
    L.se_amd_lintrans_destroy(plan)
    ctx.close()


# ---- test 9: the example --------------------------------------------------------------------------------------------
def test_matvec_fresh_example(env, tmp_path):
    """examples/matvec_fresh_roundtrip.c from plain gcc: encrypt, drop to np - 1, the diagonals of M encoded at Delta and
    folded into a special-prime plan, ONE se_amd_ct_lintrans_sp_device call, rescale and decrypt_level come back within the
    reference's 0.1 of M x."""
    run_example("matvec_fresh_roundtrip", tmp_path, ("4096", "3", "8"))
