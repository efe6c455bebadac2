"""Baby-step / giant-step transforms on the special-prime keys with the division by P deferred (-m gpu):
se_amd_ct_galois_many_ext_sp_device, se_amd_ct_mul_plain_sum_ext_sp_device, se_amd_ct_mod_down_sp_device,
se_amd_ct_galois_accum_sp_device, se_amd_bsgs_create_sp and se_amd_ct_bsgs_sp_device.
Every expectation is the definition in tests/ct_model_bsgs_sp.py (and tests/ct_model.py for the entries that exist): the
oracle's primitives and Python / NumPy integers, never the code under test.  Every comparison is bit-exact except the
reference's own acceptance criterion |values - expected| < 0.1.
Oracle(n, L) is the oracle of a level-L record of Oracle(n, np): the default chains are prefixes of one another."""
import numpy as np
import pytest

from ct_model import (CASE_IDS, SHAPE_IDS, SP_CASES, add_mod, edge_diagonals, edge_row, galois_sp_expect, matrix,
                      matrix_diagonals, rand_key, rand_slab)
from ct_model_bsgs_sp import (accum_sp_expect, bsgs_sp_expect, ext_primes, many_ext_expect, mod_down_expect,
                              stack_sum_ext_expect)
from gpu_support import (NULL, SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched,  # noqa: F401
                         assert_zero_prefix, check_level_decrypt, create_handle, creates_refused, dev_t, dptr,
                         drop_records, encode_diagonals, env, fresh_records, guarded_pair, host_u32, hptr,
                         install_galois_keys, keyed_cases, periodic_values, rescale_records, run_example, run_galois_sp,
                         sentinel_out, step_elements, stream_of, take)

pytestmark = pytest.mark.gpu


# ---- one call each, outputs backed by sentinels ---------------------------------------------------------------------
def run_many_ext(env, ctx, c0, c1, elts, L):
    return guarded_pair(env, ctx.n, (len(elts), c0.shape[0], L + 1, ctx.n), "many_ext",
                        lambda a, b: ctx.ct_galois_many_ext_sp(c0, c1, elts, a, b, primes=L))


def run_sum_ext(env, ctx, in0, in1, pt, L):
    return guarded_pair(env, ctx.n, (pt.shape[0], in0.shape[1], L + 1, ctx.n), "sum_ext",
                        lambda a, b: ctx.ct_mul_plain_sum_ext_sp(in0, pt, a, in1, b, primes=L))


def run_mod_down(env, ctx, in0, in1, L):
    lead = tuple(in0.shape[:-2])
    return guarded_pair(env, ctx.n, lead + (L, ctx.n), "mod_down",
                        lambda a, b: ctx.ct_mod_down_sp(in0, a, in1, b, primes=L))


def run_accum_sp(env, ctx, in0, in1, elts, L):
    return guarded_pair(env, ctx.n, (in0.shape[1], L, ctx.n), "accum_sp",
                        lambda a, b: ctx.ct_galois_accum_sp(in0, in1, elts, a, b, primes=L))


def run_bsgs_sp(env, ctx, plan, c0, c1, L, records):
    """One plan call with a workspace for `records` records; the words behind the workspace must stay untouched."""
    ws_bytes = ctx.bsgs_workspace_bytes(plan, records, L)
    assert ws_bytes % 16 == 0 and ws_bytes > 0
    ws = sentinel_out(env, ws_bytes // 4, 2 * ctx.n)
    out = guarded_pair(env, ctx.n, (c0.shape[0], L, ctx.n), "bsgs_sp",
                       lambda a, b: ctx.ct_bsgs_sp(plan, c0, c1, a, b, ws, primes=L, workspace_bytes=ws_bytes))
    assert (host_u32(ws)[ws_bytes // 4:] == SENTINEL).all(), "words behind the workspace are written"
    return out


def key_elements(n):
    """The installed elements of a case; the reduced list above 4096, as the sibling modules do."""
    return [3, n + 1] if n > 4096 else [3, 9, 27, n + 1, 2 * n - 1]


@pytest.fixture(scope="module")
def slab_cases(env):
    """slab_cases(shape, levels, B) -> per shape, computed once: a context without a secret key, random special-prime
    Galois keys of key_elements(n) installed (key words 0, 1 and q - 1 on a data column and on column p), and per level the
    slabs: record 0 of c1 holds the centring edge rows 0, 1, (q - 1)/2, (q + 1)/2, q - 1, record 1 is all q_j - 1."""
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
        rng = np.random.default_rng(47 * n + npr)
        elts = key_elements(n)
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
                c1[0, j] = edge_row(o, j, rng, [3, n + 1], edges="centring")
            c0[1] = c1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
            slabs[L] = (c0, c1)
        cache[shape] = dict(o=o, ctx=ctx, elts=elts, keys={g: (gk0[k], gk1[k]) for k, g in enumerate(elts)},
                            slabs=slabs, rng=rng)
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()


def ext_slab(rng, o, lead, L):
    """Random extended records [*lead][L+1][n]: rows r < L below q_r, row L below P."""
    rows = [rng.integers(0, o.q[i], tuple(lead) + (o.n,), dtype=np.uint32) for i in ext_primes(o, L)]
    return np.ascontiguousarray(np.stack(rows, axis=len(lead)))


# ---- the undivided baby steps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,levels,B", SP_CASES, ids=CASE_IDS)
def test_many_ext_matches_the_definition(env, slab_cases, shape, levels, B):
    """Arbitrary slabs and keys, record 0 of c1 on the centring edges, record 1 all q - 1; the element lists [3],
    [3, n + 1, 3] (three elements: two groups, the last one short) and [1, 2n - 1] (the reduced list [3, n + 1, 3] above
    4096) against the definition, at every level of the case.  L below np - 1 is where row L is not prime L."""
    case = slab_cases(shape, levels, B)
    n, npr = shape
    o, ctx = case["o"], case["ctx"]
    lists = [[3, n + 1, 3]] if n > 4096 else [[3], [3, n + 1, 3], [1, 2 * n - 1]]
    for L in levels:
        c0, c1 = case["slabs"][L]
        d0, d1 = dev_t(env, c0), dev_t(env, c1)
        for elts in lists:
            e0, e1 = many_ext_expect(env["pkg"].galois_table, o, c0, c1, elts, case["keys"])
            g0, g1 = run_many_ext(env, ctx, d0, d1, elts, L)
            assert (g0 == e0).all() and (g1 == e1).all(), (L, elts)


def test_many_ext_saturation(env):
    """4096 x 2, L = 1, G = 64: every key word and every record word at q - 1 resp. P - 1, 64 distinct elements (32
    groups).  The lazy accumulators and the (P mod q) . c0 product at their largest."""
    from oracle.pyoracle import Oracle
    n, npr, L, B = 4096, 2, 1, 2
    o = Oracle(n, npr)
    q = o.q
    ctx = env["pkg"].Context(n, npr)
    elts = [2 * k + 3 for k in range(64)]
    key = np.zeros((64, npr - 1, npr, n), dtype=np.uint32)
    key[:] = (np.array(q, dtype=np.uint32) - 1)[None, None, :, None]
    ctx.set_galois_keys_sp(elts, key, key)
    c = np.full((B, L, n), q[0] - 1, dtype=np.uint32)
    e0, e1 = many_ext_expect(env["pkg"].galois_table, o, c, c, elts, {g: (key[0], key[0]) for g in elts})
    g0, g1 = run_many_ext(env, ctx, dev_t(env, c), dev_t(env, c), elts, L)
    assert (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


# ---- the weighted sum on extended records ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,levels,B", SP_CASES, ids=CASE_IDS)
def test_sum_ext_matches_the_definition(env, slab_cases, shape, levels, B):
    """E, Gout = 3, 2 on random extended stacks, plaintexts of arbitrary 32-bit words with 0, 1, q - 1, q and 2^32 - 1 on
    every row, the row at P among them.  At L = np - 1 the bytes are those of ct_mul_plain_sum with primes = np."""
    case = slab_cases(shape, levels, B)
    n, npr = shape
    o, ctx, rng = case["o"], case["ctx"], case["rng"]
    E, Gout = 3, 2
    pt = edge_diagonals(rng, o.q, Gout * E, n).reshape(Gout, E, npr, n)
    t_pt = dev_t(env, pt)
    for L in levels:
        s0, s1 = ext_slab(rng, o, (E, B), L), ext_slab(rng, o, (E, B), L)
        d0, d1 = dev_t(env, s0), dev_t(env, s1)
        g0, g1 = run_sum_ext(env, ctx, d0, d1, t_pt, L)
        assert (g0 == stack_sum_ext_expect(o, s0, pt)).all() and (g1 == stack_sum_ext_expect(o, s1, pt)).all(), L
        if L == npr - 1:
            p0, p1 = guarded_pair(env, n, (Gout, B, npr, n), "sum",
                                  lambda a, b: ctx.ct_mul_plain_sum(d0, t_pt, a, d1, b, primes=npr))
            assert (g0 == p0).all() and (g1 == p1).all()


def test_sum_ext_saturation(env):
    """4096 x 3 at L = 1: E = 64 with every record word at q_r - 1 resp. P - 1 and every plaintext word the same."""
    from oracle.pyoracle import Oracle
    n, npr, L, B, E = 4096, 3, 1, 3, 64
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    top = np.array(o.q, dtype=np.uint32) - 1
    stack = np.zeros((E, B, L + 1, n), dtype=np.uint32)
    stack[:] = top[ext_primes(o, L)][None, None, :, None]
    pt = np.zeros((1, E, npr, n), dtype=np.uint32)
    pt[:] = top[None, None, :, None]
    g0, g1 = run_sum_ext(env, ctx, dev_t(env, stack), dev_t(env, stack), dev_t(env, pt), L)
    want = stack_sum_ext_expect(o, stack, pt)
    assert (g0 == want).all() and (g1 == want).all()
    ctx.close()


# ---- the division by the special prime ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,levels,B", SP_CASES, ids=CASE_IDS)
def test_mod_down_matches_the_definition(env, slab_cases, shape, levels, B):
    """Random extended records; record 0's row at P is the oracle's NTT of coefficients that hold 0, 1, (P - 1)/2, (P + 1)/2
    and P - 1 -- both sides of the centring edge -- at the start, the middle and the end.  One slab and two.  At L = np - 1
    the bytes are those of ct_rescale with primes = np."""
    case = slab_cases(shape, levels, B)
    n, npr = shape
    o, ctx, rng = case["o"], case["ctx"], case["rng"]
    p = npr - 1
    P = o.q[p]
    edges = np.array([0, 1, (P - 1) // 2, (P + 1) // 2, P - 1], dtype=np.uint32)
    for L in levels:
        x0, x1 = ext_slab(rng, o, (B,), L), ext_slab(rng, o, (B,), L)
        coeff = rng.integers(2, P - 1, n, dtype=np.uint32)
        for at in (0, n // 2, n - 5):
            coeff[at:at + 5] = edges
        x0[0, L] = o.ntt(coeff, p)
        assert (o.intt(x0[0, L], p) == coeff).all()
        d0, d1 = dev_t(env, x0), dev_t(env, x1)
        g0, g1 = run_mod_down(env, ctx, d0, d1, L)
        assert (g0 == mod_down_expect(o, x0)).all() and (g1 == mod_down_expect(o, x1)).all(), L
        words = B * L * n
        single = sentinel_out(env, words, 2 * n)
        ctx.ct_mod_down_sp(d0, single, primes=L)
        env["torch"].cuda.synchronize()
        assert (take(single, words, (B, L, n), "one slab") == g0).all()
        if L == npr - 1:
            r0, r1 = guarded_pair(env, n, (B, L, n), "rescale", lambda a, b: ctx.ct_rescale(d0, a, d1, b, primes=npr))
            assert (g0 == r0).all() and (g1 == r1).all()


# ---- the one-division giant sum -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,levels,B", SP_CASES, ids=CASE_IDS)
def test_accum_sp_matches_the_definition(env, slab_cases, shape, levels, B):
    """G different records (the case's slab, with its edge rows, among random ones) under [3, n + 1], [1, 3, 3] and [1]
    ([3, n + 1] alone above 4096) against the definition; G = 1 has the bytes of ct_galois_sp."""
    case = slab_cases(shape, levels, B)
    n, npr = shape
    o, ctx, rng = case["o"], case["ctx"], case["rng"]
    lists = [[3, n + 1]] if n > 4096 else [[3, n + 1], [1, 3, 3], [1]]
    for L in levels:
        c0, c1 = case["slabs"][L]
        for elts in lists:
            G = len(elts)
            in0 = np.stack([c0] + [rand_slab(rng, o.q, B, n, L) for _ in range(G - 1)])
            in1 = np.stack([c1] + [rand_slab(rng, o.q, B, n, L) for _ in range(G - 1)])
            e0, e1 = accum_sp_expect(o, in0, in1, elts, case["keys"])
            g0, g1 = run_accum_sp(env, ctx, dev_t(env, in0), dev_t(env, in1), elts, L)
            assert (g0 == e0).all() and (g1 == e1).all(), (L, elts)
        d0, d1 = dev_t(env, c0), dev_t(env, c1)
        s0, s1 = run_galois_sp(env, ctx, d0, d1, 3, L)
        a0, a1 = run_accum_sp(env, ctx, d0[None].contiguous(), d1[None].contiguous(), [3], L)
        assert (a0 == s0).all() and (a1 == s1).all(), L


def test_accum_sp_rounds_once(env, slab_cases):
    """4096 x 3, L = 2, G = 2 on random records: the output equals the definition and differs from the device's own sum
    of two ct_galois_sp outputs, which round twice."""
    shape, levels, B = SP_CASES[0]
    case = slab_cases(shape, levels, B)
    n, L = shape[0], 2
    o, ctx = case["o"], case["ctx"]
    rng = np.random.default_rng(83)
    elts = [3, n + 1]
    in0 = np.stack([rand_slab(rng, o.q, B, n, L) for _ in elts])
    in1 = np.stack([rand_slab(rng, o.q, B, n, L) for _ in elts])
    t0, t1 = dev_t(env, in0), dev_t(env, in1)
    g0, g1 = run_accum_sp(env, ctx, t0, t1, elts, L)
    e0, e1 = accum_sp_expect(o, in0, in1, elts, case["keys"])
    assert (g0 == e0).all() and (g1 == e1).all()
    s0, s1 = np.zeros_like(g0), np.zeros_like(g1)
    for k, g in enumerate(elts):
        r0, r1 = run_galois_sp(env, ctx, t0[k].contiguous(), t1[k].contiguous(), g, L)
        w0, w1 = galois_sp_expect(o, in0[k], in1[k], g, *case["keys"][g])
        assert (r0 == w0).all() and (r1 == w1).all()
        for b in range(B):
            s0[b], s1[b] = add_mod(o, s0[b], r0[b]), add_mod(o, s1[b], r1[b])
    assert (g0 != s0).any() and (g1 != s1).any()
    print(f"{int((g0 != s0).sum())} of {g0.size} words of out0 differ from the sum of two single calls")


# ---- the plan -------------------------------------------------------------------------------------------------------
def plan_lists(n):
    """(baby, giant) pairs of a case: 3 x 2 with and without the identity in each list; 2 x 2 above 4096."""
    if n > 4096:
        return [([1, 3], [1, n + 1])]
    return [([1, 3, 9], [1, n + 1]), ([3, 9, 27], [n + 1, 2 * n - 1]), ([9, 1, 3], [2 * n - 1, 1])]


@pytest.mark.parametrize("shape,levels,B", SP_CASES, ids=CASE_IDS)
def test_plan_matches_the_definition_and_the_device_composition(env, slab_cases, shape, levels, B):
    """The plan call against bsgs_sp_expect on diagonals of arbitrary 32-bit words, with a workspace for one record and
    for all of them (the same bytes), and against the four entries composed on the device with the pre-rotated
    diagonals."""
    from ct_model import permute_diagonals
    case = slab_cases(shape, levels, B)
    n, npr = shape
    o, ctx, rng = case["o"], case["ctx"], case["rng"]
    table = env["pkg"].galois_table
    for baby, giant in plan_lists(n):
        n1, n2 = len(baby), len(giant)
        diag = edge_diagonals(rng, o.q, n1 * n2, n).reshape(n2, n1, npr, n)
        plan = ctx.bsgs_plan_sp(baby, giant, dev_t(env, diag))
        t_dp = dev_t(env, permute_diagonals(table, n, diag, giant))
        for L in levels:
            c0, c1 = case["slabs"][L]
            d0, d1 = dev_t(env, c0), dev_t(env, c1)
            assert ctx.bsgs_workspace_bytes(plan, 5, L) == 5 * 2 * ((n1 + n2) * (L + 1) + n2 * L) * n * 4
            e0, e1 = bsgs_sp_expect(table, o, c0, c1, baby, giant, diag, case["keys"])
            g0, g1 = run_bsgs_sp(env, ctx, plan, d0, d1, L, B)
            assert (g0 == e0).all() and (g1 == e1).all(), (L, baby, giant)
            h0, h1 = run_bsgs_sp(env, ctx, plan, d0, d1, L, 1)
            assert (h0 == g0).all() and (h1 == g1).all(), (L, baby, giant, "one record per chunk")
            u0, u1 = run_many_ext(env, ctx, d0, d1, baby, L)
            v0, v1 = run_sum_ext(env, ctx, dev_t(env, u0), dev_t(env, u1), t_dp, L)
            w0, w1 = run_mod_down(env, ctx, dev_t(env, v0), dev_t(env, v1), L)
            k0, k1 = run_accum_sp(env, ctx, dev_t(env, w0), dev_t(env, w1), giant, L)
            assert (k0 == g0).all() and (k1 == g1).all(), (L, baby, giant, "composition")
        plan.close()


def test_plan_with_the_identity_giant_step_has_the_bytes_of_lintrans_sp(env, slab_cases):
    """4096 x 3, both levels: giant = [1] and the same diagonals give the bytes of ct_lintrans_sp, with the record's own
    diagonal (baby holds 1; diag0) and without."""
    shape, levels, B = SP_CASES[0]
    case = slab_cases(shape, levels, B)
    n, npr = shape
    o, ctx, rng = case["o"], case["ctx"], case["rng"]
    diag = edge_diagonals(rng, o.q, 3, n).reshape(1, 3, npr, n)
    t = dev_t(env, diag)
    with0 = ctx.bsgs_plan_sp([1, 3, n + 1], [1], t)
    without = ctx.bsgs_plan_sp([3, n + 1], [1], t[:, 1:].contiguous())
    flat0 = ctx.lintrans_plan_sp([3, n + 1], t[0, 1:].contiguous(), t[0, 0].contiguous())
    flat = ctx.lintrans_plan_sp([3, n + 1], t[0, 1:].contiguous(), None)
    for L in levels:
        c0, c1 = case["slabs"][L]
        d0, d1 = dev_t(env, c0), dev_t(env, c1)
        for bs, fl in ((with0, flat0), (without, flat)):
            g0, g1 = run_bsgs_sp(env, ctx, bs, d0, d1, L, 2)
            f0, f1 = guarded_pair(env, n, (B, L, n), "lintrans_sp",
                                  lambda a, b: ctx.ct_lintrans_sp(fl, d0, d1, a, b, primes=L))
            assert (g0 == f0).all() and (g1 == f1).all(), L
    for pl in (with0, without, flat0, flat):
        pl.close()


def test_plan_reads_the_keys_at_call_time_and_kinds_are_refused(env):
    """A plan is made without any key installed; the call is SE_ERR_NO_KEY naming the element, also with the DIGIT key of
    that element installed; after set_galois_keys_sp it succeeds and equals the definition.  A digit plan passed to the
    special-prime entry and a special-prime plan passed to se_amd_ct_bsgs_device are -22, as is a plan of another
    context; nothing is written."""
    from oracle.pyoracle import Oracle
    torch, pkg = env["torch"], env["pkg"]
    n, npr, L, B = 4096, 3, 1, 2
    o = Oracle(n, npr)
    ctx, other = pkg.Context(n, npr), pkg.Context(n, npr)
    lib, h = ctx.L, ctx.h
    rng = np.random.default_rng(97)
    baby, giant = [1, 3], [1, 9]
    diag = edge_diagonals(rng, o.q, 4, n).reshape(2, 2, npr, n)
    t_diag = dev_t(env, diag)
    plan = ctx.bsgs_plan_sp(baby, giant, t_diag)
    digit = ctx.bsgs_plan(baby, giant, t_diag)
    foreign = other.bsgs_plan_sp(baby, giant, t_diag)
    c0, c1 = rand_slab(rng, o.q, B, n, L), rand_slab(rng, o.q, B, n, L)
    d0, d1 = dev_t(env, c0), dev_t(env, c1)
    out0 = torch.full((B, L, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    ws_bytes = ctx.bsgs_workspace_bytes(plan, B, L)
    assert ws_bytes >= ctx.bsgs_workspace_bytes(digit, B, L) > 0
    ws = torch.full((ws_bytes // 4,), SENTINEL, dtype=torch.int32, device=env["dev"])
    run = dict(ctx=h, plan=plan.h, c0=dptr(d0), c1=dptr(d1), B=B, primes=L, out0=dptr(out0), out1=dptr(out1),
               workspace=dptr(ws), bytes=ws_bytes, stream=stream_of(env))
    fd, fp = CEntry(lib.se_amd_ct_bsgs_device, **run), CEntry(lib.se_amd_ct_bsgs_sp_device, **run)
    assert fp() == SE_ERR_NO_KEY
    assert "special-prime" in lib.se_amd_last_error().decode() and "element 3" in lib.se_amd_last_error().decode()
    dkey = np.zeros((2, 2 * npr, npr, n), dtype=np.uint32)
    ctx.set_galois_keys([3, 9], dkey, dkey)
    assert fp() == SE_ERR_NO_KEY                                   # an installed digit key does not serve
    keys = {g: (rand_key(rng, o.q, n), rand_key(rng, o.q, n)) for g in (3, 9)}
    ctx.set_galois_keys_sp([3], keys[3][0][None], keys[3][1][None])
    assert fp() == SE_ERR_NO_KEY and "element 9" in lib.se_amd_last_error().decode()
    ctx.set_galois_keys_sp([3, 9], np.stack([keys[3][0], keys[9][0]]), np.stack([keys[3][1], keys[9][1]]))
    other.set_galois_keys_sp([3, 9], np.stack([keys[3][0], keys[9][0]]), np.stack([keys[3][1], keys[9][1]]))
    fp.refused([dict(plan=digit.h)])                               # each entry refuses the other kind's plan
    fd.refused([dict(plan=plan.h)])
    fp.refused([dict(plan=foreign.h), dict(ctx=other.h)])          # and a plan of another context
    assert_untouched(out0, out1, ws)
    g0, g1 = run_bsgs_sp(env, ctx, plan, d0, d1, L, B)
    e0, e1 = bsgs_sp_expect(pkg.galois_table, o, c0, c1, baby, giant, diag, keys)
    assert (g0 == e0).all() and (g1 == e1).all()
    assert fd(plan=digit.h) == 0                                   # the digit plan still serves its own entry
    torch.cuda.synchronize()
    for pl in (plan, digit, foreign):
        pl.close()
    ctx.close()
    other.close()


# ---- arguments ------------------------------------------------------------------------------------------------------
def test_bsgs_sp_arguments(env):
    """Every argument error returns -22 and writes nothing: a NULL context, NULL pointers, each alignment, B = 2^32,
    primes 0, np and np + 1, elts NULL, G = 0 and 65, an even element, an element >= 2n, G . B, E . B and Gout . B at
    2^32, E and Gout 0 and 65, count 2^31, one of d_in1 / d_out1 alone, pt_primes other than np, a repeated element in
    a plan list, a NULL, misaligned or short workspace, and every entry on a context of one prime.  B = 0 returns 0."""
    torch, pkg = env["torch"], env["pkg"]
    n, npr, B = 4096, 3, 2
    ctx = pkg.Context(n, npr)
    lib, h = ctx.L, ctx.h
    key = np.zeros((2, npr - 1, npr, n), dtype=np.uint32)
    ctx.set_galois_keys_sp([3, 9], key, key)
    big_in = torch.zeros((2, B, npr, n), dtype=torch.int32, device=env["dev"])
    c0 = big_in[0, :, :2].contiguous()
    c1 = torch.zeros_like(c0)
    out0 = torch.full((2 * B * npr * n,), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    ws = torch.full((1 << 20,), SENTINEL, dtype=torch.int32, device=env["dev"])
    diag = torch.ones((2, 2, npr, n), dtype=torch.int32, device=env["dev"])
    s = stream_of(env)
    el = lambda *g: np.array(g + (0,) * (65 - len(g)), dtype=np.uint32)
    good, even, big, twice, nokey = el(3, 9), el(3, 4), el(3, 2 * n + 1), el(3, 3), el(3, 5)
    rot = dict(ctx=h, in0=dptr(c0), in1=dptr(c1), B=B, primes=2, elts=hptr(good), G=2, out0=dptr(out0), out1=dptr(out1),
               stream=s)
    fm = CEntry(lib.se_amd_ct_galois_many_ext_sp_device, **rot)
    fa = CEntry(lib.se_amd_ct_galois_accum_sp_device, **{**rot, "in0": dptr(big_in), "in1": dptr(big_in)})
    for f in (fm, fa):
        f.refused([
            dict(ctx=None),
            dict(in0=NULL), dict(in1=NULL),
            dict(out0=NULL), dict(out1=NULL),
            dict(primes=0), dict(primes=npr), dict(primes=npr + 1),
            dict(B=2 ** 32), dict(B=2 ** 31),                                                     # B, G . B
            dict(in0=dptr(c0, 4)), dict(in1=dptr(c1, 8)),
            dict(out0=dptr(out0, 12)), dict(out1=dptr(out1, 4)),
            dict(elts=NULL), dict(G=0), dict(G=65),
            dict(elts=hptr(even)), dict(elts=hptr(big)),
        ])
        assert f(elts=hptr(nokey)) == SE_ERR_NO_KEY
        assert "element 5" in lib.se_amd_last_error().decode()
        assert f(B=0) == 0
    fs = CEntry(lib.se_amd_ct_mul_plain_sum_ext_sp_device, ctx=h, in0=dptr(big_in), in1=dptr(big_in), E=2, B=B, primes=2,
                pt=dptr(diag), Gout=2, out0=dptr(out0), out1=dptr(out1), stream=s)
    fs.refused([
        dict(ctx=None),
        dict(in0=NULL), dict(pt=NULL), dict(out0=NULL),
        dict(in1=NULL), dict(out1=NULL),                                                       # one of in1 / out1 alone
        dict(primes=0), dict(primes=npr),
        dict(E=0), dict(E=65),
        dict(Gout=0), dict(Gout=65),
        dict(B=2 ** 32), dict(B=2 ** 31, Gout=1),
        dict(E=1, B=2 ** 31),
        dict(in0=dptr(big_in, 4)), dict(pt=dptr(diag, 8)),
        dict(out1=dptr(out1, 4)),
    ])
    assert fs(B=0) == 0
    fd = CEntry(lib.se_amd_ct_mod_down_sp_device, ctx=h, in0=dptr(big_in), in1=dptr(big_in), count=B, primes=2,
                out0=dptr(out0), out1=dptr(out1), stream=s)
    fd.refused([
        dict(ctx=None), dict(in0=NULL), dict(out0=NULL),
        dict(in1=NULL), dict(out1=NULL),
        dict(primes=0), dict(primes=npr), dict(count=2 ** 31),
        dict(in0=dptr(big_in, 4)), dict(out0=dptr(out0, 8)),
    ])
    assert fd(count=0) == 0 and fd(in1=NULL, count=0, out1=NULL) == 0

    fc = CEntry(lib.se_amd_bsgs_create_sp, ctx=h, baby=hptr(good), n1=2, giant=hptr(good), n2=2, diag=dptr(diag),
                pt_primes=npr, out=None)
    creates_refused(fc, [
        dict(ctx=None), dict(baby=NULL), dict(giant=NULL), dict(diag=NULL),
        dict(n1=0), dict(n1=65), dict(n2=0), dict(n2=65),
        dict(pt_primes=0), dict(pt_primes=npr - 1), dict(pt_primes=npr + 1),                    # pt_primes must be np
        dict(baby=hptr(even)), dict(giant=hptr(big)), dict(baby=hptr(twice)),
        dict(diag=dptr(diag, 4)),
    ])
    assert create_handle(fc, out=None)[0] == SE_ERR_INVALD_ARGUMENT
    rc, plan = create_handle(fc)
    assert rc == 0 and plan.value
    per = lib.se_amd_bsgs_workspace_bytes(plan, 1, 2)
    assert per == 2 * ((2 + 2) * 3 + 2 * 2) * n * 4 and lib.se_amd_bsgs_workspace_bytes(None, 1, 2) == 0
    wb = ws.numel() * 4
    assert wb >= 2 * per
    fp = CEntry(lib.se_amd_ct_bsgs_sp_device, ctx=h, plan=plan, c0=dptr(c0), c1=dptr(c1), B=B, primes=2,
                out0=dptr(out0), out1=dptr(out1), workspace=dptr(ws), bytes=wb, stream=s)
    fp.refused([
        dict(ctx=None), dict(plan=NULL),
        dict(c0=NULL), dict(c1=NULL),
        dict(out0=NULL), dict(out1=NULL),
        dict(primes=0), dict(primes=npr),
        dict(B=2 ** 32),
        dict(c0=dptr(c0, 4)), dict(out1=dptr(out1, 8)),
        dict(workspace=NULL), dict(workspace=dptr(ws, 4), bytes=wb - 4),
        dict(bytes=per - 4),
    ])
    assert fp(B=0) == 0
    # a context of one prime has no prime to reserve
    one = pkg.Context(1024, 1)
    for f in (fm, fa, fs, fd):
        f.refused([dict(ctx=one.h, primes=1)])
    creates_refused(fc, [dict(ctx=one.h, pt_primes=1)])
    fp.refused([dict(ctx=one.h, primes=1)])
    one.close()
    assert_untouched(out0, out1, ws)
    # a level-1 call on zero slabs and zero keys writes B . n zero words and nothing behind them
    assert fp(primes=1) == 0
    for o in (out0, out1):
        assert_zero_prefix(o, B * n)
    lib.se_amd_bsgs_destroy(plan)
    ctx.close()


def test_digit_and_special_prime_twins_refuse_in_their_own_order(env):
    """The three pairs of entries that share one host body (ct_galois_accum, ct_galois_sum, ct_mul_plain_sum and their
    special-prime forms) on calls that are wrong in TWO ways at once, B = 1: the code and the last error say which check
    came first.  The expected values are literals read off the two separate bodies each pair had before they were merged.
    A refusal of the call's shape (a slab, the level, an alignment) sets no message, so the last error is seeded before
    every call and must come back unchanged.
      1. a misaligned output slab and an element without an installed key (the key-free pair: and E = 65): the shape
         check comes first on both sides, -22 and no message -- not SE_ERR_NO_KEY, not the stack's message.
      2. a level of np and an even element (the key-free pair: and E = 65): np is a level of the digit side, which goes
         on to refuse the element resp. the stack with its message; the special-prime side stops at the level, silently.
    Nothing is written.  4096 x 2 is the smallest parameter set with a special prime (the chains of 1024 and 2048 have
    one prime)."""
    torch, pkg = env["torch"], env["pkg"]
    n, npr, B = 4096, 2, 1
    ctx = pkg.Context(n, npr)
    lib, h = ctx.L, ctx.h
    ctx.set_galois_keys([3], *(np.zeros((1, 2 * npr, npr, n), dtype=np.uint32),) * 2)
    ctx.set_galois_keys_sp([3], *(np.zeros((1, npr - 1, npr, n), dtype=np.uint32),) * 2)
    stack = torch.zeros((2, B, npr + 1, n), dtype=torch.int32, device=env["dev"])
    pt = torch.ones((1, 2, npr, n), dtype=torch.int32, device=env["dev"])
    out0 = torch.full((2 * B * (npr + 1) * n,), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    s = stream_of(env)
    keyed, keyless, even = (np.array(g, dtype=np.uint32) for g in ([3, 3], [3, 7], [3, 4]))
    SEED = "unsupported parameter set (degree, primes), or primes < 2"
    ELEMENT = "Galois element 4 is not odd and below 2n"
    STACK = "weighted sum over a stack: E and Gout between 1 and 64, E B and Gout B below 2^32"
    # the lists the edits below start from; none is called as it stands
    rot = dict(ctx=h, in0=dptr(stack), in1=dptr(stack), B=B, primes=1, elts=hptr(keyed), G=2, out0=dptr(out0),
               out1=dptr(out1), stream=s)
    tot = dict(ctx=h, in0=dptr(stack), in1=dptr(stack), B=B, primes=1, elts=hptr(keyed), G=2, add_input=0,
               out0=dptr(out0), out1=dptr(out1), stream=s)
    fa, fa_sp = CEntry(lib.se_amd_ct_galois_accum_device, **rot), CEntry(lib.se_amd_ct_galois_accum_sp_device, **rot)
    fg, fg_sp = CEntry(lib.se_amd_ct_galois_sum_device, **tot), CEntry(lib.se_amd_ct_galois_sum_sp_device, **tot)
    fs = CEntry(lib.se_amd_ct_mul_plain_sum_device, ctx=h, in0=dptr(stack), in1=dptr(stack), E=1, B=B, primes=1,
                pt=dptr(pt), Gout=1, pt_primes=npr, out0=dptr(out0), out1=dptr(out1), stream=s)
    fs_sp = CEntry(lib.se_amd_ct_mul_plain_sum_ext_sp_device, ctx=h, in0=dptr(stack), in1=dptr(stack), E=1, B=B, primes=1,
                   pt=dptr(pt), Gout=1, out0=dptr(out0), out1=dptr(out1), stream=s)

    def refused(f, edits, text):
        assert lib.se_amd_rescale_constants(n, 1, None, None) == SE_ERR_INVALD_ARGUMENT      # seeds the last error
        assert lib.se_amd_last_error().decode() == SEED
        f.refused([edits])
        assert lib.se_amd_last_error().decode() == text, (f.fn.__name__, edits)

    # 1. a misaligned output slab in front of everything else
    for f in (fa, fa_sp, fg, fg_sp):
        refused(f, dict(elts=hptr(keyless), out0=dptr(out0, 4)), SEED)
    refused(fs, dict(E=65, out0=dptr(out0, 4)), SEED)
    refused(fs_sp, dict(E=65, out0=dptr(out0, 4)), SEED)
    # 2. the level np: the digit side's highest, above the special-prime side's
    refused(fa, dict(primes=npr, elts=hptr(even)), ELEMENT)
    refused(fa_sp, dict(primes=npr, elts=hptr(even)), SEED)
    refused(fg, dict(primes=npr, elts=hptr(even)), ELEMENT)
    refused(fg_sp, dict(primes=npr, elts=hptr(even)), SEED)
    refused(fs, dict(E=65, primes=npr), STACK)
    refused(fs_sp, dict(E=65, primes=npr), SEED)
    assert_untouched(out0, out1)
    ctx.close()


# ---- end to end with a real key -------------------------------------------------------------------------------------
DIM = 16
N1 = N2 = 4


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: the six special-prime Galois
    keys of the steps 1, 2, 3 and 4, 8, 12, installed; B = 4 fresh symmetric records of 16-periodic slot values in
    [-1, 1], dropped to np - 1 primes."""
    ctx = case["ctx"]
    n, npr = ctx.n, ctx.np
    steps = (1, 2, 3, 4, 8, 12)
    elts = step_elements(env, n, steps)
    gk0, gk1 = install_galois_keys(case, elts, "bsgs-sp-gk", sp=True)
    vals = periodic_values(4, n, DIM, 8000 + n)
    c0, c1 = fresh_records(env, ctx, vals, 480)
    case.update(keys={g: (gk0[k], gk1[k]) for k, g in enumerate(elts)}, vals=vals,
                dropped=drop_records(env, ctx, c0, c1, npr - 1))


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_matvec_bsgs_fresh_end_to_end(env, keyed_cases, shape):
    """encrypt -> ct_drop_primes to np - 1 -> ONE ct_bsgs_sp call (baby steps 0 .. 3, giant steps 0, 4, 8, 12: six
    special-prime keys; the sixteen diagonals of M, entries in [-1/2, 1/2], encoded at Delta on the device) -> ct_rescale ->
    decrypt_level(np - 2, Delta^2 / q_{np-2}) on B = 4 records, no lift.  The plan call equals its definition bit for bit,
    the decode equals the oracle's, and every slot is within the reference's 0.1 of M x, on the expectation first
    (tools/ct_keyswitch_sp_noise_sim.py --bsgs admits both shapes).  The worst error is printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    ctx, o, pkg = c["ctx"], c["o"], env["pkg"]
    n, npr = shape
    L = npr - 1
    lo, lo1 = Oracle(n, L), Oracle(n, L - 1)
    vals = c["vals"]
    l0, l1 = c["dropped"]
    M = matrix(DIM)
    diag = encode_diagonals(env, ctx, o, matrix_diagonals(M, n)).reshape(N2, N1, npr, n)
    baby = [pkg.galois_element(n, b) for b in range(N1)]
    giant = [pkg.galois_element(n, N1 * g) for g in range(N2)]
    assert baby[0] == giant[0] == 1 and len(set(baby + giant)) == N1 + N2 - 1
    plan = ctx.bsgs_plan_sp(baby, giant, dev_t(env, diag))
    g0, g1 = run_bsgs_sp(env, ctx, plan, dev_t(env, l0), dev_t(env, l1), L, 3)          # two chunks, the last one short
    plan.close()
    e0, e1 = bsgs_sp_expect(pkg.galois_table, o, l0, l1, baby, giant, diag, c["keys"])
    assert (g0 == e0).all() and (g1 == e1).all(), "plan call"
    f0, f1 = rescale_records(env, ctx, lo, g0, g1, L)
    scale = o.scale * o.scale / o.q[L - 1]
    want_slots = np.tile(vals.astype(np.float64)[:, :DIM] @ M.T, (1, n // 2 // DIM))
    check_level_decrypt(env, ctx, lo1, f0, f1, c["s_hat"], L - 1, scale, want_slots, "16 x 16 M x on fresh records, 4 x 4")


def test_matvec_bsgs_fresh_example(env, tmp_path):
    """examples/matvec_bsgs_fresh_roundtrip.c from plain gcc: six special-prime keys, drop to np - 1, the sixteen diagonals
    of M at Delta in a 4 x 4 plan, ONE se_amd_ct_bsgs_sp_device call, one rescale and decrypt_level come back within the
    reference's 0.1 of M x."""
    run_example("matvec_bsgs_fresh_roundtrip", tmp_path, ("4096", "3", "4"))
