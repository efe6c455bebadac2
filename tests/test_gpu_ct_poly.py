"""Slot-wise polynomials (-m gpu): se_amd_ct_affine_rescale_device and the plans of se_amd_ct_poly_sp_device.
Every expectation is the definition in tests/ct_model_poly.py on top of tests/ct_model.py and tests/ct_model_dot.py: the
oracle's primitives and Python / NumPy integers, never the code under test.  Every comparison is bit-exact except the
reference's own acceptance criterion |values - expected| < 0.1 (device/test/ckks_tests_common.c:132).
Oracle(n, L) is the oracle of a level-L record of Oracle(n, np): the default chains are prefixes of one another."""
import ctypes as C

import numpy as np
import pytest

from ct_model import centred, galois_seeds, rand_key, rand_slab
from ct_model_poly import affine_rescale_expect, depth, poly_expect, poly_schedule, poly_value, weighted_sum_expect
from gpu_support import (NULL, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched, check_headroom,  # noqa: F401
                         check_level_decrypt, dev_t, dptr, drop_records, env, expectation, fresh_records, guarded_pair,
                         host_u32, hptr, keyed_cases, lift_records, run_example, stream_of, unit_values)

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
LOGISTIC7 = [0.5, 0.25, 0.0, -1.0 / 48, 0.0, 1.0 / 480, 0.0, -17.0 / 80640]


# ---- the runners ----------------------------------------------------------------------------------------------------
def run_affine(env, ctx, terms0, terms1, w, c_after, primes):
    """One ct_affine_rescale call on host term slabs, two rows of sentinels behind each output -> host out0, out1."""
    d0, d1 = [dev_t(env, t) for t in terms0], [dev_t(env, t) for t in terms1]
    return guarded_pair(env, ctx.n, (terms0[0].shape[0], primes - 1, ctx.n), "affine",
                        lambda a, b: ctx.ct_affine_rescale(d0, d1, w, c_after, a, b, primes))


def slab_like(env, B, rows, n):
    return env["torch"].empty((B, rows, n), dtype=env["torch"].int32, device=env["dev"])


def gpu_composition(env, ctx, sched, c0, c1):
    """The schedule run entry by entry on device records [B][L][n]: per needed power above 1 ct_drop_primes of the lower
    operand where it is higher, a one-pair row of ct_dot_sp per record, ct_rescale; then ONE ct_affine_rescale over the
    terms -> (host out0, out1, {power: device pair})."""
    B, n = c0.shape[0], ctx.n
    rp = dev_t(env, np.arange(B + 1, dtype=np.uint32))
    x, lv = {1: (c0, c1)}, sched["levels"]
    for d in sched["powers"]:
        if d == 1:
            continue
        h, m = 1 << (depth(d) - 1), lv[d] + 1
        (a0, a1), (b0, b1) = x[h], x[d - h]
        assert a0.shape[1] == m
        if b0.shape[1] > m:
            t0, t1 = slab_like(env, B, m, n), slab_like(env, B, m, n)
            ctx.ct_drop_primes(b0, t0, b1, t1, primes_in=b0.shape[1], primes_out=m)
            b0, b1 = t0, t1
        p0, p1 = slab_like(env, B, m, n), slab_like(env, B, m, n)
        ctx.ct_dot_sp(a0, a1, b0, b1, rp, None, None, p0, p1, primes=m)
        r0, r1 = slab_like(env, B, m - 1, n), slab_like(env, B, m - 1, n)
        ctx.ct_rescale(p0, r0, p1, r1, primes=m)
        x[d] = (r0, r1)
    ts = sched["terms"]
    out = guarded_pair(env, n, (B, sched["out_primes"], n), "composition", lambda a, b: ctx.ct_affine_rescale(
        [x[d][0] for d in ts], [x[d][1] for d in ts], [sched["weights"][d] for d in ts], sched["c_after"], a, b,
        sched["level"]))
    return out[0], out[1], x


def run_poly(env, ctx, plan, c0, c1):
    """One ct_poly_sp call in a workspace of exactly the bytes the plan asks for, guard words behind it."""
    B = c0.shape[0]
    need = plan.workspace_bytes(B)
    assert need % 16 == 0
    work = env["torch"].full((need // 4 + 64,), SENTINEL, dtype=env["torch"].int32, device=env["dev"])
    out = guarded_pair(env, ctx.n, (B, plan.result()[0], ctx.n), "poly",
                       lambda a, b: ctx.ct_poly_sp(plan, c0, c1, a, b, work, workspace_bytes=need))
    assert bool((work[need // 4:] == SENTINEL).all()), "words behind the workspace are written"
    return out


# ---- tests 1 and 2: the definition on arbitrary slabs ---------------------------------------------------------------
AFFINE_CASES = [((4096, 3), 2, 3, (1, 2, 5, 16)), ((4096, 3), 3, 3, (1, 2, 5, 16)), ((8192, 6), 4, 3, (1, 2, 5, 16)),
                ((16384, 13), 13, 1, (2,))]
AFFINE_IDS = [f"{n}x{npr}-primes{p}" for (n, npr), p, _, _ in AFFINE_CASES]


def term_levels(T, primes, npr):
    """Mixed levels: some equal to `primes`, some larger, up to np."""
    return [primes + t % (npr - primes + 1) if t % 3 else primes for t in range(T)]


@pytest.mark.parametrize("shape,primes,B,Ts", AFFINE_CASES, ids=AFFINE_IDS)
def test_affine_arbitrary_slabs_against_the_model(env, shape, primes, B, Ts):
    """Test 1: random residue slabs at mixed term levels (a wrong record stride reads other rows), weights among 0, 1, -1,
    q_j, q_j - 1, +-(2^62 - 1) and INT64_MIN and random int64, c_after among 0, -1, q_0 and INT64_MAX: both outputs equal
    the model bit for bit and the sentinels behind them survive.  No key is installed."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    o = Oracle(n, npr)
    q = o.q
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(101 * n + primes)
    pool = [0, 1, -1, q[0], q[primes - 1] - 1, 2 ** 62 - 1, -(2 ** 62 - 1), I64_MIN, q[primes - 1], q[0] - 1]
    consts = [0, -1, q[0], I64_MAX]
    for k, T in enumerate(Ts):
        levels = term_levels(T, primes, npr)
        if primes < npr and T > 1:
            assert primes in levels and max(levels) > primes
        terms0 = [rand_slab(rng, q, B, n, lv) for lv in levels]
        terms1 = [rand_slab(rng, q, B, n, lv) for lv in levels]
        w = [pool[(3 * k + t) % len(pool)] if t < len(pool) else int(rng.integers(I64_MIN, I64_MAX)) for t in range(T)]
        if T == 1:
            w = [-(2 ** 62 - 1)]
        c_after = consts[k % len(consts)]
        e0, e1 = affine_rescale_expect(o, terms0, terms1, w, c_after, primes)
        g0, g1 = run_affine(env, ctx, terms0, terms1, w, c_after, primes)
        assert (g0 == e0).all() and (g1 == e1).all(), (T, w, c_after)
    ctx.close()


@pytest.mark.parametrize("shape,primes", [((4096, 3), 3), ((8192, 6), 4)], ids=["4096x3-primes3", "8192x6-primes4"])
def test_affine_all_maximal_words(env, shape, primes):
    """Test 2: T = 16, every residue q_j - 1 and every weight = q_j - 1 mod q_j (the weight -1): sixteen products of
    (q_j - 1)^2, the largest the 64-bit sum of a row may hold before its one reduction (16 (q - 1)^2 < 2^64).  An
    accumulator that reduced a term too late, or kept the sum in fewer bits, fails here."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    levels = term_levels(16, primes, npr)
    top = np.array(o.q, dtype=np.uint32) - 1
    terms = [np.broadcast_to(top[None, :lv, None], (1, lv, n)).copy() for lv in levels]
    w = [-1] * 16
    assert all(16 * (qj - 1) ** 2 < 2 ** 64 < 17 * (qj - 1) ** 2 for qj in o.q[:primes])
    e0, e1 = affine_rescale_expect(o, terms, terms, w, I64_MAX, primes)
    g0, g1 = run_affine(env, ctx, terms, terms, w, I64_MAX, primes)
    assert (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


# ---- test 3: the centring edges lie on the SUM ----------------------------------------------------------------------
def test_affine_centring_edges_of_the_summed_row(env):
    """Test 3 at 4096 x 3, primes = 2, weights (3, -2): two terms whose last rows hold interior coefficients u, v with
    3 u - 2 v = 0, (q - 1)/2, (q + 1)/2 and q - 1 mod q = q_1 on the first four coefficients, on both slabs, so delta of
    the sum is 0, (q - 1)/2, -(q - 1)/2, -1 there, which the model confirms before the device is asked.  A kernel that
    centres per term, or rescales the terms before it sums them, fails here."""
    from oracle.pyoracle import Oracle
    n, npr, primes = 4096, 3, 2
    o = Oracle(n, npr)
    q = o.q[primes - 1]
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(103)
    w = [3, -2]
    targets = np.array([0, (q - 1) // 2, (q + 1) // 2, q - 1], dtype=np.int64)
    edges = {0, 1, (q - 1) // 2, (q + 1) // 2, q - 1}
    u = q // 5 + np.arange(4, dtype=np.int64)
    v = np.array([((3 * int(a) - int(t)) * pow(2, -1, q)) % q for a, t in zip(u, targets)], dtype=np.int64)
    assert not edges & set(u.tolist()) and not edges & set(v.tolist())              # each term is interior
    assert all((3 * int(a) - 2 * int(b)) % q == int(t) for a, b, t in zip(u, v, targets))
    terms = []
    for s in range(2):
        pair = [rand_slab(rng, o.q, 1, n, 2), rand_slab(rng, o.q, 1, n, 3)]
        for term, vals in zip(pair, (u, v)):
            c = o.intt(term[0, primes - 1], primes - 1)
            c[:4] = vals
            term[0, primes - 1] = o.ntt(c, primes - 1)
        terms.append(pair)
    for s in range(2):
        acc = weighted_sum_expect(o, terms[s], w, primes)
        delta = centred(o.intt(acc[0, primes - 1], primes - 1), q)
        assert (delta[:4] == [0, (q - 1) // 2, -(q - 1) // 2, -1]).all()
    e0, e1 = affine_rescale_expect(o, terms[0], terms[1], w, 7, primes)
    g0, g1 = run_affine(env, ctx, terms[0], terms[1], w, 7, primes)
    assert (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


# ---- test 4: the twins on the GPU -----------------------------------------------------------------------------------
def test_affine_equals_drop_lincomb_rescale_and_the_constant(env):
    """Test 4 at 8192 x 6, primes = 4, T = 5 terms at mixed levels, B = 3, weights inside int32: the bits of
    ct_drop_primes per term, ct_lincomb (one CSR row per record over the stacked terms, which it takes as records of np
    rows), ct_rescale of the first `primes` rows of its sums, and c_after mod q_i added to slab 0 on the host."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, primes, T, B = 8192, 6, 4, 5, 3
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(107)
    levels = term_levels(T, primes, npr)
    terms0 = [rand_slab(rng, o.q, B, n, lv) for lv in levels]
    terms1 = [rand_slab(rng, o.q, B, n, lv) for lv in levels]
    w = [2 ** 31 - 1, -2 ** 31, 1, -77, 123456789]
    c_after = -(2 ** 40) - 3
    g0, g1 = run_affine(env, ctx, terms0, terms1, w, c_after, primes)
    # ct_lincomb works on records of np rows: the dropped terms fill rows 0 .. primes - 1 of a zeroed stack of such records
    stack0, stack1 = (torch.zeros((T * B, npr, n), dtype=torch.int32, device=env["dev"]) for _ in range(2))
    for t in range(T):
        t0, t1 = slab_like(env, B, primes, n), slab_like(env, B, primes, n)
        ctx.ct_drop_primes(dev_t(env, terms0[t]), t0, dev_t(env, terms1[t]), t1, primes_in=levels[t], primes_out=primes)
        stack0[t * B:(t + 1) * B, :primes], stack1[t * B:(t + 1) * B, :primes] = t0, t1
    rp = dev_t(env, np.arange(0, T * B + 1, T, dtype=np.uint32))
    idx = dev_t(env, np.array([t * B + b for b in range(B) for t in range(T)], dtype=np.uint32))
    wd = dev_t(env, np.array(w * B, dtype=np.int32))
    f0, f1 = slab_like(env, B, npr, n), slab_like(env, B, npr, n)
    ctx.ct_lincomb(stack0, f0, stack1, f1, row_ptr=rp, idx=idx, w=wd)
    s0, s1 = f0[:, :primes].contiguous(), f1[:, :primes].contiguous()
    r0, r1 = guarded_pair(env, n, (B, primes - 1, n), "rescale", lambda a, b: ctx.ct_rescale(s0, a, s1, b, primes=primes))
    torch.cuda.synchronize()
    for i in range(primes - 1):
        r0[:, i] = ((r0[:, i].astype(np.uint64) + np.uint64(c_after % o.q[i])) % np.uint64(o.q[i])).astype(np.uint32)
    assert g0.tobytes() == r0.tobytes() and g1.tobytes() == r1.tobytes()
    ctx.close()


# ---- test 5: arguments ----------------------------------------------------------------------------------------------
def test_affine_arguments(env):
    """Test 5: every argument error returns -22 and writes nothing: NULL ctx, pointer arrays, term_primes, w and outputs;
    a NULL term pointer in either array; T = 0 and 17; primes outside [2, np]; a term_primes[t] below primes or above np;
    each misaligned device pointer; B = 2^31.  B = 0 is a successful no-op."""
    torch, pkg = env["torch"], env["pkg"]
    n, npr, B, T, primes = 4096, 3, 2, 2, 2
    ctx = pkg.Context(n, npr)
    L = ctx.L
    ta = [torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"]) for _ in range(2)]
    tb = [torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"]) for _ in range(2)]
    out0 = torch.full((B, primes - 1, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    ptrs = lambda *v: (C.c_void_p * len(v))(*v)  # noqa: E731
    p0, p1 = ptrs(ta[0].data_ptr(), ta[1].data_ptr()), ptrs(tb[0].data_ptr(), tb[1].data_ptr())
    many0, many1 = ptrs(*[ta[0].data_ptr()] * 17), ptrs(*[tb[0].data_ptr()] * 17)
    tp, w = np.array([2, 3], dtype=np.uint32), np.array([5, -6], dtype=np.int64)
    tp17, w17 = np.full(17, 3, dtype=np.uint32), np.ones(17, dtype=np.int64)
    low, high = np.array([2, 1], dtype=np.uint32), np.array([4, 2], dtype=np.uint32)
    call = CEntry(L.se_amd_ct_affine_rescale_device, ctx=ctx.h, t0=p0, t1=p1, tp=hptr(tp), w=hptr(w), T=T, c=9, B=B,
                  primes=primes, o0=dptr(out0), o1=dptr(out1), stream=stream_of(env))
    call.refused([
        dict(ctx=None), dict(t0=None), dict(t1=None), dict(tp=None), dict(w=None), dict(o0=NULL), dict(o1=NULL),
        dict(t0=ptrs(ta[0].data_ptr(), None)), dict(t1=ptrs(None, tb[1].data_ptr())),
        dict(T=0), dict(t0=many0, t1=many1, tp=hptr(tp17), w=hptr(w17), T=17),
        dict(primes=1), dict(primes=0), dict(primes=4),
        dict(tp=hptr(low)), dict(tp=hptr(high)), dict(primes=3),             # term 0 has 2 rows: below primes = 3
        dict(t0=ptrs(ta[0].data_ptr() + 4, ta[1].data_ptr())), dict(t1=ptrs(tb[0].data_ptr(), tb[1].data_ptr() + 8)),
        dict(o0=dptr(out0, 12)), dict(o1=dptr(out1, 4)),
        dict(B=2 ** 31)])
    assert call(B=0) == 0
    assert_untouched(out0, out1)
    assert call() == 0 and call(t0=many0, t1=many1, tp=hptr(tp17), w=hptr(w17), T=16, primes=3, B=0) == 0
    torch.cuda.synchronize()
    assert not bool((out0 == SENTINEL).any())
    ctx.close()


# ---- test 6: the plan on arbitrary slabs under an arbitrary installed key -------------------------------------------
PLAN_KINDS = {"3": [0.25, -0.5, 0.75, 1.0], "7odd": LOGISTIC7, "8": [1.0, 0, -0.5, 0, 0.25, 0.125, 0, 0, 2.0]}


@pytest.fixture(scope="module")
def plan_case(env):
    """8192 x 6, L = 5, B = 2: a context with a random special-prime relinearisation key installed (no secret key) and
    random level-5 records, computed once."""
    from oracle.pyoracle import Oracle
    n, npr, L, B = 8192, 6, 5, 2
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(109)
    k0, k1 = rand_key(rng, o.q, n), rand_key(rng, o.q, n)
    ctx.set_relin_key_sp(k0, k1)
    c0, c1 = rand_slab(rng, o.q, B, n, L), rand_slab(rng, o.q, B, n, L)
    yield dict(o=o, ctx=ctx, k0=k0, k1=k1, c0=c0, c1=c1, L=L)
    ctx.close()


@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_plan_equals_the_composition_and_the_model(env, plan_case, kind):
    """Test 6: degrees 3, 7 odd-only and 8 on random records under a random key: ONE ct_poly_sp call has the bits of the
    schedule run entry by entry on the GPU (ct_drop_primes, one-pair ct_dot_sp rows, ct_rescale, ct_affine_rescale) and of
    poly_expect; it stays inside the workspace it asked for."""
    c = plan_case
    o, ctx, L = c["o"], c["ctx"], c["L"]
    coeff = PLAN_KINDS[kind]
    scale_in, scale_out = float(o.q[L - 1]), 2.0 ** 25
    sched = poly_schedule(o.q, L, coeff, scale_in, scale_out)
    plan = env["pkg"].poly_create(ctx.n, ctx.np, L, coeff, scale_in, scale_out)
    assert [t["power"] for t in plan.terms()] == sched["powers"] and plan.result() == (sched["out_primes"], sched["c_after"])
    d0, d1 = dev_t(env, c["c0"]), dev_t(env, c["c1"])
    g0, g1 = run_poly(env, ctx, plan, d0, d1)
    t0, t1, _ = gpu_composition(env, ctx, sched, d0, d1)
    assert g0.tobytes() == t0.tobytes() and g1.tobytes() == t1.tobytes()
    e0, e1, _ = poly_expect(o, c["c0"], c["c1"], sched, c["k0"], c["k1"])
    assert (g0 == e0).all() and (g1 == e1).all()
    plan.close()


def test_plan_arguments(env, plan_case):
    """Test 6, the refusals: NULL ctx, plan, records, outputs and workspace; each misaligned pointer; B = 2^31; a workspace
    one byte short; a context of another shape; all -22 with nothing written.  SE_ERR_NO_KEY on a context that holds
    only a digit relinearisation key.  B = 0 is a successful no-op; a plan of degree 1 needs no workspace."""
    torch, pkg = env["torch"], env["pkg"]
    c = plan_case
    ctx, L = c["ctx"], c["L"]
    n, npr, B = ctx.n, ctx.np, 2
    lib = ctx.L
    plan = pkg.poly_create(n, npr, L, PLAN_KINDS["3"], 2.0 ** 30, 2.0 ** 25)
    need = plan.workspace_bytes(B)
    d0, d1 = dev_t(env, c["c0"]), dev_t(env, c["c1"])
    out0 = torch.full((B, plan.result()[0], n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    work = torch.full((need // 4,), SENTINEL, dtype=torch.int32, device=env["dev"])
    call = CEntry(lib.se_amd_ct_poly_sp_device, ctx=ctx.h, plan=plan.h, c0=dptr(d0), c1=dptr(d1), B=B, work=dptr(work),
                  bytes=need, o0=dptr(out0), o1=dptr(out1), stream=stream_of(env))
    other = pkg.Context(8192, 5)
    bare = pkg.Context(n, npr)
    bare.set_relin_key(np.zeros((2 * npr, npr, n), dtype=np.uint32), np.zeros((2 * npr, npr, n), dtype=np.uint32))
    call.refused([
        dict(ctx=None), dict(plan=None), dict(c0=NULL), dict(c1=NULL), dict(o0=NULL), dict(o1=NULL), dict(work=NULL),
        dict(c0=dptr(d0, 4)), dict(c1=dptr(d1, 8)), dict(o0=dptr(out0, 12)), dict(o1=dptr(out1, 4)),
        dict(work=dptr(work, 4)), dict(B=2 ** 31, bytes=2 ** 62), dict(bytes=need - 1), dict(bytes=0),
        dict(ctx=other.h)])
    call.refused([dict(ctx=bare.h), dict(ctx=bare.h, B=0)], SE_ERR_NO_KEY)
    assert call(B=0) == 0
    assert_untouched(out0, out1, work)
    one = pkg.poly_create(n, npr, L, [0.5, 0.25], 2.0 ** 30, 2.0 ** 25)
    assert one.workspace_bytes(B) == 0 and one.result()[0] == L - 1
    big0 = torch.full((B, L - 1, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    big1 = torch.full_like(big0, SENTINEL)
    assert call(plan=one.h, work=NULL, bytes=0, o0=dptr(big0), o1=dptr(big1)) == 0
    torch.cuda.synchronize()
    sched = poly_schedule(c["o"].q, L, [0.5, 0.25], 2.0 ** 30, 2.0 ** 25)
    e0, e1 = affine_rescale_expect(c["o"], [c["c0"]], [c["c1"]], [sched["weights"][1]], sched["c_after"], L)
    assert (host_u32(big0) == e0).all() and (host_u32(big1) == e1).all()
    for x in (plan, one, other, bare):
        x.close()


# ---- tests 7 and 8: real keys ---------------------------------------------------------------------------------------
E2E = {(8192, 6): dict(L=5, B=2), (16384, 13): dict(L=12, B=1)}


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: the special-prime
    relinearisation key, generated on the device and installed; B records of unit_values encrypted fresh, lifted by ONE
    ct_lincomb with the weight round(q_{L-1} / Delta) so that scale_in = weight . Delta is about q, and dropped to L."""
    ctx, o = case["ctx"], case["o"]
    n, npr = ctx.n, ctx.np
    L, B = E2E[(n, npr)]["L"], E2E[(n, npr)]["B"]
    evk0, evk1 = ctx.gen_relin_key_sp(case["sk"], *galois_seeds(npr, 1, "poly-relin-e2e", sp=True))
    ctx.set_relin_key_sp(evk0, evk1)
    vals = unit_values(B, n, 9000 + n)
    weight = round(o.q[L - 1] / o.scale)
    l0, l1 = lift_records(env, ctx, o, fresh_records(env, ctx, vals, 600), weight)
    case.update(evk0=evk0, evk1=evk1, vals=vals, L=L, scale_in=float(weight) * o.scale,
                dropped=drop_records(env, ctx, dev_t(env, l0), dev_t(env, l1), L))


def test_logistic_activation_end_to_end(env, keyed_cases):
    """Test 7 at 8192 x 6: records of unit_values, lifted to scale_in = 31 Delta (about q_4), dropped to L = 5 -> ONE
    ct_poly_sp call with the degree-7 Taylor polynomial of the logistic function, 0.5 + x/4 - x^3/48 + x^5/480 -
    17 x^7/80640, scale_out = Delta -> decrypt_level at level out_primes = 1 and Delta: the call equals poly_expect bit for
    bit, the decrypt outputs equal the oracle's, and every slot is within the reference's 0.1 of p(x) in float64 (on the
    expectation first).  Range, the caller's condition: the combine's input, the weighted sum at level l = 2, decrypts
    to coefficients below Q_2 / 2 (|p(x)| . scale_out . q_1 < Q_2 / 2), checked on the model's sum."""
    from oracle.pyoracle import Oracle
    shape = (8192, 6)
    c = keyed_cases(shape)
    ctx, o, L = c["ctx"], c["o"], c["L"]
    n, npr = shape
    scale_out = o.scale
    sched = poly_schedule(o.q, L, LOGISTIC7, c["scale_in"], scale_out)
    assert sched["powers"] == [1, 2, 3, 4, 5, 7] and sched["level"] == 2 and sched["out_primes"] == 1
    plan = env["pkg"].poly_create(n, npr, L, LOGISTIC7, c["scale_in"], scale_out)
    l0, l1 = c["dropped"]
    r0, r1 = run_poly(env, ctx, plan, dev_t(env, l0), dev_t(env, l1))
    e0, e1, x = poly_expect(o, l0, l1, sched, c["evk0"], c["evk1"])
    assert (r0 == e0).all() and (r1 == e1).all()
    ts, lv = sched["terms"], sched["level"]
    w = [sched["weights"][d] for d in ts]
    s0, s1 = (weighted_sum_expect(o, [x[d][k] for d in ts], w, lv) for k in (0, 1))
    lo2 = Oracle(n, lv)
    check_headroom(lo2, s0, s1, c["s_hat"][:lv], "the combine's input")
    half = o.q[0] * o.q[1] // 2
    for b in range(s0.shape[0]):
        assert max(abs(v) for v in expectation(lo2, s0[b], s1[b], c["s_hat"][:lv])["y"]) < half
    want = poly_value(LOGISTIC7, c["vals"].astype(np.float64))
    check_level_decrypt(env, ctx, Oracle(n, sched["out_primes"]), r0, r1, c["s_hat"], sched["out_primes"], scale_out, want,
                        "logistic degree 7")
    plan.close()


def test_degree_15_at_16384x13(env, keyed_cases):
    """Test 8 at 16384 x 13, L = 12, B = 1: degree 15, every coefficient in [-1/16, 1/16], scale_in = 32 Delta = 2^30 and
    scale_out = q_7 (about q): ONE ct_poly_sp call has the bits of the schedule run entry by entry on the GPU (no host
    model of the ladder at this size), and decrypt_level at level out_primes = 7 and scale_out is within the reference's
    0.1 of p(x) in float64."""
    from oracle.pyoracle import Oracle
    shape = (16384, 13)
    c = keyed_cases(shape)
    ctx, o, L = c["ctx"], c["o"], c["L"]
    n, npr = shape
    rng = np.random.default_rng(113)
    coeff = [float(a) for a in rng.uniform(-1.0 / 16, 1.0 / 16, 16)]
    assert all(a != 0 for a in coeff)
    scale_out = float(o.q[7])
    sched = poly_schedule(o.q, L, coeff, c["scale_in"], scale_out)
    assert sched["powers"] == list(range(1, 16)) and sched["out_primes"] == 7
    plan = env["pkg"].poly_create(n, npr, L, coeff, c["scale_in"], scale_out)
    l0, l1 = c["dropped"]
    d0, d1 = dev_t(env, l0), dev_t(env, l1)
    r0, r1 = run_poly(env, ctx, plan, d0, d1)
    t0, t1, _ = gpu_composition(env, ctx, sched, d0, d1)
    assert r0.tobytes() == t0.tobytes() and r1.tobytes() == t1.tobytes()
    want = poly_value(coeff, c["vals"].astype(np.float64))
    check_level_decrypt(env, ctx, Oracle(n, 7), r0, r1, c["s_hat"], 7, scale_out, want, "degree 15")
    plan.close()


# ---- test 9: the example --------------------------------------------------------------------------------------------
def test_poly_activation_example(env, tmp_path):
    """examples/poly_activation_roundtrip.c from plain gcc: records encrypted, lifted, dropped to L = 5, one
    se_amd_ct_poly_sp_device call with the degree-7 logistic polynomial, decrypted within the reference's 0.1."""
    run_example("poly_activation_roundtrip", tmp_path, ("8192", "6", "4"))
