"""Linear transforms (-m gpu): se_amd_lintrans_create / se_amd_ct_lintrans_device, plaintext-weighted sums of hoisted
rotations (the diagonal method) under a plan that holds the diagonals folded into the Galois keys.
Every expectation is written from the definition with the oracle's primitives (ntt, intt,
decrypt, fft, expand_ternary, encode_ntt_batch), se_amd_galois_table -- a host-only entry pinned against the
coefficient-domain automorphism by tests/test_ct_galois_build.py -- and Python / NumPy integers, never from the device
code under test:
    D_{j,t}          = digits_of(c1)                                  (of c1 itself, not of sigma(c1))
    rot0[e][b][i][k] = c0[b][i][src_e(k)] + sum_r NTT_i(D_r)[src_e(k)] . gk0_e[r][i][k]   mod q_i
    rot1[e][b][i][k] =                      sum_r NTT_i(D_r)[src_e(k)] . gk1_e[r][i][k]   mod q_i
    out0[b][i][k]    = d0[i][k] . c0[b][i][k] + sum_e d_e[i][k] . rot0[e][b][i][k]        mod q_i   (out1: c1, rot1)
with the keys installed when the plan was created, any 32-bit word of a diagonal standing for its residue.
Every comparison is bit-exact except the reference's own acceptance criterion |values - expected| < 0.1
(device/test/ckks_tests_common.c:132).  Oracle(n, L - 1) is the oracle of the level below Oracle(n, L)."""
import numpy as np
import pytest

from ct_model import (CASE_IDS, GALOIS_CASES, SHAPE_IDS, call_elements, edge_row, hoist_expect, lintrans_expect, matrix,
                      matrix_diagonals, rand_slab, random_diagonals, random_keys)
from gpu_support import (NULL, SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_untouched,  # noqa: F401
                         assert_zero_prefix, check_headroom, check_level_decrypt, create_handle, creates_refused, dev_t,
                         dptr, encode_diagonals, env, fresh_records, hptr, install_galois_keys, keyed_cases,
                         lift_records, periodic_values, rescale_records, run_example, run_many, run_plan, sentinel_out,
                         step_elements, stream_of, take)

pytestmark = pytest.mark.gpu


# ---- tests 1 to 3: the definition on arbitrary slabs, keys and diagonals --------------------------------------------
@pytest.fixture(scope="module")
def slab_cases(env):
    """slab_cases(shape, levels, B) -> the context with random key words installed (no secret key), the diagonals, and
    per level the slabs with the expectation of the hoisted rotations of every call element -- computed once and shared
    by tests 1 to 3."""
    from oracle.pyoracle import Oracle
    cache = {}

    def get(shape, levels, B):
        if shape in cache:
            return cache[shape]
        n, npr = shape
        o = Oracle(n, npr)
        ctx = env["pkg"].Context(n, npr)
        q = o.q
        rng = np.random.default_rng(43 * n + npr)
        elts = call_elements(n, npr)
        keys = sorted(set(elts))
        key_of = {g: k for k, g in enumerate(keys)}
        gk0, gk1 = random_keys(rng, q, len(keys), n, npr)
        ctx.set_galois_keys(keys, gk0, gk1)
        diag, diag0 = random_diagonals(rng, q, len(elts), n)
        per_level = {}
        for L in levels:
            c0, c1 = rand_slab(rng, q, B, n, L), rand_slab(rng, q, B, n, L)
            for j in range(L):
                c1[0, j] = edge_row(o, j, rng, elts, starts=6)
            c0[1] = c1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
            rot = hoist_expect(env["pkg"].galois_table, o, c0, c1, elts, key_of, gk0, gk1)
            per_level[L] = dict(c0=c0, c1=c1, d0=dev_t(env, c0), d1=dev_t(env, c1), rot=rot)
        cache[shape] = dict(ctx=ctx, o=o, elts=elts, keys=keys, key_of=key_of, gk=(gk0, gk1), diag=diag, diag0=diag0,
                            t_diag=dev_t(env, diag), t_diag0=dev_t(env, diag0), levels=per_level)
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()


@pytest.mark.parametrize("shape,levels,B", GALOIS_CASES, ids=CASE_IDS)
def test_plan_call_matches_the_definition(env, slab_cases, shape, levels, B):
    """Test 1: random residues for both slabs, the installed keys and the diagonals; one diagonal row of arbitrary 32-bit
    words >= q_i, 0 / 1 / q - 1 at fixed positions of every diagonal; record 0 of c1 is the edge row of the hoist tests,
    record 1 all q_j - 1.  With and without diag0, G = 1 and the full list (at 4096 x 3 one element twice with two
    diagonals); the level-2 call runs on the plans built with pt_primes = 3; a plan with pt_primes = 2 refuses level 3.
    Bit for bit, sentinels behind the outputs intact (run_plan)."""
    case = slab_cases(shape, levels, B)
    o, ctx, elts, n, npr = case["o"], case["ctx"], case["elts"], shape[0], shape[1]
    for G in (1, len(elts)):
        for with0 in (False, True):
            plan = ctx.lintrans_plan(elts[:G], case["t_diag"][:G].contiguous(), case["t_diag0"] if with0 else None)
            for L in levels:
                lv = case["levels"][L]
                want = lintrans_expect(o, (lv["rot"][0][:G], lv["rot"][1][:G]), case["diag"][:G], lv["c0"], lv["c1"],
                                       case["diag0"] if with0 else None)
                got = run_plan(env, ctx, plan, lv["d0"], lv["d1"], L)
                assert (got[0] == want[0]).all(), (G, with0, L, "out0")
                assert (got[1] == want[1]).all(), (G, with0, L, "out1")
            plan.close()
    if npr == 3:
        lv = case["levels"][3]
        short = ctx.lintrans_plan(elts, dev_t(env, case["diag"][:, :2]), dev_t(env, case["diag0"][:2]))
        out0, out1 = sentinel_out(env, B * 3 * n, 0), sentinel_out(env, B * 3 * n, 0)
        with pytest.raises(env["pkg"].SealEmbeddedAmdError, match="-22"):
            ctx.ct_lintrans(short, lv["d0"], lv["d1"], out0, out1, primes=3)
        env["torch"].cuda.synchronize()
        assert bool((out0 == SENTINEL).all()) and bool((out1 == SENTINEL).all())
        l2 = case["levels"][2]
        want = lintrans_expect(o, l2["rot"], case["diag"], l2["c0"], l2["c1"], case["diag0"])
        got = run_plan(env, ctx, short, l2["d0"], l2["d1"], 2)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), "pt_primes = 2 at level 2"
        short.close()


@pytest.mark.parametrize("shape,levels,B", GALOIS_CASES, ids=CASE_IDS)
def test_plan_call_is_the_composition_on_the_device(env, slab_cases, shape, levels, B):
    """Test 2: on the slabs of test 1, ONE many-form call, then one ct_mul_plain per element and one for diag0 (the
    diagonals reduced mod q_i, which is what a plaintext holds), summed mod q_i in NumPy: equal to the plan call bit for
    bit."""
    torch = env["torch"]
    case = slab_cases(shape, levels, B)
    o, ctx, elts, n = case["o"], case["ctx"], case["elts"], shape[0]
    G = len(elts)
    qv = np.array(o.q, dtype=np.uint64)[:, None]
    red = (case["diag"].astype(np.uint64) % qv[None]).astype(np.uint32)
    red0 = (case["diag0"].astype(np.uint64) % qv).astype(np.uint32)
    plan = ctx.lintrans_plan(elts, case["t_diag"], case["t_diag0"])
    for L in levels:
        lv = case["levels"][L]
        m0, m1 = run_many(env, ctx, lv["d0"], lv["d1"], elts, L)
        words = B * L * n
        acc = [np.zeros((B, L, n), dtype=np.uint64), np.zeros((B, L, n), dtype=np.uint64)]
        terms = [(dev_t(env, m0[e]), dev_t(env, m1[e]), red[e]) for e in range(G)] + [(lv["d0"], lv["d1"], red0)]
        for in0, in1, pt in terms:
            p0, p1 = sentinel_out(env, words, 2 * n), sentinel_out(env, words, 2 * n)
            ctx.ct_mul_plain(in0, dev_t(env, pt[None]), p0, in1, p1, primes=L)
            torch.cuda.synchronize()
            acc[0] += take(p0, words, (B, L, n), "mul_plain out0")
            acc[1] += take(p1, words, (B, L, n), "mul_plain out1")
        got = run_plan(env, ctx, plan, lv["d0"], lv["d1"], L)
        for h in (0, 1):
            assert (got[h] == (acc[h] % qv[None, :L]).astype(np.uint32)).all(), (L, h)
    plan.close()


def test_plan_is_a_snapshot_of_the_keys(env, slab_cases):
    """Test 3: a plan, then different random keys installed for the same elements: the old plan still returns the bits
    of test 1, a new plan the expectation under the new keys, which differs.  Destroying both, then closing the
    context (the fixture), is clean; the first keys are put back for the other tests."""
    shape, levels, B = GALOIS_CASES[1]
    case = slab_cases(shape, levels, B)
    o, ctx, elts, n, npr = case["o"], case["ctx"], case["elts"], shape[0], shape[1]
    lv = case["levels"][npr]
    old = ctx.lintrans_plan(elts, case["t_diag"], case["t_diag0"])
    want_old = lintrans_expect(o, lv["rot"], case["diag"], lv["c0"], lv["c1"], case["diag0"])
    nk0, nk1 = random_keys(np.random.default_rng(77), o.q, len(case["keys"]), n, npr)
    ctx.set_galois_keys(case["keys"], nk0, nk1)
    try:
        new = ctx.lintrans_plan(elts, case["t_diag"], case["t_diag0"])
        rot_new = hoist_expect(env["pkg"].galois_table, o, lv["c0"], lv["c1"], elts, case["key_of"], nk0, nk1)
        want_new = lintrans_expect(o, rot_new, case["diag"], lv["c0"], lv["c1"], case["diag0"])
        assert (want_new[0] != want_old[0]).any() and (want_new[1] != want_old[1]).any()
        got_old = run_plan(env, ctx, old, lv["d0"], lv["d1"], npr)
        got_new = run_plan(env, ctx, new, lv["d0"], lv["d1"], npr)
        assert (got_old[0] == want_old[0]).all() and (got_old[1] == want_old[1]).all(), "the old plan changed"
        assert (got_new[0] == want_new[0]).all() and (got_new[1] == want_new[1]).all(), "the new plan"
        old.close()
        new.close()
        old.close()                                        # closing twice is a no-op
    finally:
        ctx.set_galois_keys(case["keys"], *case["gk"])


# ---- test 4: arguments ----------------------------------------------------------------------------------------------
def test_lintrans_arguments(env):
    """Every documented error returns its code and leaves the sentinel-filled outputs untouched.  The call: the pointer,
    alignment, level and B checks of se_amd_ct_galois_device, a NULL plan, a plan of another context, a level above the
    plan's.  Create: NULL elts / d_diag / out, G = 0 and 65, pt_primes = 0, an even element, one >= 2n, a misaligned
    diagonal -- the handle stays NULL --, an element without a key: SE_ERR_NO_KEY with the element named.  B = 0
    succeeds and writes nothing; se_amd_lintrans_destroy(NULL) is safe."""
    torch, pkg = env["torch"], env["pkg"]
    n, npr, B = 4096, 3, 2
    ctx, other = pkg.Context(n, npr), pkg.Context(n, npr)
    L, h = ctx.L, ctx.h
    key = np.zeros((2, 2 * npr, npr, n), dtype=np.uint32)
    ctx.set_galois_keys([3, 9], key, key)
    other.set_galois_keys([3, 9], key, key)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    diag = torch.ones((2, npr, n), dtype=torch.int32, device=env["dev"])
    diag0 = torch.ones((npr, n), dtype=torch.int32, device=env["dev"])
    el = lambda *g: np.array(g + (0,) * (65 - len(g)), dtype=np.uint32)     # room for the G = 65 call
    good, even, big, nokey = el(3, 9), el(3, 4), el(3, 2 * n + 1), el(3, 5)
    mk = CEntry(L.se_amd_lintrans_create, ctx=h, elts=hptr(good), G=2, diag=dptr(diag), diag0=dptr(diag0), pt_primes=npr,
                out=None)
    creates_refused(mk, [
        dict(ctx=None),
        dict(elts=NULL),                                     # NULL elts, d_diag
        dict(diag=NULL),
        dict(G=0),                                           # G = 0, G = 65
        dict(G=65),
        dict(pt_primes=0),                                   # pt_primes = 0
        dict(elts=hptr(even)),                               # an even element, one >= 2n
        dict(elts=hptr(big)),
        dict(diag=dptr(diag, 4)),                            # alignment of either diagonal pointer
        dict(diag0=dptr(diag0, 8)),
    ])
    assert create_handle(mk, out=None)[0] == SE_ERR_INVALD_ARGUMENT                       # NULL out
    creates_refused(mk, [dict(elts=hptr(nokey))], SE_ERR_NO_KEY)
    assert "element 5" in L.se_amd_last_error().decode(), L.se_amd_last_error()
    rc, plan = create_handle(mk, pt_primes=2)                # a plan of two levels, with diag0
    assert rc == 0 and plan.value
    rc, foreign = create_handle(mk, ctx=other.h)
    assert rc == 0 and foreign.value
    rc, no0 = create_handle(mk, G=1, diag0=NULL, pt_primes=7)    # no diag0; pt_primes above np serves np levels
    assert rc == 0 and no0.value

    call = CEntry(L.se_amd_ct_lintrans_device, ctx=h, plan=plan, c0=dptr(c0), c1=dptr(c1), B=B, primes=2,
                  out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    call.refused([
        dict(ctx=None),
        dict(c0=NULL),                                       # NULL slab pointers
        dict(c1=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(primes=0),                                      # primes outside [1, np]
        dict(primes=4),
        dict(B=2 ** 32),                                     # B >= 2^32
        dict(c0=dptr(c0, 4)),                                # alignment, each slab
        dict(c1=dptr(c1, 8)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
        dict(plan=NULL),                                     # no plan
        dict(plan=foreign),                                  # a plan of another context
        dict(ctx=other.h),
        dict(primes=3),                                      # a level above the plan's
    ])
    assert call(B=0) == 0
    assert_untouched(out0, out1)
    # the plans work: zero keys and zero slabs give zero rows, at level 2 resp. 3
    for pl, lv in ((plan, 2), (no0, 3)):
        out0.fill_(SENTINEL)
        out1.fill_(SENTINEL)
        assert call(plan=pl, primes=lv) == 0
        for o in (out0, out1):
            assert_zero_prefix(o, B * lv * n)
    L.se_amd_lintrans_destroy(None)
    for pl in (plan, foreign, no0):
        L.se_amd_lintrans_destroy(pl)
    ctx.close()
    other.close()


# ---- test 5: end to end with a real key -------------------------------------------------------------------------------
DIM = 8
STEPS = tuple(range(1, DIM))
LIFT = 1 << 18            # tools/ct_galois_noise_sim.py --lintrans: the example's bookkeeping
DIAG_SHIFT = 256.0        # the diagonals are encoded from M / 2^8: their scale is Delta / 2^8


def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: the Galois keys of the
    steps 1 .. 7, installed; B = 4 fresh symmetric records holding 8-periodic slot values in [-1, 1]."""
    ctx = case["ctx"]
    n = ctx.n
    elts = step_elements(env, n, STEPS)
    gk0, gk1 = install_galois_keys(case, elts, "gk-lintrans")
    vals = periodic_values(4, n, DIM, 5000 + n)
    case.update(elts=elts, key_of={g: k for k, g in enumerate(elts)}, gk0=gk0, gk1=gk1, vals=vals,
                fresh=fresh_records(env, ctx, vals, 300))


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_matvec_end_to_end(env, keyed_cases, shape):
    """Test 5: ct_lincomb with weight 2^18 -> ONE plan call (steps 1 .. 7 and diag0; the diagonals of M / 2^8 encoded on
    the device) -> ct_rescale -> decrypt_level(primes = np - 1, scale = Delta 2^18 (Delta / 2^8) / q_last) on B = 4
    records of 8-periodic slot values in [-1, 1].  Every stage equals its definition bit for bit (the encoded diagonals
    equal the oracle's), the final pte / values / values_f64 equal the oracle's on the final records, every coefficient
    before the rescale is below 2^62, and the slots of the expectation and of the GPU are within the reference's 0.1 of
    M x.  The worst errors are printed."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    lo = Oracle(n, npr - 1)
    M = matrix(DIM)
    l0, l1 = lift_records(env, ctx, o, c["fresh"], LIFT)
    diag = encode_diagonals(env, ctx, o, matrix_diagonals(M, n, DIAG_SHIFT))
    # one plan, one call
    t_diag = dev_t(env, diag)
    plan = ctx.lintrans_plan(c["elts"], t_diag[1:].contiguous(), t_diag[0].contiguous())
    g0, g1 = run_plan(env, ctx, plan, dev_t(env, l0), dev_t(env, l1), npr)
    plan.close()
    rot = hoist_expect(env["pkg"].galois_table, o, l0, l1, c["elts"], c["key_of"], c["gk0"], c["gk1"])
    want = lintrans_expect(o, rot, diag[1:], l0, l1, diag[0])
    assert (g0 == want[0]).all() and (g1 == want[1]).all(), "plan call"
    check_headroom(o, g0, g1, c["s_hat"], "before the rescale")
    # rescale, decrypt one level lower
    f0, f1 = rescale_records(env, ctx, o, g0, g1, npr)
    scale = o.scale * LIFT * (o.scale / DIAG_SHIFT) / o.q[npr - 1]
    want_slots = np.tile(c["vals"].astype(np.float64)[:, :DIM] @ M.T, (1, n // 2 // DIM))
    check_level_decrypt(env, ctx, lo, f0, f1, c["s_hat"], npr - 1, scale, want_slots, "M x by the diagonal method")


# ---- test 6: the example --------------------------------------------------------------------------------------------
def test_matvec_example(env, tmp_path):
    """examples/matvec_roundtrip.c from plain gcc: the diagonals encoded and folded into a plan, lift, ONE
    se_amd_ct_lintrans_device call, rescale and decrypt_level come back within the reference's 0.1 of M x."""
    run_example("matvec_roundtrip", tmp_path, ("4096", "3", "8"))
