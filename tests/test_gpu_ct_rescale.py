"""Rescale, plaintext products and the level-aware decrypt (-m gpu): se_amd_ct_rescale_device,
se_amd_ct_mul_plain_device, se_amd_decrypt_level[_keyed]_device.
Every expectation is built from the oracle's primitives (ntt, intt, decrypt, fft, expand_ternary) and Python / NumPy
integers, never from the code under test; every comparison is bit-exact except the reference's own acceptance criterion
|values - expected| < 0.1 (device/test/ckks_tests_common.c:132).  Oracle(n, L - 1) is the oracle of the level below
Oracle(n, L): the default chains are prefixes of one another."""
import numpy as np
import pytest

import vectors as V
from ct_model import SHAPE_IDS, centred, negacyclic, rescale_expect
from gpu_support import (NULL, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_matches, assert_untouched,  # noqa: F401
                         assert_zero_prefix, bits, check_level_decrypt, dev_t, dptr, encrypt_sym, env, expectation,
                         host_u32, ntt_secret, records, run_decrypt, run_example, same_bytes, stream_of)

pytestmark = pytest.mark.gpu

WEIGHT_BITS = 30


# ---- expectations ----------------------------------------------------------------------------------------------------
def run_rescale(env, ctx, in0, in1, primes):
    """One call; the outputs carry two extra rows behind the packed [B][primes-1][n] result, pre-filled with a
    sentinel that must survive.  -> out0, out1 | None (host uint32 [B][primes-1][n])."""
    torch = env["torch"]
    B, n = in0.shape[0], ctx.n
    words = B * (primes - 1) * n

    def fresh():
        return torch.full((words + 2 * n,), SENTINEL, dtype=torch.int32, device=env["dev"])

    out0 = fresh()
    out1 = fresh() if in1 is not None else None
    ctx.ct_rescale(in0, out0, in1, out1, primes=primes)
    torch.cuda.synchronize()
    res = []
    for o in (out0, out1):
        if o is None:
            res.append(None)
            continue
        h = host_u32(o)
        assert (h[words:] == SENTINEL).all(), "rows behind the result are not written"
        res.append(h[:words].reshape(B, primes - 1, n))
    return res


# ---- test 1: the rescale on arbitrary slabs -------------------------------------------------------------------------
def boundary_row(o, j, rng):
    """NTT form of a natural-order vector that holds both ends of the centred range, (q-1)/2 -> +(q-1)/2 and
    (q+1)/2 -> -(q-1)/2, beside 0, 1, q-1 and random values."""
    q = o.q[j]
    d = rng.integers(0, q, o.n, dtype=np.uint32)
    d[::3] = (q - 1) // 2
    d[1::3] = (q + 1) // 2
    d[-5:] = [0, 1, q - 1, (q - 1) // 2, (q + 1) // 2]
    row = o.ntt(d, j)
    assert (o.intt(row, j) == d).all()
    return row


def arbitrary_slab(o, L, rng, B=4):
    """Records 0, 1: random residues.  Records 2, 3: lower rows alternately all 0 and all q_j - 1 (record 3 the other
    way round), last row = boundary_row."""
    slab = np.stack([rng.integers(0, o.q[j], (B, o.n), dtype=np.uint32) for j in range(L)], axis=1)
    for b in (2, 3):
        for j in range(L - 1):
            slab[b, j] = 0 if (j + b) % 2 == 0 else o.q[j] - 1
        slab[b, L - 1] = boundary_row(o, L - 1, rng)
    return slab


RESCALE_CASES = [((4096, 2), (2,)), ((4096, 3), (3, 2)), ((8192, 6), (6,)), ((16384, 6), (6,)), ((16384, 13), (13,))]


@pytest.mark.parametrize("shape,levels", RESCALE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_rescale_arbitrary_slabs(env, shape, levels):
    """Test 1: random residues, all-0 and all-(q_j - 1) rows and the centred lift's two boundaries; both slabs, then
    one slab alone; chained levels run on the expectation of the level above; nothing behind the result is written."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)          # no key is ever installed on this context
    rng = np.random.default_rng(100 * npr + n)
    slabs = [arbitrary_slab(o, levels[0], rng) for _ in range(2)]
    for L in levels:
        exp = [rescale_expect(o, s) for s in slabs]
        for e, s in zip(exp, slabs):
            assert e.shape == (4, L - 1, n)
            assert all((e[:, j] < o.q[j]).all() for j in range(L - 1))
        d0, d1 = dev_t(env, slabs[0]), dev_t(env, slabs[1])
        out0, out1 = run_rescale(env, ctx, d0, d1, L)
        assert (out0 == exp[0]).all() and (out1 == exp[1]).all(), L
        one, none = run_rescale(env, ctx, d1, None, L)
        assert none is None and (one == exp[1]).all(), L
        slabs = exp
    ctx.close()


def test_rescale_arguments(env):
    """The argument errors of the entry return -22 and write nothing; B = 0 is a successful no-op; no key is needed."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 2
    ctx = env["pkg"].Context(n, npr)
    in0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    in1 = torch.zeros_like(in0)
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    f = CEntry(ctx.L.se_amd_ct_rescale_device, ctx=ctx.h, in0=dptr(in0), in1=dptr(in1), B=B, primes=3, out0=dptr(out0),
               out1=dptr(out1), stream=stream_of(env))
    f.refused([
        dict(ctx=None),
        dict(in0=NULL),                                        # NULL d_in0
        dict(out0=NULL),                                       # NULL d_out0
        dict(out1=NULL),                                       # half a second pair
        dict(in1=NULL),
        dict(primes=1),                                        # primes outside [2, np]
        dict(primes=0),
        dict(primes=4),
        dict(in0=dptr(in0, 4)),                                # alignment, each slab
        dict(in1=dptr(in1, 8)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
    ])
    assert f(B=0) == 0
    assert_untouched(out0, out1)
    # the all-zero slab rescales to zero: (0 - NTT(0)) . inv
    assert f(in1=NULL, out1=NULL) == 0
    assert_zero_prefix(out0, B * 2 * n)
    ctx.close()


# ---- test 2: the exact integer identity -----------------------------------------------------------------------------
def ternary_natural(o, sk):
    """The secret key as int64 coefficients in {-1, 0, 1}, natural order."""
    s = o.expand_ternary(sk, 0).astype(np.int64)
    return np.where(s == o.q[0] - 1, -1, s)


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_rescale_exact_integer_identity(env, shape):
    """Test 2: with y, y' the oracle's centred CRT values of a symmetric ciphertext before and after the rescale and
    delta_i the oracle's centred INTT of the last-prime rows, q_last . y' + delta_0 + (delta_1 * s) == y as integers,
    for every coefficient.  No model of the rescale is involved."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    B = 2
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    c0, c1, _, st = encrypt_sym(env, ctx, V.bench_values(B, n, first=3), first=3)
    assert bool((st == 1).all())
    r0, r1 = run_rescale(env, ctx, c0, c1, npr)
    o, lo = Oracle(n, npr), Oracle(n, npr - 1)
    s_hat = ntt_secret(o, sk)
    s_nat = ternary_natural(o, sk)
    h0, h1 = host_u32(c0), host_u32(c1)
    q_last = o.q[-1]
    for b in range(B):
        y = np.array(expectation(o, h0[b], h1[b], s_hat)["y"], dtype=object)
        y2 = np.array(expectation(lo, r0[b], r1[b], s_hat[:npr - 1])["y"], dtype=object)
        d0 = centred(o.intt(h0[b, npr - 1], npr - 1), q_last)
        d1 = centred(o.intt(h1[b, npr - 1], npr - 1), q_last)
        lhs = q_last * y2 + d0.astype(object) + negacyclic(d1, s_nat).astype(object)
        assert (lhs == y).all(), b
    ctx.close()


# ---- test 3: decrypt_level ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def level_cases(env):
    """Per shape, computed once: four records encrypted under one key, on a context that keeps the key installed."""
    cache = {}

    def get(shape):
        if shape not in cache:
            n, npr = shape
            ctx = env["pkg"].Context(n, npr)
            sk = V.secret_key(n)
            ctx.set_secret_key(sk)
            recs = [r for r in records(n) if r[0] in ("bench", "pattern8x100", "1e6", "pattern4")]
            vals = np.stack([v for _, v in recs]).astype(np.float32)
            c0, c1, _, st = encrypt_sym(env, ctx, vals, first=11)
            assert bool((st == 1).all())
            cache[shape] = dict(ctx=ctx, sk=sk, c0=c0, c1=c1, B=len(recs))
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()


def test_level_full_is_decrypt_full(env, level_cases):
    """Test 3a: primes = np and the context's scale give the bytes of decrypt_full on every output."""
    c = level_cases((4096, 3))
    ctx = c["ctx"]
    full = run_decrypt(env, ctx, c["c0"], c["c1"])
    got = run_decrypt(env, ctx, c["c0"], c["c1"], 3, ctx.scale())
    assert bool((full["status"] == 1).all())
    for f in ("pte", "values", "values_f64", "status"):
        assert same_bytes(got[f], full[f]), f


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_level_below_is_the_smaller_parameter_set(env, level_cases, shape):
    """Test 3b: the first np - 1 rows of each record, re-packed, at primes = np - 1: the bytes of decrypt_full on
    Context(n, np - 1) with the same key."""
    n, npr = shape
    c = level_cases(shape)
    ctx = c["ctx"]
    l0, l1 = c["c0"][:, :npr - 1].contiguous(), c["c1"][:, :npr - 1].contiguous()
    small = env["pkg"].Context(n, npr - 1)
    small.set_secret_key(c["sk"])
    assert small.scale() == ctx.scale()
    ref = run_decrypt(env, small, l0, l1)
    got = run_decrypt(env, ctx, l0, l1, npr - 1, ctx.scale())
    assert bool((ref["status"] == 1).all())
    for f in ("pte", "values", "values_f64", "status"):
        assert same_bytes(got[f], ref[f]), f
    small.close()


def test_level_one_is_the_single_prime_entry(env, level_cases):
    """Test 3c: primes = 1 on row 0 of each record: values bit-identical to decrypt_decode for prime 0."""
    torch = env["torch"]
    c = level_cases((4096, 3))
    ctx, n, B = c["ctx"], 4096, c["B"]
    ref = torch.zeros((B, n // 2), dtype=torch.float32, device=env["dev"])
    ctx.decrypt_decode(c["c0"], c["c1"], 0, None, None, ref)
    got = run_decrypt(env, ctx, c["c0"][:, :1].contiguous(), c["c1"][:, :1].contiguous(), 1, ctx.scale())
    assert bool((got["status"] == 1).all())
    assert torch.equal(got["values"].view(torch.int32), ref.view(torch.int32))


def test_level_scale_is_the_callers(env, level_cases):
    """Test 3d: scale = 2 . se_amd_scale: values_f64 (and the rest) equal the oracle expectation at that scale."""
    from oracle.pyoracle import Oracle
    c = level_cases((4096, 3))
    ctx = c["ctx"]
    o = Oracle(4096, 3)
    s_hat = ntt_secret(o, c["sk"])
    scale = 2.0 * ctx.scale()
    got = run_decrypt(env, ctx, c["c0"], c["c1"], 3, scale)
    h0, h1 = host_u32(c["c0"]), host_u32(c["c1"])
    for b in range(c["B"]):
        e = expectation(o, h0[b], h1[b], s_hat, scale)
        assert e["status"] == 1
        assert_matches(got, b, e, b)
        half = expectation(o, h0[b], h1[b], s_hat, ctx.scale())
        assert (bits(half["values_f64"] * 0.5) == bits(e["values_f64"])).all()      # a power of two: exact


def test_level_keyed_twin(env):
    """Test 3e: record b under ring key idx[b] at primes = np - 1 equals the unkeyed entry with that key installed, on
    all four outputs; an index == K gives status 2 and zero outputs; no ring is SE_ERR_NO_KEY."""
    torch = env["torch"]
    pkg = env["pkg"]
    n, npr, K, B = 4096, 3, 3, 12
    ctx = pkg.Context(n, npr)
    sk, _, _ = ctx.gen_keys_batch(V.derive_seeds("level-pk", K), V.derive_seeds("level-ep", K),
                                  sk_seeds=V.derive_seeds("level-sk", K))
    idx = np.array([0, 1, 2, 2, 1, 0, 0, 2, 1, 1, 0, 2], dtype=np.uint32)
    vals = V.bench_values(B, n, first=30)
    ss, sd = V.bench_seeds(B, first=30)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    ti = dev_t(env, idx)
    scale = ctx.scale() * 1.5
    l0, l1 = c0[:, :2].contiguous(), c1[:, :2].contiguous()
    with pytest.raises(pkg.SealEmbeddedAmdError, match="ring") as ei:
        ctx.decrypt_level_keyed(l0, l1, ti, 2, scale, status=torch.zeros(B, dtype=torch.uint8, device=env["dev"]))
    assert f"code {SE_ERR_NO_KEY}" in str(ei.value)
    ctx.set_secret_keyring(sk)
    ctx.encrypt_sym_keyed(dev_t(env, vals), ti, dev_t(env, ss), dev_t(env, sd), c0, c1)
    torch.cuda.synchronize()
    l0, l1 = c0[:, :2].contiguous(), c1[:, :2].contiguous()
    bad = idx.copy()
    bad[7] = K
    got = run_decrypt(env, ctx, l0, l1, 2, scale, key_idx=dev_t(env, bad))
    for k in range(K):
        sel = np.nonzero((idx == k) & (bad < K))[0]
        ts = torch.from_numpy(sel).to(env["dev"])
        ctx.set_secret_key(sk[k])
        ref = run_decrypt(env, ctx, l0.index_select(0, ts).contiguous(), l1.index_select(0, ts).contiguous(), 2, scale)
        assert bool((ref["status"] == 1).all())
        for f in ("pte", "values", "values_f64", "status"):
            assert same_bytes(got[f].index_select(0, ts), ref[f]), (k, f)
    assert int(got["status"][7]) == 2
    for f in ("pte", "values", "values_f64"):
        assert int(torch.count_nonzero(got[f][7])) == 0, f
    ctx.close()


def test_level_arguments(env):
    """Test 3f: primes = 0 and np + 1, scale 0, NaN (and negative, infinite) are -22; no key is SE_ERR_NO_KEY; the other
    argument errors and B = 0 are those of the full entry."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 2
    ctx = env["pkg"].Context(n, npr)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    good = ctx.scale()
    f = CEntry(ctx.L.se_amd_decrypt_level_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, primes=3, scale=good,
               pte=NULL, values=NULL, values_f64=NULL, status=dptr(st), stream=stream_of(env))
    assert f() == SE_ERR_NO_KEY
    ctx.set_secret_key(V.secret_key(n))
    f.refused([dict(primes=0), dict(primes=4), dict(scale=0.0), dict(scale=float("nan")), dict(scale=-good),
               dict(scale=float("inf")),
               dict(ctx=None), dict(c0=NULL), dict(c1=NULL),
               dict(status=NULL)])                                                           # no output requested
    assert f(B=0) == 0
    # keyed twin
    ki = torch.zeros(B, dtype=torch.int32, device=env["dev"])
    fk = CEntry(ctx.L.se_amd_decrypt_level_keyed_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, primes=3, scale=good,
                key_idx=dptr(ki), pte=NULL, values=NULL, values_f64=NULL, status=dptr(st), stream=stream_of(env))
    assert fk() == SE_ERR_NO_KEY
    sk, _, _ = ctx.gen_keys_batch(V.derive_seeds("larg-pk", 2), V.derive_seeds("larg-ep", 2),
                                  sk_seeds=V.derive_seeds("larg-sk", 2))
    ctx.set_secret_keyring(sk)
    fk.refused([dict(primes=0), dict(primes=4), dict(scale=0.0), dict(scale=float("nan")),
                dict(key_idx=NULL)])                                                         # NULL d_key_idx
    assert_untouched(st, fill=77)
    assert fk(primes=2) == 0
    torch.cuda.synchronize()
    assert bool((st == 1).all())
    ctx.close()


# ---- test 4: the plaintext product ----------------------------------------------------------------------------------
def mul_expect(slab, pt, q, pidx):
    """slab uint32 [B][L][n], pt uint32 [P][>= L][n], pidx [B] -> (a . b) % q in uint64, zero rows for pidx >= P."""
    B, L, n = slab.shape
    qv = np.array(q[:L], dtype=np.uint64)[:, None]
    out = np.zeros_like(slab)
    for b in range(B):
        if pidx[b] < pt.shape[0]:
            out[b] = ((slab[b].astype(np.uint64) * pt[pidx[b], :L].astype(np.uint64)) % qv).astype(np.uint32)
    return out


def run_mul(env, ctx, in0, in1, pt, pt_idx=None, primes=None, in_place=False):
    torch = env["torch"]
    B = in0.shape[0]
    if in_place:
        in0 = in0.clone()
        in1 = in1.clone() if in1 is not None else None
        out0, out1 = in0, in1
    else:
        out0 = torch.full_like(in0, SENTINEL)
        out1 = torch.full_like(in1, SENTINEL) if in1 is not None else None
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    ctx.ct_mul_plain(in0, pt, out0, in1, out1, pt_idx=None if pt_idx is None else dev_t(env, pt_idx), primes=primes,
                     status=st)
    torch.cuda.synchronize()
    return host_u32(out0), (host_u32(out1) if out1 is not None else None), st.cpu().numpy()


@pytest.mark.parametrize("shape", [(1024, 1), (4096, 3), (16384, 13)], ids=SHAPE_IDS)
def test_mul_plain(env, shape):
    """Test 4: broadcast, identity, indexed with a repeated index, pt_primes > primes, in place, one slab, and an index
    == P (status 2, zero rows, neighbours intact); records 3 (slabs) and 1 (plaintexts) are all q_j - 1."""
    n, npr = shape
    B, P = 5, 3
    ctx = env["pkg"].Context(n, npr)          # no key is ever installed on this context
    q = ctx.moduli()
    rng = np.random.default_rng(4 * n + npr)
    rand = lambda cnt: np.stack([rng.integers(0, q[j], (cnt, n), dtype=np.uint32) for j in range(npr)], axis=1)
    s0, s1, pts, ptb = rand(B), rand(B), rand(P), rand(B)
    top = (np.array(q, dtype=np.uint32) - 1)[:, None]
    s0[3] = s1[3] = pts[1] = ptb[3] = top
    d0, d1, dP, dB = (dev_t(env, a) for a in (s0, s1, pts, ptb))
    ident = np.arange(B)
    # broadcast: P = 1, no index
    o0, o1, st = run_mul(env, ctx, d0, d1, dP[:1].contiguous())
    zero = np.zeros(B, dtype=np.int64)
    assert (st == 1).all() and (o0 == mul_expect(s0, pts[:1], q, zero)).all() and \
        (o1 == mul_expect(s1, pts[:1], q, zero)).all()
    # identity: P = B, no index
    o0, o1, st = run_mul(env, ctx, d0, d1, dB)
    assert (st == 1).all() and (o0 == mul_expect(s0, ptb, q, ident)).all() and (o1 == mul_expect(s1, ptb, q, ident)).all()
    # indexed, a repeated index; then the same in place, then one slab
    idx = np.array([2, 0, 2, 1, 1], dtype=np.uint32)
    e0, e1 = mul_expect(s0, pts, q, idx), mul_expect(s1, pts, q, idx)
    assert int(e0[3, 0, 0]) == (q[0] - 1) * (q[0] - 1) % q[0] == 1
    o0, o1, st = run_mul(env, ctx, d0, d1, dP, idx)
    assert (st == 1).all() and (o0 == e0).all() and (o1 == e1).all()
    o0, o1, st = run_mul(env, ctx, d0, d1, dP, idx, in_place=True)
    assert (st == 1).all() and (o0 == e0).all() and (o1 == e1).all()
    o0, none, st = run_mul(env, ctx, d1, None, dP, idx)
    assert none is None and (st == 1).all() and (o0 == e1).all()
    # an index == P and one far beyond: status 2 and zero rows, the neighbours are intact
    bad = np.array([2, P, 0, 0xFFFFFFFF, 1], dtype=np.uint32)
    o0, o1, st = run_mul(env, ctx, d0, d1, dP, bad)
    assert list(st) == [1, 2, 1, 2, 1]
    assert (o0 == mul_expect(s0, pts, q, bad)).all() and (o1 == mul_expect(s1, pts, q, bad)).all()
    assert not o0[1].any() and not o1[3].any()
    # pt_primes > primes: level np - 1 records against plaintexts of np rows
    if npr > 1:
        l0, l1 = s0[:, :npr - 1].copy(), s1[:, :npr - 1].copy()
        o0, o1, st = run_mul(env, ctx, dev_t(env, l0), dev_t(env, l1), dP, idx, primes=npr - 1)
        assert (st == 1).all() and (o0 == mul_expect(l0, pts, q, idx)).all() and (o1 == mul_expect(l1, pts, q, idx)).all()
    ctx.close()


def test_mul_plain_more_records_than_grid_rows(env):
    """The kernel walks records blockIdx.y, blockIdx.y + 65 535, ...: 65 540 records at 1024 x 1, one slab, in place,
    one plaintext for all."""
    torch = env["torch"]
    n, B = 1024, 65540
    ctx = env["pkg"].Context(n, 1)
    q = ctx.moduli()[0]
    rng = np.random.default_rng(65540)
    slab = rng.integers(0, q, (B, 1, n), dtype=np.uint32)
    pt = rng.integers(0, q, (1, 1, n), dtype=np.uint32)
    d = dev_t(env, slab)
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    ctx.ct_mul_plain(d, dev_t(env, pt), d, status=st)
    torch.cuda.synchronize()
    exp = ((slab.astype(np.uint64) * pt.astype(np.uint64)) % np.uint64(q)).astype(np.uint32)
    assert bool((st == 1).all())
    assert (host_u32(d) == exp).all()
    ctx.close()


def test_mul_plain_arguments(env):
    """The argument errors of the entry return -22 and write nothing; B = 0 is a successful no-op."""
    torch = env["torch"]
    n, npr, B, P = 4096, 3, 4, 2
    ctx = env["pkg"].Context(n, npr)
    in0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    in1 = torch.zeros_like(in0)
    out0 = torch.full_like(in0, SENTINEL)
    out1 = torch.full_like(in0, SENTINEL)
    pt = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    idx = torch.zeros(B, dtype=torch.int32, device=env["dev"])
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    f = CEntry(ctx.L.se_amd_ct_mul_plain_device, ctx=ctx.h, in0=dptr(in0), in1=dptr(in1), B=B, primes=3, pt=dptr(pt),
               P=P, pt_primes=3, pt_idx=dptr(idx), out0=dptr(out0), out1=dptr(out1), status=dptr(st),
               stream=stream_of(env))
    big = 2 ** 32
    f.refused([
        dict(ctx=None),
        dict(in0=NULL),                                        # NULL d_in0
        dict(out0=NULL),                                       # NULL d_out0
        dict(pt=NULL),                                         # NULL d_pt
        dict(out1=NULL),                                       # half a second pair
        dict(in1=NULL),
        dict(primes=0),                                        # primes outside [1, np]
        dict(primes=4, pt_primes=4),
        dict(pt_primes=2),                                     # pt_primes < primes
        dict(P=2, pt_idx=NULL),                                # no index, P neither 1 nor B
        dict(P=0, pt_idx=NULL),
        dict(P=B + 1, pt_idx=NULL),
        dict(B=big),                                           # B, P >= 2^32
        dict(P=big),
        dict(in0=dptr(in0, 4)),                                # alignment
        dict(in1=dptr(in1, 8)),
        dict(pt=dptr(pt, 4)),
        dict(out0=dptr(out0, 12)),
        dict(out1=dptr(out1, 4)),
    ])
    assert f(B=0) == 0
    assert_untouched(out0, out1)
    assert_untouched(st, fill=77)
    # the valid calls work without a key and without a status
    assert f(P=B, pt_idx=NULL, status=NULL) == 0
    assert f(in1=NULL, P=1, pt_idx=NULL, out1=NULL, status=NULL) == 0
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(out0)) == 0 and int(torch.count_nonzero(out1)) == 0
    ctx.close()


# ---- tests 5 and 6: end to end --------------------------------------------------------------------------------------
def test_weighted_sum_end_to_end(env):
    """Test 5: 4096 x 3, 16 records, weights uniform in [-1, 1] applied as round(w . 2^30): lincomb (one group) ->
    rescale -> decrypt_level(primes = 2, scale = Delta . 2^30 / q_2).  The rescaled record equals the expectation built
    on the aggregator's sum, pte / values / values_f64 equal the oracle's on that record, status is 1 and the result is
    within the reference's 0.1 of sum_k (round(w_k . 2^30) / 2^30) . v_k (a CPU simulation of noise, encode rounding
    and rescale rounding puts the error at 1.5e-4 .. 2.0e-4 for this shape)."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 4096, 3, 16
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    vals = V.bench_values(B, n, first=50)
    c0, c1, _, st = encrypt_sym(env, ctx, vals, first=50)
    assert bool((st == 1).all())
    rng = np.random.default_rng(5)
    w = np.rint(rng.uniform(-1.0, 1.0, B) * 2.0 ** WEIGHT_BITS).astype(np.int64)
    assert np.abs(w).max() <= 2 ** WEIGHT_BITS
    s0 = torch.full((1, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    s1 = torch.full_like(s0, SENTINEL)
    ast = torch.full((1,), 77, dtype=torch.uint8, device=env["dev"])
    ctx.ct_lincomb(c0, s0, c1, s1, w=dev_t(env, w.astype(np.int32).reshape(1, B)), G=1, status=ast)
    torch.cuda.synchronize()
    assert int(ast[0]) == 1
    r0, r1 = run_rescale(env, ctx, s0, s1, npr)
    o, lo = Oracle(n, npr), Oracle(n, npr - 1)
    assert (r0 == rescale_expect(o, host_u32(s0))).all() and (r1 == rescale_expect(o, host_u32(s1))).all()
    scale = o.scale * 2.0 ** WEIGHT_BITS / o.q[npr - 1]
    want = [(w.astype(np.float64) / 2.0 ** WEIGHT_BITS) @ vals.astype(np.float64)]
    check_level_decrypt(env, ctx, lo, r0, r1, ntt_secret(o, sk), npr - 1, scale, want)
    ctx.close()


@pytest.mark.parametrize("shape", [(4096, 3), (16384, 6)], ids=SHAPE_IDS)
def test_slotwise_product_end_to_end(env, shape):
    """Test 6: 4 records, one weight vector per record uniform in [-1, 1] encoded with encode_ntt: ct_mul_plain ->
    rescale -> decrypt_level(primes = np - 1, scale = Delta^2 / q_last), bit-exact against the oracle on the rescaled
    records and within the reference's 0.1 of v (.) w (the same simulation gives 4.3e-3 at n = 4096, 2.2e-2 at
    n = 16384)."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    B = 4
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    vals = V.bench_values(B, n, first=70)
    c0, c1, _, st = encrypt_sym(env, ctx, vals, first=70)
    assert bool((st == 1).all())
    wv = np.random.default_rng(6 + n).uniform(-1.0, 1.0, (B, n // 2)).astype(np.float32)
    pt = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    est = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encode_ntt(dev_t(env, wv), pt, status=est)
    torch.cuda.synchronize()
    assert bool((est == 1).all())
    m0, m1 = torch.full_like(c0, SENTINEL), torch.full_like(c0, SENTINEL)
    mst = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    ctx.ct_mul_plain(c0, pt, m0, c1, m1, status=mst)
    torch.cuda.synchronize()
    assert bool((mst == 1).all())
    o, lo = Oracle(n, npr), Oracle(n, npr - 1)
    q = o.q
    ident = np.arange(B)
    hp = host_u32(pt)
    assert (host_u32(m0) == mul_expect(host_u32(c0), hp, q, ident)).all()
    assert (host_u32(m1) == mul_expect(host_u32(c1), hp, q, ident)).all()
    r0, r1 = run_rescale(env, ctx, m0, m1, npr)
    assert (r0 == rescale_expect(o, host_u32(m0))).all() and (r1 == rescale_expect(o, host_u32(m1))).all()
    scale = o.scale * o.scale / q[npr - 1]
    want = [vals[b].astype(np.float64) * wv[b].astype(np.float64) for b in range(B)]
    check_level_decrypt(env, ctx, lo, r0, r1, ntt_secret(o, sk), npr - 1, scale, want)
    ctx.close()


# ---- test 7: the example --------------------------------------------------------------------------------------------
def test_weighted_average_example(env, tmp_path):
    """examples/weighted_average_roundtrip.c from plain gcc: real weights through lincomb, rescale and decrypt_level
    come back within the reference's 0.1."""
    run_example("weighted_average_roundtrip", tmp_path, ("4096", "3", "16"))
