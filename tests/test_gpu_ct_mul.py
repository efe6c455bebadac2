"""Ciphertext products (-m gpu): the key-free tensor se_amd_ct_mul_device, the degree-2 decrypt
se_amd_decrypt3_level[_keyed]_device, the relinearisation key (se_amd_gen_relin_key, se_amd_set_relin_key) and
se_amd_ct_relin_device.
Every expectation is built from the oracle's primitives (ntt, intt, decrypt, fft, expand_ternary) and Python / NumPy
integers, never from the code under test; every comparison is bit-exact except the reference's own acceptance criterion
|values - expected| < 0.1 (device/test/ckks_tests_common.c:132).  Oracle(n, L - 1) is the oracle of the level below
Oracle(n, L): the default chains are prefixes of one another."""
import numpy as np
import pytest

import vectors as V
from ct_model import (DIGIT_MASK, SHAPE_IDS, crt_centred, digit_key_errors, digits_of, negacyclic, rand_slab,
                      relin_diagonal, relin_expect)
from gpu_support import (NULL, SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY, SENTINEL, CEntry, assert_matches,  # noqa: F401
                         assert_untouched, assert_zero_prefix, check_level_decrypt, decode_expect, dev_t, dptr,
                         encrypt_sym, env, expectation, fresh_records, keyed_cases, ntt_secret, rescale_records,
                         run_decrypt, run_example, run_relin, same_bytes, sentinel_out, stream_of, take, unit_values)

pytestmark = pytest.mark.gpu


# ---- test 1: the tensor on arbitrary slabs --------------------------------------------------------------------------
def tensor_expect(a0, a1, b0, b1, q, ia, ib):
    """-> uint32 [3][P][L][n]: (x . y) % q in uint64, the two products of out1 reduced before they are added; zero
    rows for an index out of range."""
    P, L, n = len(ia), a0.shape[1], a0.shape[2]
    qv = np.array(q[:L], dtype=np.uint64)[:, None]
    out = np.zeros((3, P, L, n), dtype=np.uint32)
    for p in range(P):
        if ia[p] >= a0.shape[0] or ib[p] >= b0.shape[0]:
            continue
        x0, x1 = a0[ia[p]].astype(np.uint64), a1[ia[p]].astype(np.uint64)
        y0, y1 = b0[ib[p]].astype(np.uint64), b1[ib[p]].astype(np.uint64)
        out[0, p] = (x0 * y0) % qv
        out[1, p] = ((x0 * y1) % qv + (x1 * y0) % qv) % qv
        out[2, p] = (x1 * y1) % qv
    return out


def run_tensor(env, ctx, a0, a1, b0, b1, ia=None, ib=None, primes=None):
    """One call on device slabs; every output has two rows of sentinels behind it.  -> (uint32 [3][P][L][n], status)."""
    torch = env["torch"]
    n = ctx.n
    L = a0.shape[1] if primes is None else primes
    P = a0.shape[0] if ia is None else len(ia)
    words = P * L * n
    outs = [sentinel_out(env, words, 2 * n) for _ in range(3)]
    st = torch.full((P,), 77, dtype=torch.uint8, device=env["dev"])
    ctx.ct_mul(a0, a1, b0, b1, *outs, ia=None if ia is None else dev_t(env, np.asarray(ia, dtype=np.uint32)),
               ib=None if ib is None else dev_t(env, np.asarray(ib, dtype=np.uint32)), primes=L, status=st)
    torch.cuda.synchronize()
    return np.stack([take(o, words, (P, L, n), "tensor") for o in outs]), st.cpu().numpy()


@pytest.mark.parametrize("shape", [(1024, 1), (4096, 3), (16384, 13)], ids=SHAPE_IDS)
def test_tensor_arbitrary_slabs(env, shape):
    """Test 1: Ba = 5, Bb = 3, record 3 of a and record 1 of b all q_j - 1.  Identity pairs (b padded to 5), an index list
    with a repeat, a = b for squares, primes = np - 1, and indices == Ba / 0xFFFFFFFF (status 2, zero rows, neighbours
    intact); the sentinel rows behind each output survive.  No key is ever installed on this context."""
    n, npr = shape
    Ba, Bb = 5, 3
    ctx = env["pkg"].Context(n, npr)
    q = ctx.moduli()
    rng = np.random.default_rng(7 * n + npr)
    a0, a1 = rand_slab(rng, q, Ba, n), rand_slab(rng, q, Ba, n)
    b0, b1 = rand_slab(rng, q, Bb, n), rand_slab(rng, q, Bb, n)
    top = (np.array(q, dtype=np.uint32) - 1)[:, None]
    a0[3] = a1[3] = b0[1] = b1[1] = top
    p0 = np.concatenate([b0, rand_slab(rng, q, Ba - Bb, n)])
    p1 = np.concatenate([b1, rand_slab(rng, q, Ba - Bb, n)])
    dA0, dA1, dB0, dB1, dP0, dP1 = (dev_t(env, x) for x in (a0, a1, b0, b1, p0, p1))
    ident = np.arange(Ba)
    # identity pairs, no index lists
    got, st = run_tensor(env, ctx, dA0, dA1, dP0, dP1)
    assert (st == 1).all() and (got == tensor_expect(a0, a1, p0, p1, q, ident, ident)).all()
    # index lists with a repeated pair; pair 3 is (all q - 1) x (all q - 1): 1, 2 (mod q), 1
    ia, ib = [4, 0, 4, 3, 1, 2, 3], [2, 0, 2, 1, 1, 0, 0]
    exp = tensor_expect(a0, a1, b0, b1, q, ia, ib)
    assert int(exp[0, 3, 0, 0]) == 1 and int(exp[1, 3, 0, 0]) == 2 and int(exp[2, 3, 0, 0]) == 1
    got, st = run_tensor(env, ctx, dA0, dA1, dB0, dB1, ia, ib)
    assert (st == 1).all() and (got == exp).all()
    # a = b: squares, the same pointers on both sides
    got, st = run_tensor(env, ctx, dA0, dA1, dA0, dA1)
    assert (st == 1).all() and (got == tensor_expect(a0, a1, a0, a1, q, ident, ident)).all()
    # out-of-range indices
    ia, ib = [4, Ba, 0, 0xFFFFFFFF, 2, 1], [2, 0, 0xFFFFFFFF, 1, Bb, 1]
    got, st = run_tensor(env, ctx, dA0, dA1, dB0, dB1, ia, ib)
    assert list(st) == [1, 2, 2, 2, 2, 1]
    assert (got == tensor_expect(a0, a1, b0, b1, q, ia, ib)).all()
    assert not got[:, 1:5].any() and got[:, 0].any() and got[:, 5].any()
    # one level down
    if npr > 1:
        la0, la1, lb0, lb1 = (x[:, :npr - 1].copy() for x in (a0, a1, b0, b1))
        ia, ib = [0, 3, 2], [1, 1, 2]
        got, st = run_tensor(env, ctx, *(dev_t(env, x) for x in (la0, la1, lb0, lb1)), ia, ib, primes=npr - 1)
        assert (st == 1).all() and (got == tensor_expect(la0, la1, lb0, lb1, q, ia, ib)).all()
    ctx.close()


def test_tensor_more_pairs_than_grid_rows(env):
    """The kernel walks pairs blockIdx.y, blockIdx.y + 65 535, ...: 65 540 pairs at 1024 x 1 over 4 records, a index
    p % 4, b index (p / 4) % 4.  The 16 distinct pairs are computed on the CPU; the comparison runs on the device."""
    torch = env["torch"]
    n, R, P = 1024, 4, 65540
    ctx = env["pkg"].Context(n, 1)
    q = ctx.moduli()
    rng = np.random.default_rng(65540)
    a0, a1 = rand_slab(rng, q, R, n), rand_slab(rng, q, R, n)
    p = np.arange(P)
    ia, ib = (p % 4).astype(np.uint32), ((p // 4) % 4).astype(np.uint32)
    table = tensor_expect(a0, a1, a0, a1, q, np.arange(16) % 4, np.arange(16) // 4)      # pair id = ia + 4 ib
    pid = dev_t(env, (ia + 4 * ib).astype(np.int64))
    dA0, dA1 = dev_t(env, a0), dev_t(env, a1)
    outs = [torch.full((P, 1, n), SENTINEL, dtype=torch.int32, device=env["dev"]) for _ in range(3)]
    st = torch.full((P,), 77, dtype=torch.uint8, device=env["dev"])
    ctx.ct_mul(dA0, dA1, dA0, dA1, *outs, ia=dev_t(env, ia), ib=dev_t(env, ib), status=st)
    torch.cuda.synchronize()
    assert bool((st == 1).all())
    for k in range(3):
        want = dev_t(env, table[k]).index_select(0, pid)
        assert torch.equal(outs[k], want), k
    ctx.close()


def test_tensor_arguments(env):
    """The argument errors return -22 and write nothing; P = 0 is a successful no-op; no key is needed."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 2
    ctx = env["pkg"].Context(n, npr)
    a0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    a1, b0, b1 = torch.zeros_like(a0), torch.zeros_like(a0), torch.zeros_like(a0)
    o0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    o1, o2 = torch.full_like(o0, SENTINEL), torch.full_like(o0, SENTINEL)
    idx = torch.zeros(B, dtype=torch.int32, device=env["dev"])
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    call = CEntry(ctx.L.se_amd_ct_mul_device, ctx=ctx.h, A0=dptr(a0), A1=dptr(a1), Ba=B, B0=dptr(b0), B1=dptr(b1), Bb=B,
                  primes=3, P=B, ia=dptr(idx), ib=dptr(idx), O0=dptr(o0), O1=dptr(o1), O2=dptr(o2), status=dptr(st),
                  stream=stream_of(env))
    big = 2 ** 32
    call.refused([
        dict(ctx=None), dict(A0=NULL), dict(A1=NULL), dict(B0=NULL), dict(B1=NULL), dict(O0=NULL), dict(O1=NULL),
        dict(O2=NULL),
        dict(ia=NULL), dict(ib=NULL),                               # only one index list
        dict(ia=NULL, ib=NULL, P=B + 1), dict(ia=NULL, ib=NULL, Ba=B + 1), dict(ia=NULL, ib=NULL, Bb=B + 1),
        dict(primes=0), dict(primes=4),
        dict(P=big), dict(Ba=big), dict(Bb=big),
        dict(A0=dptr(a0, 4)), dict(A1=dptr(a1, 8)), dict(B0=dptr(b0, 12)), dict(B1=dptr(b1, 4)), dict(O0=dptr(o0, 4)),
        dict(O1=dptr(o1, 8)), dict(O2=dptr(o2, 12))])
    assert call(P=0) == 0
    assert_untouched(o0, o1, o2)
    assert_untouched(st, fill=77)
    assert call() == 0 and call(ia=NULL, ib=NULL) == 0
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(o0)) == 0 and int(torch.count_nonzero(o1)) == 0 and int(torch.count_nonzero(o2)) == 0
    assert bool((st == 1).all())
    ctx.close()


# ---- test 2: the degree-2 decrypt -----------------------------------------------------------------------------------
def run_decrypt3(env, ctx, c0, c1, c2, primes, scale, key_idx=None):
    """decrypt3_level[_keyed] into outputs pre-filled with -7 (status: 77)."""
    torch = env["torch"]
    B, n = c0.shape[0], ctx.n
    out = dict(pte=torch.full((B, n), -7, dtype=torch.int64, device=env["dev"]),
               values=torch.full((B, n // 2), -7.0, dtype=torch.float32, device=env["dev"]),
               values_f64=torch.full((B, n // 2), -7.0, dtype=torch.float64, device=env["dev"]),
               status=torch.full((B,), 77, dtype=torch.uint8, device=env["dev"]))
    if key_idx is None:
        ctx.decrypt3_level(c0, c1, c2, primes, scale, **out)
    else:
        ctx.decrypt3_level_keyed(c0, c1, c2, key_idx, primes, scale, **out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("primes", [3, 2])
def test_decrypt3_zero_c2_is_decrypt_level(env, primes):
    """Test 2a: with an all-zero c2 slab every output has the bytes of decrypt_level, 4096 x 3 at primes 3 and 2."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 4
    ctx = env["pkg"].Context(n, npr)
    ctx.set_secret_key(V.secret_key(n))
    c0, c1, _, st = encrypt_sym(env, ctx, V.bench_values(B, n, first=90), first=90)
    assert bool((st == 1).all())
    l0, l1 = c0[:, :primes].contiguous(), c1[:, :primes].contiguous()
    scale = ctx.scale() * 1.25
    ref = run_decrypt(env, ctx, l0, l1, primes, scale)
    got = run_decrypt3(env, ctx, l0, l1, torch.zeros_like(l0), primes, scale)
    assert bool((ref["status"] == 1).all())
    for f in ("pte", "values", "values_f64", "status"):
        assert same_bytes(got[f], ref[f]), f
    ctx.close()


PAIRS_A, PAIRS_B = [0, 0, 1], [1, 0, 1]


@pytest.fixture(scope="module")
def product_cases(env):
    """Per shape, computed once: two symmetric records with slot values uniform in [-1, 1], their tensor for the pairs
    (0, 1), (0, 0), (1, 1), and the exact integer negacyclic products of the plaintexts the encryptor reported."""
    from oracle.pyoracle import Oracle
    cache = {}

    def get(shape):
        if shape in cache:
            return cache[shape]
        n, npr = shape
        o = Oracle(n, npr)
        ctx = env["pkg"].Context(n, npr)
        sk = V.secret_key(n)
        ctx.set_secret_key(sk)
        vals = unit_values(2, n, 1000 + n)
        c0, c1, pte, st = encrypt_sym(env, ctx, vals, first=120)
        assert bool((st == 1).all())
        t, tst = run_tensor(env, ctx, c0, c1, c0, c1, PAIRS_A, PAIRS_B)
        assert (tst == 1).all()
        m = pte.cpu().numpy()
        Q = 1
        for qj in o.q:
            Q *= qj
        prods = []
        for a, b in zip(PAIRS_A, PAIRS_B):
            # n . max|x| . max|y| < Q / 2: the centred CRT value of the per-prime products IS the integer product
            assert n * int(np.abs(m[a]).max()) * int(np.abs(m[b]).max()) < Q // 2
            pts = []
            for j, qj in enumerate(o.q):
                fa = o.ntt((m[a] % qj).astype(np.uint32), j).astype(np.uint64)
                fb = o.ntt((m[b] % qj).astype(np.uint32), j).astype(np.uint64)
                pts.append(o.intt(((fa * fb) % np.uint64(qj)).astype(np.uint32), j))
            y = crt_centred(o.q, pts)
            assert max(abs(v) for v in y) < 2 ** 62, "shrink the value range: a product coefficient reaches 2^62"
            prods.append(np.array(y, dtype=np.int64))
        # the first product once more in plain integers (int64 convolution: every sum is below 2^62 by the assert)
        assert (negacyclic(m[PAIRS_A[0]], m[PAIRS_B[0]]) == prods[0]).all()
        cache[shape] = dict(ctx=ctx, o=o, sk=sk, vals=vals, tensor=[dev_t(env, t[k]) for k in range(3)], prods=prods)
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_decrypt3_exact_integer_identity(env, product_cases, shape):
    """Tests 2b and 2d: decrypt3_level(tensor(x, y), primes = np, scale = Delta^2).pte equals the negacyclic product of
    the two plaintexts m + e the encryptor reported, as integers; values_f64 / values equal the oracle's decode of that
    product at Delta^2 bit for bit and are within the reference's 0.1 of x (.) y (applied to the expectation first)."""
    c = product_cases(shape)
    ctx, o = c["ctx"], c["o"]
    scale = o.scale * o.scale
    got = run_decrypt3(env, ctx, *c["tensor"], ctx.np, scale)
    for p, (a, b) in enumerate(zip(PAIRS_A, PAIRS_B)):
        f64 = decode_expect(o, c["prods"][p], scale)
        exp = dict(status=1, pte=c["prods"][p], values_f64=f64, values=f64.astype(np.float32))
        assert_matches(got, p, exp, (a, b))
        want = c["vals"][a].astype(np.float64) * c["vals"][b].astype(np.float64)
        err_e = float(np.abs(exp["values"].astype(np.float64) - want).max())
        err_g = float(np.abs(got["values"][p].cpu().numpy().astype(np.float64) - want).max())
        print(f"pair ({a}, {b}): max |values - x.y| = {err_e:.3e} (expectation), {err_g:.3e} (GPU)")
        assert err_e < 0.1 and err_g < 0.1, (a, b, err_e, err_g)


def test_decrypt3_keyed_twin(env):
    """Test 2c: record b under ring key idx[b] equals the unkeyed entry with that key installed, on all four outputs;
    an index == K gives status 2 and zero outputs; no ring is SE_ERR_NO_KEY."""
    torch = env["torch"]
    pkg = env["pkg"]
    n, npr, K, B = 4096, 3, 2, 6
    ctx = pkg.Context(n, npr)
    sk, _, _ = ctx.gen_keys_batch(V.derive_seeds("d3-pk", K), V.derive_seeds("d3-ep", K),
                                  sk_seeds=V.derive_seeds("d3-sk", K))
    idx = np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32)
    ti = dev_t(env, idx)
    ss, sd = V.bench_seeds(B, first=140)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    scale = ctx.scale() ** 2
    with pytest.raises(pkg.SealEmbeddedAmdError, match="ring") as ei:
        ctx.decrypt3_level_keyed(c0, c1, c1, ti, npr, scale, status=torch.zeros(B, dtype=torch.uint8, device=env["dev"]))
    assert f"code {SE_ERR_NO_KEY}" in str(ei.value)
    ctx.set_secret_keyring(sk)
    ctx.encrypt_sym_keyed(dev_t(env, unit_values(B, n, 141)), ti, dev_t(env, ss), dev_t(env, sd), c0, c1)
    torch.cuda.synchronize()
    t, tst = run_tensor(env, ctx, c0, c1, c0, c1)          # squares: both factors under the record's key
    assert (tst == 1).all()
    d = [dev_t(env, t[k]) for k in range(3)]
    bad = idx.copy()
    bad[4] = K
    got = run_decrypt3(env, ctx, *d, npr, scale, key_idx=dev_t(env, bad))
    for k in range(K):
        sel = np.nonzero((idx == k) & (bad < K))[0]
        ts = torch.from_numpy(sel).to(env["dev"])
        ctx.set_secret_key(sk[k])
        ref = run_decrypt3(env, ctx, *(x.index_select(0, ts).contiguous() for x in d), npr, scale)
        assert bool((ref["status"] == 1).all())
        for f in ("pte", "values", "values_f64", "status"):
            assert same_bytes(got[f].index_select(0, ts), ref[f]), (k, f)
    assert int(got["status"][4]) == 2
    for f in ("pte", "values", "values_f64"):
        assert int(torch.count_nonzero(got[f][4])) == 0, f
    # the argument errors of the level entry, and the third slab
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    f3 = CEntry(ctx.L.se_amd_decrypt3_level_device, ctx=ctx.h, c0=dptr(d[0]), c1=dptr(d[1]), c2=dptr(d[2]), B=B,
                primes=npr, scale=scale, pte=NULL, values=NULL, values_f64=NULL, status=dptr(st), stream=stream_of(env))
    f3.refused([dict(c2=NULL), dict(primes=npr + 1), dict(scale=0.0)])
    assert f3(B=0) == 0
    assert_untouched(st, fill=77)
    ctx.close()


# ---- test 3: key generation -----------------------------------------------------------------------------------------
def relin_seeds(npr, label):
    return V.derive_seeds(label + "-a", 2 * npr), V.derive_seeds(label + "-e", 2 * npr)


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_relin_key_generation(env, shape):
    """Test 3: gen_relin_key equals gen_keys_batch(K = 2 np, this key replicated, the same seeds) plus the diagonal term
    computed from the oracle's NTT(s) in Python ints; the keys installed in the context are not touched; set_relin_key
    refuses a word equal to q_i and ct_relin without an installed key is SE_ERR_NO_KEY."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    pkg = env["pkg"]
    n, npr = shape
    R = 2 * npr
    o = Oracle(n, npr)
    ctx = pkg.Context(n, npr)
    sk = V.secret_key(n, seed=3)
    sa, se = relin_seeds(npr, "keygen")
    evk0, evk1 = ctx.gen_relin_key(sk, sa, se)
    _, pk0, pk1 = ctx.gen_keys_batch(sa, se, sk_in=np.tile(sk, (R, 1)))
    s_hat = ntt_secret(o, sk)
    exp0 = pk0.copy()
    for j in range(npr):
        for t in range(2):
            exp0[2 * j + t, j] = (pk0[2 * j + t, j].astype(np.uint64) + relin_diagonal(o, s_hat, j, t)) % np.uint64(o.q[j])
    assert (evk1 == pk1).all()
    assert (evk0 == exp0).all()
    assert (evk0 != pk0).any(axis=2).sum() == R            # exactly the diagonal columns changed
    # no secret key was installed by the generator
    B = 1
    slab = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    st = torch.full((B,), 77, dtype=torch.uint8, device=env["dev"])
    assert ctx.L.se_amd_decrypt_level_device(ctx.h, dptr(slab), dptr(slab), B, npr, ctx.scale(), NULL, NULL, NULL,
                                             dptr(st), stream_of(env)) == SE_ERR_NO_KEY
    # ct_relin before an install, a refused install, and ct_relin after the refused install
    out0, out1 = torch.full_like(slab, SENTINEL), torch.full_like(slab, SENTINEL)
    relin = CEntry(ctx.L.se_amd_ct_relin_device, ctx=ctx.h, d0=dptr(slab), d1=dptr(slab), d2=dptr(slab), B=B, primes=npr,
                   out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    assert relin() == SE_ERR_NO_KEY
    for which, (r, i, c) in ((0, (0, 0, 0)), (1, (R - 1, npr - 1, n - 1))):
        k0, k1 = evk0.copy(), evk1.copy()
        (k0, k1)[which][r, i, c] = o.q[i]
        with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
            ctx.set_relin_key(k0, k1)
        assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    assert relin() == SE_ERR_NO_KEY
    ctx.set_relin_key(evk0, evk1)
    assert relin() == 0
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(out0)) == 0 and int(torch.count_nonzero(out1)) == 0     # the zero slabs relinearise to zero
    assert_untouched(st, fill=77)
    ctx.close()


# ---- test 4: the relinearisation on arbitrary slabs and key words ---------------------------------------------------
def digit_edge_row(o, j, rng):
    """NTT form of natural-order coefficients that hold both sides of the digit boundary -- 0, 2^15 - 1, 2^15,
    2^15 + 1 -- and q - 1, beside random values."""
    q = o.q[j]
    c = rng.integers(0, q, o.n, dtype=np.uint32)
    edges = np.array([0, DIGIT_MASK, DIGIT_MASK + 1, DIGIT_MASK + 2, q - 1], dtype=np.uint32)
    c[::7] = np.resize(edges, c[::7].shape)
    c[-5:] = edges
    row = o.ntt(c, j)
    assert (o.intt(row, j) == c).all()
    return row


RELIN_CASES = [((1024, 1), (1,)), ((4096, 2), (2,)), ((4096, 3), (3, 2)), ((8192, 6), (6,)), ((16384, 13), (13,))]


@pytest.mark.parametrize("shape,levels", RELIN_CASES, ids=lambda v: "x".join(map(str, v)))
def test_relin_arbitrary_slabs_and_key(env, shape, levels):
    """Test 4: random residues for the three slabs and for the installed key (B = 3; record 2 of d2 holds the digit
    boundaries), against the definition; a lower level uses the rows r < 2L and columns i < L of the same key; the
    sentinels behind the outputs survive.  No secret key is installed."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    B, R = 3, 2 * npr
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    q = o.q
    rng = np.random.default_rng(31 * n + npr)
    evk0 = np.stack([rand_slab(rng, q, 1, n)[0] for _ in range(R)])
    evk1 = np.stack([rand_slab(rng, q, 1, n)[0] for _ in range(R)])
    evk0[0, 0, :4] = [0, 1, q[0] - 1, q[0] - 1]
    ctx.set_relin_key(evk0, evk1)
    for L in levels:
        d0, d1, d2 = (rand_slab(rng, q, B, n, L) for _ in range(3))
        for j in range(L):
            d2[2, j] = digit_edge_row(o, j, rng)
        d0[1] = d1[1] = (np.array(q[:L], dtype=np.uint32) - 1)[:, None]
        e0, e1 = relin_expect(o, d0, d1, d2, evk0, evk1)
        g0, g1 = run_relin(env, ctx, dev_t(env, d0), dev_t(env, d1), dev_t(env, d2), L)
        assert (g0 == e0).all() and (g1 == e1).all(), L
    ctx.close()


def test_refused_relin_key_leaves_the_installed_one(env):
    """The replacement rule of the evaluation keys, on the relinearisation key (1024 x 1, B = 2): with key A installed,
    a key with one word equal to q_0 is refused as an invalid argument, and ct_relin afterwards still gives the
    definition under key A."""
    from oracle.pyoracle import Oracle
    pkg = env["pkg"]
    n, npr, B = 1024, 1, 2
    o = Oracle(n, npr)
    ctx = pkg.Context(n, npr)
    rng = np.random.default_rng(77)
    evk0, evk1 = (np.stack([rand_slab(rng, o.q, 1, n)[0] for _ in range(2 * npr)]) for _ in range(2))
    ctx.set_relin_key(evk0, evk1)
    bad = evk1.copy()
    bad[1, 0, n // 2] = o.q[0]
    with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
        ctx.set_relin_key(evk0, bad)
    assert f"code {SE_ERR_INVALD_ARGUMENT}" in str(ei.value)
    d0, d1, d2 = (rand_slab(rng, o.q, B, n) for _ in range(3))
    e0, e1 = relin_expect(o, d0, d1, d2, evk0, evk1)
    g0, g1 = run_relin(env, ctx, dev_t(env, d0), dev_t(env, d1), dev_t(env, d2), npr)
    assert (g0 == e0).all() and (g1 == e1).all()
    ctx.close()


def test_relin_arguments(env):
    """The argument errors return -22 and write nothing; B = 0 is a successful no-op."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 2
    ctx = env["pkg"].Context(n, npr)
    key = np.zeros((2 * npr, npr, n), dtype=np.uint32)
    ctx.set_relin_key(key, key)
    d0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    d1, d2 = torch.zeros_like(d0), torch.zeros_like(d0)
    out0 = torch.full((B, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    f = CEntry(ctx.L.se_amd_ct_relin_device, ctx=ctx.h, d0=dptr(d0), d1=dptr(d1), d2=dptr(d2), B=B, primes=3,
               out0=dptr(out0), out1=dptr(out1), stream=stream_of(env))
    f.refused([
        dict(ctx=None),
        dict(d0=NULL),                                                 # NULL mandatory pointers
        dict(d1=NULL),
        dict(d2=NULL),
        dict(out0=NULL),
        dict(out1=NULL),
        dict(primes=0),                                                # primes outside [1, np]
        dict(primes=4),
        dict(B=2 ** 32),                                               # B >= 2^32
        dict(d0=dptr(d0, 4)),                                          # alignment, each slab
        dict(d1=dptr(d1, 8)),
        dict(d2=dptr(d2, 12)),
        dict(out0=dptr(out0, 4)),
        dict(out1=dptr(out1, 8)),
    ])
    assert f(B=0) == 0
    assert_untouched(out0, out1)
    # a level-2 call writes B . 2 . n words and nothing behind them
    assert f(primes=2) == 0
    assert_zero_prefix(out0, B * 2 * n)
    ctx.close()


# ---- tests 5 and 6: a real key ---------------------------------------------------------------------------------------
def fill_keyed_case(env, case):
    """What keyed_cases (gpu_support) holds per shape beside the context and its secret key: the relinearisation key,
    installed; B = 4 records with slot values in [-1, 1], the tensor of the pairs (b, b + 1 mod B) and its
    relinearisation."""
    ctx, sk = case["ctx"], case["sk"]
    n, npr, B = ctx.n, ctx.np, 4
    evk0, evk1 = ctx.gen_relin_key(sk, *relin_seeds(npr, "e2e"))
    ctx.set_relin_key(evk0, evk1)
    vals = unit_values(B, n, 2000 + n)
    c0, c1 = fresh_records(env, ctx, vals, 160)
    ia, ib = list(range(B)), [(b + 1) % B for b in range(B)]
    t, tst = run_tensor(env, ctx, c0, c1, c0, c1, ia, ib)
    assert (tst == 1).all()
    r0, r1 = run_relin(env, ctx, *(dev_t(env, t[k]) for k in range(3)), npr)
    case.update(evk0=evk0, evk1=evk1, vals=vals, ia=ia, ib=ib, tensor=t, relin=(r0, r1))


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_relin_exact_key_switch_identity(env, keyed_cases, shape):
    """Test 5: with y3 the oracle's centred degree-2 value of (d0, d1, d2), y2 the oracle expectation of the relinearised
    pair and e_r the key's errors recovered with the oracle (centred INTT of evk0 + evk1 . s_hat - diagonal),
    y2 - y3 == sum_r negacyclic(D_r, e_r) as integers, for every coefficient.  No model of the kernel enters."""
    c = keyed_cases(shape)
    o, s_hat, npr = c["o"], c["s_hat"], c["o"].np
    errs = digit_key_errors(o, c["evk0"], c["evk1"], s_hat, lambda j, t: relin_diagonal(o, s_hat, j, t))
    d0, d1, d2 = c["tensor"]
    for p in range(2):
        pts = [o.intt(o.decrypt(d0[p, j], o.decrypt(d1[p, j], d2[p, j], s_hat[j], j), s_hat[j], j), j)
               for j in range(npr)]
        y3 = np.array(crt_centred(o.q, pts), dtype=object)
        e = expectation(o, c["relin"][0][p], c["relin"][1][p], s_hat)
        y2 = np.array(e["y"], dtype=object)
        D = digits_of(o, d2[p], npr)
        ks = np.zeros(o.n, dtype=np.int64)
        for dig, er in zip(D, errs):
            ks += negacyclic(dig.astype(np.int64), er)         # n . 2^15 . 64 per term: far below 2^62
        assert ((y2 - y3) == ks.astype(object)).all(), p
        print(f"pair {p}: max |key-switch term| = {int(np.abs(ks).max())}")


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=SHAPE_IDS)
def test_product_end_to_end(env, keyed_cases, shape):
    """Test 6: tensor -> relin -> rescale -> decrypt_level(primes = np - 1, scale = Delta^2 / q_last) on B = 4 pairs of
    records with slot values in [-1, 1]: every stage equals its definition, the final pte / values / values_f64 equal
    the oracle's on the final records bit for bit, and the result is within the reference's 0.1 of x (.) y (applied to
    the expectation first).  The worst error is printed (a CPU simulation of the same chain on records of the same
    distribution, tools/ct_mul_noise_sim.py, puts it at 3.0e-3 for 4096 x 3 and 8.3e-3 for 8192 x 6, of which the
    key-switch term contributes 8.6e-6 and 6.7e-5; the rest is the rescale's rounding)."""
    from oracle.pyoracle import Oracle
    c = keyed_cases(shape)
    ctx, o = c["ctx"], c["o"]
    n, npr = shape
    lo = Oracle(n, npr - 1)
    r0, r1 = c["relin"]
    e0, e1 = relin_expect(o, *(c["tensor"][k][:2] for k in range(3)), c["evk0"], c["evk1"])
    assert (r0[:2] == e0).all() and (r1[:2] == e1).all()
    f0, f1 = rescale_records(env, ctx, o, r0, r1, npr)
    scale = o.scale * o.scale / o.q[npr - 1]
    v64 = c["vals"].astype(np.float64)
    check_level_decrypt(env, ctx, lo, f0, f1, c["s_hat"], npr - 1, scale, v64[c["ia"]] * v64[c["ib"]], "x.y")


# ---- test 7: the example --------------------------------------------------------------------------------------------
def test_ct_product_example(env, tmp_path):
    """examples/ct_product_roundtrip.c from plain gcc: squares through the tensor, relin, a plain sum, rescale and
    decrypt_level come back within the reference's 0.1 of sum v^2."""
    run_example("ct_product_roundtrip", tmp_path, ("4096", "3", "16"))
