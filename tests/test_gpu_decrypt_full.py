"""Full-modulus decrypt and decode (-m gpu): se_amd_decrypt_full_device recombines all primes of a ciphertext on the GPU.
Every expectation is built from the oracle's primitives (decrypt, intt, fft) and Python integers, never from the code
under test; every comparison is bit-exact except the reference's own acceptance criterion |values - input| < 0.1
(device/test/ckks_tests_common.c:132).  The constructed records at the end (tests/recv_model.py) are planted Python integers,
one for every branch of the recombination: the record's own integers are the expectation."""
import numpy as np
import pytest

import vectors as V
from ct_model import CASE_IDS
from gpu_support import (NULL, SE_ERR_NO_KEY, CEntry, assert_matches, bits, decode_expect, dev_t, dptr,  # noqa: F401
                         encrypt_sym, env, expectation, host_u32, ntt_secret, records, run_decrypt, run_example,
                         stream_of)
from recv_model import SHAPES as RECV_SHAPES
from recv_model import ciphertext_of, expect_at_level, in_range_vectors, out_of_range_vectors

pytestmark = pytest.mark.gpu

SHAPES = V.ALL_SHAPES + [(16384, 13), (4096, 2)]


@pytest.fixture(scope="module")
def sym_cases(env):
    """Per shape, computed once: the six records encrypted on the GPU, the new entry's outputs and the expectation."""
    cache = {}

    def get(shape):
        if shape in cache:
            return cache[shape]
        from oracle.pyoracle import Oracle
        n, npr = shape
        ctx = env["pkg"].Context(n, npr)
        sk = V.secret_key(n)
        ctx.set_secret_key(sk)
        recs = records(n)
        vals = np.stack([v for _, v in recs]).astype(np.float32)
        c0, c1, enc_pte, enc_st = encrypt_sym(env, ctx, vals)
        assert bool((enc_st == 1).all()), "every record encodes (|m| < 2^63)"
        got = run_decrypt(env, ctx, c0, c1)
        o = Oracle(n, npr)
        s_hat = ntt_secret(o, sk)
        h0, h1 = host_u32(c0), host_u32(c1)
        exp = [expectation(o, h0[b], h1[b], s_hat) for b in range(len(recs))]
        cache[shape] = dict(ctx=ctx, o=o, recs=recs, vals=vals, c0=c0, c1=c1, enc_pte=enc_pte, got=got, exp=exp)
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_parity_sym(env, sym_cases, shape):
    """Test 1: pte, values, values_f64 and status equal the oracle + Python-int CRT expectation, bit for bit."""
    torch = env["torch"]
    n, npr = shape
    c = sym_cases(shape)
    got, exp = c["got"], c["exp"]
    for b, (name, v) in enumerate(c["recs"]):
        assert_matches(got, b, exp[b], (shape, name))
        if exp[b]["status"] == 1 and npr >= 3:
            # Q > 2^64: the recombined integer is the plaintext the encryption entry reports
            assert torch.equal(got["pte"][b], c["enc_pte"][b]), (shape, name)
        if npr >= 2 and name in ("bench", "pattern8x100"):
            # the reference's acceptance criterion, first on the expectation, then on the GPU result
            assert exp[b]["status"] == 1
            assert np.abs(exp[b]["values"] - v).max() < 0.1, (shape, name)
            assert np.abs(got["values"][b].cpu().numpy() - v).max() < 0.1, (shape, name)
    if npr >= 3:
        # the four rows of the issue's table fit int64 and Q/2 on these shapes
        assert all(exp[b]["status"] == 1 for b in range(4)), shape


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_agrees_with_single_prime_entry(env, sym_cases, shape):
    """Test 2: where the plaintext fits one prime (and always on the one-prime shapes) the new entry's values are
    bit-identical to se_amd_decrypt_decode_device for every prime."""
    torch = env["torch"]
    n, npr = shape
    c = sym_cases(shape)
    ctx, o = c["ctx"], c["o"]
    qualifying = 0
    for b, (name, _) in enumerate(c["recs"]):
        e = c["exp"][b]
        if npr > 1 and not (e["status"] == 1 and max(abs(v) for v in e["y"]) < min(o.q) / 2):
            continue
        qualifying += 1
        for j in range(npr):
            out = torch.zeros((1, n // 2), dtype=torch.float32, device=env["dev"])
            ctx.decrypt_decode(c["c0"][b:b + 1].contiguous(), c["c1"][b:b + 1].contiguous(), j, None, None, out)
            torch.cuda.synchronize()
            assert torch.equal(out[0].view(torch.int32), c["got"]["values"][b].view(torch.int32)), (shape, name, j)
    assert qualifying >= 2, (shape, qualifying)


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6), (16384, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_parity_public_key(env, shape):
    """Test 3: public-key ciphertexts (pte = m + e0 + e1.s + ep.u): oracle parity, decode within 0.1 for bench_values."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    ctx = env["pkg"].Context(n, npr)
    sk, pk0, pk1 = ctx.gen_keys_batch(V.derive_seeds("full-pk", 1), V.derive_seeds("full-ep", 1),
                                      sk_seeds=V.derive_seeds("full-sk", 1))
    ctx.set_secret_key(sk[0])
    ctx.set_public_key(pk0[0], pk1[0])
    recs = records(n)
    vals = np.stack([v for _, v in recs]).astype(np.float32)
    B = vals.shape[0]
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encrypt_asym(dev_t(env, vals), dev_t(env, V.derive_seeds("full-enc", B)), c0, c1, status=st)
    torch.cuda.synchronize()
    assert bool((st == 1).all())
    got = run_decrypt(env, ctx, c0, c1)
    o = Oracle(n, npr)
    s_hat = ntt_secret(o, sk[0])
    h0, h1 = host_u32(c0), host_u32(c1)
    for b, (name, v) in enumerate(recs):
        e = expectation(o, h0[b], h1[b], s_hat)
        assert_matches(got, b, e, (shape, name))
        if name == "bench":
            assert e["status"] == 1
            assert np.abs(e["values"] - v).max() < 0.1
            assert np.abs(got["values"][b].cpu().numpy() - v).max() < 0.1
    ctx.close()


def test_wrong_key_is_flagged(env):
    """Test 4(a): a record decrypted under another key recombines to a uniformly random residue vector."""
    from oracle.pyoracle import Oracle
    n, npr = 4096, 3
    ctx = env["pkg"].Context(n, npr)
    ctx.set_secret_key(V.secret_key(n, seed=1))
    c0, c1, _, _ = encrypt_sym(env, ctx, V.bench_values(2, n))
    other = V.secret_key(n, seed=2)
    ctx.set_secret_key(other)
    got = run_decrypt(env, ctx, c0, c1)
    o = Oracle(n, npr)
    s_hat = ntt_secret(o, other)
    h0, h1 = host_u32(c0), host_u32(c1)
    for b in range(2):
        e = expectation(o, h0[b], h1[b], s_hat)
        assert e["status"] == 0
        assert int(got["status"][b]) == e["status"], b
    ctx.close()


@pytest.mark.parametrize("shape", [(4096, 3), (16384, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_int64_boundary(env, shape):
    """Test 4(b): c1 = 0, c0_j = NTT(v mod q_j).  Record 0 holds one coefficient 2^63 (just outside), record 1 holds
    2^63 - 1 and -2^63 (just inside) among smaller values of both signs."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    ctx.set_secret_key(V.secret_key(n))
    rng = np.random.default_rng(n + npr)
    base = [int(x) for x in rng.integers(-2 ** 62, 2 ** 62, n)]
    base[:6] = [0, 1, -1, o.q[0] // 2, -(o.q[0] // 2) - 1, -(2 ** 40)]
    v_out, v_in = list(base), list(base)
    v_out[n // 3] = 2 ** 63
    v_in[n // 3] = 2 ** 63 - 1
    v_in[n - 1] = -2 ** 63
    c0 = np.zeros((2, npr, n), dtype=np.uint32)
    for b, v in enumerate((v_out, v_in)):
        for j in range(npr):
            c0[b, j] = o.ntt(np.array([x % o.q[j] for x in v], dtype=np.uint32), j)
    got = run_decrypt(env, ctx, dev_t(env, c0), dev_t(env, np.zeros_like(c0)))
    assert int(got["status"][0]) == 0
    assert int(got["status"][1]) == 1
    assert (got["pte"][1].cpu().numpy() == np.array(v_in, dtype=np.int64)).all()
    ctx.close()


@pytest.mark.parametrize("shape", [(1024, 1), (2048, 1), (4096, 3), (8192, 6), (16384, 6)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_keyed_equals_unkeyed(env, shape):
    """Test 5: record b under ring key idx[b] equals the unkeyed entry with that key installed, on all four outputs;
    an index == K gives status 2 and zero outputs; no ring is SE_ERR_NO_KEY."""
    torch = env["torch"]
    pkg = env["pkg"]
    n, npr = shape
    K, B = 5, 64
    ctx = pkg.Context(n, npr)
    sk, _, _ = ctx.gen_keys_batch(V.derive_seeds("fullring-pk", K), V.derive_seeds("fullring-ep", K),
                                  sk_seeds=V.derive_seeds("fullring-sk", K))
    rng = np.random.default_rng(5)
    idx = rng.integers(0, K, size=B).astype(np.uint32)
    idx[B // 2] = K - 1
    idx[0] = idx[1]
    vals = V.bench_values(B, n, first=21)
    vals[3] *= 1.0e4                        # beyond one prime
    ss, sd = V.bench_seeds(B, first=21)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    ti = dev_t(env, idx)
    with pytest.raises(pkg.SealEmbeddedAmdError, match="ring") as ei:
        ctx.decrypt_full_keyed(c0, c1, ti, status=torch.zeros(B, dtype=torch.uint8, device=env["dev"]))
    assert f"code {SE_ERR_NO_KEY}" in str(ei.value)
    ctx.set_secret_keyring(sk)
    ctx.encrypt_sym_keyed(dev_t(env, vals), ti, dev_t(env, ss), dev_t(env, sd), c0, c1)
    torch.cuda.synchronize()
    bad = idx.copy()
    bad[7] = K
    got = run_decrypt(env, ctx, c0, c1, key_idx=dev_t(env, bad))
    for k in np.unique(idx):
        sel = np.nonzero((idx == k) & (bad < K))[0]
        ts = torch.from_numpy(sel).to(env["dev"])
        ctx.set_secret_key(sk[int(k)])
        ref = run_decrypt(env, ctx, c0.index_select(0, ts).contiguous(), c1.index_select(0, ts).contiguous())
        assert bool((ref["status"] == 1).all())
        for f in ("pte", "status"):
            assert torch.equal(got[f].index_select(0, ts), ref[f]), (int(k), f)
        assert torch.equal(got["values"].index_select(0, ts).view(torch.int32), ref["values"].view(torch.int32)), int(k)
        assert torch.equal(got["values_f64"].index_select(0, ts).view(torch.int64),
                           ref["values_f64"].view(torch.int64)), int(k)
    assert int(got["status"][7]) == 2
    for f in ("pte", "values", "values_f64"):
        assert int(torch.count_nonzero(got[f][7])) == 0, f
    ctx.close()


def test_optional_outputs_and_arguments(env):
    """Test 6: each output alone gives the bytes of the all-outputs call; argument errors; B = 0."""
    torch = env["torch"]
    pkg = env["pkg"]
    n, npr, B = 4096, 3, 5
    ctx = pkg.Context(n, npr)
    L = ctx.L
    stream = stream_of(env)
    vals = V.bench_values(B, n, first=9)
    vals[2] *= 300.0
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    # no secret key yet
    assert L.se_amd_decrypt_full_device(ctx.h, dptr(c0), dptr(c1), B, NULL, NULL, NULL, dptr(st),
                                        stream) == SE_ERR_NO_KEY
    ctx.set_secret_key(V.secret_key(n))
    c0, c1, _, _ = encrypt_sym(env, ctx, vals, first=9)
    full = run_decrypt(env, ctx, c0, c1)
    for f in ("pte", "values", "values_f64", "status"):
        alone = run_decrypt(env, ctx, c0, c1, want=(f,))
        assert alone[f].cpu().numpy().tobytes() == full[f].cpu().numpy().tobytes(), f
        for g in ("pte", "values", "values_f64", "status"):
            if g != f:      # an output that was not requested is not written
                assert alone[g].cpu().numpy().tobytes() != full[g].cpu().numpy().tobytes(), (f, g)
    f = CEntry(L.se_amd_decrypt_full_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, pte=NULL, values=NULL,
               values_f64=NULL, status=dptr(st), stream=stream)
    f.refused([dict(status=NULL), dict(c0=NULL), dict(c1=NULL), dict(ctx=None)])
    assert f(B=0) == 0
    # keyed twin
    sk, _, _ = ctx.gen_keys_batch(V.derive_seeds("arg-pk", 2), V.derive_seeds("arg-ep", 2),
                                  sk_seeds=V.derive_seeds("arg-sk", 2))
    ctx.set_secret_keyring(sk)
    ki = torch.zeros(B, dtype=torch.int32, device=env["dev"])
    fk = CEntry(L.se_amd_decrypt_full_keyed_device, ctx=ctx.h, c0=dptr(c0), c1=dptr(c1), B=B, key_idx=dptr(ki), pte=NULL,
                values=NULL, values_f64=NULL, status=dptr(st), stream=stream)
    fk.refused([dict(status=NULL), dict(key_idx=NULL), dict(c0=NULL)])
    assert fk(B=0) == 0
    assert fk() == 0
    torch.cuda.synchronize()
    ctx.close()


def test_full_size(env):
    """Test 7: 4096 x 3, B = 65 536, the C2 inputs: pte equals the encryption's d_pte for every record, every status
    is 1, and a strided sample of 256 records matches the oracle expectation for values."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 4096, 3, 65536
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    vals = V.bench_values(B, n)
    c0, c1, enc_pte, st = encrypt_sym(env, ctx, vals)
    assert bool((st == 1).all())
    pte = torch.zeros((B, n), dtype=torch.int64, device=env["dev"])
    values = torch.zeros((B, n // 2), dtype=torch.float32, device=env["dev"])
    status = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.decrypt_full(c0, c1, pte=pte, values=values, status=status)
    torch.cuda.synchronize()
    assert torch.equal(pte, enc_pte)
    assert bool((status == 1).all())
    o = Oracle(n, npr)
    s_hat = ntt_secret(o, sk)
    sample = list(range(0, B, B // 256))
    assert len(sample) == 256
    ts = torch.tensor(sample, device=env["dev"])
    h0, h1 = host_u32(c0.index_select(0, ts)), host_u32(c1.index_select(0, ts))
    gv = values.index_select(0, ts).cpu().numpy()
    for i, b in enumerate(sample):
        e = expectation(o, h0[i], h1[i], s_hat)
        assert e["status"] == 1
        assert (bits(gv[i]) == bits(e["values"])).all(), b
    ctx.close()


def test_roundtrip_example(env, tmp_path):
    """examples/batch_roundtrip.c from plain gcc: values around +-1000 come back within the reference's 0.1."""
    run_example("batch_roundtrip", tmp_path, ("4096", "3", "16"))


# ---- constructed plaintexts: every branch of the recombination decides a record (tests/recv_model.py) ---------------------
LEVELS = {(4096, 3): (1, 2, 3), (8192, 6): (1, 2, 3, 4, 5, 6), (16384, 13): (1, 2, 3, 4, 8, 12, 13)}


@pytest.fixture(scope="module")
def recv_cases(env):
    """recv_cases(shape) -> computed once and left unchanged: a context with one secret key installed, the oracle, the
    named vectors (the first n_in in range, the rest out of range) and host slabs c0, c1 [B][np][n] that decrypt to them."""
    from oracle.pyoracle import Oracle
    cache = {}

    def get(shape):
        if shape not in cache:
            n, npr = shape
            o = Oracle(n, npr)
            ctx = env["pkg"].Context(n, npr)
            sk = V.secret_key(n, seed=3)
            ctx.set_secret_key(sk)
            s_hat = ntt_secret(o, sk)
            inside = in_range_vectors(o)
            named = inside + ([(r["name"], r["vec"]) for r in out_of_range_vectors(o)] if npr >= 3 else [])
            rng = np.random.default_rng(31 * n + npr)
            rows = [ciphertext_of(o, vec, s_hat, rng) for _, vec in named]
            cache[shape] = dict(ctx=ctx, o=o, named=named, n_in=len(inside), c0=np.stack([r[0] for r in rows]),
                                c1=np.stack([r[1] for r in rows]))
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()


def assert_planted(got, b, o, y, what, scale=None):
    """Record b has status 1, pte equal to the Python integers y and values_f64 / values bit-equal to the oracle's decode
    of them."""
    pte = np.array(y, dtype=np.int64)
    f64 = decode_expect(o, pte, scale)
    assert_matches(got, b, dict(status=1, pte=pte, values_f64=f64, values=f64.astype(np.float32)), what)


@pytest.mark.parametrize("shape", RECV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_constructed_in_range(env, recv_cases, shape):
    """The in-range records: zero, and every multiple and half-way point of the primes and of q_0 q_1 with both ends of
    int64 (np <= 2: of the centred range of Q), each held by a low and by a high thread.  Status 1, pte the planted
    integers, both decodes bit-equal to the oracle's decode of them."""
    c = recv_cases(shape)
    k = c["n_in"]
    got = run_decrypt(env, c["ctx"], dev_t(env, c["c0"][:k]), dev_t(env, c["c1"][:k]))
    for b, (name, vec) in enumerate(c["named"][:k]):
        assert_planted(got, b, c["o"], vec, (shape, name))


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6), (16384, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_constructed_out_of_range(env, recv_cases, shape):
    """Every out-of-range record (ONE coefficient outside int64, decided at the prime recv_model names, at a rotating
    position) has status 0; the in-range records interleaved in the same call keep status 1 and their exact outputs."""
    c = recv_cases(shape)
    k, B = c["n_in"], len(c["named"])
    order = []
    for i, b in enumerate(range(k, B)):
        if i % 2 == 0:
            order.append((i // 2) % k)
        order.append(b)
    order.append(0)
    assert len(order) <= 40
    got = run_decrypt(env, c["ctx"], dev_t(env, c["c0"][order]), dev_t(env, c["c1"][order]))
    for at, b in enumerate(order):
        name, vec = c["named"][b]
        if b < k:
            assert_planted(got, at, c["o"], vec, (shape, at, name))
        else:
            assert int(got["status"][at]) == 0, (shape, at, name)


@pytest.mark.parametrize("shape,p", [(s, p) for s in LEVELS for p in LEVELS[s]], ids=CASE_IDS)
def test_levels_cut_the_recombination(env, recv_cases, shape, p):
    """decrypt_level with primes = p on the first p rows of the full-chain slab stops after p primes: status and, where
    it is 1, pte and the decodes are those of the coefficients' centred representatives mod q_0 ... q_{p-1}.  A record
    12345 + q_0 ... q_{j-1} is 12345 at level j and out of range from level j + 1 on."""
    c = recv_cases(shape)
    o, ctx = c["o"], c["ctx"]
    got = run_decrypt(env, ctx, dev_t(env, c["c0"][:, :p]), dev_t(env, c["c1"][:, :p]), primes=p)
    seen = set()
    for b, (name, vec) in enumerate(c["named"]):
        status, y = expect_at_level(o, vec, p)
        seen.add(status)
        if status == 1:
            assert_planted(got, b, o, y, (shape, p, name), ctx.scale())
        else:
            assert int(got["status"][b]) == 0, (shape, p, name)
    assert seen == ({1} if p <= 2 else {0, 1}), (shape, p)


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_constructed_keyed_and_degree2(env, shape):
    """The same vectors through decrypt_full_keyed, decrypt3_level and decrypt3_level_keyed: record b is built under key
    b mod 3 of a ring of three distinct keys (degree 2: c0 = m - c1 s - c2 s^2 with random c1, c2), the unkeyed degree-2
    records under the installed key.  The expectations are the planted integers; a last record with index K comes back
    with status 2 and zeros."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    K = 3
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    sks = [V.secret_key(n, seed=s) for s in (11, 12, 13)]
    assert len({sk.tobytes() for sk in sks}) == K
    s_hats = [ntt_secret(o, sk) for sk in sks]
    ctx.set_secret_keyring(np.stack(sks))
    ctx.set_secret_key(sks[1])
    inside = in_range_vectors(o)
    named = inside + [(r["name"], r["vec"]) for r in out_of_range_vectors(o)]
    B = len(named)
    idx = np.arange(B + 1, dtype=np.uint32) % K
    idx[B] = K
    rng = np.random.default_rng(7 * n + npr)
    source = list(range(B)) + [0]                       # the rejected record is a copy of record 0's vector

    def slabs(degree, key_of):
        rows = [ciphertext_of(o, named[b][1], s_hats[key_of(at)], rng, degree) for at, b in enumerate(source)]
        return [dev_t(env, np.stack([r[i] for r in rows])) for i in range(degree + 1)]

    def check(got, what, rejected):
        for b, (name, vec) in enumerate(named):
            if b < len(inside):
                assert_planted(got, b, o, vec, (shape, what, name))
            else:
                assert int(got["status"][b]) == 0, (shape, what, name)
        if rejected:
            assert int(got["status"][B]) == 2, what
            for f in ("pte", "values", "values_f64"):
                assert int(torch.count_nonzero(got[f][B])) == 0, (what, f)
        else:
            assert_planted(got, B, o, named[0][1], (shape, what, "copy of record 0"))

    ring_key = lambda at: int(idx[at]) % K  # noqa: E731  (the rejected record is built under key 0)
    ti = dev_t(env, idx)
    c0, c1 = slabs(1, ring_key)
    check(run_decrypt(env, ctx, c0, c1, key_idx=ti), "full_keyed", True)
    c0, c1, c2 = slabs(2, ring_key)
    check(run_decrypt(env, ctx, c0, c1, key_idx=ti, c2=c2), "decrypt3_level_keyed", True)
    c0, c1, c2 = slabs(2, lambda at: 1)
    check(run_decrypt(env, ctx, c0, c1, c2=c2), "decrypt3_level", False)
    ctx.close()


@pytest.mark.parametrize("shape", [(4096, 3), (1024, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_zero_record_single_prime_entry(env, recv_cases, shape):
    """The zero record (c0 = -c1 s with random c1: every word of c0 + c1 s is q or 0 before the reduction) through
    se_amd_decrypt_decode_device, for every prime: dec_ntt, pt and values are all zero."""
    torch = env["torch"]
    n, npr = shape
    c = recv_cases(shape)
    b = [name for name, _ in c["named"]].index("zero")
    assert not any(c["named"][b][1]) and c["c1"][b].any()
    c0, c1 = dev_t(env, c["c0"][b:b + 1]), dev_t(env, c["c1"][b:b + 1])
    for j in range(npr):
        dec_ntt = torch.full((1, n), 0x5A5A5A5A, dtype=torch.int32, device=env["dev"])
        pt = torch.full_like(dec_ntt, 0x5A5A5A5A)
        values = torch.full((1, n // 2), -7.0, dtype=torch.float32, device=env["dev"])
        c["ctx"].decrypt_decode(c0, c1, j, dec_ntt, pt, values)
        torch.cuda.synchronize()
        for name, t in (("dec_ntt", dec_ntt), ("pt", pt), ("values", values)):
            assert int(torch.count_nonzero(t)) == 0, (shape, j, name)
