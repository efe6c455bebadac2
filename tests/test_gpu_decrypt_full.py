"""Full-modulus decrypt and decode (-m gpu): se_amd_decrypt_full_device recombines all primes of a ciphertext on the GPU.
Every expectation is built from the oracle's primitives (decrypt, intt, fft) and Python integers, never from the code
under test; every comparison is bit-exact except the reference's own acceptance criterion |values - input| < 0.1
(device/test/ckks_tests_common.c:132)."""
import ctypes as C

import numpy as np
import pytest

import vectors as V
from gpu_support import (SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY, assert_matches, bits, dev_t, encrypt_sym, env,  # noqa: F401
                         expectation, host_u32, ntt_secret, records, run_decrypt, run_example, stream_of)

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
    z = C.c_void_p(None)
    stream = stream_of(env)
    vals = V.bench_values(B, n, first=9)
    vals[2] *= 300.0
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    p = lambda t: C.c_void_p(t.data_ptr())
    # no secret key yet
    assert L.se_amd_decrypt_full_device(ctx.h, p(c0), p(c1), B, z, z, z, p(st), stream) == SE_ERR_NO_KEY
    ctx.set_secret_key(V.secret_key(n))
    c0, c1, _, _ = encrypt_sym(env, ctx, vals, first=9)
    full = run_decrypt(env, ctx, c0, c1)
    for f in ("pte", "values", "values_f64", "status"):
        alone = run_decrypt(env, ctx, c0, c1, want=(f,))
        assert alone[f].cpu().numpy().tobytes() == full[f].cpu().numpy().tobytes(), f
        for g in ("pte", "values", "values_f64", "status"):
            if g != f:      # an output that was not requested is not written
                assert alone[g].cpu().numpy().tobytes() != full[g].cpu().numpy().tobytes(), (f, g)
    assert L.se_amd_decrypt_full_device(ctx.h, p(c0), p(c1), B, z, z, z, z, stream) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_decrypt_full_device(ctx.h, z, p(c1), B, z, z, z, p(st), stream) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_decrypt_full_device(ctx.h, p(c0), z, B, z, z, z, p(st), stream) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_decrypt_full_device(None, p(c0), p(c1), B, z, z, z, p(st), stream) == SE_ERR_INVALD_ARGUMENT
    assert L.se_amd_decrypt_full_device(ctx.h, p(c0), p(c1), 0, z, z, z, p(st), stream) == 0
    # keyed twin
    sk, _, _ = ctx.gen_keys_batch(V.derive_seeds("arg-pk", 2), V.derive_seeds("arg-ep", 2),
                                  sk_seeds=V.derive_seeds("arg-sk", 2))
    ctx.set_secret_keyring(sk)
    ki = torch.zeros(B, dtype=torch.int32, device=env["dev"])
    fk = L.se_amd_decrypt_full_keyed_device
    assert fk(ctx.h, p(c0), p(c1), B, p(ki), z, z, z, z, stream) == SE_ERR_INVALD_ARGUMENT
    assert fk(ctx.h, p(c0), p(c1), B, z, z, z, z, p(st), stream) == SE_ERR_INVALD_ARGUMENT
    assert fk(ctx.h, z, p(c1), B, p(ki), z, z, z, p(st), stream) == SE_ERR_INVALD_ARGUMENT
    assert fk(ctx.h, p(c0), p(c1), 0, p(ki), z, z, z, p(st), stream) == 0
    assert fk(ctx.h, p(c0), p(c1), B, p(ki), z, z, z, p(st), stream) == 0
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
