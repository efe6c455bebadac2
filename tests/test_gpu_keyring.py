"""Key rings (-m gpu): one batch encrypted under many keys, chosen per ciphertext by a device array of indices.
Keyed output must equal the oracle under the chosen key, and the unkeyed entry with that key installed, bit for bit,
through every dispatch branch of the unkeyed calls."""

import numpy as np
import pytest

import vectors as V
from gpu_support import dev_t, env, host_u32  # noqa: F401  (env is a fixture)

pytestmark = pytest.mark.gpu


def make_keys(ctx, K, tag="ring"):
    sks = V.derive_seeds(tag + "-sk", K)
    pks = V.derive_seeds(tag + "-pk", K)
    eps = V.derive_seeds(tag + "-ep", K)
    return ctx.gen_keys_batch(pks, eps, sk_seeds=sks)


def key_indices(B, K, seed=5):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, K, size=B).astype(np.uint32)
    idx[B // 2] = K - 1
    if B > 2:
        idx[0] = idx[1]          # a repeat
    return idx


def outputs(env, B, npr, n):
    torch = env["torch"]
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    return dict(c0=c0, c1=torch.zeros_like(c0), ntt_pte=torch.zeros_like(c0),
                pte=torch.zeros((B, n), dtype=torch.int64, device=env["dev"]),
                status=torch.zeros(B, dtype=torch.uint8, device=env["dev"]))


def run_keyed(env, ctx, mode, vals, idx, ss, sd):
    B, n, npr = vals.shape[0], ctx.n, ctx.np
    o = outputs(env, B, npr, n)
    ti = dev_t(env, idx)
    if mode == "sym":
        ctx.encrypt_sym_keyed(dev_t(env, vals), ti, dev_t(env, ss), dev_t(env, sd), o["c0"], o["c1"], o["ntt_pte"],
                              o["pte"], o["status"])
    else:
        ctx.encrypt_asym_keyed(dev_t(env, vals), ti, dev_t(env, sd), o["c0"], o["c1"], o["ntt_pte"], o["pte"],
                               o["status"])
    env["torch"].cuda.synchronize()
    return o


def run_unkeyed(env, ctx, mode, vals, ss, sd):
    B, n, npr = vals.shape[0], ctx.n, ctx.np
    o = outputs(env, B, npr, n)
    if mode == "sym":
        ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), o["c0"], o["c1"], o["ntt_pte"], o["pte"],
                        o["status"])
    else:
        ctx.encrypt_asym(dev_t(env, vals), dev_t(env, sd), o["c0"], o["c1"], o["ntt_pte"], o["pte"], o["status"])
    env["torch"].cuda.synchronize()
    return o


def install(ctx, mode, keys, k=None):
    sk, pk0, pk1 = keys
    if k is None:
        if mode == "sym":
            ctx.set_secret_keyring(sk)
        else:
            ctx.set_public_keyring(pk0, pk1)
    elif mode == "sym":
        ctx.set_secret_key(sk[k])
    else:
        ctx.set_public_key(pk0[k], pk1[k])


def assert_equals_grouped(env, ctx, mode, keys, vals, idx, ss, sd, got, what=""):
    """Group the records by key, encrypt each group with the unkeyed entry under that key: bit-identical."""
    torch = env["torch"]
    for k in np.unique(idx):
        sel = np.nonzero(idx == k)[0]
        install(ctx, mode, keys, int(k))
        ref = run_unkeyed(env, ctx, mode, vals[sel], ss[sel], sd[sel])
        ts = torch.from_numpy(sel).to(env["dev"])
        for f in ("c0", "c1", "ntt_pte", "pte", "status"):
            assert torch.equal(got[f].index_select(0, ts), ref[f]), (what, int(k), f)


SHAPES = V.ALL_SHAPES + [(16384, 13)]


@pytest.mark.parametrize("mode", ["sym", "asym"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_keyed_oracle_parity(env, shape, mode):
    from oracle.pyoracle import Oracle
    n, npr = shape
    K = 5
    B = 9 if n <= 4096 else 3
    ctx = env["pkg"].Context(n, npr)
    keys = make_keys(ctx, K)
    sk, pk0, pk1 = keys
    install(ctx, mode, keys)
    vals = V.bench_values(B, n, first=11)
    ss, sd = V.bench_seeds(B, first=400)
    idx = key_indices(B, K)
    got = run_keyed(env, ctx, mode, vals, idx, ss, sd)
    o = Oracle(n, npr)
    g0, g1, gp = host_u32(got["c0"]), host_u32(got["c1"]), host_u32(got["ntt_pte"])
    gpte = got["pte"].cpu().numpy()
    assert (got["status"].cpu().numpy() == 1).all()
    for b in range(B):
        k = int(idx[b])
        if mode == "sym":
            r = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk[k])
            assert (gp[b] == r["ntt_pte"]).all(), b
        else:
            r = o.encrypt_asym(vals[b], sd[b].tobytes(), pk0[k], pk1[k])
        assert (g0[b] == r["c0"]).all(), (b, k)
        assert (g1[b] == r["c1"]).all(), (b, k)
        assert (gpte[b] == r["pte"]).all(), (b, k)
    ctx.close()


def branch_batches(n):
    out = []
    for B in (1, 5, 67):
        out.append((f"B{B}", V.bench_values(B, n, first=100 + B)))
    v = V.bench_values(66, n, first=31)
    v[1] *= 1.0e6               # beyond 32 bits: the general kernels
    v[2][3] = np.nan            # non-finite: the general kernels' exact transform
    out.append(("general", v))
    return out


@pytest.mark.parametrize("shape", [(4096, 3), (16384, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_keyed_sym_every_branch_equals_unkeyed(env, shape):
    n, npr = shape
    K = 6
    ctx = env["pkg"].Context(n, npr)
    keys = make_keys(ctx, K, "branch")
    ctx.set_secret_keyring(keys[0])
    # (overlap, split, debug flags) as test_all_pipeline_shapes_agree, plus the default dispatch (split chosen per
    # call, small batches through the prime speculation)
    configs = [(0, 0, 32), (0, 1, 32 + 8), (1, 0, 32 + 8), (1, 1, 0), (1, 2, 0)]
    for name, vals in branch_batches(n):
        if n >= 16384 and vals.shape[0] > 5:
            vals = vals[:5] if name != "general" else vals[:4]
        B = vals.shape[0]
        ss, sd = V.bench_seeds(B, first=700 + B)
        idx = key_indices(B, K, seed=B)
        for overlap, split, flags in configs:
            ctx.set_pipeline(overlap, split)
            ctx.set_debug_flags(flags)
            got = run_keyed(env, ctx, "sym", vals, idx, ss, sd)
            assert_equals_grouped(env, ctx, "sym", keys, vals, idx, ss, sd, got, (name, overlap, split, flags))
    ctx.close()


@pytest.mark.parametrize("shape", [(4096, 3), (8192, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_keyed_asym_every_branch_equals_unkeyed(env, shape):
    n, npr = shape
    K = 6
    ctx = env["pkg"].Context(n, npr)
    keys = make_keys(ctx, K, "branch-pk")
    ctx.set_public_keyring(keys[1], keys[2])
    for name, vals in branch_batches(n):
        B = vals.shape[0]
        ss, sd = V.bench_seeds(B, first=900 + B)
        idx = key_indices(B, K, seed=B + 1)
        for overlap, flags in ((1, 0), (0, 32)):   # ternary sampler: wave form / lane form
            ctx.set_pipeline(overlap, 2)
            ctx.set_debug_flags(flags)
            got = run_keyed(env, ctx, "asym", vals, idx, ss, sd)
            assert_equals_grouped(env, ctx, "asym", keys, vals, idx, ss, sd, got, (name, overlap, flags))
    ctx.close()


@pytest.mark.parametrize("cfg", [("sym", (4096, 3), 65536, 16), ("asym", (4096, 3), 65536, 16),
                                 ("sym", (16384, 6), 32768, 8)], ids=["C2", "C3", "C4"])
def test_keyed_full_size(env, cfg):
    mode, (n, npr), B, K = cfg
    ctx = env["pkg"].Context(n, npr)
    if mode == "asym":
        ctx.set_asym_chunks(4)            # the chunked CBD / fused pipeline
    keys = make_keys(ctx, K, "full")
    install(ctx, mode, keys)
    vals = V.bench_values(B, n)
    ss, sd = V.bench_seeds(B)
    idx = key_indices(B, K, seed=77)
    got = run_keyed(env, ctx, mode, vals, idx, ss, sd)
    assert_equals_grouped(env, ctx, mode, keys, vals, idx, ss, sd, got, mode)
    ctx.close()


def test_keyed_seed_compressed(env):
    torch = env["torch"]
    n, npr, B, K = 4096, 3, 67, 5
    ctx = env["pkg"].Context(n, npr)
    keys = make_keys(ctx, K, "seeded")
    ctx.set_secret_keyring(keys[0])
    vals = V.bench_values(B, n, first=3)
    ss, sd = V.bench_seeds(B, first=3)
    idx = key_indices(B, K, seed=3)
    full = run_keyed(env, ctx, "sym", vals, idx, ss, sd)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encrypt_sym_keyed(dev_t(env, vals), dev_t(env, idx), dev_t(env, ss), dev_t(env, sd), c0, None, status=st)
    c1 = torch.zeros_like(c0)
    ctx.expand_c1(dev_t(env, ss), c1)
    torch.cuda.synchronize()
    assert torch.equal(c0, full["c0"]) and torch.equal(c1, full["c1"]) and torch.equal(st, full["status"])
    ctx.close()


@pytest.mark.parametrize("shape", [(1024, 1), (2048, 1), (4096, 3), (8192, 6), (16384, 6)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_decrypt_decode_keyed(env, shape):
    torch = env["torch"]
    n, npr = shape
    K, B = 5, 7
    ctx = env["pkg"].Context(n, npr)
    keys = make_keys(ctx, K, "dec")
    ctx.set_secret_keyring(keys[0])
    ctx.set_public_keyring(keys[1], keys[2])
    vals = V.bench_values(B, n, first=8)
    if n == 2048:
        vals *= 0.01    # one 27-bit prime under the scale 2^25 holds |v| < 2
    ss, sd = V.bench_seeds(B, first=8)
    idx = key_indices(B, K, seed=8)
    ti = dev_t(env, idx)
    for mode in ("sym", "asym"):
        got = run_keyed(env, ctx, mode, vals, idx, ss, sd)
        for j in range(npr):
            c0, c1 = got["c0"], got["c1"]        # [B][np][n]: the entry picks prime j
            dec = torch.zeros((B, n), dtype=torch.int32, device=env["dev"])
            out = torch.zeros((B, n // 2), dtype=torch.float32, device=env["dev"])
            ctx.decrypt_decode_keyed(c0, c1, ti, j, dec_ntt=dec, values=out)
            torch.cuda.synchronize()
            if mode == "sym":
                assert (host_u32(dec) == host_u32(got["ntt_pte"][:, j].contiguous())).all(), j
            assert np.abs(out.cpu().numpy() - vals).max() < 0.1, (mode, j)
    ctx.close()


def test_keyed_validation(env):
    torch = env["torch"]
    pkg = env["pkg"]
    n, npr, K, B = 4096, 3, 5, 9
    ctx = pkg.Context(n, npr)
    keys = make_keys(ctx, K, "valid")
    sk, pk0, pk1 = keys
    vals = V.bench_values(B, n, first=1)
    ss, sd = V.bench_seeds(B, first=1)
    idx = key_indices(B, K, seed=1)
    # no ring installed (a single key does not count)
    ctx.set_secret_key(sk[0])
    ctx.set_public_key(pk0[0], pk1[0])
    for mode in ("sym", "asym"):
        with pytest.raises(pkg.SealEmbeddedAmdError, match="ring"):
            run_keyed(env, ctx, mode, vals, idx, ss, sd)
    with pytest.raises(pkg.SealEmbeddedAmdError, match="ring"):
        c = torch.zeros((B, n), dtype=torch.int32, device=env["dev"])
        ctx.decrypt_decode_keyed(c, c, dev_t(env, idx), 0)
    # a code-3 key, an unreduced public-key coefficient
    bad_sk = sk.copy()
    bad_sk[3, 17] |= 0x0C
    with pytest.raises(pkg.SealEmbeddedAmdError, match="code"):
        ctx.set_secret_keyring(bad_sk)
    q = ctx.moduli()
    bad_pk = pk1.copy()
    bad_pk[2, npr - 1, 5] = q[npr - 1]
    with pytest.raises(pkg.SealEmbeddedAmdError, match="reduced"):
        ctx.set_public_keyring(pk0, bad_pk)
    # out-of-range indices: status 2, zero c0 (and c1 in public-key mode), the other records bit-exact
    ctx.set_secret_keyring(sk)
    ctx.set_public_keyring(pk0, pk1)
    vals[4] *= 1.0e30           # an encode overflow: status 0 ...
    bad = idx.copy()
    bad[2], bad[4], bad[6] = K, K + 1, 0xFFFFFFFF   # ... which status 2 overrides
    for mode in ("sym", "asym"):
        ref = run_keyed(env, ctx, mode, vals, idx, ss, sd)
        got = run_keyed(env, ctx, mode, vals, bad, ss, sd)
        st = got["status"].cpu().numpy()
        assert int(ref["status"][4]) == 0
        for b in range(B):
            if b in (2, 4, 6):
                assert st[b] == 2, (mode, b)
                assert int(torch.count_nonzero(got["c0"][b])) == 0, (mode, b)
                if mode == "asym":
                    assert int(torch.count_nonzero(got["c1"][b])) == 0, (mode, b)
                else:
                    assert torch.equal(got["c1"][b], ref["c1"][b])
            else:
                for f in ("c0", "c1", "ntt_pte", "pte", "status"):
                    assert torch.equal(got[f][b], ref[f][b]), (mode, b, f)
    ctx.close()


def test_keyring_and_single_key_are_independent(env):
    n, npr, K, B = 4096, 3, 4, 9
    ctx = env["pkg"].Context(n, npr)
    keys = make_keys(ctx, K, "indep")
    other = make_keys(ctx, K, "indep-other")
    vals = V.bench_values(B, n, first=2)
    ss, sd = V.bench_seeds(B, first=2)
    idx = key_indices(B, K, seed=2)
    torch = env["torch"]
    for mode in ("sym", "asym"):
        install(ctx, mode, keys, 1)
        single = run_unkeyed(env, ctx, mode, vals, ss, sd)
        install(ctx, mode, keys)                 # a ring leaves the single key alone
        again = run_unkeyed(env, ctx, mode, vals, ss, sd)
        keyed = run_keyed(env, ctx, mode, vals, idx, ss, sd)
        install(ctx, mode, other, 2)             # a single key leaves the ring alone
        keyed2 = run_keyed(env, ctx, mode, vals, idx, ss, sd)
        for f in ("c0", "c1", "ntt_pte", "pte", "status"):
            assert torch.equal(single[f], again[f]), (mode, f)
            assert torch.equal(keyed[f], keyed2[f]), (mode, f)
    ctx.close()
