"""Weighted sums of ciphertexts (-m gpu): se_amd_ct_lincomb_device, the key-free aggregation entry.
Every expectation is built from NumPy integers (exact: every intermediate stays below 2^64), Python integers and the
oracle, never from the code under test; every comparison is bit-exact."""
import numpy as np
import pytest

import vectors as V
from ct_model import lincomb_expect
from gpu_support import (NULL, SE_ERR_INVALD_ARGUMENT, SENTINEL, CEntry, assert_untouched, bits,  # noqa: F401
                         decode_expect, dev_t, dptr, encrypt_sym, env, expectation, host_u32, ntt_secret, run_decrypt,
                         stream_of)

pytestmark = pytest.mark.gpu

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
SPLITS = (0, 1, 2, 7, 64)      # 0 = the automatic choice; 64 is more slices than most rows have entries
B_CONSTRUCTED = 40
ALL_MAX = (3, 17)              # the records whose residues are all q_j - 1


# ---- the expectation -------------------------------------------------------------------------------------------------
def spot_check(slab, q, rows, exp, rng):
    """The regrouped NumPy expectation against the issue's formula in plain Python integers, on a few elements."""
    npr, n = slab.shape[1], slab.shape[2]
    for g, (idx, w) in enumerate(rows):
        for _ in range(3):
            j, i = int(rng.integers(0, npr)), int(rng.integers(0, n))
            want = sum(((1 if w is None else int(w[k])) % q[j]) * int(slab[int(r), j, i]) for k, r in enumerate(idx))
            assert int(exp[g, j, i]) == want % q[j], (g, j, i)


def csr(rows, with_w=True):
    """rows -> (row_ptr, idx, w) as numpy arrays (w None if the rows carry no weights)."""
    ptr = np.zeros(len(rows) + 1, dtype=np.uint32)
    ptr[1:] = np.cumsum([len(i) for i, _ in rows])
    idx = np.array([x for i, _ in rows for x in i], dtype=np.uint32)
    w = np.array([x for _, ws in rows for x in ws], dtype=np.int32) if with_w else None
    return ptr, idx, w


def run(env, ctx, in0, in1, G, row_ptr=None, idx=None, w=None, split=0):
    """One call on device tensors; the outputs are pre-filled with a sentinel.  -> out0, out1 | None, status (host)."""
    torch = env["torch"]
    npr, n = ctx.np, ctx.n
    out0 = torch.full((G, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full((G, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"]) if in1 is not None else None
    st = torch.full((G,), 77, dtype=torch.uint8, device=env["dev"])
    ctx.set_lincomb_split(split)
    t = lambda a: None if a is None else dev_t(env, a)
    ctx.ct_lincomb(in0, out0, in1, out1, row_ptr=t(row_ptr), idx=t(idx), w=t(w), G=G, status=st)
    torch.cuda.synchronize()
    ctx.set_lincomb_split(0)
    return host_u32(out0), (host_u32(out1) if out1 is not None else None), st.cpu().numpy()


def weights(rng, count):
    special = np.array([0, 1, -1, INT32_MAX, INT32_MIN], dtype=np.int64)
    pick = rng.integers(0, 8, count)
    rnd = rng.integers(INT32_MIN, INT32_MAX + 1, count)
    return [int(special[p]) if p < 5 else int(r) for p, r in zip(pick, rnd)]


def constructed_rows(rng, B, unit):
    rows = []
    for ln in (0, 1, 2, 15, 16, 17, 31, 32, 33, 70):
        idx = [int(x) for x in rng.integers(0, B, ln)]
        if ln >= 2:
            idx[-1] = idx[0]                      # a repeated index in every row that can hold one
        rows.append((idx, None if unit else weights(rng, ln)))
    worst = 1000 if unit else 300                 # every term the largest a lazy accumulator can meet
    rows.append(([ALL_MAX[k & 1] for k in range(worst)], None if unit else [-1] * worst))
    return rows


CONSTRUCTED_SHAPES = [(1024, 1), (4096, 3), (8192, 6), (16384, 13)]


@pytest.fixture(scope="module")
def constructed(env):
    """Per shape, computed once and left unchanged: two residue slabs, the weighted and the unit-weight row lists and
    their expectations."""
    cache = {}

    def get(shape):
        if shape in cache:
            return cache[shape]
        n, npr = shape
        ctx = env["pkg"].Context(n, npr)          # no key is ever installed on these contexts
        q = [int(x) for x in ctx.moduli()]
        rng = np.random.default_rng(1000 * npr + n)
        slabs = []
        for _ in range(2):
            s = np.stack([rng.integers(0, q[j], (B_CONSTRUCTED, n), dtype=np.uint32) for j in range(npr)], axis=1)
            for b in ALL_MAX:
                s[b] = (np.array(q, dtype=np.uint32) - 1)[:, None]
            slabs.append(s)
        case = dict(ctx=ctx, q=q, slabs=slabs, dev=[dev_t(env, s) for s in slabs])
        for name, unit in (("weighted", False), ("unit", True)):
            rows = constructed_rows(rng, B_CONSTRUCTED, unit)
            exp = [lincomb_expect(s, q, rows) for s in slabs]
            spot_check(slabs[0], q, rows, exp[0], rng)
            case[name] = dict(rows=rows, exp=exp, csr=csr(rows, with_w=not unit))
        cache[shape] = case
        return case

    yield get
    for c in cache.values():
        c["ctx"].close()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shape", CONSTRUCTED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_constructed_csr(env, constructed, shape, split):
    """Tests 1 and 4: rows of 0 .. 70 entries with repeated indices, weights from {0, 1, -1, INT32_MAX, INT32_MIN,
    random}, and 300 entries of weight -1 on all-(q - 1) records; both slabs, then the one-slab call; every split."""
    c = constructed(shape)
    k = c["weighted"]
    ptr, idx, w = k["csr"]
    G = len(k["rows"])
    out0, out1, st = run(env, c["ctx"], c["dev"][0], c["dev"][1], G, ptr, idx, w, split=split)
    assert (st == 1).all(), st
    assert (out0 == k["exp"][0]).all() and (out1 == k["exp"][1]).all()
    assert not out0[0].any() and not out1[0].any()            # the empty row
    one, none, st = run(env, c["ctx"], c["dev"][1], None, G, ptr, idx, w, split=split)
    assert none is None and (st == 1).all()
    assert (one == k["exp"][1]).all()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shape", CONSTRUCTED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unit_weights(env, constructed, shape, split):
    """Tests 2 and 4: d_w = NULL over the same structure, with a 1 000-entry row of all-(q - 1) records."""
    c = constructed(shape)
    k = c["unit"]
    ptr, idx, _ = k["csr"]
    out0, out1, st = run(env, c["ctx"], c["dev"][0], c["dev"][1], len(k["rows"]), ptr, idx, None, split=split)
    assert (st == 1).all(), st
    assert (out0 == k["exp"][0]).all() and (out1 == k["exp"][1]).all()


@pytest.fixture(scope="module")
def dense(env):
    n, npr, B, G = 4096, 3, 37, 3
    ctx = env["pkg"].Context(n, npr)
    q = [int(x) for x in ctx.moduli()]
    rng = np.random.default_rng(37)
    slabs = [np.stack([rng.integers(0, q[j], (B, n), dtype=np.uint32) for j in range(npr)], axis=1) for _ in range(2)]
    w = np.array([weights(rng, B) for _ in range(G)], dtype=np.int32)
    rows = [(list(range(B)), [int(x) for x in w[g]]) for g in range(G)]
    plain = [(list(range(B)), None)]
    yield dict(ctx=ctx, B=B, G=G, w=w, dev=[dev_t(env, s) for s in slabs],
               exp=[lincomb_expect(s, q, rows) for s in slabs], exp_sum=[lincomb_expect(s, q, plain) for s in slabs])
    ctx.close()


@pytest.mark.parametrize("split", SPLITS)
def test_dense_form(env, dense, split):
    """Tests 3 and 4: G = 3 dense weight rows over B = 37 records; G = 1 without weights is the plain sum."""
    d = dense
    out0, out1, st = run(env, d["ctx"], d["dev"][0], d["dev"][1], d["G"], w=d["w"], split=split)
    assert (st == 1).all()
    assert (out0 == d["exp"][0]).all() and (out1 == d["exp"][1]).all()
    out0, out1, st = run(env, d["ctx"], d["dev"][0], d["dev"][1], 1, split=split)
    assert (st == 1).all()
    assert (out0 == d["exp_sum"][0]).all() and (out1 == d["exp_sum"][1]).all()


def test_split_hook_restores_automatic(env, constructed):
    """Test 4, last line: after a forced split, 0 gives the automatic choice again (same bits, as for every split)."""
    c = constructed((4096, 3))
    k = c["weighted"]
    ptr, idx, w = k["csr"]
    ctx = c["ctx"]
    assert ctx.L.se_amd_set_lincomb_split(ctx.h, 7) == 0
    assert ctx.L.se_amd_set_lincomb_split(ctx.h, 0) == 0
    assert ctx.L.se_amd_set_lincomb_split(None, 0) == SE_ERR_INVALD_ARGUMENT
    out0, out1, st = run(env, ctx, c["dev"][0], c["dev"][1], len(k["rows"]), ptr, idx, w, split=0)
    assert (st == 1).all() and (out0 == k["exp"][0]).all() and (out1 == k["exp"][1]).all()


@pytest.mark.parametrize("split", (0, 1, 7))
def test_status_2(env, constructed, split):
    """Test 5: an index == B, an index 0xFFFFFFFF, a decreasing row_ptr pair and row_ptr[G] > nnz give zero rows with
    status 2; their neighbours are exact with status 1."""
    c = constructed((4096, 3))
    ctx, q, B = c["ctx"], c["q"], B_CONSTRUCTED
    rng = np.random.default_rng(5)
    idx = rng.integers(0, B, 30).astype(np.uint32)
    w = np.array(weights(rng, 30), dtype=np.int32)
    idx[8] = B                                      # row 1
    idx[18] = 0xFFFFFFFF                            # row 3
    ptr = np.array([0, 5, 11, 16, 21, 26, 23, 30], dtype=np.uint32)   # row 5 decreases; row 6 = [23, 30) is valid
    G = len(ptr) - 1
    bad = {1, 3, 5}
    rows = [([] if g in bad else list(idx[ptr[g]:ptr[g + 1]]), [] if g in bad else list(w[ptr[g]:ptr[g + 1]]))
            for g in range(G)]
    exp = [lincomb_expect(s, q, rows) for s in c["slabs"]]
    out0, out1, st = run(env, ctx, c["dev"][0], c["dev"][1], G, ptr, idx, w, split=split)
    assert list(st) == [2 if g in bad else 1 for g in range(G)], st
    assert (out0 == exp[0]).all() and (out1 == exp[1]).all()
    for g in bad:
        assert not out0[g].any() and not out1[g].any(), g
    # row_ptr[G] = 30 beyond nnz = 28: the last row is rejected, row 4 = [21, 26) is not
    out0, out1, st = run(env, ctx, c["dev"][0], c["dev"][1], G, ptr, idx[:28].copy(), w[:28].copy(), split=split)
    assert list(st) == [2 if g in bad | {6} else 1 for g in range(G)], st
    assert not out0[6].any() and not out1[6].any()
    assert (out0[:6] == exp[0][:6]).all() and (out1[:6] == exp[1][:6]).all()


def test_empty_batch_rows(env):
    """B = 0: non-empty rows have nothing to point at (status 2), empty rows are zero with status 1."""
    torch = env["torch"]
    ctx = env["pkg"].Context(1024, 1)
    anchor = torch.zeros(4, dtype=torch.int32, device=env["dev"])          # a valid pointer for the empty slab
    out0 = torch.full((2, 1, 1024), SENTINEL, dtype=torch.int32, device=env["dev"])
    st = torch.full((2,), 77, dtype=torch.uint8, device=env["dev"])
    ptr, idx = dev_t(env, np.array([0, 0, 2], dtype=np.uint32)), dev_t(env, np.array([0, 1], dtype=np.uint32))
    stream = stream_of(env)
    rc = ctx.L.se_amd_ct_lincomb_device(ctx.h, dptr(anchor), None, 0, 2, dptr(ptr), dptr(idx), None, 2, dptr(out0), None,
                                        dptr(st), stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert list(st.cpu().numpy()) == [1, 2]
    assert int(torch.count_nonzero(out0)) == 0
    ctx.close()


def test_argument_errors(env, constructed):
    """Test 6: every SE_ERR_INVALD_ARGUMENT condition returns -22 and writes nothing; G = 0 is a successful no-op; the
    context has no key installed."""
    torch = env["torch"]
    c = constructed((4096, 3))
    ctx = c["ctx"]
    n, npr, B, G = 4096, 3, B_CONSTRUCTED, 2
    in0, in1 = c["dev"]
    out0 = torch.full((G, npr, n), SENTINEL, dtype=torch.int32, device=env["dev"])
    out1 = torch.full_like(out0, SENTINEL)
    st = torch.full((G,), 77, dtype=torch.uint8, device=env["dev"])
    ptr = dev_t(env, np.array([0, 2, 4], dtype=np.uint32))
    idx = dev_t(env, np.array([0, 1, 2, 3], dtype=np.uint32))
    w = dev_t(env, np.array([1, 2, 3, 4], dtype=np.int32))
    wd = dev_t(env, np.ones(G * B, dtype=np.int32))
    f = CEntry(ctx.L.se_amd_ct_lincomb_device, ctx=ctx.h, in0=dptr(in0), in1=dptr(in1), B=B, G=G, row_ptr=dptr(ptr),
               idx=dptr(idx), w=dptr(w), nnz=4, out0=dptr(out0), out1=dptr(out1), status=dptr(st), stream=stream_of(env))
    big = 2 ** 32
    f.refused([
        dict(ctx=None),
        dict(in0=NULL),                                                    # NULL d_in0
        dict(out0=NULL),                                                   # NULL d_out0
        dict(out1=NULL),                                                   # in1 without out1
        dict(in1=NULL),                                                    # out1 without in1
        dict(idx=NULL),                                                    # row_ptr without idx
        dict(row_ptr=NULL),                                                # idx without row_ptr
        dict(row_ptr=NULL, idx=NULL, w=dptr(wd), nnz=G * B - 1),           # dense, nnz != G B
        dict(B=big),                                                       # B >= 2^32
        dict(G=big),                                                       # G >= 2^32
        dict(nnz=big),                                                     # nnz >= 2^32
        dict(in0=dptr(in0, 4)),                                            # alignment, each slab
        dict(in1=dptr(in1, 8)),
        dict(out0=dptr(out0, 4)),
        dict(out1=dptr(out1, 12)),
    ])
    assert_untouched(out0, out1)
    assert_untouched(st, fill=77)
    assert f(G=0) == 0
    assert f(G=0, row_ptr=NULL, idx=NULL, w=NULL, nnz=0, status=NULL) == 0
    assert_untouched(out0, out1)
    assert_untouched(st, fill=77)
    # and the valid call works without a key (status optional)
    assert f(status=NULL) == 0
    torch.cuda.synchronize()
    rows = [([0, 1], [1, 2]), ([2, 3], [3, 4])]
    assert (host_u32(out0) == lincomb_expect(c["slabs"][0], c["q"], rows)).all()
    assert (host_u32(out1) == lincomb_expect(c["slabs"][1], c["q"], rows)).all()


def test_offsets_beyond_4gib(env):
    """Test 7: 16384 x 13 (851 968 bytes per row), one slab of 5 100 rows = 4.35 GB, zero but for four rows, two of
    them beyond byte 2^32; the expectation is built from those four rows alone."""
    torch = env["torch"]
    n, npr, B = 16384, 13, 5100
    live = [0, 5041, 5042, 5099]
    assert 5041 * npr * n * 4 < 2 ** 32 < 5042 * npr * n * 4
    ctx = env["pkg"].Context(n, npr)
    q = [int(x) for x in ctx.moduli()]
    rng = np.random.default_rng(7)
    small = np.stack([rng.integers(0, q[j], (len(live), n), dtype=np.uint32) for j in range(npr)], axis=1)
    slab = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    for k, b in enumerate(live):
        slab[b] = dev_t(env, small[k])
    rows = [([0, 5041, 5099, 2500, 5042], [3, -5, INT32_MAX, 11, 1]), ([5042, 5099, 5042, 0], [INT32_MIN, 7, 9, -1])]
    ptr, idx, w = csr(rows)
    local = {b: k for k, b in enumerate(live)}
    exp = lincomb_expect(small, q, [([local[i] for i in ix if i in local], [x for i, x in zip(ix, ws) if i in local])
                                    for ix, ws in rows])
    for split in (1, 2):
        out0, _, st = run(env, ctx, slab, None, len(rows), ptr, idx, w, split=split)
        assert (st == 1).all()
        assert (out0 == exp).all(), split
    del slab
    ctx.close()


# ---- end to end: encrypt, aggregate without a key, decrypt ----------------------------------------------------------
def aggregate_and_decrypt(env, ctx, c0, c1, rows):
    torch = env["torch"]
    G = len(rows)
    ptr, idx, w = csr(rows)
    s0 = torch.full((G, ctx.np, ctx.n), SENTINEL, dtype=torch.int32, device=env["dev"])
    s1 = torch.full_like(s0, SENTINEL)
    st = torch.full((G,), 77, dtype=torch.uint8, device=env["dev"])
    ctx.ct_lincomb(c0, s0, c1, s1, row_ptr=dev_t(env, ptr), idx=dev_t(env, idx), w=dev_t(env, w), status=st)
    torch.cuda.synchronize()
    assert bool((st == 1).all())
    return run_decrypt(env, ctx, s0, s1)


def weighted_rows(rng, G, B, wmax, longest):
    rows = []
    for g in range(G):
        ln = longest if g == 0 else int(rng.integers(1, longest + 1))
        rows.append(([int(x) for x in rng.integers(0, B, ln)], [int(x) for x in rng.integers(-wmax, wmax + 1, ln)]))
    rows[1][1][0] = wmax
    rows[1][1][-1] = -wmax
    return rows


def check_against_pte(env, ctx, o, c0, c1, pte, rows, bound):
    """decrypt_full(sum w ct) == sum w (m + e) in int64, and values_f64 is the oracle's decode of that sum."""
    hp = pte.cpu().numpy()
    want = []
    for idx, w in rows:
        y = sum(int(wk) * hp[i].astype(object) for i, wk in zip(idx, w))
        assert max(abs(int(v)) for v in y) < bound      # the range condition, asserted on the expectation
        want.append(np.array([int(v) for v in y], dtype=np.int64))
    got = aggregate_and_decrypt(env, ctx, c0, c1, rows)
    for g, y in enumerate(want):
        assert int(got["status"][g]) == 1, g
        assert (got["pte"][g].cpu().numpy() == y).all(), g
        f64 = decode_expect(o, y)
        assert (bits(got["values_f64"][g].cpu().numpy()) == bits(f64)).all(), g
        assert (bits(got["values"][g].cpu().numpy()) == bits(f64.astype(np.float32))).all(), g


@pytest.mark.parametrize("seeded", (False, True), ids=("full", "seed-compressed"))
def test_end_to_end_symmetric(env, seeded):
    """Test 8: 4096 x 3, 24 records of bench_values, G = 5 rows of at most 24 entries, |w| <= 2^20.  Per coefficient
    |m + e| <= 25.5 . 2^25 + 21 < 2^30, so every sum is below 2^30 . 2^20 . 24 < 2^55 < min(2^63, Q/2)."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 4096, 3, 24
    ctx = env["pkg"].Context(n, npr)
    ctx.set_secret_key(V.secret_key(n))
    vals = V.bench_values(B, n, first=40)
    c0, c1, pte, st = encrypt_sym(env, ctx, vals, first=40)
    assert bool((st == 1).all())
    if seeded:
        ss, sd = V.bench_seeds(B, first=40)
        c0s = torch.zeros_like(c0)
        ctx.encrypt_sym_seeded(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), c0s)
        c1s = torch.zeros_like(c1)
        ctx.expand_c1(dev_t(env, ss), c1s)
        torch.cuda.synchronize()
        c0, c1 = c0s, c1s
    o = Oracle(n, npr)
    rows = weighted_rows(np.random.default_rng(8), 5, B, 2 ** 20, 24)
    assert int(pte.abs().max()) < 2 ** 30
    check_against_pte(env, ctx, o, c0, c1, pte, rows, 2 ** 55)
    ctx.close()


def test_end_to_end_single_prime(env):
    """Test 9: 1024 x 1, 8 records of pattern 7, weights in [-4, 4]: |sum| <= 8 . 4 . (0.15 . 2^20 + 21) ~ 4.8 . 2^20,
    below Q / 2 ~ 2^26."""
    from oracle.pyoracle import Oracle
    n, npr, B = 1024, 1, 8
    ctx = env["pkg"].Context(n, npr)
    ctx.set_secret_key(V.secret_key(n))
    vals = np.stack([V.pattern_values(7, n, seed=7 + b) for b in range(B)]).astype(np.float32)
    c0, c1, pte, st = encrypt_sym(env, ctx, vals, first=60)
    assert bool((st == 1).all())
    o = Oracle(n, npr)
    rng = np.random.default_rng(9)
    rows = [(list(range(B)), [4, -4, 3, -1, 0, 2, -3, 1])]
    rows += [([int(x) for x in rng.integers(0, B, 8)], [int(x) for x in rng.integers(-4, 5, 8)]) for _ in range(2)]
    bound = 8 * 4 * (0.15 * 2 ** 20 + 21)
    assert bound < o.q[0] / 2
    check_against_pte(env, ctx, o, c0, c1, pte, rows, bound)
    ctx.close()


def test_end_to_end_public_key(env):
    """Test 10: 4096 x 3, 16 records under one generated key pair: decrypt_full(sum w ct) == sum w y_b, y_b the
    oracle's decrypt, inverse NTT and CRT of each input record."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 4096, 3, 16
    ctx = env["pkg"].Context(n, npr)
    sk, pk0, pk1 = ctx.gen_keys_batch(V.derive_seeds("agg-pk", 1), V.derive_seeds("agg-ep", 1),
                                      sk_seeds=V.derive_seeds("agg-sk", 1))
    ctx.set_secret_key(sk[0])
    ctx.set_public_key(pk0[0], pk1[0])
    vals = V.bench_values(B, n, first=80)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encrypt_asym(dev_t(env, vals), dev_t(env, V.derive_seeds("agg-enc", B)), c0, c1, status=st)
    torch.cuda.synchronize()
    assert bool((st == 1).all())
    o = Oracle(n, npr)
    s_hat = ntt_secret(o, sk[0])
    h0, h1 = host_u32(c0), host_u32(c1)
    y = [np.array(expectation(o, h0[b], h1[b], s_hat)["y"], dtype=object) for b in range(B)]
    rows = weighted_rows(np.random.default_rng(10), 4, B, 2 ** 20, 16)
    got = aggregate_and_decrypt(env, ctx, c0, c1, rows)
    for g, (idx, w) in enumerate(rows):
        want = sum(int(wk) * y[i] for i, wk in zip(idx, w))
        assert max(abs(int(v)) for v in want) < 2 ** 62
        want = np.array([int(v) for v in want], dtype=np.int64)
        assert int(got["status"][g]) == 1, g
        assert (got["pte"][g].cpu().numpy() == want).all(), g
        assert (bits(got["values_f64"][g].cpu().numpy()) == bits(decode_expect(o, want))).all(), g
    ctx.close()
