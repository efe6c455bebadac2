"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on the
same seeded inputs, against the committed golden fixtures, and -- at BASELINE sizes -- through
size-independent properties.  Bar: bit-exact (all outputs are integers / bytes).
Nothing here reads /root/reference.
"""
import ctypes as C
import hashlib
import os
import struct

import numpy as np
import pytest

import vectors as V
from gpu_support import (SEED_A, SEED_B, SEED_EP, SEED_PK, build_example, check_host_tables, dev_t, env,  # noqa: F401
                         host_u32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def seeds_np(B, tag):
    return V.derive_seeds(tag, B)


# --------------------------------------------------------------------------- SURVEY trap T8 on the GPU box
@pytest.mark.parametrize("n", [1024, 2048, 4096, 8192, 16384])
def test_t8_root_tables_on_this_box(env, golden, n):
    """SURVEY 8(c) T8 asks for the twiddle digests to be recomputed "at start-up on the GPU box": the IFFT roots
    are cos/sin of the HOST libm (fft.c:39-45), so the box that runs the kernels is the one whose libm counts.
    Three tables must carry the committed digest here: the oracle's (this host's libm), the product's host table
    (se_amd_host_tables) and the table the DEVICE holds (copied back and hashed by se_amd_ifft_table_sha256)."""
    from oracle.pyoracle import Oracle
    want = golden["digests"]["ifft_twiddle_sha256"][str(n)]
    assert hashlib.sha256(Oracle(n, 1).twiddles().astype("<f8").tobytes()).hexdigest() == want
    t = env["pkg"].host_tables(n, 1)
    assert hashlib.sha256(t["ifft_w"].astype("<f8").tobytes()).hexdigest() == want
    ctx = env["pkg"].Context(n, 1)
    assert ctx.ifft_table_sha256() == want
    ctx.close()


def test_t8_host_tables_match_oracle_on_this_box(env):
    """The CPU-suite check of every setup-time table (tests/test_cabi.py) repeated where the product runs."""
    for shape in [(1024, 1), (4096, 3), (16384, 13)]:
        check_host_tables(env["pkg"], shape)


# --------------------------------------------------------------------------- PRNG / Keccak
def test_prng_blocks_match_hashlib(env):
    torch = env["torch"]
    ctx = env["pkg"].Context(1024, 1)
    cnt = 130
    seeds = seeds_np(cnt, "prng-test")
    ctrs = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5] + list(range(5, cnt)), dtype=np.uint64)
    for outlen in (1, 4, 96, 136, 137, 300, 4096):
        out = torch.zeros((cnt, outlen), dtype=torch.uint8, device=env["dev"])
        ctx.prng_blocks(dev_t(env, seeds), dev_t(env, ctrs.view(np.int64)), out, outlen)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i in range(cnt):
            exp = hashlib.shake_256(seeds[i].tobytes() + struct.pack("<Q", int(ctrs[i]))).digest(outlen)
            assert got[i].tobytes() == exp, (outlen, i)


# --------------------------------------------------------------------------- samplers
@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sample_uniform_vs_oracle(env, shape):
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    B = 70  # crosses a wave boundary (64) and leaves a ragged tail
    o = Oracle(n, npr)
    seeds = seeds_np(B, f"uni-{n}")
    exp, ectr = [], []
    for b in range(B):
        ctr, row = 0, []
        for j in range(npr):
            a, ctr = o.sample_uniform(j, seeds[b].tobytes(), ctr)
            row.append(a)
        exp.append(row)
        ectr.append(ctr)
    # flags 0: a batch this small takes the WAVE-per-ciphertext kernel (k_sample_uniform_wave); 32 forces the
    # lane-per-ciphertext kernel, in its three shapes: + 0 helper waves precompute redraw candidates during the
    # squeeze (small-batch shape); + 16 helper waves only pool the redraw phase; + 8 wave-local redraw phase
    # (the shape a full 65 536 batch runs)
    for flags in (0, 32, 32 + 8, 32 + 16):
        ctx = env["pkg"].Context(n, npr)
        ctx.set_debug_flags(flags)
        out = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
        ctr_out = torch.zeros(B, dtype=torch.int64, device=env["dev"])
        ctx.sample_uniform(dev_t(env, seeds), out, ctr_out=ctr_out)
        torch.cuda.synchronize()
        got, gctr = host_u32(out), ctr_out.cpu().numpy()
        for b in range(B):
            for j in range(npr):
                assert (got[b, j] == exp[b][j]).all(), (flags, b, j)
            assert int(gctr[b]) == ectr[b]


def test_sample_uniform_golden_and_ctr_in(env, golden):
    torch = env["torch"]
    for (n, npr) in [(1024, 1), (4096, 3)]:
        d = golden["digests"]["shapes"][f"{n}x{npr}"]["samplers"]
        ctx = env["pkg"].Context(n, npr)
        seeds = np.frombuffer(SEED_A, dtype=np.uint8).reshape(1, 64).copy()
        out = torch.zeros((1, npr, n), dtype=torch.int32, device=env["dev"])
        ctx.sample_uniform(dev_t(env, seeds), out)
        torch.cuda.synchronize()
        for j in range(npr):
            assert V.sha256_hex(host_u32(out)[0, j]) == d[f"uniform_p{j}"]["sha256"]
        # non-zero starting counter
        from oracle.pyoracle import Oracle
        o = Oracle(n, npr)
        cin = np.array([12345678901], dtype=np.int64)
        ctx.sample_uniform(dev_t(env, seeds), out, ctr_in=dev_t(env, cin))
        torch.cuda.synchronize()
        ctr = int(cin[0])
        for j in range(npr):
            a, ctr = o.sample_uniform(j, SEED_A, ctr)
            assert (host_u32(out)[0, j] == a).all()


def test_sample_uniform_reject_list_overflow_path(env):
    """The rare branch (more rejections than list entries) forced by a tiny capacity: the
    marker-rescan path must give the same polynomial (cdna guide rule 26)."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 4096, 3, 66
    o = Oracle(n, npr)
    seeds = seeds_np(B, "uni-overflow")
    exp = np.zeros((B, npr, n), dtype=np.uint32)
    for b in range(B):
        ctr = 0
        for j in range(npr):
            exp[b, j], ctr = o.sample_uniform(j, seeds[b].tobytes(), ctr)
    for cap in (0, 1, 7, 64):
        # wave form (marker scan by the whole wave) / lane form: speculating helpers, no helpers, pooling-only
        for flags in (0, 32, 32 + 8, 32 + 16):
            ctx = env["pkg"].Context(n, npr)
            ctx.set_reject_list_capacity(cap)
            ctx.set_debug_flags(flags)
            out = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
            ctx.sample_uniform(dev_t(env, seeds), out)
            torch.cuda.synchronize()
            assert (host_u32(out) == exp).all(), (cap, flags)


@pytest.mark.parametrize("asym", [False, True])
def test_host_pipeline_chunks_and_pinned_outputs(env, asym):
    """The host-pointer entry is a chunked PCIe pipeline (se_hostpipe.cpp): forced small chunks with
    a ragged tail, more chunks than device slots, pageable (staged through the pinned ring) and
    pinned (direct DMA) destinations all have to give the device-pointer path's bytes."""
    torch = env["torch"]
    n, npr, B = 1024, 1, 300
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    if asym:
        ctx.set_public_key(*ctx.gen_public_key(sk, bytes(range(64)), bytes(range(64, 128))))
    vals = V.bench_values(B, n, seed=99)
    ss, sd = V.bench_seeds(B, first=500)
    run = (lambda **kw: ctx.encrypt_asym_host(vals, sd, **kw)) if asym else \
          (lambda **kw: ctx.encrypt_sym_host(vals, ss, sd, **kw))
    ref = run(want_extra=True)                       # automatic chunking: one chunk
    assert ref["failed"] == 0 and ref["status"].all()
    d0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    d1 = torch.zeros_like(d0)
    if asym:
        ctx.encrypt_asym(dev_t(env, vals), dev_t(env, sd), d0, d1)
    else:
        ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), d0, d1)
    torch.cuda.synchronize()
    assert (host_u32(d0) == ref["c0"]).all() and (host_u32(d1) == ref["c1"]).all()
    for chunk in (64, 7, 299):
        ctx.set_host_chunk(chunk)
        r = run(want_extra=True)
        for k in ("c0", "c1", "ntt_pte", "pte", "status"):
            assert (r[k] == ref[k]).all(), (chunk, k)
    # pinned destinations: direct DMA, no staging ring
    p0 = torch.zeros((B, npr, n), dtype=torch.int32).pin_memory()
    p1 = torch.zeros((B, npr, n), dtype=torch.int32).pin_memory()
    ctx.set_host_chunk(64)
    r = run(out=(p0.numpy().view(np.uint32), p1.numpy().view(np.uint32)))
    assert (r["c0"] == ref["c0"]).all() and (r["c1"] == ref["c1"]).all()
    if not asym:                                     # seed-compressed host form: c0 only
        r = ctx.encrypt_sym_host(vals, ss, sd, seed_compressed=True)
        assert r["c1"] is None and (r["c0"] == ref["c0"]).all()
    ctx.set_host_chunk(0)


def test_host_pipeline_large_pieces(env):
    """Outputs larger than one 64 MiB ring piece and more pieces than ring entries (n=4096, 3 primes,
    B=4096 -> 192 MiB per component per chunk, two chunks)."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 4096
    ctx = env["pkg"].Context(n, npr)
    ctx.set_secret_key(V.secret_key(n))
    vals = V.bench_values(B, n, seed=5)
    ss, sd = V.bench_seeds(B)
    d0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    d1 = torch.zeros_like(d0)
    ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), d0, d1)
    torch.cuda.synchronize()
    ctx.set_host_chunk(2048)
    r = ctx.encrypt_sym_host(vals, ss, sd)
    assert r["failed"] == 0
    assert (r["c0"] == host_u32(d0)).all() and (r["c1"] == host_u32(d1)).all()


@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sample_uniform_wave_form_equals_lane_form(env, shape):
    """The wave-per-ciphertext kernel (one Keccak state over the 64 lanes of a wave: DPP row shifts,
    v_permlane16/32_swap, ds_bpermute) against the lane-per-ciphertext kernel and the oracle: ragged batch
    sizes around a workgroup (4 waves), non-zero start counters, end counters, forced beyond its dispatch
    threshold (flag 64) at a size where the lane form runs full workgroups, and a masked redo launch shape."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    o = Oracle(n, npr)
    for B in (1, 3, 4, 5, 9):
        seeds = seeds_np(B, f"wave-{n}-{B}")
        cin = (np.arange(B, dtype=np.int64) * 1234567 + (1 << 33)) * (B % 2)
        ctx = env["pkg"].Context(n, npr)
        outs = []
        for flags in (0, 32):
            ctx.set_debug_flags(flags)
            out = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
            cout = torch.zeros(B, dtype=torch.int64, device=env["dev"])
            ctx.sample_uniform(dev_t(env, seeds), out, ctr_in=dev_t(env, cin), ctr_out=cout)
            torch.cuda.synchronize()
            outs.append((host_u32(out), cout.cpu().numpy()))
        assert (outs[0][0] == outs[1][0]).all() and (outs[0][1] == outs[1][1]).all(), B
        for b in range(B):
            ctr = int(cin[b])
            for j in range(npr):
                a, ctr = o.sample_uniform(j, seeds[b].tobytes(), ctr)
                assert (outs[0][0][b, j] == a).all(), (B, b, j)
            assert int(outs[0][1][b]) == ctr
        ctx.close()
    if n <= 4096:
        B = 700                                   # forced wave form well beyond a few waves per CU
        seeds = seeds_np(B, f"wave-big-{n}")
        ctx = env["pkg"].Context(n, npr)
        res = []
        for flags in (64, 32):
            ctx.set_debug_flags(flags)
            out = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
            cout = torch.zeros(B, dtype=torch.int64, device=env["dev"])
            ctx.sample_uniform(dev_t(env, seeds), out, ctr_out=cout)
            torch.cuda.synchronize()
            res.append((out.clone(), cout.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        ctx.close()


@pytest.mark.parametrize("shape,B", [((1024, 1), 70), ((2048, 1), 33), ((4096, 3), 131), ((8192, 6), 33),
                                     ((16384, 6), 70)],
                         ids=lambda v: str(v))
def test_staged_sampler_pipeline(env, shape, B):
    """The staged form of the symmetric pipeline (one ciphertext per LANE PAIR for the bulk squeeze --
    KeccakHalf --, the redraw candidates as a throughput kernel on a stream of its own, one wave per ciphertext
    to resolve them; chosen for batches between the wave form's limit and one pair wave per SIMD, forced here
    with debug flag 512) against the oracle: odd batch sizes (idle pairs, partial workgroups), a candidate row
    that is too short (the rest is computed by the resolving wave), a reject list that is too short (marker
    scan), and repeated calls on the same scratch."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    o = Oracle(n, npr)
    sk = V.secret_key(n, seed=17)
    vals = V.bench_values(B, n, first=900)
    ss, sd = V.bench_seeds(B, first=900)
    exp = [o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk) for b in range(B)]
    for spec_cap, rej_cap in ((None, None), (8, None), (None, 5), (1, 0)):
        ctx = env["pkg"].Context(n, npr)
        ctx.set_secret_key(sk)
        ctx.set_pipeline(1, 1)
        ctx.set_debug_flags(512)
        if spec_cap is not None:
            ctx.set_speculation_capacity(spec_cap)
        if rej_cap is not None:
            ctx.set_reject_list_capacity(rej_cap)
        for rep in range(2):
            c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
            c1 = torch.zeros_like(c0)
            st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
            ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), c0, c1, status=st)
            torch.cuda.synchronize()
            g0, g1 = host_u32(c0), host_u32(c1)
            assert bool(st.all())
            for b in range(B):
                assert (g1[b] == exp[b]["c1"]).all(), (spec_cap, rej_cap, rep, b)
                assert (g0[b] == exp[b]["c0"]).all(), (spec_cap, rej_cap, rep, b)
        ctx.close()


def test_sample_uniform_speculation_shortfall_path(env):
    """Helper waves precompute spec_cap redraw candidates per ciphertext; when a ciphertext needs
    more, the rest goes through the pooled loop.  Forced here with tiny capacities."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 4096, 3, 130
    o = Oracle(n, npr)
    seeds = seeds_np(B, "uni-spec")
    exp = np.zeros((B, npr, n), dtype=np.uint32)
    ectr = []
    for b in range(B):
        ctr = 0
        for j in range(npr):
            exp[b, j], ctr = o.sample_uniform(j, seeds[b].tobytes(), ctr)
        ectr.append(ctr)
    for cap in (1, 8, 70, 90):
        ctx = env["pkg"].Context(n, npr)
        ctx.set_debug_flags(32)                  # the lane-per-ciphertext kernel (the wave form has no helpers)
        ctx.set_speculation_capacity(cap)
        out = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
        ctr_out = torch.zeros(B, dtype=torch.int64, device=env["dev"])
        ctx.sample_uniform(dev_t(env, seeds), out, ctr_out=ctr_out)
        torch.cuda.synchronize()
        assert (host_u32(out) == exp).all(), cap
        assert [int(x) for x in ctr_out.cpu().numpy()] == ectr, cap


@pytest.mark.parametrize("n", [1024, 2048, 4096, 16384])
def test_sample_ternary_and_cbd_vs_oracle(env, n):
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    npr = 1 if n <= 2048 else 3
    B = 67
    ctx = env["pkg"].Context(n, npr)
    o = Oracle(n, npr)
    seeds = seeds_np(B, f"tern-{n}")
    codes = torch.zeros((B, n), dtype=torch.int8, device=env["dev"])
    ctr_out = torch.zeros(B, dtype=torch.int64, device=env["dev"])
    # flag 32 forces the lane-per-ciphertext chain kernel (the form of rounds 1-3 for full batches)
    ctx.set_debug_flags(32)
    lane_codes = torch.zeros_like(codes)
    lane_ctr = torch.zeros_like(ctr_out)
    ctx.sample_ternary(dev_t(env, seeds), lane_codes, lane_ctr)
    # 0: the window form (round 4: one permutation per counter of a window, roles dealt afterwards); 64: the
    # wave-per-ciphertext chains; 4096: a window of blocks + 2 counters, so that nearly every chain leaves it and is
    # redone by the sequential fallback of the window kernel
    for flags in (64, 4096, 0):
        ctx.set_debug_flags(flags)
        codes.zero_(), ctr_out.zero_()
        ctx.sample_ternary(dev_t(env, seeds), codes, ctr_out)
        torch.cuda.synchronize()
        assert torch.equal(codes, lane_codes) and torch.equal(ctr_out, lane_ctr), flags
    err = torch.zeros((B, 2 * n), dtype=torch.int8, device=env["dev"])
    ctx.sample_cbd(dev_t(env, seeds), err, 2 * (n // 16), ctr_base=ctr_out)
    torch.cuda.synchronize()
    gc, gctr, ge = codes.cpu().numpy(), ctr_out.cpu().numpy(), err.cpu().numpy()
    for b in range(B):
        u, c = o.sample_ternary_small(seeds[b].tobytes(), 0)
        assert (ctx.pack_ternary(gc[b]) == u).all(), b
        assert int(gctr[b]) == c
        e0, c2 = o.cbd_int8(seeds[b].tobytes(), c)
        e1, c3 = o.cbd_int8(seeds[b].tobytes(), c2)
        assert (ge[b, :n] == e0).all() and (ge[b, n:] == e1).all(), b


def test_sample_ternary_cbd_golden(env, golden):
    torch = env["torch"]
    for (n, npr) in [(1024, 1), (4096, 3), (16384, 6)]:
        d = golden["digests"]["shapes"][f"{n}x{npr}"]["samplers"]
        ctx = env["pkg"].Context(n, npr)
        seeds = np.frombuffer(SEED_B, dtype=np.uint8).reshape(1, 64).copy()
        codes = torch.zeros((1, n), dtype=torch.int8, device=env["dev"])
        ctr_out = torch.zeros(1, dtype=torch.int64, device=env["dev"])
        ctx.sample_ternary(dev_t(env, seeds), codes, ctr_out)
        e = torch.zeros((1, n), dtype=torch.int8, device=env["dev"])
        ctx.sample_cbd(dev_t(env, seeds), e, n // 16, ctr_base=ctr_out)
        torch.cuda.synchronize()
        assert int(ctr_out[0]) == d["ternary"]["ctr_out"]
        assert V.sha256_hex(ctx.pack_ternary(codes.cpu().numpy()[0])) == d["ternary"]["sha256"]
        assert V.sha256_hex(e.cpu().numpy()[0]) == d["cbd_int8"]["sha256"]


# --------------------------------------------------------------------------- transforms
@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ntt_vs_oracle_and_golden(env, golden, shape):
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    d = golden["digests"]["shapes"][f"{n}x{npr}"]
    ctx = env["pkg"].Context(n, npr)
    o = Oracle(n, npr)
    rng = np.random.default_rng(d["ntt_random_seed"])   # same draw order as make_golden.py
    rng2 = np.random.default_rng(4242 + n)
    for j in range(npr):
        q = o.q[j]
        delta = np.zeros(n, dtype=np.uint32)
        delta[1] = 1
        ins = {"delta1": delta, "ones": np.ones(n, dtype=np.uint32),
               "ramp": (np.arange(n, dtype=np.uint64) % q).astype(np.uint32),
               "qm1": np.full(n, q - 1, dtype=np.uint32),
               "random": rng.integers(0, q, n, dtype=np.uint64).astype(np.uint32)}
        names = list(ins)
        # extra: the non-canonical input q (reduce_pte_core edge) and a batch of randoms
        extra = rng2.integers(0, q, (5, n), dtype=np.uint64).astype(np.uint32)
        extra[0, :8] = q
        batch = np.concatenate([np.stack([ins[k] for k in names]), extra])
        t = dev_t(env, batch.view(np.int32))
        ctx.ntt(j, t)
        torch.cuda.synchronize()
        got = host_u32(t)
        for i, name in enumerate(names):
            assert V.sha256_hex(got[i]) == d["ntt"][f"{name}_p{j}"]["sha256"], (name, j)
        for i in range(5):
            assert (got[len(names) + i] == o.ntt(extra[i], j)).all()


@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_vs_oracle_and_golden(env, golden, shape):
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    d = golden["digests"]["shapes"][f"{n}x{npr}"]["encode"]
    ctx = env["pkg"].Context(n, npr)
    o = Oracle(n, npr)
    rng = np.random.default_rng(77 + n)
    rows = [V.pattern_values(t, n) for t in range(9)]
    rows.append(V.bench_values(1, n)[0])
    rows.append(np.full(n // 2, 3.0e38, dtype=np.float32))                 # overflow -> status 0
    rows.append((rng.standard_normal(n // 2) * 1e6).astype(np.float32))    # large magnitudes
    rows.append((rng.standard_normal(n // 2) * 1e-3).astype(np.float32))   # tiny magnitudes
    big = np.zeros(n // 2, dtype=np.float32)
    big[0] = 2.0 ** 40                                                     # near the int64 edge
    rows.append(big)
    vals = np.stack(rows)
    out = torch.zeros((vals.shape[0], n), dtype=torch.int64, device=env["dev"])
    status = torch.zeros(vals.shape[0], dtype=torch.uint8, device=env["dev"])
    ctx.encode(dev_t(env, vals), out, status)
    torch.cuda.synchronize()
    got, st = out.cpu().numpy(), status.cpu().numpy()
    for t in range(9):
        assert st[t] == 1 and V.sha256_hex(got[t]) == d[f"pattern{t}"]["sha256"], t
    assert V.sha256_hex(got[9]) == d["bench0"]["sha256"]
    assert st[10] == 0 and d["overflow_3e38_ok"] is False
    for i in (11, 12, 13):
        ok, m = o.encode(vals[i])
        assert bool(st[i]) == ok
        if ok:
            assert (got[i] == m).all(), i


# --------------------------------------------------------------------------- whole path
@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encrypt_sym_vs_oracle(env, golden, shape):
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    B = 9 if n >= 8192 else 67
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    vals = V.bench_values(B, n)
    vals[0] = V.survey_values(n)
    ss, sd = V.bench_seeds(B)
    ss[0] = np.frombuffer(V.SURVEY_SHARE_SEED, dtype=np.uint8)
    sd[0] = np.frombuffer(V.SURVEY_SEED, dtype=np.uint8)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    ntt_pte = torch.zeros_like(c0)
    pte = torch.zeros((B, n), dtype=torch.int64, device=env["dev"])
    status = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), c0, c1, ntt_pte, pte, status)
    torch.cuda.synchronize()
    g0, g1, gp, gm = host_u32(c0), host_u32(c1), host_u32(ntt_pte), pte.cpu().numpy()
    assert status.cpu().numpy().all()
    for b in range(B):
        r = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
        assert (gm[b] == r["pte"]).all(), ("pte", b)
        assert (g1[b] == r["c1"]).all(), ("c1", b)
        assert (gp[b] == r["ntt_pte"]).all(), ("ntt_pte", b)
        assert (g0[b] == r["c0"]).all(), ("c0", b)
    g = golden["digests"]["shapes"][f"{n}x{npr}"]["sym_survey"]
    assert V.sha256_hex(g0[0]) == g["c0_sha256"] and V.sha256_hex(g1[0]) == g["c1_sha256"]
    assert V.sha256_hex(gm[0]) == g["pte_sha256"]
    assert V.sha256_hex(gp[0]) == g["c1_alias_sha256"]


@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encrypt_asym_vs_oracle(env, golden, shape):
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    B = 5 if n >= 8192 else 66
    o = Oracle(n, npr)
    sk = V.secret_key(n)
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    g = golden["digests"]["shapes"][f"{n}x{npr}"]["asym_survey"]
    assert V.sha256_hex(pk0) == g["pk0_sha256"]
    ctx = env["pkg"].Context(n, npr)
    ctx.set_public_key(pk0, pk1)
    vals = V.bench_values(B, n)
    vals[0] = V.survey_values(n)
    _, sd = V.bench_seeds(B)
    sd[0] = np.frombuffer(V.SURVEY_SEED, dtype=np.uint8)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    pte = torch.zeros((B, n), dtype=torch.int64, device=env["dev"])
    ctx.encrypt_asym(dev_t(env, vals), dev_t(env, sd), c0, c1, pte=pte)
    torch.cuda.synchronize()
    g0, g1, gm = host_u32(c0), host_u32(c1), pte.cpu().numpy()
    for b in range(B):
        r = o.encrypt_asym(vals[b], sd[b].tobytes(), pk0, pk1)
        assert (gm[b] == r["pte"]).all(), ("pte", b)
        assert (g1[b] == r["c1"]).all(), ("c1", b)
        assert (g0[b] == r["c0"]).all(), ("c0", b)
    assert V.sha256_hex(g0[0]) == g["c0_sha256"] and V.sha256_hex(g1[0]) == g["c1_sha256"]


@pytest.mark.parametrize("shape", [(1024, 1), (4096, 3), (16384, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_pipeline_shapes_agree(env, shape):
    """The symmetric path has four launch shapes (aux-stream overlap on/off x fused / per-prime
    split); all must produce the oracle's bytes."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    B = 66 if n < 16384 else 5
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n, seed=9)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    vals = V.bench_values(B, n, first=31)
    vals[1] *= 1.0e6          # a plaintext beyond 32 bits: takes the general reduction path
    ss, sd = V.bench_seeds(B, first=31)
    exp = [o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk) for b in range(B)]
    for overlap in (0, 1):
        for split in (0, 1):
            ctx.set_pipeline(overlap, split)
            # lane form with helper waves on / off, and (flags 0) the wave-per-ciphertext form
            ctx.set_debug_flags({0: 32, 1: 32 + 8, 2: 0}[overlap + split])
            c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
            c1 = torch.zeros_like(c0)
            ntt_pte = torch.zeros_like(c0)
            ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), c0, c1, ntt_pte)
            torch.cuda.synchronize()
            g0, g1, gp = host_u32(c0), host_u32(c1), host_u32(ntt_pte)
            for b in range(B):
                assert (g0[b] == exp[b]["c0"]).all(), (overlap, split, b)
                assert (g1[b] == exp[b]["c1"]).all(), (overlap, split, b)
                assert (gp[b] == exp[b]["ntt_pte"]).all(), (overlap, split, b)


@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gen_public_key_vs_reference_golden(env, golden, shape):
    """gen_pk on the GPU equals the compiled reference's gen_pk (golden digests) and the oracle."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    g = golden["digests"]["shapes"][f"{n}x{npr}"]["asym_survey"]
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    pk0, pk1 = ctx.gen_public_key(sk, SEED_PK, SEED_EP)
    assert V.sha256_hex(pk0) == g["pk0_sha256"] and V.sha256_hex(pk1) == g["pk1_sha256"]
    o0, o1 = Oracle(n, npr).gen_pk(sk, SEED_PK, SEED_EP)
    assert (pk0 == o0).all() and (pk1 == o1).all()


@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_intt_and_decrypt_decode_vs_oracle_and_golden(env, golden, shape):
    """Verification side: batched ckks_decrypt + intt_inpl + ckks_decode on the
    GPU, bit-exact against the oracle and the compiled reference's golden digests, plus the
    reference's own acceptance criteria (exact pseudo-decrypt, decode within 0.1)."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    g = golden["digests"]["shapes"][f"{n}x{npr}"]["verify_pattern4"]
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    B = 5
    vals = np.stack([V.pattern_values(4, n)] + [V.pattern_values(t, n) * 0.01 for t in (2, 5, 6, 8)])
    ss = np.stack([np.frombuffer(SEED_A, dtype=np.uint8)] * B).copy()
    sd = np.stack([np.frombuffer(SEED_B, dtype=np.uint8)] * B).copy()
    ss[1:] = V.derive_seeds("vfy-a", B - 1)
    sd[1:] = V.derive_seeds("vfy-b", B - 1)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    ntt_pte = torch.zeros_like(c0)
    ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), c0, c1, ntt_pte)
    for j in range(npr):
        dec = torch.zeros((B, n), dtype=torch.int32, device=env["dev"])
        pt = torch.zeros_like(dec)
        out = torch.zeros((B, n // 2), dtype=torch.float32, device=env["dev"])
        ctx.decrypt_decode(c0, c1, j, dec, pt, out)
        torch.cuda.synchronize()
        gd, gp, gv = host_u32(dec), host_u32(pt), out.cpu().numpy()
        assert (gd == host_u32(ntt_pte)[:, j, :]).all()            # exact pseudo-decrypt
        assert V.sha256_hex(gp[0]) == g[f"p{j}"]["pt_sha256"]
        assert V.sha256_hex(gv[0]) == g[f"p{j}"]["values_sha256"]
        for b in range(B):
            ptj = o.intt(gd[b], j)
            assert (gp[b] == ptj).all(), (j, b)
            assert (gv[b].view(np.uint32) == o.decode(ptj, j).view(np.uint32)).all(), (j, b)
            assert np.abs(gv[b] - vals[b]).max() < 0.1            # ckks_tests_common.c:132
        # stand-alone INTT inverts the stand-alone NTT
        rng = np.random.default_rng(n + j)
        x = rng.integers(0, o.q[j], (3, n), dtype=np.uint64).astype(np.uint32)
        t = dev_t(env, x.view(np.int32))
        ctx.ntt(j, t)
        ctx.intt(j, t)
        torch.cuda.synchronize()
        assert (host_u32(t) == x).all()


@pytest.mark.parametrize("shape", [(16384, 13), (8192, 1), (4096, 1), (4096, 2), (16384, 1)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_other_prime_counts_including_maximum(env, shape):
    """Every (degree, nprimes) the reference accepts is a prefix of its prime chain
    (parameters.c:176-230); the largest is n=16384 with all 13 primes."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    B = 3
    o = Oracle(n, npr)
    sk = V.secret_key(n, seed=21)
    ctx = env["pkg"].Context(n, npr)
    assert ctx.moduli() == o.q and ctx.scale() == o.scale
    assert (ctx.index_map() == o.map).all()
    ctx.set_secret_key(sk)
    vals = V.bench_values(B, n, first=90) * np.float32(0.05)
    ss, sd = V.bench_seeds(B, first=90)
    r = ctx.encrypt_sym_host(vals, ss, sd, want_extra=True)
    assert r["failed"] == 0
    pk0, pk1 = ctx.gen_public_key(sk, SEED_PK, SEED_EP)
    ctx.set_public_key(pk0, pk1)
    ra = ctx.encrypt_asym_host(vals, sd)
    for b in range(B):
        e = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
        assert (r["c0"][b] == e["c0"]).all() and (r["c1"][b] == e["c1"]).all()
        assert (r["pte"][b] == e["pte"]).all()
        ea = o.encrypt_asym(vals[b], sd[b].tobytes(), pk0, pk1)
        assert (ra["c0"][b] == ea["c0"]).all() and (ra["c1"][b] == ea["c1"]).all()


def test_seed_compressed_symmetric_ciphertext(env):
    """(share_seed, c0) travels; the receiver re-expands c1 = a from the seed."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 4096, 3, 65
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    vals = V.bench_values(B, n, first=500)
    ss, sd = V.bench_seeds(B, first=500)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    ctx.encrypt_sym_seeded(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), c0)
    c1 = torch.zeros_like(c0)
    env["pkg"].Context(n, npr).expand_c1(dev_t(env, ss), c1)     # a different ("receiver") context
    torch.cuda.synchronize()
    for b in (0, 1, 63, 64):
        r = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
        assert (host_u32(c0[b]) == r["c0"]).all() and (host_u32(c1[b]) == r["c1"]).all()


def test_encode_only_config5(env):
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 4096, 3, 33
    ctx = env["pkg"].Context(n, npr)
    o = Oracle(n, npr)
    vals = V.bench_values(B, n, first=1000)
    out = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    ctx.encode_ntt(dev_t(env, vals), out)
    torch.cuda.synchronize()
    got = host_u32(out)
    for b in range(B):
        ok, m = o.encode(vals[b])
        for j in range(npr):
            assert (got[b, j] == o.ntt(o.reduce_pte(m, j), j)).all()


@pytest.mark.parametrize("B", [1, 3, 130])
def test_pair_form_of_the_fused_kernels_on_odd_batches(env, B):
    """Round 6: the fast symmetric / encode-only kernels at n = 4096 take TWO plaintexts per workgroup (half-size
    transform + guard band + exact redo, encode_encrypt.hip: encrypt_pair).  Odd batches end with a workgroup that holds
    one plaintext; a pair may consist of one ordinary and one declined (large / NaN) plaintext in either position.
    Every record against the oracle, encode-only and fused symmetric, with pte / ntt_pte / status."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = 4096, 3
    o = Oracle(n, npr)
    sk = V.secret_key(n, seed=5)
    vals = V.bench_values(B, n, first=4200 + B)
    if B >= 3:
        vals[1] *= 60.0                 # not small: the general kernel, second of its pair
        vals[B - 1, 7] = float("nan")   # non-finite, last plaintext (first of a one-plaintext workgroup when B is odd)
        # an EXACT rounding tie: a constant slot vector v = 75 / 2^26 encodes to m_0 = v * 2^25 = 37.5 exactly (sums of
        # equal values and the power-of-two scaling are exact), every other coefficient ~0: the half-size transform must
        # flag it (distance 0 to the half-integer) and the full transform must round it half away from zero as round() does
        vals[0, :] = np.float32(75.0 / 2.0 ** 26)
    if B >= 130:
        vals[5, :] = np.float32(-(2 * 4001 + 1) / 2.0 ** 26)   # a negative tie, first of its pair
        # ties decided by ROUNDING NOISE: one non-zero slot v = (2k+1) / 2^15 encodes to m_j = (k + 0.5) cos(phi_j) -- the
        # coefficients with |cos| = 1 land within ~1e-13 of a half-integer after 12 butterfly stages, on whichever side
        # the reference's own rounding errors put them.  Only the full transform can reproduce that; the half-size form
        # must flag these plaintexts (guard band ~1e-10 here)
        for row, slot, k in ((6, 0, 50), (7, 17, 12345), (8, 2047, 3)):
            vals[row, :] = 0.0
            vals[row, slot] = np.float32((2 * k + 1) / 2.0 ** 15)
    if B >= 130:
        vals[64] *= 1000.0              # first of its pair
    ss, sd = V.bench_seeds(B, first=4200 + B)
    ctx = env["pkg"].Context(n, npr)
    ctx.set_secret_key(sk)
    ctx.set_pipeline(True, False)       # the fused kernel whatever the batch
    out = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    pte = torch.zeros((B, n), dtype=torch.int64, device=env["dev"])
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encode_ntt(dev_t(env, vals), out, pte=pte, status=st)
    c0 = torch.zeros_like(out)
    c1 = torch.zeros_like(out)
    npte = torch.zeros_like(out)
    st2 = torch.zeros_like(st)
    ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), c0, c1, npte, None, st2)
    torch.cuda.synchronize()
    got, gpte, g0, g1 = host_u32(out), pte.cpu().numpy(), host_u32(c0), host_u32(c1)
    for b in range(B):
        ok, m = o.encode(vals[b])
        assert int(st[b]) == int(ok) and int(st2[b]) == int(ok), b
        assert np.array_equal(gpte[b], m), b
        for j in range(npr):
            assert (got[b, j] == o.ntt(o.reduce_pte(m, j), j)).all(), (b, j)
        r = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
        assert (g0[b] == r["c0"]).all() and (g1[b] == r["c1"]).all(), b
    ctx.close()


def test_encode_coefficient_of_exactly_2_pow_63(env):
    """A coefficient of exactly +-2^63 is NOT an overflow for the reference (it rejects only
    |coeff| > 2^63, ckks_common.c:195) and its build converts +2^63 to INT64_MIN: a constant vector
    of 2^38 at scale 2^25 produces exactly that in coefficient 0 (all other coefficients 0)."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = 4096, 3
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rows = np.stack([np.full(n // 2, s * 2.0 ** 38, dtype=np.float32) for s in (1.0, -1.0, 0.5, 2.0)])
    out = torch.zeros((4, n), dtype=torch.int64, device=env["dev"])
    st = torch.zeros(4, dtype=torch.uint8, device=env["dev"])
    ctx.encode(dev_t(env, rows), out, st)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b in range(4):
        ok, m = o.encode(rows[b])
        assert bool(st[b]) == ok, b
        if ok:
            assert (got[b] == m).all(), b
    assert list(st.cpu().numpy()) == [1, 1, 1, 0]
    assert got[0, 0] == -2 ** 63 and got[1, 0] == -2 ** 63 and got[2, 0] == 2 ** 62
    res = torch.zeros((4, npr, n), dtype=torch.int32, device=env["dev"])
    ctx.encode_ntt(dev_t(env, rows), res)
    torch.cuda.synchronize()
    for b in range(3):
        ok, m = o.encode(rows[b])
        for j in range(npr):
            assert (host_u32(res[b, j]) == o.ntt(o.reduce_pte(m, j), j)).all(), (b, j)


@pytest.mark.parametrize("n,npr", [(4096, 3), (1024, 1)])
def test_magnitude_classes_through_every_path(env, n, npr):
    """The encoder has a wave-uniform fast path for coefficients below 2 q_min - 64 (one-instruction
    int conversion; m + 2q as the NTT's input representative instead of a signed reduction) and a general
    int64 path.  Plaintexts whose coefficients sit
    well below, just around (2^31 -/+ a few) and far above that boundary go through encode-only,
    symmetric and public-key encryption and must match the oracle (values chosen per row, so
    different waves/workgroups take different paths in one launch)."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    o = Oracle(n, npr)
    scale = o.p.scale
    rng = np.random.default_rng(1234 + n)
    rows = []
    two_q = 2.0 * min(o.q)          # the fast path needs every |m + e| < 2 q_min (single-add representative)
    for amp in (1e-3, 1.0, 30.0, two_q / scale * 0.99, two_q / scale * 0.99999, two_q / scale * 1.00001,
                two_q / scale * 1.01, 2.0 ** 31 / scale * 0.999, 2.0 ** 31 / scale * 1.001, 1e3, 1e6, 1e9):
        rows.append((rng.uniform(-1, 1, n // 2) * amp).astype(np.float32))
        one = np.zeros(n // 2, dtype=np.float32)
        one[int(rng.integers(0, n // 2))] = amp * n / 2       # a single large slot: flat coefficients ~ amp
        rows.append(one)
    vals = np.stack(rows)
    B = vals.shape[0]
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n, seed=9)
    ctx.set_secret_key(sk)
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    ctx.set_public_key(pk0, pk1)
    ss, sd = V.bench_seeds(B, first=4242)
    out = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    pte = torch.zeros((B, n), dtype=torch.int64, device=env["dev"])
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encode_ntt(dev_t(env, vals), out, pte=pte, status=st)
    torch.cuda.synchronize()
    g, gp, gs = host_u32(out), pte.cpu().numpy(), st.cpu().numpy()
    kinds = set()
    for b in range(B):
        ok, m = o.encode(vals[b])
        assert bool(gs[b]) == ok, b
        if not ok:
            continue
        kinds.add(bool(np.abs(m).max() < two_q - 64))
        assert (gp[b] == m).all(), b
        for j in range(npr):
            assert (g[b, j] == o.ntt(o.reduce_pte(m, j), j)).all(), (b, j)
    assert kinds == {True, False}
    for split in (0, 1):
        ctx.set_pipeline(1, split)
        r = ctx.encrypt_sym_host(vals, ss, sd, want_extra=True)
        ra = ctx.encrypt_asym_host(vals, sd, want_extra=True)
        for b in range(B):
            e = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
            ea = o.encrypt_asym(vals[b], sd[b].tobytes(), pk0, pk1)
            assert bool(r["status"][b]) == e["ok"] and bool(ra["status"][b]) == ea["ok"]
            if e["ok"]:
                assert (r["c0"][b] == e["c0"]).all() and (r["c1"][b] == e["c1"]).all(), (split, b)
                assert (r["pte"][b] == e["pte"]).all()
                assert (ra["c0"][b] == ea["c0"]).all() and (ra["c1"][b] == ea["c1"]).all(), (split, b)


def test_contexts_release_their_device_memory(env):
    """Create / use / destroy cycles leave the device's free memory where it was: every table, scratch
    slab (incl. the ones grown by a larger batch), stream and event of a context is released by
    se_amd_destroy."""
    torch = env["torch"]
    n, npr = 4096, 3
    sk = V.secret_key(n)

    def cycle(B):
        ctx = env["pkg"].Context(n, npr)
        ctx.set_secret_key(sk)
        pk0, pk1 = ctx.gen_public_key(sk, SEED_PK, SEED_EP)
        ctx.set_public_key(pk0, pk1)
        vals = V.bench_values(B, n)
        ss, sd = V.bench_seeds(B)
        r = ctx.encrypt_sym_host(vals, ss, sd)
        ra = ctx.encrypt_asym_host(vals, sd)
        assert r["failed"] == 0 and bool(ra["status"].all())
        ctx.close()

    cycle(8)                                         # first use: runtime pools, code objects
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for B in (3, 700, 64, 700):
        cycle(B)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert abs(free0 - free1) <= 8 << 20, (free0, free1)   # allocator granularity, not a leak per cycle


def test_chain_kernels_in_their_1024_thread_form(env):
    """The per-ciphertext chain kernels (uniform `a`, ternary `u`) exist in two instantiations: up to 8
    waves per workgroup (256-VGPR budget, every BASELINE shape) and up to 16 (batches beyond
    8 x 64 x CUs per launch, 128-VGPR budget).  A batch of 140 000 at n = 1024 takes the second form in
    both the symmetric and the public-key path; every ciphertext is compared with the oracle."""
    from oracle import pyoracle
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 1024, 1, 140000
    o = Oracle(n, npr)
    nth = pyoracle.host_threads()
    vals = V.bench_values(B, n, first=5)
    ss, sd = V.bench_seeds(B, first=999)
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n, seed=11)
    ctx.set_secret_key(sk)
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    ctx.set_public_key(pk0, pk1)
    dv, dss, dsd = dev_t(env, vals), dev_t(env, ss), dev_t(env, sd)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    for split in (0, 1):
        ctx.set_pipeline(1, split)
        c0.zero_(), c1.zero_()
        ctx.encrypt_sym(dv, dss, dsd, c0, c1, status=st)
        torch.cuda.synchronize()
        _compare_all_with_oracle(c0, c1, lambda lo, hi: o.encrypt_sym_batch(vals[lo:hi], ss[lo:hi], sd[lo:hi], sk,
                                                                           nthreads=nth), B, chunk=35000)
    c0.zero_(), c1.zero_()
    ctx.encrypt_asym(dv, dsd, c0, c1, status=st)
    torch.cuda.synchronize()
    _compare_all_with_oracle(c0, c1, lambda lo, hi: o.encrypt_asym_batch(vals[lo:hi], sd[lo:hi], pk0, pk1,
                                                                        nthreads=nth), B, chunk=35000)
    assert bool(st.all())


@pytest.mark.parametrize("n,npr,B,large_every", [(1024, 1, 2600, 1), (2048, 1, 1500, 2), (4096, 3, 1300, 3)])
def test_declined_plaintexts_take_the_general_kernel(env, n, npr, B, large_every):
    """The fused kernel is two launches: the fast form (int32 plaintext) declines every plaintext with a
    coefficient >= 2 q_min - 64 and queues it for k_encode_encrypt_general, which walks the queue with a
    grid of 4 workgroups per CU.  Batches in which every / every 2nd / every 3rd plaintext is too large
    (more queued plaintexts than that grid has workgroups at n = 1024 and 2048) must equal the oracle on
    all three entries, element for element."""
    from oracle import pyoracle
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    o = Oracle(n, npr)
    nth = pyoracle.host_threads()
    two_q = 2.0 * min(o.q)
    vals = V.bench_values(B, n, first=77).copy()     # |value| <= 25.5
    vals *= min(1.0, 0.25 * two_q / (o.p.scale * 25.5))   # n = 2048: scale 2^25 over a 27-bit prime
    vals[::large_every] *= 100.0                    # far above 2 q_min
    assert np.abs(o.encode(vals[0])[1]).max() > two_q and (large_every == 1 or
                                                            np.abs(o.encode(vals[1])[1]).max() < two_q - 64)
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n, seed=5)
    ctx.set_secret_key(sk)
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    ctx.set_public_key(pk0, pk1)
    ss, sd = V.bench_seeds(B, first=31337)
    dv, dss, dsd = dev_t(env, vals), dev_t(env, ss), dev_t(env, sd)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.set_pipeline(1, 0)                           # the fused symmetric kernel at every degree
    ctx.encrypt_sym(dv, dss, dsd, c0, c1, status=st)
    torch.cuda.synchronize()
    ok, e0, e1 = o.encrypt_sym_batch(vals, ss, sd, sk, nthreads=nth)
    assert ok and bool(st.all())
    assert np.array_equal(host_u32(c0), e0) and np.array_equal(host_u32(c1), e1)
    c0.zero_(), c1.zero_(), st.zero_()
    ctx.encrypt_asym(dv, dsd, c0, c1, status=st)
    torch.cuda.synchronize()
    ok, e0, e1 = o.encrypt_asym_batch(vals, sd, pk0, pk1, nthreads=nth)
    assert ok and bool(st.all())
    assert np.array_equal(host_u32(c0), e0) and np.array_equal(host_u32(c1), e1)
    c0.zero_(), st.zero_()
    ctx.encode_ntt(dv, c0, status=st)
    torch.cuda.synchronize()
    ok, e0 = o.encode_ntt_batch(vals, nthreads=nth)
    assert ok and bool(st.all()) and np.array_equal(host_u32(c0), e0)


@pytest.mark.parametrize("n,npr,B", [(4096, 3, 1), (4096, 3, 5), (4096, 2, 16), (8192, 6, 2), (16384, 6, 1),
                                       (16384, 3, 2), (16384, 13, 1)])
def test_small_batch_prime_speculation(env, n, npr, B):
    """Host-pointer calls with a handful of ciphertexts run every prime's uniform sampler at once
    under guessed start counters (k_spec_*, Context::encrypt_sym_small) and then follow the true
    counter chain through the guesses.  Results must equal the oracle's; with debug flag 256 every
    window has a single guess, so the chain misses and the call is redone sequentially."""
    from oracle.pyoracle import Oracle
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n, seed=3)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    vals = V.bench_values(B, n, first=31)
    ss, sd = V.bench_seeds(B, first=900)
    exp = [o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk) for b in range(B)]
    for flags in (0, 256, 32, 32 + 256):           # wave-per-ciphertext chains / lane-per-ciphertext chains
        ctx.set_debug_flags(flags)
        for rep in range(2):                       # second call reuses streams and scratch
            r = ctx.encrypt_sym_host(vals, ss, sd, want_extra=True)
            assert r["failed"] == 0
            for b in range(B):
                assert (r["c0"][b] == exp[b]["c0"]).all() and (r["c1"][b] == exp[b]["c1"]).all(), (flags, b)
                assert (r["ntt_pte"][b] == exp[b]["ntt_pte"]).all() and (r["pte"][b] == exp[b]["pte"]).all()


@pytest.mark.parametrize("cus,spec,staged,B", [("16", None, None, 8), ("16", "1", None, 2), ("32", "0", None, 3),
                                               ("16", None, "1", 300), ("64", None, "0", 1100)])
def test_small_device_dispatch_limits(env, monkeypatch, cus, spec, staged, B):
    """The dispatch on a device / partition with few CUs (SE_AMD_NUM_CUS plans launches as if the device had k
    CUs) and under the form overrides SE_AMD_SPECULATION / SE_AMD_STAGED.  Round-3 advisor finding: with 16 CUs
    the guesses of 8 ciphertexts at n = 8192 x 6 (about 1 200 virtual ciphertexts each) exceed the 512 per CU the
    lane form's per-lane-prime instantiation serves; the plan is refused now (the call used to fail with
    hipErrorInvalidValue) and the ordinary per-prime chain runs.  Bit-exact vs the oracle in every case."""
    from oracle.pyoracle import Oracle
    monkeypatch.setenv("SE_AMD_NUM_CUS", cus)
    if spec is not None:
        monkeypatch.setenv("SE_AMD_SPECULATION", spec)
    if staged is not None:
        monkeypatch.setenv("SE_AMD_STAGED", staged)
    n, npr = (8192, 6) if B <= 8 else (1024, 1)
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n, seed=3)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    vals = V.bench_values(B, n, first=5)
    ss, sd = V.bench_seeds(B, first=77)
    for rep in range(2):
        r = ctx.encrypt_sym_host(vals, ss, sd)
        assert r["failed"] == 0
        for b in sorted({0, 1, B // 2, B - 1} & set(range(B))):
            e = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
            assert (r["c0"][b] == e["c0"]).all() and (r["c1"][b] == e["c1"]).all(), (rep, b)
    ctx.close()


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 129])
def test_ragged_batch_sizes(env, B):
    from oracle.pyoracle import Oracle
    n, npr = 1024, 1
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n, seed=5)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    vals = V.bench_values(B, n, first=7)
    ss, sd = V.bench_seeds(B, first=7)
    r = ctx.encrypt_sym_host(vals, ss, sd)
    assert r["failed"] == 0
    for b in sorted({0, B // 2, B - 1}):
        e = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
        assert (r["c0"][b] == e["c0"]).all() and (r["c1"][b] == e["c1"]).all()


def test_empty_batch_and_missing_key(env):
    pkg = env["pkg"]
    ctx = pkg.Context(1024, 1)
    with pytest.raises(pkg.SealEmbeddedAmdError):
        ctx.encrypt_sym_host(V.bench_values(1, 1024), *V.bench_seeds(1))   # no key set
    ctx.set_secret_key(V.secret_key(1024))
    r = ctx.encrypt_sym_host(np.zeros((0, 512), dtype=np.float32), np.zeros((0, 64), np.uint8),
                             np.zeros((0, 64), np.uint8))
    assert r["failed"] == 0 and r["c0"].shape[0] == 0
    with pytest.raises(pkg.SealEmbeddedAmdError):
        pkg.Context(1000, 1)            # unsupported degree
    with pytest.raises(pkg.SealEmbeddedAmdError):
        pkg.Context(4096, 4)            # too many primes for n=4096 (parameters.c:212)


@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nonfinite_values_through_every_path(env, golden, shape):
    """NaN, +-Inf, FLT_MAX, subnormal and -0.0 plaintext values (tests/vectors.py, nonfinite_values) through
    every batched entry.  The reference ACCEPTS a NaN coefficient (fabs(NaN) > 2^63 is false,
    ckks_common.c:195; its x86-64 build stores INT64_MIN) and rejects an infinite one; which coefficients are
    which is decided by its Annex-G complex product (oracle/se_oracle.c, seo_cmul; transform.cuh,
    cmul_annexg).  The device's fast kernels decline such plaintexts, the general kernels reproduce them.
    Checked against the goldens of the compiled reference AND the oracle, ordinary plaintexts interleaved so
    that one launch mixes fast and general workgroups."""
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = shape
    o = Oracle(n, npr)
    gold = golden["digests"]["shapes"][f"{n}x{npr}"]["encode"]["nonfinite"]
    rows, case_of = [], []
    ordinary = V.bench_values(V.NONFINITE_CASES, n, first=77)
    for c in range(V.NONFINITE_CASES):
        rows.append(V.nonfinite_values(c, n)), case_of.append(c)
        rows.append(ordinary[c]), case_of.append(None)
    vals = np.stack(rows)
    B = vals.shape[0]
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n, seed=11)
    ctx.set_secret_key(sk)
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    ctx.set_public_key(pk0, pk1)
    ss, sd = V.bench_seeds(B, first=9000)

    # ckks_encode_base (int64 plaintext + status), and encode + RNS + NTT
    pte = torch.zeros((B, n), dtype=torch.int64, device=env["dev"])
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encode(dev_t(env, vals), pte, st)
    out = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    pte2 = torch.zeros((B, n), dtype=torch.int64, device=env["dev"])
    st2 = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encode_ntt(dev_t(env, vals), out, pte=pte2, status=st2)
    torch.cuda.synchronize()
    gp, gs, gp2, gs2, gout = pte.cpu().numpy(), st.cpu().numpy(), pte2.cpu().numpy(), st2.cpu().numpy(), host_u32(out)
    accepted_nan = rejected = 0
    for b in range(B):
        idx, m = o.encode_ex(vals[b])
        ok = idx == n
        if case_of[b] is not None:
            g = gold[case_of[b]]
            assert idx == g["fail_index"], (b, case_of[b])
            if ok:
                assert V.sha256_hex(gp[b]) == g["prefix_sha256"], (b, case_of[b])
                assert int((gp[b] == -2 ** 63).sum()) == g["int64_min_count"]
                accepted_nan += g["int64_min_count"] > 0
            rejected += not ok
        assert bool(gs[b]) == ok and bool(gs2[b]) == ok, (b, case_of[b], gs[b], gs2[b], ok)
        if ok:
            assert (gp[b] == m).all() and (gp2[b] == m).all(), (b, case_of[b])
            for j in range(npr):
                assert (gout[b, j] == o.ntt(o.reduce_pte(m, j), j)).all(), (b, j)
    assert accepted_nan >= 3 and rejected >= 5

    # symmetric (fused and split pipelines) and public-key encryption
    for split in (0, 1):
        ctx.set_pipeline(1, split)
        r = ctx.encrypt_sym_host(vals, ss, sd, want_extra=True)
        ra = ctx.encrypt_asym_host(vals, sd, want_extra=True)
        for b in range(B):
            e = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
            ea = o.encrypt_asym(vals[b], sd[b].tobytes(), pk0, pk1)
            assert bool(r["status"][b]) == e["ok"] and bool(ra["status"][b]) == ea["ok"], (split, b, case_of[b])
            if e["ok"]:
                assert (r["pte"][b] == e["pte"]).all(), (split, b, case_of[b])
                assert (r["c0"][b] == e["c0"]).all() and (r["c1"][b] == e["c1"]).all(), (split, b, case_of[b])
                assert (ra["c0"][b] == ea["c0"]).all() and (ra["c1"][b] == ea["c1"]).all(), (split, b)
                if case_of[b] is not None and "c0_sha256" not in gold[case_of[b]]:
                    raise AssertionError("golden lacks the accepted case")
    # the compiled reference's own ciphertext digests for the accepted cases (golden seeds)
    acc = [c for c in range(V.NONFINITE_CASES) if gold[c]["fail_index"] == n]
    av = np.stack([V.nonfinite_values(c, n) for c in acc])
    ctx.set_secret_key(V.secret_key(n))
    sa = np.tile(np.frombuffer(SEED_A, dtype=np.uint8), (len(acc), 1))
    sb = np.tile(np.frombuffer(SEED_B, dtype=np.uint8), (len(acc), 1))
    r = ctx.encrypt_sym_host(av, sa, sb, want_extra=True)
    for i, c in enumerate(acc):
        assert r["status"][i] == 1
        assert V.sha256_hex(r["c0"][i]) == gold[c]["c0_sha256"], c
        assert V.sha256_hex(r["pte"][i]) == gold[c]["pte_sha256"], c
    ctx.close()


def test_nonfinite_plaintexts_fill_a_whole_launch(env):
    """More NaN plaintexts than the general kernels' grids have workgroups (their queue loops), all of them
    accepted, every second one ordinary; small batch shape and full-chip shape of the symmetric pipeline."""
    from oracle.pyoracle import Oracle
    n, npr, B = 1024, 1, 2300
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    vals = V.bench_values(B, n, first=5)
    vals[0::2, 3] = np.nan
    vals[1::4, 7] = np.float32(-0.0)
    ss, sd = V.bench_seeds(B, first=123)
    for split in (0, 1):
        ctx.set_pipeline(1, split)
        r = ctx.encrypt_sym_host(vals, ss, sd, want_extra=True)
        assert r["failed"] == 0
        ok, e0, e1 = o.encrypt_sym_batch(vals, ss, sd, sk, nthreads=8)
        assert ok and np.array_equal(r["c0"], e0) and np.array_equal(r["c1"], e1), split
        assert (r["pte"][0::2] == -2 ** 63).sum() > 0
    ctx.close()


def test_overflow_reports_failed_plaintexts(env):
    n = 1024
    ctx = env["pkg"].Context(n, 1)
    ctx.set_secret_key(V.secret_key(n))
    vals = V.bench_values(3, n)
    vals[1, :] = 3.0e38
    r = ctx.encrypt_sym_host(vals, *V.bench_seeds(3))
    assert r["failed"] == 1 and list(r["status"]) == [1, 0, 1]


# --------------------------------------------------------------------------- full-size properties
def _compare_all_with_oracle(c0, c1, oracle_chunk, B, chunk=4096):
    """EVERY ciphertext of a full batch against the threaded oracle, chunk by chunk (bounded host
    memory): exact element-wise equality of the c0 and c1 records."""
    # the oracle's C threads work on chunk k + 1 while this thread copies chunk k back and compares it
    from concurrent.futures import ThreadPoolExecutor
    spans = [(lo, min(B, lo + chunk)) for lo in range(0, B, chunk)]
    pool = ThreadPoolExecutor(1)
    nxt = pool.submit(oracle_chunk, *spans[0])
    for i, (lo, hi) in enumerate(spans):
        ok, e0, e1 = nxt.result()
        if i + 1 < len(spans):
            nxt = pool.submit(oracle_chunk, *spans[i + 1])
        assert ok
        g0 = host_u32(c0[lo:hi])
        assert np.array_equal(g0, e0), f"c0 differs in ciphertexts [{lo},{hi})"
        del g0, e0
        if c1 is not None:
            g1 = host_u32(c1[lo:hi])
            assert np.array_equal(g1, e1), f"c1 differs in ciphertexts [{lo},{hi})"
            del g1
        del e1
    pool.shutdown()


@pytest.mark.parametrize("form", ["dispatch"])
def test_full_size_properties_config2(env, form):
    """(form: what the library's dispatch picks at this batch -- one-launch lane chains || CBD, then the fused kernel;
    SE_TEST_C2_FORMS=split adds the per-prime software pipeline forced at the same batch.)
    BASELINE config 2 shape (n=4096, 3 primes) at a large batch: (a) the reference's own
    round-trip criterion c0 + c1*NTT(s) == NTT(m+e) exactly (ckks_tests_common.c:206) evaluated
    on the GPU outputs for EVERY ciphertext; (b) oracle spot checks on scattered records;
    (c) determinism: a second run gives identical bytes; (d) EXHAUSTIVE parity: all B ciphertexts
    (c0 and c1, every coefficient) equal the threaded oracle's."""
    from oracle import pyoracle
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = 4096, 3
    B = int(os.environ.get("SE_TEST_FULL_B", "65536"))   # BASELINE config 2 batch
    ctx = env["pkg"].Context(n, npr)
    if form == "split_pipeline" or os.environ.get("SE_TEST_C2_FORMS") == "split":
        ctx.set_pipeline(True, True)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    vals = V.bench_values(B, n)
    ss, sd = V.bench_seeds(B)
    dv, dss, dsd = dev_t(env, vals), dev_t(env, ss), dev_t(env, sd)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    ntt_pte = torch.zeros_like(c0)
    status = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encrypt_sym(dv, dss, dsd, c0, c1, ntt_pte, None, status)
    torch.cuda.synchronize()
    assert bool(status.all())
    for j in range(npr):
        q = o.q[j]
        s_hat = dev_t(env, o.ntt(o.expand_ternary(sk, j), j).astype(np.int64))
        a = c1[:, j, :].to(torch.int64)
        lhs = (c0[:, j, :].to(torch.int64) + (a * s_hat) % q) % q
        assert bool((lhs == ntt_pte[:, j, :].to(torch.int64)).all()), j
        assert int(c0[:, j, :].max()) < q and int(c0[:, j, :].min()) >= 0
        assert int(c1[:, j, :].max()) < q and int(c1[:, j, :].min()) >= 0
    # (a') the same criterion plus decode-within-0.1 through the on-GPU verifier
    # (se_amd_decrypt_decode_device), every ciphertext, prime 0
    dec = torch.zeros((B, n), dtype=torch.int32, device=env["dev"])
    dvals = torch.zeros((B, n // 2), dtype=torch.float32, device=env["dev"])
    ctx.decrypt_decode(c0, c1, 0, dec, None, dvals)
    torch.cuda.synchronize()
    assert bool((dec == ntt_pte[:, 0, :]).all())
    assert float((dvals - dv).abs().max()) < 0.1          # ckks_tests_common.c:132,228
    d0 = torch.zeros_like(c0)
    d1 = torch.zeros_like(c0)
    ctx.encrypt_sym(dv, dss, dsd, d0, d1)
    torch.cuda.synchronize()
    assert bool((d0 == c0).all()) and bool((d1 == c1).all())
    del d0, d1, dec, dvals, ntt_pte
    nt = pyoracle.host_threads()
    _compare_all_with_oracle(c0, c1, lambda lo, hi: o.encrypt_sym_batch(vals[lo:hi], ss[lo:hi], sd[lo:hi], sk,
                                                                        nthreads=nt), B)


def test_full_size_properties_config4(env):
    """BASELINE config 4 shape at its per-GPU batch (n=16384, 6 primes, 32768 ciphertexts = 24 GiB
    of output), every plaintext distinct: the exact round-trip criterion through the on-GPU verifier
    for every ciphertext (first and last prime), canonical ranges, and EXHAUSTIVE parity: all 32 768
    ciphertexts (c0 and c1, every coefficient) equal the threaded oracle's."""
    from oracle import pyoracle
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = 16384, 6
    B = int(os.environ.get("SE_TEST_FULL_B4", "32768"))
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    vals = V.bench_values(B, n)                          # B distinct plaintexts (1 GiB)
    ss, sd = V.bench_seeds(B)
    dv, dss, dsd = dev_t(env, vals), dev_t(env, ss), dev_t(env, sd)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    ntt_pte = torch.zeros_like(c0)
    status = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encrypt_sym(dv, dss, dsd, c0, c1, ntt_pte, None, status)
    torch.cuda.synchronize()
    assert bool(status.all())
    dec = torch.zeros((B, n), dtype=torch.int32, device=env["dev"])
    for j in (0, npr - 1):
        q = o.q[j]
        ctx.decrypt_decode(c0, c1, j, dec, None, None)
        torch.cuda.synchronize()
        assert bool((dec == ntt_pte[:, j, :]).all()), j
        for t in (c0, c1):
            assert int(t[:, j, :].max()) < q and int(t[:, j, :].min()) >= 0
    del dec, ntt_pte
    # EXHAUSTIVE parity: every one of the B ciphertexts (48 GiB of c0 + c1) against the threaded oracle
    nt = pyoracle.host_threads()
    _compare_all_with_oracle(c0, c1, lambda lo, hi: o.encrypt_sym_batch(vals[lo:hi], ss[lo:hi], sd[lo:hi], sk,
                                                                       nthreads=nt), B, chunk=512)


def test_full_size_properties_config3(env):
    """BASELINE config 3 (public-key, n=4096, 3 primes) at batch 65536: canonical ranges,
    determinism, and EXHAUSTIVE parity -- all B ciphertexts equal the threaded oracle's."""
    from oracle import pyoracle
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = 4096, 3
    B = int(os.environ.get("SE_TEST_FULL_B", "65536"))
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    o = Oracle(n, npr)
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    ctx.set_public_key(pk0, pk1)
    vals = V.bench_values(B, n)
    _, sd = V.bench_seeds(B)
    dv, dsd = dev_t(env, vals), dev_t(env, sd)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    status = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encrypt_asym(dv, dsd, c0, c1, status=status)
    torch.cuda.synchronize()
    assert bool(status.all())
    for j in range(npr):
        for t in (c0, c1):
            assert int(t[:, j, :].max()) < o.q[j] and int(t[:, j, :].min()) >= 0
    d0, d1 = torch.zeros_like(c0), torch.zeros_like(c0)
    ctx.encrypt_asym(dv, dsd, d0, d1)
    torch.cuda.synchronize()
    assert bool((d0 == c0).all()) and bool((d1 == c1).all())
    del d0, d1
    nt = pyoracle.host_threads()
    _compare_all_with_oracle(c0, c1, lambda lo, hi: o.encrypt_asym_batch(vals[lo:hi], sd[lo:hi], pk0, pk1,
                                                                         nthreads=nt), B)


def test_full_size_encode_only_config5(env):
    """BASELINE config 5 at its full batch (n=4096, 3 primes, encode + RNS + NTT, 1 048 576
    plaintexts = 48 GiB of output, all distinct): canonical ranges for every record, and EXHAUSTIVE
    parity: all 1 048 576 records equal the threaded oracle's, element for element."""
    from oracle import pyoracle
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr = 4096, 3
    B = int(os.environ.get("SE_TEST_FULL_B5", "1048576"))
    ctx = env["pkg"].Context(n, npr)
    o = Oracle(n, npr)
    import bench
    dv = bench.bench_values_device(B, n, env["dev"])
    out = torch.empty((B, npr, n), dtype=torch.int32, device=env["dev"])
    status = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encode_ntt(dv, out, status=status)
    torch.cuda.synchronize()
    assert bool(status.all())
    step = 65536
    for lo in range(0, B, step):
        blk = out[lo:lo + step]
        for j in range(npr):
            assert int(blk[:, j, :].max()) < o.q[j] and int(blk[:, j, :].min()) >= 0
    # EXHAUSTIVE parity: every one of the B records against the threaded oracle (same counter-based
    # values, regenerated on the host chunk by chunk)
    # (the next chunk's values are generated by a helper thread while the oracle's C threads work on this one: numpy and
    # ctypes both release the GIL -- 63 -> ~45 s of a GPU suite the driver runs under a budget)
    from concurrent.futures import ThreadPoolExecutor
    nt = pyoracle.host_threads()
    chunks = [(a, min(B, a + 8192)) for a in range(0, B, 8192)]
    with ThreadPoolExecutor(1) as pool:
        nxt = pool.submit(V.bench_values, chunks[0][1] - chunks[0][0], n, first=chunks[0][0])
        for i, (a, b) in enumerate(chunks):
            vals = nxt.result()
            if i + 1 < len(chunks):
                nxt = pool.submit(V.bench_values, chunks[i + 1][1] - chunks[i + 1][0], n, first=chunks[i + 1][0])
            ok, e = o.encode_ntt_batch(vals, nthreads=nt)
            assert ok and np.array_equal(host_u32(out[a:b]), e), f"records [{a},{b}) differ"


# --------------------------------------------------------------------------- reference API layer
def test_reference_api_callback_stream(env, golden, tmp_path):
    """se_setup / se_encrypt_seeded through the drop-in symbols: 2*np callbacks of 4n bytes, c0
    then c1 per prime; with SE_AMD_REFERENCE_C1_ALIAS=1 the byte stream equals the compiled
    reference's (FNV digest in the golden file), without it c1 is the true `a`."""
    from oracle import pyoracle
    from oracle.pyoracle import Oracle
    L = env["pkg"].lib()
    n, npr = 4096, 3
    d = golden["digests"]["shapes"][f"{n}x{npr}"]
    data = tmp_path / "adapter_output_data"
    data.mkdir()
    sk = V.secret_key(n)
    sk.tofile(data / f"sk_{n}.dat")
    os.environ["SE_AMD_DATA_PATH"] = str(data)

    class SE_PARMS(C.Structure):
        _fields_ = [("parms", C.c_void_p), ("se_ptrs", C.c_void_p)]

    SEND = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.c_size_t)
    L.se_setup.restype = C.POINTER(SE_PARMS)
    L.se_setup.argtypes = [C.c_size_t, C.c_size_t, C.c_double, C.c_int]
    L.se_encrypt_seeded.restype = C.c_bool
    L.se_encrypt_seeded.argtypes = [C.c_void_p, C.c_void_p, SEND, C.c_void_p, C.c_size_t,
                                    C.c_bool, C.POINTER(SE_PARMS)]
    L.se_cleanup.argtypes = [C.POINTER(SE_PARMS)]
    chunks = []

    def cb(ptr, nbytes):
        chunks.append(C.string_at(ptr, nbytes))
        return nbytes

    vals = V.survey_values(n)
    s1 = (C.c_uint8 * 64).from_buffer_copy(V.SURVEY_SHARE_SEED)
    s2 = (C.c_uint8 * 64).from_buffer_copy(V.SURVEY_SEED)
    o = Oracle(n, npr)
    exp = o.encrypt_sym(vals, V.SURVEY_SHARE_SEED, V.SURVEY_SEED, sk)
    try:
        for alias in ("1", "0"):
            os.environ["SE_AMD_REFERENCE_C1_ALIAS"] = alias
            sp = L.se_setup(n, npr, 0.0, 0)
            chunks.clear()
            ok = L.se_encrypt_seeded(s1, s2, SEND(cb), vals.ctypes.data, vals.nbytes, False, sp)
            assert ok and len(chunks) == 2 * npr and all(len(c) == 4 * n for c in chunks)
            stream = b"".join(chunks)
            if alias == "1":
                assert "%016x" % pyoracle.fnv1a64(stream) == d["api_fnv1a64_sym"]
                # print = true: the reference's print_poly("c0: ", ...) lines (seal_embedded.c:160-163,
                # SE_PRINT_SMALL: 8 values then "... }"), captured at the file-descriptor level
                import sys
                cap = tmp_path / "printed.txt"
                sys.stdout.flush()
                saved, fd = os.dup(1), os.open(str(cap), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
                os.dup2(fd, 1)
                try:
                    ok = L.se_encrypt_seeded(s1, s2, SEND(cb), vals.ctypes.data, vals.nbytes, True, sp)
                    C.CDLL(None).fflush(None)
                finally:
                    os.dup2(saved, 1)
                    os.close(saved)
                    os.close(fd)
                assert ok
                lines = [l for l in cap.read_text().splitlines(True) if l.startswith(("c0: ", "c1: "))]
                assert lines == d["api_print_sym"]
            else:
                want = b"".join(exp["c0"][j].tobytes() + exp["c1"][j].tobytes() for j in range(npr))
                assert stream == want
            L.se_cleanup(sp)
    finally:
        os.environ.pop("SE_AMD_REFERENCE_C1_ALIAS", None)
        os.environ.pop("SE_AMD_DATA_PATH", None)


# --------------------------------------------------------------------------- C callers (examples/)
def _key_dir(env, tmp_path, n, npr, asym):
    data = tmp_path / f"adapter_output_data_{n}_{int(asym)}"
    data.mkdir()
    sk = V.secret_key(n)
    sk.tofile(data / f"sk_{n}.dat")
    if asym:
        ctx = env["pkg"].Context(n, npr)
        pk0, pk1 = ctx.gen_public_key(sk, SEED_PK, SEED_EP)
        for j, q in enumerate(ctx.moduli()):
            pk0[j].tofile(data / f"pk0_ntt_{n}_{q}.dat")
            pk1[j].tofile(data / f"pk1_ntt_{n}_{q}.dat")
        ctx.close()
    return data


@pytest.mark.parametrize("shape,mode", [((1024, 1), "sym"), ((4096, 3), "sym"), ((4096, 3), "asym"),
                                        ((16384, 6), "sym")])
def test_c_caller_of_reference_api_reproduces_reference_digest(env, golden, tmp_path, shape, mode):
    """examples/api_digest.c is written against the reference's API only and linked against this
    library with plain gcc; with SE_AMD_REFERENCE_C1_ALIAS=1 its callback byte stream has the FNV
    digest the compiled reference produced for the same input (golden, made by make_golden.py)."""
    import subprocess
    n, npr = shape
    exe = build_example("api_digest", tmp_path)
    data = _key_dir(env, tmp_path, n, npr, mode == "asym")
    e = dict(os.environ, SE_AMD_DATA_PATH=str(data), SE_AMD_REFERENCE_C1_ALIAS="1")
    out = subprocess.run([str(exe), str(n), str(npr), mode], env=e, check=True, capture_output=True,
                         text=True, timeout=300).stdout
    line = [l for l in out.splitlines() if l.startswith("ok=")][-1]
    kv = dict(f.split("=") for f in line.split())
    assert kv["ok"] == "1" and int(kv["callbacks"]) == 2 * npr and int(kv["bytes"]) == 8 * n * npr
    assert kv["fnv1a64"] == golden["digests"]["shapes"][f"{n}x{npr}"][f"api_fnv1a64_{mode}"]


@pytest.mark.parametrize("devices", [None, "0,0", "0,0,0", "visible:0,0", "inject1:0,0,0"])
def test_c_caller_of_batch_entry(env, tmp_path, devices):
    """examples/batch_encrypt.c: se_encrypt_batch from C with malloc'ed (pageable) buffers; the
    records equal the oracle's per-ciphertext results in the reference's callback order.  With
    SE_AMD_DEVICES the batch is sharded over several contexts in one process (one host thread per
    device; the same device listed repeatedly here, a single-GPU box, still exercises the split; 7
    ciphertexts over 2 or 3 devices = unequal shards).  SE_AMD_DEVICES holds HIP ordinals, i.e. positions
    in the process's visible-device list: under HIP_VISIBLE_DEVICES they are remapped like every HIP
    index ("visible:" case), and an ordinal outside that list is refused at se_setup.  "inject1": shard 1
    fails (fault injection) and is re-run on the next healthy device slot -- identical records."""
    import subprocess
    from oracle import pyoracle
    from oracle.pyoracle import Oracle
    n, npr, B = 1024, 1, 7
    exe = build_example("batch_encrypt", tmp_path)
    data = _key_dir(env, tmp_path, n, npr, False)
    e = dict(os.environ, SE_AMD_DATA_PATH=str(data))
    inject = None
    if devices and devices.startswith("inject"):
        # a shard whose device "fails" (fault injection) is re-run on a healthy one: same records
        inject, devices = devices.split(":", 1)
        e["SE_AMD_INJECT_SHARD_FAILURE"] = inject[len("inject"):]
        # the hook exists only in the test build of the library (make testhooks, -DSEAMD_TEST_HOOKS), which
        # the loader finds first through LD_LIBRARY_PATH; the product ignores the variable (checked below)
        ignored = subprocess.run([str(exe), str(n), str(npr), str(B)], env=dict(e, SE_AMD_DEVICES=devices),
                                 check=True, capture_output=True, text=True, timeout=300)
        assert "re-running" not in ignored.stderr
        e["LD_LIBRARY_PATH"] = env["pkg"].TESTHOOKS_LIB_DIR + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    if devices and devices.startswith("visible:"):
        e["HIP_VISIBLE_DEVICES"] = "0"
        devices = devices.split(":", 1)[1]
        bad = subprocess.run([str(exe), str(n), str(npr), str(B)], env=dict(e, SE_AMD_DEVICES="0,1"),
                             capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0 and "device index out of range" in bad.stderr
    if devices:
        e["SE_AMD_DEVICES"] = devices
    res = subprocess.run([str(exe), str(n), str(npr), str(B)], env=e, check=True, capture_output=True,
                         text=True, timeout=300)
    out = res.stdout
    if inject:
        assert "shard 1" in res.stderr and "re-running it on device slot 2" in res.stderr
    kv = dict(f.split("=") for f in [l for l in out.splitlines() if l.startswith("failed=")][-1].split())
    o = Oracle(n, npr)
    sk = V.secret_key(n)
    h = 0xcbf29ce484222325
    first = None
    for b in range(B):
        i = np.arange(n // 2, dtype=np.uint64) + np.uint64(b)
        with np.errstate(over="ignore"):
            v = ((i * np.uint64(2654435761)) % np.uint64(100000)).astype(np.float64) / 1000 - 50
        share = bytes((k + b) & 255 for k in range(64))
        seed = bytes((255 - k + 3 * b) & 255 for k in range(64))
        r = o.encrypt_sym(v.astype(np.float32), share, seed, sk)
        for j in range(npr):
            h = pyoracle.fnv1a64(r["c0"][j].tobytes(), h)
            h = pyoracle.fnv1a64(r["c1"][j].tobytes(), h)
        if b == 0:
            first = h
    assert kv["failed"] == "0"
    assert kv["first"] == "%016x" % first and kv["all"] == "%016x" % h


@pytest.mark.parametrize("devices,B", [("0", 7), ("0,0", 7), ("0,0,0", 200), ("0,0,0,0,0,0,0,0", 5)])
def test_c_caller_of_multi_device_entry(env, tmp_path, devices, B):
    """examples/multi_device_encrypt.c: se_amd_encrypt_sym_multi_device from plain C with hipMalloc'ed blocks
    (one per group member, inputs and outputs resident on the member's device) and the peer-to-peer gather
    into the root's slab, the root producing its block in place.  The gathered records equal the oracle's in
    batch order however many members the batch is cut over (a single-GPU box lists the same ordinal
    several times: separate contexts, streams and host threads; 5 units over 8 members leaves members with
    EMPTY blocks, 7 over 2 and 200 over 3 unequal ones)."""
    import subprocess
    from oracle import pyoracle
    from oracle.pyoracle import Oracle
    n, npr = 1024, 1
    exe = build_example("multi_device_encrypt", tmp_path, hip=True)
    sk = V.secret_key(n)
    skf = tmp_path / "sk.dat"
    sk.tofile(skf)
    res = subprocess.run([str(exe), str(n), str(npr), str(B), devices, str(skf)], check=True, capture_output=True,
                         text=True, timeout=300)
    kv = dict(f.split("=") for f in [l for l in res.stdout.splitlines() if l.startswith("failed=")][-1].split())
    assert kv["failed"] == "0" and int(kv["devices"]) == len(devices.split(","))
    # the program compared the gathered slab with one single-device pass over the whole batch itself
    assert kv["gather_verified"] == "1" and kv["distinct_devices"] == "1"
    o = Oracle(n, npr)
    h = 0xcbf29ce484222325
    for b in range(B):
        i = np.arange(n // 2, dtype=np.uint64) + np.uint64(b)
        with np.errstate(over="ignore"):
            v = ((i * np.uint64(2654435761)) % np.uint64(100000)).astype(np.float64) / 1000 - 50
        share = bytes((k + b) & 255 for k in range(64))
        seed = bytes((255 - k + 3 * b) & 255 for k in range(64))
        r = o.encrypt_sym(v.astype(np.float32), share, seed, sk)
        for j in range(npr):
            h = pyoracle.fnv1a64(r["c0"][j].tobytes(), h)
            h = pyoracle.fnv1a64(r["c1"][j].tobytes(), h)
    assert kv["all"] == "%016x" % h


@pytest.mark.parametrize("mode", ["sym", "sym_seeded", "asym", "encode"])
def test_group_entries_match_single_device(env, mode):
    """The three multi-device entries through ctypes (se_amd_group over the same GPU listed three times):
    resident outputs, gathered outputs with an in-place root block, the seed-compressed symmetric form
    (c1 == NULL: only c0 travels) -- all bit-identical to one single-context call on the whole batch."""
    torch = env["torch"]
    from oracle.pyoracle import Oracle
    n, npr, B = 4096, 3, 301
    dev = env["dev"]
    sk = V.secret_key(n, seed=21)
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    ctx.set_secret_key(sk)
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    ctx.set_public_key(pk0, pk1)
    vals = V.bench_values(B, n, first=31)
    ss, sd = V.bench_seeds(B, first=31)
    tv, tss, tsd = dev_t(env, vals), dev_t(env, ss), dev_t(env, sd)
    e0 = torch.zeros((B, npr, n), dtype=torch.int32, device=dev)
    e1 = torch.zeros_like(e0)
    if mode in ("sym", "sym_seeded"):
        ctx.encrypt_sym(tv, tss, tsd, e0, e1)
    elif mode == "asym":
        ctx.encrypt_asym(tv, tsd, e0, e1)
    else:
        ctx.encode_ntt(tv, e0)
    torch.cuda.synchronize()

    g = env["pkg"].Group(n, npr, devices=[0, 0, 0])
    assert g.size == 3 and g.devices == [0, 0, 0]
    g.set_secret_key(sk)
    g.set_public_key(pk0, pk1)
    g.reserve(B)
    first, count = g.partition(B)
    assert sum(count) == B and first == [0, count[0], count[0] + count[1]] and max(count) - min(count) <= 1
    blk = lambda t: [t[f:f + c].contiguous() for f, c in zip(first, count)]
    bv, bss, bsd = blk(tv), blk(tss), blk(tsd)
    c0_all = torch.full((B, npr, n), -1, dtype=torch.int32, device=dev)
    c1_all = torch.full((B, npr, n), -1, dtype=torch.int32, device=dev)
    root = 1
    # member `root` writes in place inside the slab, the others into blocks of their own
    c0 = [c0_all[f:f + c] if i == root else torch.zeros((c, npr, n), dtype=torch.int32, device=dev)
          for i, (f, c) in enumerate(zip(first, count))]
    c1 = [c1_all[f:f + c] if i == root else torch.zeros((c, npr, n), dtype=torch.int32, device=dev)
          for i, (f, c) in enumerate(zip(first, count))]
    st = [torch.zeros(c, dtype=torch.uint8, device=dev) for c in count]
    if mode == "sym":
        g.encrypt_sym(B, bv, bss, bsd, c0, c1, st, gather_root=root, c0_all=c0_all, c1_all=c1_all)
    elif mode == "sym_seeded":
        g.encrypt_sym(B, bv, bss, bsd, c0, None, st, gather_root=root, c0_all=c0_all)
    elif mode == "asym":
        g.encrypt_asym(B, bv, bsd, c0, c1, st, gather_root=root, c0_all=c0_all, c1_all=c1_all)
    else:
        g.encode_ntt(B, bv, c0, st, gather_root=root, out_all=c0_all)
    torch.cuda.synchronize()
    assert all(bool(s.all()) for s in st)
    assert torch.equal(c0_all, e0)
    if mode in ("sym", "asym"):
        assert torch.equal(c1_all, e1)
    elif mode == "sym_seeded":
        assert bool((c1_all == -1).all())                     # untouched: only c0 travels
        ctx.expand_c1(tss, c1_all)
        torch.cuda.synchronize()
        assert torch.equal(c1_all, e1)
    for i, (f, c) in enumerate(zip(first, count)):            # the resident blocks themselves
        assert torch.equal(c0[i], e0[f:f + c])
    # resident form (no gather), B smaller than the group: members with empty blocks
    small = 2
    f2, n2 = g.partition(small)
    assert n2 == [1, 1, 0]
    o0 = [torch.zeros((max(c, 1), npr, n), dtype=torch.int32, device=dev) for c in n2]
    o1 = [torch.zeros((max(c, 1), npr, n), dtype=torch.int32, device=dev) for c in n2]
    bb = lambda t: [t[f:f + c].contiguous() if c else None for f, c in zip(f2, n2)]
    if mode in ("sym", "sym_seeded"):
        g.encrypt_sym(small, bb(tv), bb(tss), bb(tsd), o0, o1)
    elif mode == "asym":
        g.encrypt_asym(small, bb(tv), bb(tsd), o0, o1)
    else:
        g.encode_ntt(small, bb(tv), o0)
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(o0[i][0], e0[i])
    # argument errors are reported, not crashed on
    with pytest.raises(env["pkg"].SealEmbeddedAmdError):
        g.encode_ntt(B, bv, c0, st, gather_root=7, out_all=c0_all)
    g.close()
    ctx.close()


# --------------------------------------------------------------------------- device word arithmetic
@pytest.mark.parametrize("shape,prime", [((1024, 1), 0), ((4096, 3), 0), ((4096, 3), 2), ((16384, 6), 5)])
def test_device_word_arithmetic_kats(env, golden, shape, prime):
    """The reference's own Barrett / mul_mod / add / neg edge vectors (device/test/modulo_tests.c:78-179,
    uintmodarith_tests.c:96-192, tests/golden/ref_kats.json) pushed through the DEVICE inlines of
    kernels/modarith.cuh (se_amd_word_ops_device), plus MAX_ZZ-class and full-range 64-bit operands
    against exact integer arithmetic, and both butterflies against their definitions."""
    n, npr = shape
    ctx = env["pkg"].Context(n, npr)
    q = ctx.moduli()[prime]
    k = golden["kats"]
    MAX = 0xFFFFFFFF
    u64 = lambda xs: np.array(xs, dtype=np.uint64)

    rows = [r for r in k["barrett32"] if r[0] == q]
    if rows:
        assert list(ctx.word_ops(prime, 0, u64([r[1] for r in rows]))) == [r[2] for r in rows]
    rows = [r for r in k["barrett64"] if r[0] == q]
    if rows:
        assert list(ctx.word_ops(prime, 1, u64([(r[1] << 32) | r[2] for r in rows]))) == [r[3] for r in rows]
    rows = [r for r in k["mul_mod"] if r[0] == q]
    if rows:
        a, b, e = u64([r[1] for r in rows]), u64([r[2] for r in rows]), [r[3] for r in rows]
        assert list(ctx.word_ops(prime, 2, a, b)) == e
    # generic cases of uintmodarith_tests.c:96-140, parametrised on q
    add = [(0, 0, 0), (0, 1, 1), (0, q, 0), (1, q, 1), (1, q - 1, 0), (q, q - 2, q - 2), (q - 1, q - 1, q - 2),
           (0, 2 * q - 2, q - 2), (q - 10, q, q - 10), (q + 10, q - 12, q - 2)]
    assert list(ctx.word_ops(prime, 4, u64([r[0] for r in add]), u64([r[1] for r in add]))) == [r[2] for r in add]
    neg = [(0, 0), (1, q - 1), (q - 1, 1), (q, 0), (10, q - 10), (q - 10, 10)]
    assert list(ctx.word_ops(prime, 5, u64([r[0] for r in neg]))) == [r[1] for r in neg]
    mul = [(0, 0, 0), (1, 1, 1), (1, q, 0), (q + 1, 1, 1), (q - 1, 1, q - 1), (0, 12345, 0), (1, MAX, MAX % q),
           (1, 12345, 12345 % q), (MAX, MAX, MAX * MAX % q), (q - 1, q - 1, 1)]
    assert list(ctx.word_ops(prime, 2, u64([r[0] for r in mul]), u64([r[1] for r in mul]))) == [r[2] for r in mul]

    rng = np.random.default_rng(q)
    # 32-bit Barrett over the whole input range incl. the rejection bound neighbourhood
    x32 = np.concatenate([rng.integers(0, 2 ** 32, 4096, dtype=np.uint64),
                          u64([0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, 3 * q, 4 * q - 1, MAX - 1, MAX,
                               MAX - MAX % q - 1, MAX - MAX % q - 2])])
    x32 = x32[x32 <= MAX]
    assert (ctx.word_ops(prime, 0, x32) == (x32 % np.uint64(q)).astype(np.uint32)).all()
    # 64-bit Barrett: full-range operands (the "remainder estimate is in [0, 2q)" claim of modarith.cuh)
    edge = [0, 1, q, q * q, q * q - 1, (q - 1) * (q - 1), 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1,
            2 ** 64 - q, (2 ** 64 // q) * q, (2 ** 64 // q) * q - 1, MAX * MAX, MAX << 32, (MAX << 32) | MAX]
    x64 = np.concatenate([rng.integers(0, 2 ** 64, 8192, dtype=np.uint64), u64(edge)])
    exp = np.array([int(v) % q for v in x64], dtype=np.uint32)
    assert (ctx.word_ops(prime, 1, x64) == exp).all()
    # Shoup product: a may be ANY 32-bit word (lazy NTT values < 4q, raw PRNG words), b < q
    a = np.concatenate([rng.integers(0, 2 ** 32, 4096, dtype=np.uint64), u64([0, 1, q - 1, q, 2 * q, 4 * q - 1, MAX])])
    b = np.concatenate([rng.integers(0, q, 4096, dtype=np.uint64), u64([0, 1, q - 1, q - 1, q - 1, q - 1, q - 1])])
    exp = np.array([int(x) * int(y) % q for x, y in zip(a, b)], dtype=np.uint32)
    assert (ctx.word_ops(prime, 3, a, b) == exp).all()
    a, b = rng.integers(0, q + 1, 4096, dtype=np.uint64), rng.integers(0, q + 1, 4096, dtype=np.uint64)
    assert (ctx.word_ops(prime, 6, a, b) == ((a + np.uint64(2 * q) - b) % np.uint64(q)).astype(np.uint32)).all()
    # signed reduction incl. the reference's non-canonical q for negative multiples (ckks_common.c:234)
    m = np.concatenate([rng.integers(-2 ** 63, 2 ** 63, 4096, dtype=np.int64),
                        np.array([0, -1, 1, -q, q, -2 * q, -(2 ** 63) + 1, 2 ** 63 - 1, -q * q, -(2 ** 31), 2 ** 31],
                                 dtype=np.int64)])
    exp = []
    for v in m:
        r = abs(int(v)) % q
        exp.append(q - r if v < 0 else r)
    assert list(ctx.word_ops(prime, 7, m.view(np.uint64))) == exp
    x = rng.integers(0, 4 * q, 4096, dtype=np.uint64)
    assert (ctx.word_ops(prime, 8, x) == (x % np.uint64(q)).astype(np.uint32)).all()
    # butterflies on lazy operands (< 4q) against their definitions
    X, Y = rng.integers(0, 4 * q, 4096, dtype=np.uint64), rng.integers(0, 4 * q, 4096, dtype=np.uint64)
    W = rng.integers(1, q, 4096, dtype=np.uint64)
    t = np.array([int(y) * int(w) % q for y, w in zip(Y, W)], dtype=np.uint64)
    assert (ctx.word_ops(prime, 9, X, Y, W) == ((X + t) % np.uint64(q)).astype(np.uint32)).all()
    assert (ctx.word_ops(prime, 10, X, Y, W) == ((X + np.uint64(4 * q) - t) % np.uint64(q)).astype(np.uint32)).all()
    X, Y = rng.integers(0, 2 * q, 4096, dtype=np.uint64), rng.integers(0, 2 * q, 4096, dtype=np.uint64)
    assert (ctx.word_ops(prime, 11, X, Y, W) == ((X + Y) % np.uint64(q)).astype(np.uint32)).all()
    d = np.array([(int(x) - int(y)) * int(w) % q for x, y, w in zip(X, Y, W)], dtype=np.uint32)
    assert (ctx.word_ops(prime, 12, X, Y, W) == d).all()
    ctx.close()


# --------------------------------------------------------------------------- randomised slice
def test_bounded_fuzz_slice():
    """A bounded (~10 s) slice of the randomised parity soak (tools/fuzz_parity.py): random parameter
    sets, batch sizes around the wave boundaries, value distributions, pipeline shapes, reject-list
    capacities, device / host entries with forced chunk sizes, sym and asym, and the stage operators,
    every checked ciphertext bit for bit against the oracle.  Fixed master seed: the same cases on
    every run (the long soak with fresh seeds stays a tool)."""
    import subprocess
    import sys
    env = dict(os.environ, FUZZ_SECONDS=os.environ.get("SE_TEST_FUZZ_SECONDS", "10"), FUZZ_SEED="20260929")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("fuzz ok:"), last
    assert int(last.split()[2]) >= 10, last          # cases actually run


# --------------------------------------------------------------------------- batched key generation
@pytest.mark.parametrize("shape", [(1024, 1), (4096, 3), (16384, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gen_keys_batch(env, golden, shape):
    """se_amd_gen_keys_batch: K secret keys from the ternary sampler (the sample branch of ckks_setup_s,
    ckks_sym.c:162-179) and their public keys (gen_pk per prime) in one launch chain.  Key 0 is given
    (sk_in) and pinned to the golden digest of the REFERENCE's gen_pk for the same seeds; sampled keys
    and their public keys equal the oracle's for every k."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    ctx = env["pkg"].Context(n, npr)
    o = Oracle(n, npr)
    g = golden["digests"]["shapes"][f"{n}x{npr}"]["asym_survey"]
    sk0 = V.secret_key(n)
    _, pk0, pk1 = ctx.gen_keys_batch(np.frombuffer(SEED_PK, np.uint8), np.frombuffer(SEED_EP, np.uint8), sk_in=sk0)
    assert V.sha256_hex(pk0[0]) == g["pk0_sha256"] and V.sha256_hex(pk1[0]) == g["pk1_sha256"]
    K = 67                                             # crosses a wave of the lane-per-key samplers
    sks, pks, eps = V.derive_seeds(f"kg-sk-{n}", K), V.derive_seeds(f"kg-pk-{n}", K), V.derive_seeds(f"kg-ep-{n}", K)
    sk, pk0, pk1 = ctx.gen_keys_batch(pks, eps, sk_seeds=sks)
    for k in range(K):
        es, _ = o.sample_ternary_small(sks[k].tobytes(), 0)
        assert (sk[k] == es).all(), k
        e0, e1 = o.gen_pk(es, pks[k].tobytes(), eps[k].tobytes())
        assert (pk0[k] == e0).all() and (pk1[k] == e1).all(), k
    # a generated pair works: encrypt under pk, decrypt under sk (exact pseudo-decrypt criterion is
    # symmetric-only; here decode within the reference's 0.1 tolerance, ckks_tests_common.c:132)
    torch = env["torch"]
    ctx.set_secret_key(sk[3])
    ctx.set_public_key(pk0[3], pk1[3])
    vals = V.pattern_values(4, n)[None, :]
    c0 = torch.zeros((1, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    ctx.encrypt_asym(dev_t(env, vals), dev_t(env, V.derive_seeds("kg-enc", 1)), c0, c1)
    dvals = torch.zeros((1, n // 2), dtype=torch.float32, device=env["dev"])
    ctx.decrypt_decode(c0, c1, 0, None, None, dvals)
    torch.cuda.synchronize()
    assert float((dvals.cpu() - torch.from_numpy(vals)).abs().max()) < 0.1
    ctx.close()


# --------------------------------------------------------------------------- one context, many callers
def test_calls_from_two_streams_and_two_threads_are_ordered(env):
    """A context has ONE set of scratch (error polynomial, counters, reject lists, auxiliary streams).
    Calls issued back to back on DIFFERENT streams, and from different host threads, must still each
    produce their own ciphertexts: the library orders successive calls on the scratch (event chain +
    mutex, se_context.cpp begin_call / end_call).  Without that ordering the second call overwrites the
    error polynomial the first one's fused kernel has yet to read."""
    import threading
    from oracle.pyoracle import Oracle
    torch = env["torch"]
    n, npr, B = 4096, 3, 3000
    ctx = env["pkg"].Context(n, npr)
    sk = V.secret_key(n)
    ctx.set_secret_key(sk)
    o = Oracle(n, npr)
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    ctx.set_public_key(pk0, pk1)
    jobs = []
    for k in range(4):
        vals = V.bench_values(B, n, first=10000 * k)
        ss, sd = V.bench_seeds(B, first=10000 * k)
        jobs.append(dict(vals=vals, ss=ss, sd=sd, dv=dev_t(env, vals), dss=dev_t(env, ss), dsd=dev_t(env, sd),
                         c0=torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"]),
                         c1=torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"]),
                         stream=torch.cuda.Stream(), asym=(k == 3)))
    torch.cuda.synchronize()

    def issue(j):
        with torch.cuda.stream(j["stream"]):
            if j["asym"]:
                ctx.encrypt_asym(j["dv"], j["dsd"], j["c0"], j["c1"])
            else:
                ctx.encrypt_sym(j["dv"], j["dss"], j["dsd"], j["c0"], j["c1"])

    issue(jobs[0])                      # two streams, one thread, no synchronisation in between
    issue(jobs[1])
    th = [threading.Thread(target=issue, args=(jobs[k],)) for k in (2, 3)]   # two more from other threads
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        for b in (0, 1, 63, 64, B // 2, B - 1):
            r = (o.encrypt_asym(j["vals"][b], j["sd"][b].tobytes(), pk0, pk1) if j["asym"] else
                 o.encrypt_sym(j["vals"][b], j["ss"][b].tobytes(), j["sd"][b].tobytes(), sk))
            assert (host_u32(j["c0"][b]) == r["c0"]).all() and (host_u32(j["c1"][b]) == r["c1"]).all(), (k, b)
    ctx.close()


def test_asym_chunked_pipeline_is_bit_identical(env):
    """The public-key path cut into chunks (CBD sampler of chunk k+1 beside the fused kernel of chunk
    k on the auxiliary stream) gives the same bytes as the serial launch chain, for even and ragged
    chunk boundaries."""
    torch = env["torch"]
    n, npr, B = 4096, 3, 3 * 4096 + 77
    ctx = env["pkg"].Context(n, npr)
    from oracle.pyoracle import Oracle
    o = Oracle(n, npr)
    sk = V.secret_key(n)
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    ctx.set_public_key(pk0, pk1)
    vals, (_, sd) = V.bench_values(B, n), V.bench_seeds(B)
    dv, dsd = dev_t(env, vals), dev_t(env, sd)
    outs = []
    for chunks in (1, 2, 3):
        ctx.set_asym_chunks(chunks)
        c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
        c1 = torch.zeros_like(c0)
        ctx.encrypt_asym(dv, dsd, c0, c1)
        torch.cuda.synchronize()
        outs.append((c0, c1))
    for c0, c1 in outs[1:]:
        assert bool((c0 == outs[0][0]).all()) and bool((c1 == outs[0][1]).all())
    for b in (0, 4095, 4096, B - 1):
        r = o.encrypt_asym(vals[b], sd[b].tobytes(), pk0, pk1)
        assert (host_u32(outs[0][0][b]) == r["c0"]).all() and (host_u32(outs[0][1][b]) == r["c1"]).all()
    ctx.close()



_WATCHDOG_CHILD = r'''
import os, sys, threading, time
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import __graft_entry__ as ge
pkg = ge.load_package()
import vectors as V
dev = torch.device("cuda:0")
state = {"what": "start", "t0": time.time()}
def watchdog():
    while True:
        time.sleep(0.25)
        if state["what"] is not None and time.time() - state["t0"] > float(sys.argv[2]):
            print("WATCHDOG: no progress in", state["what"], flush=True)
            os._exit(3)
threading.Thread(target=watchdog, daemon=True).start()
def step(what):
    torch.cuda.synchronize()
    state["what"], state["t0"] = what, time.time()
def dt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
rng = np.random.default_rng(5)
# warm-up outside the watchdog window: library load, first context, kernel code upload
state["what"] = None
ctx = pkg.Context(1024, 1); ctx.close()
for n, npr in ((1024, 1), (4096, 3)):
    ctx = pkg.Context(n, npr)
    sk = V.secret_key(n, seed=3)
    ctx.set_secret_key(sk)
    pk0, pk1 = ctx.gen_public_key(sk, bytes(range(64)), bytes(range(64, 128)))
    ctx.set_public_key(pk0, pk1)
    for B in (1, 2, 3, 7, 9, 65, 129):
        seeds = dt(rng.integers(0, 256, (B, 64), dtype=np.uint8))
        # k_sample_cbd: B * blocks not a multiple of 512; blocks_per_ct = 1 leaves ONE live lane in the only workgroup
        for blocks in (1, 3, n // 16, 2 * (n // 16) + 1):
            step("cbd n=%d B=%d blocks=%d" % (n, B, blocks))
            out = torch.zeros((B, blocks * 16), dtype=torch.int8, device=dev)
            ctx.sample_cbd(seeds, out, blocks)
        # k_sample_ternary_window (+ redo): one ciphertext = a fraction of a workgroup
        step("ternary n=%d B=%d" % (n, B))
        codes = torch.zeros((B, n), dtype=torch.int8, device=dev)
        ctx.sample_ternary(seeds, codes)
        vals = dt(V.bench_values(B, n, first=11))
        ss, sd = V.bench_seeds(B, first=11)
        c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=dev); c1 = torch.zeros_like(c0)
        # k_candidates through the staged dispatch (pair form: per-prime rows), tiny capacities so that
        # B * spec_cap is nowhere near a multiple of 512 and k_resolve_wave walks a flagged list
        for flags, split in ((512, 1),):
            for cap in (None, 1, 7):
                step("staged flags=%d n=%d B=%d cap=%s" % (flags, n, B, cap))
                c2 = pkg.Context(n, npr); c2.set_secret_key(sk); c2.set_pipeline(1, split); c2.set_debug_flags(flags)
                if cap is not None:
                    c2.set_speculation_capacity(cap)
                c2.encrypt_sym(vals, dt(ss), dt(sd), c0, c1)
                torch.cuda.synchronize(); c2.close()
        # the redo launches of the prime speculation (UniformArgs::only_from): windows of one guess force misses
        step("spec redo n=%d B=%d" % (n, B))
        c3 = pkg.Context(n, npr); c3.set_secret_key(sk); c3.set_debug_flags(256)
        c3.encrypt_sym(vals, dt(ss), dt(sd), c0, c1); torch.cuda.synchronize(); c3.close()
        step("asym n=%d B=%d" % (n, B))
        ctx.encrypt_asym(vals, dt(sd), c0, c1)
    step("close")
    ctx.close()
state["what"] = None
print("WATCHDOG-OK", flush=True)
'''


def test_synchronised_kernels_do_not_hang_on_ragged_shapes(env, tmp_path):
    """The phase-synchronised kernels (k_sample_cbd, k_candidates, k_sample_ternary_window: 96 workgroup barriers
    per permutation) on the shapes where a barrier contract could break -- a last workgroup with ONE live lane, whole
    waves past the end, B * blocks not a multiple of the workgroup size, candidate rows of 1 and 7, the masked redo
    launches of the prime speculation -- run in a CHILD process under a watchdog: a launch that makes no progress for
    5 s ends the child (exit code 3) instead of hanging the suite (a hang on the driver's box would cost the whole GPU
    record).  Results are checked by the other tests; this one checks that every launch RETURNS."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "watchdog_child.py"
    script.write_text(_WATCHDOG_CHILD)
    try:
        r = subprocess.run([sys.executable, str(script), root, "5"], capture_output=True, text=True, timeout=600,
                           cwd=root)
    except subprocess.TimeoutExpired as e:   # the child's own watchdog should have fired long before
        pytest.fail("watchdog child did not end: " + str(e.stdout)[-500:])
    assert r.returncode == 0 and "WATCHDOG-OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
