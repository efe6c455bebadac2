"""Pins the CPU oracle (oracle/se_oracle.c) before anything trusts it:
  * the reference's own known-answer values (tests/golden/ref_kats.json),
  * golden vectors produced by the compiled reference (tests/golden/golden_*.{npz,json}),
  * hashlib's SHAKE256 for the PRNG layer,
  * and, when oracle/_ref/libse_ref.so is present, the compiled reference itself on fresh
    random inputs.
CPU only; runs in the build container and on the GPU box alike.
"""
import hashlib
import os
import struct

import numpy as np
import pytest

import vectors as V
from gpu_support import SEED_A, SEED_B, SEED_EP, SEED_PK
from oracle import pyoracle
from oracle.pyoracle import Oracle



def ends(a, k=8):
    a = np.asarray(a).ravel()
    return [int(x) for x in a[:k]] + [int(x) for x in a[-k:]]


@pytest.fixture(scope="module", autouse=True)
def _built():
    pyoracle.build(ref=True)


# ---------------------------------------------------------------- reference's own KATs
def test_barrett_kats(golden):
    k = golden["kats"]
    O = {134012929: (Oracle(1024, 1), 0), 1053818881: (Oracle(4096, 3), 0)}
    for q, x, exp in k["barrett32"]:
        o, j = O[q]
        assert o.barrett32(x, j) == exp == x % q
    for q, hi, lo, exp in k["barrett64"]:
        o, j = O[q]
        x = (hi << 32) | lo
        assert o.barrett64(x, j) == exp == x % q
    for q, a, b, exp in k["mul_mod"]:
        o, j = O[q]
        assert o.mul_mod(a, b, j) == exp


def test_modarith_generic_cases():
    # uintmodarith_tests.c:96-140 (parametrised on q)
    for o in (Oracle(1024, 1), Oracle(4096, 3)):
        q = o.q[0]
        MAX = 0xFFFFFFFF
        for a, b, e in [(0, 0, 0), (0, 1, 1), (0, q, 0), (1, q, 1), (1, q - 1, 0), (q, q - 2, q - 2),
                        (q - 1, q - 1, q - 2), (0, 2 * q - 2, q - 2), (q - 10, q, q - 10),
                        (q + 10, q - 12, q - 2)]:
            assert o.add_mod(a, b) == e
        for a, e in [(0, 0), (1, q - 1), (q - 1, 1), (q, 0), (10, q - 10), (q - 10, 10)]:
            assert o.neg_mod(a) == e
        for a, b, e in [(0, 0, 0), (1, 1, 1), (1, q, 0), (q + 1, 1, 1), (q - 1, 1, q - 1),
                        (0, 12345, 0), (1, MAX, MAX % q), (1, 12345, 12345 % q)]:
            assert o.mul_mod(a, b) == e


def test_const_ratio_and_roots_tables():
    for n, npr in V.ALL_SHAPES:
        o = Oracle(n, npr)
        for j in range(npr):
            q = o.q[j]
            ratio = (1 << 64) // q
            assert (int(o.p.cr_hi[j]) << 32 | int(o.p.cr_lo[j])) == ratio
            psi = int(o.p.psi[j])
            assert pow(psi, n, q) == q - 1          # primitive 2n-th root of unity
            assert (q - 1) % (2 * n) == 0


# ---------------------------------------------------------------- PRNG layer
def test_shake_matches_hashlib():
    rng = np.random.default_rng(5)
    for inlen in (0, 1, 71, 72, 135, 136, 137, 300):
        msg = rng.integers(0, 256, inlen, dtype=np.uint8).tobytes()
        for outlen in (1, 4, 96, 135, 136, 137, 1000):
            assert Oracle.shake256(msg, outlen) == hashlib.shake_256(msg).digest(outlen)


def test_prng_block_golden(golden):
    for e in golden["digests"]["prng"]:
        out = Oracle.prng_block(SEED_A, e["ctr"], e["len"])
        assert hashlib.sha256(out).hexdigest() == e["sha256"]
        assert out[:16].hex() == e["head"][:2 * min(16, e["len"])]
        assert out == hashlib.shake_256(SEED_A + struct.pack("<Q", e["ctr"])).digest(e["len"])


def test_keccak_zero_state_kat():
    # Keccak-f[1600] on the all-zero state (well-known first lane of the KAT)
    st = Oracle.keccak_f1600(np.zeros(25, dtype=np.uint64))
    assert int(st[0]) == 0xF1258F7940E1DDE7
    assert int(st[24]) == 0xEAF1FF7B5CECA249


# ---------------------------------------------------------------- golden vectors (all shapes)
@pytest.mark.parametrize("shape", V.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_vs_golden(golden, shape):
    n, npr = shape
    d = golden["digests"]["shapes"][f"{n}x{npr}"]
    o = Oracle(n, npr)
    assert o.q == d["q"] and o.scale == d["scale"]
    assert V.sha256_hex(o.map) == d["index_map_sha256"]

    for t in range(9):
        ok, m = o.encode(V.pattern_values(t, n))
        assert ok and V.sha256_hex(m) == d["encode"][f"pattern{t}"]["sha256"]
    ok, m = o.encode(V.bench_values(1, n)[0])
    assert ok and V.sha256_hex(m) == d["encode"]["bench0"]["sha256"]
    ok, _ = o.encode(np.full(n // 2, 3.0e38, dtype=np.float32))
    assert ok == d["encode"]["overflow_3e38_ok"] and not ok

    # non-finite / edge-magnitude values (NaN -> INT64_MIN, Inf -> return false at a definite index)
    sk = V.secret_key(n)
    kinds = set()
    for c, g in enumerate(d["encode"]["nonfinite"]):
        vals = V.nonfinite_values(c, n)
        idx, m = o.encode_ex(vals)
        assert idx == g["fail_index"] and V.sha256_hex(m[:idx]) == g["prefix_sha256"], c
        assert int((m[:idx] == -2 ** 63).sum()) == g["int64_min_count"]
        kinds.add((idx == n, g["int64_min_count"] > 0))
        if idx == n:
            r = o.encrypt_sym(vals, SEED_A, SEED_B, sk)
            assert r["ok"] and V.sha256_hex(r["c0"]) == g["c0_sha256"], c
            assert V.sha256_hex(r["pte"]) == g["pte_sha256"], c
    assert {(True, True), (True, False), (False, False)} <= kinds   # accepted NaN, ordinary, rejected
    assert any(0 < g["fail_index"] < n for g in d["encode"]["nonfinite"])   # rejected behind a prefix

    ctr = 0
    for j in range(npr):
        g = d["samplers"][f"uniform_p{j}"]
        a, ctr2 = o.sample_uniform(j, SEED_A, ctr)
        assert ctr == g["ctr_in"] and ctr2 == g["ctr_out"] and V.sha256_hex(a) == g["sha256"]
        ctr = ctr2
    u, c2 = o.sample_ternary_small(SEED_B, 0)
    assert c2 == d["samplers"]["ternary"]["ctr_out"]
    assert V.sha256_hex(u) == d["samplers"]["ternary"]["sha256"]
    e, c3 = o.cbd_int8(SEED_B, c2)
    assert c3 == d["samplers"]["cbd_int8"]["ctr_out"]
    assert V.sha256_hex(e) == d["samplers"]["cbd_int8"]["sha256"]

    rng = np.random.default_rng(d["ntt_random_seed"])
    for j in range(npr):
        q = o.q[j]
        delta = np.zeros(n, dtype=np.uint32)
        delta[1] = 1
        ins = {"delta1": delta, "ones": np.ones(n, dtype=np.uint32),
               "ramp": (np.arange(n, dtype=np.uint64) % q).astype(np.uint32),
               "qm1": np.full(n, q - 1, dtype=np.uint32),
               "random": rng.integers(0, q, n, dtype=np.uint64).astype(np.uint32)}
        for name, x in ins.items():
            assert V.sha256_hex(o.ntt(x, j)) == d["ntt"][f"{name}_p{j}"]["sha256"], (name, j)
        assert V.sha256_hex(o.ntt_roots(j)) == d["ntt"][f"roots_p{j}"]["sha256"]

    x = np.zeros(n, dtype=np.int64)
    x[:6] = [0, -o.q[0], o.q[0], -1, 1, -(2 ** 62)]
    assert [int(v) for v in o.reduce_pte(x, 0)[:6]] == d["reduce_edge"]
    assert d["reduce_edge"][1] == o.q[0]          # the non-canonical q (ckks_common.c:234)

    sk = V.secret_key(n)
    for tag, vals, s1, s2 in [("survey", V.survey_values(n), V.SURVEY_SHARE_SEED, V.SURVEY_SEED),
                              ("bench0", V.bench_values(1, n)[0], SEED_A, SEED_B)]:
        g = d[f"sym_{tag}"]
        r = o.encrypt_sym(vals, s1, s2, sk)
        assert r["ok"] and r["end_ctr"] == g["end_ctr"]
        assert V.sha256_hex(r["c0"]) == g["c0_sha256"]
        assert V.sha256_hex(r["c1"]) == g["c1_sha256"]
        assert V.sha256_hex(r["pte"]) == g["pte_sha256"]
        assert V.sha256_hex(r["ntt_pte"]) == g["c1_alias_sha256"]   # the alias quirk, SURVEY 0.5
        assert [ends(r["c0"][j]) for j in range(npr)] == g["c0_ends"]

    # verification side (intt / decrypt / decode) against the reference's own helpers
    vv = V.pattern_values(4, n)
    r = o.encrypt_sym(vv, SEED_A, SEED_B, sk)
    for j in range(npr):
        gv = d["verify_pattern4"][f"p{j}"]
        s_hat = o.ntt(o.expand_ternary(sk, j), j)
        dec = o.decrypt(r["c0"][j], r["c1"][j], s_hat, j)
        assert (dec == r["ntt_pte"][j]).all()
        ptj = o.intt(dec, j)
        assert V.sha256_hex(ptj) == gv["pt_sha256"]
        val = o.decode(ptj, j)
        assert V.sha256_hex(val) == gv["values_sha256"]
        assert np.abs(val - vv).max() < 0.1

    g = d["asym_survey"]
    pk0, pk1 = o.gen_pk(sk, SEED_PK, SEED_EP)
    assert V.sha256_hex(pk0) == g["pk0_sha256"] and V.sha256_hex(pk1) == g["pk1_sha256"]
    r = o.encrypt_asym(V.survey_values(n), V.SURVEY_SEED, pk0, pk1)
    assert r["ok"] and r["end_ctr"] == g["end_ctr"]
    for key in ("c0", "c1", "pte", "u", "e1"):
        assert V.sha256_hex(r[key]) == g[f"{key}_sha256"], key

    # API-level callback stream (per prime: c0 then the aliased c1 buffer in sym mode)
    r = o.encrypt_sym(V.survey_values(n), V.SURVEY_SHARE_SEED, V.SURVEY_SEED, sk)
    stream = b"".join(r["c0"][j].tobytes() + r["ntt_pte"][j].tobytes() for j in range(npr))
    assert "%016x" % pyoracle.fnv1a64(stream) == d["api_fnv1a64_sym"]
    r = o.encrypt_asym(V.survey_values(n), V.SURVEY_SEED, pk0, pk1)
    stream = b"".join(r["c0"][j].tobytes() + r["c1"][j].tobytes() for j in range(npr))
    assert "%016x" % pyoracle.fnv1a64(stream) == d["api_fnv1a64_asym"]


def test_full_vectors_c1(golden):
    g = golden["c1"]
    o = Oracle(1024, 1)
    sk = V.secret_key(1024)
    for t in range(9):
        assert (o.encode(V.pattern_values(t, 1024))[1] == g[f"encode_pattern{t}"]).all()
    assert (o.sample_uniform(0, SEED_A, 0)[0] == g["uniform_p0"]).all()
    assert (o.sample_ternary_small(SEED_B, 0)[0] == g["ternary"]).all()
    assert (o.ntt(g["ntt_random_in"], 0) == g["ntt_random_out"]).all()
    r = o.encrypt_sym(V.survey_values(1024), V.SURVEY_SHARE_SEED, V.SURVEY_SEED, sk)
    assert (r["c0"] == g["sym_c0"]).all() and (r["c1"] == g["sym_c1"]).all()
    assert (r["pte"] == g["sym_pte"]).all() and (r["ntt_pte"] == g["sym_c1_alias"]).all()
    # the value quoted in SURVEY.md section 0.8
    assert [int(x) for x in r["c0"][0, :4]] == [2684880, 75498332, 27037551, 131419181]
    ra = o.encrypt_asym(V.survey_values(1024), V.SURVEY_SEED, g["pk0"], g["pk1"])
    assert (ra["c0"] == g["asym_c0"]).all() and (ra["c1"] == g["asym_c1"]).all()


def test_twiddle_digest_matches_host_libm(golden):
    """SURVEY trap T8: encode goldens assume this host's libm cos/sin equal the generating
    host's.  If this fails on another box the encode goldens may differ in last-bit cases."""
    for n, dg in golden["digests"]["ifft_twiddle_sha256"].items():
        w = Oracle(int(n), 1).twiddles()
        assert hashlib.sha256(w.astype("<f8").tobytes()).hexdigest() == dg


# ---------------------------------------------------------------- properties
def test_pseudo_decrypt_identity():
    """c0 + c1 . NTT(s) == NTT(m + e) exactly (device/test/ckks_tests_common.c:206)."""
    for n, npr in [(1024, 1), (4096, 3)]:
        o = Oracle(n, npr)
        sk = V.secret_key(n, seed=3)
        r = o.encrypt_sym(V.bench_values(1, n)[0], SEED_A, SEED_B, sk)
        for j in range(npr):
            q = o.q[j]
            s_hat = o.ntt(o.expand_ternary(sk, j), j).astype(np.uint64)
            lhs = (r["c0"][j].astype(np.uint64) + r["c1"][j].astype(np.uint64) * s_hat % q) % q
            assert (lhs == r["ntt_pte"][j]).all()


def test_ntt_is_negacyclic_convolution():
    """ntt(a) . ntt(b) == ntt(a*b mod (x^n+1)) against schoolbook (device/test/ntt_tests.c)."""
    o = Oracle(1024, 1)
    q, n = o.q[0], 1024
    rng = np.random.default_rng(9)
    a = rng.integers(0, q, n, dtype=np.uint64)
    b = np.zeros(n, dtype=np.uint64)
    b[[0, 3, 700]] = [5, q - 2, 7]
    prod = np.zeros(n, dtype=object)
    for i in (0, 3, 700):
        for k in range(n):
            t = int(a[k]) * int(b[i])
            idx = k + i
            if idx >= n:
                prod[idx - n] -= t
            else:
                prod[idx] += t
    prod = np.array([int(x) % q for x in prod], dtype=np.uint32)
    lhs = (o.ntt(a.astype(np.uint32), 0).astype(np.uint64) *
           o.ntt(b.astype(np.uint32), 0).astype(np.uint64)) % q
    assert (lhs.astype(np.uint32) == o.ntt(prod, 0)).all()


def test_encode_decode_roundtrip_within_tolerance():
    """FFT(decode) of the encoded polynomial returns the inputs within 0.1
    (device/test/ckks_tests_common.c:132); done here with numpy's canonical embedding."""
    n = 1024
    o = Oracle(n, 1)
    vals = V.pattern_values(8, n)
    ok, m = o.encode(vals)
    assert ok
    # evaluate m(x) at zeta^(3^i), zeta = e^{i pi / n}
    pos = 1
    coeffs = m.astype(np.float64) / o.scale
    for i in range(0, n // 2, 37):
        p = pow(3, i, 2 * n)
        z = np.exp(1j * np.pi * p / n)
        val = np.polyval(coeffs[::-1], z)
        assert abs(val.real - float(vals[i])) < 0.1 and abs(val.imag) < 0.1


# ---------------------------------------------------------------- live reference cross-check
@pytest.mark.ref
@pytest.mark.skipif(not pyoracle.ref_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("shape", [(1024, 1), (4096, 3), (16384, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_vs_live_reference_random(shape):
    from oracle.pyoracle import Reference
    n, npr = shape
    o, R = Oracle(n, npr), Reference(n, npr)
    rng = np.random.default_rng(n)
    sk = V.secret_key(n, seed=11)
    R.set_sk(sk)
    for trial in range(3):
        vals = (rng.standard_normal(n // 2) * 10 ** trial).astype(np.float32)
        s1 = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
        s2 = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
        a, b = o.encrypt_sym(vals, s1, s2, sk), R.encrypt_sym(vals, s1, s2)
        for k in ("c0", "c1", "pte"):
            assert (a[k] == b[k]).all(), k
        assert a["end_ctr"] == b["end_ctr"]
    # short input (zero fill) and ragged lengths
    for vlen in (0, 1, 7, n // 2 - 1):
        vals = rng.standard_normal(vlen).astype(np.float32)
        a, b = o.encrypt_sym(vals, s1, s2, sk), R.encrypt_sym(vals, s1, s2)
        assert (a["c0"] == b["c0"]).all() and (a["c1"] == b["c1"]).all()
    # word-level cross-check on random operands
    for j in range(npr):
        for _ in range(200):
            x = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))
            assert o.barrett64(x, j) == R.barrett64(x, j) == x % o.q[j]
            w = int(rng.integers(0, 2 ** 32))
            assert o.barrett32(w, j) == R.barrett32(w, j) == w % o.q[j]
    R.close()


@pytest.mark.ref
@pytest.mark.skipif(not pyoracle.ref_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("shape", [(1024, 1), (4096, 3), (16384, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_nonfinite_matches_reference(shape):
    """NaN / Inf / FLT_MAX / subnormal / -0.0 plaintext values, fresh random placements: the index at which
    the compiled reference's ckks_encode_base returns false (n: it does not) and everything its in-place
    loop converted before that equal the restatement's -- including the Annex-G infinity recovery of the
    complex product (seo_cmul), without which about 1 case in 300 differs."""
    n, npr = shape
    o, r = Oracle(n, npr), pyoracle.Reference(n, npr)
    rng = np.random.default_rng(n + 77)
    specials = np.array([np.inf, -np.inf, np.nan, 3.4028235e38, -3.4028235e38, 1e-45, -0.0, 0.0, 1e-39],
                        dtype=np.float32)
    seen_fail = seen_nan = 0
    for trial in range(120 if n < 16384 else 30):
        v = (rng.random(n // 2, dtype=np.float32) * 50 - 25).astype(np.float32)
        pool = specials[rng.choice(len(specials), size=int(rng.integers(1, len(specials) + 1)), replace=False)]
        k = int(rng.integers(1, 6))
        v[rng.choice(n // 2, size=k, replace=False)] = rng.choice(pool, size=k)
        if trial % 7 == 0:
            v[:] = rng.choice(pool, size=n // 2)
        if trial % 7 == 1:
            v[rng.random(n // 2) < 0.5] = rng.choice(pool)
        ia, a = o.encode_ex(v)
        ib, b = r.encode_ex(v)
        assert ia == ib and np.array_equal(a[:ia], b[:ib]), (trial, ia, ib)
        seen_fail += ib < n
        seen_nan += ib == n and bool((b == -2 ** 63).any())
    assert seen_fail and seen_nan
    r.close()


def test_batched_driver_matches_single():
    n, npr, B = 1024, 1, 6
    o = Oracle(n, npr)
    vals = V.bench_values(B, n)
    ss, sd = V.bench_seeds(B)
    sk = V.secret_key(n)
    ok, c0, c1 = o.encrypt_sym_batch(vals, ss, sd, sk, nthreads=3)
    assert ok
    for b in range(B):
        r = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
        assert (c0[b] == r["c0"]).all() and (c1[b] == r["c1"]).all()


def test_oracle_is_sanitizer_clean():
    """`make -C oracle sanitize`: the C restatement under AddressSanitizer + UndefinedBehaviorSanitizer,
    every entry point (incl. the threaded batch drivers, extreme magnitudes, overflow, all five
    shapes up to 13 primes) driven by oracle/oracle_selftest.c -- SURVEY.md section 5."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-C", os.path.join(root, "oracle"), "sanitize"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "all shapes clean under ASan + UBSan" in r.stdout


def test_round_half_away_form():
    """The device encoder rounds with trunc(x + copysign(0.5 - 2^-54, x)) (encode_encrypt.hip, round_half_away: 3
    VALU operations instead of the library's 6-7).  It must equal C round() -- what ckks_common.c:183,192 calls --
    for EVERY double: checked here against libm's round() on the boundary cases (k + 0.5 and its neighbours over
    30 binades, pred(0.5), the 2^52 / 2^53 integers, zeros, extremes) and on 2 M random doubles of all magnitudes.
    (NaN / infinity never reach it: the fast kernels decline such plaintexts; both forms pass them through.)"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.round.restype = ctypes.c_double
    libm.round.argtypes = [ctypes.c_double]
    c = np.float64(0.49999999999999994)
    assert c == np.nextafter(np.float64(0.5), np.float64(0.0))
    form = lambda x: np.trunc(x + np.copysign(c, x))
    xs = [0.0, -0.0, 0.5, -0.5, float(c), -float(c), 1.5, 2.5, -2.5, 4503599627370495.5, 4503599627370496.0,
          4503599627370497.0, 9007199254740992.0, 9007199254740993.0, 1e300, -1e300, 5e-324, 2.2250738585072014e-308]
    for k in range(-40, 41):
        for e in range(0, 52, 3):
            base = float(k) * 2.0 ** e + 0.5
            for v in (base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf)):
                xs.append(float(v))
    rng = np.random.default_rng(7)
    mant = rng.random(2_000_000) * 2 - 1
    expo = rng.integers(-60, 64, 2_000_000)
    xs = np.concatenate([np.array(xs, dtype=np.float64), mant * np.exp2(expo.astype(np.float64)),
                         np.trunc(mant * 1e6) + 0.5, np.nextafter(np.trunc(mant * 1e9) + 0.5, 0.0)])
    want = np.array([libm.round(float(v)) for v in xs[:4000]], dtype=np.float64)
    assert (form(xs[:4000]) == want).all()
    # the rest vectorised: C round() == sign(x) * floor(|x| + 0.5) computed EXACTLY (split off the integer part first)
    ax = np.abs(xs)
    ip = np.floor(ax)
    ref = np.copysign(ip + (ax - ip >= 0.5), xs)          # ax - ip is exact for doubles
    got = form(xs)
    assert (got == ref).all() and (np.signbit(got) == np.signbit(ref)).all()


def test_half_size_ifft_model_and_guard_band():
    """Round 6: the fast fused kernels at n = 4096 encode through a HALF-SIZE transform (encode_encrypt.hip,
    encode_pair_half; transform.cuh, ifft_pair_real_half) and keep the reference's bits by a guard band.  This is the
    CPU model of that construction, against the oracle's IFFT (the reference's algorithm and libm root table):
      (a) the slot vector is real and reverse-symmetric in stored order, A[n-1-k] == A[k];
      (b) DIF stages 0..10 restricted to the lower half + the closed-form last stage (2 Re u, -2 Im u Im W[1]) give the
          oracle's real parts up to a few ulp -- far inside the kernel's guard band delta = 3e-14 ||m||_2 (the proved
          bound on that deviation; the kernel's constant is read from the source);
      (c) a plaintext whose rounded coefficients differ between the two algorithms (none is expected) must be flagged by
          the guard, and exact ties (constant slot vectors encoding to k + 0.5) ARE flagged."""
    import re
    n, logn = 4096, 12
    o = Oracle(n, 3)
    W = o.twiddles().view(np.complex128)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seal-embedded_amd", "csrc",
                            "kernels", "encode_encrypt.hip")).read()
    m = re.search(r"constexpr double kHalfDelta\s*=\s*([0-9.e-]+)\s*\*\s*([0-9.]+);", src)
    k_delta = float(m.group(1)) * float(m.group(2))
    assert 2.2e-14 < k_delta < 4e-14          # above the derived bound 1.5e-14 (x sqrt(2) in the source's looser form)
    n_inv = float(o.p.scale) / n if hasattr(o.p, "scale") else 2.0 ** 25 / n

    def annexg(a, w):
        return (a.real * w.real - a.imag * w.imag) + 1j * (a.real * w.imag + a.imag * w.real)

    def half(A):
        A = A[: n // 2].copy()
        k = np.arange(n // 2)
        for i in range(logn - 1):
            lo = k[(k >> i) & 1 == 0]
            hi = lo | (1 << i)
            u, v = A[lo], A[hi]
            A[lo] = u + v
            A[hi] = annexg(u - v, W[(n >> (i + 1)) + (lo >> (i + 1))])
        return np.concatenate([2 * A.real, -(2 * A.imag * W[1].imag)])

    rha = lambda x: np.sign(x) * np.floor(np.abs(x) + 0.5)
    imap = np.asarray(o.map, dtype=np.int64)
    rng = np.random.default_rng(20261001)
    cases = [V.bench_values(1, n, first=9000 + i)[0].astype(np.float64) for i in range(6)]
    cases.append(np.full(n // 2, np.float32(75.0 / 2.0 ** 26), dtype=np.float64))           # exact tie: m_0 = 37.5
    for slot, kk in ((0, 50), (17, 12345), (2047, 3)):
        v = np.zeros(n // 2)
        v[slot] = np.float32((2 * kk + 1) / 2.0 ** 15)                                       # ties decided by rounding noise
        cases.append(v)
    cases.append((rng.integers(-64, 65, n // 2) / 2.0 ** 15).astype(np.float32).astype(np.float64))
    worst = 0.0
    for ci, vals in enumerate(cases):
        A = np.zeros(n, dtype=np.complex128)
        A[imap[: n // 2]] = vals
        A[imap[n // 2:]] = vals
        assert np.array_equal(A[::-1], A)                                                    # (a)
        R = o.ifft(A).real * n_inv
        H = half(A) * n_inv
        delta = k_delta * n_inv * np.sqrt(2.0 * n * float((vals.astype(np.float32) ** 2).sum(dtype=np.float32)))
        norm = np.linalg.norm(R)
        dev = np.abs(R - H).max()
        worst = max(worst, dev / max(norm, 1e-300))
        assert dev <= 1e-2 * delta + 1e-300, (ci, dev, delta)                                # (b)
        a = np.abs(H)
        flagged = np.abs((a - np.trunc(a)) - 0.5) < delta
        differ = rha(R) != rha(H)
        assert not (differ & ~flagged).any(), ci                                              # (c)
        if ci == 6:
            assert flagged[0] and abs(H[0]) == 37.5
    assert worst < 1e-15          # measured 1.9e-17 ||m||_2
