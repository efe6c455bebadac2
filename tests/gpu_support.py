"""What the GPU test modules (tests/test_gpu_*.py) share.  Tests import helpers from here (`from gpu_support import
env, dev_t, ...`), never from another test module; a helper that a second module needs moves here.

- env: the module-scoped fixture (torch, the loaded package, cuda:0); gpu_env() is the same setup as a plain function.
- dev_t, host_u32, bits, stream_of, same_bytes: host <-> device and bit-pattern conveniences.
- SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY: the C ABI's error codes; SEED_A, SEED_B, SEED_PK, SEED_EP: the golden seeds.
- the receiving side: records, encrypt_sym, ntt_secret, crt_centred, decode_expect, expectation (oracle + Python
  ints), run_decrypt (decrypt_full / decrypt_level and their keyed twins over sentinel-filled outputs), assert_matches.
- ciphertext operations (tests/test_gpu_ct_*.py): SENTINEL, sentinel_out, take (outputs with guard words behind them);
  DIGIT_BITS, DIGIT_MASK; centred, negacyclic, rand_slab, unit_values; the definitions the kernels are tested against,
  rescale_expect, digits_of and relin_expect; keyed_cases, the module-scoped fixture of the end-to-end tests.
- build_example, build_caller: plain-gcc programs of examples/ and tests/c/ linked against the product library.
- check_host_tables: every setup-time table against the oracle and the golden digests (CPU suite and GPU box).
"""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SE_ERR_INVALD_ARGUMENT = -22
SE_ERR_NO_KEY = -1002

SENTINEL = 0x5A5A5A5A                 # fill of an output no call may have written
DIGIT_BITS = 15                       # SE_AMD_RELIN_DIGIT_BITS
DIGIT_MASK = (1 << DIGIT_BITS) - 1

SEED_A = hashlib.shake_256(b"golden-share").digest(64)
SEED_B = hashlib.shake_256(b"golden-secret").digest(64)
SEED_PK = hashlib.shake_256(b"golden-pk").digest(64)
SEED_EP = hashlib.shake_256(b"golden-ep").digest(64)


def gpu_env():
    """No GPU is a failure, never a skip: the product has no CPU fallback."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from oracle import pyoracle
    pyoracle.build(ref=False)
    return dict(torch=torch, pkg=pkg, dev=torch.device("cuda:0"))


@pytest.fixture(scope="module")
def env():
    return gpu_env()


def dev_t(env, a):
    """Host array -> tensor on cuda:0; uint32 travels as int32 (same bytes: only the pointer reaches the C ABI)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return env["torch"].from_numpy(a).to(env["dev"])


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def stream_of(env):
    return C.c_void_p(env["torch"].cuda.current_stream().cuda_stream)


def same_bytes(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- the receiving side: expectations from the oracle's primitives and Python integers ------------------------------
def crt_centred(o, pts):
    """pts[j][k] = value mod q_j  ->  Python ints in (-Q/2, Q/2], Q = prod q_j."""
    Q = 1
    for q in o.q:
        Q *= q
    acc = np.zeros(o.n, dtype=object)
    for j, q in enumerate(o.q):
        M = Q // q
        acc = acc + pts[j].astype(object) * (M * pow(M % q, -1, q))
    acc = acc % Q
    return [int(v) - Q if int(v) > Q // 2 else int(v) for v in acc]


def ntt_secret(o, sk):
    return [o.ntt(o.expand_ternary(sk, j), j) for j in range(o.np)]


def decode_expect(o, pte, scale=None):
    """The oracle's decode of an int64 plaintext at `scale` (default: the oracle's) -> float64 [n/2]."""
    res = o.fft((pte / (o.scale if scale is None else scale)).astype(np.complex128))
    return np.ascontiguousarray(res.real[o.map[:o.n // 2].astype(np.int64)])


def expectation(o, c0, c1, s_hat, scale=None):
    """c0, c1 [np][n] uint32 -> dict(status, pte int64 | None, y, values_f64, values) from the oracle and Python ints,
    on a record of o.np primes, decoded with `scale` (default: the oracle's)."""
    pts = [o.intt(o.decrypt(c0[j], c1[j], s_hat[j], j), j) for j in range(o.np)]
    y = crt_centred(o, pts)
    if not all(-2 ** 63 <= v < 2 ** 63 for v in y):
        return dict(status=0, pte=None, y=y)
    pte = np.array(y, dtype=np.int64)
    f64 = decode_expect(o, pte, scale)
    return dict(status=1, pte=pte, y=y, values_f64=f64, values=f64.astype(np.float32))


def run_decrypt(env, ctx, c0, c1, primes=None, scale=None, key_idx=None,
                want=("pte", "values", "values_f64", "status")):
    """decrypt_full[_keyed], or with `primes` or `scale` (the other defaults to the context's) decrypt_level[_keyed], into
    outputs pre-filled with -7 (status: 77).  -> all four outputs whatever `want` selects: one that was not requested
    must keep its fill."""
    torch = env["torch"]
    B, n = c0.shape[0], ctx.n
    out = dict(pte=torch.full((B, n), -7, dtype=torch.int64, device=env["dev"]),
               values=torch.full((B, n // 2), -7.0, dtype=torch.float32, device=env["dev"]),
               values_f64=torch.full((B, n // 2), -7.0, dtype=torch.float64, device=env["dev"]),
               status=torch.full((B,), 77, dtype=torch.uint8, device=env["dev"]))
    kw = {k: out[k] for k in want}
    keyed = () if key_idx is None else (key_idx,)
    if primes is None and scale is None:
        (ctx.decrypt_full if key_idx is None else ctx.decrypt_full_keyed)(c0, c1, *keyed, **kw)
    else:
        (ctx.decrypt_level if key_idx is None else ctx.decrypt_level_keyed)(
            c0, c1, *keyed, ctx.np if primes is None else primes, ctx.scale() if scale is None else scale, **kw)
    torch.cuda.synchronize()
    return out


def assert_matches(got, b, exp, what):
    assert int(got["status"][b]) == exp["status"], (what, "status")
    if exp["status"] != 1:
        return
    assert (got["pte"][b].cpu().numpy() == exp["pte"]).all(), (what, "pte")
    assert (bits(got["values_f64"][b].cpu().numpy()) == bits(exp["values_f64"])).all(), (what, "values_f64")
    assert (bits(got["values"][b].cpu().numpy()) == bits(exp["values"])).all(), (what, "values")


def records(n):
    """The records of the full-modulus decrypt's table plus the reference's small patterns."""
    half = n // 2
    return [("bench", V.bench_values(1, n)[0]),
            ("pattern8x100", V.pattern_values(8, n) * np.float32(100)),
            ("1e6", np.full(half, 1e6, dtype=np.float32)),
            ("2.7e11", np.full(half, 2.7e11, dtype=np.float32)),
            ("pattern4", V.pattern_values(4, n)),
            ("survey", V.survey_values(n))]


def encrypt_sym(env, ctx, vals, first=0):
    torch = env["torch"]
    B, n, npr = vals.shape[0], ctx.n, ctx.np
    ss, sd = V.bench_seeds(B, first=first)
    c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=env["dev"])
    c1 = torch.zeros_like(c0)
    pte = torch.zeros((B, n), dtype=torch.int64, device=env["dev"])
    st = torch.zeros(B, dtype=torch.uint8, device=env["dev"])
    ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), c0, c1, pte=pte, status=st)
    torch.cuda.synchronize()
    return c0, c1, pte, st


# ---- ciphertext operations: guarded outputs, inputs and the definitions of rescale and key switch -------------------
def sentinel_out(env, words, extra):
    return env["torch"].full((words + extra,), SENTINEL, dtype=env["torch"].int32, device=env["dev"])


def take(t, words, shape, what):
    """Host copy of the first `words` words of a sentinel-backed output; the words behind them must be untouched."""
    h = host_u32(t)
    assert (h[words:] == SENTINEL).all(), f"{what}: words behind the result are written"
    return h[:words].reshape(shape)


def rand_slab(rng, q, count, n, primes=None):
    primes = len(q) if primes is None else primes
    return np.stack([rng.integers(0, q[j], (count, n), dtype=np.uint32) for j in range(primes)], axis=1)


def unit_values(B, n, seed):
    """float32 [B][n/2], uniform in [-1, 1]."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, n // 2)).astype(np.float32)


def centred(x, q):
    """canonical residues -> int64 representatives in (-q/2, q/2]  (q odd)."""
    x = x.astype(np.int64)
    return np.where(x > q // 2, x - q, x)


def negacyclic(a, s):
    """a * s mod (x^n + 1) in int64 (the callers keep every sum below 2^62)."""
    n = a.shape[0]
    full = np.convolve(a, s)
    res = full[:n].copy()
    res[:n - 1] -= full[n:]
    return res


def rescale_expect(o, slab):
    """slab uint32 [B][L][n] -> uint32 [B][L-1][n]: out[j] = (in[j] - NTT_j(delta mod q_j)) . q_last^-1 mod q_j with
    delta the centred INTT of the last row, from o.intt / o.ntt and uint64 arithmetic."""
    B, L, n = slab.shape
    q_last = o.q[L - 1]
    out = np.zeros((B, L - 1, n), dtype=np.uint32)
    for b in range(B):
        delta = centred(o.intt(slab[b, L - 1], L - 1), q_last)
        for j in range(L - 1):
            q = o.q[j]
            inv = pow(q_last, -1, q)
            t = o.ntt((delta % q).astype(np.uint32), j).astype(np.uint64)
            diff = (slab[b, j].astype(np.uint64) + np.uint64(q) - t) % np.uint64(q)
            out[b, j] = ((diff * np.uint64(inv)) % np.uint64(q)).astype(np.uint32)
    return out


def digits_of(o, rec, L):
    """Record [L][n] -> the 2 L digit polynomials D_{j,t} (uint32, natural order), row r = 2j + t."""
    out = []
    for j in range(L):
        c = o.intt(rec[j], j)
        out += [c & np.uint32(DIGIT_MASK), c >> np.uint32(DIGIT_BITS)]
    return out


def relin_expect(o, d0, d1, d2, evk0, evk1):
    """The definition of the key switch, which relinearisation and rotation are both tested against:
    out_k[b][i] = d_k[b][i] + sum_r NTT_i(D_r) . evk_k[r][i] mod q_i, from o.intt / o.ntt and uint64 arithmetic (a
    product is below 2^60, reduced before it is added)."""
    B, L, n = d0.shape
    out0, out1 = np.zeros_like(d0), np.zeros_like(d1)
    for b in range(B):
        D = digits_of(o, d2[b], L)
        for i in range(L):
            q = np.uint64(o.q[i])
            acc0, acc1 = d0[b, i].astype(np.uint64), d1[b, i].astype(np.uint64)
            for r, dig in enumerate(D):
                f = o.ntt(dig, i).astype(np.uint64)
                acc0 = (acc0 + (f * evk0[r, i].astype(np.uint64)) % q) % q
                acc1 = (acc1 + (f * evk1[r, i].astype(np.uint64)) % q) % q
            out0[b, i], out1[b, i] = acc0, acc1
    return out0, out1


@pytest.fixture(scope="module")
def keyed_cases(env, request):
    """keyed_cases(shape) -> the importing module's end-to-end case of that shape, computed once: a context of the shape
    ("ctx") with the secret key V.secret_key(n, seed=5) installed ("sk", "s_hat" its NTT form from the oracle "o"), then
    whatever the module's fill_keyed_case(env, case) adds to the dict -- its evaluation keys, records and results.  The
    contexts are closed when the module is done."""
    from oracle.pyoracle import Oracle
    cache = {}

    def get(shape):
        if shape not in cache:
            n, npr = shape
            o = Oracle(n, npr)
            ctx = env["pkg"].Context(n, npr)
            sk = V.secret_key(n, seed=5)
            ctx.set_secret_key(sk)
            cache[shape] = case = dict(ctx=ctx, o=o, sk=sk, s_hat=ntt_secret(o, sk))
            request.module.fill_keyed_case(env, case)
        return cache[shape]

    yield get
    for c in cache.values():
        c["ctx"].close()


# ---- C callers ------------------------------------------------------------------------------------------------------
def _link(src, exe, flags):
    lib = os.path.join(ROOT, "seal-embedded_amd", "lib")
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", src, "-I" + os.path.join(ROOT, "include"), "-L" + lib,
                    "-lseal_embedded_amd", "-Wl,-rpath," + lib, "-o", str(exe), *flags], check=True)
    return exe


def build_example(name, tmp_path, hip=False, extra=()):
    """examples/<name>.c -> tmp_path/<name>, plain gcc against the product library.  hip: a C caller that owns device
    memory (the HIP runtime's C API, still plain gcc); extra: further flags, such as -lm."""
    flags = ["-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-L/opt/rocm/lib", "-lamdhip64",
             "-Wl,-rpath,/opt/rocm/lib"] if hip else []
    return _link(os.path.join(ROOT, "examples", name + ".c"), tmp_path / name, flags + list(extra))


def build_caller(name, tmp_path):
    """tests/c/<name>.c (written against the reference's header names) -> tmp_path/<name>, with -Wextra."""
    return _link(os.path.join(ROOT, "tests", "c", name + ".c"), tmp_path / name,
                 ["-Wextra", "-I" + os.path.join(ROOT, "include", "compat")])


# ---- host tables ----------------------------------------------------------------------------------------------------
def check_host_tables(pkg, shape):
    """The setup-time tables the context uploads (host logic, no GPU): parameter set, index map, libm IFFT roots
    (bit-exact doubles; digest pinned to the reference build host), NTT roots + Shoup companions, inverse
    roots."""
    from oracle.pyoracle import Oracle
    n, npr = shape
    t = pkg.host_tables(n, npr)
    o = Oracle(n, npr)
    assert [int(x) for x in t["q"]] == [int(o.p.q[j]) for j in range(npr)]
    assert [(int(a), int(b)) for a, b in t["const_ratio"]] == \
        [(int(o.p.cr_lo[j]), int(o.p.cr_hi[j])) for j in range(npr)]
    for j in range(npr):
        q = int(t["q"][j])
        cr = (int(t["const_ratio"][j][1]) << 32) | int(t["const_ratio"][j][0])
        assert cr == (1 << 64) // q
    assert t["scale"] == o.p.scale
    assert (t["index_map"] == o.map).all()
    tw = o.twiddles()
    assert t["ifft_w"].ravel().tobytes() == tw.tobytes()
    dig = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_digests.json")))["ifft_twiddle_sha256"]
    assert hashlib.sha256(t["ifft_w"].astype("<f8").tobytes()).hexdigest() == dig[str(n)]
    for j in range(npr):
        q = int(t["q"][j])
        r = t["ntt_rw"][j, :, 0].astype(np.uint64)
        assert (r == o.ntt_roots(j)).all()
        assert (t["ntt_rw"][j, :, 1].astype(np.uint64) == (r << np.uint64(32)) // np.uint64(q)).all()
        ir = t["intt_rw"][j, :, 0].astype(np.uint64)
        assert ((r * ir) % np.uint64(q) == 1).all()       # same bit-reversed slot: psi^i * psi^-i
        assert (t["intt_rw"][j, :, 1].astype(np.uint64) == (ir << np.uint64(32)) // np.uint64(q)).all()
    with pytest.raises(pkg.SealEmbeddedAmdError):
        pkg.host_tables(3000, 1)
