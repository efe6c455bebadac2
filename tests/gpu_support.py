"""Device plumbing that the GPU test modules (tests/test_gpu_*.py) share.  Tests import helpers from here (`from
gpu_support import env, dev_t, ...`) and the host model from ct_model, never from another test module; a helper that a
second module needs moves here (device code) or to ct_model (definitions and inputs).  Nothing of ct_model is re-exported.

- env: the module-scoped fixture (torch, the loaded package, cuda:0); gpu_env() is the same setup as a plain function.
- dev_t, host_u32, bits, stream_of, same_bytes: host <-> device and bit-pattern conveniences.
- SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY: the C ABI's error codes; SEED_A, SEED_B, SEED_PK, SEED_EP: the golden seeds.
- the C entries called directly (the arguments tests): NULL, dptr, hptr (pointers); CEntry, a good argument list by name
  whose calls replace named fields and whose refused() runs a table of such edits; create_handle, creates_refused (the
  same for the create entries, which hand back a handle); assert_untouched, assert_zero_prefix (what the refused and
  the zero-slab calls may have written).
- the receiving side: records, encrypt_sym, fresh_records, ntt_secret, decode_expect, expectation (oracle + Python ints),
  run_decrypt (decrypt_full / decrypt_level / decrypt3_level and their keyed twins over filled outputs), assert_matches,
  check_level_decrypt.
- ciphertext operations (tests/test_gpu_ct_*.py): SENTINEL, sentinel_out, take (outputs with guard words behind them); one
  runner per entry (run_relin, run_galois, run_many, run_sum, run_plan and the special-prime run_relin_sp,
  run_galois_sp), each one call with two rows of sentinels behind each output; keyed_cases, the module-scoped fixture of
  the end-to-end tests, with step_elements, install_galois_keys, lift_records, rescale_records and encode_diagonals, the
  blocks those tests repeat.
- batches at scale (tests/test_gpu_ct_scale.py; shown on the CPU by tests/test_tiled_support.py): tiled (K records repeated
  to B on the device), assert_tiles (every record of a slab against its pattern record, on the device, with slab_position
  in its report), tiled_row_ptr, tiled_idx, tiled_entries (CSR rows that repeat a local pattern per tile).
- build_example, build_caller, run_example: plain-gcc programs of examples/ and tests/c/ linked against the product library.
- check_host_tables: every setup-time table against the oracle and the golden digests (CPU suite and GPU box).
"""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import vectors as V
from ct_model import crt_centred, galois_seeds, lift_expect, rescale_expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SE_ERR_INVALD_ARGUMENT = -22
SE_ERR_NO_KEY = -1002

SENTINEL = 0x5A5A5A5A                 # fill of an output no call may have written

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


# ---- the C entries called directly: pointers, a good argument list by name, what a refused call must leave alone ------
NULL = C.c_void_p(None)


def dptr(t, off=0):
    """The device pointer of tensor `t`, `off` bytes in (the misalignment cases)."""
    return C.c_void_p(t.data_ptr() + off)


def hptr(a):
    """The host pointer of NumPy array `a`."""
    return C.c_void_p(a.ctypes.data)


class CEntry:
    """A C entry with a good argument list by name: CEntry(fn, ctx=h, c0=dptr(c0), ..., stream=s), the keywords in the
    C parameter order.  entry(**edits) calls fn with the named fields replaced and returns its code."""

    def __init__(self, fn, **good):
        self.fn, self.good = fn, good

    def __call__(self, **edits):
        unknown = [k for k in edits if k not in self.good]
        if unknown:
            raise TypeError(f"no argument named {unknown} among {list(self.good)}")
        return self.fn(*{**self.good, **edits}.values())

    def refused(self, cases, code=SE_ERR_INVALD_ARGUMENT):
        """Every edit dict of `cases`, in order, must make the entry return `code`."""
        name = getattr(self.fn, "__name__", self.fn)
        for k, edits in enumerate(cases):
            got = self(**edits)
            assert got == code, f"{name}, case {k} {edits}: returned {got}, not {code}"


def create_handle(entry, **edits):
    """One call of a create entry (se_amd_lintrans_create*, se_amd_bsgs_create*) whose `out` field, unless edited, is
    the byref of a handle that holds 0xDEAD: a failed create must overwrite it with NULL.  -> code, handle."""
    handle = C.c_void_p(0xDEAD)
    return entry(**{"out": C.byref(handle), **edits}), handle


def creates_refused(entry, cases, code=SE_ERR_INVALD_ARGUMENT):
    """CEntry.refused for a create entry: every case returns `code` and leaves the handle NULL."""
    for k, edits in enumerate(cases):
        rc, handle = create_handle(entry, **edits)
        assert rc == code and handle.value is None, (k, edits, rc, handle.value)


def assert_untouched(*tensors, fill=SENTINEL):
    """After a synchronise every word of every tensor still holds its fill (status tensors: 77)."""
    import torch
    torch.cuda.synchronize()
    for k, t in enumerate(tensors):
        assert bool((t == fill).all()), f"tensor {k} was written"


def assert_zero_prefix(t, words):
    """After a synchronise the first `words` words of `t` are zero and everything behind is SENTINEL."""
    import torch
    torch.cuda.synchronize()
    flat = t.reshape(-1)
    assert int(torch.count_nonzero(flat[:words])) == 0 and bool((flat[words:] == SENTINEL).all())


# ---- the receiving side: expectations from the oracle's primitives and Python integers ------------------------------
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
    y = crt_centred(o.q, pts)
    if not all(-2 ** 63 <= v < 2 ** 63 for v in y):
        return dict(status=0, pte=None, y=y)
    pte = np.array(y, dtype=np.int64)
    f64 = decode_expect(o, pte, scale)
    return dict(status=1, pte=pte, y=y, values_f64=f64, values=f64.astype(np.float32))


def run_decrypt(env, ctx, c0, c1, primes=None, scale=None, key_idx=None,
                want=("pte", "values", "values_f64", "status"), c2=None):
    """decrypt_full[_keyed], or with `primes` or `scale` (the other defaults to the context's) decrypt_level[_keyed], or
    with a third slab `c2` decrypt3_level[_keyed], into outputs pre-filled with -7 (status: 77).  -> all four outputs
    whatever `want` selects: one that was not requested must keep its fill."""
    torch = env["torch"]
    B, n = c0.shape[0], ctx.n
    out = dict(pte=torch.full((B, n), -7, dtype=torch.int64, device=env["dev"]),
               values=torch.full((B, n // 2), -7.0, dtype=torch.float32, device=env["dev"]),
               values_f64=torch.full((B, n // 2), -7.0, dtype=torch.float64, device=env["dev"]),
               status=torch.full((B,), 77, dtype=torch.uint8, device=env["dev"]))
    kw = {k: out[k] for k in want}
    keyed = () if key_idx is None else (key_idx,)
    if c2 is not None:
        (ctx.decrypt3_level if key_idx is None else ctx.decrypt3_level_keyed)(
            c0, c1, c2, *keyed, ctx.np if primes is None else primes, ctx.scale() if scale is None else scale, **kw)
    elif primes is None and scale is None:
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


# ---- ciphertext operations: guarded outputs, one runner per entry, the blocks of the end-to-end tests ----------------
def sentinel_out(env, words, extra):
    return env["torch"].full((words + extra,), SENTINEL, dtype=env["torch"].int32, device=env["dev"])


def take(t, words, shape, what):
    """Host copy of the first `words` words of a sentinel-backed output; the words behind them must be untouched."""
    h = host_u32(t)
    assert (h[words:] == SENTINEL).all(), f"{what}: words behind the result are written"
    return h[:words].reshape(shape)


def guarded_pair(env, n, shape, what, call):
    """call(out0, out1) on two outputs of `shape` words with two rows of sentinels behind each -> their host copies (take:
    the sentinels must have survived)."""
    words = int(np.prod(shape))
    out0, out1 = sentinel_out(env, words, 2 * n), sentinel_out(env, words, 2 * n)
    call(out0, out1)
    env["torch"].cuda.synchronize()
    return take(out0, words, shape, what + " out0"), take(out1, words, shape, what + " out1")


def run_relin(env, ctx, d0, d1, d2, primes):
    """One ct_relin call on device slabs [B][primes][n]."""
    return guarded_pair(env, ctx.n, (d0.shape[0], primes, ctx.n), "relin",
                        lambda a, b: ctx.ct_relin(d0, d1, d2, a, b, primes=primes))


def run_relin_sp(env, ctx, d0, d1, d2, primes):
    return guarded_pair(env, ctx.n, (d0.shape[0], primes, ctx.n), "relin_sp",
                        lambda a, b: ctx.ct_relin_sp(d0, d1, d2, a, b, primes=primes))


def run_galois(env, ctx, c0, c1, elt, primes):
    """One ct_galois call on device slabs [B][primes][n]."""
    return guarded_pair(env, ctx.n, (c0.shape[0], primes, ctx.n), "galois",
                        lambda a, b: ctx.ct_galois(c0, c1, elt, a, b, primes=primes))


def run_galois_sp(env, ctx, c0, c1, elt, primes):
    return guarded_pair(env, ctx.n, (c0.shape[0], primes, ctx.n), "galois_sp",
                        lambda a, b: ctx.ct_galois_sp(c0, c1, elt, a, b, primes=primes))


def run_many(env, ctx, c0, c1, elts, primes):
    """One many-form call on device slabs [B][primes][n] -> [G][B][primes][n] each."""
    return guarded_pair(env, ctx.n, (len(elts), c0.shape[0], primes, ctx.n), "many",
                        lambda a, b: ctx.ct_galois_many(c0, c1, elts, a, b, primes=primes))


def run_sum(env, ctx, c0, c1, elts, primes, add_input):
    """One sum-form call (ct_galois_sum) on device slabs [B][primes][n]."""
    return guarded_pair(env, ctx.n, (c0.shape[0], primes, ctx.n), "sum",
                        lambda a, b: ctx.ct_galois_sum(c0, c1, elts, a, b, add_input=add_input, primes=primes))


def run_plan(env, ctx, plan, c0, c1, primes):
    """One ct_lintrans call of a flat plan on device slabs [B][primes][n]."""
    return guarded_pair(env, ctx.n, (c0.shape[0], primes, ctx.n), "lintrans",
                        lambda a, b: ctx.ct_lintrans(plan, c0, c1, a, b, primes=primes))


def unit_values(B, n, seed):
    """float32 [B][n/2], uniform in [-1, 1]."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, n // 2)).astype(np.float32)


def periodic_values(B, n, dim, seed):
    """float32 [B][n/2]: per record a dim-vector uniform in [-1, 1], repeated through the slots."""
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, (B, dim))
    return np.tile(x, (1, n // 2 // dim)).astype(np.float32)


def fresh_records(env, ctx, vals, first):
    """vals encrypted under the installed secret key with the bench seeds from `first` on; every record must encode."""
    c0, c1, _, st = encrypt_sym(env, ctx, vals, first=first)
    assert bool((st == 1).all())
    return c0, c1


def step_elements(env, n, steps):
    """The Galois elements of the slot rotations by `steps` from the package, which must be 3^step mod 2n."""
    elts = [env["pkg"].galois_element(n, s) for s in steps]
    assert elts == [pow(3, s % (n // 2), 2 * n) for s in steps]
    return elts


def install_galois_keys(case, elts, label, sp=False):
    """Generate the Galois keys of `elts` under the case's secret key from the seeds derive_seeds(label + "-a" / "-e")
    and install them: digit keys, or with sp the special-prime keys.  -> gk0, gk1."""
    ctx = case["ctx"]
    gen, install = (ctx.gen_galois_keys_sp, ctx.set_galois_keys_sp) if sp else (ctx.gen_galois_keys, ctx.set_galois_keys)
    gk0, gk1 = gen(case["sk"], elts, *galois_seeds(ctx.np, len(elts), label, sp))
    install(elts, gk0, gk1)
    return gk0, gk1


def drop_records(env, ctx, c0, c1, L):
    """ct_drop_primes of full records to L primes, which must equal the slices -> host l0, l1 [B][L][n]."""
    l0, l1 = guarded_pair(env, ctx.n, (c0.shape[0], L, ctx.n), "drop",
                          lambda a, b: ctx.ct_drop_primes(c0, a, c1, b, primes_in=ctx.np, primes_out=L))
    assert (l0 == host_u32(c0)[:, :L]).all() and (l1 == host_u32(c1)[:, :L]).all()
    return l0, l1


def lift_records(env, ctx, o, fresh, weight):
    """The lift: ct_lincomb with one CSR row per record holding the single weight; equal to the product in the test's
    own integers -> host l0, l1 [B][np][n]."""
    c0, c1 = fresh
    B = c0.shape[0]
    l0, l1 = guarded_pair(env, ctx.n, (B, ctx.np, ctx.n), "lift", lambda a, b: ctx.ct_lincomb(
        c0, a, c1, b, row_ptr=dev_t(env, np.arange(B + 1, dtype=np.uint32)), idx=dev_t(env, np.arange(B, dtype=np.uint32)),
        w=dev_t(env, np.full(B, weight, dtype=np.int32))))
    assert (l0 == lift_expect(o, host_u32(c0), weight)).all() and (l1 == lift_expect(o, host_u32(c1), weight)).all()
    return l0, l1


def encode_diagonals(env, ctx, o, dvals):
    """encode_ntt of float32 [dim][n/2] on the device, equal to the oracle's encoding -> host uint32 [dim][np][n]."""
    dim, npr, n = dvals.shape[0], ctx.np, ctx.n
    enc = sentinel_out(env, dim * npr * n, 2 * n)
    ctx.encode_ntt(dev_t(env, dvals), enc)
    env["torch"].cuda.synchronize()
    ok, enc_want = o.encode_ntt_batch(dvals)
    assert ok
    diag = take(enc, dim * npr * n, (dim, npr, n), "encoded diagonals")
    assert (diag == enc_want).all()
    return diag


def check_headroom(o, g0, g1, s_hat, what):
    """Every coefficient of the records' centred decrypt is below 2^62, the room the int64 stages need."""
    for b in range(g0.shape[0]):
        big = max(abs(v) for v in expectation(o, g0[b], g1[b], s_hat)["y"])
        print(f"{what}, record {b}: log2 of the largest coefficient = {np.log2(float(big)):.2f}")
        assert big < 2 ** 62, (what, b, big)


def rescale_records(env, ctx, o, g0, g1, primes, what="rescale"):
    """ct_rescale of host records [B][primes][n], equal to rescale_expect -> host f0, f1 [B][primes - 1][n]."""
    f0, f1 = guarded_pair(env, ctx.n, (g0.shape[0], primes - 1, ctx.n), "rescale",
                          lambda a, b: ctx.ct_rescale(dev_t(env, g0), a, dev_t(env, g1), b, primes=primes))
    assert (f0 == rescale_expect(o, g0)).all() and (f1 == rescale_expect(o, g1)).all(), what
    return f0, f1


def check_level_decrypt(env, ctx, lo, r0, r1, s_hat, primes, scale, want, what="decrypt"):
    """decrypt_level on host records [B][primes][n] against the oracle expectation (lo: the oracle of that level) on the
    same records, bit for bit; the reference's 0.1 against want[b] first on the expectation, then on the GPU result.
    -> the largest error of the GPU result, printed."""
    got = run_decrypt(env, ctx, dev_t(env, r0), dev_t(env, r1), primes, scale)
    worst = 0.0
    for b in range(r0.shape[0]):
        e = expectation(lo, r0[b], r1[b], s_hat[:primes], scale)
        assert e["status"] == 1
        assert_matches(got, b, e, (what, b))
        err_e = float(np.abs(e["values"].astype(np.float64) - want[b]).max())
        err_g = float(np.abs(got["values"][b].cpu().numpy().astype(np.float64) - want[b]).max())
        print(f"{what}, record {b}: max |values - expected| = {err_e:.3e} (expectation), {err_g:.3e} (GPU)")
        assert err_e < 0.1 and err_g < 0.1, (what, b, err_e, err_g)
        worst = max(worst, err_g)
    print(f"{ctx.n} x {ctx.np}, {what}: worst error {worst:.3e}")
    assert worst < 0.1
    return worst


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


# ---- K records tiled to a batch of B: built and compared on the device (tests/test_gpu_ct_scale.py) -------------------
def as_tensor(env, a):
    """A tensor on env["dev"] of a host array (dev_t) or of a tensor, which is returned as it is."""
    return dev_t(env, a) if isinstance(a, np.ndarray) else a


def tiled(env, base, B, out=None):
    """base [K, ...] (a tensor on the device, or a host array that goes there) -> [B, ...] whose record b is base[b % K],
    B a multiple of K, from one broadcast assignment into the [B / K, K, ...] view: no host slab.  `out`: a contiguous
    view of a caller's buffer of that shape and type, which is written and returned."""
    base = as_tensor(env, base)
    K, rest = base.shape[0], tuple(base.shape[1:])
    assert K >= 1 and B >= K and B % K == 0, (B, K)
    if out is None:
        out = env["torch"].empty((B,) + rest, dtype=base.dtype, device=base.device)
    assert tuple(out.shape) == (B,) + rest and out.dtype == base.dtype and out.is_contiguous(), (out.shape, out.dtype)
    out.view(B // K, K, *rest)[...] = base
    return out


def _bit_view(env, t):
    """The same bytes as integers: floats compare by bit pattern (a NaN equals itself, -0.0 differs from 0.0)."""
    torch = env["torch"]
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def slab_position(record, words, size):
    """Where record `record` of a slab of `words`-word records of `size`-byte words starts, against the three offsets at
    which a narrow index wraps: byte 2^32, word 2^31 (an int) and word 2^32 (a uint32_t)."""
    off = record * words
    side = lambda past: "at or past" if past else "before"  # noqa: E731
    return (f"starts at word {off} = byte {off * size} of the slab: {side(off * size >= 2 ** 32)} byte 2^32, "
            f"{side(off >= 2 ** 31)} word 2^31, {side(off >= 2 ** 32)} word 2^32")


def assert_tiles(env, got, exp, what, guard=None, chunk_bytes=1 << 30):
    """Every record b of the device tensor got [B, ...] equals exp[b % K] (exp [K, ...], a tensor or a host array),
    compared on the device bit for bit in chunks of whole tiles whose temporaries stay within about `chunk_bytes`; no
    record is left out.  `guard`: the words behind the result, which must all still hold SENTINEL.  A mismatch names the
    first bad record with its row and word, how many records differ, and where that record's first word lies relative
    to byte 2^32, word 2^31 and word 2^32 of the slab."""
    torch = env["torch"]
    exp = _bit_view(env, as_tensor(env, exp)).contiguous()
    got = _bit_view(env, got)
    assert got.is_contiguous() and got.dtype == exp.dtype, (what, got.dtype, exp.dtype)
    B, K = got.shape[0], exp.shape[0]
    assert B % K == 0 and tuple(got.shape[1:]) == tuple(exp.shape[1:]), (what, tuple(got.shape), tuple(exp.shape))
    words = max(1, exp[0].numel())                                       # words of one record
    last = exp.shape[-1] if exp.dim() > 1 else 1                         # words of one row
    # per compared word: one bool of the comparison and, for the broadcast, at most one word of `exp`
    tiles_per_chunk = max(1, chunk_bytes // (K * words * (1 + exp.element_size())))
    g3, e3 = got.view(B // K, K, words), exp.view(1, K, words)
    bad = torch.zeros((B // K, K), dtype=torch.bool, device=got.device)
    for t0 in range(0, B // K, tiles_per_chunk):
        t1 = min(B // K, t0 + tiles_per_chunk)
        bad[t0:t1] = (g3[t0:t1] != e3).any(dim=2)
    bad = bad.view(B)
    count = int(bad.sum())
    if count:
        first = int(torch.nonzero(bad)[0, 0])
        diff = torch.nonzero(g3.view(B, words)[first] != e3.view(K, words)[first % K])
        at = int(diff[0, 0])
        raise AssertionError(
            f"{what}: {count} of {B} records differ; first bad record {first} (tile {first // K}, pattern record "
            f"{first % K}), row {at // last}, word {at % last}: got {int(g3.view(B, words)[first, at]):#x}, expected "
            f"{int(e3.view(K, words)[first % K, at]):#x} ({int(diff.shape[0])} words of that record differ); the record "
            + slab_position(first, words, exp.element_size()))
    if guard is not None:
        wrong = int((guard != SENTINEL).sum())
        assert wrong == 0, f"{what}: {wrong} of the {guard.numel()} guard words behind the result are written"


def tiled_row_ptr(env, local_ptr, tiles):
    """CSR row_ptr of `tiles` copies of a pattern of R rows with local row_ptr `local_ptr` [R + 1] (local_ptr[0] == 0):
    row g starts at (g // R) . nnz + local_ptr[g % R], built on the device -> int32 [tiles . R + 1]."""
    torch = env["torch"]
    lp = torch.as_tensor(np.asarray(local_ptr, dtype=np.int64), device=env["dev"])
    R, nnz = lp.numel() - 1, int(local_ptr[-1])
    assert R >= 1 and int(local_ptr[0]) == 0 and tiles * nnz < 2 ** 31, (R, nnz, tiles)
    out = torch.empty(tiles * R + 1, dtype=torch.int64, device=env["dev"])
    out[:tiles * R].view(tiles, R)[...] = torch.arange(tiles, device=env["dev"])[:, None] * nnz + lp[None, :R]
    out[tiles * R] = tiles * nnz
    return out.to(torch.int32)


def tiled_idx(env, local_idx, K, tiles):
    """CSR record indices of the same: entry k = (k // nnz) . K + local_idx[k % nnz], every local index below K, so that
    a row of tile t reads records of tile t alone -> int32 [tiles . nnz]."""
    torch = env["torch"]
    li = torch.as_tensor(np.asarray(local_idx, dtype=np.int64), device=env["dev"])
    assert li.numel() >= 1 and 0 <= int(li.min()) and int(li.max()) < K and tiles * K < 2 ** 31, (K, tiles)
    out = torch.arange(tiles, device=env["dev"])[:, None] * K + li[None, :]
    return out.reshape(-1).to(torch.int32)


def tiled_entries(env, local, tiles):
    """What a CSR entry carries beside its record index (eidx, weights) or a record carries beside its rows (key_idx):
    the pattern's values as they are, repeated per tile -> [tiles . len(local)] of the pattern's own type."""
    base = as_tensor(env, np.ascontiguousarray(local))
    return tiled(env, base, tiles * base.shape[0])


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


def run_example(name, tmp_path, args, bound=0.1):
    """Build examples/<name>.c (a HIP-owning C caller, with -lm), run it with `args` = n, np, B, ...: it must exit 0 and
    report failed=0 for its B records with a largest absolute error below `bound`, the reference's 0.1."""
    exe = build_example(name, tmp_path, hip=True, extra=("-lm",))
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"failed=0 B=%s .*max_abs_error=([0-9.e+-]+)" % args[2], r.stdout)
    assert m and float(m.group(1)) < bound, r.stdout


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
