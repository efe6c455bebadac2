"""The two-way pair form of the fused n = 4096 kernels (-m gpu): k_encode_encrypt_pair2 takes the whole pairs of a fast,
unkeyed symmetric / encode-only launch; debug flag 8192 keeps the one-plane pair form (k_encode_encrypt) for everything.
Every record of every case against the oracle, bit for bit on c0, c1, ntt_pte, pte and status, and the two forms against
each other byte for byte.  n = 4096, three primes."""
import numpy as np
import pytest

import vectors as V
from gpu_support import dev_t, env, host_u32  # noqa: F401  (env is a fixture)

pytestmark = pytest.mark.gpu

N, NPR = 4096, 3
ONE_PLANE = 8192        # kEncFlagOnePlane (kernels/kernel_args.h)
FIELDS = ("c0", "c1", "ntt_pte", "pte", "status")


@pytest.fixture(scope="module")
def case(env):
    from oracle.pyoracle import Oracle
    sk = V.secret_key(N, seed=5)
    ctx = env["pkg"].Context(N, NPR)
    ctx.set_secret_key(sk)
    ctx.set_pipeline(True, False)       # the fused kernel whatever the batch
    yield dict(ctx=ctx, sk=sk, o=Oracle(N, NPR))
    ctx.close()


def outputs(env, B):
    torch = env["torch"]
    c0 = torch.zeros((B, NPR, N), dtype=torch.int32, device=env["dev"])
    return dict(c0=c0, c1=torch.zeros_like(c0), ntt_pte=torch.zeros_like(c0),
                pte=torch.zeros((B, N), dtype=torch.int64, device=env["dev"]),
                status=torch.full((B,), 77, dtype=torch.uint8, device=env["dev"]))


def run_sym(env, ctx, vals, ss, sd, flags, extras=True):
    o = outputs(env, vals.shape[0])
    ctx.set_debug_flags(flags)
    ctx.encrypt_sym(dev_t(env, vals), dev_t(env, ss), dev_t(env, sd), o["c0"], o["c1"],
                    o["ntt_pte"] if extras else None, o["pte"] if extras else None, o["status"])
    env["torch"].cuda.synchronize()
    ctx.set_debug_flags(0)
    return {k: v.cpu().numpy() for k, v in o.items()}


def run_encode(env, ctx, vals, flags, extras=True):
    o = outputs(env, vals.shape[0])
    ctx.set_debug_flags(flags)
    if extras:
        ctx.encode_ntt(dev_t(env, vals), o["c0"], pte=o["pte"], status=o["status"])
    else:
        ctx.encode_ntt(dev_t(env, vals), o["c0"])
    env["torch"].cuda.synchronize()
    ctx.set_debug_flags(0)
    return {k: v.cpu().numpy() for k, v in o.items()}


def same(a, b, fields, what):
    for f in fields:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def check_both_forms(env, case, vals, first, what):
    """vals through the symmetric and the encode-only entry in both forms: each record equals the oracle's, and the forms
    equal each other byte for byte."""
    ctx, o, sk = case["ctx"], case["o"], case["sk"]
    B = vals.shape[0]
    ss, sd = V.bench_seeds(B, first=first)
    exp = []
    for b in range(B):
        ok, m = o.encode(vals[b])
        exp.append((ok, m, o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)))
    got = {}
    for flags in (0, ONE_PLANE):
        g = got[flags] = run_sym(env, ctx, vals, ss, sd, flags)
        for b, (ok, m, r) in enumerate(exp):
            assert int(g["status"][b]) == int(ok) == int(r["ok"]), (what, flags, b)
            if not ok:
                continue        # the reference's `return false`: nothing else of the record is defined
            assert (g["c0"][b].view(np.uint32) == r["c0"]).all(), (what, flags, b, "c0")
            assert (g["c1"][b].view(np.uint32) == r["c1"]).all(), (what, flags, b, "c1")
            assert (g["ntt_pte"][b].view(np.uint32) == r["ntt_pte"]).all(), (what, flags, b, "ntt_pte")
            assert (g["pte"][b] == r["pte"]).all(), (what, flags, b, "pte")
    same(got[0], got[ONE_PLANE], FIELDS, what)
    enc = {}
    for flags in (0, ONE_PLANE):
        g = enc[flags] = run_encode(env, ctx, vals, flags)
        for b, (ok, m, r) in enumerate(exp):
            assert int(g["status"][b]) == int(ok), (what, "encode", flags, b)
            if not ok:
                continue
            assert (g["pte"][b] == m).all(), (what, "encode", flags, b, "pte")
            for j in range(NPR):
                assert (g["c0"][b, j].view(np.uint32) == o.ntt(o.reduce_pte(m, j), j)).all(), (what, "encode", flags, b, j)
    same(enc[0], enc[ONE_PLANE], ("c0", "pte", "status"), what + " encode")
    return got[0], enc[0]


@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_batch_sizes(env, case, B):
    """B = 1: the one-plane form alone; 2: one pair; 3 and 5: pairs plus the odd last plaintext on the one-plane form."""
    check_both_forms(env, case, V.bench_values(B, N, first=7300 + B), 7300 + B, f"B{B}")


def tie_rows():
    """Constructed rounding ties (as tests/test_gpu_parity.py::test_pair_form_of_the_fused_kernels_on_odd_batches): a
    constant slot vector v = (2k+1) / 2^26 encodes to m_0 = k + 0.5 exactly, every other coefficient 0 -- distance 0 to
    the half-integer, so the half-size transform must flag the plaintext and the full transform must round half away from
    zero; one non-zero slot (2k+1) / 2^15 gives ties decided by the reference's own rounding noise."""
    pos = np.full(N // 2, np.float32(75.0 / 2.0 ** 26), dtype=np.float32)              # m_0 = 37.5 -> 38
    neg = np.full(N // 2, np.float32(-(2 * 4001 + 1) / 2.0 ** 26), dtype=np.float32)   # m_0 = -4001.5 -> -4002
    noise = np.zeros(N // 2, dtype=np.float32)
    noise[17] = np.float32((2 * 12345 + 1) / 2.0 ** 15)
    return pos, neg, noise


def test_guard_band_in_either_both_or_neither_plaintext_of_a_pair(env, case):
    pos, neg, noise = tie_rows()
    o = case["o"]
    # the constructed inputs are what they are meant to be, on the host: exact ties rounded half away from zero
    assert o.encode(pos)[1][0] == 38 and o.encode(neg)[1][0] == -4002
    assert not o.encode(pos)[1][1:].any() and not o.encode(neg)[1][1:].any()
    assert np.abs(o.encode(noise)[1]).max() in (12345, 12346)
    plain = V.bench_values(4, N, first=7400)
    #        A tie, B plain | A plain, B tie | both     | neither            | noise tie first | noise tie second
    vals = np.stack([pos, plain[0], plain[1], neg, neg, pos, plain[2], plain[3], noise, plain[0], plain[1], noise])
    check_both_forms(env, case, vals, 7400, "guard band")


def test_pair_with_a_declined_partner(env, case):
    """One plaintext of a pair over the int32 range or non-finite (the general list and its status bytes), in either
    position, and a pair that is declined altogether."""
    v = V.bench_values(10, N, first=7500)
    v[1] *= 60.0                  # not small, second of its pair
    v[2] *= 1000.0                # first of its pair
    v[5, 7] = float("nan")        # non-finite, second
    v[6, 2047] = float("inf")     # infinite (status 0), first
    v[8] *= 1.0e6                 # both declined: beyond 32 bits ...
    v[9, 0] = float("nan")        # ... and non-finite
    sym, _ = check_both_forms(env, case, v, 7500, "declined partner")
    assert list(sym["status"]) == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1]


def test_optional_outputs(env, case):
    """ntt_pte / pte not requested: c0, c1 and status are those of the call that requests them, in both forms."""
    ctx = case["ctx"]
    vals = V.bench_values(4, N, first=7600)
    ss, sd = V.bench_seeds(4, first=7600)
    full = run_sym(env, ctx, vals, ss, sd, 0)
    for flags in (0, ONE_PLANE):
        bare = run_sym(env, ctx, vals, ss, sd, flags, extras=False)
        same(full, bare, ("c0", "c1", "status"), ("bare", flags))
        assert not bare["ntt_pte"].any() and not bare["pte"].any()
    efull = run_encode(env, ctx, vals, 0)
    for flags in (0, ONE_PLANE):
        ebare = run_encode(env, ctx, vals, flags, extras=False)
        same(efull, ebare, ("c0",), ("bare encode", flags))
        assert not ebare["pte"].any() and (ebare["status"] == 77).all()


def test_keyed_call_is_unchanged(env, case):
    """A keyed launch keeps the one-plane form whatever the flag: equal in both settings, and equal to the unkeyed call
    under each record's key (which takes the two-way form)."""
    torch = env["torch"]
    K, B = 3, 6
    ctx = env["pkg"].Context(N, NPR)
    ctx.set_pipeline(True, False)
    sk, _, _ = ctx.gen_keys_batch(V.derive_seeds("pair2-pk", K), V.derive_seeds("pair2-ep", K),
                                  sk_seeds=V.derive_seeds("pair2-sk", K))
    ctx.set_secret_keyring(sk)
    vals = V.bench_values(B, N, first=7700)
    ss, sd = V.bench_seeds(B, first=7700)
    idx = np.array([0, 0, 1, 1, 2, 2], dtype=np.uint32)
    got = {}
    for flags in (0, ONE_PLANE):
        o = outputs(env, B)
        ctx.set_debug_flags(flags)
        ctx.encrypt_sym_keyed(dev_t(env, vals), dev_t(env, idx), dev_t(env, ss), dev_t(env, sd), o["c0"], o["c1"],
                              o["ntt_pte"], o["pte"], o["status"])
        torch.cuda.synchronize()
        got[flags] = {k: v.cpu().numpy() for k, v in o.items()}
    ctx.set_debug_flags(0)
    same(got[0], got[ONE_PLANE], FIELDS, "keyed")
    for k in range(K):
        ctx.set_secret_key(sk[k])
        sel = np.nonzero(idx == k)[0]
        ref = run_sym(env, ctx, vals[sel], ss[sel], sd[sel], 0)
        for f in FIELDS:
            assert got[0][f][sel].tobytes() == ref[f].tobytes(), (k, f)
    ctx.close()
