"""The stream contract on the real runtime: "asynchronous on `stream`" for one entry of each host-side shape, on a stream
of the caller's that is NOT the null stream.  Every other GPU test passes torch.cuda.current_stream() outside a stream
context, which is the null stream and orders itself against everything, so a launch that escaped to another stream, or
an auxiliary stream the caller's stream never waits for, gives the right bits there.

Each case, inside `with torch.cuda.stream(torch.cuda.Stream())` and with no host synchronisation in between:
  1. the entry's input tensors hold SENTINEL bytes;
  2. a device-to-device copy of DELAY_BYTES is queued on the stream, which keeps it busy for longer than the host needs
     to issue everything that follows;
  3. the copies that put the real inputs in place are queued behind it;
  4. the entry is called;
then the stream is synchronised and the result must equal the host model bit for bit.  Work that did not wait for the
caller's stream read sentinels.  tests/test_host_model.py checks the same contract for EVERY entry against a model of
the runtime; this module is its anchor on the device.  A difference here is a finding to be read out of that model's log
on the CPU, not something to run again.

The entry is first run once in the ordinary way (null stream), which loads its kernels and grows the context's scratch
(not stream-ordered, by the header) and is checked against the same expectation."""
import numpy as np
import pytest

import vectors as V
from ct_model import bsgs_expect, rand_key, rand_slab, random_keys, random_plaintexts, rescale_expect
from ct_model_poly import poly_expect, poly_schedule
from gpu_support import (SENTINEL, assert_matches, dev_t, env, expectation, host_u32, ntt_secret, sentinel_out,  # noqa: F401
                         take)

pytestmark = pytest.mark.gpu

N, NP, B = 4096, 3, 3
# The delaying copy.  On an MI355X the host needs 0.038 ms (median of 20, largest 0.052 ms) to issue the longest entry
# here, ct_poly_sp of degree 3 (6 launches, 2 pitched copies); ten times that is 0.4 to 0.5 ms.  A device-to-device copy
# of 1 GiB takes 0.43 ms there, which is no margin, and one of 4 GiB takes 1.77 ms (LABNOTES Part E).  Each case checks
# the premise itself: the copy is still running when the entry has been issued.
DELAY_BYTES = 4 << 30


@pytest.fixture(scope="module")
def delay(env):
    torch = env["torch"]
    pair = [torch.zeros(DELAY_BYTES, dtype=torch.uint8, device=env["dev"]) for _ in range(2)]
    torch.cuda.synchronize()
    yield pair
    del pair[:]
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def case(env):
    """The 4096 x 3 context of the module: secret key, random digit Galois keys of 3 and 9, a random special-prime
    relinearisation key."""
    from oracle.pyoracle import Oracle
    o = Oracle(N, NP)
    ctx = env["pkg"].Context(N, NP)
    rng = np.random.default_rng(20261021)
    sk = V.secret_key(N, seed=5)
    ctx.set_secret_key(sk)
    keys = [3, 9]
    gk0, gk1 = random_keys(rng, o.q, len(keys), N, NP)
    ctx.set_galois_keys(keys, gk0, gk1)
    k0, k1 = rand_key(rng, o.q, N), rand_key(rng, o.q, N)
    ctx.set_relin_key_sp(k0, k1)
    yield dict(o=o, ctx=ctx, rng=rng, sk=sk, s_hat=ntt_secret(o, sk), keys=keys, key_of={3: 0, 9: 1}, gk=(gk0, gk1),
               relin_sp=(k0, k1))
    ctx.close()


def both_ways(env, delay, real, outs, call, check):
    """real: {name: host array}, the entry's inputs.  outs() -> fresh output tensors; call(ins, out) issues the entry on
    the current stream; check(out, what) compares with the expectation.  Once in the ordinary way, then behind the long
    copy on a stream of the caller's."""
    torch = env["torch"]
    staged = {k: dev_t(env, v) for k, v in real.items()}
    out = outs()
    call(staged, out)
    torch.cuda.synchronize()
    check(out, "null stream")

    ins = {k: torch.empty_like(t) for k, t in staged.items()}
    for t in ins.values():
        t.view(torch.uint8).fill_(SENTINEL & 0xFF)
    out = outs()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        delay[1].copy_(delay[0], non_blocking=True)
        copied = torch.cuda.Event()
        copied.record()
        for k, t in ins.items():
            t.copy_(staged[k], non_blocking=True)
        call(ins, out)
        behind = not copied.query()
    side.synchronize()
    assert behind, "the delaying copy had finished before the entry was issued: the case shows nothing (DELAY_BYTES)"
    check(out, "the caller's stream")


def pair_outs(env, shape):
    words = int(np.prod(shape))
    return lambda: dict(o0=sentinel_out(env, words, 2 * shape[-1]), o1=sentinel_out(env, words, 2 * shape[-1]))


def pair_check(shape, want0, want1):
    words = int(np.prod(shape))

    def check(out, what):
        assert (take(out["o0"], words, shape, what) == want0).all(), (what, "out0")
        assert (take(out["o1"], words, shape, what) == want1).all(), (what, "out1")
    return check


def test_ct_rescale_one_launch(env, delay, case):
    o, ctx = case["o"], case["ctx"]
    in0, in1 = rand_slab(case["rng"], o.q, B, N), rand_slab(case["rng"], o.q, B, N)
    shape = (B, NP - 1, N)
    both_ways(env, delay, dict(in0=in0, in1=in1), pair_outs(env, shape),
              lambda i, r: ctx.ct_rescale(i["in0"], r["o0"], i["in1"], r["o1"], primes=NP),
              pair_check(shape, rescale_expect(o, in0), rescale_expect(o, in1)))


def test_ct_drop_primes_the_pitched_copy(env, delay, case):
    o, ctx = case["o"], case["ctx"]
    in0, in1 = rand_slab(case["rng"], o.q, B, N), rand_slab(case["rng"], o.q, B, N)
    shape = (B, NP - 1, N)
    both_ways(env, delay, dict(in0=in0, in1=in1), pair_outs(env, shape),
              lambda i, r: ctx.ct_drop_primes(i["in0"], r["o0"], i["in1"], r["o1"], primes_in=NP, primes_out=NP - 1),
              pair_check(shape, in0[:, :NP - 1], in1[:, :NP - 1]))


def test_ct_bsgs_many_launches_and_a_workspace(env, delay, case):
    """A 2 x 2 plan with the identity in both lists: the chunk is copied into the workspace, then three launches."""
    o, ctx, rng = case["o"], case["ctx"], case["rng"]
    baby, giant = [1, 3], [1, 9]
    diag = random_plaintexts(rng, o.q, (2, 2), N)
    plan = ctx.bsgs_plan(baby, giant, dev_t(env, diag))
    c0, c1 = rand_slab(rng, o.q, B, N), rand_slab(rng, o.q, B, N)
    want = bsgs_expect(env["pkg"].galois_table, o, c0, c1, baby, giant, diag, case["key_of"], *case["gk"])
    shape = (B, NP, N)
    ws_bytes = ctx.bsgs_workspace_bytes(plan, B, NP)
    make = pair_outs(env, shape)
    both_ways(env, delay, dict(c0=c0, c1=c1), lambda: dict(make(), ws=sentinel_out(env, ws_bytes // 4, 2 * N)),
              lambda i, r: ctx.ct_bsgs(plan, i["c0"], i["c1"], r["o0"], r["o1"], r["ws"], primes=NP, workspace_bytes=ws_bytes),
              pair_check(shape, want[0], want[1]))
    plan.close()


def run_poly(env, delay, o, ctx, rng, keys, L, coeff, records):
    n = o.n
    scale_in, scale_out = float(o.q[L - 1]), 2.0 ** 25
    sched = poly_schedule(o.q, L, coeff, scale_in, scale_out)
    plan = env["pkg"].poly_create(n, len(o.q), L, coeff, scale_in, scale_out)
    c0, c1 = rand_slab(rng, o.q, records, n, L), rand_slab(rng, o.q, records, n, L)
    e0, e1, _ = poly_expect(o, c0, c1, sched, *keys)
    shape = (records, sched["out_primes"], n)
    need = plan.workspace_bytes(records)
    make = pair_outs(env, shape)
    both_ways(env, delay, dict(c0=c0, c1=c1),
              lambda: dict(make(), ws=sentinel_out(env, need // 4, 2 * n) if need else None),
              lambda i, r: ctx.ct_poly_sp(plan, i["c0"], i["c1"], r["o0"], r["o1"], r["ws"], workspace_bytes=need),
              pair_check(shape, e0, e1))
    plan.close()


def test_ct_poly_sp_a_plan_at_4096x3(env, delay, case):
    """4096 x 3 leaves the special-prime path two data primes, which a plan of degree 1 uses up: the combine alone."""
    run_poly(env, delay, case["o"], case["ctx"], case["rng"], case["relin_sp"], NP - 1, [0.25, -0.5], B)


def test_ct_poly_sp_a_plan_over_many_entries(env, delay):
    """The ladder needs more levels than 4096 x 3 has: degree 3 at 8192 x 6, level 5 -- the row pointers, two products
    with their rescales and dropped operands, the combine, all in the caller's workspace."""
    from oracle.pyoracle import Oracle
    n, npr = 8192, 6
    o = Oracle(n, npr)
    ctx = env["pkg"].Context(n, npr)
    rng = np.random.default_rng(109)
    keys = rand_key(rng, o.q, n), rand_key(rng, o.q, n)
    ctx.set_relin_key_sp(*keys)
    run_poly(env, delay, o, ctx, rng, keys, 5, [0.25, -0.5, 0.75, 1.0], 2)
    ctx.close()


def test_decrypt_full(env, delay, case):
    o, ctx = case["o"], case["ctx"]
    torch = env["torch"]
    vals = V.bench_values(B, N)
    ss, sd = V.bench_seeds(B)
    ok, c0, c1 = o.encrypt_sym_batch(vals, ss, sd, case["sk"])
    assert ok
    exp = [expectation(o, c0[b], c1[b], case["s_hat"]) for b in range(B)]

    def outs():
        return dict(pte=torch.full((B, N), -7, dtype=torch.int64, device=env["dev"]),
                    values=torch.full((B, N // 2), -7.0, dtype=torch.float32, device=env["dev"]),
                    values_f64=torch.full((B, N // 2), -7.0, dtype=torch.float64, device=env["dev"]),
                    status=torch.full((B,), 77, dtype=torch.uint8, device=env["dev"]))

    def check(out, what):
        for b in range(B):
            assert exp[b]["status"] == 1
            assert_matches(out, b, exp[b], (what, b))

    both_ways(env, delay, dict(c0=c0, c1=c1), outs, lambda i, r: ctx.decrypt_full(i["c0"], i["c1"], **r), check)


def test_encrypt_sym_fork_and_join_over_the_librarys_streams(env, delay, case):
    o, ctx = case["o"], case["ctx"]
    torch = env["torch"]
    vals = V.bench_values(B, N, first=7)
    ss, sd = V.bench_seeds(B, first=7)
    ok, e0, e1 = o.encrypt_sym_batch(vals, ss, sd, case["sk"])
    assert ok
    words = B * NP * N

    def outs():
        return dict(c0=sentinel_out(env, words, 2 * N), c1=sentinel_out(env, words, 2 * N),
                    status=torch.full((B,), 77, dtype=torch.uint8, device=env["dev"]))

    def check(out, what):
        assert (take(out["c0"], words, (B, NP, N), what) == e0).all(), (what, "c0")
        assert (take(out["c1"], words, (B, NP, N), what) == e1).all(), (what, "c1")
        assert (out["status"].cpu().numpy() == 1).all(), (what, "status")

    both_ways(env, delay, dict(values=vals, share=ss, seeds=sd), outs,
              lambda i, r: ctx.encrypt_sym(i["values"], i["share"], i["seeds"], r["c0"], r["c1"], status=r["status"]), check)
