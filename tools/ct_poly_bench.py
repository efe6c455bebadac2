#!/usr/bin/env python3
"""Time of the last step of a slot-wise polynomial on resident records, HIP events, one process, the sides alternating
inside one loop (the protocol of tools/ct_pack_bench.py):
  affine T  (1) ONE se_amd_ct_affine_rescale_device call over T term records at mixed levels (every third term at the
            call's level, the others one level up), against
            (2) the composition it replaces: T se_amd_ct_drop_primes_device calls into a stack at the call's level, the
            se_amd_ct_lincomb_device sum of every record's T entries on a context of that many primes, and
            se_amd_ct_rescale_device.  Weights fit int32 so that (2) can hold them; the constant is left out of both.
  Shapes: 4096 x 3, primes = 2, 65 536 records; 16384 x 13, primes = 12, 2 048 records; T = 4 and 15.
  Device memory beside the terms and the result: (1) none, (2) the dropped terms and the sum, 2 (T + 1) B rows of
  primes . n words.
  plan      the whole degree-7 odd plan (the logistic polynomial) at 8192 x 6, L = 5: ONE se_amd_ct_poly_sp_device call, five
            products and the combine, in the caller's workspace.
The ratio is reported, not required: by rows moved (1) reads the terms once and writes the result, (2) also writes and
re-reads every dropped term and the sum.  Slabs and key words are random residues (no secret key: no entry needs one).
The engine clock is sampled (bench.ClockSampler) while the loops run.  Prints one JSON line; --out also writes it.
  python tools/ct_poly_bench.py [--reps 20 --warmup 2 --small --out profiles/ct_poly_bench.json]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true", help="1/16 of the records of every shape (a quick look)")
bs.add_common_args(ap, reps=20, warmup=2)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_poly_bench")
SHAPES = [(4096, 3, 2, 65536, (4, 15)), (16384, 13, 12, 2048, (4, 15))]      # n, np, primes, records, term counts
PLAN = (8192, 6, 5, 4096)                                                     # n, np, L, records
LOGISTIC7 = [0.5, 0.25, 0.0, -1.0 / 48, 0.0, 1.0 / 480, 0.0, -17.0 / 80640]


def timed(fns, reps, warmup, B):
    """bs.timed with every list of milliseconds made a record."""
    ms, clock = bs.timed(fns, reps, warmup)
    return [bs.record(v, records_per_s=bs.per_s(B, v)) for v in ms], clock


result = dict(tool="ct_poly_bench", device=torch.cuda.get_device_name(0), cases=[])
gen = torch.Generator(device=dev)
gen.manual_seed(7)
for N, NP, P, B, counts in SHAPES:
    if args.small:
        B //= 16
    ctx = pkg.Context(N, NP)
    low = pkg.Context(N, P)                                    # ct_lincomb on level-P records: rows of P n words
    q = ctx.moduli()
    assert low.moduli() == q[:P]
    slab = lambda rows: bs.slab(q, (B, rows, N), dev, gen)  # noqa: E731
    for T in counts:
        levels = [P if t % 3 == 0 else min(P + 1, NP) for t in range(T)]
        terms0, terms1 = [slab(lv) for lv in levels], [slab(lv) for lv in levels]
        w = [int(x) for x in np.random.default_rng(T).integers(-2 ** 31, 2 ** 31, T)]
        g0, g1, h0, h1 = (torch.empty((B, P - 1, N), dtype=torch.int32, device=dev) for _ in range(4))
        stack0, stack1 = (torch.empty((T * B, P, N), dtype=torch.int32, device=dev) for _ in range(2))
        sum0, sum1 = (torch.empty((B, P, N), dtype=torch.int32, device=dev) for _ in range(2))
        ptr = (torch.arange(B + 1, dtype=torch.int64, device=dev) * T).to(torch.int32)
        e = torch.arange(T * B, dtype=torch.int64, device=dev)
        idx = ((e % T) * B + e // T).to(torch.int32)
        wd = torch.tensor(w * B, dtype=torch.int32, device=dev)

        def affine_call():
            ctx.ct_affine_rescale(terms0, terms1, w, 0, g0, g1, P)

        def composition():
            for t in range(T):
                ctx.ct_drop_primes(terms0[t], stack0[t * B:(t + 1) * B], terms1[t], stack1[t * B:(t + 1) * B],
                                   primes_in=levels[t], primes_out=P)
            low.ct_lincomb(stack0, sum0, stack1, sum1, row_ptr=ptr, idx=idx, w=wd)
            ctx.ct_rescale(sum0, h0, sum1, h1, primes=P)

        (t_aff, t_comp), clock = timed([affine_call, composition], max(args.reps, 5), args.warmup, B)
        rows_in = 2 * B * P * T
        result["cases"].append(dict(
            n=N, primes=NP, level=P, B=B, T=T, term_levels=levels, affine=t_aff, drops_lincomb_rescale=t_comp,
            affine_over_composition_ms=round(t_aff["ms"] / t_comp["ms"], 3),
            rows_moved=dict(affine=rows_in + 2 * B * (P - 1), composition=3 * rows_in + 2 * 2 * B * P + 2 * B * (P - 1)),
            extra_device_bytes=dict(affine=0, composition=2 * (T + 1) * B * P * N * 4),
            equal_bits=bool((g0 == h0).all()) and bool((g1 == h1).all()), clock=clock))
        del terms0, terms1, g0, g1, h0, h1, stack0, stack1, sum0, sum1
        torch.cuda.empty_cache()
    ctx.close()
    low.close()

N, NP, L, B = PLAN
if args.small:
    B //= 16
ctx = pkg.Context(N, NP)
q = ctx.moduli()
rng = np.random.default_rng(13)
ctx.set_relin_key_sp(bs.key_words(rng, q, NP - 1, N, NP), bs.key_words(rng, q, NP - 1, N, NP))
plan = pkg.poly_create(N, NP, L, LOGISTIC7, float(q[L - 1]), ctx.scale())
c0 = bs.slab(q, (B, L, N), dev, gen)
c1 = bs.slab(q, (B, L, N), dev, gen)
out_primes = plan.result()[0]
o0, o1 = (torch.empty((B, out_primes, N), dtype=torch.int32, device=dev) for _ in range(2))
work = torch.empty((plan.workspace_bytes(B) // 4,), dtype=torch.int32, device=dev)
(t_plan,), clock = timed([lambda: ctx.ct_poly_sp(plan, c0, c1, o0, o1, work)], max(args.reps, 5), args.warmup, B)
result["plan"] = dict(n=N, primes=NP, level=L, B=B, degree=7, powers=[t["power"] for t in plan.terms()],
                      out_primes=out_primes, workspace_bytes=plan.workspace_bytes(B), poly_sp=t_plan, clock=clock)
plan.close()
ctx.close()

bs.emit(result, args.out)
