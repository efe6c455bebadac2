#!/usr/bin/env python3
"""Time of a linear transform (se_amd_ct_lintrans_device: the plaintext-weighted sum of a record and its hoisted
rotations, the diagonal method) on resident slabs against the calls of the same build it stands beside, HIP events, one
process, the contenders alternating inside one loop.  G = 7 (steps 1 .. 7) plus diag0, B = --batch records:
    plan         one se_amd_ct_lintrans_device call on a plan with the diagonals folded into the keys
    sum          one se_amd_ct_galois_sum_device call with the same G and add_input: the same pass WITHOUT weights, so
                 plan / sum is what the weighted epilogue and the second set of key blocks cost
    composition  what computes the same record without the entry: one se_amd_ct_galois_many_device call into [7][B]
                 rows, eight se_amd_ct_mul_plain_device calls (in place; diag0 on the input into an eighth block of
                 rows) and one se_amd_ct_lincomb_device call over the rows {b, B + b, .., 7 B + b}
Before anything is timed the plan's output is compared with the composition's, bit for bit.  The plan creation (fold
kernels and the synchronisation) is timed with the host clock.  Random residues, key words and diagonal words below
every prime: no entry needs a secret key, and none of them branches on data.  The engine clock is sampled
(bench.ClockSampler) while the loop runs.  Prints one JSON line; --out also writes it.
  python tools/ct_lintrans_bench.py [--n 4096 --primes 3 --batch 16384 --reps 20 --warmup 3 --out FILE]"""
import argparse
import statistics
import sys
import time

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=3)
ap.add_argument("--batch", type=int, default=16384)
bs.add_common_args(ap, reps=20, warmup=3)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_lintrans_bench")
n, L, B = args.n, args.primes, args.batch
G = 7
ctx = pkg.Context(n, L)                         # no secret key: no entry here needs one
q = ctx.moduli()
gen = torch.Generator(device=dev)
gen.manual_seed(1)
rng = np.random.default_rng(2)
steps = list(range(1, G + 1))
elts = [pkg.galois_element(n, s) for s in steps]
keys = [np.stack([bs.key_words(rng, q, 2 * L, n, L) for _ in elts]) for _ in range(2)]
ctx.set_galois_keys(elts, *keys)
diag = bs.slab(q, (G + 1, L, n), dev, gen)      # [0] is diag0
c0 = bs.slab(q, (B, L, n), dev, gen)
c1 = bs.slab(q, (B, L, n), dev, gen)
p0, p1, s0, s1, k0, k1 = (torch.empty((B, L, n), dtype=torch.int32, device=dev) for _ in range(6))
m0, m1 = (torch.empty((G + 1, B, L, n), dtype=torch.int32, device=dev) for _ in range(2))
row_ptr = torch.arange(0, (G + 1) * B + 1, G + 1, dtype=torch.int32, device=dev)
idx = (torch.arange(G + 1, dtype=torch.int32, device=dev)[None, :] * B
       + torch.arange(B, dtype=torch.int32, device=dev)[:, None]).reshape(-1).contiguous()

create_ms = []
plan = None
for _ in range(5):
    if plan is not None:
        plan.close()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = ctx.lintrans_plan(elts, diag[1:], diag[0])
    create_ms.append((time.perf_counter() - t0) * 1e3)


def composition():
    ctx.ct_galois_many(c0, c1, elts, m0, m1)
    for e in range(G):
        ctx.ct_mul_plain(m0[e], diag[e + 1:e + 2], m0[e], m1[e], m1[e])
    ctx.ct_mul_plain(c0, diag[0:1], m0[G], c1, m1[G])
    ctx.ct_lincomb(m0.view((G + 1) * B, L, n), k0, m1.view((G + 1) * B, L, n), k1, row_ptr=row_ptr, idx=idx)


ctx.ct_lintrans(plan, c0, c1, p0, p1)
composition()
torch.cuda.synchronize()
if not (torch.equal(p0, k0) and torch.equal(p1, k1)):
    sys.exit("ct_lintrans_bench: the plan call and the composition differ")


def report(v):
    return bs.record(v, records_per_s=bs.per_s(B, v))


ms, clock = bs.timed([lambda: ctx.ct_lintrans(plan, c0, c1, p0, p1),
                      lambda: ctx.ct_galois_sum(c0, c1, elts, s0, s1, add_input=True), composition],
                     max(args.reps, 10), args.warmup)
result = dict(tool="ct_lintrans_bench", n=n, primes=L, device=torch.cuda.get_device_name(0), B=B, G=G, diag0=True,
              steps=steps, outputs_equal=True, plan=report(ms[0]), sum=report(ms[1]),
              composition=report(ms[2]), clock=clock,
              plan_create_ms=dict(median=round(statistics.median(create_ms), 3), min=round(min(create_ms), 3),
                                  max=round(max(create_ms), 3), reps=len(create_ms)),
              plan_bytes=(G * 16 * 2 * L * L + (G + 1) * 8 * L) * n)
result["plan_over_sum_ms"] = round(result["plan"]["ms"] / result["sum"]["ms"], 3)
result["plan_over_composition_ms"] = round(result["plan"]["ms"] / result["composition"]["ms"], 3)
plan.close()
ctx.close()
bs.emit(result, args.out)
