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
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=3)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()

import numpy as np
import torch

import __graft_entry__ as ge
from bench import ClockSampler

if not torch.cuda.is_available():
    sys.exit("ct_lintrans_bench needs a GPU")
pkg = ge.load_package()
dev = torch.device("cuda:0")
n, L, B = args.n, args.primes, args.batch
G = 7
ctx = pkg.Context(n, L)                         # no secret key: no entry here needs one
q = ctx.moduli()
qmin = min(q)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
rng = np.random.default_rng(2)
steps = list(range(1, G + 1))
elts = [pkg.galois_element(n, s) for s in steps]
keys = [np.stack([np.stack([rng.integers(0, q[i], (2 * L, n), dtype=np.uint32) for i in range(L)], axis=1)
                  for _ in elts]) for _ in range(2)]
ctx.set_galois_keys(elts, *keys)
diag = torch.randint(0, qmin, (G + 1, L, n), dtype=torch.int32, device=dev, generator=gen)   # [0] is diag0
c0 = torch.randint(0, qmin, (B, L, n), dtype=torch.int32, device=dev, generator=gen)
c1 = torch.randint(0, qmin, (B, L, n), dtype=torch.int32, device=dev, generator=gen)
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


def timed(fns, reps, warmup):
    """The contenders alternate inside one loop; -> per contender the list of milliseconds, and the clock summary."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    with ClockSampler(torch, 0) as cs:
        for _ in range(max(reps, 10)):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
    return ms, cs.summary()


def report(v, records):
    med = statistics.median(v)
    return dict(ms=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), reps=len(v),
                records_per_s=round(records / med * 1e3))


ms, clock = timed([lambda: ctx.ct_lintrans(plan, c0, c1, p0, p1),
                   lambda: ctx.ct_galois_sum(c0, c1, elts, s0, s1, add_input=True), composition], args.reps, args.warmup)
result = dict(tool="ct_lintrans_bench", n=n, primes=L, device=torch.cuda.get_device_name(0), B=B, G=G, diag0=True,
              steps=steps, outputs_equal=True, plan=report(ms[0], B), sum=report(ms[1], B),
              composition=report(ms[2], B), clock=clock,
              plan_create_ms=dict(median=round(statistics.median(create_ms), 3), min=round(min(create_ms), 3),
                                  max=round(max(create_ms), 3), reps=len(create_ms)),
              plan_bytes=(G * 16 * 2 * L * L + (G + 1) * 8 * L) * n)
result["plan_over_sum_ms"] = round(result["plan"]["ms"] / result["sum"]["ms"], 3)
result["plan_over_composition_ms"] = round(result["plan"]["ms"] / result["composition"]["ms"], 3)
plan.close()
ctx.close()
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
