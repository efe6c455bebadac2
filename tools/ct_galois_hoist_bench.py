#!/usr/bin/env python3
"""Time of the hoisted rotations (se_amd_ct_galois_many_device, se_amd_ct_galois_sum_device) on resident slabs against
the calls of the same build they replace, HIP events, one process, the contenders of a form alternating inside one loop.
  many form, G = 8 (steps 1 .. 8), B = --batch-many records:
    many      one se_amd_ct_galois_many_device call: ceil(8 / 2) = 4 times the transforms of one rotation
    singles   eight se_amd_ct_galois_device calls on the same rows into the same [8][B] outputs
  sum form, the sum of 8 (the record and its rotations by 1 .. 7), B = --batch records:
    sum       one se_amd_ct_galois_sum_device call with G = 7 and add_input: the transforms of one rotation
    rounds    the three rotate-and-add rounds that compute the same sum today: se_amd_ct_galois_device (steps 1, 2, 4)
              into the second half of a 2B-record slab, then se_amd_ct_lincomb_device over the rows {b, B + b}
    singles   seven se_amd_ct_galois_device calls (steps 1 .. 7) without the adds that would follow them
Random residues and random key words below every prime: no entry needs a secret key, and none of them branches on data.
The engine clock is sampled (bench.ClockSampler) while each loop runs.  Prints one JSON line; --out also writes it.
  python tools/ct_galois_hoist_bench.py [--n 4096 --primes 3 --batch 65536 --batch-many 16384 --reps 20 --warmup 3
                                         --out FILE]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=3)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--batch-many", type=int, default=16384)
bs.add_common_args(ap, reps=20, warmup=3)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_galois_hoist_bench")
n, L, B, Bm = args.n, args.primes, args.batch, args.batch_many
G_MANY, WINDOW = 8, 8
ctx = pkg.Context(n, L)                         # no secret key: no entry here needs one
q = ctx.moduli()
gen = torch.Generator(device=dev)
gen.manual_seed(1)
rng = np.random.default_rng(2)
steps = list(range(1, G_MANY + 1))
elts = [pkg.galois_element(n, s) for s in steps]
keys = [np.stack([bs.key_words(rng, q, 2 * L, n, L) for _ in elts]) for _ in range(2)]
ctx.set_galois_keys(elts, *keys)


def report(v, records):
    return bs.record(v, records_per_s=bs.per_s(records, v))


result = dict(tool="ct_galois_hoist_bench", n=n, primes=L, device=torch.cuda.get_device_name(0))

# ---- many form ----
c0 = bs.slab(q, (Bm, L, n), dev, gen)
c1 = bs.slab(q, (Bm, L, n), dev, gen)
m0, m1 = (torch.empty((G_MANY, Bm, L, n), dtype=torch.int32, device=dev) for _ in range(2))


def many_singles():
    for e, g in enumerate(elts):
        ctx.ct_galois(c0, c1, g, m0[e], m1[e])


ms, clock = bs.timed([lambda: ctx.ct_galois_many(c0, c1, elts, m0, m1), many_singles], max(args.reps, 10), args.warmup)
result["many"] = dict(B=Bm, G=G_MANY, steps=steps, many=report(ms[0], Bm), singles=report(ms[1], Bm), clock=clock)
result["many"]["many_over_singles_ms"] = round(result["many"]["many"]["ms"] / result["many"]["singles"]["ms"], 3)
del c0, c1, m0, m1
torch.cuda.empty_cache()

# ---- sum form ----
cur0, cur1, nxt0, nxt1 = (torch.empty((2 * B, L, n), dtype=torch.int32, device=dev) for _ in range(4))
for t in (cur0, cur1):
    t[:B] = bs.slab(q, (B, L, n), dev, gen)
s0, s1 = (torch.empty((B, L, n), dtype=torch.int32, device=dev) for _ in range(2))
row_ptr = torch.arange(0, 2 * B + 1, 2, dtype=torch.int32, device=dev)
idx = torch.stack([torch.arange(B, dtype=torch.int32, device=dev), torch.arange(B, 2 * B, dtype=torch.int32, device=dev)],
                  dim=1).reshape(-1).contiguous()
window = elts[:WINDOW - 1]
round_elts = [pkg.galois_element(n, s) for s in (1, 2, 4)]


def rounds():
    a0, a1, b0, b1 = cur0, cur1, nxt0, nxt1
    for g in round_elts:
        ctx.ct_galois(a0[:B], a1[:B], g, a0[B:], a1[B:])
        ctx.ct_lincomb(a0, b0[:B], a1, b1[:B], row_ptr=row_ptr, idx=idx)
        a0, a1, b0, b1 = b0, b1, a0, a1


def sum_singles():
    for g in window:
        ctx.ct_galois(cur0[:B], cur1[:B], g, s0, s1)


ms, clock = bs.timed([lambda: ctx.ct_galois_sum(cur0[:B], cur1[:B], window, s0, s1, add_input=True), rounds,
                      sum_singles], max(args.reps, 10), args.warmup)
result["sum"] = dict(B=B, G=WINDOW - 1, add_input=True, sum=report(ms[0], B), rounds=report(ms[1], B),
                     singles=report(ms[2], B), clock=clock)
result["sum"]["sum_over_rounds_ms"] = round(result["sum"]["sum"]["ms"] / result["sum"]["rounds"]["ms"], 3)
result["sum"]["sum_over_singles_ms"] = round(result["sum"]["sum"]["ms"] / result["sum"]["singles"]["ms"], 3)
ctx.close()
bs.emit(result, args.out)
