#!/usr/bin/env python3
"""Time of se_amd_ct_mul_device and se_amd_ct_relin_device on resident slabs, HIP events, one process:
  tensor  squares of B records (a = b, identity pairs): 4 slab reads + 3 slab writes, against a device-to-device copy
          that moves the same 7 slabs of bytes (3.5 read, 3.5 written).
  relin   (d0, d1, d2) -> (out0, out1) at level L, against the summed time of the stage operators it replaces, run on
          the same number of rows: L calls of se_amd_intt_device on B rows plus 2 L^2 calls of se_amd_ntt_device on B
          rows (prime 0's tables; every prime of a chain costs the same).  The stage operators work in place on rows of
          their own, so the sum counts their HBM round trips and none of the multiply-accumulate the fused kernel adds.
The two sides of a pair alternate inside one loop.  Prints one JSON line; --out also writes it to a file.
  python tools/ct_mul_bench.py [--n 4096 --primes 3 --batch 65536 --reps 20 --warmup 3 --out FILE]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=3)
ap.add_argument("--batch", type=int, default=65536)
bs.add_common_args(ap, reps=20, warmup=3)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_mul_bench")
n, L, B = args.n, args.primes, args.batch
slab_words = B * L * n
slab_bytes = slab_words * 4
ctx = pkg.Context(n, L)                         # no secret key: neither entry needs one
q = ctx.moduli()
gen = torch.Generator(device=dev)
gen.manual_seed(1)
c0 = bs.slab(q, (B, L, n), dev, gen)
c1 = bs.slab(q, (B, L, n), dev, gen)


def timed(fns):
    """The lists of milliseconds, one per function; the clock is not sampled."""
    return bs.timed(fns, max(args.reps, 10), args.warmup, clock=False)[0]


def report(ms, nbytes):
    return bs.record(ms, bytes=nbytes, tb_per_s=bs.tb_per_s(nbytes, ms))


result = dict(tool="ct_mul_bench", n=n, primes=L, B=B, device=torch.cuda.get_device_name(0))

# ---- tensor against a copy of the same bytes
t0, t1, t2 = (torch.empty_like(c0) for _ in range(3))
st = torch.zeros(B, dtype=torch.uint8, device=dev)
half = (7 * slab_words) // 2
src = bs.slab(q, (half,), dev, gen)
dst = torch.empty_like(src)
mul, copy = timed([lambda: ctx.ct_mul(c0, c1, c0, c1, t0, t1, t2, status=st), lambda: dst.copy_(src)])
assert bool((st == 1).all())
result["tensor"] = report(mul, 7 * slab_bytes)
result["copy_same_bytes"] = report(copy, 2 * half * 4)
result["tensor_over_copy_ms"] = round(result["tensor"]["ms"] / result["copy_same_bytes"]["ms"], 3)
del src, dst

# ---- relin against the stage operators it replaces
rng = np.random.default_rng(2)
key = [bs.key_words(rng, q, 2 * L, n, L) for _ in range(2)]
ctx.set_relin_key(*key)
m0, m1 = torch.empty_like(c0), torch.empty_like(c0)
rows = bs.slab(q, (B, n), dev, gen)


def stage_ops():
    for j in range(L):
        ctx.intt(j, rows)
    for _ in range(2 * L * L):
        ctx.ntt(0, rows)


fused, stages = timed([lambda: ctx.ct_relin(t0, t1, t2, m0, m1), stage_ops])
# algorithmic bytes of the fused entry: three slabs read, two written (the key is cache-resident)
result["relin"] = report(fused, 5 * slab_bytes)
result["stage_ops"] = report(stages, (L + 2 * L * L) * 2 * B * n * 4)
result["stage_ops"]["calls"] = dict(intt=L, ntt=2 * L * L, rows_per_call=B)
result["relin_over_stage_ops_ms"] = round(result["relin"]["ms"] / result["stage_ops"]["ms"], 3)

ctx.close()
bs.emit(result, args.out)
