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
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=3)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()

import numpy as np
import torch

import __graft_entry__ as ge

if not torch.cuda.is_available():
    sys.exit("ct_mul_bench needs a GPU")
pkg = ge.load_package()
dev = torch.device("cuda:0")
n, L, B = args.n, args.primes, args.batch
slab_words = B * L * n
slab_bytes = slab_words * 4
ctx = pkg.Context(n, L)                         # no secret key: neither entry needs one
q = ctx.moduli()
qmin = min(q)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
c0 = torch.randint(0, qmin, (B, L, n), dtype=torch.int32, device=dev, generator=gen)
c1 = torch.randint(0, qmin, (B, L, n), dtype=torch.int32, device=dev, generator=gen)


def timed(fns):
    """Median-ready lists of milliseconds, one per function; the functions alternate inside every repetition."""
    for _ in range(args.warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(max(args.reps, 10)):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def report(ms, nbytes):
    med = statistics.median(ms)
    return dict(ms=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), reps=len(ms), bytes=nbytes,
                tb_per_s=round(nbytes / med / 1e9, 3))


result = dict(tool="ct_mul_bench", n=n, primes=L, B=B, device=torch.cuda.get_device_name(0))

# ---- tensor against a copy of the same bytes
t0, t1, t2 = (torch.empty_like(c0) for _ in range(3))
st = torch.zeros(B, dtype=torch.uint8, device=dev)
half = (7 * slab_words) // 2
src = torch.randint(0, qmin, (half,), dtype=torch.int32, device=dev, generator=gen)
dst = torch.empty_like(src)
mul, copy = timed([lambda: ctx.ct_mul(c0, c1, c0, c1, t0, t1, t2, status=st), lambda: dst.copy_(src)])
assert bool((st == 1).all())
result["tensor"] = report(mul, 7 * slab_bytes)
result["copy_same_bytes"] = report(copy, 2 * half * 4)
result["tensor_over_copy_ms"] = round(result["tensor"]["ms"] / result["copy_same_bytes"]["ms"], 3)
del src, dst

# ---- relin against the stage operators it replaces
rng = np.random.default_rng(2)
key = [np.stack([rng.integers(0, q[i], (2 * L, n), dtype=np.uint32) for i in range(L)], axis=1) for _ in range(2)]
ctx.set_relin_key(*key)
m0, m1 = torch.empty_like(c0), torch.empty_like(c0)
rows = torch.randint(0, qmin, (B, n), dtype=torch.int32, device=dev, generator=gen)


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
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
