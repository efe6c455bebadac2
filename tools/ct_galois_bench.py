#!/usr/bin/env python3
"""Time of se_amd_ct_galois_device on resident slabs against se_amd_ct_relin_device on the same rows of the same build,
HIP events, one process, the two sides alternating inside one loop.
  galois  (c0, c1) -> (out0, out1) at level L: L INTTs and 2 L NTTs per output prime, one LDS scatter per input prime
          and one LDS gather per output prime for the automorphism; two slabs read, two written.
  relin   (d0, d1, d2) -> (out0, out1) with d0 = c0, d1 = 0-filled, d2 = c1 and the same key words installed as the
          relinearisation key: the identical transform count and multiply-accumulate, one slab more read, no
          automorphism.  It is the yardstick the tree already has (tools/ct_mul_bench.py times it against the stage
          operators).
The engine clock is sampled (bench.ClockSampler) while the loop runs.  Prints one JSON line; --out also writes it.
  python tools/ct_galois_bench.py [--n 4096 --primes 3 --batch 65536 --step 1 --reps 20 --warmup 3 --out FILE]"""
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
ap.add_argument("--step", type=int, default=1)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()

import numpy as np
import torch

import __graft_entry__ as ge
from bench import ClockSampler

if not torch.cuda.is_available():
    sys.exit("ct_galois_bench needs a GPU")
pkg = ge.load_package()
dev = torch.device("cuda:0")
n, L, B = args.n, args.primes, args.batch
slab_bytes = B * L * n * 4
ctx = pkg.Context(n, L)                         # no secret key: neither entry needs one
q = ctx.moduli()
qmin = min(q)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
c0 = torch.randint(0, qmin, (B, L, n), dtype=torch.int32, device=dev, generator=gen)
c1 = torch.randint(0, qmin, (B, L, n), dtype=torch.int32, device=dev, generator=gen)
zero = torch.zeros_like(c0)
g0, g1, r0, r1 = (torch.empty_like(c0) for _ in range(4))
rng = np.random.default_rng(2)
key = [np.stack([rng.integers(0, q[i], (2 * L, n), dtype=np.uint32) for i in range(L)], axis=1) for _ in range(2)]
elt = pkg.galois_element(n, args.step)
ctx.set_relin_key(*key)
ctx.set_galois_keys([elt], key[0][None], key[1][None])

fns = [lambda: ctx.ct_galois(c0, c1, elt, g0, g1), lambda: ctx.ct_relin(c0, zero, c1, r0, r1)]
for _ in range(args.warmup):
    for fn in fns:
        fn()
torch.cuda.synchronize()
ms = [[] for _ in fns]
with ClockSampler(torch, 0) as cs:
    for _ in range(max(args.reps, 10)):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))


def report(v, nbytes):
    med = statistics.median(v)
    return dict(ms=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), reps=len(v), bytes=nbytes,
                records_per_s=round(B / med * 1e3))


result = dict(tool="ct_galois_bench", n=n, primes=L, B=B, step=args.step, element=elt,
              device=torch.cuda.get_device_name(0))
result["galois"] = report(ms[0], 4 * slab_bytes)
result["relin"] = report(ms[1], 5 * slab_bytes)
result["galois_over_relin_ms"] = round(result["galois"]["ms"] / result["relin"]["ms"], 3)
result["clock"] = cs.summary()
ctx.close()
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
