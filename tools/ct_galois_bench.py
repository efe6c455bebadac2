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

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=3)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--step", type=int, default=1)
bs.add_common_args(ap, reps=20, warmup=3)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_galois_bench")
n, L, B = args.n, args.primes, args.batch
slab_bytes = B * L * n * 4
ctx = pkg.Context(n, L)                         # no secret key: neither entry needs one
q = ctx.moduli()
gen = torch.Generator(device=dev)
gen.manual_seed(1)
c0 = bs.slab(q, (B, L, n), dev, gen)
c1 = bs.slab(q, (B, L, n), dev, gen)
zero = torch.zeros_like(c0)
g0, g1, r0, r1 = (torch.empty_like(c0) for _ in range(4))
rng = np.random.default_rng(2)
key = [bs.key_words(rng, q, 2 * L, n, L) for _ in range(2)]
elt = pkg.galois_element(n, args.step)
ctx.set_relin_key(*key)
ctx.set_galois_keys([elt], key[0][None], key[1][None])

ms, clock = bs.timed([lambda: ctx.ct_galois(c0, c1, elt, g0, g1), lambda: ctx.ct_relin(c0, zero, c1, r0, r1)],
                     max(args.reps, 10), args.warmup)


def report(v, nbytes):
    return bs.record(v, bytes=nbytes, records_per_s=bs.per_s(B, v))


result = dict(tool="ct_galois_bench", n=n, primes=L, B=B, step=args.step, element=elt,
              device=torch.cuda.get_device_name(0))
result["galois"] = report(ms[0], 4 * slab_bytes)
result["relin"] = report(ms[1], 5 * slab_bytes)
result["galois_over_relin_ms"] = round(result["galois"]["ms"] / result["relin"]["ms"], 3)
result["clock"] = clock
ctx.close()
bs.emit(result, args.out)
