#!/usr/bin/env python3
"""Time of se_amd_ct_rescale_device and se_amd_ct_mul_plain_device on resident slabs, HIP events, one process:
  rescale    both slabs, level L -> L - 1, against the summed time of the stage operators that run the same transforms
             alone: se_amd_intt_device on 2B rows (the last-prime rows) + se_amd_ntt_device on 2B(L-1) rows (prime 0's
             tables; every prime of a chain costs the same).  The stage operators work in place on rows of their own, so
             the sum counts their HBM round trips and none of the subtract / multiply the fused kernel adds.
  mul_plain  both slabs times one plaintext per record (P = B), against a device-to-device copy of ONE slab.
The two sides of a pair alternate inside one loop.  Prints one JSON line; --out also writes it to a file.
  python tools/rescale_bench.py [--n 4096 --primes 3 --batch 65536 --reps 50 --warmup 5 --out FILE]"""
import argparse
import sys

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=3)
ap.add_argument("--batch", type=int, default=65536)
bs.add_common_args(ap, reps=50, warmup=5)
args = ap.parse_args()

pkg, torch, dev = bs.start("rescale_bench")
n, L, B = args.n, args.primes, args.batch
if L < 2:
    sys.exit("the rescale needs at least two primes")
row_bytes = L * n * 4
ctx = pkg.Context(n, L)                         # no key: neither entry needs one
q = ctx.moduli()
gen = torch.Generator(device=dev)
gen.manual_seed(1)
c0 = bs.slab(q, (B, L, n), dev, gen)
c1 = bs.slab(q, (B, L, n), dev, gen)


def timed(fns):
    """The lists of milliseconds, one per function; the clock is not sampled."""
    return bs.timed(fns, max(args.reps, 20), args.warmup, clock=False)[0]


def report(ms, nbytes):
    return bs.record(ms, bytes=nbytes, tb_per_s=bs.tb_per_s(nbytes, ms))


result = dict(tool="rescale_bench", n=n, primes=L, B=B, device=torch.cuda.get_device_name(0))

# ---- rescale against the stage operators
r0 = torch.empty((B, L - 1, n), dtype=torch.int32, device=dev)
r1 = torch.empty_like(r0)
last = bs.slab(q, (2 * B, n), dev, gen)
lower = bs.slab(q, (2 * B * (L - 1), n), dev, gen)
fused, intt, ntt = timed([lambda: ctx.ct_rescale(c0, r0, c1, r1),
                          lambda: ctx.intt(L - 1, last),
                          lambda: ctx.ntt(0, lower)])
# algorithmic bytes: every input row read once, every output row written once
result["rescale"] = report(fused, 2 * B * (L + L - 1) * n * 4)
result["intt_2B_rows"] = report(intt, 2 * 2 * B * n * 4)
result["ntt_2B_Lm1_rows"] = report(ntt, 2 * 2 * B * (L - 1) * n * 4)
stage_sum = result["intt_2B_rows"]["ms"] + result["ntt_2B_Lm1_rows"]["ms"]
result["stage_sum_ms"] = round(stage_sum, 4)
result["rescale_over_stage_sum"] = round(result["rescale"]["ms"] / stage_sum, 3)
del r0, r1, last, lower

# ---- plaintext product against a copy of one slab
pt = bs.slab(q, (B, L, n), dev, gen)
o0 = torch.empty_like(c0)
o1 = torch.empty_like(c0)
st = torch.zeros(B, dtype=torch.uint8, device=dev)
mul, copy = timed([lambda: ctx.ct_mul_plain(c0, pt, o0, c1, o1, status=st), lambda: o0.copy_(c0)])
assert bool((st == 1).all())
result["mul_plain"] = report(mul, 5 * B * row_bytes)        # two slabs and the plaintexts read, two slabs written
result["copy_one_slab"] = report(copy, 2 * B * row_bytes)
result["mul_plain_over_copy_ms"] = round(result["mul_plain"]["ms"] / result["copy_one_slab"]["ms"], 3)
result["mul_plain_rate_over_copy_rate"] = round(result["mul_plain"]["tb_per_s"] / result["copy_one_slab"]["tb_per_s"], 3)

ctx.close()
bs.emit(result, args.out)
