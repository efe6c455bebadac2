#!/usr/bin/env python3
"""Byte rate of se_amd_ct_lincomb_device against a device-to-device copy, resident slabs, HIP events, one process:
  copy  one B-record slab copied to another (read + write bytes)
  a     G = 1, unit weights: the whole batch summed into one record
  b     G = B / 256 groups of 256 records (CSR, shuffled members), random int32 weights
  c     dense G = 16 weight rows over the first 4 096 records
Both slabs (c0, c1) in every call.  Algorithmic bytes = inputs read once per use + outputs written.  Prints one JSON
line; --out also writes it to a file.
  python tools/lincomb_bench.py [--n 4096 --primes 3 --batch 65536 --reps 50 --warmup 5 --split 0 --out FILE]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=3)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--split", type=int, default=0, help="se_amd_set_lincomb_split (0 = automatic)")
ap.add_argument("--only", default="", help="comma list of a,b,c (default all); the copy always runs")
bs.add_common_args(ap, reps=50, warmup=5)
args = ap.parse_args()

pkg, torch, dev = bs.start("lincomb_bench")
n, npr, B = args.n, args.primes, args.batch
row_bytes = npr * n * 4
ctx = pkg.Context(n, npr)                       # no key: the entry needs none
q = ctx.moduli()
gen = torch.Generator(device=dev)
gen.manual_seed(1)
c0 = bs.slab(q, (B, npr, n), dev, gen)
c1 = bs.slab(q, (B, npr, n), dev, gen)
ctx.set_lincomb_split(args.split)


def timed(fn):
    """The list of milliseconds of one function; the clock is not sampled."""
    return bs.timed([fn], max(args.reps, 50), args.warmup, clock=False)[0][0]


def report(ms, nbytes):
    return bs.record(ms, bytes=nbytes, tb_per_s=bs.tb_per_s(nbytes, ms))


result = dict(tool="lincomb_bench", n=n, primes=npr, B=B, split=args.split, device=torch.cuda.get_device_name(0))
dst = torch.empty_like(c0)
result["copy"] = report(timed(lambda: dst.copy_(c0)), 2 * B * row_bytes)
del dst
only = set(args.only.split(",")) if args.only else {"a", "b", "c"}

if "a" in only:
    o0 = torch.zeros((1, npr, n), dtype=torch.int32, device=dev)
    o1 = torch.zeros_like(o0)
    ms = timed(lambda: ctx.ct_lincomb(c0, o0, c1, o1, G=1))
    result["a"] = report(ms, 2 * (B + 1) * row_bytes)

if "b" in only:
    members = 256
    G = B // members
    perm = torch.randperm(B, device=dev, generator=gen).to(torch.int32)
    ptr = (torch.arange(G + 1, device=dev, dtype=torch.int64) * members).to(torch.int32)
    w = torch.randint(-2 ** 31, 2 ** 31, (G * members,), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
    o0 = torch.zeros((G, npr, n), dtype=torch.int32, device=dev)
    o1 = torch.zeros_like(o0)
    st = torch.zeros(G, dtype=torch.uint8, device=dev)
    ms = timed(lambda: ctx.ct_lincomb(c0, o0, c1, o1, row_ptr=ptr, idx=perm, w=w, status=st))
    assert bool((st == 1).all())
    result["b"] = report(ms, 2 * (G * members + G) * row_bytes)
    result["b"]["G"] = G

if "c" in only:
    G, Bc = 16, min(B, 4096)
    w = torch.randint(-2 ** 31, 2 ** 31, (G, Bc), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
    o0 = torch.zeros((G, npr, n), dtype=torch.int32, device=dev)
    o1 = torch.zeros_like(o0)
    i0, i1 = c0[:Bc], c1[:Bc]
    ms = timed(lambda: ctx.ct_lincomb(i0, o0, i1, o1, w=w))
    result["c"] = report(ms, 2 * (G * Bc + G) * row_bytes)        # every use of an input row counted
    result["c"]["unique_bytes"] = 2 * (Bc + G) * row_bytes        # each input row counted once
    result["c"]["G"] = G

for k in ("a", "b", "c"):
    if k in result:
        result[k]["ratio_to_copy"] = round(result[k]["tb_per_s"] / result["copy"]["tb_per_s"], 3)
ctx.close()
bs.emit(result, args.out)
