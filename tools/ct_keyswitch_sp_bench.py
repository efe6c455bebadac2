#!/usr/bin/env python3
"""Time of the special-prime rotation se_amd_ct_galois_sp_device on resident records against what the tree offered before
it, HIP events, one process, the sides alternating inside one loop (the protocol of tools/ct_galois_bench.py):
  sp      (c0, c1) of level L -> (out0, out1) of level L under a special-prime key (np = L + 1 primes in the context):
          4 L + 2 transforms per output prime, the automorphism's LDS scatters and gathers; the record keeps its scale.
  digit   se_amd_ct_galois_device on the same rows at the same level L: 3 L transforms per output prime.  The same work
          shape, but its result is only usable at a raised scale.
  today   what a caller runs today to rotate a FRESH record (level L + 1 = np): lift by 2^30 with
          se_amd_ct_lincomb_device (one weighted entry per record, both slabs), se_amd_ct_galois_device at level L + 1,
          se_amd_ct_rescale_device down to level L.  Three entries; it ends at level L too, at scale Delta 2^30 / q_last.
Shapes: 4096 x 3 with L = 2 and 16384 x 13 with L = 12.  Key words and slabs are random residues (no secret key: no entry
needs one).  The engine clock is sampled (bench.ClockSampler) while each loop runs.  Prints one JSON line; --out also
writes it.
  python tools/ct_keyswitch_sp_bench.py [--shapes 4096x3:65536 16384x13:2048 --step 1 --reps 20 --warmup 3 --out FILE]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="*", default=["4096x3:65536", "16384x13:2048"], help="n x np : resident records")
ap.add_argument("--step", type=int, default=1)
bs.add_common_args(ap, reps=20, warmup=3)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_keyswitch_sp_bench")


def measure(n, npr, B):
    L = npr - 1
    ctx = pkg.Context(n, npr)
    q = ctx.moduli()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    f0 = bs.slab(q, (B, npr, n), dev, gen)                     # fresh records, level np
    f1 = bs.slab(q, (B, npr, n), dev, gen)
    c0, c1 = torch.empty((B, L, n), dtype=torch.int32, device=dev), torch.empty((B, L, n), dtype=torch.int32, device=dev)
    ctx.ct_drop_primes(f0, c0, f1, c1)
    s0, s1, d0, d1, t0, t1 = (torch.empty_like(c0) for _ in range(6))
    u0, u1, v0, v1 = (torch.empty_like(f0) for _ in range(4))
    rng = np.random.default_rng(2)
    words = lambda rows: bs.key_words(rng, q, rows, n, npr)
    elt = pkg.galois_element(n, args.step)
    ctx.set_galois_keys([elt], words(2 * npr)[None], words(2 * npr)[None])
    ctx.set_galois_keys_sp([elt], words(npr - 1)[None], words(npr - 1)[None])
    row_ptr = torch.arange(B + 1, dtype=torch.int32, device=dev)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    w = torch.full((B,), 1 << 30, dtype=torch.int32, device=dev)

    def today():
        ctx.ct_lincomb(f0, u0, f1, u1, row_ptr=row_ptr, idx=idx, w=w)
        ctx.ct_galois(u0, u1, elt, v0, v1)
        ctx.ct_rescale(v0, t0, v1, t1, primes=npr)

    fns = [lambda: ctx.ct_galois_sp(c0, c1, elt, s0, s1), lambda: ctx.ct_galois(c0, c1, elt, d0, d1), today]
    ms, clock = bs.timed(fns, max(args.reps, 10), args.warmup)

    def report(v):
        return bs.record(v, records_per_s=bs.per_s(B, v))

    r = dict(n=n, primes=npr, level=L, B=B, sp=report(ms[0]), digit_same_level=report(ms[1]),
             today_lift_rotate_rescale=report(ms[2]))
    r["sp_over_digit_ms"] = round(r["sp"]["ms"] / r["digit_same_level"]["ms"], 3)
    r["sp_over_today_ms"] = round(r["sp"]["ms"] / r["today_lift_rotate_rescale"]["ms"], 3)
    r["clock"] = clock
    ctx.close()
    return r


result = dict(tool="ct_keyswitch_sp_bench", step=args.step, device=torch.cuda.get_device_name(0), shapes=[])
for sh in args.shapes:
    shape, B = sh.split(":")
    n, npr = (int(v) for v in shape.split("x"))
    result["shapes"].append(measure(n, npr, int(B)))
bs.emit(result, args.out)
