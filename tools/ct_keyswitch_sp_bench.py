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
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="*", default=["4096x3:65536", "16384x13:2048"], help="n x np : resident records")
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
    sys.exit("ct_keyswitch_sp_bench needs a GPU")
pkg = ge.load_package()
dev = torch.device("cuda:0")


def measure(n, npr, B):
    L = npr - 1
    ctx = pkg.Context(n, npr)
    q = ctx.moduli()
    qmin = min(q)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    f0 = torch.randint(0, qmin, (B, npr, n), dtype=torch.int32, device=dev, generator=gen)   # fresh records, level np
    f1 = torch.randint(0, qmin, (B, npr, n), dtype=torch.int32, device=dev, generator=gen)
    c0, c1 = torch.empty((B, L, n), dtype=torch.int32, device=dev), torch.empty((B, L, n), dtype=torch.int32, device=dev)
    ctx.ct_drop_primes(f0, c0, f1, c1)
    s0, s1, d0, d1, t0, t1 = (torch.empty_like(c0) for _ in range(6))
    u0, u1, v0, v1 = (torch.empty_like(f0) for _ in range(4))
    rng = np.random.default_rng(2)
    words = lambda rows: np.stack([rng.integers(0, q[i], (rows, n), dtype=np.uint32) for i in range(npr)], axis=1)
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

    def report(v):
        med = statistics.median(v)
        return dict(ms=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), reps=len(v),
                    records_per_s=round(B / med * 1e3))

    r = dict(n=n, primes=npr, level=L, B=B, sp=report(ms[0]), digit_same_level=report(ms[1]),
             today_lift_rotate_rescale=report(ms[2]))
    r["sp_over_digit_ms"] = round(r["sp"]["ms"] / r["digit_same_level"]["ms"], 3)
    r["sp_over_today_ms"] = round(r["sp"]["ms"] / r["today_lift_rotate_rescale"]["ms"], 3)
    r["clock"] = cs.summary()
    ctx.close()
    return r


result = dict(tool="ct_keyswitch_sp_bench", step=args.step, device=torch.cuda.get_device_name(0), shapes=[])
for sh in args.shapes:
    shape, B = sh.split(":")
    n, npr = (int(v) for v in shape.split("x"))
    result["shapes"].append(measure(n, npr, int(B)))
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
