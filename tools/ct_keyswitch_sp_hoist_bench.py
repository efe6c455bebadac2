#!/usr/bin/env python3
"""Time of the hoisted special-prime forms se_amd_ct_galois_sum_sp_device and se_amd_ct_lintrans_sp_device (G = 7, the
steps 1 .. 7) on resident records against what the tree offered before them, HIP events, one process, the sides
alternating inside one loop (the protocol of tools/ct_keyswitch_sp_bench.py):
  sum_sp       (c0, c1) of level L -> the record plus its 7 rotations, ONE call under the special-prime keys (np = L + 1
               primes in the context): 4 L + 2 transforms per output prime whatever G is, one division by P.
  a_single     what the call replaces: seven se_amd_ct_galois_sp_device calls into one slab of 8 B records whose first B
               are the input, then se_amd_ct_lincomb_device summing record b of every block.  That entry works on records
               of its context's np rows, so the level-L records are summed by a second context of L primes (the default
               chains are prefixes of one another), as a caller holding level-L records would.
  b_today      today's fresh-record path: lift by 2^30 (se_amd_ct_lincomb_device), se_amd_ct_galois_sum_device with
               add_input at level L + 1 = np, se_amd_ct_rescale_device down to level L.
  lintrans_sp  ONE se_amd_ct_lintrans_sp_device call, 7 diagonals and diag0.
  c = sum_sp   the sum form above is the transform's yardstick on the same key.
  d_today      lift, se_amd_ct_lintrans_device at level np, rescale.
Sides a, b and d are entries the tree already had.  Shapes: 4096 x 3 with L = 2 and 16384 x 13 with L = 12.  Key words,
diagonal words and slabs are random residues (no secret key: no entry needs one).  The engine clock is sampled
(bench.ClockSampler) while the loop runs.  Prints one JSON line; --out also writes it.
  python tools/ct_keyswitch_sp_hoist_bench.py [--shapes 4096x3:65536 16384x13:2048 --reps 20 --warmup 3 --out FILE]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="*", default=["4096x3:65536", "16384x13:2048"], help="n x np : resident records")
bs.add_common_args(ap, reps=20, warmup=3)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_keyswitch_sp_hoist_bench")
G = 7


def measure(n, npr, B):
    L = npr - 1
    ctx = pkg.Context(n, npr)
    low = pkg.Context(n, L)                                    # ct_lincomb on level-L records: rows of L n words
    q = ctx.moduli()
    assert low.moduli() == q[:L]
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    rand = lambda *shape: bs.slab(q, shape, dev, gen)
    f0, f1 = rand(B, npr, n), rand(B, npr, n)                  # fresh records, level np
    c0, c1 = torch.empty((B, L, n), dtype=torch.int32, device=dev), torch.empty((B, L, n), dtype=torch.int32, device=dev)
    ctx.ct_drop_primes(f0, c0, f1, c1)
    s0, s1, p0, p1, a0, a1, t0, t1 = (torch.empty_like(c0) for _ in range(8))
    u0, u1, v0, v1 = (torch.empty_like(f0) for _ in range(4))
    # side a: block 0 of the slab is the input, block e + 1 takes the rotation by elts[e]
    r0 = torch.empty(((G + 1) * B, L, n), dtype=torch.int32, device=dev)
    r1 = torch.empty_like(r0)
    r0[:B].copy_(c0)
    r1[:B].copy_(c1)
    rng = np.random.default_rng(2)
    words = lambda rows: bs.key_words(rng, q, rows, n, npr)
    elts = [pkg.galois_element(n, s) for s in range(1, G + 1)]
    ctx.set_galois_keys(elts, np.stack([words(2 * npr) for _ in elts]), np.stack([words(2 * npr) for _ in elts]))
    ctx.set_galois_keys_sp(elts, np.stack([words(npr - 1) for _ in elts]), np.stack([words(npr - 1) for _ in elts]))
    diag = rand(G + 1, npr, n)
    plan_sp = ctx.lintrans_plan_sp(elts, diag[1:].contiguous(), diag[0].contiguous())
    plan = ctx.lintrans_plan(elts, diag[1:].contiguous(), diag[0].contiguous())
    row_ptr = torch.arange(B + 1, dtype=torch.int32, device=dev)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    w = torch.full((B,), 1 << 30, dtype=torch.int32, device=dev)
    sum_ptr = (torch.arange(B + 1, dtype=torch.int64, device=dev) * (G + 1)).to(torch.int32)
    sum_idx = (torch.arange(B, dtype=torch.int64, device=dev)[:, None] +
               torch.arange(G + 1, dtype=torch.int64, device=dev)[None, :] * B).reshape(-1).to(torch.int32).contiguous()

    def sum_sp():
        ctx.ct_galois_sum_sp(c0, c1, elts, s0, s1, add_input=True)

    def a_single():
        for e, g in enumerate(elts):
            ctx.ct_galois_sp(c0, c1, g, r0[(e + 1) * B:(e + 2) * B], r1[(e + 1) * B:(e + 2) * B])
        low.ct_lincomb(r0, a0, r1, a1, row_ptr=sum_ptr, idx=sum_idx)

    def b_today():
        ctx.ct_lincomb(f0, u0, f1, u1, row_ptr=row_ptr, idx=idx, w=w)
        ctx.ct_galois_sum(u0, u1, elts, v0, v1, add_input=True)
        ctx.ct_rescale(v0, t0, v1, t1, primes=npr)

    def lintrans_sp():
        ctx.ct_lintrans_sp(plan_sp, c0, c1, p0, p1)

    def d_today():
        ctx.ct_lincomb(f0, u0, f1, u1, row_ptr=row_ptr, idx=idx, w=w)
        ctx.ct_lintrans(plan, u0, u1, v0, v1)
        ctx.ct_rescale(v0, t0, v1, t1, primes=npr)

    names = ("sum_sp", "a_seven_single_calls_and_sum", "b_today_lift_sum_rescale", "lintrans_sp",
             "d_today_lift_lintrans_rescale")
    fns = [sum_sp, a_single, b_today, lintrans_sp, d_today]
    ms, clock = bs.timed(fns, max(args.reps, 10), args.warmup)
    # the seven single calls and their sum give what the definition says they may not: another rounding
    same = bool((a0 == s0).all())
    r = dict(n=n, primes=npr, level=L, B=B, G=G, single_calls_equal_the_sum_form=same)
    for name, v in zip(names, ms):
        r[name] = bs.record(v, records_per_s=bs.per_s(B, v))
    ratio = lambda x, y: round(r[x]["ms"] / r[y]["ms"], 3)
    r["sum_sp_over_a_ms"] = ratio("sum_sp", "a_seven_single_calls_and_sum")
    r["sum_sp_over_b_ms"] = ratio("sum_sp", "b_today_lift_sum_rescale")
    r["lintrans_sp_over_sum_sp_ms"] = ratio("lintrans_sp", "sum_sp")
    r["lintrans_sp_over_d_ms"] = ratio("lintrans_sp", "d_today_lift_lintrans_rescale")
    r["sum_sp_faster_than_the_calls_it_replaces"] = r["sum_sp"]["ms"] < r["a_seven_single_calls_and_sum"]["ms"]
    r["clock"] = clock
    plan_sp.close()
    plan.close()
    low.close()
    ctx.close()
    return r


result = dict(tool="ct_keyswitch_sp_hoist_bench", device=torch.cuda.get_device_name(0), shapes=[])
for sh in args.shapes:
    shape, B = sh.split(":")
    n, npr = (int(v) for v in shape.split("x"))
    result["shapes"].append(measure(n, npr, int(B)))
    torch.cuda.empty_cache()
bs.emit(result, args.out)
