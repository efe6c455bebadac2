#!/usr/bin/env python3
"""Time and device memory of the encrypted inner product on resident records, HIP events, one process, the sides
alternating inside one loop (the protocol of tools/ct_switch_bench.py).  P pairs (k, k) of two resident batches, rows of m
consecutive pairs, G = P / m output rows; four sides that compute the same sums:
  (1) dot_sp       se_amd_ct_dot_sp_device: one launch, no intermediate, no workspace.
  (2) mul_sum      se_amd_ct_mul_sum_device + se_amd_ct_relin_sp_device on the G rows: the same bits as (1).
  (3) lazy         se_amd_ct_mul_device on the P pairs + se_amd_ct_lincomb_device twice (slabs 0 / 1, then slab 2) +
                   se_amd_ct_relin_sp_device on the G rows: the composition the tree offered before, the same bits as (1).
  (4) eager        se_amd_ct_mul_device + se_amd_ct_relin_sp_device on every pair + se_amd_ct_lincomb_device: the documented
                   path, m key switches and m roundings per row (other bits for m >= 2).
ct_lincomb works on records of its context's np rows, so the level-L sums run on a context of L primes.
`extra_bytes` is what a side allocates beside the two input batches and the [G][L][n] x 2 result.  Configurations:
4096 x 3, L = 2, P = 32768, m = 1, 8, 64 and 16384 x 13, L = 12, P = 1024, m = 1, 8.  Key words and slabs are random
residues (no secret key: no entry needs one).  The engine clock is sampled (bench.ClockSampler) while the loops run.
No ratio is required: the figures are reported.  Prints one JSON line; --out also writes it.
  python tools/ct_dot_bench.py [--reps 20 --warmup 2 --configs 0,1 --out profiles/ct_dot_bench.json]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="0,1", help="indices into CONFIGS")
ap.add_argument("--pairs", type=int, default=0, help="override P of every configuration (a rehearsal at a small size)")
bs.add_common_args(ap, reps=20, warmup=2)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_dot_bench")
CONFIGS = [dict(n=4096, primes=3, pairs=32768, m=(1, 8, 64)), dict(n=16384, primes=13, pairs=1024, m=(1, 8))]


def run_config(cfg):
    N, NP = cfg["n"], cfg["primes"]
    L = NP - 1
    P = args.pairs or cfg["pairs"]
    ctx, low = pkg.Context(N, NP), pkg.Context(N, L)               # low: ct_lincomb on level-L records
    q = ctx.moduli()
    assert low.moduli() == q[:L]
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    a0, a1, b0, b1 = (bs.slab(q, (P, L, N), dev, gen) for _ in range(4))
    rng = np.random.default_rng(17)
    words = lambda: bs.key_words(rng, q, NP - 1, N, NP)
    ctx.set_relin_key_sp(words(), words())
    rec = L * N * 4                                                # bytes of one slab row of a record
    t = [torch.empty((P, L, N), dtype=torch.int32, device=dev) for _ in range(3)]     # the per-pair tensor, sides 3 and 4
    r = [torch.empty((P, L, N), dtype=torch.int32, device=dev) for _ in range(2)]     # the per-pair relinearisation, side 4
    every = torch.arange(P, dtype=torch.int32, device=dev)
    out = dict(n=N, primes=NP, level=L, pairs=P, input_bytes=4 * P * rec, rows={})
    for m in cfg["m"]:
        if P % m:
            continue
        G = P // m
        ptr = (torch.arange(G + 1, dtype=torch.int64, device=dev) * m).to(torch.int32)
        res = [[torch.empty((G, L, N), dtype=torch.int32, device=dev) for _ in range(2)] for _ in range(4)]
        s = [torch.empty((G, L, N), dtype=torch.int32, device=dev) for _ in range(3)]  # the row tensors, sides 2 and 3

        def dot_sp():
            ctx.ct_dot_sp(a0, a1, b0, b1, ptr, None, None, *res[0])

        def mul_sum():
            ctx.ct_mul_sum(a0, a1, b0, b1, ptr, None, None, *s)
            ctx.ct_relin_sp(*s, *res[1])

        def lazy():
            ctx.ct_mul(a0, a1, b0, b1, *t)
            low.ct_lincomb(t[0], s[0], t[1], s[1], row_ptr=ptr, idx=every)
            low.ct_lincomb(t[2], s[2], row_ptr=ptr, idx=every)
            ctx.ct_relin_sp(*s, *res[2])

        def eager():
            ctx.ct_mul(a0, a1, b0, b1, *t)
            ctx.ct_relin_sp(*t, *r)
            low.ct_lincomb(r[0], res[3][0], r[1], res[3][1], row_ptr=ptr, idx=every)

        ms, clock = bs.timed([dot_sp, mul_sum, lazy, eager], max(args.reps, 3), args.warmup)
        sides = [bs.record(v, pairs_per_s=bs.per_s(P, v)) for v in ms]
        same = lambda k: bool((res[0][0] == res[k][0]).all()) and bool((res[0][1] == res[k][1]).all())  # noqa: E731
        extra = [0, 3 * G * rec, 3 * P * rec + 3 * G * rec, 3 * P * rec + 2 * P * rec]
        names = ("dot_sp", "mul_sum_relin_sp", "mul_lincomb2_relin_sp", "mul_relin_sp_lincomb")
        row = {nm: dict(sd, extra_bytes=eb) for nm, sd, eb in zip(names, sides, extra)}
        row.update(rows=G, pairs_per_row=m, result_bytes=2 * G * rec,
                   equal_bits=dict(mul_sum_relin_sp=same(1), mul_lincomb2_relin_sp=same(2), mul_relin_sp_lincomb=same(3)),
                   dot_over_mul_sum_ms=round(sides[0]["ms"] / sides[1]["ms"], 3),
                   dot_over_eager_ms=round(sides[0]["ms"] / sides[3]["ms"], 3), clock=clock)
        out["rows"][f"m_{m}"] = row
        del res, s
    ctx.close()
    low.close()
    return out


result = dict(tool="ct_dot_bench", device=torch.cuda.get_device_name(0),
              configs=[run_config(CONFIGS[int(k)]) for k in args.configs.split(",")])
bs.emit(result, args.out)
