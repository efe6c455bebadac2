#!/usr/bin/env python3
"""Time of the switch-key ring entries on resident records at 4096 x 3, level L = 2, HIP events, one process, the sides
alternating inside one loop (the protocol of tools/ct_bsgs_sp_bench.py):
  switch    se_amd_ct_switch_keyed_sp_device on B records under K ring keys, against se_amd_ct_relin_sp_device(c0, 0, c1)
            on the same rows under ONE key: what choosing the key per record costs.
  sum m     se_amd_ct_switch_sum_keyed_sp_device with B / m rows of m consecutive records, m = 8 and m = 64, against the
            composition the tree offers without it: se_amd_ct_switch_keyed_sp_device on all B records, then the
            se_amd_ct_lincomb_device sum of every group on a context of L primes (that entry works on records of its
            context's np rows).  The ratio is reported, not required: a row runs on L workgroups whatever its length, so
            long rows trade transforms ((4 L - 2) m + 4 against (4 L + 2) m) for parallelism.
Key words and slabs are random residues (no secret key: no entry needs one).  The engine clock is sampled
(bench.ClockSampler) while the loops run.  Prints one JSON line; --out also writes it.
  python tools/ct_switch_bench.py [--B 65536 --K 64 --reps 40 --warmup 3 --out profiles/ct_switch_bench.json]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=65536, help="resident records (a multiple of 64)")
ap.add_argument("--K", type=int, default=64, help="keys in the ring")
bs.add_common_args(ap, reps=40, warmup=3)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_switch_bench")
N, NP = 4096, 3
L = NP - 1
B, K = args.B, args.K
assert B % 64 == 0


def timed(fns, reps, warmup):
    """bs.timed with every list of milliseconds made a record."""
    ms, clock = bs.timed(fns, reps, warmup)
    return [bs.record(v, records_per_s=bs.per_s(B, v)) for v in ms], clock


ctx = pkg.Context(N, NP)
low = pkg.Context(N, L)                                        # ct_lincomb on level-L records: rows of L n words
q = ctx.moduli()
assert low.moduli() == q[:L]
gen = torch.Generator(device=dev)
gen.manual_seed(7)
c0, c1 = bs.slab(q, (B, L, N), dev, gen), bs.slab(q, (B, L, N), dev, gen)
zero = torch.zeros_like(c1)
o0, o1, s0, s1 = (torch.empty_like(c0) for _ in range(4))
rng = np.random.default_rng(11)
words = lambda count: np.stack([rng.integers(0, q[i], (count, NP - 1, N), dtype=np.uint32) for i in range(NP)], axis=2)
wk0, wk1 = words(K), words(K)
ctx.set_switch_keyring_sp(wk0, wk1)
ctx.set_relin_key_sp(wk0[0], wk1[0])
key_idx = torch.from_numpy(rng.integers(0, K, B, dtype=np.int64).astype(np.int32)).to(dev)
idx = torch.arange(B, dtype=torch.int32, device=dev)

result = dict(tool="ct_switch_bench", device=torch.cuda.get_device_name(0), n=N, primes=NP, level=L, B=B, keys=K,
              ring_bytes=K * 16 * (NP - 1) * NP * N)


def switch_all():
    ctx.ct_switch_keyed_sp(c0, c1, key_idx, s0, s1)


def relin_all():
    ctx.ct_relin_sp(c0, zero, c1, o0, o1)


(t_switch, t_relin), clock = timed([switch_all, relin_all], max(args.reps, 5), args.warmup)
result["switch"] = dict(switch_keyed=t_switch, relin_sp_one_key=t_relin,
                        switch_over_relin_ms=round(t_switch["ms"] / t_relin["ms"], 3), clock=clock)

for m in (8, 64):
    G = B // m
    ptr = (torch.arange(G + 1, dtype=torch.int64, device=dev) * m).to(torch.int32)
    g0, g1, h0, h1 = (torch.empty((G, L, N), dtype=torch.int32, device=dev) for _ in range(4))

    def sum_call():
        ctx.ct_switch_sum_keyed_sp(c0, c1, key_idx, ptr, idx, g0, g1)

    def composition():
        ctx.ct_switch_keyed_sp(c0, c1, key_idx, s0, s1)
        low.ct_lincomb(s0, h0, s1, h1, row_ptr=ptr, idx=idx)

    (t_sum, t_comp), clock = timed([sum_call, composition], max(args.reps, 5), args.warmup)
    result[f"sum_{m}"] = dict(rows=G, records_per_row=m, switch_sum=t_sum, switch_then_lincomb=t_comp,
                              sum_over_composition_ms=round(t_sum["ms"] / t_comp["ms"], 3),
                              equal_bits=bool((g0 == h0).all()) and bool((g1 == h1).all()),   # expected false: m roundings
                              clock=clock)

ctx.close()
low.close()
bs.emit(result, args.out)
