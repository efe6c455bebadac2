#!/usr/bin/env python3
"""Time of slot packing on resident records, HIP events, one process, the sides alternating inside one loop (the protocol
of tools/ct_switch_bench.py):
  pack m    (1) ONE se_amd_ct_pack_sp_device call with B / m rows of m records, entry k of a row under the element of
            the step -k width (k = 0: the identity), against
            (2) the composition the tree offers without it: m se_amd_ct_galois_sp_device calls, call k on the B / m
            records that are entry k of their row (kept contiguous: the records lie in chunk layout for both sides) into
            the intermediate (k = 0 is a copy: those records enter the sum as they are), then the
            se_amd_ct_lincomb_device sum of every group on a context of L primes.
  Shapes: 4096 x 3, L = 2, 65 536 records, m = 1, 8, 16; 16384 x 13, L = 12, 2 048 records, m = 8.
  Device memory beside inputs and result: (1) none, (2) the rotated records, 2 B rows of L n words.
The ratio is reported, not required: counting transforms, (1) costs about (4 L - 2) / (4 L + 2) of (2)'s key switches and
saves the intermediate, but a row runs on L workgroups whatever its length.  Key words and slabs are random residues (no
secret key: no entry needs one).  The engine clock is sampled (bench.ClockSampler) while the loops run.  Prints one JSON
line; --out also writes it.
  python tools/ct_pack_bench.py [--reps 20 --warmup 2 --small --out profiles/ct_pack_bench.json]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true", help="1/16 of the records of every shape (a quick look)")
bs.add_common_args(ap, reps=20, warmup=2)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_pack_bench")
SHAPES = [(4096, 3, 65536, (1, 8, 16)), (16384, 13, 2048, (8,))]      # n, np, records, row lengths


def timed(fns, reps, warmup, B):
    """bs.timed with every list of milliseconds made a record."""
    ms, clock = bs.timed(fns, reps, warmup)
    return [bs.record(v, records_per_s=bs.per_s(B, v)) for v in ms], clock


result = dict(tool="ct_pack_bench", device=torch.cuda.get_device_name(0), cases=[])
for N, NP, B, lengths in SHAPES:
    if args.small:
        B //= 16
    L = NP - 1
    slots = N // 2
    ctx = pkg.Context(N, NP)
    low = pkg.Context(N, L)                                    # ct_lincomb on level-L records: rows of L n words
    q = ctx.moduli()
    assert low.moduli() == q[:L]
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    c0 = bs.slab(q, (B, L, N), dev, gen)
    c1 = bs.slab(q, (B, L, N), dev, gen)
    rng = np.random.default_rng(11)
    for m in lengths:
        width = slots // m
        elts = [pkg.galois_element(N, -width * k) for k in range(m)]
        assert elts[0] == 1 and len(set(elts)) == m
        if m > 1:
            words = lambda: np.stack([rng.integers(0, q[i], (m - 1, NP - 1, N), dtype=np.uint32)  # noqa: E731
                                      for i in range(NP)], axis=2)
            ctx.set_galois_keys_sp(elts[1:], words(), words())
        # records in chunk layout: record k G + g is entry k of row g, so that the composition's call k works on the
        # contiguous chunk k; both sides read the same slabs through the same CSR tables
        G = B // m
        ptr = (torch.arange(G + 1, dtype=torch.int64, device=dev) * m).to(torch.int32)
        e = torch.arange(B, dtype=torch.int64, device=dev)
        idx = ((e % m) * G + e // m).to(torch.int32)
        eidx = (e % m).to(torch.int32)
        g0, g1, h0, h1 = (torch.empty((G, L, N), dtype=torch.int32, device=dev) for _ in range(4))
        rot0, rot1 = torch.empty_like(c0), torch.empty_like(c1)    # (2)'s intermediate: 2 B rows of L n words

        def pack_call():
            ctx.ct_pack_sp(c0, c1, elts, eidx, g0, g1, primes=L, row_ptr=ptr, idx=idx)

        def composition():
            rot0[:G].copy_(c0[:G])                                 # step 0: the records as they are
            rot1[:G].copy_(c1[:G])
            for k in range(1, m):
                ctx.ct_galois_sp(c0[k * G:(k + 1) * G], c1[k * G:(k + 1) * G], elts[k], rot0[k * G:(k + 1) * G],
                                 rot1[k * G:(k + 1) * G], primes=L)
            low.ct_lincomb(rot0, h0, rot1, h1, row_ptr=ptr, idx=idx)

        (t_pack, t_comp), clock = timed([pack_call, composition], max(args.reps, 5), args.warmup, B)
        result["cases"].append(dict(
            n=N, primes=NP, level=L, B=B, m=m, rows=G, pack=t_pack, rotations_then_lincomb=t_comp,
            pack_over_composition_ms=round(t_pack["ms"] / t_comp["ms"], 3),
            transform_ratio=round((4 * L - 2) / (4 * L + 2), 3),
            extra_device_bytes=dict(pack=0, composition=2 * B * L * N * 4),
            equal_bits=bool((g0 == h0).all()) and bool((g1 == h1).all()),      # expected false for m > 2: m - 1 roundings
            clock=clock))
        del g0, g1, h0, h1, rot0, rot1
    del c0, c1
    ctx.close()
    low.close()

bs.emit(result, args.out)
