#!/usr/bin/env python3
"""Time of the baby-step / giant-step linear transform se_amd_ct_bsgs_device on resident records against what the tree
offered before it, HIP events, one process, the sides alternating inside one loop (the protocol of
tools/ct_keyswitch_sp_hoist_bench.py).  4096 x 3, level 3, B resident records walked in chunks of --chunk records by both
sides (the plan's workspace holds one chunk):
  (a) 64 diagonals:  an 8 x 8 plan (14 Galois keys) against the flat se_amd_ct_lintrans_device plan with 63 elements
      plus diag0 (63 keys and 63 folded key blocks).  No threshold: the ratio is reported whichever way it falls.
  (b) 256 diagonals: a 16 x 16 plan (30 keys) against the composition of existing entries it replaces, per chunk: the
      many form for the 15 keyed baby steps, 256 se_amd_ct_mul_plain_device calls on the pre-rotated diagonals, one
      se_amd_ct_lincomb_device per giant step for the inner sums, 15 se_amd_ct_galois_device calls, one
      se_amd_ct_lincomb_device for the outer sum.  The two give the same bits (recorded); the plan must not lose.
Also the three phases of each plan timed as separate calls (many / inner / accumulate; timing only, every chunk reuses
one set of stacks), and plan plus key bytes of both sides.  Key words, diagonal words and slabs are random residues (no secret key: no entry needs one).  The engine clock
is sampled (bench.ClockSampler) while the loop runs.  Prints one JSON line; --out also writes it.
  python tools/ct_bsgs_bench.py [--B 16384 --chunk 2048 --reps 10 --warmup 2 --out profiles/ct_bsgs_bench.json]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=16384, help="resident records")
ap.add_argument("--chunk", type=int, default=2048, help="records per chunk (the plan's workspace holds one)")
bs.add_common_args(ap, reps=10, warmup=2)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_bsgs_bench")
N, NP = 4096, 3
B, BC = args.B, min(args.chunk, args.B)


def timed(fns, reps, warmup):
    """bs.timed with every list of milliseconds made a record."""
    ms, clock = bs.timed(fns, reps, warmup)
    return [bs.record(v, records_per_s=bs.per_s(B, v)) for v in ms], clock


def measure(n1, n2, flat):
    ctx = pkg.Context(N, NP)
    q = ctx.moduli()
    gen = torch.Generator(device=dev)
    gen.manual_seed(n1)
    rand = lambda *shape: bs.slab(q, shape, dev, gen)
    c0, c1 = rand(B, NP, N), rand(B, NP, N)
    o0, o1, r0, r1 = (torch.empty_like(c0) for _ in range(4))
    rng = np.random.default_rng(n1 + 100)
    words = lambda rows: bs.key_words(rng, q, rows, N, NP)
    G = n1 * n2
    baby = [pkg.galois_element(N, b) for b in range(n1)]
    giant = [pkg.galois_element(N, n1 * g) for g in range(n2)]
    bsgs_keys = baby[1:] + giant[1:]
    all_elts = [pkg.galois_element(N, s) for s in range(1, G)]
    keys = all_elts if flat else bsgs_keys
    assert len(set(keys)) == len(keys) <= 64 and set(bsgs_keys) <= set(keys)
    ctx.set_galois_keys(keys, np.stack([words(2 * NP) for _ in keys]), np.stack([words(2 * NP) for _ in keys]))
    diag = rand(n2, n1, NP, N)                                 # diagonal n1 g + b at [g][b]
    plan = ctx.bsgs_plan(baby, giant, diag)
    ws_bytes = ctx.bsgs_workspace_bytes(plan, BC, NP)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    key_bytes = 32 * NP * NP * N                               # one installed element: 16 R np n, R = 2 np
    r = dict(diagonals=G, n1=n1, n2=n2, chunk=BC,
             bsgs=dict(galois_keys=len(bsgs_keys), key_bytes=len(bsgs_keys) * key_bytes, plan_bytes=G * NP * N * 4,
                       workspace_bytes=ws_bytes))

    def bsgs():
        ctx.ct_bsgs(plan, c0, c1, o0, o1, ws, workspace_bytes=ws_bytes)

    # the three phases as separate calls on one chunk's stacks
    rot0, rot1 = (torch.empty((n1, BC, NP, N), dtype=torch.int32, device=dev) for _ in range(2))
    in0, in1 = (torch.empty((n2, BC, NP, N), dtype=torch.int32, device=dev) for _ in range(2))
    src = torch.from_numpy(np.stack([pkg.galois_table(N, pow(g, -1, 2 * N)).astype(np.int64) for g in giant])).to(dev)
    dperm = torch.stack([diag[g][..., src[g]] for g in range(n2)]).contiguous()
    chunks = [slice(b0, min(b0 + BC, B)) for b0 in range(0, B, BC)]
    assert all(c.stop - c.start == BC for c in chunks), "--B must be a multiple of --chunk"

    def phase_many():
        for c in chunks:
            rot0[0].copy_(c0[c])
            rot1[0].copy_(c1[c])
            ctx.ct_galois_many(c0[c], c1[c], baby[1:], rot0[1:], rot1[1:])

    def phase_inner():
        for c in chunks:
            ctx.ct_mul_plain_sum(rot0, dperm, in0, rot1, in1)

    def phase_accum():
        for c in chunks:
            ctx.ct_galois_accum(in0, in1, giant, r0[c], r1[c])

    if flat:
        fplan = ctx.lintrans_plan(all_elts, diag.reshape(G, NP, N)[1:].contiguous(), diag.reshape(G, NP, N)[0].contiguous())
        r["other"] = dict(what="flat se_amd_ct_lintrans_device plan, 63 elements and diag0", galois_keys=G - 1,
                          key_bytes=(G - 1) * key_bytes, plan_bytes=((G - 1) * 32 * NP * NP + G * 8 * NP) * N)

        def other():
            for c in chunks:
                ctx.ct_lintrans(fplan, c0[c], c1[c], r0[c], r1[c])
    else:
        fplan = None
        prod0, prod1 = (torch.empty((n1, BC, NP, N), dtype=torch.int32, device=dev) for _ in range(2))
        g0, g1 = (torch.empty((n2, BC, NP, N), dtype=torch.int32, device=dev) for _ in range(2))

        def sum_lists(terms):
            ptr = (torch.arange(BC + 1, dtype=torch.int64, device=dev) * terms).to(torch.int32)
            idx = (torch.arange(BC, dtype=torch.int64, device=dev)[:, None] +
                   torch.arange(terms, dtype=torch.int64, device=dev)[None, :] * BC).reshape(-1).to(torch.int32)
            return ptr, idx.contiguous()

        ptr1, idx1 = sum_lists(n1)
        ptr2, idx2 = sum_lists(n2)
        r["other"] = dict(what="many form, 256 ct_mul_plain, 16 ct_lincomb, 15 ct_galois, ct_lincomb",
                          galois_keys=len(bsgs_keys), key_bytes=len(bsgs_keys) * key_bytes, plan_bytes=G * NP * N * 4,
                          workspace_bytes=8 * (n1 + n2) * BC * NP * N * 4 // 2)

        def other():
            for c in chunks:
                rot0[0].copy_(c0[c])
                rot1[0].copy_(c1[c])
                ctx.ct_galois_many(c0[c], c1[c], baby[1:], rot0[1:], rot1[1:])
                for g in range(n2):
                    for b in range(n1):
                        ctx.ct_mul_plain(rot0[b], dperm[g, b][None], prod0[b], rot1[b], prod1[b])
                    ctx.ct_lincomb(prod0.view(n1 * BC, NP, N), in0[g], prod1.view(n1 * BC, NP, N), in1[g], row_ptr=ptr1,
                                   idx=idx1)
                g0[0].copy_(in0[0])
                g1[0].copy_(in1[0])
                for g in range(1, n2):
                    ctx.ct_galois(in0[g], in1[g], giant[g], g0[g], g1[g])
                ctx.ct_lincomb(g0.view(n2 * BC, NP, N), r0[c], g1.view(n2 * BC, NP, N), r1[c], row_ptr=ptr2, idx=idx2)

    (t_bsgs, t_other), clock = timed([bsgs, other], max(args.reps, 5), args.warmup)
    if not flat:
        r["composition_equals_plan"] = bool((o0 == r0).all()) and bool((o1 == r1).all())
    r["bsgs"].update(t_bsgs)
    r["other"].update(t_other)
    r["bsgs_over_other_ms"] = round(t_bsgs["ms"] / t_other["ms"], 3)
    r["clock"] = clock
    phases, pclock = timed([phase_many, phase_inner, phase_accum], max(args.reps // 2, 3), 1)
    r["phases"] = dict(many=phases[0], inner=phases[1], accumulate=phases[2], clock=pclock)
    # the algorithmic bytes of the inner phase (both stacks read once, the inner stacks written once) over its time
    r["phases"]["inner_algorithmic_TBps"] = round(len(chunks) * 2 * (n1 + n2) * BC * NP * N * 4 / phases[1]["ms"] / 1e9, 3)
    plan.close()
    if fplan is not None:
        fplan.close()
    ctx.close()
    return r


result = dict(tool="ct_bsgs_bench", device=torch.cuda.get_device_name(0), n=N, primes=NP, level=NP, B=B,
              a_64_diagonals=measure(8, 8, True))
torch.cuda.empty_cache()
result["b_256_diagonals"] = measure(16, 16, False)
result["b_plan_does_not_lose"] = result["b_256_diagonals"]["bsgs_over_other_ms"] <= 1.0
bs.emit(result, args.out)
