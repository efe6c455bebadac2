#!/usr/bin/env python3
"""Time of the special-prime baby-step / giant-step transform se_amd_ct_bsgs_sp_device (division by P deferred) on resident
fresh-scale records against what the tree offered before it, HIP events, one process, the sides alternating inside one
loop (the protocol of tools/ct_bsgs_bench.py).  4096 x 3, records of level L = 2, B resident records walked in chunks of
--chunk records by every side (the plan's workspace holds one chunk); 8 x 8 and 16 x 16 plans:
  plan   ONE se_amd_ct_bsgs_sp_device call: n2 + 1 divisions by P per record.
  (a)    the composition of entries that existed before, the same result up to the roundings (n1 + n2 - 2 divisions), per
         chunk: n1 - 1 se_amd_ct_galois_sp_device calls for the baby steps, se_amd_ct_mul_plain_sum_device at level L on the
         pre-rotated diagonals, n2 - 1 se_amd_ct_galois_sp_device calls for the giant steps, and the
         se_amd_ct_lincomb_device sum of the n2 records on a context of L primes (that entry works on records of its
         context's np rows).  THE condition: the plan is faster than (a).
  (b)    the digit path, reported without a threshold: lift by 2^18 (se_amd_ct_lincomb_device) at level L + 1,
         se_amd_ct_bsgs_device with the same plan shape, se_amd_ct_rescale_device down to level L.
Also the four phases of the plan timed as separate calls (many_ext / sum_ext / mod_down / accum_sp; timing only, every
chunk reuses one set of stacks).  Key words, diagonal words and slabs are random residues (no secret key: no entry needs
one).  The engine clock is sampled (bench.ClockSampler) while the loops run.  Prints one JSON line; --out also writes it.
  python tools/ct_bsgs_sp_bench.py [--B 16384 --chunk 2048 --reps 10 --warmup 2 --out profiles/ct_bsgs_sp_bench.json]"""
import argparse

import bench_support as bs

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=16384, help="resident records")
ap.add_argument("--chunk", type=int, default=2048, help="records per chunk (the plan's workspace holds one)")
bs.add_common_args(ap, reps=10, warmup=2)
args = ap.parse_args()

import numpy as np

pkg, torch, dev = bs.start("ct_bsgs_sp_bench")
N, NP = 4096, 3
L = NP - 1
LIFT = 1 << 18
B, BC = args.B, min(args.chunk, args.B)


def timed(fns, reps, warmup):
    """bs.timed with every list of milliseconds made a record."""
    ms, clock = bs.timed(fns, reps, warmup)
    return [bs.record(v, records_per_s=bs.per_s(B, v)) for v in ms], clock


def measure(n1, n2):
    ctx = pkg.Context(N, NP)
    low = pkg.Context(N, L)                                    # ct_lincomb on level-L records: rows of L n words
    q = ctx.moduli()
    assert low.moduli() == q[:L]
    gen = torch.Generator(device=dev)
    gen.manual_seed(n1)
    rand = lambda *shape: bs.slab(q, shape, dev, gen)
    f0, f1 = rand(B, NP, N), rand(B, NP, N)                    # the fresh records; their first L rows are the level-L ones
    c0, c1 = f0[:, :L].contiguous(), f1[:, :L].contiguous()
    o0, o1, r0, r1, t0, t1 = (torch.empty_like(c0) for _ in range(6))
    rng = np.random.default_rng(n1 + 100)
    words = lambda rows: bs.key_words(rng, q, rows, N, NP)
    G = n1 * n2
    baby = [pkg.galois_element(N, b) for b in range(n1)]
    giant = [pkg.galois_element(N, n1 * g) for g in range(n2)]
    keys = baby[1:] + giant[1:]
    assert len(set(keys)) == len(keys) <= 64
    ctx.set_galois_keys_sp(keys, np.stack([words(NP - 1) for _ in keys]), np.stack([words(NP - 1) for _ in keys]))
    ctx.set_galois_keys(keys, np.stack([words(2 * NP) for _ in keys]), np.stack([words(2 * NP) for _ in keys]))
    diag = rand(n2, n1, NP, N)                                 # diagonal n1 g + b at [g][b]
    plan = ctx.bsgs_plan_sp(baby, giant, diag)
    ws_bytes = ctx.bsgs_workspace_bytes(plan, BC, L)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    dplan = ctx.bsgs_plan(baby, giant, diag)
    dws_bytes = ctx.bsgs_workspace_bytes(dplan, BC, NP)
    dws = torch.empty(dws_bytes // 4, dtype=torch.int32, device=dev)
    r = dict(diagonals=G, n1=n1, n2=n2, chunk=BC, galois_keys=len(keys),
             key_bytes_sp=len(keys) * 16 * (NP - 1) * NP * N, key_bytes_digit=len(keys) * 32 * NP * NP * N,
             plan_bytes=G * NP * N * 4, workspace_bytes=ws_bytes, digit_workspace_bytes=dws_bytes)
    chunks = [slice(b0, min(b0 + BC, B)) for b0 in range(0, B, BC)]
    assert all(c.stop - c.start == BC for c in chunks), "--B must be a multiple of --chunk"

    def plan_call():
        ctx.ct_bsgs_sp(plan, c0, c1, o0, o1, ws, workspace_bytes=ws_bytes)

    # (a): entries that existed before
    src = torch.from_numpy(np.stack([pkg.galois_table(N, pow(g, -1, 2 * N)).astype(np.int64) for g in giant])).to(dev)
    dperm = torch.stack([diag[g][..., src[g]] for g in range(n2)]).contiguous()
    rot0, rot1 = (torch.empty((n1, BC, L, N), dtype=torch.int32, device=dev) for _ in range(2))
    in0, in1, g0, g1 = (torch.empty((n2, BC, L, N), dtype=torch.int32, device=dev) for _ in range(4))
    ptr = (torch.arange(BC + 1, dtype=torch.int64, device=dev) * n2).to(torch.int32)
    idx = (torch.arange(BC, dtype=torch.int64, device=dev)[:, None] +
           torch.arange(n2, dtype=torch.int64, device=dev)[None, :] * BC).reshape(-1).to(torch.int32).contiguous()

    def a_composition():
        for c in chunks:
            rot0[0].copy_(c0[c])
            rot1[0].copy_(c1[c])
            for b in range(1, n1):
                ctx.ct_galois_sp(c0[c], c1[c], baby[b], rot0[b], rot1[b])
            ctx.ct_mul_plain_sum(rot0, dperm, in0, rot1, in1, primes=L)
            g0[0].copy_(in0[0])
            g1[0].copy_(in1[0])
            for g in range(1, n2):
                ctx.ct_galois_sp(in0[g], in1[g], giant[g], g0[g], g1[g])
            low.ct_lincomb(g0.view(n2 * BC, L, N), r0[c], g1.view(n2 * BC, L, N), r1[c], row_ptr=ptr, idx=idx)

    # (b): the digit path at level L + 1
    u0, u1, v0, v1 = (torch.empty_like(f0) for _ in range(4))
    lptr = torch.arange(B + 1, dtype=torch.int32, device=dev)
    lidx = torch.arange(B, dtype=torch.int32, device=dev)
    lw = torch.full((B,), LIFT, dtype=torch.int32, device=dev)

    def b_digit_path():
        ctx.ct_lincomb(f0, u0, f1, u1, row_ptr=lptr, idx=lidx, w=lw)
        ctx.ct_bsgs(dplan, u0, u1, v0, v1, dws, workspace_bytes=dws_bytes)
        ctx.ct_rescale(v0, t0, v1, t1, primes=NP)

    (t_plan, t_a, t_b), clock = timed([plan_call, a_composition, b_digit_path], max(args.reps, 5), args.warmup)
    r["plan"] = t_plan
    r["a_composition_of_existing_entries"] = t_a
    r["b_digit_path_lift_bsgs_rescale"] = t_b
    r["plan_over_a_ms"] = round(t_plan["ms"] / t_a["ms"], 3)
    r["plan_over_b_ms"] = round(t_plan["ms"] / t_b["ms"], 3)
    r["a_equals_plan"] = bool((o0 == r0).all()) and bool((o1 == r1).all())       # expected false: other roundings
    r["clock"] = clock

    # the four phases as separate calls on one chunk's stacks
    ua, ub = (torch.empty((n1, BC, L + 1, N), dtype=torch.int32, device=dev) for _ in range(2))
    va, vb = (torch.empty((n2, BC, L + 1, N), dtype=torch.int32, device=dev) for _ in range(2))

    def phase_many_ext():
        for c in chunks:
            ctx.ct_galois_many_ext_sp(c0[c], c1[c], baby, ua, ub)

    def phase_sum_ext():
        for c in chunks:
            ctx.ct_mul_plain_sum_ext_sp(ua, dperm, va, ub, vb)

    def phase_mod_down():
        for c in chunks:
            ctx.ct_mod_down_sp(va, in0, vb, in1)

    def phase_accum_sp():
        for c in chunks:
            ctx.ct_galois_accum_sp(in0, in1, giant, t0[c], t1[c])

    phases, pclock = timed([phase_many_ext, phase_sum_ext, phase_mod_down, phase_accum_sp], max(args.reps // 2, 3), 1)
    r["phases"] = dict(many_ext=phases[0], sum_ext=phases[1], mod_down=phases[2], accum_sp=phases[3], clock=pclock)
    plan.close()
    dplan.close()
    ctx.close()
    low.close()
    return r


result = dict(tool="ct_bsgs_sp_bench", device=torch.cuda.get_device_name(0), n=N, primes=NP, level=L, B=B,
              plan_8x8=measure(8, 8))
torch.cuda.empty_cache()
result["plan_16x16"] = measure(16, 16)
result["plan_faster_than_a"] = all(result[k]["plan_over_a_ms"] < 1.0 for k in ("plan_8x8", "plan_16x16"))
bs.emit(result, args.out)
