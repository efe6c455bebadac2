#!/usr/bin/env python3
"""Throughput of the keyed entries (key rings) against the unkeyed entry: one JSON line per configuration.

Method as bench.py: device-resident inputs, W untimed warm-up steps, then K timed steps between two device fences,
the engine clock sampled (bench.ClockSampler) over the timed steps.

  C2 (n=4096 x 3, symmetric, B=65 536) and C3 (public key): unkeyed; keyed K=1; K=64; K=2 048; K=B (distinct keys)
  C4 (n=16384 x 6, symmetric, B=32 768): unkeyed; keyed K=B

Indices are uniform random (seeded).  Keys: K <= 2 048 come from gen_keys_batch; the K = B rings are random valid keys
generated on the host (2-bit codes 0..2, public-key words below q_j) -- their values do not change the work.

  python tools/keyed_throughput.py [--steps 40] [--warmup 5] [--configs c2,c3,c4] [--no-big]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = {"c2": (4096, 3, "sym", 65536), "c3": (4096, 3, "asym", 65536), "c4": (16384, 6, "sym", 32768)}


def random_keys(ctx, K, mode, rng):
    n, npr = ctx.n, ctx.np
    if mode == "sym":
        sk = np.zeros((K, n // 4), dtype=np.uint8)
        for s in range(4):   # four 2-bit codes per byte, each 0..2
            sk |= (rng.integers(0, 3, size=(K, n // 4), dtype=np.uint8) << np.uint8(6 - 2 * s))
        return sk, None, None
    q = np.array(ctx.moduli(), dtype=np.uint32)[None, :, None]
    pk = [np.empty((K, npr, n), dtype=np.uint32) for _ in range(2)]
    for p in pk:
        for lo in range(0, K, 1024):   # bounded temporaries
            hi = min(K, lo + 1024)
            p[lo:hi] = rng.integers(0, 1 << 30, size=(hi - lo, npr, n), dtype=np.uint32) % q
    return None, pk[0], pk[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="c2,c3,c4")
    ap.add_argument("--no-big", action="store_true", help="skip the K = B rings")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import vectors as V
    from bench import ClockSampler
    ge.ensure_built()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for name in a.configs.split(","):
        n, npr, mode, B = CONFIGS[name]
        ctx = pkg.Context(n, npr)
        ctx.reserve(B)
        vals = t(V.bench_values(B, n))
        ss_np, sd_np = V.bench_seeds(B)
        ss, sd = t(ss_np), t(sd_np)
        c0 = torch.empty((B, npr, n), dtype=torch.int32, device=dev)
        c1 = torch.empty_like(c0)
        status = torch.empty(B, dtype=torch.uint8, device=dev)
        rng = np.random.default_rng(1234)
        Ks = [None, B] if name == "c4" else [None, 1, 64, 2048, B]
        if a.no_big:
            Ks = [k for k in Ks if k != B]
        base = None
        for K in Ks:
            if K is None:
                sk, pk0, pk1 = ctx.gen_keys_batch(V.derive_seeds("kt-pk", 1), V.derive_seeds("kt-ep", 1),
                                                  sk_seeds=V.derive_seeds("kt-sk", 1))
                if mode == "sym":
                    ctx.set_secret_key(sk[0])
                else:
                    ctx.set_public_key(pk0[0], pk1[0])
            else:
                if K <= 2048:
                    sk, pk0, pk1 = ctx.gen_keys_batch(V.derive_seeds("kt-pk", K), V.derive_seeds("kt-ep", K),
                                                      sk_seeds=V.derive_seeds("kt-sk", K))
                else:
                    sk, pk0, pk1 = random_keys(ctx, K, mode, rng)
                t_in = time.perf_counter()
                if mode == "sym":
                    ctx.set_secret_keyring(sk)
                else:
                    ctx.set_public_keyring(pk0, pk1)
                install_s = time.perf_counter() - t_in
                del sk, pk0, pk1
                idx = t(rng.integers(0, K, size=B).astype(np.uint32).view(np.int32))

            def step():
                if K is None and mode == "sym":
                    ctx.encrypt_sym(vals, ss, sd, c0, c1, status=status)
                elif K is None:
                    ctx.encrypt_asym(vals, sd, c0, c1, status=status)
                elif mode == "sym":
                    ctx.encrypt_sym_keyed(vals, idx, ss, sd, c0, c1, status=status)
                else:
                    ctx.encrypt_asym_keyed(vals, idx, sd, c0, c1, status=status)

            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            with ClockSampler(torch, 0) as cs:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
            ms = 1e3 * el / a.steps
            ok = bool((status == 1).all().item())
            if K is None:
                base = ms
            ring_mib = None if K is None else K * 2 * npr * n * 4 * (1 if mode == "sym" else 2) / 2 ** 20
            print(json.dumps({"config": name.upper(), "n": n, "nprimes": npr, "mode": mode, "B": B,
                              "keys": "unkeyed" if K is None else K, "ring_mib": ring_mib,
                              "ring_install_s": None if K is None else round(install_s, 3),
                              "ms_per_step": round(ms, 4), "ct_per_s": round(B / (ms / 1e3)),
                              "vs_unkeyed": None if K is None or base is None else round(ms / base, 4),
                              "status_all_ok": ok, "steps": a.steps, "warmup": a.warmup,
                              "clock": cs.summary()}), flush=True)
        ctx.close()
        del vals, ss, sd, c0, c1, status
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
