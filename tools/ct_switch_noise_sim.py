#!/usr/bin/env python3
"""CPU simulation of the switch-key ring (se_amd_ct_switch_keyed_sp_device, se_amd_ct_switch_sum_keyed_sp_device): fresh
records under K different device keys, dropped to level L, are brought under ONE aggregator key and summed, with one
division by the special prime per row; the sum is decoded under the aggregator key alone at the fresh scale Delta.
Everything is the oracle's primitives and Python / NumPy integers (tests/ct_model_switch.py holds the definition, the
switching keys come from ct_model.sp_key with target = NTT(s_from)), no GPU.
  row of m: records b = 0 .. m-1 with slot values in [-1, 1], record b under device key b mod K: the worst slot error of
            the switched sum against the sum of the values, the largest coefficient of what the switch adds to the sum of
            the records' own decrypted values, and both figures for m single switches, each rounded on its own, then
            summed ("_single").
One JSON line per case, then the table.
  python tools/ct_switch_noise_sim.py [4096x3:2:1 4096x3:2:8 8192x6:5:8 ...]   (n x np : L : m)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from oracle import pyoracle  # noqa: E402
import vectors as V  # noqa: E402
import ct_model as K  # noqa: E402
import ct_model_switch as KS  # noqa: E402
from ct_galois_noise_sim import decode, value  # noqa: E402

DEFAULT = ("4096x3:2:1", "4096x3:2:8", "4096x3:1:8", "8192x6:5:8")


def fleet(o, keys, m, L, seed):
    """m fresh records with slot values in [-1, 1], record b under device key b mod len(keys), dropped to L primes ->
    (vals float32 [m][n/2], key_idx, c0, c1 uint32 [m][L][n])."""
    n = o.n
    vals = np.random.default_rng(seed).uniform(-1.0, 1.0, (m, n // 2)).astype(np.float32)
    ss, sd = V.bench_seeds(m, first=40)
    key_idx = np.arange(m, dtype=np.uint32) % len(keys)
    c0, c1 = [], []
    for b in range(m):
        x = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), keys[key_idx[b]])
        c0.append(np.stack([np.array(x["c0"][j]) for j in range(L)]))   # dropping primes changes neither message nor scale
        c1.append(np.stack([np.array(x["c1"][j]) for j in range(L)]))
    return vals, key_idx, np.stack(c0), np.stack(c1)


def row(n, npr, L, m, nkeys=8):
    """-> dict: one row of m fresh records under nkeys device keys, switched to the aggregator key and summed."""
    o = pyoracle.Oracle(n, npr)
    p = npr - 1
    sk_to = V.secret_key(n, seed=5)
    keys = [V.secret_key(n, seed=100 + k) for k in range(nkeys)]
    hat = lambda sk: np.stack([o.ntt(o.expand_ternary(sk, j), j) for j in range(npr)])  # noqa: E731
    s_to = hat(sk_to)
    s_from = [hat(sk) for sk in keys]
    ring = [K.sp_key(o, sk_to, s_from[k][:p], f"switchsim-k{k}") for k in range(nkeys)]
    wk0, wk1 = np.stack([r[0] for r in ring]), np.stack([r[1] for r in ring])
    vals, key_idx, c0, c1 = fleet(o, keys, m, L, 7 * n + npr + m)
    want = vals.astype(np.float64).sum(axis=0)
    exact = sum(value(o, list(c0[b]), list(c1[b]), s_from[key_idx[b]]) for b in range(m))
    members = list(range(m))
    r0, r1, _ = KS.switch_sum_expect(o, c0, c1, key_idx, [members], wk0, wk1)
    s0, s1 = KS.sum_of_single_switches(o, c0, c1, key_idx, members, wk0, wk1)
    out = {}
    for name, (a0, a1) in (("", (r0[0], r1[0])), ("_single", (s0, s1))):
        y = value(o, list(a0), list(a1), s_to)
        out["key_switch_max" + name] = max(abs(int(v)) for v in y - exact)
        out["slot_error" + name] = float(np.abs(decode(o, y, o.scale) - want).max())
    return dict(op="switch_sum", n=n, primes=npr, level=L, m=m, keys=nkeys, **out)


def parse(arg):
    shape, L, m = arg.split(":")
    n, npr = (int(v) for v in shape.split("x"))
    return n, npr, int(L), int(m)


if __name__ == "__main__":
    pyoracle.build(ref=False)
    rows = []
    for arg in sys.argv[1:] or DEFAULT:
        rows.append(row(*parse(arg)))
        print(json.dumps(rows[-1]), flush=True)
    print("| context (n x np) | level L | records m | keys | largest switch coefficient | worst slot error | "
          "m single switches: coefficient | slot error |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} x {r['primes']} | {r['level']} | {r['m']} | {r['keys']} | {r['key_switch_max']} | "
              f"{r['slot_error']:.1e} | {r['key_switch_max_single']} | {r['slot_error_single']:.1e} |")
