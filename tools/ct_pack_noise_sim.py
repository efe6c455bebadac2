#!/usr/bin/env python3
"""CPU simulation of slot packing (se_amd_ct_pack_sp_device): m fresh records, each with width = slots / m values in
[-1, 1] in its low slots and zero elsewhere, dropped to level L, are packed into ONE record by one call -- record k under
the step -k width, record 0 under the identity, one division by the special prime for the row -- and decoded at the fresh
scale Delta.  Beside it the eager path: m single rotations (se_amd_ct_galois_sp_device, each rounded on its own) and a
modular sum.  Everything is the oracle's primitives and Python / NumPy integers (tests/ct_model_pack.py holds the
definition, the Galois keys come from ct_model.sp_key with target = sigma_g(NTT(s))): the model, not from a device.
  per case: the largest coefficient and the rms of what the packing adds to sum_k sigma_k(decrypted record k) -- the
            key-switch term with its rounding -- and the worst slot error against the concatenation of the m vectors; the
            same three for the eager path ("_eager").
One JSON line per case, then the table.
  python tools/ct_pack_noise_sim.py [4096x3:2:1 4096x3:2:8 4096x3:2:16 8192x6:5:8 ...]   (n x np : L : m)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from oracle import pyoracle  # noqa: E402
import vectors as V  # noqa: E402
import ct_model as K  # noqa: E402
import ct_model_pack as KP  # noqa: E402
from ct_galois_noise_sim import decode, value  # noqa: E402

DEFAULT = ("4096x3:2:1", "4096x3:2:8", "4096x3:2:16", "8192x6:5:8")


def step_element(n, step):
    """se_amd_galois_element: 3^(step mod n/2) mod 2n, a LEFT rotation by a positive step."""
    return pow(3, step % (n // 2), 2 * n)


def short_records(o, sk, m, L, seed):
    """m fresh records with width = slots / m values in [-1, 1] in the low slots, dropped to L primes ->
    (vals float32 [m][n/2], c0, c1 uint32 [m][L][n])."""
    slots = o.n // 2
    width = slots // m
    vals = np.zeros((m, slots), dtype=np.float32)
    vals[:, :width] = np.random.default_rng(seed).uniform(-1.0, 1.0, (m, width)).astype(np.float32)
    ss, sd = V.bench_seeds(m, first=60)
    c0, c1 = [], []
    for b in range(m):
        x = o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk)
        c0.append(np.stack([np.array(x["c0"][j]) for j in range(L)]))   # dropping primes changes neither message nor scale
        c1.append(np.stack([np.array(x["c1"][j]) for j in range(L)]))
    return vals, np.stack(c0), np.stack(c1)


def row(n, npr, L, m):
    """-> dict: m short records packed into one by one call, and by m single rotations and a sum."""
    o = pyoracle.Oracle(n, npr)
    p = npr - 1
    slots = n // 2
    assert slots % m == 0
    width = slots // m
    sk = V.secret_key(n, seed=5)
    s_hat = np.stack([o.ntt(o.expand_ternary(sk, j), j) for j in range(npr)])
    elts = [step_element(n, -width * k) for k in range(m)]
    assert elts[0] == 1
    keys = [None] + [K.sp_key(o, sk, K.sigma_rows(o, s_hat, g)[:p], f"packsim-{g}") for g in elts[1:]]
    vals, c0, c1 = short_records(o, sk, m, L, 11 * n + npr + m)
    want = vals[:, :width].astype(np.float64).reshape(-1)
    exact = sum(V.sigma_coeff(value(o, list(c0[b]), list(c1[b]), s_hat), elts[b]) for b in range(m))
    entries = [(k, k) for k in range(m)]
    r0, r1, _ = KP.pack_expect(o, c0, c1, elts, [entries], keys)
    s0, s1 = KP.sum_of_single_rotations(o, c0, c1, elts, entries, keys)
    out = {}
    for name, (a0, a1) in (("", (r0[0], r1[0])), ("_eager", (s0, s1))):
        y = value(o, list(a0), list(a1), s_hat)
        term = np.array([int(v) for v in y - exact], dtype=np.float64)
        out["key_switch_max" + name] = int(np.abs(term).max())
        out["key_switch_rms" + name] = float(np.sqrt((term * term).mean()))
        out["slot_error" + name] = float(np.abs(decode(o, y, o.scale) - want).max())
    return dict(op="pack", n=n, primes=npr, level=L, m=m, width=width, **out)


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
    print("| context (n x np) | level L | records m | width | one call: largest term | rms | worst slot error | "
          "m rotations and a sum: largest term | rms | worst slot error |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} x {r['primes']} | {r['level']} | {r['m']} | {r['width']} | {r['key_switch_max']} | "
              f"{r['key_switch_rms']:.1f} | {r['slot_error']:.1e} | {r['key_switch_max_eager']} | "
              f"{r['key_switch_rms_eager']:.1f} | {r['slot_error_eager']:.1e} |")
