#!/usr/bin/env python3
"""CPU simulation of the encrypted inner product (se_amd_ct_dot_sp_device): m + m fresh records with slot values uniform
in [-1, 1] under one key, dropped to level L, sum_k x_k . y_k by ONE key switch of the summed tensor, one rescale, decoded
at Delta^2 / q_{L-1}.  Everything is the oracle's primitives and Python / NumPy integers (tests/ct_model_dot.py holds the
definition, the relinearisation key comes from ct_model.sp_key with target = s_hat^2), no GPU.
  row of m: the worst slot error against the float64 inner product, the largest coefficient before the rescale (the range
            rule: it must stay below Q_L / 2), the largest coefficient of what the key switch adds to the exact product sum,
            and the root mean square of what the division(s) by P add to the decrypted value (rounding_rms) -- each for the
            one-call form (one rounding) and for the eager path, m products relinearised on their own and summed
            ("_eager", m roundings).
One JSON line per case, then the table.
  python tools/ct_dot_noise_sim.py [4096x3:2:1 4096x3:2:8 4096x3:2:16 8192x6:5:8 ...]   (n x np : L : m)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from oracle import pyoracle  # noqa: E402
import vectors as V  # noqa: E402
import ct_model as K  # noqa: E402
import ct_model_dot as KD  # noqa: E402
from ct_galois_noise_sim import decode, rescale, value  # noqa: E402
from ct_keyswitch_sp_noise_sim import rms, rounding  # noqa: E402

DEFAULT = ("4096x3:2:1", "4096x3:2:8", "4096x3:2:16", "8192x6:5:8")


def row(n, npr, L, m):
    """-> dict: one row of m pairs of fresh records, one call and the eager path."""
    o = pyoracle.Oracle(n, npr)
    sk = V.secret_key(n, seed=5)
    s_hat = np.stack([o.ntt(o.expand_ternary(sk, j), j) for j in range(npr)])
    s_nat = K.centred(o.expand_ternary(sk, 0), o.q[0])
    sq = np.stack([((s_hat[j].astype(np.uint64) ** 2) % np.uint64(o.q[j])).astype(np.uint32) for j in range(npr - 1)])
    k0, k1 = K.sp_key(o, sk, sq, "dotsim")
    vals = np.random.default_rng(11 * n + npr + m).uniform(-1.0, 1.0, (2 * m, n // 2)).astype(np.float32)
    ss, sd = V.bench_seeds(2 * m, first=60)
    recs = [o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk) for b in range(2 * m)]
    side = lambda lo, hi, c: np.stack([np.stack([np.array(r[c][j]) for j in range(L)]) for r in recs[lo:hi]])  # noqa: E731
    a0, a1, b0, b1 = side(0, m, "c0"), side(0, m, "c1"), side(m, 2 * m, "c0"), side(m, 2 * m, "c1")
    pairs = [(k, k) for k in range(m)]
    want = (vals[:m].astype(np.float64) * vals[m:].astype(np.float64)).sum(axis=0)
    ya = [value(o, list(a0[k]), list(a1[k]), s_hat) for k in range(m)]
    yb = [value(o, list(b0[k]), list(b1[k]), s_hat) for k in range(m)]
    exact = KD.product_sum(o, ya, yb, pairs)
    scale = o.scale * o.scale / o.q[L - 1]
    QL = 1
    for qj in o.q[:L]:
        QL *= qj
    d0, d1, info = KD.dot_sp_expect(o, a0, a1, b0, b1, [pairs], k0, k1)
    e0, e1 = KD.eager_dot_expect(o, a0, a1, b0, b1, [pairs], k0, k1)
    r_eager = np.zeros(n)
    for pr in pairs:
        r_eager = r_eager + rounding(o, KD.dot_sp_expect(o, a0, a1, b0, b1, [[pr]], k0, k1)[2][0]["delta"], s_nat)
    out = dict(rounding_rms=rms(rounding(o, info[0]["delta"], s_nat)), rounding_rms_eager=rms(r_eager))
    for name, (r0, r1) in (("", (d0[0], d1[0])), ("_eager", (e0[0], e1[0]))):
        y = value(o, list(r0), list(r1), s_hat)
        big = max(abs(int(v)) for v in y)
        assert big < QL // 2
        out["log2_max_coefficient" + name] = float(np.log2(float(big)))
        out["key_switch_max" + name] = max(abs(int(v)) for v in y - exact)
        z = value(o, rescale(o, list(r0)), rescale(o, list(r1)), s_hat)
        out["slot_error" + name] = float(np.abs(decode(o, z, scale) - want).max())
    return dict(op="dot_sp", n=n, primes=npr, level=L, m=m, log2_half_QL=float(np.log2(float(QL // 2))), **out)


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
    print("| context (n x np) | level L | pairs m | log2 largest coefficient | key-switch coefficient | rounding rms | "
          "worst slot error | eager: key-switch coefficient | rounding rms | slot error |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} x {r['primes']} | {r['level']} | {r['m']} | {r['log2_max_coefficient']:.1f} | "
              f"{r['key_switch_max']} | {r['rounding_rms']:.2f} | {r['slot_error']:.1e} | {r['key_switch_max_eager']} | "
              f"{r['rounding_rms_eager']:.2f} | {r['slot_error_eager']:.1e} |")
