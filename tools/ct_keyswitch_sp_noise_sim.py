#!/usr/bin/env python3
"""CPU simulation of the special-prime key switch (se_amd_ct_galois_sp_device, se_amd_ct_relin_sp_device): the last
prime of the context, P, belongs to the key, a level-L record (L <= np - 1) is switched with one centred digit per data
prime and the result is divided by P.  Everything is the oracle's primitives and Python / NumPy integers
(tests/keyswitch_sp_support.py holds the definition), no GPU.
  rotation: a fresh record dropped to level L, element 3 (one slot to the left), decoded at the fresh scale Delta with no
            lift and no rescale: the largest coefficient of the key-switch term y' - sigma(y) and the worst slot error
            against the rolled values;
  product:  the square of the dropped record (tensor), relinearised with the special-prime key, rescaled once, decoded
            at Delta^2 / q_{L-1}: the worst slot error against the squared values, and the same with the exact degree-2
            value rescaled by plain rounding, i.e. what the product costs without any key switch;
both with the centred digits of the definition and with canonical digits in [0, q_j) -- a digit of mean q/2 convolved
with the key error is a random walk of that size, which is why the definition centres.  One JSON line per case, then
the table.
  python tools/ct_keyswitch_sp_noise_sim.py [4096x3:2 4096x3:1 8192x6:5 4096x2:1 ...]      (n x np : L)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from oracle import pyoracle  # noqa: E402
import vectors as V  # noqa: E402
import keyswitch_sp_support as K  # noqa: E402
from ct_galois_noise_sim import decode, rescale, sigma_int, value  # noqa: E402
from ct_mul_noise_sim import mulmod  # noqa: E402

DEFAULT = ("4096x3:2", "4096x3:1", "8192x6:5", "4096x2:1")


def setup(n, npr):
    o = pyoracle.Oracle(n, npr)
    sk = V.secret_key(n, seed=5)
    s_hat = np.stack([o.ntt(o.expand_ternary(sk, j), j) for j in range(npr)])
    vals = np.random.default_rng(n + npr).uniform(-1.0, 1.0, n // 2).astype(np.float32)
    ss, sd = V.bench_seeds(1, first=11)
    x = o.encrypt_sym(vals, ss[0].tobytes(), sd[0].tobytes(), sk)
    c0 = np.stack([np.array(x["c0"][j]) for j in range(npr)])
    c1 = np.stack([np.array(x["c1"][j]) for j in range(npr)])
    return o, sk, s_hat, vals, c0, c1


def rotation(n, npr, L, centre=True, step=1):
    """-> dict: the key-switch term and the slot error of one rotation of a fresh record at level L."""
    o, sk, s_hat, vals, c0, c1 = setup(n, npr)
    g = pow(3, step, 2 * n)
    k0, k1 = K.sp_key(o, sk, K.sigma_rows(o, s_hat[:npr - 1], g), f"spsim-g{g}")
    c0, c1 = c0[:L], c1[:L]                                    # dropping primes changes neither message nor scale
    ks0, ks1 = K.key_switch_sp(o, K.sigma_rows(o, c1, g), k0, k1, centre)["ks"]
    r0 = K.add_mod(o, K.sigma_rows(o, c0, g), ks0)
    y_in, y_out = value(o, list(c0), list(c1), s_hat), value(o, list(r0), list(ks1), s_hat)
    term = y_out - sigma_int(y_in, g)
    want = np.roll(vals.astype(np.float64), -step)
    return dict(op="rotation", n=n, primes=npr, level=L, digits="centred" if centre else "canonical",
                key_switch_max=max(abs(int(v)) for v in term),
                slot_error=float(np.abs(decode(o, y_out, o.scale) - want).max()))


def product(n, npr, L, centre=True):
    """-> dict: the square of a fresh record at level L through tensor, relin_sp and one rescale."""
    o, sk, s_hat, vals, c0, c1 = setup(n, npr)
    q = o.q
    k0, k1 = K.sp_key(o, sk, np.stack([mulmod(s_hat[j], s_hat[j], q[j]) for j in range(npr - 1)]), "spsim-relin")
    c0, c1 = c0[:L], c1[:L]
    d0 = np.stack([mulmod(c0[j], c0[j], q[j]) for j in range(L)])
    d1 = np.stack([((2 * mulmod(c0[j], c1[j], q[j]).astype(np.uint64)) % np.uint64(q[j])).astype(np.uint32) for j in range(L)])
    d2 = np.stack([mulmod(c1[j], c1[j], q[j]) for j in range(L)])
    ks0, ks1 = K.key_switch_sp(o, d2, k0, k1, centre)["ks"]
    r0, r1 = K.add_mod(o, d0, ks0), K.add_mod(o, d1, ks1)
    want = vals.astype(np.float64) ** 2
    scale = o.scale * o.scale / q[L - 1]
    y = value(o, rescale(o, list(r0)), rescale(o, list(r1)), s_hat)
    # the degree-2 value itself divided by q_{L-1} and rounded: the product's own noise, no key switch in it
    y3 = value(o, list(d0), [o.decrypt(d1[j], d2[j], s_hat[j], j) for j in range(L)], s_hat)
    y3r = np.array([(2 * int(v) + q[L - 1]) // (2 * q[L - 1]) for v in y3], dtype=object)
    return dict(op="product", n=n, primes=npr, level=L, digits="centred" if centre else "canonical",
                log2_scale_after=float(np.log2(scale)),
                slot_error=float(np.abs(decode(o, y, scale) - want).max()),
                slot_error_without_key_switch=float(np.abs(decode(o, y3r, scale) - want).max()))


def parse(arg):
    shape, L = arg.split(":")
    n, npr = (int(v) for v in shape.split("x"))
    return n, npr, int(L)


if __name__ == "__main__":
    pyoracle.build(ref=False)
    rows = []
    for arg in sys.argv[1:] or DEFAULT:
        n, npr, L = parse(arg)
        for centre in (True, False):
            rows.append(rotation(n, npr, L, centre))
            print(json.dumps(rows[-1]), flush=True)
            if L >= 2:                                         # the product's rescale needs a prime to drop
                rows.append(product(n, npr, L, centre))
                print(json.dumps(rows[-1]), flush=True)
    print("| op | context (n x np) | level L | digits | largest key-switch coefficient | worst slot error |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['op']} | {r['n']} x {r['primes']} | {r['level']} | {r['digits']} | {r.get('key_switch_max', '')} | "
              f"{r['slot_error']:.1e} |")
