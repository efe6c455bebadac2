#!/usr/bin/env python3
"""CPU simulation of the noise of a ciphertext product: encrypt two records with slot values uniform in [-1, 1], tensor,
relinearise with 15-bit digits, rescale, decrypt -- all with the oracle's primitives and Python / NumPy integers, no
GPU; the integer helpers are those of the tests' host model, tests/ct_model.py.  Uses the exact identities the GPU tests
assert:
  relin    decrypt(out0, out1) = decrypt3(d0, d1, d2) + sum_r D_r * e_r          (key-switch term, integers)
  rescale  q_last . y' + delta_0 + delta_1 * s = y                               (delta_k = centred last-prime rows)
so only the last-prime column of the relinearised pair is formed.  Prints one JSON line per parameter set: the bound
2 L n (2^15 - 1) E on a coefficient of the key-switch term (E = 21, the support of the error sampler), the largest
coefficient seen, and the slot errors against x (.) y: of the degree-2 value at Delta^2, of the final value at
Delta^2 / q_last, and the part of it that the key-switch term alone contributes.
  python tools/ct_mul_noise_sim.py [4096x3 8192x6 ...]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import pyoracle  # noqa: E402
import vectors as V  # noqa: E402
from ct_model import DIGIT_BITS, centred, crt_centred, negacyclic  # noqa: E402

ERR_SUPPORT = 21


def decode(o, y, scale):
    res = o.fft((y.astype(np.float64) / scale).astype(np.complex128))
    return np.ascontiguousarray(res.real[o.map[:o.n // 2].astype(np.int64)])


def mulmod(a, b, q):
    return ((a.astype(np.uint64) * b.astype(np.uint64)) % np.uint64(q)).astype(np.uint32)


def simulate(n, L):
    o = pyoracle.Oracle(n, L)
    q, last = o.q, L - 1
    sk = V.secret_key(n, seed=5)
    s_hat = [o.ntt(o.expand_ternary(sk, j), j) for j in range(L)]
    s_nat = centred(o.expand_ternary(sk, 0), q[0])
    vals = np.random.default_rng(n + L).uniform(-1.0, 1.0, (2, n // 2)).astype(np.float32)
    ss, sd = V.bench_seeds(2, first=7)
    x, y = (o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk) for b in range(2))
    d0 = [mulmod(x["c0"][j], y["c0"][j], q[j]) for j in range(L)]
    d1 = [((mulmod(x["c0"][j], y["c1"][j], q[j]).astype(np.uint64) + mulmod(x["c1"][j], y["c0"][j], q[j])) %
           np.uint64(q[j])).astype(np.uint32) for j in range(L)]
    d2 = [mulmod(x["c1"][j], y["c1"][j], q[j]) for j in range(L)]
    # the degree-2 value, as integers
    y3 = np.array(crt_centred(q, [o.intt(o.decrypt(d0[j], o.decrypt(d1[j], d2[j], s_hat[j], j), s_hat[j], j), j)
                                  for j in range(L)]), dtype=object)
    # digits, key rows (last-prime column only) and the key-switch term
    a_seeds, e_seeds = V.derive_seeds("sim-a", 2 * L), V.derive_seeds("sim-e", 2 * L)
    ks = np.zeros(n, dtype=np.int64)
    c0l, c1l = d0[last].astype(np.uint64), d1[last].astype(np.uint64)
    ql = np.uint64(q[last])
    for j in range(L):
        c = o.intt(d2[j], j)
        for t in range(2):
            r = 2 * j + t
            dig = (c >> np.uint32(DIGIT_BITS * t)) & np.uint32((1 << DIGIT_BITS) - 1)
            pk0, pk1 = o.gen_pk(sk, a_seeds[r].tobytes(), e_seeds[r].tobytes())
            e_r = centred(o.intt(o.decrypt(pk0[last], pk1[last], s_hat[last], last), last), q[last])
            assert np.abs(e_r).max() <= ERR_SUPPORT
            ks += negacyclic(dig.astype(np.int64), e_r)
            k0 = pk0[last].astype(np.uint64)
            if j == last:
                s2 = (s_hat[last].astype(np.uint64) ** 2) % ql
                k0 = (k0 + (s2 << np.uint64(DIGIT_BITS * t))) % ql
            f = o.ntt(dig, last).astype(np.uint64)
            c0l = (c0l + (f * k0) % ql) % ql
            c1l = (c1l + (f * pk1[last].astype(np.uint64)) % ql) % ql
    y2 = y3 + ks.astype(object)
    delta0 = centred(o.intt(c0l.astype(np.uint32), last), q[last])
    delta1 = centred(o.intt(c1l.astype(np.uint32), last), q[last])
    num = y2 - delta0.astype(object) - negacyclic(delta1, s_nat).astype(object)
    assert all(int(v) % q[last] == 0 for v in num)
    y1 = np.array([int(v) // q[last] for v in num], dtype=object)
    want = vals[0].astype(np.float64) * vals[1].astype(np.float64)
    d2scale = o.scale * o.scale
    return dict(n=n, primes=L, scale_bits=float(np.log2(o.scale)), q_last=q[last],
                key_switch_bound=2 * L * n * ((1 << DIGIT_BITS) - 1) * ERR_SUPPORT,
                key_switch_max=int(np.abs(ks).max()),
                slot_error_degree2=float(np.abs(decode(o, y3, d2scale) - want).max()),
                slot_error_final=float(np.abs(decode(o, y1, d2scale / q[last]) - want).max()),
                slot_error_key_switch_alone=float(np.abs(decode(o, ks.astype(object), d2scale)).max()))


if __name__ == "__main__":
    pyoracle.build(ref=False)
    shapes = sys.argv[1:] or ["4096x2", "4096x3", "8192x6", "16384x6", "16384x13"]
    for sh in shapes:
        n, L = (int(v) for v in sh.split("x"))
        print(json.dumps(simulate(n, L)), flush=True)
