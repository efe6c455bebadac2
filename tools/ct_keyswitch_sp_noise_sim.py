#!/usr/bin/env python3
"""CPU simulation of the special-prime key switch (se_amd_ct_galois_sp_device, se_amd_ct_relin_sp_device): the last
prime of the context, P, belongs to the key, a level-L record (L <= np - 1) is switched with one centred digit per data
prime and the result is divided by P.  Everything is the oracle's primitives and Python / NumPy integers
(tests/ct_model.py holds the definition), no GPU.
  rotation: a fresh record dropped to level L, element 3 (one slot to the left), decoded at the fresh scale Delta with no
            lift and no rescale: the largest coefficient of the key-switch term y' - sigma(y) and the worst slot error
            against the rolled values;
  product:  the square of the dropped record (tensor), relinearised with the special-prime key, rescaled once, decoded
            at Delta^2 / q_{L-1}: the worst slot error against the squared values, and the same with the exact degree-2
            value rescaled by plain rounding, i.e. what the product costs without any key switch;
both with the centred digits of the definition and with canonical digits in [0, q_j) -- a digit of mean q/2 convolved
with the key error is a random walk of that size, which is why the definition centres.  One JSON line per case, then
the table.
The hoisted forms (se_amd_ct_galois_sum_sp_device, se_amd_ct_lintrans_sp_device; hoist_sp_expect of tests/ct_model.py is
their definition), with --hoist:
  moving_sum: a fresh record dropped to level L plus its rotations by the steps 1 .. G in ONE call, decoded at Delta;
  matvec:     the diagonal method on a dim x dim matrix with entries in [-1, 1], diagonals encoded at Delta, NO lift, one
              rescale, decoded at Delta^2 / q_{L-1};
each with the same figures for G single key switches, each rounded on its own, then summed.
The baby-step / giant-step plan with the division by P deferred (se_amd_ct_bsgs_sp_device; bsgs_sp_expect of
tests/ct_model_bsgs_sp.py is its definition), with --bsgs:
  matvec_bsgs: a 16 x 16 matrix with entries in [-1/2, 1/2] as a 4 x 4 plan (six keys), diagonals encoded at Delta, NO
              lift, one rescale, decoded at Delta^2 / q_{L-1}: the worst slot error, and the largest coefficient of what
              the plan adds to the exact weighted sum before the rescale (n2 + 1 = 5 roundings and the key errors).
  python tools/ct_keyswitch_sp_noise_sim.py [--hoist | --bsgs] [4096x3:2 4096x3:1 8192x6:5 4096x2:1 ...]   (n x np : L)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from oracle import pyoracle  # noqa: E402
import vectors as V  # noqa: E402
import ct_model as K  # noqa: E402
from ct_galois_noise_sim import decode, matvec_matrix, mul_plain, rescale, sigma_int, value  # noqa: E402
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


def step_keys(o, sk, s_hat, steps):
    """-> (elts, keys): the special-prime Galois keys of the rotations by `steps`, from the oracle alone."""
    elts = [pow(3, st, 2 * o.n) for st in steps]
    return elts, [K.sp_key(o, sk, K.sigma_rows(o, s_hat[:o.np - 1], g), f"spsim-g{g}") for g in elts]


def single_rotation(o, c0, c1, g, key):
    """One se_amd_ct_galois_sp_device on a record [L][n] -> (out0, out1, (delta_0, delta_1))."""
    r = K.key_switch_sp(o, K.sigma_rows(o, c1, g), *key)
    return K.add_mod(o, K.sigma_rows(o, c0, g), r["ks"][0]), r["ks"][1], r["delta"]


def rounding(o, delta, s_nat):
    """What one division by P adds to the decrypted value: -(delta_0 + delta_1 * s) / P, float64 [n], every coefficient of
    delta_k / P in (-1/2, 1/2]."""
    full = np.convolve(delta[1].astype(np.float64), s_nat.astype(np.float64))
    return -(delta[0].astype(np.float64) + full[:o.n] - np.append(full[o.n:], 0.0)) / float(o.q[o.np - 1])


def rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2)))


def moving_sum(n, npr, L, G):
    """-> dict: x + sum of the rotations by 1 .. G of a fresh record at level L, decoded at Delta: one call of the sum
    form (one rounding), and G single key switches each rounded, then summed ("_single").  rounding_rms: the root mean
    square over the coefficients of what the divisions by P add to the decrypted value."""
    o, sk, s_hat, vals, c0, c1 = setup(n, npr)
    s_nat = K.centred(o.expand_ternary(sk, 0), o.q[0])
    steps = tuple(range(1, G + 1))
    elts, keys = step_keys(o, sk, s_hat, steps)
    c0, c1 = c0[:L], c1[:L]
    y_in = value(o, list(c0), list(c1), s_hat)
    exact, want = y_in.copy(), vals.astype(np.float64)
    for st, g in zip(steps, elts):
        exact = exact + sigma_int(y_in, g)
        want = want + np.roll(vals.astype(np.float64), -st)
    h0, h1, info = K.hoist_sp_expect(o, c0[None], c1[None], elts, keys, w0=1)
    s0, s1, r_single = c0, c1, np.zeros(n)
    for g, key in zip(elts, keys):
        r0, r1, delta = single_rotation(o, c0, c1, g, key)
        s0, s1, r_single = K.add_mod(o, s0, r0), K.add_mod(o, s1, r1), r_single + rounding(o, delta, s_nat)
    out = dict(rounding_rms=rms(rounding(o, info[0]["delta"], s_nat)), rounding_rms_single=rms(r_single))
    for name, (r0, r1) in (("", (h0[0], h1[0])), ("_single", (s0, s1))):
        y = value(o, list(r0), list(r1), s_hat)
        out["key_switch_max" + name] = max(abs(int(v)) for v in y - exact)
        out["slot_error" + name] = float(np.abs(decode(o, y, o.scale) - want).max())
    return dict(op="moving_sum", n=n, primes=npr, level=L, G=G, **out)


def matvec(n, npr, L, dim=8):
    """-> dict: M x by the diagonal method on a fresh record at level L, the dim diagonals encoded at Delta, no lift, one
    rescale, decoded at Delta^2 / q_{L-1}: one call of the linear transform, and dim - 1 single key switches each
    rounded, multiplied by their diagonals and summed ("_single").  The key-switch coefficient and the roundings' share
    (rounding_rms, as in moving_sum; a single key switch's is multiplied by its diagonal) are taken before the rescale."""
    assert dim == 8 and L >= 2                               # the matrix of examples/matvec_roundtrip.c
    o = pyoracle.Oracle(n, npr)
    q = o.q
    sk = V.secret_key(n, seed=5)
    s_hat = np.stack([o.ntt(o.expand_ternary(sk, j), j) for j in range(npr)])
    s_nat = K.centred(o.expand_ternary(sk, 0), q[0])
    x8 = np.random.default_rng(8 * n + npr).uniform(-1.0, 1.0, dim)
    vals = np.tile(x8, n // 2 // dim).astype(np.float32)
    M = matvec_matrix()
    want = np.tile(M @ vals[:dim].astype(np.float64), n // 2 // dim)
    ss, sd = V.bench_seeds(1, first=13)
    x = o.encrypt_sym(vals, ss[0].tobytes(), sd[0].tobytes(), sk)
    c0 = np.stack([np.array(x["c0"][j]) for j in range(L)])
    c1 = np.stack([np.array(x["c1"][j]) for j in range(L)])
    elts, keys = step_keys(o, sk, s_hat, tuple(range(1, dim)))
    k = np.arange(n // 2)
    ok, diag = o.encode_ntt_batch(np.stack([M[k % dim, (k + e) % dim].astype(np.float32) for e in range(dim)]))
    assert ok
    diag = np.stack([np.stack([np.array(d[j]) for j in range(npr)]) for d in diag])    # [dim][np][n], scale Delta
    # what the sum is without any key switch: sum_e d_e . sigma_e(m) per prime on the decrypted record, recombined
    rows = []
    for i in range(L):
        m = o.decrypt(c0[i], c1[i], s_hat[i], i).astype(np.uint64)
        acc = (diag[0, i].astype(np.uint64) * m) % np.uint64(q[i])
        for e, g in enumerate(elts):
            acc = (acc + (diag[e + 1, i].astype(np.uint64) * m[K.src_table(n, g)]) % np.uint64(q[i])) % np.uint64(q[i])
        rows.append(o.intt(acc.astype(np.uint32), i))
    exact = np.array(K.crt_centred(q[:L], rows), dtype=object)
    single0, single1 = np.stack(mul_plain(o, c0, diag[0])), np.stack(mul_plain(o, c1, diag[0]))
    r_single = np.zeros(n)
    for e, (g, key) in enumerate(zip(elts, keys)):
        r0, r1, delta = single_rotation(o, c0, c1, g, key)
        single0 = K.add_mod(o, single0, np.stack(mul_plain(o, r0, diag[e + 1])))
        single1 = K.add_mod(o, single1, np.stack(mul_plain(o, r1, diag[e + 1])))
        d_nat = K.centred(o.intt(diag[e + 1, 0], 0), q[0]).astype(np.float64)      # the plaintext's coefficients
        full = np.convolve(rounding(o, delta, s_nat), d_nat)
        r_single = r_single + full[:n] - np.append(full[n:], 0.0)
    scale = o.scale * o.scale / q[L - 1]
    h0, h1, info = K.hoist_sp_expect(o, c0[None], c1[None], elts, keys, diag[1:], diag[0])
    out = dict(rounding_rms=rms(rounding(o, info[0]["delta"], s_nat)), rounding_rms_single=rms(r_single))
    for name, (r0, r1) in (("", (h0[0], h1[0])), ("_single", (single0, single1))):
        out["key_switch_max" + name] = max(abs(int(v)) for v in value(o, list(r0), list(r1), s_hat) - exact)
        y = value(o, rescale(o, list(r0)), rescale(o, list(r1)), s_hat)
        out["slot_error" + name] = float(np.abs(decode(o, y, scale) - want).max())
    return dict(op="matvec", n=n, primes=npr, level=L, G=dim - 1, log2_scale_after=float(np.log2(scale)), **out)


def matvec_bsgs(n, npr, L, n1=4, n2=4):
    """-> dict: M x for the 16 x 16 matrix of examples/matvec_bsgs_fresh_roundtrip.c on a fresh record at level L through
    the 4 x 4 plan: baby steps 0 .. 3 undivided, the diagonals (encoded at Delta, all np rows) multiplied in, one division
    per giant step 0, 4, 8, 12 and one for their sum, one rescale, decoded at Delta^2 / q_{L-1}."""
    import ct_model_bsgs_sp as KB
    assert L >= 2
    dim = n1 * n2
    o = pyoracle.Oracle(n, npr)
    q = o.q
    sk = V.secret_key(n, seed=5)
    s_hat = np.stack([o.ntt(o.expand_ternary(sk, j), j) for j in range(npr)])
    x16 = np.random.default_rng(16 * n + npr).uniform(-1.0, 1.0, dim)
    vals = np.tile(x16, n // 2 // dim).astype(np.float32)
    M = K.matrix(dim)
    want = np.tile(M @ vals[:dim].astype(np.float64), n // 2 // dim)
    ss, sd = V.bench_seeds(1, first=13)
    x = o.encrypt_sym(vals, ss[0].tobytes(), sd[0].tobytes(), sk)
    c0 = np.stack([np.array(x["c0"][j]) for j in range(L)])
    c1 = np.stack([np.array(x["c1"][j]) for j in range(L)])
    baby = [pow(3, b, 2 * n) for b in range(n1)]
    giant = [pow(3, n1 * g, 2 * n) for g in range(n2)]
    elts, keys = step_keys(o, sk, s_hat, [b for b in range(1, n1)] + [n1 * g for g in range(1, n2)])
    ok, diag = o.encode_ntt_batch(K.matrix_diagonals(M, n))
    assert ok
    diag = np.stack([np.stack([np.array(d[j]) for j in range(npr)]) for d in diag])    # [dim][np][n], scale Delta
    # the exact weighted sum: sum_e d_e . sigma_e(m) per prime on the decrypted record, recombined
    rows = []
    for i in range(L):
        m = o.decrypt(c0[i], c1[i], s_hat[i], i).astype(np.uint64)
        acc = np.zeros(n, dtype=np.uint64)
        for e in range(dim):
            src = K.src_table(n, pow(3, e, 2 * n))
            acc = (acc + (diag[e, i].astype(np.uint64) * m[src]) % np.uint64(q[i])) % np.uint64(q[i])
        rows.append(o.intt(acc.astype(np.uint32), i))
    exact = np.array(K.crt_centred(q[:L], rows), dtype=object)
    r0, r1 = KB.bsgs_sp_expect(K.src_table, o, c0[None], c1[None], baby, giant, diag.reshape(n2, n1, npr, n),
                               dict(zip(elts, keys)))
    scale = o.scale * o.scale / q[L - 1]
    term = value(o, list(r0[0]), list(r1[0]), s_hat) - exact
    y = value(o, rescale(o, list(r0[0])), rescale(o, list(r1[0])), s_hat)
    return dict(op="matvec_bsgs", n=n, primes=npr, level=L, n1=n1, n2=n2, keys=len(elts),
                log2_scale_after=float(np.log2(scale)), key_switch_max=max(abs(int(v)) for v in term),
                slot_error=float(np.abs(decode(o, y, scale) - want).max()))


def parse(arg):
    shape, L = arg.split(":")
    n, npr = (int(v) for v in shape.split("x"))
    return n, npr, int(L)


if __name__ == "__main__":
    pyoracle.build(ref=False)
    rows = []
    if "--bsgs" in sys.argv[1:]:
        for arg in [a for a in sys.argv[1:] if a != "--bsgs"] or ("4096x3:2", "8192x6:5"):
            print(json.dumps(matvec_bsgs(*parse(arg))), flush=True)
        sys.exit(0)
    args = [a for a in sys.argv[1:] if a != "--hoist"]
    if "--hoist" in sys.argv[1:]:
        for arg in args or ("4096x3:2", "8192x6:5"):
            n, npr, L = parse(arg)
            for row in (rotation(n, npr, L), moving_sum(n, npr, L, 7), matvec(n, npr, L)):
                print(json.dumps(row), flush=True)
        sys.exit(0)
    for arg in args or DEFAULT:
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
