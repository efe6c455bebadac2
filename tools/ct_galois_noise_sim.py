#!/usr/bin/env python3
"""CPU simulation of the noise of a slot rotation: encrypt a record with slot values uniform in [-1, 1], apply the
automorphism and its key switch with 15-bit digits as se_amd_ct_galois_device defines them, decrypt -- all with the
oracle's primitives and Python / NumPy integers (sigma on rows, the permutation table and the integer helpers are those of
the tests' host model, tests/ct_model.py), no GPU.  The digit key switch has no special prime, so the key-switch term
  decrypt(out0, out1) = sigma(decrypt(c0, c1)) + sum_r D_r * e_r        (D_r: digits of sigma(c1), integers)
is as large as the relinearisation's and a rotation belongs at a raised scale.  Prints one JSON line per parameter set:
the bound 2 L n (2^15 - 1) E on a coefficient of the key-switch term (E = 21, the support of the error sampler), the
largest coefficient seen, and the slot errors against the rolled values of
  - a rotation of the fresh record at Delta (no lift),
  - lift by 2^30, one rotation (step 1), rescale,
  - lift by 2^30, four rotate-and-adds (steps 1, 2, 4, 8: every slot becomes the sum of 16), rescale,
with the largest coefficient before each rescale; and the same for the hoisted form (se_amd_ct_galois_many_device /
se_amd_ct_galois_sum_device), which decomposes c1 itself and permutes the transformed digits, so that
  decrypt(rot0, rot1) = sigma(decrypt(c0, c1)) + sum_r sigma(D_r) * e_r  (D_r: digits of c1, sigma on the integers):
  - its key-switch term for step 1,
  - lift by 2^30, one hoisted rotation (step 1), rescale,
  - lift by 2^30, the record plus its hoisted rotations by 1 .. 7 in one sum (every slot becomes the sum of 8), rescale.
  python tools/ct_galois_noise_sim.py [4096x3 8192x6 ...]
With --lintrans: the weighted sum of examples/matvec_roundtrip.c (se_amd_ct_lintrans_device), y = M x on records that
hold an 8-vector repeated through the slots, M a fixed 8 x 8 matrix with entries in [-1, 1], as the plaintext-weighted sum
of the record and its hoisted rotations by 1 .. 7: diagonal e holds M[k mod 8][(k + e) mod 8] / 2^DIAG_SHIFT encoded at
Delta, so its scale is Delta / 2^DIAG_SHIFT.  One JSON line per parameter set and per bookkeeping (lift bits, diagonal
shift, rescales): the largest coefficient before the first rescale (it must stay below 2^62 for the int64 decrypt of
the stage) and the worst slot error against M x after the rescales.
  python tools/ct_galois_noise_sim.py --lintrans [4096x3 8192x6 ...]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from oracle import pyoracle  # noqa: E402
import vectors as V  # noqa: E402
from ct_model import DIGIT_BITS, centred, crt_centred, sigma_rows, src_table  # noqa: E402
from ct_mul_noise_sim import ERR_SUPPORT, decode  # noqa: E402

LIFT = 1 << 30
STEPS = (1, 2, 4, 8)
WINDOW = tuple(range(1, 8))     # the hoisted sum of 8: the record and its rotations by 1 .. 7


def sigma_int(y, g):
    n = y.shape[0]
    u = (np.arange(n, dtype=np.int64) * g) % (2 * n)
    out = np.zeros_like(y)
    out[u % n] = np.where(u >= n, -y, y)
    return out


def galois_key(o, sk, s_hat, g, label):
    """(gk0, gk1) [2L][L][n]: public key r of the seeds plus the diagonal 2^(15 t) sigma(s_hat) on column j of row 2j + t."""
    L = o.np
    a_seeds, e_seeds = V.derive_seeds(label + "-a", 2 * L), V.derive_seeds(label + "-e", 2 * L)
    sig = sigma_rows(o, s_hat, g)
    gk0, gk1 = [], []
    for r in range(2 * L):
        pk0, pk1 = o.gen_pk(sk, a_seeds[r].tobytes(), e_seeds[r].tobytes())
        k0 = [np.array(pk0[i]) for i in range(L)]
        j, t = r // 2, r % 2
        q = np.uint64(o.q[j])
        k0[j] = ((k0[j].astype(np.uint64) + (sig[j].astype(np.uint64) << np.uint64(DIGIT_BITS * t))) % q).astype(np.uint32)
        gk0.append(k0)
        gk1.append([np.array(pk1[i]) for i in range(L)])
    return gk0, gk1


def galois(o, c0, c1, g, key):
    """The entry's definition on one record of L rows."""
    L = o.np
    gk0, gk1 = key
    p0, p1 = sigma_rows(o, c0, g), sigma_rows(o, c1, g)
    digs = []
    for j in range(L):
        c = o.intt(p1[j], j)
        digs += [c & np.uint32((1 << DIGIT_BITS) - 1), c >> np.uint32(DIGIT_BITS)]
    out0, out1 = [], []
    for i in range(L):
        q = np.uint64(o.q[i])
        a0, a1 = p0[i].astype(np.uint64), np.zeros(o.n, dtype=np.uint64)
        for r, dig in enumerate(digs):
            f = o.ntt(dig, i).astype(np.uint64)
            a0 = (a0 + (f * gk0[r][i].astype(np.uint64)) % q) % q
            a1 = (a1 + (f * gk1[r][i].astype(np.uint64)) % q) % q
        out0.append(a0.astype(np.uint32))
        out1.append(a1.astype(np.uint32))
    return out0, out1


def galois_hoisted(o, c0, c1, elts, keys):
    """The hoisted entries' definition on one record of L rows: the digits of c1 itself, transformed once per output
    prime, then permuted by src_g and multiplied with the key of g, for every g of `elts`.  -> [(rot0, rot1)]."""
    L = o.np
    digs = []
    for j in range(L):
        c = o.intt(c1[j], j)
        digs += [c & np.uint32((1 << DIGIT_BITS) - 1), c >> np.uint32(DIGIT_BITS)]
    F = [[o.ntt(dig, i).astype(np.uint64) for dig in digs] for i in range(L)]
    out = []
    for g, (gk0, gk1) in zip(elts, keys):
        src = src_table(o.n, g)
        r0, r1 = [], []
        for i in range(L):
            q = np.uint64(o.q[i])
            a0, a1 = c0[i][src].astype(np.uint64), np.zeros(o.n, dtype=np.uint64)
            for r, f in enumerate(F[i]):
                a0 = (a0 + (f[src] * gk0[r][i].astype(np.uint64)) % q) % q
                a1 = (a1 + (f[src] * gk1[r][i].astype(np.uint64)) % q) % q
            r0.append(a0.astype(np.uint32))
            r1.append(a1.astype(np.uint32))
        out.append((r0, r1))
    return out


def rescale(o, rows):
    L = len(rows)
    q_last = o.q[L - 1]
    delta = centred(o.intt(rows[L - 1], L - 1), q_last)
    out = []
    for j in range(L - 1):
        q = o.q[j]
        t = o.ntt((delta % q).astype(np.uint32), j).astype(np.uint64)
        diff = (rows[j].astype(np.uint64) + np.uint64(q) - t) % np.uint64(q)
        out.append(((diff * np.uint64(pow(q_last, -1, q))) % np.uint64(q)).astype(np.uint32))
    return out


def value(o, c0, c1, s_hat):
    """The centred integer c0 + c1 s over the primes of the rows."""
    L = len(c0)
    pts = [o.intt(o.decrypt(c0[j], c1[j], s_hat[j], j), j) for j in range(L)]
    return np.array(crt_centred(o.q[:L], pts), dtype=object)


def add_rows(o, a, b):
    return [((a[j].astype(np.uint64) + b[j]) % np.uint64(o.q[j])).astype(np.uint32) for j in range(len(a))]


def simulate(n, L):
    o = pyoracle.Oracle(n, L)
    q, last = o.q, L - 1
    sk = V.secret_key(n, seed=5)
    s_hat = [o.ntt(o.expand_ternary(sk, j), j) for j in range(L)]
    vals = np.random.default_rng(n + L).uniform(-1.0, 1.0, n // 2).astype(np.float32)
    ss, sd = V.bench_seeds(1, first=11)
    x = o.encrypt_sym(vals, ss[0].tobytes(), sd[0].tobytes(), sk)
    c0, c1 = [np.array(x["c0"][j]) for j in range(L)], [np.array(x["c1"][j]) for j in range(L)]
    keys = {s: galois_key(o, sk, s_hat, pow(3, s, 2 * n), f"gsim-{s}") for s in sorted(set(STEPS + WINDOW))}
    want1 = np.roll(vals.astype(np.float64), -1)
    g1 = pow(3, 1, 2 * n)
    # no lift: the key-switch term drowns a message at Delta
    r0, r1 = galois(o, c0, c1, g1, keys[1])
    y_in, y_out = value(o, c0, c1, s_hat), value(o, r0, r1, s_hat)
    ks = y_out - sigma_int(y_in, g1)
    err_plain = float(np.abs(decode(o, y_out, o.scale) - want1).max())
    # lift by 2^30, one rotation, rescale
    lift = lambda rows: [((rows[j].astype(np.uint64) * np.uint64(LIFT)) % np.uint64(q[j])).astype(np.uint32) for j in range(L)]
    l0, l1 = lift(c0), lift(c1)
    r0, r1 = galois(o, l0, l1, g1, keys[1])
    big_one = max(abs(int(v)) for v in value(o, r0, r1, s_hat))
    scale = o.scale * LIFT / q[last]
    y = value(o, rescale(o, r0), rescale(o, r1), s_hat)
    err_one = float(np.abs(decode(o, y, scale) - want1).max())
    # lift, four rotate-and-adds, rescale: slot i becomes the sum of the slots i .. i + 15
    a0, a1 = l0, l1
    want = vals.astype(np.float64)
    for s in STEPS:
        r0, r1 = galois(o, a0, a1, pow(3, s, 2 * n), keys[s])
        a0, a1 = add_rows(o, a0, r0), add_rows(o, a1, r1)
        want = want + np.roll(want, -s)
    big_sum = max(abs(int(v)) for v in value(o, a0, a1, s_hat))
    y = value(o, rescale(o, a0), rescale(o, a1), s_hat)
    err_sum = float(np.abs(decode(o, y, scale) - want).max())
    # the hoisted form: step 1 without a lift (its key-switch term), lifted and rescaled, and the sum of 8 in one pass
    (h0, h1), = galois_hoisted(o, c0, c1, [g1], [keys[1]])
    ks_h = value(o, h0, h1, s_hat) - sigma_int(y_in, g1)
    (h0, h1), = galois_hoisted(o, l0, l1, [g1], [keys[1]])
    big_h_one = max(abs(int(v)) for v in value(o, h0, h1, s_hat))
    y = value(o, rescale(o, h0), rescale(o, h1), s_hat)
    err_h_one = float(np.abs(decode(o, y, scale) - want1).max())
    a0, a1 = l0, l1
    want = vals.astype(np.float64)
    for s, (h0, h1) in zip(WINDOW, galois_hoisted(o, l0, l1, [pow(3, s, 2 * n) for s in WINDOW], [keys[s] for s in WINDOW])):
        a0, a1 = add_rows(o, a0, h0), add_rows(o, a1, h1)
        want = want + np.roll(vals.astype(np.float64), -s)
    big_h_sum = max(abs(int(v)) for v in value(o, a0, a1, s_hat))
    y = value(o, rescale(o, a0), rescale(o, a1), s_hat)
    err_h_sum = float(np.abs(decode(o, y, scale) - want).max())
    hoisted = dict(key_switch_max=max(abs(int(v)) for v in ks_h),
                   slot_error_lift_rotate_rescale=err_h_one, log2_max_coeff_one=float(np.log2(big_h_one)),
                   slot_error_lift_sum_of_8_rescale=err_h_sum, log2_max_coeff_sum_of_8=float(np.log2(big_h_sum)))
    return dict(n=n, primes=L, hoisted=hoisted, scale_bits=float(np.log2(o.scale)), q_last=q[last],
                key_switch_bound=2 * L * n * ((1 << DIGIT_BITS) - 1) * ERR_SUPPORT,
                key_switch_max=max(abs(int(v)) for v in ks),
                slot_error_no_lift=err_plain,
                slot_error_lift_rotate_rescale=err_one, log2_max_coeff_one=float(np.log2(big_one)),
                slot_error_lift_four_rotate_adds_rescale=err_sum, log2_max_coeff_four=float(np.log2(big_sum)))


MATVEC_DIM = 8
# (lift bits, diagonal shift, rescales): the example's choice first, then the neighbours that show why
MATVEC_BOOKS = ((18, 8, 1), (30, 0, 2), (13, 8, 1), (18, 0, 1), (9, 0, 1))


def matvec_matrix():
    """The example's fixed matrix: M[r][c] = ((7 r + 3 c + 1) mod 17 - 8) / 8, entries in [-1, 1]."""
    r, c = np.meshgrid(np.arange(MATVEC_DIM), np.arange(MATVEC_DIM), indexing="ij")
    return ((7 * r + 3 * c + 1) % 17 - 8) / 8.0


def mul_plain(o, rows, pt):
    return [((rows[j].astype(np.uint64) * pt[j].astype(np.uint64)) % np.uint64(o.q[j])).astype(np.uint32)
            for j in range(len(rows))]


def simulate_lintrans(n, L, books=MATVEC_BOOKS):
    """-> one dict per bookkeeping.  The keys, the record and the hoisted rotations of a lift are shared."""
    o = pyoracle.Oracle(n, L)
    q = o.q
    sk = V.secret_key(n, seed=5)
    s_hat = [o.ntt(o.expand_ternary(sk, j), j) for j in range(L)]
    rng = np.random.default_rng(8 * n + L)
    x8 = rng.uniform(-1.0, 1.0, MATVEC_DIM)
    vals = np.tile(x8, n // 2 // MATVEC_DIM).astype(np.float32)
    M = matvec_matrix()
    want = np.tile(M @ vals[:MATVEC_DIM].astype(np.float64), n // 2 // MATVEC_DIM)
    ss, sd = V.bench_seeds(1, first=13)
    x = o.encrypt_sym(vals, ss[0].tobytes(), sd[0].tobytes(), sk)
    c0, c1 = [np.array(x["c0"][j]) for j in range(L)], [np.array(x["c1"][j]) for j in range(L)]
    steps = tuple(range(1, MATVEC_DIM))
    elts = [pow(3, s, 2 * n) for s in steps]
    keys = [galois_key(o, sk, s_hat, g, f"gsim-{s}") for s, g in zip(steps, elts)]
    k = np.arange(n // 2)
    out = []
    for lift_bits, shift, rescales in books:
        lift = lambda rows: [((rows[j].astype(np.uint64) << np.uint64(lift_bits)) % np.uint64(q[j])).astype(np.uint32)
                             for j in range(L)]
        l0, l1 = lift(c0), lift(c1)
        rots = [(l0, l1)] + galois_hoisted(o, l0, l1, elts, keys)
        a0 = a1 = None
        for e, (r0, r1) in enumerate(rots):
            d = (M[k % MATVEC_DIM, (k + e) % MATVEC_DIM] / float(1 << shift)).astype(np.float32)
            ok, pt = o.encode_ntt_batch(d[None, :])
            assert ok
            t0, t1 = mul_plain(o, r0, pt[0]), mul_plain(o, r1, pt[0])
            a0, a1 = (t0, t1) if a0 is None else (add_rows(o, a0, t0), add_rows(o, a1, t1))
        big = max(abs(int(v)) for v in value(o, a0, a1, s_hat))
        scale = o.scale * float(1 << lift_bits) * o.scale / float(1 << shift)
        for r in range(rescales):
            scale /= q[L - 1 - r]
            a0, a1 = rescale(o, a0), rescale(o, a1)
        err = float(np.abs(decode(o, value(o, a0, a1, s_hat), scale) - want).max())
        out.append(dict(n=n, primes=L, lift_bits=lift_bits, diag_shift=shift, rescales=rescales,
                        log2_max_coeff_before_rescale=float(np.log2(float(big))), fits_int64_stage=big < 2 ** 62,
                        log2_final_scale=float(np.log2(scale)), slot_error=err))
    return out


if __name__ == "__main__":
    pyoracle.build(ref=False)
    args = [a for a in sys.argv[1:] if a != "--lintrans"]
    shapes = args or ["4096x3", "8192x6"]
    for sh in shapes:
        n, L = (int(v) for v in sh.split("x"))
        if "--lintrans" in sys.argv[1:]:
            for row in simulate_lintrans(n, L):
                print(json.dumps(row), flush=True)
        else:
            print(json.dumps(simulate(n, L)), flush=True)
