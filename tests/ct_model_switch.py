"""The host model of the switch-key ring: se_amd_ct_switch_keyed_sp_device and se_amd_ct_switch_sum_keyed_sp_device of
include/seal_embedded_amd.h, word for word from their definitions, on top of ct_model (sp_digits, key_switch_sp, centred,
negacyclic).  NumPy and the oracle only: no torch, no package, no GPU.

Notation: o = Oracle(n, np), p = np - 1, P = o.q[p]; records uint32 [B][L][n], 1 <= L <= np - 1; the ring is (wk0, wk1)
uint32 [K][np - 1][np][n]; key_idx [B]; a row is a list of record indices (a record listed twice counts twice).

    switch       out0[b] = c0[b] + ks_0, out1[b] = ks_1, ks the key switch of c1[b] under ring key key_idx[b]
    switch sum   ACC_k[i] = sum_{b in row} sum_j NTT_i(D_{b,j} mod q_i) . ring[key_idx[b]]_k[j][i], ONE delta_k and one
                 division by P per row, then + sum_{b in row} c0[b] on half 0
    quotient     (T - delta_0 - delta_1 * s_to) / P with T = sum_{b in row} sum_j D_{b,j} * e_{key_idx[b], j}
"""
import numpy as np

import vectors as V
from ct_model import add_mod, centred, key_switch_sp, negacyclic, sp_digits


def switch_expect(o, c0, c1, key_idx, wk0, wk1):
    """Slabs [B][L][n] -> (out0, out1): record b under ring key key_idx[b]."""
    out0, out1 = np.zeros_like(c0), np.zeros_like(c1)
    for b in range(c0.shape[0]):
        k = int(key_idx[b])
        ks0, ks1 = key_switch_sp(o, c1[b], wk0[k], wk1[k])["ks"]
        out0[b], out1[b] = add_mod(o, c0[b], ks0), ks1
    return out0, out1


def switch_sum_expect(o, c0, c1, key_idx, rows, wk0, wk1):
    """Slabs [B][L][n], rows = G lists of record indices -> (out0, out1 uint32 [G][L][n], info), info[g] =
    dict(delta=(delta_0, delta_1) int64 [n], D={b: the digits of record b}); an empty row is all zero (delta 0)."""
    B, L, n = c0.shape
    p = o.np - 1
    P = o.q[p]
    assert 1 <= L <= p and c1.shape == c0.shape
    E = list(range(L)) + [p]
    out0 = np.zeros((len(rows), L, n), dtype=np.uint32)
    out1 = np.zeros_like(out0)
    digits, F = {}, {}                                       # per record, shared by the rows that list it

    def transformed(b, i):
        if (b, i) not in F:
            if b not in digits:
                digits[b] = sp_digits(o, c1[b])
            fs = [o.ntt((digits[b][j] % o.q[i]).astype(np.uint32), i).astype(np.uint64) for j in range(L)]
            if i < L:
                assert (fs[i] == c1[b, i]).all()             # for i = j the factor is c1[b][j] as it lies
            F[(b, i)] = fs
        return F[(b, i)]

    info = []
    for g, row in enumerate(rows):
        acc = {}
        for i in E:
            q = np.uint64(o.q[i])
            a = [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]
            for b in row:
                k = int(key_idx[b])
                for j, f in enumerate(transformed(b, i)):
                    for h, key in enumerate((wk0, wk1)):
                        a[h] = (a[h] + (f * key[k, j, i].astype(np.uint64)) % q) % q
            acc[i] = a
        deltas = []
        for h, out in enumerate((out0, out1)):
            delta = centred(o.intt(acc[p][h].astype(np.uint32), p), P)
            deltas.append(delta)
            for i in range(L):
                q = np.uint64(o.q[i])
                t = o.ntt((delta % o.q[i]).astype(np.uint32), i).astype(np.uint64)
                r = (((acc[i][h] + q - t) % q) * np.uint64(pow(P, -1, o.q[i]))) % q
                if h == 0:
                    for b in row:
                        r = (r + c0[b, i].astype(np.uint64)) % q
                out[g, i] = r.astype(np.uint32)
        info.append(dict(delta=tuple(deltas), D={b: digits[b] for b in row}))
    return out0, out1, info


def sum_of_single_switches(o, c0, c1, key_idx, row, wk0, wk1):
    """What len(row) single switches and a modular sum give (one rounding each): (out0, out1) [L][n]."""
    idx = np.array(row, dtype=np.int64)
    s0, s1 = switch_expect(o, c0[idx], c1[idx], np.asarray(key_idx)[idx], wk0, wk1)
    out0, out1 = np.zeros_like(s0[0]), np.zeros_like(s1[0])
    for a, b in zip(s0, s1):
        out0, out1 = add_mod(o, out0, a), add_mod(o, out1, b)
    return out0, out1


def row_quotient(o, info, row, key_idx, errs, s_nat):
    """(T - delta_0 - delta_1 * s_to) / P of one row of switch_sum_expect, T = sum_{b in row} sum_j D_{b,j} * e_{k_b,j}
    (negacyclic products, integers; errs[k] = the errors of ring key k, key_errors of ct_model): what the switch adds to
    the sum of the records' decrypted values.  Asserts the divisibility.  -> (quotient int64 [n], max |T|)."""
    P = o.q[o.np - 1]
    T = np.zeros(o.n, dtype=np.int64)
    for b in row:
        for Dj, ej in zip(info["D"][b], errs[int(key_idx[b])]):
            T += negacyclic(Dj, ej)                          # below n . 2^29 . 64 < 2^49 per term
    num = T - info["delta"][0] - negacyclic(info["delta"][1], s_nat)
    assert (num % P == 0).all()
    return num // P, int(np.abs(T).max())


def random_ring(rng, q, K, n):
    """(wk0, wk1) uint32 [K][np - 1][np][n] of random words below q_i, with 0, 1 and q_i - 1 among the first words of a
    data column and of column p of key 0 (half 0) and of key K - 1 (half 1)."""
    from ct_model import rand_key
    p = len(q) - 1
    wk0 = np.stack([rand_key(rng, q, n) for _ in range(K)])
    wk1 = np.stack([rand_key(rng, q, n) for _ in range(K)])
    for k in (wk0[0], wk1[K - 1]):
        k[0, 0, :4] = [0, 1, q[0] - 1, q[0] - 1]
        k[0, p, :4] = [0, 1, q[p] - 1, q[p] - 1]
    return wk0, wk1


def ring_seeds(npr, K, label):
    """The (a, e) seed blocks [K][np - 1][64] of K switching keys."""
    rows = K * (npr - 1)
    return (V.derive_seeds(label + "-a", rows).reshape(K, npr - 1, 64),
            V.derive_seeds(label + "-e", rows).reshape(K, npr - 1, 64))


__all__ = ["switch_expect", "switch_sum_expect", "sum_of_single_switches", "row_quotient", "random_ring", "ring_seeds"]
