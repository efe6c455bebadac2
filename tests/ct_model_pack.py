"""The host model of slot packing: se_amd_ct_pack_sp_device of include/seal_embedded_amd.h, word for word from its
definition, on top of ct_model (sp_digits, key_switch_sp, sigma_rows, centred, negacyclic, add_mod).  NumPy and the oracle
only: no torch, no package, no GPU.

Notation: o = Oracle(n, np), p = np - 1, P = o.q[p]; records uint32 [B][L][n], 1 <= L <= np - 1; elts the call's element
list; keys[e] = the special-prime key (k0, k1) uint32 [np - 1][np][n] of elts[e] (anything, None for instance, for the
identity, which needs none); an entry is a pair (record index, element index) and a row a list of entries (an entry
listed twice counts twice).

    pack         ACC_h[i] = sum_{k in row, elt_k != 1} sum_j NTT_i(sigma_k(D_{k,j}) mod q_i) . k_h^{e_k}[j][i], ONE delta_h
                 and one division by P per row, then + sum_k sigma_k(c0[b_k]) on half 0 and + sum_{elt_k = 1} c1[b_k] on
                 half 1
    quotient     (T - delta_0 - delta_1 * s) / P with T = sum_{k in row, elt_k != 1} sum_j sigma_k(D_{k,j}) * e^{e_k}_j
"""
import numpy as np

from ct_model import add_mod, centred, key_switch_sp, negacyclic, sigma_rows, sp_digits
from vectors import sigma_coeff


def csr_entries(rows):
    """Rows of (record, element index) pairs -> (row_ptr [G + 1], idx, eidx [max(nnz, 1)] uint32, nnz)."""
    row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    flat = [e for r in rows for e in r]
    pad = [(0, 0)] * (not flat)
    idx = np.array([b for b, _ in flat + pad], dtype=np.uint32)
    eidx = np.array([e for _, e in flat + pad], dtype=np.uint32)
    return row_ptr, idx, eidx, len(flat)


def pack_expect(o, c0, c1, elts, entries_rows, keys):
    """Slabs [B][L][n], entries_rows = G lists of (record, element index) -> (out0, out1 uint32 [G][L][n], info), info[g]
    = dict(delta=(delta_0, delta_1) int64 [n], D=[per entry of the row: the digits sigma_k(D_{k,j}) int64 [L][n], None for
    an identity entry]); an empty row is all zero (delta 0)."""
    B, L, n = c0.shape
    p = o.np - 1
    P = o.q[p]
    assert 1 <= L <= p and c1.shape == c0.shape and len(keys) == len(elts)
    E = list(range(L)) + [p]
    out0 = np.zeros((len(entries_rows), L, n), dtype=np.uint32)
    out1 = np.zeros_like(out0)
    digits, F, rot0 = {}, {}, {}                               # per (record, element), shared by the rows that list it

    def sigma_digits(b, g):
        if (b, g) not in digits:
            digits[(b, g)] = [sigma_coeff(d, g) for d in sp_digits(o, c1[b])]
        return digits[(b, g)]

    def transformed(b, g, i):
        if (b, g, i) not in F:
            fs = [o.ntt((d % o.q[i]).astype(np.uint32), i).astype(np.uint64) for d in sigma_digits(b, g)]
            if i < L:                                        # for i = j the factor is sigma_k(c1[b][j]) as it lies
                row = o.ntt(sigma_coeff(o.intt(c1[b, i], i), g, o.q[i]), i)
                assert (fs[i] == row).all()
            F[(b, g, i)] = fs
        return F[(b, g, i)]

    def rotated_c0(b, g):
        if (b, g) not in rot0:
            rot0[(b, g)] = c0[b] if g == 1 else sigma_rows(o, c0[b], g)
        return rot0[(b, g)]

    info = []
    for r, row in enumerate(entries_rows):
        acc = {}
        for i in E:
            q = np.uint64(o.q[i])
            a = [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]
            for b, e in row:
                g = int(elts[e])
                if g == 1:
                    continue
                for j, f in enumerate(transformed(b, g, i)):
                    for h in (0, 1):
                        a[h] = (a[h] + (f * keys[e][h][j, i].astype(np.uint64)) % q) % q
            acc[i] = a
        deltas = []
        for h, out in enumerate((out0, out1)):
            delta = centred(o.intt(acc[p][h].astype(np.uint32), p), P)
            deltas.append(delta)
            rows = []
            for i in range(L):
                q = np.uint64(o.q[i])
                t = o.ntt((delta % o.q[i]).astype(np.uint32), i).astype(np.uint64)
                rows.append(((((acc[i][h] + q - t) % q) * np.uint64(pow(P, -1, o.q[i]))) % q).astype(np.uint32))
            res = np.stack(rows)
            for b, e in row:
                g = int(elts[e])
                if h == 0:
                    res = add_mod(o, res, rotated_c0(b, g))
                elif g == 1:
                    res = add_mod(o, res, c1[b])
            out[r] = res
        info.append(dict(delta=tuple(deltas),
                         D=[None if int(elts[e]) == 1 else sigma_digits(b, int(elts[e])) for b, e in row]))
    return out0, out1, info


def pack_row_quotient(o, info, row, errs, s_nat):
    """(T - delta_0 - delta_1 * s) / P of one row of pack_expect, T = sum_{k in row, elt_k != 1} sum_j sigma_k(D_{k,j}) *
    e^{e_k}_j (negacyclic products, integers; errs[e] = the errors of the key of element e, key_errors of ct_model): what
    the packing adds to sum_k sigma_k(decryption of record k).  Asserts the divisibility.
    -> (quotient int64 [n], max |T|)."""
    P = o.q[o.np - 1]
    T = np.zeros(o.n, dtype=np.int64)
    for (b, e), D in zip(row, info["D"]):
        if D is None:
            continue
        for Dj, ej in zip(D, errs[e]):
            T += negacyclic(Dj, ej)                          # below n . 2^29 . 64 < 2^49 per term
    num = T - info["delta"][0] - negacyclic(info["delta"][1], s_nat)
    assert (num % P == 0).all()
    return num // P, int(np.abs(T).max())


def sum_of_single_rotations(o, c0, c1, elts, row, keys):
    """What len(row) single calls of se_amd_ct_galois_sp_device (the record itself for the identity) and a modular sum
    give, one rounding each: (out0, out1) [L][n]."""
    from ct_model import galois_sp_expect
    out0, out1 = np.zeros_like(c0[0]), np.zeros_like(c1[0])
    for b, e in row:
        g = int(elts[e])
        t0, t1 = (c0[b:b + 1], c1[b:b + 1]) if g == 1 else galois_sp_expect(o, c0[b:b + 1], c1[b:b + 1], g, *keys[e])
        out0, out1 = add_mod(o, out0, t0[0]), add_mod(o, out1, t1[0])
    return out0, out1


def single_deltas(o, c1, elts, row, keys):
    """(delta_0, delta_1) of every rotated entry of a row switched on its own -> list of pairs of int64 [n]."""
    return [key_switch_sp(o, sigma_rows(o, c1[b], int(elts[e])), *keys[e])["delta"]
            for b, e in row if int(elts[e]) != 1]


__all__ = ["csr_entries", "pack_expect", "pack_row_quotient", "sum_of_single_rotations", "single_deltas"]
