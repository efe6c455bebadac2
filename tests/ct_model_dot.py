"""The host model of the grouped product sums: se_amd_ct_mul_sum_device and se_amd_ct_dot_sp_device of
include/seal_embedded_amd.h, word for word from their definitions, on top of ct_model (key_switch_sp, add_mod, crt_centred).
NumPy and the oracle only: no torch, no package, no GPU.

Notation: o = Oracle(n, np), p = np - 1; the sides are slabs (a0, a1) [Ba][L][n] and (b0, b1) [Bb][L][n] of uint32; a row
is a list of pairs (ia, ib) (a pair listed twice counts twice); x = record ia of a, y = record ib of b.

    mul sum   T0[g] = sum x0 . y0,   T1[g] = sum (x0 . y1 + x1 . y0),   T2[g] = sum x1 . y1      mod q_j, per element
    dot       out_k[g] = T_k[g] + ks_k, ks the special-prime key switch of d = T2[g] (ONE delta and one division by P per row)
    quotient  (T - delta_0 - delta_1 * s) / P with T = sum_j D_j * e_j, D the digits of T2[g]: ct_model.switch_quotient
"""
import numpy as np

from ct_model import add_mod, crt_centred, key_switch_sp


def csr_pairs(rows):
    """Lists of (ia, ib) -> (row_ptr [G + 1], ia, ib [max(nnz, 1)], nnz)."""
    row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    flat = [pr for r in rows for pr in r] or [(0, 0)]
    nnz = sum(len(r) for r in rows)
    return row_ptr, np.array([a for a, _ in flat], dtype=np.uint32), np.array([b for _, b in flat], dtype=np.uint32), nnz


def mul_sum_expect(o, a0, a1, b0, b1, rows):
    """-> (T0, T1, T2) uint32 [G][L][n].  uint64 arithmetic with a `%` per term: a product of residues is below 2^60 and is
    reduced before it is added."""
    L, n = a0.shape[1], a0.shape[2]
    qv = np.array(o.q[:L], dtype=np.uint64)[:, None]
    T = np.zeros((3, len(rows), L, n), dtype=np.uint64)
    for g, row in enumerate(rows):
        for ia, ib in row:
            x0, x1, y0, y1 = (s.astype(np.uint64) for s in (a0[ia], a1[ia], b0[ib], b1[ib]))
            T[0, g] = (T[0, g] + (x0 * y0) % qv) % qv
            T[1, g] = (T[1, g] + (x0 * y1) % qv) % qv
            T[1, g] = (T[1, g] + (x1 * y0) % qv) % qv
            T[2, g] = (T[2, g] + (x1 * y1) % qv) % qv
    return tuple(T.astype(np.uint32))


def dot_sp_expect(o, a0, a1, b0, b1, rows, k0, k1):
    """-> (out0, out1 uint32 [G][L][n], info): the special-prime relinearisation of mul_sum_expect, row by row; info[g] is
    key_switch_sp's dict for d = T2[g] (ks, delta, D).  An empty row is all zero."""
    T0, T1, T2 = mul_sum_expect(o, a0, a1, b0, b1, rows)
    out0, out1, info = np.zeros_like(T0), np.zeros_like(T1), []
    for g in range(len(rows)):
        r = key_switch_sp(o, T2[g], k0, k1)
        out0[g], out1[g] = add_mod(o, T0[g], r["ks"][0]), add_mod(o, T1[g], r["ks"][1])
        info.append(r)
    return out0, out1, info


def eager_dot_expect(o, a0, a1, b0, b1, rows, k0, k1):
    """What the per-pair path gives: every product relinearised on its own (m roundings), then the modular sum."""
    out0 = np.zeros((len(rows),) + a0.shape[1:], dtype=np.uint32)
    out1 = np.zeros_like(out0)
    for g, row in enumerate(rows):
        for pr in row:
            e0, e1, _ = dot_sp_expect(o, a0, a1, b0, b1, [[pr]], k0, k1)
            out0[g], out1[g] = add_mod(o, out0[g], e0[0]), add_mod(o, out1[g], e1[0])
    return out0, out1


def product_sum(o, ya, yb, row):
    """sum over the row's pairs of the negacyclic products ya[ia] * yb[ib] of integer polynomials, exact: per prime of o
    the NTT-domain products summed mod q_j, then the centred CRT value, which IS the integer sum because
    len(row) . n . max|ya| . max|yb| < Q / 2 (asserted) -> object array [n] of Python ints."""
    Q = 1
    for qj in o.q:
        Q *= qj
    big = lambda y: max(abs(int(v)) for v in y)  # noqa: E731
    assert len(row) * o.n * max(big(ya[a]) for a, _ in row) * max(big(yb[b]) for _, b in row) < Q // 2
    res = lambda y, qj: np.array([int(v) % qj for v in y], dtype=np.uint32)  # noqa: E731
    pts = []
    for j, qj in enumerate(o.q):
        acc = np.zeros(o.n, dtype=np.uint64)
        for ia, ib in row:
            fa, fb = o.ntt(res(ya[ia], qj), j).astype(np.uint64), o.ntt(res(yb[ib], qj), j).astype(np.uint64)
            acc = (acc + (fa * fb) % np.uint64(qj)) % np.uint64(qj)
        pts.append(o.intt(acc.astype(np.uint32), j))
    return np.array(crt_centred(o.q, pts), dtype=object)


__all__ = ["csr_pairs", "mul_sum_expect", "dot_sp_expect", "eager_dot_expect", "product_sum"]
