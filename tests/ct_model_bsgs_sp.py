"""The host model of the special-prime baby-step / giant-step transform with the division by P deferred: the four entries
and the plan call of include/seal_embedded_amd.h, word for word from their definitions, on top of ct_model (sp_digits,
src_table, centred, permute_diagonals).  NumPy and the oracle only: no torch, no package, no GPU.

Notation: o = Oracle(n, np), p = np - 1, P = o.q[p]; records uint32 [B][L][n], 1 <= L <= np - 1; an EXTENDED record is
[L + 1][n], rows r < L modulo q_r, row L modulo P.  `keys` maps an element to its special-prime key (k0, k1), each uint32
[np - 1][np][n]; element 1 needs none.  `table` is the permutation table function (n, g) -> src, as in ct_model.

    many_ext    out_k[e][b][r] = sum_j F_{j,i_r}[src_e] . k_k^e[j][i_r] (+ (P mod q_r) . c0[b][r][src_e] for k = 0, r < L)
    stack sum   out[g][b][r]   = sum_e (pt[g][e][i_r] mod q_{i_r}) . in[e][b][r]                      i_r = r, or p for r = L
    mod_down    out[i]         = (in[i] - NTT_i(centred(INTT_p(in[L]), P) mod q_i)) . P^-1
    accum_sp    one accumulator over the keyed elements, one delta, one division; the exact addends after it
    bsgs_sp     many_ext(baby) -> stack sum with the pre-rotated diagonals -> mod_down -> accum_sp(giant)
"""
import numpy as np

from ct_model import centred, permute_diagonals, sigma_rows, sp_digits, src_table


def ext_primes(o, L):
    """The prime index of every row of an extended record of level L."""
    return list(range(L)) + [o.np - 1]


def many_ext_expect(table, o, c0, c1, elts, keys):
    """(out0, out1) uint32 [G][B][L+1][n].  The digits are those of c1 itself, taken once."""
    B, L, n = c0.shape
    p = o.np - 1
    P = o.q[p]
    assert 1 <= L <= p and c1.shape == c0.shape
    out0 = np.zeros((len(elts), B, L + 1, n), dtype=np.uint32)
    out1 = np.zeros_like(out0)
    srcs = [table(n, int(g)).astype(np.int64) for g in elts]
    for b in range(B):
        D = sp_digits(o, c1[b])
        for r, i in enumerate(ext_primes(o, L)):
            q = np.uint64(o.q[i])
            pm = np.uint64(P % o.q[i])
            F = []
            for j in range(L):
                f = o.ntt((D[j] % o.q[i]).astype(np.uint32), i).astype(np.uint64)
                if i == j:
                    assert (f == c1[b, j]).all()              # F_{j,j} is c1[b][j] as it lies
                F.append(f)
            for e, (g, src) in enumerate(zip(elts, srcs)):
                if int(g) == 1:
                    if r < L:
                        out0[e, b, r] = (c0[b, r].astype(np.uint64) * pm) % q
                        out1[e, b, r] = (c1[b, r].astype(np.uint64) * pm) % q
                    continue                                   # row L all zero
                k0, k1 = keys[int(g)]
                a0, a1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
                for j in range(L):
                    a0 = (a0 + (F[j][src] * k0[j, i].astype(np.uint64)) % q) % q
                    a1 = (a1 + (F[j][src] * k1[j, i].astype(np.uint64)) % q) % q
                if r < L:
                    a0 = (a0 + (c0[b, r][src].astype(np.uint64) * pm) % q) % q
                out0[e, b, r], out1[e, b, r] = a0, a1
    return out0, out1


def stack_sum_ext_expect(o, stack, pt):
    """stack uint32 [E][B][L+1][n] of extended records, pt [Gout][E][np][n] of any 32-bit words -> [Gout][B][L+1][n]: row
    r < L uses q_r and plaintext row r, row L uses P and plaintext row p."""
    E, B, rows, n = stack.shape
    idx = ext_primes(o, rows - 1)
    assert pt.shape[1] == E and pt.shape[2] == o.np
    qv = np.array([o.q[i] for i in idx], dtype=np.uint64)[None, :, None]
    out = np.zeros((pt.shape[0], B, rows, n), dtype=np.uint32)
    for g in range(pt.shape[0]):
        acc = np.zeros((B, rows, n), dtype=np.uint64)
        for e in range(E):
            acc = (acc + (stack[e].astype(np.uint64) * (pt[g, e][idx].astype(np.uint64)[None] % qv)) % qv) % qv
        out[g] = acc
    return out


def mod_down_expect(o, ext):
    """ext uint32 [..][L+1][n] -> [..][L][n]: the rescale's map with P as the dropped prime."""
    lead, (rows, n) = ext.shape[:-2], ext.shape[-2:]
    L, p = rows - 1, o.np - 1
    P = o.q[p]
    flat = ext.reshape(-1, rows, n)
    out = np.zeros((flat.shape[0], L, n), dtype=np.uint32)
    for c in range(flat.shape[0]):
        delta = centred(o.intt(flat[c, L], p), P)
        for i in range(L):
            q = o.q[i]
            t = o.ntt((delta % q).astype(np.uint32), i).astype(np.uint64)
            diff = (flat[c, i].astype(np.uint64) + np.uint64(q) - t) % np.uint64(q)
            out[c, i] = ((diff * np.uint64(pow(P, -1, q))) % np.uint64(q)).astype(np.uint32)
    return out.reshape(lead + (L, n))


def accum_sp_expect(o, in0, in1, elts, keys):
    """in [G][B][L][n] -> (out0, out1) [B][L][n]: ONE accumulator over the keyed elements, one delta per half, one
    division; sigma_g(a^g) of the keyed elements and both rows of the elements 1 are added after it."""
    G, B, L, n = in0.shape
    p = o.np - 1
    P = o.q[p]
    assert 1 <= L <= p and len(elts) == G
    out0, out1 = np.zeros((B, L, n), dtype=np.uint32), np.zeros((B, L, n), dtype=np.uint32)
    for b in range(B):
        acc = {i: [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)] for i in ext_primes(o, L)}
        add0 = np.zeros((L, n), dtype=np.uint64)
        add1 = np.zeros((L, n), dtype=np.uint64)
        qv = np.array(o.q[:L], dtype=np.uint64)[:, None]
        for s, g in enumerate(int(x) for x in elts):
            if g == 1:
                add0 = (add0 + in0[s, b].astype(np.uint64)) % qv
                add1 = (add1 + in1[s, b].astype(np.uint64)) % qv
                continue
            k0, k1 = keys[g]
            D = sp_digits(o, sigma_rows(o, in1[s, b], g))        # the digits of k_ct_galois_sp: of sigma_g(b^g)
            for i in ext_primes(o, L):
                q = np.uint64(o.q[i])
                for j in range(L):
                    f = o.ntt((D[j] % o.q[i]).astype(np.uint32), i).astype(np.uint64)
                    acc[i][0] = (acc[i][0] + (f * k0[j, i].astype(np.uint64)) % q) % q
                    acc[i][1] = (acc[i][1] + (f * k1[j, i].astype(np.uint64)) % q) % q
            add0 = (add0 + sigma_rows(o, in0[s, b], g).astype(np.uint64)) % qv
        for k, (out, add) in enumerate(((out0, add0), (out1, add1))):
            delta = centred(o.intt(acc[p][k].astype(np.uint32), p), P)
            for i in range(L):
                q = np.uint64(o.q[i])
                t = o.ntt((delta % o.q[i]).astype(np.uint32), i).astype(np.uint64)
                ks = (((acc[i][k] + q - t) % q) * np.uint64(pow(P, -1, o.q[i]))) % q
                out[b, i] = ((ks + add[i]) % q).astype(np.uint32)
    return out0, out1


def bsgs_sp_expect(table, o, c0, c1, baby, giant, diag, keys):
    """The four steps of se_amd_ct_bsgs_sp_device on records [B][L][n] and the caller's diagonals [n2][n1][np][n]."""
    n = c0.shape[2]
    u0, u1 = many_ext_expect(table, o, c0, c1, baby, keys)
    dp = permute_diagonals(table, n, diag, giant)
    v0, v1 = stack_sum_ext_expect(o, u0, dp), stack_sum_ext_expect(o, u1, dp)
    return accum_sp_expect(o, mod_down_expect(o, v0), mod_down_expect(o, v1), giant, keys)


def sp_keys(rng, q, elts, n):
    """Random special-prime keys for the elements other than 1: {elt: (k0, k1)}, each [np - 1][np][n] of words below q_i
    -- the first np - 1 rows of random_keys' blocks, which have 0, 1 and q - 1 among the first words of the first key."""
    from ct_model import random_keys
    keyed = sorted({int(g) for g in elts if int(g) != 1})
    npr = len(q)
    gk0, gk1 = random_keys(rng, q, max(len(keyed), 1), n, npr)
    return {g: (np.ascontiguousarray(gk0[k, :npr - 1]), np.ascontiguousarray(gk1[k, :npr - 1]))
            for k, g in enumerate(keyed)}


__all__ = ["many_ext_expect", "stack_sum_ext_expect", "mod_down_expect", "accum_sp_expect", "bsgs_sp_expect", "sp_keys",
           "ext_primes", "src_table"]
