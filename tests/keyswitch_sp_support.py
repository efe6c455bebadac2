"""The special-prime key switch as its definition states it, from the oracle's transforms and NumPy / Python integers:
what tests/test_gpu_ct_keyswitch_sp.py and tests/test_ct_keyswitch_sp_build.py compare the entries against and what
tools/ct_keyswitch_sp_noise_sim.py simulates with.  Nothing here touches the GPU or the library.

Notation: o = Oracle(n, np) of the CONTEXT, p = np - 1 the special prime's index, P = o.q[p]; records have L <= np - 1
rows; a key is (k0, k1), uint32 [np - 1][np][n] each.
"""
import numpy as np

import vectors as V
from vectors import sigma_coeff


def centred(x, q):
    """canonical residues -> int64 representatives in (-q/2, q/2]  (q odd)."""
    x = x.astype(np.int64)
    return np.where(x > q // 2, x - q, x)


def negacyclic(a, s):
    """a * s mod (x^n + 1) in int64 (the callers keep every sum below 2^62)."""
    n = a.shape[0]
    full = np.convolve(a, s)
    res = full[:n].copy()
    res[:n - 1] -= full[n:]
    return res


def sigma_rows(o, rows, g):
    """sigma_g on NTT-form rows [L][n] through the coefficient domain (o.intt, sigma_coeff, o.ntt)."""
    return np.stack([o.ntt(sigma_coeff(o.intt(rows[j], j), g, o.q[j]), j) for j in range(len(rows))])


def sigma_slab(o, slab, g):
    return np.stack([sigma_rows(o, rec, g) for rec in slab])


def sp_digits(o, d, centre=True):
    """D_j of a level-L row polynomial d [L][n]: the natural-order coefficients of row j, centred (the definition) or
    canonical in [0, q_j) (the variant the noise tool compares against) -> int64 [L][n]."""
    out = []
    for j in range(d.shape[0]):
        c = o.intt(d[j], j)
        out.append(centred(c, o.q[j]) if centre else c.astype(np.int64))
    return out


def key_switch_sp(o, d, k0, k1, centre=True):
    """The key switch of d [L][n] under (k0, k1) -> dict(ks=(ks0, ks1) uint32 [L][n], delta=(delta0, delta1) int64 [n],
    D=the digits).  Steps 1 to 4 of the definition, word for word."""
    L, p = d.shape[0], o.np - 1
    P = o.q[p]
    assert 1 <= L <= p
    D = sp_digits(o, d, centre)
    acc = {}
    for i in list(range(L)) + [p]:
        q = np.uint64(o.q[i])
        a = [np.zeros(o.n, dtype=np.uint64), np.zeros(o.n, dtype=np.uint64)]
        for j in range(L):
            f = o.ntt((D[j] % o.q[i]).astype(np.uint32), i).astype(np.uint64)
            if i == j and centre:
                assert (f == d[j]).all()          # for i = j the factor is d[j] itself
            for k, key in enumerate((k0, k1)):
                a[k] = (a[k] + (f * key[j, i].astype(np.uint64)) % q) % q
        acc[i] = a
    ks, deltas = [], []
    for k in range(2):
        delta = centred(o.intt(acc[p][k].astype(np.uint32), p), P)
        rows = []
        for i in range(L):
            q = o.q[i]
            t = o.ntt((delta % q).astype(np.uint32), i).astype(np.uint64)
            diff = (acc[i][k] + np.uint64(q) - t) % np.uint64(q)
            rows.append(((diff * np.uint64(pow(P, -1, q))) % np.uint64(q)).astype(np.uint32))
        ks.append(np.stack(rows))
        deltas.append(delta)
    return dict(ks=tuple(ks), delta=tuple(deltas), D=D)


def add_mod(o, a, b):
    """rows [L][n] + rows [L][n] mod q_j."""
    q = np.array(o.q[:a.shape[0]], dtype=np.uint64)[:, None]
    return ((a.astype(np.uint64) + b.astype(np.uint64)) % q).astype(np.uint32)


def relin_sp_expect(o, d0, d1, d2, k0, k1):
    """Slabs [B][L][n]: out0 = d0 + ks_0, out1 = d1 + ks_1 with d = d2."""
    out0, out1 = np.zeros_like(d0), np.zeros_like(d1)
    for b in range(d0.shape[0]):
        ks0, ks1 = key_switch_sp(o, d2[b], k0, k1)["ks"]
        out0[b], out1[b] = add_mod(o, d0[b], ks0), add_mod(o, d1[b], ks1)
    return out0, out1


def galois_sp_expect(o, c0, c1, g, k0, k1):
    """Slabs [B][L][n]: the relinearisation on (sigma(c0), 0, sigma(c1))."""
    return relin_sp_expect(o, sigma_slab(o, c0, g), np.zeros_like(c1), sigma_slab(o, c1, g), k0, k1)


def sp_key(o, sk, target, label):
    """A special-prime key from the oracle alone: row j is the oracle's public key of seeds derive_seeds(label) with
    (P mod q_j) . target[j] added on column j -> (k0, k1) uint32 [np - 1][np][n].  target [np - 1][n]: s_hat^2 for the
    relinearisation key, sigma(s_hat) for a Galois key."""
    npr, p = o.np, o.np - 1
    a_seeds, e_seeds = V.derive_seeds(label + "-a", p), V.derive_seeds(label + "-e", p)
    k0, k1 = [], []
    for j in range(p):
        pk0, pk1 = o.gen_pk(sk, a_seeds[j].tobytes(), e_seeds[j].tobytes())
        r0 = [np.array(pk0[i]) for i in range(npr)]
        q = np.uint64(o.q[j])
        r0[j] = ((r0[j].astype(np.uint64) + (target[j].astype(np.uint64) * np.uint64(o.q[p] % o.q[j])) % q) % q).astype(np.uint32)
        k0.append(np.stack(r0))
        k1.append(np.stack([np.array(pk1[i]) for i in range(npr)]))
    return np.stack(k0), np.stack(k1)


def key_errors(o, k0, k1, s_hat, target):
    """e_j of every key row, recovered with the oracle: the centred INTT of k0 + k1 . s_hat minus the diagonal, which
    must be the same small integer polynomial on the first data prime and on the special prime -> int64 [np - 1][n]."""
    p = o.np - 1
    errs = []
    for j in range(p):
        per_prime = []
        for i in (0, p):
            q = np.uint64(o.q[i])
            v = o.decrypt(k0[j, i], k1[j, i], s_hat[i], i).astype(np.uint64)
            if i == j:
                v = (v + q - (target[j].astype(np.uint64) * np.uint64(o.q[p] % o.q[j])) % q) % q
            per_prime.append(centred(o.intt(v.astype(np.uint32), i), o.q[i]))
        assert (per_prime[0] == per_prime[1]).all() and np.abs(per_prime[0]).max() <= 64, j
        errs.append(per_prime[0])
    return errs


def switch_quotient(o, d, k0, k1, errs, s_nat):
    """(T - delta_0 - delta_1 * s) / P with T = sum_j D_j * e_j (negacyclic products, integers): what the key switch
    of d adds to the decrypted value.  Asserts the divisibility.  -> int64 [n]."""
    P = o.q[o.np - 1]
    r = key_switch_sp(o, d, k0, k1)
    T = np.zeros(o.n, dtype=np.int64)
    for Dj, ej in zip(r["D"], errs):
        T += negacyclic(Dj, ej)                 # below n . 2^29 . 64 < 2^49 per term
    num = T - r["delta"][0] - negacyclic(r["delta"][1], s_nat)
    assert (num % P == 0).all()
    return num // P
