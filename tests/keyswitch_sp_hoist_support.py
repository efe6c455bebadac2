"""The hoisted rotations on the special-prime key (se_amd_ct_galois_sum_sp_device, se_amd_ct_lintrans_sp_device) as
their definition states them, from the oracle's transforms and NumPy / Python integers: what
tests/test_gpu_ct_keyswitch_sp_hoist.py and tests/test_ct_keyswitch_sp_hoist_build.py compare the entries against and what
tools/ct_keyswitch_sp_noise_sim.py simulates with.  Nothing here touches the GPU or the library.

Notation is that of keyswitch_sp_support: o = Oracle(n, np) of the CONTEXT, p = np - 1, P = o.q[p], records have
L <= np - 1 rows, a key is (k0, k1), uint32 [np - 1][np][n] each; keys = one such pair per element.

    D_j         = centred(INTT_j(c1[b][j]), q_j)                                              j < L
    F_{j,i}     = NTT_i(D_j mod q_i)                                                          i in E = {0 .. L-1, p}
    ACC_k[i][x] = sum_e w_e[i][x] . sum_{j<L} F_{j,i}[src_e(x)] . k_k^e[j][i][x]   mod q_i
    delta_k     = centred(INTT_p(ACC_k[p]), P)
    ks_k[i]     = (ACC_k[i] - NTT_i(delta_k mod q_i)) . P^-1   mod q_i,  i < L
    out0[i][x]  = ks_0[i][x] + w_0[i][x] . c0[b][i][x] + sum_e w_e[i][x] . c0[b][i][src_e(x)]
    out1[i][x]  = ks_1[i][x] + w_0[i][x] . c1[b][i][x]
"""
import numpy as np

from keyswitch_sp_support import add_mod, centred, galois_sp_expect, sp_digits


def _brev(v, bits):
    r = np.zeros_like(v)
    for b in range(bits):
        r |= ((v >> b) & 1) << (bits - 1 - b)
    return r


def src_table(n, g):
    """se_amd_galois_table(g) from its formula: sigma_g(x)[k] = x[src[k]] on a bit-reversed NTT-form row,
    src(k) = brev((((2 brev(k) + 1) g mod 2n) - 1) / 2)."""
    bits = n.bit_length() - 1
    k = np.arange(n, dtype=np.int64)
    return _brev((((2 * _brev(k, bits) + 1) * g) % (2 * n) - 1) // 2, bits)


def _weight(w, i, q, n):
    """Row i of a weight [np][n] of arbitrary 32-bit words reduced mod q_i (None: all ones) -> uint64 [n]."""
    if w is None:
        return np.ones(n, dtype=np.uint64)
    return w[i].astype(np.uint64) % np.uint64(q)


def hoist_sp_expect(o, c0, c1, elts, keys, weights=None, w0=None):
    """Slabs [B][L][n], elts [G], keys [G] pairs (k0, k1), weights None (the sum form: w_e = 1) or uint32 [G][np][n]
    (the diagonals, any 32-bit words, all np rows), w0 None (no term of the record itself), the integer 1 (add_input)
    or uint32 [np][n] (diag0) -> (out0, out1, info), info[b] = dict(delta=(delta_0, delta_1) int64 [n], D=the digits)."""
    B, L, n = c0.shape
    p = o.np - 1
    P = o.q[p]
    assert 1 <= L <= p and c1.shape == c0.shape and len(elts) == len(keys)
    src = [src_table(n, int(g)) for g in elts]
    if isinstance(w0, (int, np.integer)):
        assert w0 == 1
        w0 = np.ones((o.np, n), dtype=np.uint32)
    out0, out1, info = np.zeros_like(c0), np.zeros_like(c1), []
    for b in range(B):
        D = sp_digits(o, c1[b])
        acc = {}
        for i in list(range(L)) + [p]:
            q = np.uint64(o.q[i])
            F = []
            for j in range(L):
                f = o.ntt((D[j] % o.q[i]).astype(np.uint32), i).astype(np.uint64)
                if i == j:
                    assert (f == c1[b, j]).all()              # F_{j,j} is c1[b][j] as it lies
                F.append(f)
            a = [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]
            for e, (k0, k1) in enumerate(keys):
                w = _weight(None if weights is None else weights[e], i, o.q[i], n)
                for k, key in enumerate((k0, k1)):
                    inner = np.zeros(n, dtype=np.uint64)
                    for j in range(L):
                        inner = (inner + (F[j][src[e]] * key[j, i].astype(np.uint64)) % q) % q
                    a[k] = (a[k] + (w * inner) % q) % q
            acc[i] = a
        deltas = []
        for k, (out, rec) in enumerate(((out0, c0), (out1, c1))):
            delta = centred(o.intt(acc[p][k].astype(np.uint32), p), P)
            deltas.append(delta)
            for i in range(L):
                q = np.uint64(o.q[i])
                t = o.ntt((delta % o.q[i]).astype(np.uint32), i).astype(np.uint64)
                row = (((acc[i][k] + q - t) % q) * np.uint64(pow(P, -1, o.q[i]))) % q
                if w0 is not None:
                    row = (row + (_weight(w0, i, o.q[i], n) * rec[b, i].astype(np.uint64)) % q) % q
                if k == 0:
                    for e in range(len(elts)):
                        w = _weight(None if weights is None else weights[e], i, o.q[i], n)
                        row = (row + (w * c0[b, i][src[e]].astype(np.uint64)) % q) % q
                out[b, i] = row.astype(np.uint32)
        info.append(dict(delta=tuple(deltas), D=D))
    return out0, out1, info


def sum_of_single_calls(o, c0, c1, elts, keys, add_input=False):
    """What G calls of se_amd_ct_galois_sp_device and a modular sum give (G roundings): (out0, out1)."""
    out0 = c0.copy() if add_input else np.zeros_like(c0)
    out1 = c1.copy() if add_input else np.zeros_like(c1)
    for g, (k0, k1) in zip(elts, keys):
        e0, e1 = galois_sp_expect(o, c0, c1, int(g), k0, k1)
        for b in range(c0.shape[0]):
            out0[b], out1[b] = add_mod(o, out0[b], e0[b]), add_mod(o, out1[b], e1[b])
    return out0, out1
