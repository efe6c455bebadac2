"""The host model of the ciphertext operations: every definition of include/seal_embedded_amd.h that the kernels are held
to, stated once with the oracle's primitives (o.ntt, o.intt, o.decrypt, o.gen_pk), vectors and NumPy / Python integers,
and the constructed inputs the tests feed them.  Nothing here touches the GPU or the library: the module imports neither
torch, pytest, ctypes nor the package, so the CPU suite (tests/test_ct_model.py, the build checks) and the noise
simulations under tools/ import it as well as the GPU modules.  Every name has this one home.

Notation: o = Oracle(n, np); records are uint32 slabs [B][L][n] of NTT-form rows, L <= np; all results canonical mod q_i.
Digit keys are (gk0, gk1) uint32 [2 np][np][n], row r = 2 j + t the key of digit t of prime j.  Special-prime keys are
(k0, k1) uint32 [np - 1][np][n] with p = np - 1 the special prime's index, P = o.q[p], records of L <= np - 1 rows.
A `table` argument is the permutation table function (n, g) -> src with sigma_g(x)[k] = x[src[k]] on a bit-reversed row:
the GPU tests pass the package's galois_table (se_amd_galois_table, so the C table is what is checked), src_table is the
same from its formula.

    digit key switch   out_k[b][i]      = d_k[b][i] + sum_r NTT_i(D_r) . evk_k[r][i]                      D = digits_of(d2)
    rotation           relin_expect on (sigma(c0), 0, sigma(c1)) with the key of the element
    many form          rot0[e][b][i][k] = c0[b][i][src_e(k)] + sum_r NTT_i(D_r)[src_e(k)] . gk0_e[r][i][k]  D = digits of c1
                       rot1             = the same without the c0 term; element 1 gives the record itself
    linear transform   out_k[b][i]      = (d0[i] mod q_i) . c_k[b][i] + sum_e (d_e[i] mod q_i) . rot_k[e][b][i]
    stack sum          out[g][b][i][k]  = sum_e (pt[g][e][i][k] mod q_i) . in[e][b][i][k]
    accumulate         out[b]           = sum_g rho_g(in[g][b]),  rho_g the rotation, the identity for element 1
    bsgs plan          d'[g] = d[g] permuted by src_{giant[g]^-1};  many form -> stack sum with d' -> accumulate with giant
    special prime      D_j = centred(INTT_j(d[j])), ACC_k[i] = sum_j NTT_i(D_j mod q_i) . k_k[j][i] for i < L and i = p,
                       delta_k = centred(INTT_p(ACC_k[p])), ks_k[i] = (ACC_k[i] - NTT_i(delta_k mod q_i)) . P^-1
    hoisted, special   ACC_k[i][x] = sum_e w_e[i][x] . sum_j F_{j,i}[src_e(x)] . k_k^e[j][i][x], one delta and one division,
                       out0 += w_0 . c0 + sum_e w_e . c0[src_e], out1 += w_0 . c1
"""
import numpy as np

import vectors as V
from vectors import sigma_coeff

DIGIT_BITS = 15                       # SE_AMD_RELIN_DIGIT_BITS
DIGIT_MASK = (1 << DIGIT_BITS) - 1

GALOIS_CASES = [((1024, 1), (1,), 3), ((4096, 3), (3, 2), 3), ((16384, 13), (13,), 2)]     # (shape, levels, B)
SP_CASES = [((4096, 3), (2, 1), 3), ((4096, 2), (1,), 3), ((16384, 13), (12,), 2)]
CASE_IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731
SHAPE_IDS = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


# ---- integer helpers ------------------------------------------------------------------------------------------------
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


def crt_centred(q, pts):
    """pts[j][k] = value mod q[j]  ->  Python ints in (-Q/2, Q/2], Q = prod q[j]."""
    Q = 1
    for x in q:
        Q *= x
    acc = np.zeros(pts[0].shape[0], dtype=object)
    for j, x in enumerate(q):
        M = Q // x
        acc = acc + pts[j].astype(object) * (M * pow(M % x, -1, x))
    acc = acc % Q
    return [int(v) - Q if int(v) > Q // 2 else int(v) for v in acc]


def add_mod(o, a, b):
    """rows [L][n] + rows [L][n] mod q_j."""
    q = np.array(o.q[:a.shape[0]], dtype=np.uint64)[:, None]
    return ((a.astype(np.uint64) + b.astype(np.uint64)) % q).astype(np.uint32)


def modular_sum(o, rows, extra=None):
    """Sum over axis 0 of uint32 [G][B][L][n] (plus `extra` [B][L][n]) mod q_i per prime row."""
    L = rows.shape[2]
    qv = np.array(o.q[:L], dtype=np.uint64)[None, :, None]
    s = rows.astype(np.uint64).sum(axis=0)                                # G <= 64 terms below 2^30
    if extra is not None:
        s = s + extra.astype(np.uint64)
    return (s % qv).astype(np.uint32)


def lift_expect(o, slab, weight):
    """slab [B][np][n] times one integer weight below 2^32, mod q_i."""
    qv = np.array(o.q, dtype=np.uint64)[None, :, None]
    return ((slab.astype(np.uint64) * np.uint64(weight)) % qv).astype(np.uint32)


def lincomb_expect(slab, q, rows):
    """slab uint32 [B][np][n], q Python ints, rows = list of (indices, weights | None)  ->  uint32 [G][np][n].
    sum_k (w_k % q) c[idx_k] % q, regrouped per distinct record: its coefficient sum_k (w_k % q) % q is a Python int
    below 2^30, the products stay below 2^60 and are reduced one by one, and at most B < 2^34 of them are summed."""
    npr, n = slab.shape[1], slab.shape[2]
    qv = np.array(q, dtype=np.uint64)[:, None]
    out = np.zeros((len(rows), npr, n), dtype=np.uint32)
    for g, (idx, w) in enumerate(rows):
        coef = {}
        for k, i in enumerate(idx):
            wk = 1 if w is None else int(w[k])
            c = coef.setdefault(int(i), [0] * npr)
            for j in range(npr):
                c[j] = (c[j] + wk % q[j]) % q[j]
        acc = np.zeros((npr, n), dtype=np.uint64)
        for i, c in coef.items():
            acc += (slab[i].astype(np.uint64) * np.array(c, dtype=np.uint64)[:, None]) % qv
        out[g] = (acc % qv).astype(np.uint32)
    return out


# ---- rescale, digits and the digit key switch -----------------------------------------------------------------------
def rescale_expect(o, slab):
    """slab uint32 [B][L][n] -> uint32 [B][L-1][n]: out[j] = (in[j] - NTT_j(delta mod q_j)) . q_last^-1 mod q_j with
    delta the centred INTT of the last row, from o.intt / o.ntt and uint64 arithmetic."""
    B, L, n = slab.shape
    q_last = o.q[L - 1]
    out = np.zeros((B, L - 1, n), dtype=np.uint32)
    for b in range(B):
        delta = centred(o.intt(slab[b, L - 1], L - 1), q_last)
        for j in range(L - 1):
            q = o.q[j]
            inv = pow(q_last, -1, q)
            t = o.ntt((delta % q).astype(np.uint32), j).astype(np.uint64)
            diff = (slab[b, j].astype(np.uint64) + np.uint64(q) - t) % np.uint64(q)
            out[b, j] = ((diff * np.uint64(inv)) % np.uint64(q)).astype(np.uint32)
    return out


def digits_of(o, rec, L):
    """Record [L][n] -> the 2 L digit polynomials D_{j,t} (uint32, natural order), row r = 2j + t."""
    out = []
    for j in range(L):
        c = o.intt(rec[j], j)
        out += [c & np.uint32(DIGIT_MASK), c >> np.uint32(DIGIT_BITS)]
    return out


def relin_expect(o, d0, d1, d2, evk0, evk1):
    """The definition of the key switch, which relinearisation and rotation are both tested against:
    out_k[b][i] = d_k[b][i] + sum_r NTT_i(D_r) . evk_k[r][i] mod q_i, from o.intt / o.ntt and uint64 arithmetic (a
    product is below 2^60, reduced before it is added)."""
    B, L, n = d0.shape
    out0, out1 = np.zeros_like(d0), np.zeros_like(d1)
    for b in range(B):
        D = digits_of(o, d2[b], L)
        for i in range(L):
            q = np.uint64(o.q[i])
            acc0, acc1 = d0[b, i].astype(np.uint64), d1[b, i].astype(np.uint64)
            for r, dig in enumerate(D):
                f = o.ntt(dig, i).astype(np.uint64)
                acc0 = (acc0 + (f * evk0[r, i].astype(np.uint64)) % q) % q
                acc1 = (acc1 + (f * evk1[r, i].astype(np.uint64)) % q) % q
            out0[b, i], out1[b, i] = acc0, acc1
    return out0, out1


# ---- automorphisms --------------------------------------------------------------------------------------------------
def brev(v, bits):
    r = np.zeros_like(v)
    for b in range(bits):
        r |= ((v >> b) & 1) << (bits - 1 - b)
    return r


def src_table(n, g):
    """se_amd_galois_table(g) from its formula: sigma_g(x)[k] = x[src[k]] on a bit-reversed NTT-form row,
    src(k) = brev((((2 brev(k) + 1) g mod 2n) - 1) / 2)."""
    bits = n.bit_length() - 1
    k = np.arange(n, dtype=np.int64)
    return brev((((2 * brev(k, bits) + 1) * g) % (2 * n) - 1) // 2, bits)


def inverse_element(n, g):
    """g^-1 mod 2n of an odd g."""
    inv = pow(int(g), -1, 2 * n)
    assert (inv * g) % (2 * n) == 1
    return inv


def sigma_rows(o, rows, g):
    """sigma_g on NTT-form rows [L][n] through the coefficient domain (o.intt, sigma_coeff, o.ntt)."""
    return np.stack([o.ntt(sigma_coeff(o.intt(rows[j], j), g, o.q[j]), j) for j in range(len(rows))])


def sigma_slab(o, slab, g):
    """sigma_g on every record of a slab [B][L][n]."""
    return np.stack([sigma_rows(o, rec, g) for rec in slab])


def galois_expect(o, c0, c1, g, gk0, gk1):
    """The definition of se_amd_ct_galois_device: relin_expect on (sigma(c0), 0, sigma(c1)) with the key of the element."""
    return relin_expect(o, sigma_slab(o, c0, g), np.zeros_like(c1), sigma_slab(o, c1, g), gk0, gk1)


def hoist_expect(table, o, c0, c1, elts, key_of, gk0, gk1):
    """The many form: rot0, rot1 uint32 [G][B][L][n] for the call elements `elts`; key_of[g] is the row of g in gk0 / gk1
    [keys][R][np][n].  Element 1 gives the record itself and needs no key.  uint64 arithmetic: a product is below 2^60
    and is reduced before it is added."""
    B, L, n = c0.shape
    out0 = np.zeros((len(elts), B, L, n), dtype=np.uint32)
    out1 = np.zeros_like(out0)
    srcs = [table(n, g).astype(np.int64) for g in elts]
    for b in range(B):
        D = digits_of(o, c1[b], L)
        for i in range(L):
            q = np.uint64(o.q[i])
            F = [o.ntt(dig, i).astype(np.uint64) for dig in D]           # shared by the elements: the hoisting
            for e, (g, src) in enumerate(zip(elts, srcs)):
                if g == 1:
                    out0[e, b, i], out1[e, b, i] = c0[b, i], c1[b, i]
                    continue
                k0, k1 = gk0[key_of[g]], gk1[key_of[g]]
                acc0, acc1 = c0[b, i][src].astype(np.uint64), np.zeros(n, dtype=np.uint64)
                for r, f in enumerate(F):
                    acc0 = (acc0 + (f[src] * k0[r, i].astype(np.uint64)) % q) % q
                    acc1 = (acc1 + (f[src] * k1[r, i].astype(np.uint64)) % q) % q
                out0[e, b, i], out1[e, b, i] = acc0, acc1
    return out0, out1


# ---- linear transforms ----------------------------------------------------------------------------------------------
def weighted_sum(o, rot, diag, c=None, diag0=None):
    """sum_e (diag[e] mod q) . rot[e] (+ (diag0 mod q) . c) mod q_i: rot uint32 [G][B][L][n], diag [G][>= L][n] of any
    32-bit words, c [B][L][n], diag0 [>= L][n].  A product of residues is below 2^60; reduced before it is added."""
    G, B, L, n = rot.shape
    qv = np.array(o.q[:L], dtype=np.uint64)[None, :, None]
    acc = np.zeros((B, L, n), dtype=np.uint64)
    for e in range(G):
        acc = (acc + (rot[e].astype(np.uint64) * (diag[e, :L].astype(np.uint64)[None] % qv)) % qv) % qv
    if diag0 is not None:
        acc = (acc + (c.astype(np.uint64) * (diag0[:L].astype(np.uint64)[None] % qv)) % qv) % qv
    return acc.astype(np.uint32)


def lintrans_expect(o, rot, diag, c0, c1, diag0):
    return weighted_sum(o, rot[0], diag, c0, diag0), weighted_sum(o, rot[1], diag, c1, diag0)


def stack_sum_expect(o, stack, pt):
    """stack uint32 [E][B][L][n], pt [Gout][E][>= L][n] of any 32-bit words -> [Gout][B][L][n].  Every product of a
    residue below 2^30 and a 32-bit word is below 2^62 and is reduced before it is added."""
    E, B, L, n = stack.shape
    qv = np.array(o.q[:L], dtype=np.uint64)[None, :, None]
    out = np.zeros((pt.shape[0], B, L, n), dtype=np.uint32)
    for g in range(pt.shape[0]):
        acc = np.zeros((B, L, n), dtype=np.uint64)
        for e in range(E):
            acc = (acc + (stack[e].astype(np.uint64) * (pt[g, e, :L].astype(np.uint64)[None] % qv)) % qv) % qv
        out[g] = acc
    return out


def stack_sum_python(q, stack, pt):
    """The same on one row in Python integers (no word size anywhere): stack [E][n], pt [E][n] -> list of n ints."""
    E, n = stack.shape
    return [sum((int(pt[e, k]) % q) * int(stack[e, k]) for e in range(E)) % q for k in range(n)]


def accum_expect(o, in0, in1, elts, key_of, gk0, gk1):
    """in [G][B][L][n] -> the modular sum of the G rotation expectations, [B][L][n]; element 1 adds the record as it is."""
    G, B, L, n = in0.shape
    qv = np.array(o.q[:L], dtype=np.uint64)[None, :, None]
    acc = [np.zeros((B, L, n), dtype=np.uint64), np.zeros((B, L, n), dtype=np.uint64)]
    for s, g in enumerate(elts):
        term = (in0[s], in1[s]) if g == 1 else galois_expect(o, in0[s], in1[s], g, gk0[key_of[g]], gk1[key_of[g]])
        for h in (0, 1):
            acc[h] = (acc[h] + term[h].astype(np.uint64)) % qv
    return acc[0].astype(np.uint32), acc[1].astype(np.uint32)


def permute_diagonals(table, n, diag, giant):
    """d'[g][b][i][k] = d[g][b][i][src_{giant[g]^-1}(k)] on diag [n2][n1][rows][n]."""
    out = np.zeros_like(diag)
    for g, elt in enumerate(giant):
        out[g] = diag[g][..., table(n, inverse_element(n, elt)).astype(np.int64)]
    return out


def bsgs_expect(table, o, c0, c1, baby, giant, diag, key_of, gk0, gk1):
    """The three steps of se_amd_ct_bsgs_device on records [B][L][n] and the caller's diagonals [n2][n1][>= L][n]."""
    n = c0.shape[2]
    rot = hoist_expect(table, o, c0, c1, baby, key_of, gk0, gk1)
    dp = permute_diagonals(table, n, diag, giant)
    inner = stack_sum_expect(o, rot[0], dp), stack_sum_expect(o, rot[1], dp)
    return accum_expect(o, inner[0], inner[1], giant, key_of, gk0, gk1)


# ---- the special prime ----------------------------------------------------------------------------------------------
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


def digit_key_errors(o, k0, k1, s_hat, diagonal):
    """e_r of every row of a digit key [2 np][np][n], recovered with the oracle: the centred INTT of k0 + k1 . s_hat minus
    diagonal(j, t) on column j of row 2 j + t, which must be the same small integer polynomial on the first and on the
    last prime -> int64 [2 np][n]."""
    npr = o.np
    errs = []
    for r in range(2 * npr):
        per_prime = []
        for i in (0, npr - 1):
            q = np.uint64(o.q[i])
            v = o.decrypt(k0[r, i], k1[r, i], s_hat[i], i).astype(np.uint64)
            if i == r // 2:
                v = (v + q - diagonal(i, r % 2)) % q
            per_prime.append(centred(o.intt(v.astype(np.uint32), i), o.q[i]))
        assert (per_prime[0] == per_prime[1]).all() and np.abs(per_prime[0]).max() <= 64, r   # one small integer e_r
        errs.append(per_prime[0])
    return errs


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
        r0[j] = ((r0[j].astype(np.uint64) + sp_diagonal(o, target, j)) % np.uint64(o.q[j])).astype(np.uint32)
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
                v = (v + q - sp_diagonal(o, target, j)) % q
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


# ---- the diagonals of generated keys ----------------------------------------------------------------------------------
def relin_diagonal(o, s_hat, j, t):
    """(2^(DIGIT_BITS t) mod q_j) . s_hat_j^2 mod q_j, uint64 (every intermediate is below 2^60)."""
    q = np.uint64(o.q[j])
    s = s_hat[j].astype(np.uint64)
    return (((s * s) % q) * np.uint64(pow(2, DIGIT_BITS * t, o.q[j]))) % q


def galois_diagonal(o, s_hat, g, j, t):
    """(2^(DIGIT_BITS t) mod q_j) . sigma(s_hat_j) mod q_j, uint64; sigma through the coefficient domain."""
    q = o.q[j]
    s = o.ntt(sigma_coeff(o.intt(s_hat[j], j), g, q), j).astype(np.uint64)
    return (s * np.uint64(pow(2, DIGIT_BITS * t, q))) % np.uint64(q)


def sp_diagonal(o, target, j):
    """(P mod q_j) . target_j mod q_j, uint64."""
    q = o.q[j]
    return (target[j].astype(np.uint64) * np.uint64(o.q[o.np - 1] % q)) % np.uint64(q)


# ---- constructed inputs ---------------------------------------------------------------------------------------------
def edge_row(o, j, rng, elts, edges="digit", starts=3, skip_identity=False):
    """NTT form of natural-order coefficients that hold the edge values of a key switch beside random ones, each value
    planted twice, 7 apart (an even and an odd index), at every start position.
    edges "digit": 0, 1, both sides of the digit boundary and q - 1 among random values in [1, q) -- the digit key
    switch.  edges "centring": 0, 1, (q - 1)/2, (q + 1)/2 and q - 1 among random values in [2, q - 1) -- the centred
    digits of the special-prime key switch.
    starts 3: 0, n/2, n - 13, and every value must lie on an index whose image is negated and on one whose image is kept
    for every element of `elts`.  starts 6: n/9, n/5 and n/3 as well, for lists that hold 2n - 1, which negates every
    coefficient but the constant one (0 here) and is excused from the kept half; with skip_identity element 1, which
    negates nothing, is passed over."""
    n, q = o.n, o.q[j]
    if edges == "digit":
        values = np.array([0, 1, DIGIT_MASK, DIGIT_MASK + 1, DIGIT_MASK + 2, q - 1], dtype=np.uint32)
        c = rng.integers(1, q, n, dtype=np.uint32)
    else:
        assert edges == "centring"
        values = np.array([0, 1, (q - 1) // 2, (q + 1) // 2, q - 1], dtype=np.uint32)
        c = rng.integers(2, q - 1, n, dtype=np.uint32)
    w = len(values)
    for start in {3: (0, n // 2, n - 13), 6: (0, n // 9, n // 5, n // 3, n // 2, n - 13)}[starts]:
        c[start:start + w] = c[start + 7:start + 7 + w] = values
    for g in elts:
        if skip_identity and g == 1:
            continue
        _, neg = V.galois_image(n, g)
        for v in values:
            at = c == v
            assert (at & neg).any(), (g, int(v))
            assert (at & ~neg).any() or (starts == 6 and g == 2 * n - 1), (g, int(v))
    assert c[0] == 0
    row = o.ntt(c, j)
    assert (o.intt(row, j) == c).all()
    return row


def rand_slab(rng, q, count, n, primes=None):
    primes = len(q) if primes is None else primes
    return np.stack([rng.integers(0, q[j], (count, n), dtype=np.uint32) for j in range(primes)], axis=1)


def rand_key(rng, q, n):
    """One special-prime key half [np - 1][np][n] of random words below q_i."""
    return np.stack([rand_slab(rng, q, 1, n)[0] for _ in range(len(q) - 1)])


def random_keys(rng, q, count, n, npr):
    """Digit keys gk0, gk1 [count][2 np][np][n] of random residues, with 0, 1 and q - 1 among the first words."""
    R = 2 * npr
    gk0 = np.stack([np.stack([rand_slab(rng, q, 1, n)[0] for _ in range(R)]) for _ in range(count)])
    gk1 = np.stack([np.stack([rand_slab(rng, q, 1, n)[0] for _ in range(R)]) for _ in range(count)])
    gk0[0, 0, 0, :4] = [0, 1, q[0] - 1, q[0] - 1]
    return gk0, gk1


def random_plaintexts(rng, q, lead, n, rows=None):
    """[*lead][rows][n] random residues (rows defaults to len(q); a row past len(q) is arbitrary words).  The last prime
    row of the last plaintext holds arbitrary 32-bit words >= q_i, q_i itself and 0xFFFFFFFF among them; every plaintext
    holds 0, 1, q - 1 at the positions 0, 1, 2 and n - 3 .. n - 1 of every prime row."""
    npr = len(q)
    rows = npr if rows is None else rows
    count = int(np.prod(lead))
    pt = np.zeros((count, rows, n), dtype=np.uint32)
    for i in range(rows):
        pt[:, i] = rng.integers(0, q[i] if i < npr else 1 << 32, (count, n), dtype=np.uint64).astype(np.uint32)
    last = min(rows, npr) - 1
    pt[count - 1, last] = rng.integers(q[last], 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pt[count - 1, last, 3:5] = [q[last], 0xFFFFFFFF]
    for i in range(min(rows, npr)):
        pt[:, i, :3] = pt[:, i, n - 3:] = [0, 1, q[i] - 1]
    return pt.reshape(tuple(lead) + (rows, n))


def random_diagonals(rng, q, G, n):
    """[G][np][n] random residues; the last prime row of the last diagonal holds arbitrary 32-bit words >= q_i; every
    diagonal holds 0, 1, q - 1 at the positions 0, 1, 2 and n - 3 .. n - 1 of every prime row.  And a d0 [np][n]."""
    npr = len(q)
    diag = rand_slab(rng, q, G, n)
    diag0 = rand_slab(rng, q, 1, n)[0]
    diag[G - 1, npr - 1] = rng.integers(q[npr - 1], 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    diag[G - 1, npr - 1, 3:5] = [q[npr - 1], 0xFFFFFFFF]
    diag0[0, 5] = 0xFFFFFFFF
    for i in range(npr):
        for d in list(diag) + [diag0]:
            d[i, :3] = d[i, n - 3:] = [0, 1, q[i] - 1]
    return diag, diag0


def edge_diagonals(rng, q, G, n):
    """[G][np][n] arbitrary 32-bit words: random, with 0, 1, q_i - 1, q_i and 2^32 - 1 on every row, the row at the
    special prime among them."""
    d = rng.integers(0, 2 ** 32, (G, len(q), n), dtype=np.uint32)
    for i, qi in enumerate(q):
        d[:, i, 3:8] = [0, 1, qi - 1, qi, 2 ** 32 - 1]
        d[:, i, n - 5:] = [2 ** 32 - 1, qi, qi - 1, 1, 0]
    return d


def call_elements(n, npr):
    """The elements of a many-form call or a flat plan.  4096 x 3: 3, 3^-1, 3^5, n + 1, 2n - 1 and 3^2, with 3^5 listed
    twice (as a plan it carries two different diagonals).  Elsewhere 3, n + 1, 2n - 1."""
    if (n, npr) == (4096, 3):
        elts = [3, pow(3, -1, 2 * n), pow(3, 5, 2 * n), n + 1, 2 * n - 1, 9, pow(3, 5, 2 * n)]
        assert len(set(elts)) == len(elts) - 1
        return elts
    return [3, n + 1, 2 * n - 1]


def galois_seeds(npr, G, label, sp=False):
    """The (a, e) seed blocks of G evaluation keys: 2 np key rows each for digit keys, np - 1 for special-prime keys
    (G = 1: the special-prime relinearisation key)."""
    rows = G * (npr - 1 if sp else 2 * npr)
    return V.derive_seeds(label + "-a", rows), V.derive_seeds(label + "-e", rows)


def matrix(dim):
    """The examples' fixed matrix: M[r][c] = ((7 r + 3 c + 1) mod 17 - 8) / dim.  dim 8: entries in [-1, 1]; dim 16:
    entries in [-1/2, 1/2], sixteen of them against x in [-1, 1] keep |M x| <= 8, the bound of the 8 x 8 example."""
    r, c = np.meshgrid(np.arange(dim), np.arange(dim), indexing="ij")
    return ((7 * r + 3 * c + 1) % 17 - 8) / float(dim)


def matrix_diagonals(M, n, shift=1.0):
    """float32 [dim][n/2]: slot k of diagonal e = M[k mod dim][(k + e) mod dim] / shift, what the diagonal method encodes."""
    dim = M.shape[0]
    k = np.arange(n // 2)
    return np.stack([M[k % dim, (k + e) % dim] / shift for e in range(dim)]).astype(np.float32)
