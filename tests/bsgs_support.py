"""What the baby-step / giant-step tests (tests/test_ct_bsgs_build.py, tests/test_gpu_ct_bsgs.py) share: the definitions
of include/seal_embedded_amd.h restated with the oracle's primitives (ntt, intt), se_amd_galois_table -- a host-only
entry pinned against the coefficient-domain automorphism by tests/test_ct_galois_build.py -- and NumPy / Python integers.
Nothing here calls the device code under test.

    many form   rot0[e][b][i][k] = c0[b][i][src_e(k)] + sum_r NTT_i(D_r)[src_e(k)] . gk0_e[r][i][k]       D = digits of c1
    entry 1     out[g][b][i][k]  = sum_e (pt[g][e][i][k] mod q_i) . in[e][b][i][k]
    entry 2     out[b]           = sum_g rho_g(in[g][b]),  rho_g = relin_expect on (sigma(c0), 0, sigma(c1)), identity for 1
    plan        d'[g][b][i][k]   = d[g][b][i][src_{giant[g]^-1}(k)];  rot -> entry 1 with d' -> entry 2 with giant
all mod q_i and canonical."""
import numpy as np

import vectors as V
from gpu_support import DIGIT_MASK, digits_of, rand_slab, relin_expect

GALOIS_CASES = [((1024, 1), (1,), 3), ((4096, 3), (3, 2), 3), ((16384, 13), (13,), 2)]    # those of the rotation tests
CASE_IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def inverse_element(n, g):
    """g^-1 mod 2n of an odd g."""
    inv = pow(int(g), -1, 2 * n)
    assert (inv * g) % (2 * n) == 1
    return inv


def src_of(pkg, n, g):
    return pkg.galois_table(n, g).astype(np.int64)


# ---- the many form (the baby steps) ---------------------------------------------------------------------------------
def hoist_expect(pkg, o, c0, c1, elts, key_of, gk0, gk1):
    """rot0, rot1 uint32 [G][B][L][n] for the call elements `elts`; key_of[g] is the row of g in gk0 / gk1
    [keys][R][np][n].  Element 1 gives the record itself.  uint64 arithmetic: a product is below 2^60 and is reduced
    before it is added."""
    B, L, n = c0.shape
    out0 = np.zeros((len(elts), B, L, n), dtype=np.uint32)
    out1 = np.zeros_like(out0)
    srcs = [src_of(pkg, n, g) for g in elts]
    for b in range(B):
        D = digits_of(o, c1[b], L)
        for i in range(L):
            q = np.uint64(o.q[i])
            F = [o.ntt(dig, i).astype(np.uint64) for dig in D]
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


# ---- entry 1: the weighted sum over a stack ---------------------------------------------------------------------------
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


# ---- entry 2: rotate different records and add -----------------------------------------------------------------------
def sigma_slab(o, slab, g):
    """sigma_g on every NTT-form row of a slab [B][L][n], in the coefficient domain through o.intt / o.ntt."""
    out = np.zeros_like(slab)
    for b in range(slab.shape[0]):
        for j in range(slab.shape[1]):
            out[b, j] = o.ntt(V.sigma_coeff(o.intt(slab[b, j], j), g, o.q[j]), j)
    return out


def galois_expect(o, c0, c1, g, gk0, gk1):
    """The definition of se_amd_ct_galois_device: relin_expect on (sigma(c0), 0, sigma(c1)) with the key of the element."""
    return relin_expect(o, sigma_slab(o, c0, g), np.zeros_like(c1), sigma_slab(o, c1, g), gk0, gk1)


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


# ---- the plan ---------------------------------------------------------------------------------------------------------
def permute_diagonals(pkg, n, diag, giant):
    """d'[g][b][i][k] = d[g][b][i][src_{giant[g]^-1}(k)] on diag [n2][n1][rows][n]."""
    out = np.zeros_like(diag)
    for g, elt in enumerate(giant):
        out[g] = diag[g][..., src_of(pkg, n, inverse_element(n, elt))]
    return out


def bsgs_expect(pkg, o, c0, c1, baby, giant, diag, key_of, gk0, gk1):
    """The three steps of se_amd_ct_bsgs_device on records [B][L][n] and the caller's diagonals [n2][n1][>= L][n]."""
    n = c0.shape[2]
    rot = hoist_expect(pkg, o, c0, c1, baby, key_of, gk0, gk1)
    dp = permute_diagonals(pkg, n, diag, giant)
    inner = stack_sum_expect(o, rot[0], dp), stack_sum_expect(o, rot[1], dp)
    return accum_expect(o, inner[0], inner[1], giant, key_of, gk0, gk1)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def edge_row(o, j, rng, elts):
    """NTT form of natural-order coefficients that hold both sides of the digit boundary, 0, 1 and q - 1, each on an index
    whose image is negated and on one whose image is kept, for every element of `elts` that keeps more than one index
    (2n - 1 negates all but index 0; 1 negates none)."""
    n, q = o.n, o.q[j]
    edges = np.array([0, 1, DIGIT_MASK, DIGIT_MASK + 1, DIGIT_MASK + 2, q - 1], dtype=np.uint32)
    c = rng.integers(1, q, n, dtype=np.uint32)
    for start in (0, n // 9, n // 5, n // 3, n // 2, n - 13):
        c[start:start + 6] = c[start + 7:start + 13] = edges
    for g in elts:
        if g == 1:
            continue
        _, neg = V.galois_image(n, g)
        for v in edges:
            at = c == v
            assert (at & neg).any(), (g, int(v))
            assert (at & ~neg).any() or g == 2 * n - 1, (g, int(v))
    row = o.ntt(c, j)
    assert (o.intt(row, j) == c).all()
    return row


def random_keys(rng, q, count, n, npr):
    """gk0, gk1 [count][2 np][np][n] of random residues, with 0, 1 and q - 1 among the first words."""
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
