"""The host model of the receiving side: constructed plaintexts for every branch of the full-modulus decrypt
(se_amd_decrypt_full_device, its keyed, level and degree-2 siblings; one kernel body, decrypt_full_body).  Every
expectation is the planted Python integer itself, and every input is shown here, in Python integers, to be decided by the
branch it targets.  Like ct_model this module touches neither the GPU nor the library and imports neither torch, pytest
nor ctypes: tests/test_recv_model.py checks it on the CPU, tests/test_gpu_decrypt_full.py feeds it to the kernels.

Notation: q_j the chain of the shape, Q'_j = q_0 ... q_{j-1} (Q'_0 = 1), Q = Q'_np, H = 2^63.  A vector is a list of n
Python integers in (-Q/2, Q/2], natural order; the kernel's thread t holds the coefficients (e << (logn - 4)) + t,
e = 0 .. 15.  The kernel recombines the primes one by one: primes 1 and 2 add Q'_j c in 128 bits and flag a sum that
leaves int64; from prime 3 on it reduces the int64 candidate mod q_j and flags a mismatch with the residue.
"""
import numpy as np

from ct_model import crt_centred

H = 2 ** 63
SHAPES = [(1024, 1), (4096, 2), (4096, 3), (8192, 6), (16384, 13)]


def chain_products(o):
    """Q'_0 .. Q'_np."""
    Qp = [1]
    for q in o.q:
        Qp.append(Qp[-1] * q)
    return Qp


def centre(v, Q):
    """The representative of v mod Q in (-Q/2, Q/2]  (Q odd)."""
    r = v % Q
    return r - Q if r > Q // 2 else r


def fits_int64(v):
    return -H <= v < H


def plant_positions(n):
    """Where the one bad coefficient of an out-of-range record goes: the first and last thread, the first and last of a
    thread's 16 register slots, both sides of the first wave-internal boundary and one in the middle."""
    return [0, 1, 15, 16, n // 16 - 1, n // 16, n // 2 + 3, n - 1]


def background(o, seed):
    """n seeded integers: uniform in [-2^62, 2^62), or for np <= 2 (Q < 2^60) in the centred range of Q."""
    rng = np.random.default_rng(seed)
    if o.np <= 2:
        half = (chain_products(o)[o.np] - 1) // 2
        return [int(x) for x in rng.integers(-half, half + 1, o.n)]
    return [int(x) for x in rng.integers(-2 ** 62, 2 ** 62, o.n)]


def edge_values(o):
    """The values of the `multiples` record: multiples and half-way points of every prime and of Q'_2, the values around
    c Q'_2 and the two ends of int64, kept where they lie in [-H, H) and in (-Q/2, Q/2]; each once, in a fixed order.
    With one prime Q'_2 stands for Q = q_0."""
    npr, q = o.np, o.q
    Qp = chain_products(o)
    Q, Q2 = Qp[npr], Qp[min(2, npr)]
    vals = [0, 1, -1]
    for j in range(npr):
        for m in (q[j], 7 * q[j], (q[j] - 1) // 2, (q[j] + 1) // 2):
            vals += [m, -m]
    for j in range(npr):
        for k in range(j + 1, npr):
            vals += [q[j] * q[k], -q[j] * q[k]]
    for m in (Q2, (Q2 - 1) // 2, (Q2 + 1) // 2):
        vals += [m, -m]
    for c in range(-8, 9):
        for r in (-(Q2 - 1) // 2, -1, 0, 1, (Q2 - 1) // 2):
            vals.append(c * Q2 + r)
    vals += [H - 1, -H]
    kept = []
    for v in vals:
        if fits_int64(v) and -Q // 2 < v <= Q // 2 and v not in kept:
            kept.append(v)
    if npr <= 2:
        assert (Q - 1) // 2 in kept and -(Q - 1) // 2 in kept          # both ends of the centred range
    else:
        assert H - 1 in kept and -H in kept                            # both ends of int64
    return kept


def in_range_vectors(o):
    """The status-1 records -> [(name, vector)].
    multiples: edge_values planted from index 0 upward and again ending at n - 1 (a low and a high thread, the first and
    the last register slot, hold each value) in the seeded background.
    zero: all coefficients 0; with a random c1 every word of c0 + c1 . s is then exactly q or 0 before the transform."""
    n = o.n
    vals = edge_values(o)
    assert 2 * len(vals) <= n
    vec = background(o, 1000 * n + o.np)
    vec[:len(vals)] = vals
    vec[n - len(vals):] = vals
    Q = chain_products(o)[o.np]
    assert all(fits_int64(v) and -Q // 2 < v <= Q // 2 for v in vec)
    return [("multiples", vec), ("zero", [0] * n)]


def decider(o, v):
    """The prime at which the recombination of v leaves int64: the smallest j with centre(v, Q'_{j+1}) outside [-H, H);
    None for a value that stays inside through the whole chain."""
    Qp = chain_products(o)
    for j in range(o.np):
        if not fits_int64(centre(v, Qp[j + 1])):
            return j
    return None


def out_of_range_vectors(o):
    """The status-0 records (np >= 3) -> [dict(name, vec, pos, value, prime)]: the seeded background plus ONE planted
    coefficient at `pos`, which rotates through plant_positions; `prime` is the prime that decides.
    Every shape: H, -H - 1, +-(2^64 + 5) (the 128-bit sum of prime 2 leaves int64 on either side) and +-(Q - 1)/2.
    np >= 4, for j = 3 .. np - 1: 12345 + Q'_j and -7 q_j - Q'_j.  Their int64 candidate (12345, resp. -7 q_j, a negative
    multiple of the deciding prime) agrees with the value mod q_0 .. q_{j-1} and differs mod q_j: the comparison at
    prime j, and nothing before it, decides."""
    n, npr, q = o.n, o.np, o.q
    assert npr >= 3
    Qp = chain_products(o)
    Q = Qp[npr]
    plants = [("H", H, 2), ("-H-1", -H - 1, 2), ("2^64+5", 2 ** 64 + 5, 2), ("-(2^64+5)", -(2 ** 64 + 5), 2),
              ("(Q-1)/2", (Q - 1) // 2, None), ("-(Q-1)/2", -(Q - 1) // 2, None)]
    for j in range(3, npr):
        plants += [(f"12345+Q'_{j}", 12345 + Qp[j], j), (f"-7q_{j}-Q'_{j}", -7 * q[j] - Qp[j], j)]
    base = background(o, 2000 * n + npr)
    assert all(fits_int64(v) for v in base)                             # the plant alone decides
    pos = plant_positions(n)
    out = []
    for i, (name, v, j) in enumerate(plants):
        assert -Q // 2 < v <= Q // 2 and not fits_int64(v), name
        d = decider(o, v)
        assert d is not None and d >= 2 and (j is None or d == j), (name, d)
        if d >= 3:
            cand = centre(v, Qp[d])                                     # what the kernel holds when it reaches prime d
            assert fits_int64(cand), name
            assert all(cand % q[i] == v % q[i] for i in range(d)), name
            assert cand % q[d] != v % q[d], name                        # prime d decides
            if j is not None:
                assert cand == (12345 if v > 0 else -7 * q[j]), name
        vec = list(base)
        vec[pos[i % len(pos)]] = v
        out.append(dict(name=name, vec=vec, pos=pos[i % len(pos)], value=v, prime=d))
    return out


def expect_at_level(o, vec, p):
    """(status, [ints]): the centred representative of every coefficient mod Q'_p; status 1 iff all lie in [-H, H).
    The header's definition of the level decrypt and nothing else."""
    Qp = chain_products(o)[p]
    r = np.array(vec, dtype=object) % Qp
    y = [int(v) - Qp if int(v) > Qp // 2 else int(v) for v in r]
    return (1 if all(fits_int64(v) for v in y) else 0), y


def residues(o, vec):
    """vec mod q_j for every prime -> uint32 [np][n], from Python integers."""
    a = np.array(vec, dtype=object)
    return np.stack([(a % q).astype(np.uint32) for q in o.q])


def random_row(o, rng, j):
    """Random canonical residues mod q_j with 0, 1 and q_j - 1 at three positions."""
    n, q = o.n, o.q[j]
    c = rng.integers(0, q, n, dtype=np.uint32)
    c[[2, n // 2 + 1, n - 2]] = [0, 1, q - 1]
    return c


def ciphertext_of(o, vec, s_hat, rng, degree=1):
    """Rows that decrypt to `vec` under the key s_hat (its NTT form per prime, from the oracle) -> (c0, c1) or, for
    degree 2, (c0, c1, c2), each uint32 [np][n].  c1 (and c2) are random_row;
    c0_j = NTT_j(vec mod q_j) - c1_j . s_hat_j (- c2_j . s_hat_j^2) mod q_j in uint64 (a product of residues is below 2^60,
    reduced before the next step)."""
    assert degree in (1, 2)
    res = residues(o, vec)
    rows = [[] for _ in range(degree + 1)]
    for j in range(o.np):
        q = np.uint64(o.q[j])
        s = s_hat[j].astype(np.uint64)
        c1 = random_row(o, rng, j)
        sub = (c1.astype(np.uint64) * s) % q
        if degree == 2:
            c2 = random_row(o, rng, j)
            sub = (sub + (((c2.astype(np.uint64) * s) % q) * s) % q) % q
            rows[2].append(c2)
        rows[0].append(((o.ntt(res[j], j).astype(np.uint64) + q - sub) % q).astype(np.uint32))
        rows[1].append(c1)
    return tuple(np.stack(r) for r in rows)


def oracle_route(o, rows, s_hat):
    """What the oracle and Python integers make of a record: o.decrypt and o.intt per prime, then crt_centred -> n ints.
    rows (c0, c1): d = c0 + c1 . s.  rows (c0, c1, c2): the same step twice, d = c0 + (c1 + c2 . s) . s."""
    pts = []
    for j in range(o.np):
        d = rows[-1][j]
        for c in rows[-2::-1]:
            d = o.decrypt(c[j], d, s_hat[j], j)
        pts.append(o.intt(d, j))
    return crt_centred(o.q, pts)
