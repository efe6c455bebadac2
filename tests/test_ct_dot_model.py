"""The host model of the grouped product sums (tests/ct_model_dot.py) checked on the CPU at 4096 x 3, L = 2: the sums
against Python integers and the tensor formulas, and the inner product of 8 + 8 real records through the model, a model
rescale and the oracle's decode against the reference's 0.1.  The GPU module holds the kernels to this model."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vectors as V
from ct_model import crt_centred, rand_key, rand_slab, relin_sp_expect, rescale_expect, sp_key
from ct_model_dot import dot_sp_expect, eager_dot_expect, mul_sum_expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NP, L = 4096, 3, 2


@pytest.fixture(scope="module")
def o():
    from oracle import pyoracle
    pyoracle.build(ref=False)
    return pyoracle.Oracle(N, NP)


@pytest.fixture(scope="module")
def slabs(o):
    """Two sides of 3 random records at level 2 (computed once, left unchanged)."""
    rng = np.random.default_rng(4096 * 3 + 23)
    return tuple(rand_slab(rng, o.q, 3, N, L) for _ in range(4))


def test_model_imports_neither_torch_nor_pytest():
    code = ("import sys; sys.path[:0] = [%r, %r]; import ct_model_dot; "
            "assert not {'torch', 'pytest', 'seal_embedded_amd'} & set(sys.modules)" % (os.path.join(ROOT, "tests"), ROOT))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_a_row_of_three_pairs_is_the_sum_in_python_integers(o, slabs):
    a0, a1, b0, b1 = slabs
    row = [(0, 2), (1, 1), (0, 2)]                                   # a pair listed twice counts twice
    T = mul_sum_expect(o, a0, a1, b0, b1, [row, []])
    assert not any(t[1].any() for t in T)                            # an empty row is zero
    for j in range(L):
        q = o.q[j]
        for k in list(range(5)) + [N - 1]:
            x0, x1, y0, y1 = ([int(s[r, j, k]) for r in range(3)] for s in slabs)
            assert int(T[0][0, j, k]) == sum(x0[a] * y0[b] for a, b in row) % q
            assert int(T[1][0, j, k]) == sum(x0[a] * y1[b] + x1[a] * y0[b] for a, b in row) % q
            assert int(T[2][0, j, k]) == sum(x1[a] * y1[b] for a, b in row) % q


def test_a_row_of_one_pair_is_the_tensor_and_its_relinearisation(o, slabs):
    a0, a1, b0, b1 = slabs
    qv = np.array(o.q[:L], dtype=np.uint64)[:, None]
    x0, x1, y0, y1 = (s.astype(np.uint64) for s in (a0[2], a1[2], b0[0], b1[0]))
    T = mul_sum_expect(o, a0, a1, b0, b1, [[(2, 0)]])
    assert (T[0][0] == (x0 * y0) % qv).all() and (T[2][0] == (x1 * y1) % qv).all()
    assert (T[1][0] == ((x0 * y1) % qv + (x1 * y0) % qv) % qv).all()
    rng = np.random.default_rng(5)
    k0, k1 = rand_key(rng, o.q, N), rand_key(rng, o.q, N)
    d0, d1, _ = dot_sp_expect(o, a0, a1, b0, b1, [[(2, 0)]], k0, k1)
    e0, e1 = relin_sp_expect(o, T[0], T[1], T[2], k0, k1)
    assert (d0 == e0).all() and (d1 == e1).all()


def test_inner_product_of_real_records_decodes_within_the_references_bound(o):
    """8 + 8 fresh records with slots uniform in [-1, 1], dropped to L = 2: one row of 8 pairs through dot_sp_expect, the
    model rescale and the oracle's decode at Delta^2 / q_1 is within the reference's 0.1 of the float64 inner product,
    and the largest coefficient before the rescale is below Q_2 / 2.  As run: worst slot error 2.9e-03 (eager path:
    3.8e-03), largest coefficient 2^45.8; all printed, only the bounds asserted."""
    from oracle.pyoracle import Oracle
    m = 8
    lo, l1 = Oracle(N, L), Oracle(N, L - 1)
    sk = V.secret_key(N, seed=5)
    s_hat = np.stack([o.ntt(o.expand_ternary(sk, j), j) for j in range(NP)])
    sq = np.stack([((s_hat[j].astype(np.uint64) ** 2) % np.uint64(o.q[j])).astype(np.uint32) for j in range(NP - 1)])
    k0, k1 = sp_key(o, sk, sq, "dot-model")
    vals = np.random.default_rng(77).uniform(-1.0, 1.0, (2 * m, N // 2)).astype(np.float32)
    ss, sd = V.bench_seeds(2 * m, first=500)
    recs = [o.encrypt_sym(vals[b], ss[b].tobytes(), sd[b].tobytes(), sk) for b in range(2 * m)]
    side = lambda lo_, hi_, c: np.stack([np.stack([np.array(r[c][j]) for j in range(L)]) for r in recs[lo_:hi_]])  # noqa: E731
    a0, a1, b0, b1 = side(0, m, "c0"), side(0, m, "c1"), side(m, 2 * m, "c0"), side(m, 2 * m, "c1")
    row = [(k, k) for k in range(m)]
    want = (vals[:m].astype(np.float64) * vals[m:].astype(np.float64)).sum(axis=0)
    scale = o.scale * o.scale / o.q[L - 1]
    Q2 = o.q[0] * o.q[1]

    def decode(c0, c1, orc, primes, sc):
        pts = [orc.intt(orc.decrypt(c0[j], c1[j], s_hat[j], j), j) for j in range(primes)]
        y = crt_centred(orc.q, pts)
        res = orc.fft((np.array(y, dtype=np.float64) / sc).astype(np.complex128))
        return np.ascontiguousarray(res.real[orc.map[:N // 2].astype(np.int64)]), max(abs(v) for v in y)

    for name, (r0, r1) in (("one call", dot_sp_expect(o, a0, a1, b0, b1, [row], k0, k1)[:2]),
                           ("eager", eager_dot_expect(o, a0, a1, b0, b1, [row], k0, k1))):
        _, big = decode(r0[0], r1[0], lo, L, 1.0)
        f0, f1 = rescale_expect(o, r0), rescale_expect(o, r1)
        got, _ = decode(f0[0], f1[0], l1, L - 1, scale)
        err = float(np.abs(got - want).max())
        print(f"{name}: worst slot error {err:.3e}, log2 of the largest coefficient before the rescale "
              f"{np.log2(float(big)):.2f} (Q_2 / 2: {np.log2(Q2 / 2):.2f})")
        assert big < Q2 // 2 and err < 0.1, (name, big, err)
