"""The host model of the special-prime baby-step / giant-step transform (tests/ct_model_bsgs_sp.py) held to the model of
the entries that already exist (tests/ct_model.py), on the CPU: 4096 x 2 and 4096 x 3 with L = 1, 2, random slabs and keys.
The GPU module holds the kernels to this model; these tests hold its pieces to one another."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ct_model import centred, galois_sp_expect, hoist_sp_expect, rand_slab, src_table
from ct_model_bsgs_sp import (accum_sp_expect, bsgs_sp_expect, many_ext_expect, mod_down_expect, sp_keys)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [((4096, 2), 1), ((4096, 3), 1), ((4096, 3), 2)]          # (shape, L)
IDS = [f"{s[0]}x{s[1]}-L{L}" for s, L in CASES]
B = 2


@pytest.fixture(scope="module")
def oracles():
    from oracle import pyoracle
    pyoracle.build(ref=False)
    return {shape: pyoracle.Oracle(*shape) for shape in {c[0] for c in CASES}}


def setup(oracles, shape, L, elts, seed):
    o = oracles[shape]
    n, npr = shape
    rng = np.random.default_rng(seed + 7 * n + npr + L)
    return o, rng, rand_slab(rng, o.q, B, n, L), rand_slab(rng, o.q, B, n, L), sp_keys(rng, o.q, elts, n)


def test_model_imports_neither_torch_nor_pytest():
    code = ("import sys; sys.path[:0] = [%r, %r]; import ct_model_bsgs_sp; "
            "assert not {'torch', 'pytest', 'seal_embedded_amd'} & set(sys.modules)" % (os.path.join(ROOT, "tests"), ROOT))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


@pytest.mark.parametrize("shape,L", CASES, ids=IDS)
def test_mod_down_of_one_undivided_rotation_is_the_single_rotation(oracles, shape, L):
    """mod_down(many_ext([g])) == galois_sp_expect(g) for g = 3 and 2n - 1: P . sigma(c0) divides exactly and centring
    commutes with sigma.  Element 1 comes back as the record itself."""
    n = shape[0]
    elts = [3, 2 * n - 1, 1]
    o, _, c0, c1, keys = setup(oracles, shape, L, elts, 11)
    u0, u1 = many_ext_expect(src_table, o, c0, c1, elts, keys)
    assert u0.shape == (3, B, L + 1, n)
    w0, w1 = mod_down_expect(o, u0), mod_down_expect(o, u1)
    for e, g in enumerate(elts[:2]):
        e0, e1 = galois_sp_expect(o, c0, c1, g, *keys[g])
        assert (w0[e] == e0).all() and (w1[e] == e1).all(), g
    assert (w0[2] == c0).all() and (w1[2] == c1).all()
    assert not u0[2, :, L].any() and not u1[2, :, L].any()


@pytest.mark.parametrize("shape,L", CASES, ids=IDS)
def test_accum_sp_of_one_element_is_the_single_rotation(oracles, shape, L):
    n = shape[0]
    o, _, c0, c1, keys = setup(oracles, shape, L, [n + 1], 13)
    a0, a1 = accum_sp_expect(o, c0[None], c1[None], [n + 1], keys)
    e0, e1 = galois_sp_expect(o, c0, c1, n + 1, *keys[n + 1])
    assert (a0 == e0).all() and (a1 == e1).all()
    i0, i1 = accum_sp_expect(o, c0[None], c1[None], [1], keys)
    assert (i0 == c0).all() and (i1 == c1).all()


@pytest.mark.parametrize("shape,L", CASES, ids=IDS)
def test_bsgs_sp_with_the_identity_giant_step_is_the_flat_transform(oracles, shape, L):
    """giant = [1]: V = sum_b d_b . U[b], one division, nothing added: hoist_sp_expect with the same weights -- the
    record's own weight w0 where baby holds element 1."""
    n, npr = shape
    baby = [1, 3, n + 1]
    o, rng, c0, c1, keys = setup(oracles, shape, L, baby, 17)
    diag = rng.integers(0, 2 ** 32, (1, len(baby), npr, n), dtype=np.uint32)
    g0, g1 = bsgs_sp_expect(src_table, o, c0, c1, baby, [1], diag, keys)
    e0, e1, _ = hoist_sp_expect(o, c0, c1, baby[1:], [keys[g] for g in baby[1:]], diag[0, 1:], diag[0, 0])
    assert (g0 == e0).all() and (g1 == e1).all()
    h0, h1 = bsgs_sp_expect(src_table, o, c0, c1, baby[1:], [1], diag[:, 1:], keys)
    f0, f1, _ = hoist_sp_expect(o, c0, c1, baby[1:], [keys[g] for g in baby[1:]], diag[0, 1:], None)
    assert (h0 == f0).all() and (h1 == f1).all()


@pytest.mark.parametrize("shape,L", CASES, ids=IDS)
def test_mod_down_is_the_rounded_division_in_python_integers(oracles, shape, L):
    """On one row per data prime: for coefficients v = P x + e with |e| < P / 2 chosen at 0, +-1 and +-(P - 1)/2 beside
    random ones, mod_down of the extended record of v (rows v mod q_i in NTT form, row L v mod P) is x + round(e / P) = x
    -- in Python integers, no word size anywhere."""
    o = oracles[shape]
    n, npr = shape
    p = npr - 1
    P = int(o.q[p])
    rng = np.random.default_rng(19 + L)
    x = [int(v) for v in rng.integers(-2 ** 40, 2 ** 40, n)]
    e = [int(v) for v in rng.integers(-(P // 2) + 1, P // 2, n)]
    e[:5] = [0, 1, -1, (P - 1) // 2, -(P - 1) // 2]
    e[n - 5:] = [-(P - 1) // 2, (P - 1) // 2, -1, 1, 0]
    v = [P * a + b for a, b in zip(x, e)]
    assert all(abs(b) < P / 2 and round(b / P) == 0 for b in e)
    rows = [o.ntt(np.array([c % int(o.q[i]) for c in v], dtype=np.uint32), i) for i in list(range(L)) + [p]]
    got = mod_down_expect(o, np.stack(rows)[None])[0]
    assert (centred(o.intt(rows[L], p), P) == np.array(e)).all()
    for i in range(L):
        want = o.ntt(np.array([a % int(o.q[i]) for a in x], dtype=np.uint32), i)
        assert (got[i] == want).all(), i
