"""The host model of the ciphertext operations (tests/ct_model.py) checked on the CPU, on shapes the oracle handles
quickly: 1024 x 1 and 4096 x 2, the smallest shape with a special prime.  The GPU modules hold the kernels to this model;
these tests hold the model's own pieces to one another and run the constructed inputs' assertions before a GPU is
involved."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vectors as V
from ct_model import (DIGIT_MASK, brev, call_elements, digits_of, edge_row, hoist_expect, inverse_element, rand_slab,
                      random_keys, sigma_rows, src_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1024, 1), (4096, 2)]


@pytest.fixture(scope="module")
def oracles():
    from oracle import pyoracle
    pyoracle.build(ref=False)
    return {shape: pyoracle.Oracle(*shape) for shape in SHAPES}


def test_model_imports_neither_torch_nor_pytest():
    """The CPU suite and the tools import the model: it must pull in neither torch, pytest, ctypes' users nor the package."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import ct_model; "
            "assert not {'torch', 'pytest', 'seal_embedded_amd'} & set(sys.modules)" % (os.path.join(ROOT, "tests"), ROOT))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_src_table_is_the_automorphism_on_ntt_rows(oracles, shape):
    """For g in {3, 3^-1, n + 1, 2n - 1}: gathering an NTT-form row by src_table(n, g) is sigma_g through the coefficient
    domain (sigma_rows), on random rows of every prime; and the table is the one vectors.galois_image gives: slot k holds
    the evaluation at psi^e, e = 2 brev(k) + 1, sigma_g moves it to the slot of e g mod 2n, which for e = r + n [e >= n]
    is image[r] + n (neg[r] xor [e >= n])."""
    o = oracles[shape]
    n, npr = shape
    bits = n.bit_length() - 1
    rng = np.random.default_rng(n + npr)
    rows = rand_slab(rng, o.q, 1, n)[0]
    k = np.arange(n, dtype=np.int64)
    e = 2 * brev(k, bits) + 1
    for g in (3, inverse_element(n, 3), n + 1, 2 * n - 1):
        src = src_table(n, g)
        assert sorted(src.tolist()) == list(range(n)), g
        rotated = sigma_rows(o, rows, g)
        for j in range(npr):
            assert (rows[j][src] == rotated[j]).all(), (g, j)
        image, neg = V.galois_image(n, g)
        u = image[e % n] + n * (neg[e % n] ^ (e >= n))
        assert (u == (e * g) % (2 * n)).all() and (src == brev((u - 1) // 2, bits)).all(), g


def edge_row_uses(n):
    """(GPU module, element list, edge_row arguments) at the module's smallest case: what each module passes today."""
    digit6 = dict(edges="digit", starts=6)
    return [("test_gpu_ct_galois", [3, n + 1], dict(edges="digit", starts=3)),
            ("test_gpu_ct_galois_hoist", call_elements(n, 1), digit6),
            ("test_gpu_ct_lintrans", call_elements(n, 1), digit6),
            ("test_gpu_ct_bsgs accumulate", [3, 1, n + 1], dict(digit6, skip_identity=True)),
            ("test_gpu_ct_bsgs plan", [1, 3, 2 * n - 1], dict(digit6, skip_identity=True)),
            ("test_gpu_ct_keyswitch_sp", [3, n + 1], dict(edges="centring", starts=3)),
            ("test_gpu_ct_keyswitch_sp_hoist", [3, n + 1], dict(edges="centring", starts=3))]


def test_edge_row_parametrisations(oracles):
    """Every edge_row parametrisation a GPU module uses, built for that module's smallest case (1024 x 1; 4096 x 2 for the
    special prime) with its element list: the row's own coverage assertions hold, every edge value stands at every start
    position and 7 behind it, and the row is the NTT of those coefficients.  The variants stay apart: three starts refuse
    2n - 1 (nothing but index 0 is kept), and element 1 (nothing is negated) passes only where it is skipped."""
    uses = [((1024, 1), u) for u in edge_row_uses(1024) if u[2]["edges"] == "digit"] + \
        [((4096, 2), u) for u in edge_row_uses(4096) if u[2]["edges"] == "centring"]
    assert len(uses) == 7
    for shape, (module, elts, kw) in uses:
        sp = kw["edges"] == "centring"
        o, n = oracles[shape], shape[0]
        for j in range(o.np - 1 if sp else o.np):
            q = o.q[j]
            row = edge_row(o, j, np.random.default_rng(7 * n + j), elts, **kw)
            c = o.intt(row, j)
            values = [0, 1, (q - 1) // 2, (q + 1) // 2, q - 1] if sp else \
                [0, 1, DIGIT_MASK, DIGIT_MASK + 1, DIGIT_MASK + 2, q - 1]
            starts = (0, n // 2, n - 13) if kw["starts"] == 3 else (0, n // 9, n // 5, n // 3, n // 2, n - 13)
            for start in starts:
                assert c[start:start + len(values)].tolist() == values, (module, j, start)
                assert c[start + 7:start + 7 + len(values)].tolist() == values, (module, j, start)
            assert (c < q).all() and (o.ntt(c, j) == row).all(), (module, j)
    o = oracles[(1024, 1)]
    rng = np.random.default_rng(1)
    with pytest.raises(AssertionError):
        edge_row(o, 0, rng, [3, 2 * 1024 - 1], starts=3)
    edge_row(o, 0, rng, [3, 2 * 1024 - 1], starts=6)
    for starts in (3, 6):
        with pytest.raises(AssertionError):
            edge_row(o, 0, rng, [3, 1], starts=starts)
    edge_row(o, 0, rng, [3, 1], starts=6, skip_identity=True)


def hoist_of_keyed_elements(table, o, c0, c1, elts, key_of, gk0, gk1):
    """The many form as the hoist and linear-transform tests stated it before the model held it, with no case for
    element 1: kept here, literally, as the second opinion on hoist_expect."""
    B, L, n = c0.shape
    srcs = [table(n, g).astype(np.int64) for g in elts]
    out0 = np.zeros((len(elts), B, L, n), dtype=np.uint32)
    out1 = np.zeros_like(out0)
    for b in range(B):
        D = digits_of(o, c1[b], L)
        for i in range(L):
            q = np.uint64(o.q[i])
            F = [o.ntt(dig, i).astype(np.uint64) for dig in D]
            for e, (g, src) in enumerate(zip(elts, srcs)):
                k0, k1 = gk0[key_of[g]], gk1[key_of[g]]
                acc0, acc1 = c0[b, i][src].astype(np.uint64), np.zeros(n, dtype=np.uint64)
                for r, f in enumerate(F):
                    acc0 = (acc0 + (f[src] * k0[r, i].astype(np.uint64)) % q) % q
                    acc1 = (acc1 + (f[src] * k1[r, i].astype(np.uint64)) % q) % q
                out0[e, b, i], out1[e, b, i] = acc0, acc1
    return out0, out1


def test_hoist_expect_with_and_without_the_identity(oracles):
    """1024 x 1, B = 1, L = 1: for element 1 hoist_expect returns the record itself and asks for no key; for a single keyed
    element it equals the transcription above, also when 1 stands beside it in the list."""
    n, npr = 1024, 1
    o = oracles[(n, npr)]
    rng = np.random.default_rng(1024 + 23)
    gk0, gk1 = random_keys(rng, o.q, 1, n, npr)
    c0, c1 = rand_slab(rng, o.q, 1, n), rand_slab(rng, o.q, 1, n)
    c1[0, 0] = edge_row(o, 0, rng, [3], starts=6)
    i0, i1 = hoist_expect(src_table, o, c0, c1, [1], {}, gk0, gk1)
    assert i0.shape == (1, 1, 1, n) and (i0[0] == c0).all() and (i1[0] == c1).all()
    want = hoist_of_keyed_elements(src_table, o, c0, c1, [3], {3: 0}, gk0, gk1)
    got = hoist_expect(src_table, o, c0, c1, [3], {3: 0}, gk0, gk1)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    assert (got[0] != c0).any() and (got[1] != c1).any()
    both = hoist_expect(src_table, o, c0, c1, [1, 3, 1], {3: 0}, gk0, gk1)
    for h, rec in ((0, c0), (1, c1)):
        assert (both[h][0] == rec).all() and (both[h][2] == rec).all() and (both[h][1] == want[h][0]).all()
